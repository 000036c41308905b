"""CPU: the restatement of the device dropout (tests/dropout_ref.py) held to what it must be before tests/test_gpu_dropout.py
trusts it, and the host side of the three new entry points.

  * masks of another `call` or `site` are independent of each other (about half their elements agree at p = 0.5);
  * the kept share is within 4 sigma of 1 - p (sigma = sqrt(p (1 - p) / n) of n independent draws);
  * the fp64 block with an all-kept mask and scale 1 IS the existing teacher of tests/stgcn_block_ref.py;
  * the fp32 twin of every dropout teacher is inside the bars (they bite no correct fp32 evaluation);
  * the library exports the three symbols, each refuses null arguments under its own name, and rows of more than 2^22
    elements, sites >= 4096 and p outside (0, 1) are refused on the host, before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dropout_ref as D
import stgcn_block_ref as R

STATES = [(1234, 0, 0), (1234, 1, 0), (1234, 0, 3), (2 ** 40 + 7, 2 ** 33, 9)]
SHAPES = [(128, 260, .5), (256, 500, .5), (256, 175, .25), (128, 20, .9), (3, 256, .5)]
SYMBOLS = ('tamgcn_drop_add_act_fwd', 'tamgcn_drop_add_act_bwd', 'tamgcn_dropout_advance')


def test_masks_of_other_calls_and_sites_are_independent():
    rows, L = 128, 260
    base = D.mask(1234, 0, 0, rows, L, .5)
    n = rows * L
    for seed, call, site in [(1234, 1, 0), (1234, 0, 1), (1235, 0, 0), (1234, 2 ** 32, 0)]:
        other = D.mask(seed, call, site, rows, L, .5)
        agree = float((base == other).mean())
        assert abs(agree - 0.5) <= 4 * math.sqrt(0.25 / n), (seed, call, site, agree)
    assert np.array_equal(base, D.mask(1234, 0, 0, rows, L, .5))
    assert np.array_equal(base[:, :100], D.mask(1234, 0, 0, rows, 100, .5))      # position i depends on (r, i) alone


@pytest.mark.parametrize('rows,L,p', SHAPES)
def test_kept_share_within_four_sigma(rows, L, p):
    worst = 0.0
    for seed, call, site in STATES:
        m = D.mask(seed, call, site, rows, L, p)
        assert m.shape == (rows, L) and m.dtype == bool
        sigma = math.sqrt(p * (1 - p) / m.size)
        dev = abs(float(m.mean()) - (1 - p)) / sigma
        worst = max(worst, dev)
        assert dev <= 4.0, (seed, call, site, rows, L, p, dev)
    print(f'rows {rows} L {L} p {p}: largest deviation {worst:.2f} sigma')


def test_consts():
    assert D.consts(.5) == (2 ** 31, np.float32(2.0))
    assert D.consts(.25)[0] == 2 ** 30 and D.consts(.9)[1] == np.float32(1.0 / (1.0 - 0.9))
    from tam_gcn_amd import ops
    for p in (.5, .25, .9, 1e-3, 1 - 1e-7):
        thr, scale = ops.dropout_consts(p)
        assert (thr, np.float32(scale)) == D.consts(p) and float(np.float32(scale)) == scale


@pytest.mark.parametrize('tag', ['k9 64->64 s1', 'k5 64->128 s2', 'k3 3->64 nores'], ids=R.iso_id)
def test_all_kept_block_is_the_existing_teacher(tag):
    keep = torch.ones(D.out_shape(tag), dtype=torch.bool)
    _, t = D.block_teacher(tag, keep, 1.0)
    ref = R.teacher('isolated', tag, True)
    assert t.tries == ref.tries and torch.equal(t.x, ref.x)
    tq, rq = R.quantities(t), R.quantities(ref)
    assert tq.keys() == rq.keys()
    for q in tq:
        assert torch.equal(tq[q], rq[q]) or float((tq[q] - rq[q]).abs().max()) <= 1e-13 * float(rq[q].abs().max()), q


@pytest.mark.parametrize('tag', list(D.BLOCK_CASES), ids=R.iso_id)
def test_fp32_twin_of_the_dropout_teacher_is_inside_every_bar(tag):
    _, t = D.block_teacher(tag)
    kept = float(D.mask_nctv(D.DROP_SEED, D.DROP_CALL, D.DROP_SITE, D.out_shape(tag), D.DROP_P).float().mean())
    assert 0.4 < kept < 0.6
    assert float((t.y == 0).float().mean()) > 0.2          # the mask is in the teacher: dropped + negative elements
    for mode in (1, 0):
        ratios = R.verify(R._REF32[t.key][1:6], t, mode)
        print(R.line(f'dropout {R.iso_id(tag)} mode {mode} nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))


# ---------------------------------------------------------------------------------------------------------------------
# the library's host side
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from tam_gcn_amd import build, _lib
    build.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.tamgcn_last_error.restype = C.c_char_p
    for name in SYMBOLS:
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = _lib.SIGNATURES[name][1]
    return lib


def test_library_exports_the_symbols_and_they_refuse_null_arguments():
    lib = _lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    calls = {
        'tamgcn_drop_add_act_fwd': (None, None, 1, 0, 0, 0, 0, None, 0, 0, 0.0, None, None, None),
        'tamgcn_drop_add_act_bwd': (None, None, 1, 0.0, None, None, None, None, 0, 0, 0, 0, None, None, None, None),
        'tamgcn_dropout_advance': (None, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) < 0, name
        assert name.encode() in lib.tamgcn_last_error(), (name, lib.tamgcn_last_error())


def test_host_refuses_long_rows_large_sites_and_bad_p():
    from tam_gcn_amd import _lib as L, ops
    lib = _lib()
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    src = L.Src(ptr, None, None, 1, 0, 0)
    thr, scale = ops.dropout_consts(.5)

    def fwd(T, V, site, sc=scale):
        return lib.tamgcn_drop_add_act_fwd(C.byref(src), None, 1, 1, 1, T, V, ptr, site, thr, sc, ptr, ptr, None)

    assert fwd(2 ** 20, 4 + 1, 0) < 0 and b'tamgcn_drop_add_act_fwd: rows of more than 2^22' in lib.tamgcn_last_error()
    assert fwd(2 ** 22 + 1, 1, 0) < 0 and b'2^22' in lib.tamgcn_last_error()
    assert fwd(4, 4, 4096) < 0 and b'tamgcn_drop_add_act_fwd: site 4096' in lib.tamgcn_last_error()
    assert fwd(4, 4, -1) < 0 and b'site -1' in lib.tamgcn_last_error()
    for bad in (0.5, 0.0, float('inf'), float('nan')):       # no 1 / (1 - p) of a p in (0, 1)
        assert fwd(4, 4, 0, bad) < 0 and b'tamgcn_drop_add_act_fwd: scale' in lib.tamgcn_last_error(), bad
    rc = lib.tamgcn_drop_add_act_bwd(ptr, ptr, 1, scale, None, None, None, None, 1, 1, 2 ** 22 + 1, 1, ptr, None, None, None)
    assert rc < 0 and b'tamgcn_drop_add_act_bwd: rows of more than 2^22' in lib.tamgcn_last_error()
    # the Python layer refuses the same, and p, before it touches a tensor
    for p in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='0 < p < 1'):
            ops.dropout_consts(p)
    with pytest.raises(ValueError, match='2\\^22'):
        ops._drop_check(2 ** 20, 5, 0)
    with pytest.raises(ValueError, match='site'):
        ops._drop_check(4, 4, 4096)
    ops._drop_check(2 ** 20, 4, 4095)
