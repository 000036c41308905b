"""CPU: the draw stream of the device feeder as tests/feeder_draws.py restates it -- Philox known answers, structure,
distribution (a fixed seed: deterministic outcomes, not a statistical gamble), the "100 copies of every frame" semantics
of the reference's `random.sample(list(np.arange(length)) * 100, 52)` (feeder_nucla_gcn.py:112), numpy's linspace on the
val path -- and the parts of the feature that need no GPU: the two ABI entry points' argument checks and the Feeder's
public surface."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

import feeder_draws as FD

SEED, CALL, SLOTS, TS = 20240229, 3, 65536, 52
LENGTHS = (1, 7, 40, 201)


def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    for counter, key, want in [
            ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]:
        got = tuple(int(w) for w in FD.philox4x32_10(counter, key))
        assert got == want, [hex(g) for g in got]


@pytest.fixture(scope='module', params=LENGTHS)
def drawn(request):
    L = request.param
    return (L,) + FD.draws(SEED, CALL, np.full(SLOTS, L), TS)


def test_structure(drawn):
    L, agx, agy, s, idx, pos = drawn
    for a in (agx, agy):
        assert a.dtype == np.int64 and a.min() == -60 and a.max() == 60
    assert s.dtype == np.float64 and 0.5 <= s.min() and s.max() <= 1.5
    srt = np.sort(pos, axis=1)
    assert (np.diff(srt, axis=1) > 0).all(), 'positions of a slot repeat'
    assert pos.min() >= 0 and pos.max() < 100 * L
    assert idx.shape == (SLOTS, TS) and (np.diff(idx, axis=1) >= 0).all() and idx.min() >= 0 and idx.max() < L


def _pearson(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def test_distribution(drawn):
    from scipy.stats import chi2
    L, agx, agy, s, idx, pos = drawn
    stat = _pearson(np.bincount(idx.ravel(), minlength=L), SLOTS * TS / L)
    if L == 1:                                           # no degree of freedom: the one frame holds every count
        assert stat == 0.0
    else:
        bound = chi2.isf(1e-6, L - 1)
        print(f'L = {L}: frames chi2 {stat:.1f}, bound {bound:.1f}')
        assert stat < bound, f'L = {L}: frames chi2 {stat:.1f} >= {bound:.1f}'
    for name, a in (('agx', agx), ('agy', agy)):
        stat = _pearson(np.bincount(a + 60, minlength=121), SLOTS / 121)
        bound = chi2.isf(1e-6, 120)
        assert stat < bound, f'L = {L}: {name} chi2 {stat:.1f} >= {bound:.1f}'


def test_hundred_copies_of_every_frame():
    """Sampling 52 of the 100 L positions WITHOUT replacement: the expected number of distinct frames per slot is
    L (1 - prod_{i < 52} (n - 100 - i) / (n - i)), n = 100 L (29.3690 at L = 40; with replacement it would be 29.2774)."""
    L = 40
    n = 100 * L
    idx = FD.draws(SEED, CALL, np.full(SLOTS, L), TS)[3]
    distinct = 1 + (np.diff(idx, axis=1) != 0).sum(axis=1)
    exact = L * (1 - math.exp(sum(math.log((n - 100 - i) / (n - i)) for i in range(TS))))
    assert abs(exact - 29.3690) < 1e-4
    six_se = 6 * distinct.std(ddof=1) / math.sqrt(SLOTS)
    assert abs(distinct.mean() - exact) <= six_se, (distinct.mean(), exact, six_se)


def test_val_indices_equal_numpy_linspace():
    for L in range(1, 4097):
        assert np.array_equal(FD.val_indices(L, TS), np.linspace(0, L - 1, TS).astype(int)), L


def test_slots_are_independent_of_the_batch():
    """Slot b's draws depend on (seed, call, b, its clip's length) only."""
    a = FD.draws(7, 2, [40, 13, 99, 5])
    b = FD.draws(7, 2, [40, 200, 99])
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])
    assert not np.array_equal(FD.draws(7, 3, [40])[3], a[3][:1])
    assert not np.array_equal(FD.draws(8, 2, [40])[3], a[3][:1])
    assert not np.array_equal(FD.draws(7 + 2 ** 32, 2, [40])[3], a[3][:1])           # the seed's high word is used
    assert not np.array_equal(FD.draws(7, 2 + 2 ** 32, [40])[3], a[3][:1])           # and the call's


def test_abi_draw_entry_points_reject_bad_arguments_without_a_gpu():
    from tam_gcn_amd import build, _lib
    build.build()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.tamgcn_last_error.restype = C.c_char_p
    for name in ('tamgcn_feeder_draw', 'tamgcn_feeder_transform_indexed'):
        assert hasattr(lib, name), f'{name} not exported'
        assert name in _lib.SIGNATURES
    draw, tri = lib.tamgcn_feeder_draw, lib.tamgcn_feeder_transform_indexed
    draw.argtypes, tri.argtypes = _lib.SIGNATURES['tamgcn_feeder_draw'][1], _lib.SIGNATURES['tamgcn_feeder_transform_indexed'][1]
    assert draw(None, 4, None, 4, None, None, None, 52, 1, None, None, None, None, None) < 0
    assert b'tamgcn_feeder_draw' in lib.tamgcn_last_error() and b'null' in lib.tamgcn_last_error()
    assert tri(None, None, 4, None, None, None, None, 4, 20, 52, 1, 0, None, None) < 0
    assert b'tamgcn_feeder_transform_indexed' in lib.tamgcn_last_error() and b'null' in lib.tamgcn_last_error()
    # pointers that are never dereferenced: the dimension checks come before any HIP call
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert draw(p, 4, p, 0, None, p, p, 52, 1, p, p, p, None, None) < 0
    assert b'tamgcn_feeder_draw: bad dims' in lib.tamgcn_last_error()
    assert draw(p, 4, p, 4, None, p, p, 65, 1, p, p, p, None, None) < 0 and b'time_steps' in lib.tamgcn_last_error()
    assert draw(p, 4, p, 4, None, p, None, 52, 1, p, p, p, None, None) < 0 and b'cos/sin' in lib.tamgcn_last_error()
    assert draw(p, 4, p, 4, p, p, p, 52, 1, p, p, p, None, None) < 0 and b'labels' in lib.tamgcn_last_error()
    assert tri(p, p, 4, p, p, p, p, 0, 20, 52, 1, 0, p, None) < 0
    assert b'tamgcn_feeder_transform_indexed: bad dims' in lib.tamgcn_last_error()
    assert tri(p, p, 4, p, p, p, p, 4, 20, 52, 20, 0, p, None) < 0 and b'centre joint' in lib.tamgcn_last_error()
    assert tri(p, p, 4, p, p, p, p, 4, 20, 52, 1, 4, p, None) < 0 and b'mode 4' in lib.tamgcn_last_error()


def test_feeder_public_surface():
    from tam_gcn_amd import ops
    from tam_gcn_amd.feeder import feeder_nucla_gcn as F
    params = list(inspect.signature(F.Feeder.__init__).parameters.values())
    assert params[-1].name == 'seed' and params[-1].default == 0
    assert [p.name for p in params[-3:]] == ['device', 'stream', 'seed']
    for name in ('batch_device', 'manual_seed', 'rng_state', 'set_rng_state', 'batch', '_draw'):
        assert callable(getattr(F.Feeder, name)), name
    assert inspect.isclass(F.GraphedBatch)
    assert callable(ops.feeder_draw) and callable(ops.feeder_transform_indexed)


def test_load_data_refuses_clips_the_device_draw_cannot_index(tmp_path):
    """The clip lengths live on the device, so the bound of the draw (1 <= L, 100 L < 2^24) is checked where the split is
    loaded: before anything goes to a device."""
    import json
    import os
    from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder
    os.makedirs(tmp_path / 'a01_s01_e00_v01')
    with open(tmp_path / 'a01_s01_e00_v01' / 'a01_s01_e00_v01.json', 'w') as f:
        json.dump({'skeletons': []}, f)
    with pytest.raises(ValueError, match='0 frames'):
        Feeder(str(tmp_path), 'train', data_dict=[{'file_name': 'a01_s01_e00_v01', 'label': 1}], device='cpu')
    with pytest.raises(ValueError, match='seed'):
        Feeder(str(tmp_path), 'train', data_dict=[], device='cpu', seed=-1)
