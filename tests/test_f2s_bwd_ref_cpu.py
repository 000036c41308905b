"""CPU: the reference of the f2s backward stage tests (tests/f2s_bwd_ref.py) is itself pinned -- its two stages reproduce
torch.autograd through f2s_ref.block_eval in fp64, an fp32 evaluation passes every bar of tests/test_gpu_f2s_bwd_stages.py, each of
a list of real defects fails them, the engine's transposed fold equals an independent one, the body-part bookkeeping is checked
on hand-made cases, and the fp64 oracle's autograd gradient equals the fixture written from the reference's model
(tests/golden/saliency.npz)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import f2s_bwd_ref as RB
import f2s_ref as R
import fp64_bars as B
from cases import STGCN_MODEL_CASES                                                 # noqa: E402
from params import fill_state_, make_input, make_labels                             # noqa: E402
from oracle import stgcn_oracle as SO                                               # noqa: E402
from tam_gcn_amd import _lib, f2s, saliency                                               # noqa: E402
from tam_gcn_amd.models import stgcn as M                                           # noqa: E402
from test_stgcn_oracle import fill_stgcn_                                           # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'saliency.npz'))

# Cin, Cout, stride, residual, K, V: every rmode x stride that exists (the identity residual needs stride 1), Cin != Cout
BLOCKS = [(3, 16, 1, False, 3, 20), (16, 16, 2, False, 1, 20), (16, 16, 1, True, 3, 17), (16, 32, 2, True, 3, 25), (16, 32, 1, True, 1, 18),
          (32, 16, 2, True, 2, 7), (8, 16, 1, True, 3, 5)]


@pytest.mark.parametrize('T', (1, 3, 8, 9))
@pytest.mark.parametrize('cin, cout, stride, residual, K, V', BLOCKS)
def test_stages_reproduce_autograd_in_fp64(cin, cout, stride, residual, K, V, T):
    blk = M.st_gcn(cin, cout, (9, K), stride, residual=residual)
    fill_state_(blk.state_dict(), seed=cin * 100 + cout + V)
    sd = {'m.' + k: (v.double() if v.is_floating_point() else v) for k, v in blk.state_dict().items()}
    Ae = make_input((K, V, V), seed=3, lo=0.0).double() * (1 + 0.3 * make_input((K, V, V), seed=4).double())
    p = R.fold_block(sd, 'm', Ae, blk._rmode)
    x = make_input((2, cin, T, V), seed=5).double().requires_grad_(True)
    out = R.block_eval(x, p, stride)
    gout = make_input(tuple(out.shape), seed=6).double()
    (ref,) = torch.autograd.grad(out, x, gout)
    got, kept = RB.block_bwd(x.detach(), p, stride, gout)
    assert torch.equal(kept['out'], out.detach())
    assert 0.05 < float((kept['out'] > 0).double().mean()) < 0.95 or T == 1      # both masks cut something
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    for defect in RB.DEFECTS:                                                      # where a defect applies it is visible
        bad, _ = RB.block_bwd(x.detach(), p, stride, gout, defect=defect)
        applies = {'stride_phase': stride == 2, 'res_dropped': p['rmode'] != 0, 'res_not_upsampled': p['rmode'] == 2 and stride == 2 and T > 1,
                   'taps_not_mirrored': T > 1, 'ae_not_transposed': True, 'mask_wrong_tensor': True, 'drop_last_frame': True}[defect]
        if applies:
            assert float((bad - ref).abs().max()) > 1e-6 * float(ref.abs().max()), defect


def test_engine_transposed_fold_equals_the_independent_fold():
    """tam_gcn_amd.f2s._BlockST's Wtb / Wgb / Wrb against f2s_bwd_ref.fold_transposed of f2s_ref.fold_block (fp32 against fp64: 1e-6)."""
    K, V = 3, 20
    for cin, cout, stride, residual in ((3, 16, 1, False), (16, 32, 2, True), (32, 32, 1, True)):
        blk = M.st_gcn(cin, cout, (9, K), stride, residual=residual).eval()
        fill_state_(blk.state_dict(), seed=7 + cin)
        Ae = make_input((K, V, V), seed=3, lo=0.0) * (1 + 0.3 * make_input((K, V, V), seed=4))
        b = f2s._BlockST(blk, Ae, torch.device('cpu'))
        q = RB.fold_transposed(R.fold_block({'m.' + k: v for k, v in blk.state_dict().items()}, 'm', Ae, blk._rmode))
        for name, got in (('Wtb', b.Wtb), ('Wgb', b.Wgb), ('Wrb', b.Wrb)):
            ref = q[name]
            assert (got is None) == (ref is None), name
            if ref is not None:
                assert got.is_contiguous() and tuple(got.shape) == tuple(ref.shape), name
                assert float((got.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), name
        assert tuple(b.Wtb.shape) == (cout, cout, 9) and tuple(b.Wgb.shape) == (K, cin, cout)
        assert [t.data_ptr() for t in b.bparams[:3]] == [b.Ae.data_ptr(), b.Wgb.data_ptr(), b.Wtb.data_ptr()]


def _cases():
    return [('tcn_bwd', k) for k in RB.TCN_BWD_CASES] + [('gcn_bwd', k) for k in RB.GCN_BWD_CASES] + [('sal', k) for k in RB.SAL_CASES]


def _table(stage):
    return {'tcn_bwd': RB.TCN_BWD_CASES, 'gcn_bwd': RB.GCN_BWD_CASES, 'sal': RB.SAL_CASES}[stage]


@functools.lru_cache(maxsize=None)
def _ref(stage, cid):
    """(case, operands, fp64 reference, magnitude): computed once, shared by the tests below, never modified"""
    c = _table(stage)[cid]
    p = RB.problem(stage, c)
    return c, p, RB.evaluate(stage, c, p), RB.evaluate(stage, c, p, absval=True)


def test_the_case_table_covers_what_it_claims():
    t, g = RB.TCN_BWD_CASES.values(), RB.GCN_BWD_CASES.values()
    assert list(RB.TCN_BWD_CASES) == list(R.TCN_CASES)
    assert len(RB.GCN_BWD_CASES) == len(R.GCN_CASES) + sum(c['rmode'] == 2 for c in R.TCN_CASES.values())
    assert {c['rmode'] for c in g} == {0, 1, 2} and {c['stride'] for c in g} == {1, 2} and {c['K'] for c in g} == {1, 3}
    assert all(c['rmode'] == (1 if c['Cin'] == c['Cout'] else 0) for k, c in RB.GCN_BWD_CASES.items() if not k.endswith('_k3'))
    assert all(c['rmode'] == 2 and c['K'] == 3 for k, c in RB.GCN_BWD_CASES.items() if k.endswith('_k3'))
    assert {c['Cin'] for c in g} >= {2, 3, 21, 69, 128, 256}                      # rows masked inside a 16-row tile, and whole tiles
    assert any(c['rmode'] == 2 and c['stride'] == 2 and c['T'] % 2 == 0 for c in g) and any(c['rmode'] == 2 and c['stride'] == 2 and c['T'] % 2 for c in g)
    assert {c['stride'] for c in t} == {1, 2} and any(c['off'] for c in t) and any(c['off'] for c in g)


@pytest.mark.parametrize('stage, cid', _cases())
def test_an_fp32_evaluation_passes_the_bars(stage, cid):
    c, p, ref, mag = _ref(stage, cid)
    B.check(cid, RB.evaluate(stage, c, p, dt=torch.float32), ref, mag, RB.bar_L(stage, c))


@pytest.mark.parametrize('defect', RB.DEFECTS)
def test_the_bars_reject_a_real_defect(defect):
    """Each defect, evaluated in fp64 (no rounding at all), fails the bars of at least one case of every stage it can occur in."""
    stages = {'mask_wrong_tensor': ('tcn_bwd', 'gcn_bwd'), 'taps_not_mirrored': ('tcn_bwd',), 'stride_phase': ('tcn_bwd',),
              'ae_not_transposed': ('gcn_bwd',), 'res_dropped': ('gcn_bwd',), 'res_not_upsampled': ('gcn_bwd',),
              'drop_last_frame': ('tcn_bwd', 'gcn_bwd')}[defect]
    for want in stages:
        failed = 0
        for stage, cid in _cases():
            if stage != want:
                continue
            c, p, ref, mag = _ref(stage, cid)
            try:
                B.check(cid, RB.evaluate(stage, c, p, defect=defect), ref, mag, RB.bar_L(stage, c))
            except B.BarError:
                failed += 1
        assert failed >= 1, (defect, want)


# ---------------------------------------------------------------------------------------------------------------------
# body parts
# ---------------------------------------------------------------------------------------------------------------------
def _state(K, P):
    return [0] * K, [[0.0] * P for _ in range(K)]


def test_part_bookkeeping_on_hand_made_cases():
    parts = [[0, 1], [2]]
    sal = [[1.0, 3.0, 5.0], [2.0, 2.0, 8.0], [4.0, 0.0, 1.0], [9.0, 9.0, 9.0]]
    # the cap is reached in mid-batch: class 0 takes samples 0 and 1, not 3; class 2 stays empty
    count, total = _state(3, 2)
    RB.part_accumulate(count, total, sal, [0, 0, 1, 0], parts, per_class=2)
    assert count == [2, 1, 0]
    assert total == [[2.0 + 2.0, 5.0 + 8.0], [2.0, 1.0], [0.0, 0.0]]
    imp = RB.part_importance(count, total)
    assert imp == [[2.0 / 6.5, 1.0], [1.0, 0.5], [0.0, 0.0]]
    # a later batch cannot add to the full class, an out-of-range label is ignored
    RB.part_accumulate(count, total, sal, [0, 2, 7, -1], parts, per_class=2)
    assert count == [2, 1, 1] and total[0] == [4.0, 13.0] and total[2] == [2.0, 8.0]
    # an all-zero class divides by 1
    count, total = _state(2, 2)
    RB.part_accumulate(count, total, [[0.0, 0.0, 0.0]], [1], parts, per_class=5)
    assert RB.part_importance(count, total) == [[0.0, 0.0], [0.0, 0.0]] and count == [0, 1]
    # per_class 0 counts nothing
    count, total = _state(2, 2)
    RB.part_accumulate(count, total, sal, [0, 1, 0, 1], parts, per_class=0)
    assert count == [0, 0]


def test_default_parts_and_argument_checks():
    assert {k: list(v) for k, v in saliency.UCLA_PARTS.items()} == RB.UCLA_PARTS
    assert sorted(j for v in saliency.UCLA_PARTS.values() for j in v) == list(range(2, 20))

    class Fake:
        num_point, training = 17, False
    with pytest.raises(ValueError, match='needs parts='):
        saliency.PartImportance(Fake(), 10)
    with pytest.raises(ValueError, match='joints inside'):
        saliency.PartImportance(Fake(), 10, parts={'a': [17]})
    imp = saliency.PartImportance(Fake(), 3, parts={'a': [0, 16], 'b': [5]})
    assert imp.compute() == {k: {'a': 0.0, 'b': 0.0} for k in range(3)}            # nothing seen yet: no device needed
    m = M.Model(num_class=4, num_point=20, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
    with pytest.raises(ValueError, match='eval'):
        saliency.joint_saliency(m, torch.zeros(1, 3, 8, 20, 1))
    with pytest.raises(RuntimeError, match='no CPU path'):
        saliency.input_gradient(m.eval(), torch.zeros(1, 3, 8, 20, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the reference pin
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', STGCN_MODEL_CASES, ids=[c[0] for c in STGCN_MODEL_CASES])
def test_oracle_gradient_equals_the_reference_fixture(case):
    tag, margs, shape = case
    m = M.Model(**margs)
    fill_stgcn_(m.state_dict(), seed=77)
    sd = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in m.state_dict().items()}
    x = make_input(shape, seed=21).double().requires_grad_(True)
    lab = make_labels(shape[0], margs['num_class'], seed=22)
    assert np.array_equal(lab.numpy(), GOLD[f'{tag}/labels'])
    logits = SO.model_forward(x, sd, margs['num_point'], training=False)
    (g,) = torch.autograd.grad(torch.gather(logits, 1, lab.unsqueeze(1)).sum(), x)
    ref = torch.from_numpy(GOLD[f'{tag}/dx64'])
    assert g.dtype == ref.dtype == torch.float64
    assert float((g - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    sal = torch.from_numpy(GOLD[f'{tag}/saliency'])
    assert float((g.abs().sum((1, 2, 4)) - sal).abs().max()) <= 1e-12 * float(sal.abs().max())
    g32 = torch.from_numpy(GOLD[f'{tag}/dx32']).double()                            # the reference's own fp32 run sits far inside
    assert float((g32 - ref).norm() / ref.norm()) <= 5e-2 / 100                    # the end-to-end bars of test_gpu_saliency.py


def test_bad_arguments_are_refused_on_the_host():
    """Argument checks run before any HIP call: exercised here without a GPU, the entry point's name in tamgcn_last_error()."""
    lib = _lib.load()
    one = (C.c_float * 64)()
    p = C.addressof(one)
    d = _lib.F2sTcnBwdDesc(N=1, Cout=24, T=4, V=20, KT=9, stride=1, gout=p, out=p, h=p, wtb=p, dh=p)
    assert lib.tamgcn_f2s_tcn_bwd(C.byref(d), None) < 0 and b'tamgcn_f2s_tcn_bwd' in lib.tamgcn_last_error()
    d = _lib.F2sTcnBwdDesc(N=1, Cout=16, T=4, V=20, KT=5, stride=1, gout=p, out=p, h=p, wtb=p, dh=p)
    assert lib.tamgcn_f2s_tcn_bwd(C.byref(d), None) < 0 and b'tamgcn_f2s_tcn_bwd' in lib.tamgcn_last_error()
    for kw in (dict(V=33), dict(Cin=300), dict(res_mode=3), dict(res_mode=1, Cin=3), dict(res_mode=2), dict(res_mode=1, gout=None), dict(stride=3)):
        a = dict(N=1, Cin=16, Cout=16, T=4, V=20, K=3, stride=1, res_mode=0, dh=p, Ae=p, wgb=p, gout=p, out=p, wrb=None, dx=p)
        a.update(kw)
        d = _lib.F2sGcnBwdDesc(**a)
        assert lib.tamgcn_f2s_gcn_bwd(C.byref(d), None) < 0 and b'tamgcn_f2s_gcn_bwd' in lib.tamgcn_last_error(), kw
    assert lib.tamgcn_saliency_joints(None, p, 1, 3, 4, 20, 1, p, None, None) < 0 and b'tamgcn_saliency_joints' in lib.tamgcn_last_error()
    assert lib.tamgcn_saliency_joints(p, p, 0, 3, 4, 20, 1, p, None, None) < 0
    for n, P in ((0, 5), (4097, 5), (4, 257), (4, 0)):
        assert lib.tamgcn_saliency_accumulate(p, p, n, 20, p, p, P, 10, 200, p, p, None) < 0
        assert b'tamgcn_saliency_accumulate' in lib.tamgcn_last_error()
    assert lib.tamgcn_saliency_accumulate(p, None, 4, 20, p, p, 5, 10, 200, p, p, None) < 0
