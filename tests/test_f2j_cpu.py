"""CPU: the host side of the small-batch eval family at 17 and 18 joints (tam_gcn_amd/f2v.py: JOINTS, FusedEvalJ; csrc/f2v.hip:
FV_JOINTS) -- the mirrored list against the source text, engine construction and refusals, the folded blocks composed through
tests/f2_ref.py's fp64 stage references against the oracle's block, the ledger's bars under a correct fp32 evaluation at both
joint counts, and the LDS requests of the host formulas.  (The kernels themselves: tests/test_gpu_f2j_stages.py, test_gpu_f2j.py.)"""
import os
import re
import zlib

import pytest
import torch

import f2_ref as R
from params import fill_state_, make_input
from tam_gcn_amd import f2, f2v
from tam_gcn_amd.models import ctrgcn as M
from oracle import ctrgcn_oracle as O

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
OPENPOSE = dict(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=dict(labeling_mode='spatial'))
TREE7 = dict(num_class=6, num_point=7, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=7, arity=2))
UCLA = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
NTU = dict(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))


def _src(name='f2v.hip'):
    with open(os.path.join(ROOT, 'tam_gcn_amd', 'csrc', name)) as f:
        return f.read()


def test_joints_mirror_the_instantiation_list_of_the_source():
    src = _src()
    lists = re.findall(r'^#define FV_JOINTS\(X\)((?:\s*X\(\d+\))+)\s*$', src, re.M)
    assert len(lists) == 1, 'the joint counts are kept in ONE place'
    joints = tuple(int(v) for v in re.findall(r'X\((\d+)\)', lists[0]))
    assert joints == f2v.JOINTS == (17, 18, 25)
    # nothing is instantiated past the list: no kernel, host template or geometry is named with a literal joint count -- in
    # f2v.hip or in the bodies it shares with f2g.hip
    for text in (src, _src('f2x_body.h'), _src('f2_common.h')):
        assert not re.search(r'_kernel<\s*\d+\s*>', text) and not re.search(r'FvHost<\s*\d+\s*>', text) and not re.search(r'FvGeo<\s*\d+\s*>', text)
    assert all(v % 4 for v in joints)                            # V % 4 != 0 stays asserted in FvGeo
    assert 'V % 4 != 0' in src


def test_engine_constructs_for_coco_and_openpose_and_refuses_the_rest():
    for margs in (COCO, OPENPOSE):
        m = M.Model(**margs)
        with pytest.raises(ValueError):
            f2v.FusedEvalJ(m)                                       # train mode
        m.eval()
        eng = f2v.FusedEvalJ(m)
        assert isinstance(eng, f2.FusedEval) and eng.V == margs['num_point'] and eng.FAMILY == 'f2v'
        assert type(eng)._state_key is f2.FusedEval._state_key and type(eng)._packed is f2.FusedEval._packed
        blocks = eng._packed(torch.device('cpu'))
        assert len(blocks) == 10 and all(isinstance(b, f2._Block) for b in blocks)
        with pytest.raises(f2.Unsupported, match='V = 25'):
            f2v.FusedEvalV(m)                                       # the 25-joint engine stays that
        x = make_input((1, 3, 8, margs['num_point'], margs['num_person']), seed=1)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match='no CPU path'):
                eng(x)
            with pytest.raises(RuntimeError, match='no CPU path'):
                torch.ops.tamgcn.tcn_gcn_unit_eval_vj(torch.zeros(1, 64, 8, margs['num_point']), None, blocks[1].params, blocks[1].geom)
            assert m._f2(x) is None and m._f2v(x) is None and m._f2j(x) is None      # CPU tensors route nowhere
    for margs in (UCLA, NTU, TREE7):
        with pytest.raises(f2.Unsupported, match=re.escape(str(f2v.JOINTS))):      # the message names the list
            f2v.FusedEvalJ(M.Model(**margs).eval())
    assert f2v.FusedEvalJ.__mro__[1] is f2.FusedEval


def test_non_family_block_plans_are_refused_before_any_launch():
    """The plans tests/test_f2v_cpu.py uses, on a 17-joint graph."""
    A = M.Model(**COCO).graph.A
    blk = M.TCN_GCN_unit(65, 65, A, kernel_size=5, dilations=[1, 2, 3])
    with pytest.raises(f2.Unsupported):                          # 3 temporal branches of 13 channels: not a multiple of 16
        f2._Block(blk, torch.device('cpu'))
    m = M.Model(**COCO).eval()
    m.l4 = M.TCN_GCN_unit(64, 64, A[:2]).eval()                     # two subsets
    with pytest.raises(f2.Unsupported, match='subsets'):
        f2v.FusedEvalJ(m)._packed(torch.device('cpu'))


def test_grouped_engine_picks_the_new_engine_and_operator():
    for margs in (COCO, OPENPOSE):
        eng = f2.GroupedEval([M.Model(**margs).eval() for _ in range(2)])
        assert eng.FAMILY == 'f2v' and all(type(e) is f2v.FusedEvalJ for e in eng.engines)
        assert eng._blk is torch.ops.tamgcn.tcn_gcn_unit_eval_vj_grouped
    eng = f2.GroupedEval([M.Model(**NTU).eval()])
    assert type(eng.engines[0]) is f2v.FusedEvalV and eng._blk is torch.ops.tamgcn.tcn_gcn_unit_eval_v25_grouped
    with pytest.raises(f2.Unsupported):
        f2.GroupedEval([M.Model(**TREE7).eval()])


def test_operators_are_registered_with_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for margs in (COCO, OPENPOSE):
        V = margs['num_point']
        blocks = f2v.FusedEvalJ(M.Model(**margs).eval())._packed(torch.device('cpu'))
        b = blocks[4]                                               # 64 -> 128, stride 2
        stacked = [torch.stack([t, t]) for t in b.params]
        with FakeTensorMode() as mode:
            x = mode.from_tensor(torch.zeros(2, 64, 11, V))
            params = [mode.from_tensor(t) for t in b.params]
            out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_vj(x, None, params, b.geom)
            assert tuple(out.shape) == (2, 128, 6, V) and tuple(xp.shape) == (2, 2, 128, 20)
            gp = [mode.from_tensor(t) for t in stacked]
            x4 = mode.from_tensor(torch.zeros(4, 64, 11, V))
            out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_vj_grouped(x4, None, gp, b.geom, 2)
            assert tuple(out.shape) == (4, 128, 6, V) and tuple(xp.shape) == (4, 2, 128, 20)


# ---------------------------------------------------------------------------------------------------------------------
# the folded blocks through f2_ref's fp64 stage references == the oracle's block
# ---------------------------------------------------------------------------------------------------------------------
def _through_stage_refs(b, x):
    """e -> gcn -> gemm 0 -> gemm 1 -> tcn of tests/f2_ref.py on the folded tensors of one f2._Block"""
    N, Cin, T, V = x.shape
    none = lambda t: None if t is None or t.numel() == 0 else t          # noqa: E731
    p = dict(N=N, T=T, Cin=Cin, Cout=b.Cout, R=b.R, res_mode=b.gmode, x=x, xpart=None, A=b.PA, alpha=b.alpha,
             w12=b.W12, b12=b.B12, w4=b.W4.reshape(3, b.Cout, b.R), b4=b.B4.reshape(3, b.Cout), w3=b.W3, b3=b.B3, sy=b.sy, ty=b.ty,
             wd=none(b.Wd), bd=none(b.bd))
    p['E'] = R.e(p)
    sm, df = R.gcn(p)
    g = R.gemm(dict(mode=0, relu_rows=0, K=b.Cout, M=b.Cout, x=df, add=sm, w=b.Wo, b=b.bo))
    h = R.gemm(dict(mode=1, relu_rows=(b.nb + 1) * b.Cb, K=b.Cout, M=b.Cout, x=g, w=b.We, b=b.be))
    q = dict(N=N, T=T, Cin=Cin, Cout=b.Cout, Cb=b.Cb, nb=b.nb, ks=b.ks, dils=tuple(b.dils), stride=b.stride, res_mode=b.rmode, h=h, x=x,
             wt=b.Wt, bt=b.bt, sp=b.sp, tp=b.tp, wr=none(b.Wr), br=none(b.br))
    return R.tcn(q)


@pytest.mark.parametrize('margs, shape', [(COCO, (2, 3, 13, 17, 1)), (OPENPOSE, (1, 3, 20, 18, 2)), (OPENPOSE, (1, 3, 13, 18, 2))],
                         ids=['coco_t13', 'openpose_t20_two_persons', 'openpose_t13_two_persons'])
def test_folded_blocks_through_the_stage_references_equal_the_oracle(margs, shape):
    V = margs['num_point']
    m = M.Model(**margs).double()
    sd = m.state_dict()
    fill_state_(sd, seed=42)
    with torch.no_grad():                                   # moderate running statistics (seeded ones blow the activations up tenfold per block)
        for k, v in sd.items():
            if k.endswith('running_var'):
                v.mul_(4.0)
    m.eval()
    x = make_input(shape, seed=5).double()
    h, _, Mp = O._stem(x, sd, V, False)
    assert Mp == shape[4] and h.shape[0] == shape[0] * shape[4]
    blocks = f2v.FusedEvalJ(m)._packed(torch.device('cpu'))
    for i, blk in enumerate(blocks, 1):
        ref = O.tcn_gcn_unit(h, sd, f'l{i}', O._STRIDES.get(i, 1), residual=(i != 1), training=False)
        with torch.no_grad():
            got = _through_stage_refs(blk, h)
        assert got.shape == ref.shape and got.dtype == F64
        assert float((got - ref).abs().max()) <= 1e-11 * float(ref.abs().max()), f'l{i}'
        h = ref


# ---------------------------------------------------------------------------------------------------------------------
# the ledger's bars hold for a correct fp32 evaluation at these joint counts (the ledger's seeds: crc32 of the case id)
# ---------------------------------------------------------------------------------------------------------------------
def _fp32(stage, p):
    if stage == 'e':
        return R.check_e('fp32', p, R.e(p, F32))
    if stage == 'gcn':
        return R.check_gcn('fp32', p, *R.gcn(p, F32), p['V'])
    if stage == 'gemm':
        return R.check_gemm('fp32', p, R.gemm(p, F32))
    out = R.tcn(p, F32)
    return R.check_tcn('fp32', p, out, R.tile_sums(out, F32))


@pytest.mark.parametrize('V', [17, 18])
@pytest.mark.parametrize('stage', list(R.STAGES))
def test_fp32_evaluation_passes_every_bar_of_the_ledger(stage, V):
    n = 0
    for cid, c in R.STAGES[stage].items():
        p = R.problem(stage, c, V, zlib.crc32(cid.encode()) & 0xffff)
        for g in range(c['G']):
            _fp32(stage, R.sub(stage, p, g))
            n += 1
    assert n == sum(c['G'] for c in R.STAGES[stage].values())


# ---------------------------------------------------------------------------------------------------------------------
# the host LDS requests, restated from the geometry (FvGeo of csrc/f2v.hip and the f2_*_lds formulas of csrc/f2_common.h)
# ---------------------------------------------------------------------------------------------------------------------
def _geo(V):
    VP = (V + 3) & ~3
    NC = R.BT * VP
    EC = V * VP
    ECT = (EC + 15) // 16
    return dict(VP=VP, QF=VP // 4, NC=NC, NCT=NC // 16, PB=NC + 4, EC=EC, ECT=ECT, PD=ECT * 16 + 4, PH=R.HF * VP + 4,
                ES=((8 * EC + 255) // 256) * 256)


def _lds(V, Cin, Rr, Cb):
    g = _geo(V)
    Kp, R2p, Rp = (Cin + 15) & ~15, max(16, 2 * Rr), (Rr + 15) & ~15
    e = 4 * (Kp * R.PX + R2p * R.PX + 64 * R.PX + max(Rp * g['PD'], 4 * Kp * g['VP']))
    gcn = 4 * (min(Kp, R.KC) * g['PB'] + 2 * 32 * g['PB'] + 3 * g['ES'])
    gemm = 4 * (Kp * g['PB'] + 4 * 16 * g['PB'])
    tcn = 4 * (5 * 16 * g['PB'] + max(Kp * g['PB'], Cb * g['PH']))
    return e, gcn, gemm, tcn


@pytest.mark.parametrize('V', [17, 18])
def test_lds_requests_fit_at_every_served_width(V):
    g = _geo(V)
    assert (g['VP'], g['NC'], g['NCT'], g['EC']) == (20, 80, 5, V * 20)
    assert g['NC'] % 16 == 0 and (4 * g['PB']) % 64 == 16 and (4 * g['PD']) % 64 == 16 and (4 * g['EC']) % 16 == 0   # FvGeo's asserts
    assert V - 4 * (g['QF'] - 1) == (1 if V == 17 else 2)          # live lanes of a frame's last 16-byte piece
    worst = [0, 0, 0, 0]
    for Cin in (3, 16, 40, 64, 128, 144, 200, 256):
        for Rr in (1, 8, 16, 20, 32):
            for Cb in (16, 32, 48, 64):
                req = _lds(V, Cin, Rr, Cb)
                assert req[0] == R.fv_e_lds(Cin, Rr, 4, V)          # four frame phases always fit: the two-phase fallback is never taken
                assert all(r <= R.LDS_MAX for r in req), (Cin, Rr, Cb, req)
                worst = [max(a, b) for a, b in zip(worst, req)]
    # the stock model's widest layers (Cin 256, R 32; l8's convolutional residual from 128 channels, Cb 64)
    assert _lds(V, 256, 32, 64)[0] == worst[0] and worst[0] <= 141 * 1024
    assert worst[1] <= 100 * 1024 and _lds(V, 128, 8, 64)[3] <= 116 * 1024
