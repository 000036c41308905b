"""CPU: the host side of the run-time-V small-batch eval family (csrc/f2g.hip, tam_gcn_amd/f2g.py): which joint counts the
library serves, its LDS requests over the whole range against the 160 KB cap (and against the formulas restated here), the
refusals of every entry point without a GPU, engine construction and refusals, the registered operator's fake implementation
and the routing conditions of Model._f2g.  (The kernels themselves: tests/test_gpu_f2g_stages.py, tests/test_gpu_f2g.py.)"""
import ctypes as C
import re

import pytest
import torch

import f2_ref as R
from params import make_input
from tam_gcn_amd import _lib, f2, f2g, f2v
from tam_gcn_amd.models import ctrgcn as M

CAP = 160 * 1024
E, GCN, GEMM, TCN = 0, 1, 2, 3
UCLA = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
NTU = dict(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
OPENPOSE = dict(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=dict(labeling_mode='spatial'))


def tree(V, persons=1, classes=6):
    return dict(num_class=classes, num_point=V, num_person=persons, graph='tam_gcn_amd.graph.synthetic.Graph',
                graph_args=dict(num_node=V, arity=2))


def test_supported_exactly_on_the_range_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.tamgcn_version() == 401
    assert f2g.JOINTS_RANGE == (8, 28)
    for V in range(-2, 70):
        assert lib.tamgcn_f2g_supported(V) == (1 if 8 <= V <= 28 else 0), V


def _lds(stage, V, c, r):
    """the requests restated from the geometry (FgGeo, FgRt and the fg_*_lds formulas of csrc/f2g.hip)"""
    VP = (V + 3) & ~3
    PB, PH, EC = R.BT * VP + 4, R.HF * VP + 4, V * VP
    PD, ES = ((EC + 15) // 16) * 16 + 4, ((8 * EC + 255) // 256) * 256
    Kp = (c + 15) & ~15
    if stage == E:
        R2p, Rp = max(16, 2 * r), (r + 15) & ~15
        req = [4 * (Kp * R.PX + R2p * R.PX + 64 * R.PX + max(Rp * PD, ntp * Kp * VP)) for ntp in (4, 2)]
        return req[0] if req[0] <= CAP else req[1]
    if stage == GCN:
        kc = 128
        while kc > 16 and 4 * (min(Kp, kc) * PB + 64 * PB + 3 * ES) > CAP:
            kc -= 16
        return 4 * (min(Kp, kc) * PB + 64 * PB + 3 * ES)
    if stage == GEMM:
        return 4 * (Kp + 64) * PB
    return 4 * (80 * PB + max(Kp * PB, r * PH))


def test_lds_requests_fit_the_cap_over_the_whole_range():
    lib = _lib.load()
    worst = {}
    for V in range(8, 29):
        for Cin in (3, 64, 256):
            for Rr in (1, 8, 32):
                for Cb in (16, 64):
                    for stage, r in ((E, Rr), (GCN, Rr), (GEMM, Rr), (TCN, Cb)):
                        got = lib.tamgcn_f2g_lds_bytes(stage, V, Cin, r)
                        assert 0 < got <= CAP, (stage, V, Cin, r, got)
                        assert got == _lds(stage, V, Cin, r), (stage, V, Cin, r)
                        worst[stage] = max(worst.get(stage, 0), got)
    # the wide end: f2v's 128-row K chunk would need 165.9 KB at V = 28 (three E runs of 25.6 KB, two x3 tiles of 29.7 KB, 59.4 KB
    # of K rows); 112 rows fit
    PB, ES = 116, 6400
    assert 4 * (128 * PB + 64 * PB + 3 * ES) > CAP
    assert lib.tamgcn_f2g_lds_bytes(GCN, 28, 256, 0) == 4 * (112 * PB + 64 * PB + 3 * ES)
    assert lib.tamgcn_f2g_lds_bytes(GCN, 27, 256, 0) == 4 * (128 * PB + 64 * PB + 3 * 6144) == worst[GCN]    # 128 rows below 28 joints
    assert lib.tamgcn_f2g_lds_bytes(E, 28, 256, 32) == 156160                                     # two frame phases
    assert all(w <= CAP for w in worst.values())


def test_lds_bytes_refuses_what_the_entry_points_refuse():
    lib = _lib.load()
    for stage in (E, GCN, GEMM, TCN):
        for V in (7, 29):
            assert lib.tamgcn_f2g_lds_bytes(stage, V, 64, 16) == -1
        assert lib.tamgcn_f2g_lds_bytes(stage, 16, 257, 16) == -1 and lib.tamgcn_f2g_lds_bytes(stage, 16, 0, 16) == -1
    assert lib.tamgcn_f2g_lds_bytes(E, 16, 64, 33) == -1 and lib.tamgcn_f2g_lds_bytes(E, 16, 64, 0) == -1
    assert lib.tamgcn_f2g_lds_bytes(TCN, 16, 64, 80) == -1 and lib.tamgcn_f2g_lds_bytes(TCN, 16, 64, 24) == -1
    assert lib.tamgcn_f2g_lds_bytes(4, 16, 64, 16) == -1


_DESC = {'e': _lib.F2GcnDesc, 'gcn': _lib.F2GcnDesc, 'gemm': _lib.F2GemmDesc, 'tcn': _lib.F2TcnDesc}


@pytest.mark.parametrize('stage', list(_DESC))
def test_entry_points_refuse_on_the_host_without_a_gpu(stage):
    lib = _lib.load()
    name = f'tamgcn_f2g_{stage}'
    fn = getattr(lib, name)
    assert fn(None, None) < 0
    msg = lib.tamgcn_last_error()
    assert name.encode() in msg and b'V=' in msg and b'null' in msg, msg
    for V in (0, 7, 29, 32):
        d = _DESC[stage](V=V)                                      # every pointer NULL: V is looked at first
        assert fn(C.byref(d), None) < 0
        msg = lib.tamgcn_last_error()
        assert name.encode() in msg and f'V={V} '.encode() in msg and b'8 <= V <= 28' in msg, msg
    d = _DESC[stage](V=21)                                         # a served joint count: the next check refuses, still before any HIP call
    assert fn(C.byref(d), None) < 0
    assert name.encode() in lib.tamgcn_last_error() and b'V=21 (' not in lib.tamgcn_last_error()


def test_engine_constructs_and_refuses():
    for V, persons in ((16, 1), (21, 2)):
        m = M.Model(**tree(V, persons))
        with pytest.raises(ValueError):
            f2g.FusedEvalG(m)                                       # train mode
        m.eval()
        eng = f2g.FusedEvalG(m)
        assert isinstance(eng, f2.FusedEval) and eng.V == V and eng.FAMILY == 'f2g'
        assert type(eng)._state_key is f2.FusedEval._state_key and type(eng)._packed is f2.FusedEval._packed
        blocks = eng._packed(torch.device('cpu'))
        assert len(blocks) == 10 and all(isinstance(b, f2._Block) for b in blocks)
        x = make_input((1, 3, 8, V, persons), seed=1)
        with torch.no_grad():
            with pytest.raises(RuntimeError, match='no CPU path'):
                eng(x)
            with pytest.raises(RuntimeError, match='no CPU path'):
                torch.ops.tamgcn.tcn_gcn_unit_eval_vg(torch.zeros(1, 64, 8, V), None, blocks[1].params, blocks[1].geom)
            assert m._f2g(x) is None                                # CPU tensors route nowhere
            assert m._f2(x) is None and m._f2v(x) is None and m._f2j(x) is None
    for V in (7, 32):
        with pytest.raises(f2.Unsupported, match=re.escape('8 <= V <= 28')):      # the message names the range
            f2g.FusedEvalG(M.Model(**tree(V)).eval())
    assert f2g.FusedEvalG.__mro__[1] is f2.FusedEval
    # the engine itself takes the dedicated joint counts too (measured against f2 / f2v); the routing does not send them
    assert f2g.FusedEvalG(M.Model(**COCO).eval()).V == 17


def test_operator_is_registered_with_a_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    blocks = f2g.FusedEvalG(M.Model(**tree(21, 2)).eval())._packed(torch.device('cpu'))
    b = blocks[4]                                                   # 64 -> 128, stride 2
    with FakeTensorMode() as mode:
        x = mode.from_tensor(torch.zeros(2, 64, 11, 21))
        params = [mode.from_tensor(t) for t in b.params]
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_vg(x, None, params, b.geom)
        assert tuple(out.shape) == (2, 128, 6, 21) and tuple(xp.shape) == (2, 2, 128, 24)
        x = mode.from_tensor(torch.zeros(1, 64, 8, 16))             # a multiple of four: no pad columns
        out, xp = torch.ops.tamgcn.tcn_gcn_unit_eval_vg(x, None, params, b.geom)
        assert tuple(out.shape) == (1, 128, 4, 16) and tuple(xp.shape) == (1, 1, 128, 16)


class _OnDevice:
    """a CPU tensor that answers is_cuda: the routing conditions without a GPU (no engine is built for a refused model)"""

    def __init__(self, t):
        self.t, self.is_cuda, self.dtype, self.shape, self.device = t, True, t.dtype, t.shape, t.device

    def dim(self):
        return self.t.dim()


def test_routing_leaves_the_dedicated_and_the_outside_joint_counts_alone(monkeypatch):
    assert f2g.DEDICATED == (17, 18, 20, 25) and set(f2v.JOINTS) | {20} == set(f2g.DEDICATED)
    with torch.no_grad():
        for margs in (COCO, OPENPOSE, UCLA, NTU, tree(7), tree(29), tree(32)):
            m = M.Model(**margs).eval()
            x = _OnDevice(torch.zeros(1, 3, 8, margs['num_point'], margs['num_person']))
            assert m._f2g(x) is None and '_tamgcn_f2g' not in m.__dict__, margs['num_point']
        m = M.Model(**tree(21, 2)).eval()
        x = _OnDevice(torch.zeros(1, 3, 8, 21, 2))
        monkeypatch.setattr(f2g, 'F2G_MAX_FRAMES', 15)               # 1 clip x 2 persons x 8 frames
        assert m._f2g(x) is None and '_tamgcn_f2g' not in m.__dict__
        monkeypatch.setattr(f2g, 'F2G_MAX_FRAMES', 16)
        monkeypatch.setenv('TAMGCN_F2', '0')
        assert m._f2g(x) is None and '_tamgcn_f2g' not in m.__dict__
        monkeypatch.delenv('TAMGCN_F2')
        eng = m._f2g(x)                                              # every condition met: the engine, in its own slot
        assert type(eng) is f2g.FusedEvalG and m.__dict__['_tamgcn_f2g'] is eng
        assert '_tamgcn_f2' not in m.__dict__ and '_tamgcn_f2v' not in m.__dict__ and '_tamgcn_f2j' not in m.__dict__
        h = m.l3.register_forward_hook(lambda *a: None)
        assert m._f2g(x) is None
        h.remove()
        assert m._f2g(x) is eng
        m.train()
        assert m._f2g(x) is None
    m.eval()
    assert m._f2g(x) is None                                         # autograd on


def test_ledger_bars_hold_for_a_correct_fp32_evaluation_at_the_new_joint_counts():
    """the GPU ledger's own table (tests/test_gpu_f2g_stages.py) evaluated in fp32 on the CPU: the derived bars are not too tight"""
    import zlib
    import f2g_cases as T
    for stage, table in T.STAGES.items():
        for cid, c in table.items():
            for V in (9, 22):
                p = R.sub(stage, R.problem(stage, c, V, zlib.crc32(cid.encode()) & 0xffff), 0)
                if stage == 'e':
                    R.check_e('fp32', p, R.e(p, torch.float32))
                elif stage == 'gcn':
                    R.check_gcn('fp32', p, *R.gcn(p, torch.float32), V)
                elif stage == 'gemm':
                    R.check_gemm('fp32', p, R.gemm(p, torch.float32))
                else:
                    out = R.tcn(p, torch.float32)
                    R.check_tcn('fp32', p, out, R.tile_sums(out, torch.float32))


def test_the_ledger_table_reaches_what_it_must():
    """the conditions of tests/f2_ref.py's `paths`, on the table of tests/f2g_cases.py"""
    import f2g_cases as T
    reach = {s: set().union(*(R.paths(s, c, 'f2v') for c in T.STAGES[s].values())) for s in T.STAGES}
    assert {'w12:vec', 'w12:scalar', 'w12:ktail', 'w4:vec', 'w4:scalar', 'w4:second', 'alpha0', 'alpha', 'xsrc:x', 'xsrc:xpart',
            'T1', 'T3', 'T4', 'T5', 'framestep', 'tiles3', 'tiles9'} <= reach['e']
    assert {c['R'] for c in T.E_CASES.values()} >= {1, 12, 32}
    assert {'w3:vec', 'w3:scalar', 'w3:ktail', 'wd:vec', 'wd:scalar', 'res0', 'res1', 'res2', 'chunks2', 'chunk:partial',
            'chunk:scalartail'} <= reach['gcn']
    assert {'w:vec', 'w:scalar', 'w:ktail', 'mode0', 'mode1', 'relu:none', 'relu:all', 'relu:midtile', 'relu:tileedge'} <= reach['gemm']
    assert {'nb1', 'nb2', 'nb4', 'Cb16', 'Cb64', 'stride1', 'stride2', 'res0@s2', 'res1@s1', 'res2@s1', 'res2@s2', 'pool:lastframe',
            'atlimit:k3d5@s1', 'atlimit:k5d2@s1', 'atlimit:k9d1@s1', 'atlimit:k5d2@s2', 'atlimit:k9d1@s2', 'wr:vec', 'wr:scalar',
            'wt:vec', 'wt:scalar', 'xpart:given', 'xpart:null'} <= reach['tcn']
    for s, key in (('e', 'T'), ('gcn', 'T'), ('gemm', 'T'), ('tcn', 'T')):
        assert {c[key] for c in T.STAGES[s].values()} >= {1, 3, 4, 5, 9, 33}, s
    assert any(c['Cin'] == 256 for c in T.E_CASES.values()) and any(c['Cin'] == 256 for c in T.GCN_CASES.values())
    assert any(c['K'] == 256 for c in T.GEMM_CASES.values()) and any(c['Cin'] == 256 and c['res_mode'] == 2 for c in T.TCN_CASES.values())
    assert 28 in T.JOINTS and {R.vp(V) for V in T.JOINTS} == {8, 12, 16, 20, 24, 28}
    assert {V - (R.vp(V) - 4) for V in T.JOINTS} == {1, 2, 3, 4}
