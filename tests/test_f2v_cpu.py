"""CPU: the host side of the 25-joint small-batch eval family (tam_gcn_amd/f2v.py, csrc/f2v.hip) -- engine construction and
guards, the argument checks of the four entry points (all of them run before any HIP call), and the folded block at V = 25,
M = 2 against the oracle.  (The kernels themselves: tests/test_gpu_f2v.py.)"""
import ctypes as C

import pytest
import torch

from cases import MODEL_CASES, MODEL_PARAM_SEED
from params import fill_state_, make_input
from tam_gcn_amd import f2, f2v, _lib
from tam_gcn_amd.models import ctrgcn as M
from oracle import ctrgcn_oracle as O
from test_f2_cpu import _restate

NTU = next(c for c in MODEL_CASES if c[0] == 'ntu_t20')[1]
UCLA = next(c for c in MODEL_CASES if c[0] == 'ucla_t52')[1]


def test_engine_constructs_on_an_eval_ntu_model_and_refuses_the_rest():
    m = M.Model(**NTU)
    with pytest.raises(ValueError):
        f2v.FusedEvalV(m)                                   # train mode
    m.eval()
    eng = f2v.FusedEvalV(m)
    assert isinstance(eng, f2.FusedEval) and eng.V == 25   # one engine class: state key and re-fold are f2's
    assert type(eng)._state_key is f2.FusedEval._state_key and type(eng)._packed is f2.FusedEval._packed
    blocks = eng._packed(torch.device('cpu'))
    assert len(blocks) == 10 and all(isinstance(b, f2._Block) for b in blocks)
    with pytest.raises(f2v.Unsupported, match='V = 25'):
        f2v.FusedEvalV(M.Model(**UCLA).eval())              # 20 joints: the other family
    with pytest.raises(f2.Unsupported, match='V = 20'):
        f2.FusedEval(m)                                     # ... and that one still refuses 25
    assert f2v.Unsupported is f2.Unsupported
    x = make_input((1, 3, 8, 25, 2), seed=1)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU path'):
            eng(x)
        with pytest.raises(RuntimeError, match='no CPU path'):
            torch.ops.tamgcn.tcn_gcn_unit_eval_v25(torch.zeros(1, 64, 8, 25), None, blocks[1].params, blocks[1].geom)
    m.train()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='train'):
            eng(x)


def test_unsupported_geometries_are_refused_before_any_launch():
    A = M.Model(**NTU).graph.A
    blk = M.TCN_GCN_unit(65, 65, A, kernel_size=5, dilations=[1, 2, 3])
    with pytest.raises(f2v.Unsupported):                   # 3 temporal branches of 13 channels: not a multiple of 16
        f2._Block(blk, torch.device('cpu'))
    m = M.Model(**NTU).eval()
    m.l4 = M.TCN_GCN_unit(64, 64, A[:2]).eval()             # two subsets
    with pytest.raises(f2v.Unsupported, match='subsets'):
        f2v.FusedEvalV(m)._packed(torch.device('cpu'))
    assert m._f2(torch.zeros(1, 3, 8, 25, 2)) is None and m._f2v(torch.zeros(1, 3, 8, 25, 2)) is None     # CPU tensors route nowhere


def _descs(V=25, M_=64, K=64):
    p = 1 << 20
    gcn = _lib.F2GcnDesc(N=1, Cin=K, Cout=M_, T=8, V=V, S=3, R=8, res_mode=0, x=p, w12=p, b12=p, w4=p, b4=p, A=p, alpha=p, w3=p, b3=p,
                         sy=p, ty=p, wd=None, bd=None, E=p, sum=p, diff=p, xpart=None)
    gemm = _lib.F2GemmDesc(N=1, K=K, M=M_, T=8, V=V, mode=1, relu_rows=0, x=p, w=p, b=p, add=None, out=p)
    tcn = _lib.F2TcnDesc(N=1, Cin=K, Cout=M_, T=8, V=V, stride=2, Cb=M_ // 4, nb=2, ks=5, res_mode=2, h=p, sp=p, tp=p, x=p, wr=p, br=p,
                         out=p, xpart=None)
    for i in range(2):
        tcn.dil[i] = i + 1
        tcn.wt[i] = p
        tcn.bt[i] = p
    return {'tamgcn_f2v_e': gcn, 'tamgcn_f2v_gcn': gcn, 'tamgcn_f2v_gemm': gemm, 'tamgcn_f2v_tcn': tcn}


@pytest.mark.parametrize('name', ['tamgcn_f2v_e', 'tamgcn_f2v_gcn', 'tamgcn_f2v_gemm', 'tamgcn_f2v_tcn'])
def test_entry_points_check_their_arguments_before_any_hip_call(name):
    """No GPU here: a call that got past its checks would fail in the launch (-2) with another message."""
    lib = _lib.load()
    fn = getattr(lib, name)

    def refused(d, what):
        assert fn(C.byref(d), None) == -1
        err = lib.tamgcn_last_error()
        assert err.startswith(name.encode() + b':') and what in err, err
    assert fn(None, None) == -1 and name.encode() in lib.tamgcn_last_error() and b'null' in lib.tamgcn_last_error()
    d = _descs()[name]
    setattr(d, 'h' if name == 'tamgcn_f2v_tcn' else 'x', None)
    refused(d, b'null pointer')
    refused(_descs(V=20)[name], b'V = 25')
    if name == 'tamgcn_f2v_gemm':
        refused(_descs(M_=60)[name], b'M %')
        refused(_descs(K=272)[name], b'K <= 256')
    elif name == 'tamgcn_f2v_tcn':
        d = _descs()[name]
        d.Cout, d.Cb = 96, 24
        refused(d, b'Cb %')
        refused(_descs(K=272)[name], b'Cin=272')
    else:
        refused(_descs(M_=60)[name], b'Cout %')
        refused(_descs(K=272)[name], b'Cin <= 256')


@pytest.mark.parametrize('T', [13, 20])
def test_folded_blocks_equal_the_oracle_at_25_joints_two_persons(T):
    m = M.Model(**NTU).double()
    sd = m.state_dict()
    fill_state_(sd, seed=MODEL_PARAM_SEED)
    with torch.no_grad():                                   # moderate running statistics (seeded ones blow the activations up tenfold per block)
        for k, v in sd.items():
            if k.endswith('running_var'):
                v.mul_(4.0)
    m.eval()
    x = make_input((1, 3, T, 25, 2), seed=5).double()
    h, _, Mp = O._stem(x, sd, 25, False)
    assert Mp == 2 and h.shape[0] == 2
    blocks = f2v.FusedEvalV(m)._packed(torch.device('cpu'))
    for i, blk in enumerate(blocks, 1):
        ref = O.tcn_gcn_unit(h, sd, f'l{i}', O._STRIDES.get(i, 1), residual=(i != 1), training=False)
        with torch.no_grad():
            got = _restate(blk, h)
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), f'l{i}'
        h = ref
