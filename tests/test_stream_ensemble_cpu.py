"""CPU: the host side of the grouped small-batch eval pass (tam_gcn_amd.f2.GroupedEval / stack_blocks,
tam_gcn_amd.inference.StreamEnsemble): stacking, the grouped contract of include/tamgcn.h restated in plain torch, the stream
derivations, the default bone table, the guards that need no device, and the ABI.  (The kernels: tests/test_gpu_stream_ensemble.py.)"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cases import MODEL_CASES
from params import make_input
from tam_gcn_amd import f2, f2v, _lib
from tam_gcn_amd.feeder.feeder_nucla_gcn import BONE_PARENT
from tam_gcn_amd.inference import StreamEnsemble, default_parent
from tam_gcn_amd.models import ctrgcn as M
from oracle import feeder_oracle as FO
import stream_ensemble_models as SM
from test_f2_cpu import _restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')
NTU = next(c for c in MODEL_CASES if c[0] == 'ntu_t20')[1]
UCLA = next(c for c in MODEL_CASES if c[0] == 'ucla_t52')[1]


@pytest.mark.parametrize('tag, shape', [('ucla_t52', (2, 3, 13, 20, 1)), ('ntu_t20', (1, 3, 20, 25, 2))])
def test_perturbed_models_stay_tame(tag, shape):
    """The ensemble's models (stream_ensemble_models.perturbed_model, EPS = 0.02): max|activation| after l10 within 10x of
    the unperturbed model's, fp64 oracle.  Measured 0.83x .. 1.26x."""
    x = make_input(shape, seed=21)
    a0 = SM.l10_absmax(SM.base_model(tag).eval(), x)
    for g in range(4):
        a = SM.l10_absmax(SM.perturbed_model(tag, g).eval(), x)
        assert a0 / 10 <= a <= a0 * 10, (g, a, a0)


def _restate_grouped(stacked, geom, x, groups):
    """The grouped contract: sample n runs the block with the stacked parameters indexed by n // (N / groups)."""
    npg = x.shape[0] // groups
    outs = []
    for n in range(x.shape[0]):
        b = SimpleNamespace(params=[t[n // npg] for t in stacked], geom=geom)
        outs.append(_restate(b, x[n:n + 1]))
    return torch.cat(outs)


def test_stacking_and_the_grouped_contract():
    G, n = 3, 2
    models = [SM.perturbed_model('ucla_t52', g).double().eval() for g in range(G)]
    per_model = [f2.FusedEval(m)._packed(CPU) for m in models]
    stacked = f2.stack_blocks(per_model)
    assert len(stacked) == 10
    x = make_input((G * n, 3, 13, 20), seed=4).double()
    for i, (params, geom) in enumerate(stacked):
        for g in range(G):
            b = per_model[g][i]
            assert geom == b.geom and len(params) == len(b.params)
            for t, src in zip(params, b.params):
                assert t.shape[0] == G and torch.equal(t[g], src)
        with torch.no_grad():
            got = _restate_grouped(params, geom, x, G)
            ref = torch.cat([_restate(per_model[g][i], x[g * n:(g + 1) * n]) for g in range(G)])
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), f'l{i + 1}'
        assert float((got[:n] - _restate(per_model[1][i], x[:n])).abs().max()) > 0      # the groups really differ
        x = ref


def test_stack_blocks_names_the_first_differing_field():
    a = f2.FusedEval(M.Model(**UCLA).eval())._packed(CPU)
    b = f2v.FusedEvalV(M.Model(**NTU).eval())._packed(CPU)
    b[4].geom = list(b[4].geom)
    b[4].geom[5] = 1                                        # l5 without its stride
    with pytest.raises(ValueError, match=r'model 1 differs from model 0 in l5\.geom'):
        f2.stack_blocks([f2v.FusedEvalV(M.Model(**NTU).eval())._packed(CPU), b])
    with pytest.raises(ValueError, match='parameter shapes of l1'):
        f2.stack_blocks([a, f2v.FusedEvalV(M.Model(**NTU).eval())._packed(CPU)])      # PA is (3, 20, 20) against (3, 25, 25)


def test_stream_derivations_agree_with_the_feeder_oracle():
    """A feeder-shaped sample: the oracle's bone / motion / bone_motion of a clip against the restatement applied to the
    oracle's joint stream (fp32 after the fp64 transform: one rounding of values in [-1, 1] per operand)."""
    r = np.random.RandomState(3)
    value = r.standard_normal((37, 20, 3))
    idx = FO.val_indices(37, 52)
    joint = torch.from_numpy(FO.transform(value, 0, 0, 1.0, idx, 'joint'))[None]
    for stream in ('bone', 'motion', 'bone_motion'):
        ref = torch.from_numpy(FO.transform(value, 0, 0, 1.0, idx, stream))[None]
        got = SM.derive(joint, BONE_PARENT, stream)
        assert float((got - ref).abs().max()) <= 4 * 2.0 ** -23, stream
    assert torch.equal(SM.derive(joint, BONE_PARENT, 'joint'), joint)
    assert float(SM.derive(joint, BONE_PARENT, 'motion')[:, :, -1].abs().max()) == 0


def test_default_parent_of_both_graphs():
    for margs, V, root in ((UCLA, 20, 2), (NTU, 25, 20)):
        p = default_parent(M.Model(**margs).graph)
        assert len(p) == V and all(0 <= q < V for q in p)
        assert [v for v in range(V) if p[v] == v] == [root]
    assert tuple(default_parent(M.Model(**UCLA).graph)) == BONE_PARENT       # the reference N-UCLA feeder's bone table


def test_constructor_guards():
    mk = lambda margs=UCLA, **over: M.Model(**dict(margs, **over)).eval()
    two = [mk(), mk()]
    with pytest.raises(ValueError, match='2 models but 4 streams'):
        StreamEnsemble(two)
    with pytest.raises(ValueError, match='unknown stream'):
        StreamEnsemble(two, streams=('joint', 'velocity'))
    with pytest.raises(ValueError, match='2 models but 3 weights'):
        StreamEnsemble(two, streams=('joint', 'bone'), weights=(1, 1, 1))
    with pytest.raises(ValueError, match='model 1 is in train mode'):
        StreamEnsemble([mk(), mk().train()], streams=('joint', 'bone'))
    with pytest.raises(ValueError, match='model 1 differs from model 0 in num_class'):
        StreamEnsemble([mk(), mk(num_class=12)], streams=('joint', 'bone'))
    with pytest.raises(ValueError, match='model 2 differs from model 0 in num_point'):
        StreamEnsemble([mk(), mk(), mk(NTU)], streams=('joint', 'bone', 'motion'))
    with pytest.raises(ValueError, match='model 1 differs from model 0 in num_person'):
        StreamEnsemble([mk(), mk(num_person=2)], streams=('joint', 'bone'))
    with pytest.raises(ValueError, match='parent'):
        StreamEnsemble(two, streams=('joint', 'bone'), parent=list(range(19)) + [20])
    ens = StreamEnsemble(two, streams=('joint', 'bone_motion'), weights=(0.6, 0.4))
    assert not ens.training and ens.parent.dtype == torch.int32 and ens.parent.tolist() == list(BONE_PARENT)
    assert ens.modes.tolist() == [0, 3] and ens.weights.tolist() == [pytest.approx(0.6), pytest.approx(0.4)]
    x = make_input((1, 3, 13, 20, 1), seed=1)
    with pytest.raises(RuntimeError, match='no_grad'):
        ens(x)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU path'):
            ens(x)
        with pytest.raises(RuntimeError, match='no CPU path'):
            b = ens._eng.engines[0]._packed(CPU)[1]
            torch.ops.tamgcn.tcn_gcn_unit_eval_grouped(torch.zeros(2, 64, 8, 20), None, [torch.stack([t, t]) for t in b.params], b.geom, 2)


NEW = ['tamgcn_f2_e_grouped', 'tamgcn_f2_gcn_grouped', 'tamgcn_f2_gemm_grouped', 'tamgcn_f2_tcn_grouped',
       'tamgcn_f2v_e_grouped', 'tamgcn_f2v_gcn_grouped', 'tamgcn_f2v_gemm_grouped', 'tamgcn_f2v_tcn_grouped',
       'tamgcn_stem_streams_eval', 'tamgcn_head_fc_grouped']


def test_header_declares_the_new_entry_points_and_the_version_stays():
    src = open(os.path.join(ROOT, 'include', 'tamgcn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(tamgcn_[a-z0-9_]+)\s*\(', src))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert '#define TAMGCN_VERSION 401' in src and _lib.ABI_VERSION == 401


def _descs(V, N=4):
    p = 1 << 20
    gcn = _lib.F2GcnDesc(N=N, Cin=64, Cout=64, T=8, V=V, S=3, R=8, res_mode=0, x=p, w12=p, b12=p, w4=p, b4=p, A=p, alpha=p, w3=p, b3=p,
                         sy=p, ty=p, wd=None, bd=None, E=p, sum=p, diff=p, xpart=None)
    gemm = _lib.F2GemmDesc(N=N, K=64, M=64, T=8, V=V, mode=1, relu_rows=0, x=p, w=p, b=p, add=None, out=p)
    tcn = _lib.F2TcnDesc(N=N, Cin=64, Cout=64, T=8, V=V, stride=2, Cb=16, nb=2, ks=5, res_mode=2, h=p, sp=p, tp=p, x=p, wr=p, br=p,
                         out=p, xpart=None)
    for i in range(2):
        tcn.dil[i] = i + 1
        tcn.wt[i] = p
        tcn.bt[i] = p
    return {'e': gcn, 'gcn': gcn, 'gemm': gemm, 'tcn': tcn}


@pytest.mark.parametrize('name', NEW[:8])
def test_grouped_entry_points_check_their_arguments_before_any_hip_call(name):
    """No GPU here: a call that got past its checks would fail in the launch (-2) with another message."""
    lib = _lib.load()
    fn = getattr(lib, name)
    fam, stage = name.split('_')[1], name.split('_')[2]
    V = 20 if fam == 'f2' else 25

    def refused(d, groups, what):
        assert fn(C.byref(d), groups, None) == -1
        err = lib.tamgcn_last_error()
        assert err.startswith(name.encode() + b':') and what in err, err
    refused(_descs(V)[stage], 3, b'N=4 is not a multiple of groups=3')
    refused(_descs(V)[stage], 0, b'groups=0')
    refused(_descs(V, N=2)[stage], 4, b'N=2 is not a multiple of groups=4')
    refused(_descs(45 - V)[stage], 2, b'V = %d' % V)       # the plain entry point's checks hold here too
    assert fn(None, 2, None) == -1 and b'null' in lib.tamgcn_last_error()


def test_stem_and_head_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    p = 1 << 20
    assert lib.tamgcn_stem_streams_eval(p, p, None, p, 4, 1, 3, 8, 20, 1, p, None) == -1 and b'tamgcn_stem_streams_eval' in lib.tamgcn_last_error()
    assert lib.tamgcn_stem_streams_eval(p, p, p, p, 0, 1, 3, 8, 20, 1, p, None) == -1
    assert lib.tamgcn_stem_streams_eval(p, p, p, p, 4, 1, 3, 1 << 18, 20, 1, p, None) == -1 and b'2^20' in lib.tamgcn_last_error()
    assert lib.tamgcn_head_fc_grouped(p, None, p, 4, 1, 256, 10, p, None) == -1 and b'tamgcn_head_fc_grouped' in lib.tamgcn_last_error()
    assert lib.tamgcn_head_fc_grouped(p, p, p, 0, 1, 256, 10, p, None) == -1
