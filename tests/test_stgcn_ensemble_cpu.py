"""CPU: the host side of the grouped small-batch eval pass for ST-GCN ensembles (tam_gcn_amd.f2s.GroupedEvalST,
tam_gcn_amd.inference.StreamEnsemble on models.stgcn.Model): construction, the guards that need no device, the stacking, the
routing bound of tam_gcn_amd.streaming, the ABI checks made before any HIP call, and that the ensemble's seeded models stay
tame.  (The kernels: tests/test_gpu_stgcn_ensemble.py.)"""
import ctypes as C
import os
import re

import pytest
import torch

from cases import MODEL_CASES
from params import make_input
from oracle import stgcn_oracle as SO
from tam_gcn_amd import f2, f2s, streaming, _lib
from tam_gcn_amd.inference import StreamEnsemble
from tam_gcn_amd.models import ctrgcn, stgcn
import stgcn_ensemble_models as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')
UCLA = dict(num_class=10, num_point=20, num_person=1, graph='tam_gcn_amd.graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


def mk(**over):
    return stgcn.Model(**dict(UCLA, **over)).eval()


@pytest.mark.parametrize('G', [2, 4])
def test_an_stgcn_ensemble_constructs(G):
    """(Before GroupedEvalST: AttributeError, 'Model' object has no attribute 'l1'.)"""
    ens = StreamEnsemble([mk() for _ in range(G)], streams=SE.STREAMS[:G])
    assert isinstance(ens._eng, f2s.GroupedEvalST) and len(ens._eng.engines) == G
    assert all(isinstance(e, f2s.FusedEvalST) for e in ens._eng.engines)
    assert (ens._eng.V, ens._eng.M, ens._eng.K, ens._eng.FAMILY) == (20, 1, 10, 'f2s')
    assert not ens.training and ens.modes.tolist() == list(range(G))
    x = make_input((1, 3, 13, 20, 1), seed=1)
    with pytest.raises(RuntimeError, match='no_grad'):
        ens(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU path'):
        ens(x)


def test_constructor_guards():
    two = [mk(), mk()]
    with pytest.raises(ValueError, match='2 models but 4 streams'):
        StreamEnsemble(two)
    with pytest.raises(ValueError, match='2 models but 3 weights'):
        StreamEnsemble(two, streams=('joint', 'bone'), weights=(1, 1, 1))
    with pytest.raises(ValueError, match='model 1 is in train mode'):
        StreamEnsemble([mk(), mk().train()], streams=('joint', 'bone'))
    with pytest.raises(ValueError, match='model 1 differs from model 0 in num_class'):
        StreamEnsemble([mk(), mk(num_class=12)], streams=('joint', 'bone'))
    ntu = dict(num_class=10, num_point=25, graph='tam_gcn_amd.graph.ntu_rgb_d.Graph')
    with pytest.raises(ValueError, match='model 2 differs from model 0 in num_point'):
        StreamEnsemble([mk(), mk(), mk(**ntu)], streams=('joint', 'bone', 'motion'))
    with pytest.raises(ValueError, match='model 1 differs from model 0 in num_person'):
        StreamEnsemble([mk(), mk(num_person=2)], streams=('joint', 'bone'))
    with pytest.raises(ValueError, match='model 1 differs from model 0 in in_channels'):
        StreamEnsemble([mk(), mk(in_channels=2)], streams=('joint', 'bone'))
    two_subsets = mk()
    two_subsets.A = two_subsets.A[:2].clone()
    with pytest.raises(ValueError, match='model 1 differs from model 0 in subsets'):
        StreamEnsemble([mk(), two_subsets], streams=('joint', 'bone'))
    ctr = ctrgcn.Model(**next(c for c in MODEL_CASES if c[0] == 'ucla_t52')[1]).eval()
    for models in ([mk(), ctr], [ctr, mk()]):
        with pytest.raises(ValueError, match='mix of ST-GCN and CTR-GCN'):
            StreamEnsemble(models, streams=('joint', 'bone'))
    with pytest.raises(f2.Unsupported, match='models.stgcn.Model'):
        f2s.GroupedEvalST([ctr, ctr])
    with pytest.raises(ValueError, match='no models'):
        f2s.GroupedEvalST([])


def test_stacking_puts_model_g_at_index_g_and_refuses_a_geometry_change():
    G = 3
    models = [SE.model('ucla', g) for g in range(G)]
    eng = f2s.GroupedEvalST(models)
    per_model = [e._packed(CPU) for e in eng.engines]
    assert eng._restack(per_model) == list(range(G))
    stacked = eng._stacked
    assert len(stacked) == 10
    for i, (params, geom) in enumerate(stacked):
        for g, m in enumerate(models):
            with torch.no_grad():
                b = f2s._BlockST(m.st_gcn_networks[i], m.A * m.edge_importance[i], CPU)       # folded anew, not the engine's
            assert geom == b.geom and len(params) == 7
            for t, src in zip(params, b.params):
                assert t.shape[0] == G and torch.equal(t[g], src)
        assert not torch.equal(params[0][0], params[0][1])          # Ae differs per group: every model has its own edge_importance
    # a re-fold of one model: its slice is rewritten in place, the stacked tensor objects stay
    ids = [[id(t) for t in params] for params, _ in stacked]
    old = stacked[3][0][0].clone()
    with torch.no_grad():
        models[1].edge_importance[3].mul_(1.5)
    per_model2 = [e._packed(CPU) for e in eng.engines]
    assert per_model2[1] is not per_model[1] and per_model2[0] is per_model[0]
    eng._seen = per_model
    assert eng._restack(per_model2) == [1]
    assert eng._stacked is stacked and [[id(t) for t in params] for params, _ in stacked] == ids
    new = stacked[3][0][0]
    assert torch.equal(new[0], old[0]) and torch.equal(new[2], old[2]) and not torch.equal(new[1], old[1])
    assert torch.equal(new[1], models[1].A * models[1].edge_importance[3])
    # a geometry change after the stacking is refused, naming the block
    blk = models[2].st_gcn_networks[6]
    models[2].st_gcn_networks[6] = stgcn.st_gcn(blk.in_channels, blk.out_channels, (9, 3), 2).eval()
    with pytest.raises(ValueError, match='model 2 no longer has the geometry of its group in st_gcn block 7'):
        eng._restack([e._packed(CPU) for e in eng.engines])
    # differing block geometry at the first stacking: f2.stack_blocks names the field
    a = f2s.FusedEvalST(SE.model('ucla', 0))._packed(CPU)
    b = f2s.FusedEvalST(SE.model('ucla', 1))._packed(CPU)
    b[4].geom = [3, 9, 1, 2]
    with pytest.raises(ValueError, match=r'model 1 differs from model 0 in st_gcn block 5\.geom'):
        f2.stack_blocks([a, b], f2s.GroupedEvalST.LABEL)


def test_family_batch_counts_the_groups(monkeypatch):
    monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', 1024)
    one = mk()
    assert streaming._family_batch(one, 52, 20, 1) == 1024 // 52
    for G in (2, 4):
        ens = StreamEnsemble([mk() for _ in range(G)], streams=SE.STREAMS[:G])
        assert streaming._family_batch(ens, 52, 20, 1) == 1024 // (G * 52)
        assert streaming._family_batch(ens, 20, 20, 2) == 1024 // (G * 2 * 20)
    assert streaming._family_batch(StreamEnsemble([mk() for _ in range(4)]), 300, 20, 1) == 1     # never below one window


@pytest.mark.parametrize('name, shape', [('ucla', (2, 3, 13, 20, 1)), ('coco', (1, 3, 9, 17, 1)), ('tree7', (2, 2, 8, 7, 1))])
def test_seeded_models_stay_tame(name, shape):
    """fill_stgcn_(state, seed=42 + g): every group's fp64 logits (oracle/stgcn_oracle.py) are finite and within 10x of group 0's
    in max|.|, so one absolute bar serves all groups."""
    x = make_input(shape, seed=21).double()
    a = []
    for g in range(4):
        m = SE.model(name, g)
        y = SO.model_forward(x, SE.sd64(m), m.num_point, training=False)
        assert bool(torch.isfinite(y).all())
        a.append(float(y.abs().max()))
    print(name, a)
    for g in range(1, 4):
        assert a[0] / 10 <= a[g] <= a[0] * 10, (g, a)


NEW = ['tamgcn_f2s_gcn_grouped', 'tamgcn_f2s_tcn_grouped']


def test_header_declares_the_new_entry_points_and_the_version_stays():
    src = open(os.path.join(ROOT, 'include', 'tamgcn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(tamgcn_[a-z0-9_]+)\s*\(', src))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert '#define TAMGCN_VERSION 401' in src and _lib.ABI_VERSION == 401


def _desc(stage, N=4, **over):
    p = 1 << 20
    if stage == 'gcn':
        return _lib.F2sGcnDesc(**dict(dict(N=N, Cin=64, Cout=64, T=8, V=20, K=3, x=p, Ae=p, wg=p, bg=p, h=p), **over))
    return _lib.F2sTcnDesc(**dict(dict(N=N, Cin=64, Cout=128, T=8, V=20, KT=9, stride=2, res_mode=2, h=p, wt=p, bt=p, x=p, wr=p, br=p, out=p), **over))


@pytest.mark.parametrize('stage', ['gcn', 'tcn'])
def test_grouped_entry_points_check_their_arguments_before_any_hip_call(stage):
    """No GPU here: a call that got past its checks would fail in the launch (-2) with another message."""
    lib = _lib.load()
    name = f'tamgcn_f2s_{stage}_grouped'
    fn = getattr(lib, name)

    def refused(d, groups, what):
        assert fn(None if d is None else C.byref(d), groups, None) == -1
        err = lib.tamgcn_last_error()
        assert err.startswith(name.encode() + b':') and what in err, err
    refused(_desc(stage), 3, b'N=4 is not a multiple of groups=3')
    refused(_desc(stage), 0, b'groups=0')
    refused(_desc(stage), -2, b'groups=-2')
    refused(_desc(stage, N=2), 4, b'N=2 is not a multiple of groups=4')
    refused(_desc(stage, N=65536), 2, b'bad dims N=65536')                      # the grid's z is the TOTAL sample
    refused(_desc(stage, N=65532, T=64), 4, b'2^31 elements')                   # ... and so is the element bound
    refused(_desc(stage, V=33), 2, b'V=33')                                     # the plain entry point's checks hold here too
    refused(None, 2, b'null descriptor')
    # the group stride of a weight array read in 16-byte pieces: unreachable through the geometry checks (Cin % 4 == 0 and
    # Cout % 16 == 0 make every stride a multiple of four floats), so no descriptor gets there; Cin = 3 takes the 4-byte path
    if stage == 'gcn':
        assert fn(C.byref(_desc(stage, Cin=3)), 2, None) != -1 or b'group stride' not in lib.tamgcn_last_error()


def test_the_grouped_operator_refuses_cpu_tensors():
    b = f2s.FusedEvalST(SE.model('ucla', 0))._packed(CPU)[1]
    with pytest.raises(RuntimeError, match='no CPU path'):
        torch.ops.tamgcn.st_gcn_eval_grouped(torch.zeros(2, 64, 8, 20), [torch.stack([t, t]) for t in b.params], b.geom, 2)
