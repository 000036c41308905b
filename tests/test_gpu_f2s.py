"""-m gpu: the ST-GCN small-batch eval family (csrc/f2s.hip; tam_gcn_amd/f2s.py: FusedEvalST, tamgcn::st_gcn_eval) through whole
models: against the fp64 oracle (oracle/stgcn_oracle.py on a .double() state, fill_stgcn_ parameters) at the project's ST-GCN
bar -- logits within 1e-3 absolute, same arg max -- and against the general eval path's own error on the same input (the
family's max error at most 4 x the general path's: both are exact fp32 and differ in summation order only, which moves an
error by small factors; a wrong term moves it by orders of magnitude).  Then routing, re-fold, graph replay, launch count, the
registered operator and CapturedEval.  `pytest -s` prints both errors per shape."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from params import make_input                                                     # noqa: E402
from oracle import stgcn_oracle as SO                                               # noqa: E402
from oracle import ctrgcn_oracle as CO                                              # noqa: E402
from tam_gcn_amd import f2, f2s, _lib                                               # noqa: E402
from tam_gcn_amd.evaluation import CapturedEval, EvalMeter                          # noqa: E402
from tam_gcn_amd.inference import GraphedForward                                    # noqa: E402
from tam_gcn_amd.models import stgcn as M                                           # noqa: E402
from test_stgcn_oracle import fill_stgcn_                                           # noqa: E402
from test_gpu_f2j import Count, _counted, _general, _rel                            # noqa: E402

DEV = 'cuda:0'
SP = dict(labeling_mode='spatial')
MODELS = {
    'ucla': dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=SP),
    'openpose': dict(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=SP),
    'coco': dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=SP),
    'ntu': dict(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=SP),
    'tree7': dict(in_channels=2, num_class=6, num_point=7, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph',
                  graph_args=dict(num_node=7, arity=2)),
}
SHAPES = [('ucla', (2, 3, 13, 20, 1)), ('openpose', (1, 3, 20, 18, 2)), ('coco', (1, 3, 9, 17, 1)), ('ntu', (1, 3, 12, 25, 2)),
          ('tree7', (2, 2, 8, 7, 1)), ('ucla', (2, 13, 60))]
BOUND = 1024                   # the routing tests set the bound themselves: they test the routing, not the measured value


@pytest.fixture(autouse=True)
def _bound(monkeypatch):
    monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', BOUND)
    monkeypatch.setenv('TAMGCN_F2', '1')


@functools.lru_cache(maxsize=None)
def _state(name):
    m = M.Model(**MODELS[name])
    fill_stgcn_(m.state_dict(), seed=42)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(name, **kw):
    m = M.Model(**dict(MODELS[name], **kw))
    m.load_state_dict(_state(name))
    return m.to(DEV).eval()


def _sd64(m):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}


def _oracle(x, sd, V):
    """(logits, extract_feature output, feature) of stgcn_oracle in eval mode.  Its stem (the reference's view(N*M, V*C, T)) takes
    ONE person per BatchNorm channel set; the mirror model's data_bn spans (person, joint, channel) as CTR-GCN's does, so for
    two-person inputs the stem is ctrgcn_oracle._stem (that arrangement) and everything behind it -- the ten st_gcn blocks, the
    pooling, fcn -- is stgcn_oracle's own code.  With one person this IS stgcn_oracle.model_forward / model_extract_feature."""
    h, N, M = CO._stem(x, sd, V, False)
    for i, (_, stride, res) in enumerate(SO.PLAN):
        h = SO.st_gcn(h, sd, f'st_gcn_networks.{i}', sd['A'] * sd[f'edge_importance.{i}'], stride, res, False)
    _, c, t, v = h.size()
    feature = h.view(N, M, c, t, v).permute(0, 2, 3, 4, 1)
    o = torch.nn.functional.conv2d(h, sd['fcn.weight'], sd['fcn.bias'])
    out = o.view(N, M, -1, t, v).permute(0, 2, 3, 4, 1)
    p = torch.nn.functional.avg_pool2d(h, h.size()[2:]).view(N, M, -1, 1, 1).mean(dim=1)
    logits = torch.nn.functional.conv2d(p, sd['fcn.weight'], sd['fcn.bias'])
    logits = logits.view(logits.size(0), -1)
    if M == 1:
        assert torch.equal(logits, SO.model_forward(x, sd, V, training=False))
        ro, rf = SO.model_extract_feature(x, sd, V, training=False)
        assert torch.equal(out, ro) and torch.equal(feature, rf)
    return logits, out, feature


def _bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _spy(monkeypatch):
    calls = []
    real = f2s.FusedEvalST.blocks
    monkeypatch.setattr(f2s.FusedEvalST, 'blocks', lambda self, x: (calls.append(1), real(self, x))[1])
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# whole models against the fp64 oracle, and the family's error against the general path's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, shape', SHAPES, ids=[f'{n}_{"x".join(map(str, s))}' for n, s in SHAPES])
def test_model_against_the_fp64_oracle_and_the_general_path(name, shape, monkeypatch):
    m = _model(name)
    V = MODELS[name]['num_point']
    x = make_input(shape, seed=21)
    sd64 = _sd64(m)
    ref, ro, rf = _oracle(x.double(), sd64, V)
    calls = _spy(monkeypatch)
    xd = x.to(DEV)
    with torch.no_grad():
        with _general():
            g = m(xd).double().cpu()
            go, gf = (t.double().cpu() for t in m.extract_feature(xd))
        assert not calls and not m.__dict__.get('_tamgcn_f2s'), 'TAMGCN_F2=0 is the general eval path'
        a = m(xd).double().cpu()
        ao, af = (t.double().cpu() for t in m.extract_feature(xd))
    assert len(calls) == 2 and isinstance(m.__dict__.get('_tamgcn_f2s'), f2s.FusedEvalST)
    err_f, err_g = float((a - ref).abs().max()), float((g - ref).abs().max())
    ef_feat, eg_feat = float((af - rf).abs().max()), float((gf - rf).abs().max())
    ef_out, eg_out = float((ao - ro).abs().max()), float((go - ro).abs().max())
    print(f'\n{name} {shape}: logits max|err| family {err_f:.3e}  general {err_g:.3e} (max|ref| {float(ref.abs().max()):.3e});  '
          f'features family {ef_feat:.3e}  general {eg_feat:.3e} (max|ref| {float(rf.abs().max()):.3e});  '
          f'extract_feature output family {ef_out:.3e}  general {eg_out:.3e}')
    assert a.shape == ref.shape and af.shape == rf.shape and ao.shape == ro.shape
    assert err_f <= 1e-3 and torch.equal(a.argmax(1), ref.argmax(1))
    assert err_g <= 1e-3
    assert err_f <= 4 * err_g
    assert ef_feat <= 4 * eg_feat and ef_out <= 4 * eg_out


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
def test_model_forward_routes_small_eval_batches_here(monkeypatch):
    m = _model('openpose')
    V, P = 18, 2
    x = make_input((1, 3, 16, V, P), seed=2).to(DEV)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        m(x)
        m.extract_feature(x)
        assert len(calls) == 2 and m._f2s(x) is not None
        T = 8
        big = make_input((BOUND // (P * T) + 1, 3, T, V, P), seed=3).to(DEV)
        assert m._f2s(big[:-1]) is not None and m._f2s(big) is None
        m(big)                                              # one clip over the bound (clip-persons x frames): general path
        assert len(calls) == 2
        monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', 0)       # bound 0: the family is opt-in only
        m(x)
        assert len(calls) == 2
        monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', BOUND)
        monkeypatch.setenv('TAMGCN_F2', '0')
        m(x)
        assert len(calls) == 2
        monkeypatch.setenv('TAMGCN_F2', '1')
        h = m.st_gcn_networks[3].register_forward_hook(lambda mod, i, o: None)
        m(x)                                                # a forward hook would not fire inside the engine
        assert len(calls) == 2
        h.remove()
        m(x)
        assert len(calls) == 3
    m(x)                                                    # grad mode: general path (autograd)
    assert len(calls) == 3
    m.train()
    with torch.no_grad():
        m(x)
    assert len(calls) == 3


def test_a_kt5_model_takes_the_general_path_without_error(monkeypatch):
    m = _model('ucla')
    blk = M.st_gcn(64, 64, (5, 3), 1)
    torch.manual_seed(0)
    m.st_gcn_networks[2] = blk.to(DEV).eval()
    x = make_input((1, 3, 12, 20, 1), seed=2).to(DEV)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        y, cnt = _counted(lambda: m(x))
        assert m.__dict__.get('_tamgcn_f2s') is False and not calls
        assert not any(n in ('tamgcn_f2s_gcn', 'tamgcn_f2s_tcn') for n in cnt.names)
        with _general():
            assert torch.equal(m(x), y)
    with pytest.raises(f2.Unsupported):
        f2s.FusedEvalST(m)._packed(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# re-fold
# ---------------------------------------------------------------------------------------------------------------------
def _pair(m, x):
    """family and general path on the same state: equal to rounding (both exact fp32: 2e-5 relative, the families' bar)"""
    with torch.no_grad():
        a = m(x)
        with _general():
            b = m(x)
    assert _rel(a, b) <= 2e-5, _rel(a, b)
    return a


def test_refolds_after_every_kind_of_state_change():
    m = _model('coco')
    x = make_input((1, 3, 20, 17, 1), seed=21).to(DEV)
    a0 = _pair(m, x)
    assert m.__dict__.get('_tamgcn_f2s')
    with torch.no_grad():
        m.edge_importance[3].mul_(1.3)                       # in place
        m.st_gcn_networks[6].tcn[2].bias.add_(0.3)
    a1 = _pair(m, x)
    assert float((a1 - a0).abs().max()) > 0
    m2 = _model('coco')
    with torch.no_grad():
        for p in m2.parameters():
            p.mul_(0.9)
    m.load_state_dict(m2.state_dict())
    a2 = _pair(m, x)
    assert float((a2 - a1).abs().max()) > 1e-3 * float(a1.abs().max())
    m.train()                                               # a train-mode forward rewrites the running statistics
    with torch.no_grad():
        m(make_input((4, 3, 12, 17, 1), seed=8).to(DEV) * 1.5)
    m.eval()
    a3 = _pair(m, x)
    assert float((a3 - a2).abs().max()) > 0


def test_refolds_after_a_flat_arena_step():
    from tam_gcn_amd.distributed import ParamArena, SGDNesterov
    m = _model('coco')
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    opt = SGDNesterov(arena.params, lr=0.05, momentum=0.9, weight_decay=1e-4, arena=arena, bucket=bucket)
    x = make_input((1, 3, 20, 17, 1), seed=21).to(DEV)
    a0 = _pair(m, x)
    g = torch.Generator().manual_seed(3)
    for p in arena.params:
        p.grad = (torch.randn(p.shape, generator=g) * p.detach().abs().mean().cpu()).to(DEV)
    bucket.pack()
    opt.step()
    a1 = _pair(m, x)
    assert float((a1 - a0).abs().max()) > 1e-3 * float(a0.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# graph replay, launch count, the operator, CapturedEval
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_and_launch_count():
    """Replay = eager bit for bit, two eager runs are bit-equal, the capture keeps the engine's folded weights alive; TWO family
    launches per block -- exactly 20 per forward -- and at most 6 other ABI launches (the allowance of the CTR-GCN families)."""
    m = _model('openpose')
    V, P = 18, 2
    fast = GraphedForward(m)
    for shape in ((1, 3, 13, V, P), (2, 3, 20, V, P)):
        x = make_input(shape, seed=shape[2]).to(DEV)
        with torch.no_grad():
            ref = m(x)
            assert torch.equal(m(x), ref)
        assert torch.equal(fast(x).clone(), ref)
        assert torch.equal(fast(x).clone(), ref)
    eng = m.__dict__['_tamgcn_f2s']
    assert all(any(k is eng._blocks for k in ent[3]) for ent in fast._graphs.values())
    _, cnt = _counted(lambda: m(make_input((1, 3, 20, V, P), seed=9).to(DEV)))
    fam = [n for n in cnt.names if n.startswith('tamgcn_f2s_')]
    assert fam == ['tamgcn_f2s_gcn', 'tamgcn_f2s_tcn'] * 10, fam
    assert cnt.n - len(fam) <= 6, cnt.names


def test_block_is_a_registered_operator():
    m = _model('ucla')
    eng = f2s.FusedEvalST(m)
    blocks = eng._packed(torch.device(DEV))
    for i, cin in ((0, 3), (2, 64), (4, 64), (8, 256)):
        b = blocks[i]
        x = make_input((2, cin, 11, 20), seed=3 + i).to(DEV)
        want = eng._block(b, x)
        got = torch.ops.tamgcn.st_gcn_eval(x, b.params, b.geom)
        assert got.shape == (2, b.Cout, (11 - 1) // b.stride + 1, 20) and torch.equal(got, want)
        torch.library.opcheck(torch.ops.tamgcn.st_gcn_eval.default, (x, b.params, b.geom), test_utils=('test_schema', 'test_faketensor'))
    with pytest.raises(RuntimeError, match='no CPU path'):
        torch.ops.tamgcn.st_gcn_eval(torch.zeros(1, 3, 8, 20), blocks[0].params, blocks[0].geom)
    with pytest.raises(RuntimeError, match='outside the f2s kernels'):
        torch.ops.tamgcn.st_gcn_eval(torch.zeros(1, 3, 8, 20, device=DEV), blocks[0].params, [3, 5, 1, 0])


def test_captured_eval_routes_a_four_clip_batch_through_the_family(monkeypatch):
    """CapturedEval takes an ST-GCN model as it is (it asks a model for nothing beyond forward): metrics and scores of a captured
    pass over 4-clip batches equal those of the eager EvalMeter loop, bit for bit, and the forward it captured is the family's."""
    m = _model('ucla')
    B, n, K = 4, 10, 10
    xs = make_input((12, 3, 16, 20, 1), seed=4).to(DEV)
    ys = torch.arange(12, device=DEV) % K
    calls = _spy(monkeypatch)
    ev = CapturedEval(m, None, B, example_x=xs[:B], num_samples=n)
    assert calls, 'the captured forward did not take the family'
    ev.reset()
    eager = EvalMeter(K, n, device=DEV)
    for b in range(0, n, B):
        valid = min(B, n - b)
        ev.update(xs[b:b + B], ys[b:b + B], valid=valid)
        with torch.no_grad():
            eager.update(m(xs[b:b + B]), ys[b:b + B], valid=valid)
    for k, t in ev.meter.state().items():
        assert torch.equal(_bits(t), _bits(eager.state()[k])), k
    got, want = ev.meter.compute(), eager.compute()
    assert got['count'] == n and got['top1'] == want['top1'] and got['loss'] == want['loss']
