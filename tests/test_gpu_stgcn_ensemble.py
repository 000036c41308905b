"""-m gpu: a multi-stream ST-GCN ensemble as one grouped small-batch eval pass -- the grouped entry points of the f2s family
(tamgcn_f2s_gcn_grouped, tamgcn_f2s_tcn_grouped), the operator tamgcn::st_gcn_eval_grouped, f2s.GroupedEvalST and
inference.StreamEnsemble on models.stgcn.Model, and the callers that take such an ensemble.

The models: tests/stgcn_ensemble_models.py (test_gpu_f2s.py's MODELS, fill_stgcn_(state, seed=42 + g) for group g: every tensor
differs between the groups, edge_importance included; max|logits| of the four groups, fp64: 6.9 / 4.1 / 12.3 / 7.1 at 20 joints,
13.1 / 7.8 / 14.1 / 5.9 at 25 -- tests/test_stgcn_ensemble_cpu.py::test_seeded_models_stay_tame).

Bars.  Grouped against single kernels, the ensemble against its parts, the arrangements, graph replay: bit equality.  Against
the fp64 oracle (test_gpu_f2s.py::_oracle on streams derived in fp64): each group's scores within 1e-3 absolute (the project's
ST-GCN bar, test_gpu_f2s.py), the raw-fused scores within sum_g |w_g| 1e-3 (triangle inequality), pred = the fp64 arg max with
input seed 1: at both shapes and both weight sets every sample's fp64 top-2 margin of the fused reference (20 joints: 9.996 /
3.843, 25 joints: 0.2406 / 2.247 for weights (1, 1, 1, 1) / (0.6, 0.6, 0.4, 0.4)) exceeds twice that bar (0.008 / 0.004) --
searched on the CPU from seed 1 upwards, the first one holds.  The general path against the grouped one: 2e-5 max|.| (the
project's bar between the family and the general path).

The group-stride alignment check of the grouped entry points has no test: no descriptor reaches it.  A launch reads wg / wr
in 16-byte pieces only when Cin % 4 == 0 and wt always with Cout % 16 == 0, and then every group stride (K Cout Cin, Cout Cin,
9 Cout Cout) is a multiple of four floats."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from params import make_input                                                      # noqa: E402
from tam_gcn_amd import f2s, ops, ensemble, _lib                                    # noqa: E402
from tam_gcn_amd.inference import GraphedForward, StreamEnsemble, default_parent   # noqa: E402
from tam_gcn_amd.streaming import FrameRing, LiveClassifier, SlidingWindow         # noqa: E402
import f2s_ref                                                                     # noqa: E402
import stgcn_ensemble_models as SE                                                 # noqa: E402
import stream_ensemble_models as SM                                                # noqa: E402
from test_gpu_f2s import _oracle                                                   # noqa: E402
from test_gpu_stream_ensemble import _counted                                      # noqa: E402

DEV = 'cuda:0'
STREAMS = SE.STREAMS
SHAPES = [('ucla', (2, 3, 13, 20, 1)), ('ntu', (1, 3, 12, 25, 2)), ('openpose', (1, 3, 20, 18, 2))]
WEIGHTS = [(1, 1, 1, 1), (0.6, 0.6, 0.4, 0.4)]
X_SEED = 1
BAR = 1e-3                     # the project's ST-GCN logits bar against fp64 (test_gpu_f2s.py)
BOUND = 1024                   # the routing tests set the bound themselves: they test the routing, not the measured value


@pytest.fixture(autouse=True)
def _bound(monkeypatch):
    monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', BOUND)
    monkeypatch.setenv('TAMGCN_F2', '1')


@functools.lru_cache(maxsize=None)
def _models(name):
    return tuple(SE.model(name, g).to(DEV) for g in range(4))


@functools.lru_cache(maxsize=None)
def _blocks(name):
    return tuple(f2s.FusedEvalST(m)._packed(torch.device(DEV)) for m in _models(name))


@functools.lru_cache(maxsize=None)
def _engine(name, g):
    return f2s.FusedEvalST(_models(name)[g])


@functools.lru_cache(maxsize=None)
def _shared_ens(name):
    return StreamEnsemble(_models(name), STREAMS)


def _ens(name, weights=WEIGHTS[0], softmax=False):
    """One ensemble per model set on the shared (never modified) models; its weights live in a device tensor."""
    ens = _shared_ens(name)
    ens.weights.copy_(torch.tensor(weights, dtype=torch.float32))
    ens.softmax = softmax
    return ens


def _parent(name):
    return torch.tensor(default_parent(_models(name)[0].graph), dtype=torch.int32, device=DEV)


def _stack(per_group):
    return [torch.stack(ts) for ts in zip(*per_group)]


def _grouped_n(names):
    return sum(n.startswith('tamgcn_f2s_') and n.endswith('_grouped') for n in names)


single, grouped = torch.ops.tamgcn.st_gcn_eval, torch.ops.tamgcn.st_gcn_eval_grouped


# ---- 1: the block ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [13, 9])
@pytest.mark.parametrize('name', ['tree7', 'coco', 'ucla', 'ntu'], ids=['v7_c2', 'v17', 'v20', 'v25'])
def test_grouped_block_equals_the_single_block_bit_for_bit(name, T):
    """Every block down the depth (T 13 -> 7 -> 4, 9 -> 5 -> 3: partial last tiles, odd T under stride 2, a tile larger than T),
    groups 2 and 4, 1 and 2 samples per group: group g's slice of the grouped operator equals the single operator on model g's
    _BlockST; two grouped runs are equal; group 1's parameters on group 0's samples give something else."""
    blocks = _blocks(name)
    V = SE.MODELS[name]['num_point']
    Tin = T
    for i in range(10):
        b0 = blocks[0][i]
        for G in (2, 4):
            params = _stack([blocks[g][i].params for g in range(G)])
            for n in (1, 2):
                x = make_input((G * n, b0.Cin, Tin, V), seed=100 * i + 10 * G + n).to(DEV)
                out = grouped(x, params, b0.geom, G)
                assert torch.equal(out, grouped(x, params, b0.geom, G)), f'block {i} G={G} n={n}: two runs differ'
                assert tuple(out.shape) == (G * n, b0.Cout, (Tin - 1) // b0.stride + 1, V) and bool(torch.isfinite(out).all())
                for g in range(G):
                    sl = slice(g * n, (g + 1) * n)
                    b = blocks[g][i]
                    assert torch.equal(out[sl], single(x[sl].contiguous(), b.params, b.geom)), f'block {i} G={G} n={n} group {g}'
                if G == 2:
                    b = blocks[1][i]
                    assert not torch.equal(out[:n], single(x[:n].contiguous(), b.params, b.geom))
        Tin = (Tin - 1) // b0.stride + 1
    assert Tin == {13: 4, 9: 3}[T]


def _problem(V, K, n, Cin, Cout, T, stride, rmode, g):
    """Group g's operands as f2s_ref.problem makes them (the extra key only moves the seed)."""
    pg = f2s_ref.problem('gcn', dict(V=V, K=K, N=n, Cin=Cin, Cout=Cout, T=T, g=g))
    pt = f2s_ref.problem('tcn', dict(V=V, N=n, Cin=Cin, Cout=Cout, T=T, stride=stride, rmode=rmode, g=g))
    none = torch.empty(0)
    params = [pg['Ae'], pg['Wg'], pg['bg'], pt['Wt'].reshape(Cout, Cout * 9), pt['bt'], none if pt['Wr'] is None else pt['Wr'],
              none if pt['br'] is None else pt['br']]
    return pg['x'], [t.to(DEV).contiguous() for t in params]


@pytest.mark.parametrize('case', [dict(V=18, K=1, n=2, Cin=3, Cout=16, T=7, stride=2, rmode=2),      # 4-byte weight paths (Cin = 3)
                                  dict(V=9, K=2, n=1, Cin=64, Cout=64, T=10, stride=1, rmode=1)],     # 16-byte ones, tf = 7
                         ids=['k1_conv_residual', 'k2_identity_residual'])
def test_one_and_two_subsets_and_a_canary(case):
    """K = 1 and K = 2 (the models have K = 3) on hand-built Ae and random parameters, G = 3; then the same call on an input and
    on parameters that are slices of NaN-filled buffers: a read outside a group's slice, or outside the arrays, would show."""
    G, n, geom = 3, case['n'], [case['K'], 9, case['stride'], case['rmode']]
    xs, per = zip(*[_problem(g=g, **case) for g in range(G)])
    x, params = torch.cat(xs).to(DEV), _stack(per)
    out = grouped(x, params, geom, G)
    assert bool(torch.isfinite(out).all())
    for g in range(G):
        sl = slice(g * n, (g + 1) * n)
        assert torch.equal(out[sl], single(x[sl].contiguous(), per[g], geom)), g
    assert not torch.equal(out[:n], single(x[:n].contiguous(), per[1], geom))
    buf = torch.full((G * n + 2,) + tuple(x.shape[1:]), float('nan'), device=DEV)
    buf[1:-1] = x
    framed = []
    for t in params:
        if t.numel():
            b = torch.full((G + 2,) + tuple(t.shape[1:]), float('nan'), device=DEV)
            b[1:-1] = t
            t = b[1:-1]
            assert t.is_contiguous()
        framed.append(t)
    assert buf[1:-1].is_contiguous()
    assert torch.equal(grouped(buf[1:-1], framed, geom, G), out)


# ---- 2: the ensemble equals its parts -------------------------------------------------------------------------------
def _parts(name, x, weights, softmax):
    """Model g's own small-batch engine on its derived stream, then ensemble.fuse."""
    parent = _parent(name)
    with torch.no_grad():
        scores = [_engine(name, g)(ops.stream_derive(x, parent, s)) for g, s in enumerate(STREAMS)]
    fused, pred, _ = ensemble.fuse(scores, weights, softmax=softmax)
    return fused, pred, torch.stack(scores)


@pytest.mark.parametrize('name, shape', SHAPES, ids=[n for n, _ in SHAPES])
def test_ensemble_equals_its_parts(name, shape):
    x = make_input(shape, seed=X_SEED).to(DEV)
    for weights in WEIGHTS:
        for softmax in (False, True):
            ens = _ens(name, weights, softmax)
            (fused, pred, scores), cnt = _counted(lambda: ens.predict(x))
            assert _grouped_n(cnt.names) == 20                                    # the grouped route ran
            rf, rp, rs = _parts(name, x, weights, softmax)
            assert tuple(scores.shape) == (4, shape[0], rs.shape[2]) and pred.dtype == torch.int64
            assert torch.equal(scores, rs) and torch.equal(fused, rf) and torch.equal(pred, rp), (weights, softmax)
            with torch.no_grad():
                assert torch.equal(ens(x), fused)


def test_flat_input_layout():
    """(N, T, V*C), the feeder's other layout, gives the result of its (N, C, T, V, 1) form."""
    x = make_input((2, 3, 13, 20, 1), seed=X_SEED).to(DEV)
    ens = _ens('ucla')
    with torch.no_grad():
        a = ens(x)
        b = ens(x[..., 0].permute(0, 2, 3, 1).reshape(2, 13, 60).contiguous())
    assert torch.equal(a, b)


# ---- 3: fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, shape', SHAPES[:2], ids=['ucla', 'ntu'])
def test_ensemble_against_the_fp64_oracle(name, shape):
    x = make_input(shape, seed=X_SEED)
    models = _models(name)
    parent = default_parent(models[0].graph)
    ref = torch.stack([_oracle(SM.derive(x.double(), parent, s), SE.sd64(m), m.num_point)[0] for m, s in zip(models, STREAMS)])
    for weights in WEIGHTS:
        ens = _ens(name, weights)
        with torch.no_grad():
            fused, pred, scores = ens.predict(x.to(DEV))
        scores, fused = scores.double().cpu(), fused.double().cpu()
        for g in range(4):
            err = float((scores[g] - ref[g]).abs().max())
            print(f'{name} group {g}: {err:.3e} against {BAR:.1e} (max|ref| {float(ref[g].abs().max()):.3e})')
            assert err <= BAR, (g, err)
        w64 = torch.tensor(weights, dtype=torch.float32).double()
        rf = (ref * w64[:, None, None]).sum(0)
        bar = float(w64.abs().sum()) * BAR
        top = rf.topk(2, dim=1).values
        margin = float((top[:, 0] - top[:, 1]).min())
        err = float((fused - rf).abs().max())
        print(f'{name} weights {weights}: fused {err:.3e} against {bar:.3e}, top-2 margin {margin:.4g}')
        assert margin > 2 * bar                                                    # the seed's margin (module docstring)
        assert err <= bar
        assert torch.equal(pred.cpu(), rf.argmax(1))


# ---- 4: launches, arrangements, replay -----------------------------------------------------------------------------
@pytest.mark.parametrize('name, shape', [('ucla', (1, 3, 52, 20, 1)), ('ntu', (1, 3, 20, 25, 2))], ids=['ucla', 'ntu'])
def test_launch_count(name, shape):
    """1 stem + 20 block launches + pool + fc + fuse."""
    ens = _ens(name)
    x = make_input(shape, seed=9).to(DEV)
    with torch.no_grad():
        ens(x)                                              # folds and stacks
    _, cnt = _counted(lambda: ens(x))
    assert cnt.n <= 28, (cnt.n, cnt.names)
    assert _grouped_n(cnt.names) == 20
    assert cnt.names.count('tamgcn_f2s_gcn_grouped') == 10 and cnt.names.count('tamgcn_f2s_tcn_grouped') == 10
    assert 'tamgcn_stream_derive' not in cnt.names and cnt.names.count('tamgcn_stem_streams_eval') == 1
    assert cnt.names.count('tamgcn_head_fc_grouped') == 1 and cnt.names.count('tamgcn_score_fuse') == 1


def test_arrangements_agree():
    x = make_input((2, 3, 13, 20, 1), seed=X_SEED).to(DEV)
    models = _models('ucla')
    with torch.no_grad():
        ref = _ens('ucla').predict(x)
    for arrangement in ('grouped', 'streams', 'serial'):
        ens = StreamEnsemble(models, STREAMS, arrangement=arrangement)
        (f, p, s), cnt = _counted(lambda: ens.predict(x))
        assert (_grouped_n(cnt.names) == 20) == (arrangement == 'grouped')
        assert (cnt.names.count('tamgcn_stream_derive') == 3) == (arrangement != 'grouped')
        assert (ens._side is not None) == (arrangement == 'streams')
        assert torch.equal(f, ref[0]) and torch.equal(p, ref[1]) and torch.equal(s, ref[2]), arrangement


@pytest.mark.parametrize('arrangement', ['grouped', 'streams'])
def test_graph_replay_equals_eager(arrangement):
    ens = StreamEnsemble(_models('ucla'), STREAMS, weights=WEIGHTS[1], arrangement=arrangement)
    fast = GraphedForward(ens)
    shape = (2, 3, 13, 20, 1)
    x, x2 = make_input(shape, seed=1).to(DEV), make_input(shape, seed=11).to(DEV)
    with torch.no_grad():
        ref, ref2 = ens(x).clone(), ens(x2).clone()
    _, cnt = _counted(lambda: fast(x))
    assert (_grouped_n(cnt.captured) == 20) == (arrangement == 'grouped')
    assert torch.equal(fast(x).clone(), ref)
    assert torch.equal(fast(x2).clone(), ref2) and not torch.equal(ref, ref2)         # a second replay, other data
    keep = fast._graphs[next(iter(fast._graphs))][3]
    if arrangement == 'grouped':                            # _tamgcn_keep_alive is honoured: the stacked tensors live with the graph
        assert any(k is not None and any(e is ens._eng._stacked for e in k) for k in keep if isinstance(k, list))
    else:                                                   # ... and each model's own folded blocks
        assert all(any(isinstance(k, list) and any(e is m.__dict__['_tamgcn_f2s']._blocks for e in k) for k in keep) for m in ens.models)


# ---- 5: re-fold ------------------------------------------------------------------------------------------------------
def test_refolds_the_model_whose_state_changed():
    models = [SE.model('ucla', g).to(DEV) for g in range(4)]
    ens = StreamEnsemble(models, STREAMS)
    x = make_input((2, 3, 13, 20, 1), seed=X_SEED).to(DEV)
    with torch.no_grad():
        f0, _, s0 = ens.predict(x)
        stacked = ens._eng._stacked
        ids = [[id(t) for t in params] for params, _ in stacked]
        models[2].edge_importance[3].mul_(1.1)
        f1, p1, s1 = ens.predict(x)
        assert ens._eng._stacked is stacked                 # rewritten in place: a captured graph reads the new values
        assert [[id(t) for t in params] for params, _ in stacked] == ids
        fresh = StreamEnsemble(models, STREAMS).predict(x)
    assert not torch.equal(f1, f0) and not torch.equal(s1[2], s0[2])
    for g in (0, 1, 3):
        assert torch.equal(s1[g], s0[g])
    assert torch.equal(f1, fresh[0]) and torch.equal(p1, fresh[1]) and torch.equal(s1, fresh[2])


# ---- 6: the other routes ---------------------------------------------------------------------------------------------
def test_fallback_routes(monkeypatch):
    ens = _ens('ucla', WEIGHTS[1])
    x = make_input((1, 3, 52, 20, 1), seed=X_SEED).to(DEV)
    with torch.no_grad():
        f0, p0, s0 = ens.predict(x)

    def check():
        (f, p, s), cnt = _counted(lambda: ens.predict(x))
        assert not any(n.endswith('_grouped') for n in cnt.names) and cnt.names.count('tamgcn_stream_derive') == 3
        ds, df = float((s - s0).abs().max()), float((f - f0).abs().max())
        print(f'scores {ds:.3e} against {2e-5 * float(s0.abs().max()):.3e}, fused {df:.3e} against {2e-5 * float(f0.abs().max()):.3e}')
        assert ds <= 2e-5 * float(s0.abs().max())
        assert df <= 2e-5 * float(f0.abs().max())
        assert torch.equal(p, p0)
    monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', 4 * 52 - 1)  # G*N*M*T = 208 frames: over the bound
    check()
    monkeypatch.setattr(f2s, 'F2S_MAX_FRAMES', BOUND)
    monkeypatch.setenv('TAMGCN_F2', '0')
    check()
    monkeypatch.setenv('TAMGCN_F2', '1')
    h = ens.models[1].st_gcn_networks[2].register_forward_hook(lambda *a: None)       # hooks would not fire on the grouped route
    try:
        check()
    finally:
        h.remove()
    _, cnt = _counted(lambda: ens.predict(x))
    assert _grouped_n(cnt.names) == 20


# ---- 7: guards -------------------------------------------------------------------------------------------------------
def test_abi_and_operator_guards_on_real_buffers():
    b = _blocks('ucla')[0][1]                               # 64 -> 64, identity residual
    xb = torch.zeros(3, 64, 8, 20, device=DEV)
    h = torch.zeros(3, 64, 8, 20, device=DEV)
    out = torch.zeros(3, 64, 8, 20, device=DEV)
    lib = _lib.load()
    two = [torch.stack([t, t]) for t in b.params]
    d = _lib.F2sGcnDesc(N=3, Cin=64, Cout=64, T=8, V=20, K=3, x=xb.data_ptr(), Ae=two[0].data_ptr(), wg=two[1].data_ptr(),
                        bg=two[2].data_ptr(), h=h.data_ptr())
    assert lib.tamgcn_f2s_gcn_grouped(C.byref(d), 2, None) == -1
    assert b'tamgcn_f2s_gcn_grouped: N=3 is not a multiple of groups=2' in lib.tamgcn_last_error()
    t = _lib.F2sTcnDesc(N=3, Cin=64, Cout=64, T=8, V=20, KT=9, stride=1, res_mode=1, h=h.data_ptr(), wt=two[3].data_ptr(),
                        bt=two[4].data_ptr(), x=xb.data_ptr(), wr=None, br=None, out=out.data_ptr())
    assert lib.tamgcn_f2s_tcn_grouped(C.byref(t), 2, None) == -1
    assert b'tamgcn_f2s_tcn_grouped: N=3 is not a multiple of groups=2' in lib.tamgcn_last_error()
    with pytest.raises(RuntimeError, match='multiple of groups'):
        grouped(xb, two, b.geom, 2)
    with pytest.raises(RuntimeError, match='leading axis'):
        grouped(xb, two, b.geom, 3)
    torch.cuda.synchronize()
    assert float(h.abs().max()) == 0 and float(out.abs().max()) == 0


def test_the_grouped_block_is_a_registered_operator():
    blocks = _blocks('ucla')
    x = make_input((4, 64, 12, 20), seed=3).to(DEV)
    for i in (1, 4):                                        # identity residual, stride 1; 64 -> 128, stride 2, convolutional residual
        params = _stack([blocks[g][i].params for g in range(2)])
        torch.library.opcheck(grouped.default, (x, params, blocks[0][i].geom, 2), test_utils=('test_schema', 'test_faketensor'))


# ---- 8: callers ------------------------------------------------------------------------------------------------------
def test_live_classifier_and_sliding_window_take_an_stgcn_ensemble():
    from test_gpu_streaming import _dev, _feeder_transform, _walk
    ens = StreamEnsemble(_models('ucla')[:2], STREAMS[:2])
    seq = _walk(np.random.default_rng(6), 44)

    def direct(rows):
        with torch.no_grad():
            return ens(_feeder_transform([seq[s:s + L] for s, L in rows], 52, 'joint'))
    live = LiveClassifier(ens, FrameRing(64, prep='nucla', V=20, device=DEV), window=20, frames_per_step=20)
    label, conf, smoothed, logits = live.step(_dev(seq[:20]))
    want = direct([(0, 20)])
    assert torch.equal(logits, want) and int(label) == int(want.argmax(1)) and ens.arrangement is None
    res = SlidingWindow(ens, window=20, hop=8, prep='nucla', batch_windows=4).run(_dev(seq))
    rows = [(0, 20), (8, 20), (16, 20), (24, 20)]
    assert res.plan.tolist() == [list(r) for r in rows]
    assert torch.equal(res.window_logits, direct(rows)) and res.frame_label.shape == (44,)
