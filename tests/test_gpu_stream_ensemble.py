"""-m gpu: a multi-stream ensemble as one grouped small-batch eval pass -- the grouped entry points of both kernel families
(tamgcn_f2_*_grouped, tamgcn_f2v_*_grouped), the fused stem and the grouped head (csrc/stemhead.hip), the grouped operators,
f2.GroupedEval and inference.StreamEnsemble.

The models: tests/stream_ensemble_models.py (golden running statistics, every parameter of model g scaled by 1 + 0.02 u from
seed g; max|activation| after l10 stays within 0.83x .. 1.26x of the unperturbed model's, fp64 oracle,
tests/test_stream_ensemble_cpu.py::test_perturbed_models_stay_tame).

Bars.  Grouped against single kernels, fused stem / head against their parts, the ensemble against its parts, graph replay:
bit equality.  Against the fp64 oracle: each group's scores within 1e-4 max|ref_g| (the project's logits bar for this path,
test_gpu_f2.py), the raw-fused scores within sum_g |w_g| 1e-4 max|ref_g| (triangle inequality), pred = the fp64 arg max with
input seed 1: at both shapes and both weight sets every sample's fp64 top-2 margin (V = 20: 2293 / 797, V = 25: 63 / 51)
exceeds twice that bar (3.6 / 1.8, 2.7 / 1.4) -- searched on the CPU from seed 1 upwards, the first one holds.  The general
path against the grouped one: 2e-5 max|.| (the project's bar between the family and the general path).

The group-stride alignment check of the grouped entry points has no test: no descriptor reaches it.  A launch takes a
16-byte path for a weight array only when the row length (Cin, R, K, Cb*ks) is a multiple of 16, and every group stride is a
multiple of that row length."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from params import make_input                                                      # noqa: E402
from tam_gcn_amd import f2, f2v, ops, ensemble, _lib                                # noqa: E402
from tam_gcn_amd.inference import GraphedForward, StreamEnsemble, default_parent   # noqa: E402
import stream_ensemble_models as SM                                                # noqa: E402

DEV = 'cuda:0'
STREAMS = ['joint', 'bone', 'motion', 'bone_motion']
TAG = {20: 'ucla_t52', 25: 'ntu_t20'}
SHAPES = [(2, 3, 13, 20, 1), (1, 3, 20, 25, 2)]
WEIGHTS = [(1, 1, 1, 1), (0.6, 0.6, 0.4, 0.4)]
X_SEED = 1


@functools.lru_cache(maxsize=None)
def _models(V, num_person=None):
    over = {} if num_person is None else dict(num_person=num_person)
    return tuple(SM.perturbed_model(TAG[V], g, **over).to(DEV).eval() for g in range(4))


@functools.lru_cache(maxsize=None)
def _blocks(V, num_person=None):
    cls = f2.FusedEval if V == 20 else f2v.FusedEvalV
    return tuple(cls(m)._packed(torch.device(DEV)) for m in _models(V, num_person))


@functools.lru_cache(maxsize=None)
def _engine(V, g):
    return (f2.FusedEval if V == 20 else f2v.FusedEvalV)(_models(V)[g])


@functools.lru_cache(maxsize=None)
def _shared_ens(V):
    return StreamEnsemble(_models(V), STREAMS)


def _ens(V, weights=WEIGHTS[0], softmax=False):
    """One ensemble per family on the shared (never modified) models; its weights live in a device tensor."""
    ens = _shared_ens(V)
    ens.weights.copy_(torch.tensor(weights, dtype=torch.float32))
    ens.softmax = softmax
    return ens


def _parent(V):
    return torch.tensor(default_parent(_models(V)[0].graph), dtype=torch.int32, device=DEV)


def _ops(V):
    t = torch.ops.tamgcn
    return (t.tcn_gcn_unit_eval, t.tcn_gcn_unit_eval_grouped) if V == 20 else (t.tcn_gcn_unit_eval_v25, t.tcn_gcn_unit_eval_v25_grouped)


class Count:
    """The counting wrapper of test_gpu_f2.py::test_graph_replay_and_launch_count."""

    def __init__(self, lib):
        self.lib, self.n, self.names, self.captured = lib, 0, [], []       # captured: the calls made inside a graph capture

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith('tamgcn_') or name in ('tamgcn_last_error',):
            return fn

        def w(*args):
            self.n += 1
            self.names.append(name)
            if torch.cuda.is_current_stream_capturing():
                self.captured.append(name)
            return fn(*args)
        return w


def _counted(fn, grad=False):
    real = _lib.load()
    cnt = Count(real)
    _lib._lib = cnt
    try:
        with torch.set_grad_enabled(grad):
            out = fn()
    finally:
        _lib._lib = real
    return out, cnt


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V, T, num_person', [(20, 13, None), (20, 52, None), (20, 30, 2), (25, 20, None), (25, 13, None)],
                         ids=['v20_t13', 'v20_t52', 'v20_t30_two_persons', 'v25_t20', 'v25_t13'])
def test_grouped_block_equals_the_single_block_bit_for_bit(V, T, num_person):
    """Every block l1..l10, groups 2 and 4, n = 1 (mean over T from x) and n = 2 (from a given xpart): group g's slice of
    the grouped operator's out and xpart equals the single operator on model g's _Block; two grouped runs are equal.
    T = 13: tiles of 1, 3 and 4 frames down the depth."""
    blocks = _blocks(V, num_person)
    single, grouped = _ops(V)
    VP = 20 if V == 20 else 28
    Tin = T
    for i in range(10):
        b0 = blocks[0][i]
        for G in (2, 4):
            params = [torch.stack([blocks[g][i].params[j] for g in range(G)]) for j in range(len(b0.params))]
            for n in (1, 2):
                x = make_input((G * n, b0.Cin, Tin, V), seed=100 * i + 10 * G + n).to(DEV)
                xp = None if n == 1 else make_input((G * n, (Tin + 3) // 4, b0.Cin, VP), seed=7 + i).to(DEV)
                out, xo = grouped(x, xp, params, b0.geom, G)
                out2, xo2 = grouped(x, xp, params, b0.geom, G)
                assert torch.equal(out, out2) and torch.equal(xo, xo2), f'l{i + 1} G={G} n={n}: two runs differ'
                assert bool(torch.isfinite(out).all())
                for g in range(G):
                    sl = slice(g * n, (g + 1) * n)
                    b = blocks[g][i]
                    ro, rx = single(x[sl].contiguous(), None if xp is None else xp[sl].contiguous(), b.params, b.geom)
                    assert torch.equal(out[sl], ro), f'l{i + 1} G={G} n={n} group {g}: out'
                    assert torch.equal(xo[sl], rx), f'l{i + 1} G={G} n={n} group {g}: xpart'
                if G == 2:                                  # the groups really differ: group 1's parameters on group 0's samples
                    b = blocks[1][i]
                    ro, _ = single(x[:n].contiguous(), None if xp is None else xp[:n].contiguous(), b.params, b.geom)
                    assert not torch.equal(out[:n], ro)
        Tin = (Tin - 1) // b0.stride + 1


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=['v20', 'v25'])
@pytest.mark.parametrize('modes', [(0, 1, 2, 3), (3, 3)])
def test_fused_stem_equals_stream_derive_then_stem_apply(shape, modes):
    N, C_, T, V, M = shape
    G = len(modes)
    eng = f2.GroupedEval(_models(V)[:G])
    eng._packed(torch.device(DEV))
    coef = eng._coef
    buf = torch.full((N + 2,) + tuple(shape[1:]), float('nan'), device=DEV)
    buf[1:1 + N] = make_input(shape, seed=X_SEED).to(DEV)
    x = buf[1:1 + N]
    assert x.is_contiguous()
    parent, mt = _parent(V), torch.tensor(modes, dtype=torch.int32, device=DEV)
    out = ops.stem_streams_eval(x, parent, mt, coef)
    assert tuple(out.shape) == (G * N * M, C_, T, V) and bool(torch.isfinite(out).all())
    if V % 4:                                               # f2v reads 12 bytes past the last frame
        assert out.untyped_storage().nbytes() - (out.storage_offset() + out.numel()) * 4 >= 12
    for g, mode in enumerate(modes):
        ref = ops.stem_apply(ops.stream_derive(x, parent, mode), coef[g].contiguous())
        got = out[g * N * M:(g + 1) * N * M]
        assert torch.equal(got, ref), (g, mode)
        if mode >= 2:                                       # motion of the last frame is 0: exactly c1*0 + c0
            c0 = coef[g, 2].view(M, V, C_).permute(0, 2, 1)                        # [m][c][v]
            last = got.view(N, M, C_, T, V)[:, :, :, T - 1]
            assert torch.equal(last, c0.expand(N, M, C_, V))


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [10, 60])
@pytest.mark.parametrize('N', [1, 3])
def test_grouped_head_equals_the_single_head(K, N):
    G, C_ = 4, 256
    pooled = make_input((G * N, C_), seed=K + N).to(DEV)
    W, b = make_input((G, K, C_), seed=2).to(DEV), make_input((G, K), seed=3).to(DEV)
    got = ops.head_fc_grouped(pooled, W, b, G)
    assert tuple(got.shape) == (G, N, K)
    for g in range(G):
        assert torch.equal(got[g], ops.head_fc_fwd(pooled[g * N:(g + 1) * N].contiguous(), W[g].contiguous(), b[g].contiguous()))


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def _parts(V, x, weights, softmax):
    """Model g's own small-batch engine on its derived stream, then ensemble.fuse."""
    parent = _parent(V)
    with torch.no_grad():
        scores = [_engine(V, g)(ops.stream_derive(x, parent, s)) for g, s in enumerate(STREAMS)]
    fused, pred, _ = ensemble.fuse(scores, weights, softmax=softmax)
    return fused, pred, torch.stack(scores)


@pytest.mark.parametrize('shape', SHAPES + [(2, 3, 52, 20, 1)], ids=['v20_t13', 'v25_t20', 'v20_t52'])
def test_ensemble_equals_its_parts(shape):
    V = shape[3]
    x = make_input(shape, seed=X_SEED).to(DEV)
    for weights in WEIGHTS:
        for softmax in (False, True):
            ens = _ens(V, weights, softmax)
            (fused, pred, scores), cnt = _counted(lambda: ens.predict(x))
            assert sum(n.endswith('_grouped') for n in cnt.names) == 51          # the grouped route ran
            rf, rp, rs = _parts(V, x, weights, softmax)
            assert tuple(scores.shape) == (4, shape[0], rs.shape[2]) and pred.dtype == torch.int64
            assert torch.equal(scores, rs) and torch.equal(fused, rf) and torch.equal(pred, rp), (weights, softmax)
            with torch.no_grad():
                assert torch.equal(ens(x), fused)


def test_flat_input_layout():
    """(N, T, V*C), the feeder's other layout, gives the result of its (N, C, T, V, 1) form."""
    x = make_input((2, 3, 13, 20, 1), seed=X_SEED).to(DEV)
    ens = _ens(20)
    with torch.no_grad():
        a = ens(x)
        b = ens(x[..., 0].permute(0, 2, 3, 1).reshape(2, 13, 60).contiguous())
    assert torch.equal(a, b)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=['v20', 'v25'])
def test_ensemble_against_the_fp64_oracle(shape):
    V = shape[3]
    x = make_input(shape, seed=X_SEED)
    models = _models(V)
    ref = SM.oracle_scores([m for m in models], STREAMS, default_parent(models[0].graph), x)       # (G, N, K) fp64
    for weights in WEIGHTS:
        ens = _ens(V, weights)
        with torch.no_grad():
            fused, pred, scores = ens.predict(x.to(DEV))
        scores, fused = scores.double().cpu(), fused.double().cpu()
        bars = [1e-4 * float(r.abs().max()) for r in ref]
        for g in range(4):
            err = float((scores[g] - ref[g]).abs().max())
            print(f'V={V} group {g}: {err:.3e} against {bars[g]:.3e}')
            assert err <= bars[g], (g, err, bars[g])
        w64 = torch.tensor(weights, dtype=torch.float32).double()
        rf = (ref * w64[:, None, None]).sum(0)
        bar = sum(abs(float(w)) * b for w, b in zip(w64, bars))
        top = rf.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 2 * bar               # the seed's margin (module docstring)
        err = float((fused - rf).abs().max())
        print(f'V={V} weights {weights}: fused {err:.3e} against {bar:.3e}')
        assert err <= bar
        assert torch.equal(pred.cpu(), rf.argmax(1))


# ---- 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, fam', [((1, 3, 52, 20, 1), 'f2'), ((1, 3, 20, 25, 2), 'f2v')], ids=['v20', 'v25'])
def test_launch_count(shape, fam):
    """1 stem + 50 block launches + pool + fc + fuse: at most 58 ABI calls, exactly 50 grouped block launches, no stream_derive."""
    ens = _ens(shape[3])
    x = make_input(shape, seed=9).to(DEV)
    with torch.no_grad():
        ens(x)                                              # folds and stacks
    _, cnt = _counted(lambda: ens(x))
    assert cnt.n <= 58, (cnt.n, cnt.names)
    assert sum(n.startswith(f'tamgcn_{fam}_') and n.endswith('_grouped') for n in cnt.names) == 50
    assert 'tamgcn_stream_derive' not in cnt.names and cnt.names.count('tamgcn_stem_streams_eval') == 1
    assert cnt.names.count('tamgcn_head_fc_grouped') == 1 and cnt.names.count('tamgcn_score_fuse') == 1


# ---- 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [20, 25])
def test_graph_replay_equals_eager(V):
    ens = _ens(V, WEIGHTS[1])
    fast = GraphedForward(ens)
    for nb in (1, 2):
        shape = (nb, 3, 52, 20, 1) if V == 20 else (nb, 3, 20, 25, 2)
        x = make_input(shape, seed=nb).to(DEV)
        with torch.no_grad():
            ref = ens(x).clone()
        assert torch.equal(fast(x).clone(), ref)
        x2 = make_input(shape, seed=nb + 10).to(DEV)
        with torch.no_grad():
            ref2 = ens(x2).clone()
        assert torch.equal(fast(x2).clone(), ref2) and not torch.equal(ref, ref2)      # a second replay, other data
    keep = fast._graphs[next(iter(fast._graphs))][3]
    assert any(k is not None and any(e is ens._eng._stacked for e in k) for k in keep if isinstance(k, list))


def test_arrangements_agree_and_graphed_forward_takes_the_streams_route():
    """profiles/stream_ensemble_bench.txt: under graph replay the grouped pass ties with the G models on G streams at one
    clip-person per model and loses beyond, so GraphedForward -- its warm-up calls and its capture alike -- takes the streams
    with more than one clip-person per model unless told otherwise; every other call takes the grouped pass.  All
    arrangements give the same bits."""
    x = make_input((2, 3, 52, 20, 1), seed=X_SEED).to(DEV)
    models = _models(20)
    with torch.no_grad():
        ref = _ens(20).predict(x)
    for arrangement in ('grouped', 'streams', 'serial'):
        ens = StreamEnsemble(models, STREAMS, arrangement=arrangement)
        (f, p, s), cnt = _counted(lambda: ens.predict(x))
        assert (sum(n.endswith('_grouped') for n in cnt.names) == 51) == (arrangement == 'grouped')
        assert (ens._side is not None) == (arrangement == 'streams')            # side streams only where they are used
        assert torch.equal(f, ref[0]) and torch.equal(p, ref[1]) and torch.equal(s, ref[2]), arrangement
    ens = StreamEnsemble(models, STREAMS)
    fast = GraphedForward(ens)
    _, cnt = _counted(lambda: fast(x))                      # two warm-up calls and the capture: all three on the streams
    assert 'tamgcn_stem_streams_eval' not in cnt.names and cnt.names.count('tamgcn_stream_derive') == 9
    assert cnt.captured.count('tamgcn_stream_derive') == 3 and not ens._tamgcn_graphed
    assert torch.equal(fast(x), ref[0])
    (f, _, _), cnt = _counted(lambda: ens.predict(x))       # the same object called directly: grouped
    assert cnt.names.count('tamgcn_stem_streams_eval') == 1 and torch.equal(f, ref[0])
    forced = GraphedForward(StreamEnsemble(models, STREAMS, arrangement='grouped'))
    _, cnt = _counted(lambda: forced(x))
    assert cnt.names.count('tamgcn_stem_streams_eval') == 3 and 'tamgcn_stream_derive' not in cnt.names
    assert torch.equal(forced(x), ref[0])
    _, cnt = _counted(lambda: fast(x[:1]))                  # one clip-person per model: warm-up and capture grouped
    assert cnt.names.count('tamgcn_stem_streams_eval') == 3 and 'tamgcn_stream_derive' not in cnt.names
    with pytest.raises(ValueError, match='arrangement'):
        StreamEnsemble(models, STREAMS, arrangement='fastest')


@pytest.mark.parametrize('shape, fam', [((2, 3, 13, 20, 1), 'f2'), ((1, 3, 20, 25, 2), 'f2v')], ids=['v20', 'v25'])
def test_capture_on_fresh_models_holds_the_forward_alone(shape, fam):
    """Models that never ran a forward: each model's own engine is built and folded in GraphedForward's warm-up calls, which
    take the route of the capture.  The captured graph then holds exactly 3 stream_derive + G * 53 + 1 score_fuse ABI
    launches and equals the eager result."""
    V = shape[3]
    models = [SM.perturbed_model(TAG[V], g).to(DEV).eval() for g in range(4)]
    ens = StreamEnsemble(models, STREAMS)
    x = make_input(shape, seed=X_SEED).to(DEV)
    fast = GraphedForward(ens)
    out, cnt = _counted(lambda: fast(x))
    c = cnt.captured
    assert len(c) == 3 + 4 * 53 + 1, (len(c), sorted(set(c)))
    assert c.count('tamgcn_stream_derive') == 3 and c.count('tamgcn_score_fuse') == 1 and c.count('tamgcn_stem_apply') == 4
    assert sum(n.startswith(f'tamgcn_{fam}_') and not n.endswith('_grouped') for n in c) == 200
    assert c.count('tamgcn_head_pool_fwd') == 4 and c.count('tamgcn_head_fc_fwd') == 4
    slot = '_tamgcn_f2' if V == 20 else '_tamgcn_f2v'
    assert all(m.__dict__.get(slot) for m in models)        # built before the capture, kept alive by the graph entry
    with torch.no_grad():
        assert torch.equal(ens(x), out)


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def test_refolds_the_model_whose_state_changed():
    models = [SM.perturbed_model(TAG[20], g).to(DEV).eval() for g in range(4)]
    ens = StreamEnsemble(models, STREAMS)
    x = make_input((2, 3, 13, 20, 1), seed=X_SEED).to(DEV)
    with torch.no_grad():
        f0, _, s0 = ens.predict(x)
        stacked = ens._eng._stacked
        models[2].l6.gcn1.convs[1].conv3.weight.mul_(1.1)
        f1, p1, s1 = ens.predict(x)
        assert ens._eng._stacked is stacked                 # rewritten in place: a captured graph reads the new values
        fresh = StreamEnsemble(models, STREAMS).predict(x)
    assert not torch.equal(f1, f0) and not torch.equal(s1[2], s0[2])
    for g in (0, 1, 3):
        assert torch.equal(s1[g], s0[g])
    assert torch.equal(f1, fresh[0]) and torch.equal(p1, fresh[1]) and torch.equal(s1, fresh[2])


# ---- 9 ---------------------------------------------------------------------------------------------------------------
def test_fallback_routes(monkeypatch):
    ens = _ens(20, WEIGHTS[1])
    x = make_input((1, 3, 52, 20, 1), seed=X_SEED).to(DEV)
    with torch.no_grad():
        f0, p0, s0 = ens.predict(x)

    def check():
        (f, p, s), cnt = _counted(lambda: ens.predict(x))
        assert not any(n.endswith('_grouped') for n in cnt.names) and cnt.names.count('tamgcn_stream_derive') == 3
        assert float((s - s0).abs().max()) <= 2e-5 * float(s0.abs().max())
        assert float((f - f0).abs().max()) <= 2e-5 * float(f0.abs().max())
        assert torch.equal(p, p0)
    monkeypatch.setattr(f2, 'F2_MAX_CLIPS', 3)              # G*N*M = 4 clip-persons: over the bound
    check()
    monkeypatch.undo()
    monkeypatch.setenv('TAMGCN_F2', '0')
    check()
    monkeypatch.undo()
    h = ens.models[1].l3.register_forward_hook(lambda *a: None)             # hooks would not fire on the grouped route
    check()
    h.remove()
    ens25 = _ens(25)
    x25 = make_input((1, 3, 20, 25, 2), seed=X_SEED).to(DEV)
    with torch.no_grad():
        s0 = ens25.predict(x25)[2]
    monkeypatch.setattr(f2v, 'F2V_MAX_FRAMES', 159)         # G*N*M*T = 160 frames
    (_, _, s), cnt = _counted(lambda: ens25.predict(x25))
    assert not any(n.endswith('_grouped') for n in cnt.names)
    assert float((s - s0).abs().max()) <= 2e-5 * float(s0.abs().max())


# ---- 10 --------------------------------------------------------------------------------------------------------------
def test_guards_raise_before_any_launch():
    from cases import MODEL_CASES
    from tam_gcn_amd.models import ctrgcn as M
    ucla = next(c for c in MODEL_CASES if c[0] == 'ucla_t52')[1]
    ntu = next(c for c in MODEL_CASES if c[0] == 'ntu_t20')[1]
    mk = lambda margs=ucla, **over: M.Model(**dict(margs, **over)).to(DEV).eval()
    x = make_input((1, 3, 13, 20, 1), seed=1)

    def refused(exc, match, fn, grad=False):
        def run():
            with pytest.raises(exc, match=match):
                fn()
        _, cnt = _counted(run, grad)
        launches = [n for n in cnt.names if n not in ('tamgcn_version', 'tamgcn_last_kernel')]
        assert not launches, launches
    two = [mk(), mk()]
    refused(ValueError, 'num_class', lambda: StreamEnsemble([mk(), mk(num_class=12)], STREAMS[:2]))
    refused(ValueError, 'num_point', lambda: StreamEnsemble([mk(), mk(), mk(ntu)], STREAMS[:3]))
    refused(ValueError, 'train mode', lambda: StreamEnsemble([mk(), mk().train()], STREAMS[:2]))
    refused(ValueError, '2 models but 4 streams', lambda: StreamEnsemble(two))
    refused(ValueError, 'unknown stream', lambda: StreamEnsemble(two, ('joint', 'velocity')))
    refused(ValueError, 'is on cpu', lambda: StreamEnsemble([mk(), mk().cpu()], STREAMS[:2]))
    ens = StreamEnsemble(two, STREAMS[:2])
    refused(RuntimeError, 'no CPU path', lambda: ens(x))
    refused(RuntimeError, 'no_grad', lambda: ens(x.to(DEV)), grad=True)
    two[1].train()
    refused(RuntimeError, 'train', lambda: ens(x.to(DEV)))
    two[1].eval()
    # the ABI: N % groups, on real buffers
    b = _blocks(20)[0][1]
    xb = torch.zeros(3, 64, 8, 20, device=DEV)
    out = torch.zeros(3, 64, 8, 20, device=DEV)
    lib = _lib.load()
    d = _lib.F2GemmDesc(N=3, K=64, M=64, T=8, V=20, mode=1, relu_rows=0, x=xb.data_ptr(), w=b.Wo.data_ptr(), b=b.bo.data_ptr(), add=None, out=out.data_ptr())
    assert lib.tamgcn_f2_gemm_grouped(C.byref(d), 2, None) == -1
    assert b'N=3 is not a multiple of groups=2' in lib.tamgcn_last_error()
    with pytest.raises(RuntimeError, match='multiple of groups'):
        torch.ops.tamgcn.tcn_gcn_unit_eval_grouped(xb, None, [torch.stack([t, t]) for t in b.params], b.geom, 2)
    with pytest.raises(RuntimeError, match='leading axis'):
        torch.ops.tamgcn.tcn_gcn_unit_eval_grouped(xb, None, [torch.stack([t, t]) for t in b.params], b.geom, 3)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0


# ---- 11 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [20, 25])
def test_grouped_blocks_are_registered_operators(V):
    blocks = _blocks(V)
    _, grouped = _ops(V)
    x = make_input((4, 64, 12, V), seed=3).to(DEV)
    for i in (1, 4):                                        # identity residual, stride 1; 64 -> 128, stride 2, convolutional residuals
        params = [torch.stack([blocks[g][i].params[j] for g in range(2)]) for j in range(len(blocks[0][i].params))]
        torch.library.opcheck(grouped.default, (x, None, params, blocks[0][i].geom, 2), test_utils=('test_schema', 'test_faketensor'))
