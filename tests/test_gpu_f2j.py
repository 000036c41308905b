"""-m gpu: the small-batch eval kernel family on 17- and 18-joint skeletons (csrc/f2v.hip at V = 17, 18; tam_gcn_amd/f2v.py:
FusedEvalJ, tamgcn::tcn_gcn_unit_eval_vj[_grouped]) -- the COCO (17 joints, one person) and OpenPose (18 joints, two persons)
models of tests/test_gpu_vgen_model.py with seeded parameters and running statistics settled by one momentum-1 train-mode
pass on inputs of their own (no golden eval statistics exist for these models).

Bars (the project's own, tests/test_gpu_f2v.py; none is fitted to this code): every block, fed the fp64 oracle's own input for
that block (teacher-forced), within 4 x 1.21e-6 of max|ref|; logits within 1e-4 max|ref| of the fp64 oracle with the same arg
max; logits and features within 2e-5 (relative) of the general eval path (TAMGCN_F2=0), which is itself held to the fp64
oracle at 1e-3 here (tests/test_gpu_vgen_model.py's batch-1 eval forward now runs through this family).  Per output element
the sums run over the same K in the same order as at 25 joints.  `pytest -s` prints the measured ratios and, beside them, the
error of an fp32 torch evaluation of the same blocks (MI355X: worst block 5.1e-7 against torch's 5.3e-7, worst logits 2.0e-6
against 2.2e-6)."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from params import fill_state_, make_input                                        # noqa: E402
from tam_gcn_amd import f2, f2v, ops, _lib                                          # noqa: E402
from tam_gcn_amd.inference import GraphedForward, StreamEnsemble, default_parent  # noqa: E402
from tam_gcn_amd.models import ctrgcn as M                                          # noqa: E402
from oracle import ctrgcn_oracle as O                                               # noqa: E402

DEV = 'cuda:0'
COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
OPENPOSE = dict(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=dict(labeling_mode='spatial'))
TREE7 = dict(num_class=6, num_point=7, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=7, arity=2))
MARGS = {17: COCO, 18: OPENPOSE}
PARAM_SEED = 42
BLOCK_BAR = 4 * 1.21e-6


@functools.lru_cache(maxsize=None)
def _settled_state(V, num_person):
    """CPU state of the model with running statistics of its own inputs (one momentum-1 pass in train mode)."""
    m = M.Model(**dict(MARGS[V], num_person=num_person))
    fill_state_(m.state_dict(), seed=PARAM_SEED)
    m = m.to(DEV).train()
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m(make_input((8 // num_person, 3, 16, V, num_person), seed=5).to(DEV))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _model(V, num_person=None):
    num_person = num_person or MARGS[V]['num_person']
    m = M.Model(**dict(MARGS[V], num_person=num_person))
    m.load_state_dict(_settled_state(V, num_person))
    return m.to(DEV).eval()


def _sd64(m):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


class _general:
    """Model.forward on the general eval path (what TAMGCN_F2=0 selects)."""

    def __enter__(self):
        self.old = os.environ.get('TAMGCN_F2')
        os.environ['TAMGCN_F2'] = '0'

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ['TAMGCN_F2']
        else:
            os.environ['TAMGCN_F2'] = self.old


class Count:
    """The counting wrapper of test_gpu_f2v.py::test_graph_replay_and_launch_count."""

    def __init__(self, lib):
        self.lib, self.n, self.names = lib, 0, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith('tamgcn_') or name in ('tamgcn_last_error',):
            return fn

        def w(*args):
            self.n += 1
            self.names.append(name)
            return fn(*args)
        return w


def _counted(fn):
    real = _lib.load()
    cnt = Count(real)
    _lib._lib = cnt
    try:
        with torch.no_grad():
            out = fn()
    finally:
        _lib._lib = real
    return out, cnt


# ---------------------------------------------------------------------------------------------------------------------
# every block, teacher-forced on the fp64 oracle's input for that block
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 13, 17, 1), (1, 3, 30, 17, 1), (1, 3, 20, 18, 2), (1, 3, 13, 18, 1)]


@pytest.mark.parametrize('shape', SHAPES, ids=['coco_t13_two_clips', 'coco_t30', 'openpose_t20_two_persons', 'openpose_t13_one_person'])
def test_every_block_against_the_fp64_oracle(shape):
    """Frames per depth 13 -> 7 -> 4, 30 -> 15 -> 8 and 20 -> 10 -> 5: ragged last tiles of 1, 2 and 3 frames, odd T under
    stride 2, every residue of T*V mod 4, one and two persons."""
    V = shape[3]
    m = _model(V, shape[4])
    sd64 = _sd64(m)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd64.items()}
    x = make_input(shape, seed=21)
    h, N, Mp = O._stem(x.double(), sd64, V, False)
    ins, outs, e32 = [], [], []
    for i in range(1, 11):
        ins.append(h)
        kw = dict(residual=(i != 1), training=False)
        f32 = O.tcn_gcn_unit(h.float(), sd32, f'l{i}', O._STRIDES.get(i, 1), **kw)     # torch's own fp32 evaluation of the same block
        h = O.tcn_gcn_unit(h, sd64, f'l{i}', O._STRIDES.get(i, 1), **kw)
        outs.append(h)
        e32.append(_rel(f32.double(), h))
    eng = f2v.FusedEvalJ(m)
    blocks = eng._packed(torch.device(DEV))
    errs = []
    for i, (b, xin, ref) in enumerate(zip(blocks, ins, outs), 1):
        got = eng._block(b, xin.float().to(DEV).contiguous()).double().cpu()
        assert got.shape == ref.shape, (i, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), f'l{i}'
        errs.append(_rel(got, ref))
    print(f'\n{shape}: block error / max|ref|: ' + ' '.join(f'l{i}={e:.2e}' for i, e in enumerate(errs, 1)))
    print(f'{shape}: fp32 torch evaluation:   ' + ' '.join(f'l{i}={e:.2e}' for i, e in enumerate(e32, 1)))
    for i, e in enumerate(errs, 1):
        assert e <= BLOCK_BAR, f'l{i}: {e:.3e} of max|ref|'
    with torch.no_grad():
        logits = eng(x.to(DEV)).double().cpu()
    ref = O.model_forward(x.double(), sd64, V, training=False)
    l32 = O.model_forward(x, sd32, V, training=False).double()
    print(f'{shape}: logits error / max|ref| = {_rel(logits, ref):.2e} (fp32 torch evaluation {_rel(l32, ref):.2e})')
    assert float((logits - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    assert torch.equal(logits.argmax(1), ref.argmax(1))


@pytest.mark.parametrize('shape', [(2, 3, 13, 17, 1), (1, 3, 20, 18, 2)], ids=['coco', 'openpose'])
def test_model_forward_against_the_general_path_and_that_against_the_oracle(shape, monkeypatch):
    """Through Model.forward and extract_feature: the family within 2e-5 (relative) of the general path, logits and features; the
    general path (TAMGCN_F2=0: no engine is built) within 1e-3 of the fp64 oracle with its arg max."""
    V = shape[3]
    m = _model(V)
    x = make_input(shape, seed=21).to(DEV)
    calls = []
    real = f2v.FusedEvalJ.blocks
    monkeypatch.setattr(f2v.FusedEvalJ, 'blocks', lambda self, x: (calls.append(1), real(self, x))[1])
    with torch.no_grad():
        with _general():
            b = m(x)
            fb, _ = m.extract_feature(x)
        assert not calls and not m.__dict__.get('_tamgcn_f2j'), 'TAMGCN_F2=0 is the general eval path'
        a = m(x)
        fa, _ = m.extract_feature(x)
    assert len(calls) == 2 and isinstance(m.__dict__.get('_tamgcn_f2j'), f2v.FusedEvalJ)
    ref = O.model_forward(x.cpu().double(), _sd64(m), V, training=False)
    err = float((b.cpu().double() - ref).abs().max())
    print(f'\n{shape}: general vs oracle {err:.2e} (abs), family vs general logits {_rel(a, b):.2e}, features {_rel(fa, fb):.2e}')
    assert err <= 1e-3 and torch.equal(b.argmax(1).cpu(), ref.argmax(1))
    assert _rel(a, b) <= 2e-5
    assert fa.shape == fb.shape and _rel(fa, fb) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# slack and alignment of the contiguous block input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [6, 7])
@pytest.mark.parametrize('which', [1, 4], ids=['identity', 'stride2_conv'])
@pytest.mark.parametrize('V', [17, 18])
def test_nan_before_the_input_and_in_its_slack_reaches_nothing(V, which, T):
    """The input is a slice of a NaN-filled buffer: NaN in front of it (the slice starts 3 floats in: dword-aligned only) and in
    the 4 slack floats behind it, which the last 16-byte piece of the last frame reads (3 of them at V = 17, 2 at V = 18).
    Same bits as on a clean copy."""
    m = _model(V)
    b = f2v.FusedEvalJ(m)._packed(torch.device(DEV))[which]
    data = make_input((2, 64, T, V), seed=3).to(DEV)
    n = data.numel()
    buf = torch.full((3 + n + 4,), float('nan'), device=DEV)
    buf[3:3 + n] = data.view(-1)
    dirty = buf[3:3 + n].view(data.shape)
    assert dirty.data_ptr() % 16 == 12 and bool(torch.isnan(buf[3 + n:]).all())
    clean, cxp = torch.ops.tamgcn.tcn_gcn_unit_eval_vj(data, None, b.params, b.geom)
    got, gxp = torch.ops.tamgcn.tcn_gcn_unit_eval_vj(dirty, None, b.params, b.geom)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gxp).all())
    assert torch.equal(got, clean) and torch.equal(gxp, cxp)
    assert bool(torch.isnan(buf[:3]).all()) and bool(torch.isnan(buf[3 + n:]).all())
    assert torch.equal(buf[3:3 + n], data.view(-1))


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [17, 18])
def test_model_forward_routes_small_eval_batches_here(V, monkeypatch):
    m = _model(V)
    P = MARGS[V]['num_person']
    x = make_input((1, 3, 16, V, P), seed=2).to(DEV)
    calls = []
    real = f2v.FusedEvalJ.blocks
    monkeypatch.setattr(f2v.FusedEvalJ, 'blocks', lambda self, x: (calls.append(1), real(self, x))[1])
    with torch.no_grad():
        m(x)
        m.extract_feature(x)
        assert len(calls) == 2
        assert m._f2(x) is None and m._f2v(x) is None and m._f2j(x) is not None
        assert not m.__dict__.get('_tamgcn_f2') and not m.__dict__.get('_tamgcn_f2v')
        T = 8
        big = make_input((f2v.F2J_MAX_FRAMES // (P * T) + 1, 3, T, V, P), seed=3).to(DEV)
        assert m._f2j(big[:-1]) is not None and m._f2j(big) is None
        m(big)                                              # over the bound (clip-persons x frames): general path
        assert len(calls) == 2
        monkeypatch.setenv('TAMGCN_F2', '0')
        m(x)
        assert len(calls) == 2
        monkeypatch.setenv('TAMGCN_F2', '1')
        h = m.l3.register_forward_hook(lambda mod, i, o: None)
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


def test_a_seven_joint_model_is_untouched():
    m = M.Model(**TREE7)
    fill_state_(m.state_dict(), seed=PARAM_SEED)
    m = m.to(DEV).eval()
    x = make_input((1, 3, 8, 7, 1), seed=2).to(DEV)
    (_, cnt) = _counted(lambda: m(x))
    assert m._f2j(x) is None and '_tamgcn_f2j' not in m.__dict__
    assert not any(n.startswith('tamgcn_f2') for n in cnt.names)
    with pytest.raises(f2.Unsupported):
        f2v.FusedEvalJ(m)


# ---------------------------------------------------------------------------------------------------------------------
# re-fold
# ---------------------------------------------------------------------------------------------------------------------
def _pair(m, x):
    with torch.no_grad():
        a = m(x)
        with _general():
            b = m(x)
    assert _rel(a, b) <= 2e-5
    return a


@pytest.mark.parametrize('V', [17, 18])
def test_refolds_after_every_kind_of_state_change(V):
    m = _model(V)
    P = MARGS[V]['num_person']
    x = make_input((1, 3, 20, V, P), seed=21).to(DEV)
    a0 = _pair(m, x)
    assert m.__dict__.get('_tamgcn_f2j')
    with torch.no_grad():
        m.l3.tcn1.branches[0][1].weight.mul_(1.5)
        m.l6.gcn1.convs[1].conv4.bias.add_(0.3)
    a1 = _pair(m, x)
    assert float((a1 - a0).abs().max()) > 0
    m2 = _model(V)
    with torch.no_grad():
        for p in m2.parameters():
            p.mul_(0.9)
    m.load_state_dict(m2.state_dict())
    a2 = _pair(m, x)
    assert float((a2 - a1).abs().max()) > 1e-3 * float(a1.abs().max())
    m.train()                                               # a train-mode forward rewrites the running statistics
    with torch.no_grad():
        m(make_input((4, 3, 12, V, P), seed=8).to(DEV) * 1.5)
    m.eval()
    a3 = _pair(m, x)
    assert float((a3 - a2).abs().max()) > 0


def test_refolds_after_a_flat_arena_step():
    from tam_gcn_amd.distributed import ParamArena, SGDNesterov
    m = _model(17)
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
# graph replay, launch count, the operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [17, 18])
def test_graph_replay_and_launch_count(V):
    """GraphedForward captures this path: replay = eager bit for bit, two eager runs are bit-equal, the capture keeps the folded
    weights of the engine alive; 50 family launches per forward and at most 56 ABI launches in all, as at 20 and 25 joints."""
    m = _model(V)
    P = MARGS[V]['num_person']
    fast = GraphedForward(m)
    for shape in ((1, 3, 13, V, P), (2, 3, 20, V, P)):
        x = make_input(shape, seed=shape[2]).to(DEV)
        with torch.no_grad():
            ref = m(x)
            assert torch.equal(m(x), ref)
        assert torch.equal(fast(x).clone(), ref)
        assert torch.equal(fast(x).clone(), ref)
    eng = m.__dict__['_tamgcn_f2j']
    assert all(any(k is eng._blocks for k in ent[3]) for ent in fast._graphs.values())
    _, cnt = _counted(lambda: m(make_input((1, 3, 20, V, P), seed=9).to(DEV)))
    assert cnt.n <= 56, (cnt.n, cnt.names)
    assert sum(n.startswith('tamgcn_f2v_') for n in cnt.names) == 50
    assert not any(n.startswith('tamgcn_f2_') for n in cnt.names)


@pytest.mark.parametrize('V', [17, 18])
def test_block_is_a_registered_operator(V):
    """torch.ops.tamgcn.tcn_gcn_unit_eval_vj: schema and fake-tensor checks on a stride-1 identity block and a stride-2 block with
    convolutional residuals; the second output holds the frame sums of the first over tiles of four frames, pad joints zero.
    The 25-joint operator still accepts 25 joints only."""
    m = _model(V)
    blocks = f2v.FusedEvalJ(m)._packed(torch.device(DEV))
    x = make_input((2, 64, 11, V), seed=3).to(DEV)
    op = torch.ops.tamgcn.tcn_gcn_unit_eval_vj
    for b in (blocks[1], blocks[4]):
        torch.library.opcheck(op.default, (x, None, b.params, b.geom), test_utils=('test_schema', 'test_faketensor'))
    for b, shp in ((blocks[1], (2, 64, 11, V)), (blocks[4], (2, 128, 6, V))):
        out, xp = op(x, None, b.params, b.geom)
        T2 = shp[2]
        assert tuple(out.shape) == shp and tuple(xp.shape) == (2, (T2 + 3) // 4, shp[1], 20)
        assert float(xp[..., V:].abs().max()) == 0.0
        pad = torch.zeros(2, shp[1], (-T2) % 4, V, device=DEV)
        want = torch.cat((out, pad), 2).view(2, shp[1], -1, 4, V).sum(3).permute(0, 2, 1, 3)
        assert float((xp[..., :V] - want).abs().max()) <= 1e-6 * float(out.abs().max()) * 4
        nb = blocks[2] if b is blocks[1] else blocks[5]
        o1, _ = op(out, xp, nb.params, nb.geom)
        o2, _ = op(out, None, nb.params, nb.geom)
        assert _rel(o1, o2) <= 1e-5
    with pytest.raises(RuntimeError, match='25'):
        torch.ops.tamgcn.tcn_gcn_unit_eval_v25(x, None, blocks[1].params, blocks[1].geom)
    with pytest.raises(RuntimeError, match=r'17 \| 18 \| 25'):
        op(make_input((2, 64, 11, 19), seed=3).to(DEV), None, blocks[1].params, blocks[1].geom)


# ---------------------------------------------------------------------------------------------------------------------
# StreamEnsemble: the grouped pass
# ---------------------------------------------------------------------------------------------------------------------
STREAMS = ['joint', 'bone', 'motion', 'bone_motion']


@functools.lru_cache(maxsize=None)
def _streams_models(V, G):
    """G models of one geometry: the settled model, every floating-point parameter of model g scaled by 1 + 0.02 u (seed g)."""
    base = _model(V)
    out = []
    for g in range(G):
        mg = copy.deepcopy(base)
        gen = torch.Generator().manual_seed(g)
        with torch.no_grad():
            for p in mg.parameters():
                p.mul_((1 + 0.02 * (2 * torch.rand(p.shape, generator=gen) - 1)).to(DEV))
        out.append(mg.eval())
    return tuple(out)


@pytest.mark.parametrize('V, G, shapes', [(17, 4, ((1, 3, 16, 17, 1), (2, 3, 16, 17, 1))), (18, 2, ((1, 3, 16, 18, 2),))], ids=['coco_x4', 'openpose_x2'])
def test_stream_ensemble_runs_as_one_grouped_pass(V, G, shapes):
    models = _streams_models(V, G)
    streams = STREAMS[:G]
    ens = StreamEnsemble(models, streams, arrangement='grouped')
    assert type(ens._eng.engines[0]) is f2v.FusedEvalJ
    parent = torch.tensor(default_parent(models[0].graph), dtype=torch.int32, device=DEV)
    fast = GraphedForward(ens)
    for shape in shapes:
        x = make_input(shape, seed=1).to(DEV)
        (fused, pred, scores), cnt = _counted(lambda: ens.predict(x))
        assert sum(n.startswith('tamgcn_f2v_') and n.endswith('_grouped') for n in cnt.names) == 50
        assert cnt.names.count('tamgcn_stem_streams_eval') == 1 and 'tamgcn_stream_derive' not in cnt.names
        with torch.no_grad():
            own = torch.stack([f2v.FusedEvalJ(m)(ops.stream_derive(x, parent, s)) for m, s in zip(models, streams)])
            with _general():
                gen = torch.stack([m(ops.stream_derive(x, parent, s)) for m, s in zip(models, streams)])
        assert torch.equal(scores, own), float((scores - own).abs().max())     # each model's own small-batch pass, bit for bit
        assert torch.equal(fused, ops.score_fuse(own, ens.weights, False)[0])
        print(f'\nV={V} {shape}: grouped vs general ' + ' '.join(f'{_rel(scores[g], gen[g]):.2e}' for g in range(G)))
        for g in range(G):
            assert _rel(scores[g], gen[g]) <= 2e-5, g
        assert torch.equal(fast(x).clone(), fused)                               # capturable: replay = eager
        assert torch.equal(fast(x).clone(), fused)
