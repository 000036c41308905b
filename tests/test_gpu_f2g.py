"""-m gpu: the run-time-V small-batch eval family at the model level (csrc/f2g.hip; tam_gcn_amd/f2g.py: FusedEvalG,
tamgcn::tcn_gcn_unit_eval_vg; Model._f2g) -- synthetic-graph models of 16 joints (one person: no pad columns), 21 joints (two
persons: one live lane in a frame's last piece) and 28 joints (one person: the LDS edge), seeded parameters, running statistics
settled by one momentum-1 train-mode pass on inputs of their own.

Bars (the project's own, tests/test_gpu_f2j.py; none is fitted to this code): every block, fed the fp64 oracle's own input for
that block (teacher-forced), within 4 x 1.21e-6 of max|ref|; logits within 1e-4 max|ref| of the fp64 oracle with the same arg
max; logits and features within 2e-5 (relative) of the general eval path (TAMGCN_F2=0).  `pytest -s` prints the measured ratios
beside the error of an fp32 torch evaluation of the same blocks."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from params import fill_state_, make_input                                        # noqa: E402
from tam_gcn_amd import f2g, ops, _lib                                              # noqa: E402
from tam_gcn_amd.inference import GraphedForward, StreamEnsemble, default_parent  # noqa: E402
from tam_gcn_amd.models import ctrgcn as M                                          # noqa: E402
from oracle import ctrgcn_oracle as O                                               # noqa: E402

DEV = 'cuda:0'
PERSONS = {16: 1, 21: 2, 28: 1}
PARAM_SEED = 42
BLOCK_BAR = 4 * 1.21e-6


def _margs(V, num_person=None):
    return dict(num_class=9, num_point=V, num_person=num_person or PERSONS[V], graph='tam_gcn_amd.graph.synthetic.Graph',
                graph_args=dict(num_node=V, arity=2))


@functools.lru_cache(maxsize=None)
def _settled_state(V, num_person):
    """CPU state of the model with running statistics of its own inputs (one momentum-1 pass in train mode)."""
    m = M.Model(**_margs(V, num_person))
    fill_state_(m.state_dict(), seed=PARAM_SEED)
    m = m.to(DEV).train()
    for b in m.modules():
        if isinstance(b, torch.nn.modules.batchnorm._BatchNorm):
            b.momentum = 1.0
    with torch.no_grad():
        m(make_input((8 // num_person, 3, 16, V, num_person), seed=5).to(DEV))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _model(V, num_person=None):
    num_person = num_person or PERSONS[V]
    m = M.Model(**_margs(V, num_person))
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


def _spy(monkeypatch):
    calls = []
    real = f2g.FusedEvalG.blocks
    monkeypatch.setattr(f2g.FusedEvalG, 'blocks', lambda self, x: (calls.append(1), real(self, x))[1])
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# every block, teacher-forced on the fp64 oracle's input for that block
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 13, 16, 1), (1, 3, 20, 21, 2), (1, 3, 30, 21, 1), (1, 3, 13, 28, 1)]


@pytest.mark.parametrize('shape', SHAPES, ids=['v16_t13_two_clips', 'v21_t20_two_persons', 'v21_t30_one_person', 'v28_t13'])
def test_every_block_against_the_fp64_oracle(shape):
    """Frames per depth 13 -> 7 -> 4, 20 -> 10 -> 5 and 30 -> 15 -> 8: ragged last tiles of 1, 2 and 3 frames, odd T under stride
    2, one and two persons; at 28 joints l8..l10 (Cin = 256) take the 112-row K chunks and the two-phase E builder."""
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
    eng = f2g.FusedEvalG(m)
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


@pytest.mark.parametrize('shape', [(2, 3, 13, 16, 1), (1, 3, 20, 21, 2), (1, 3, 13, 28, 1)], ids=['v16', 'v21', 'v28'])
def test_model_forward_against_the_general_path(shape, monkeypatch):
    """Through Model.forward and extract_feature, in both input forms: the family within 2e-5 (relative) of the general path
    (TAMGCN_F2=0: no engine is built), logits and features."""
    V = shape[3]
    m = _model(V)
    x = make_input(shape, seed=21).to(DEV)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        with _general():
            b = m(x)
            fb, _ = m.extract_feature(x)
        assert not calls and not m.__dict__.get('_tamgcn_f2g'), 'TAMGCN_F2=0 is the general eval path'
        a = m(x)
        fa, _ = m.extract_feature(x)
        assert len(calls) == 2 and isinstance(m.__dict__.get('_tamgcn_f2g'), f2g.FusedEvalG)
        for slot in ('_tamgcn_f2', '_tamgcn_f2v', '_tamgcn_f2j'):
            assert not m.__dict__.get(slot), slot
        print(f'\n{shape}: family vs general logits {_rel(a, b):.2e}, features {_rel(fa, fb):.2e}')
        assert _rel(a, b) <= 2e-5
        assert fa.shape == fb.shape and _rel(fa, fb) <= 2e-5
        if shape[4] == 1:                                       # the (N, T, V*C) input form
            x3 = x[..., 0].permute(0, 2, 3, 1).reshape(shape[0], shape[2], V * 3).contiguous()
            a3 = m(x3)
            assert len(calls) == 3 and torch.equal(a3, a)


# ---------------------------------------------------------------------------------------------------------------------
# slack and alignment of the contiguous block input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [1, 4], ids=['identity', 'stride2_conv'])
@pytest.mark.parametrize('V', [21, 22, 23, 28])
def test_nan_before_the_input_and_in_its_slack_reaches_nothing(V, which):
    """The input is a slice of a NaN-filled buffer: NaN in front of it (the slice starts 3 floats in: dword-aligned only) and in
    the 4 slack floats behind it, which the last 16-byte piece of the last frame reads (3, 2, 1 and none of them).  Same bits
    as on a clean copy."""
    b = f2g.FusedEvalG(M.Model(**_margs(V, 1)).to(DEV).eval())._packed(torch.device(DEV))[which]
    data = make_input((2, 64, 7, V), seed=3).to(DEV)
    n = data.numel()
    buf = torch.full((3 + n + 4,), float('nan'), device=DEV)
    buf[3:3 + n] = data.view(-1)
    dirty = buf[3:3 + n].view(data.shape)
    assert dirty.data_ptr() % 16 == 12 and bool(torch.isnan(buf[3 + n:]).all())
    op = torch.ops.tamgcn.tcn_gcn_unit_eval_vg
    clean, cxp = op(data, None, b.params, b.geom)
    got, gxp = op(dirty, None, b.params, b.geom)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gxp).all())
    assert torch.equal(got, clean) and torch.equal(gxp, cxp)
    assert bool(torch.isnan(buf[:3]).all()) and bool(torch.isnan(buf[3 + n:]).all())
    assert torch.equal(buf[3:3 + n], data.view(-1))


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [16, 21])
def test_model_forward_routes_small_eval_batches_here(V, monkeypatch):
    m = _model(V)
    P = PERSONS[V]
    T = 8
    x = make_input((1, 3, T, V, P), seed=2).to(DEV)
    calls = _spy(monkeypatch)
    with torch.no_grad():
        m(x)
        m.extract_feature(x)
        assert len(calls) == 2
        assert m._f2(x) is None and m._f2v(x) is None and m._f2j(x) is None and isinstance(m._f2g(x), f2g.FusedEvalG)
        for slot in ('_tamgcn_f2', '_tamgcn_f2v', '_tamgcn_f2j'):
            assert not m.__dict__.get(slot), slot
        monkeypatch.setattr(f2g, 'F2G_MAX_FRAMES', 4 * P * T)
        big = make_input((5, 3, T, V, P), seed=3).to(DEV)
        assert m._f2g(big[:-1]) is not None and m._f2g(big) is None
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


def test_refolds_after_a_parameter_edit_and_after_load_state_dict():
    V, P = 21, 2
    m = _model(V)
    x = make_input((1, 3, 20, V, P), seed=21).to(DEV)
    a0 = _pair(m, x)
    assert m.__dict__.get('_tamgcn_f2g')
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


# ---------------------------------------------------------------------------------------------------------------------
# graph replay, launch count, the operator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [16, 21])
def test_graph_replay_and_launch_count(V):
    """GraphedForward captures this path: replay = eager bit for bit at batch 1 and batch 4, two eager runs are bit-equal, the
    capture keeps the folded weights of the engine alive; 50 family launches per forward and at most 56 ABI launches in all."""
    m = _model(V)
    P = PERSONS[V]
    fast = GraphedForward(m)
    for shape in ((1, 3, 13, V, P), (4, 3, 20, V, P)):
        x = make_input(shape, seed=shape[2]).to(DEV)
        with torch.no_grad():
            ref = m(x)
            assert torch.equal(m(x), ref)
        assert torch.equal(fast(x).clone(), ref)
        assert torch.equal(fast(x).clone(), ref)
    eng = m.__dict__['_tamgcn_f2g']
    assert isinstance(eng, f2g.FusedEvalG)
    assert all(any(k is eng._blocks for k in ent[3]) for ent in fast._graphs.values())
    _, cnt = _counted(lambda: m(make_input((1, 3, 20, V, P), seed=9).to(DEV)))
    assert cnt.n <= 56, (cnt.n, cnt.names)
    assert sum(n.startswith('tamgcn_f2g_') for n in cnt.names) == 50
    assert not any(n.startswith('tamgcn_f2_') or n.startswith('tamgcn_f2v_') for n in cnt.names)


@pytest.mark.parametrize('V', [16, 21, 26])
def test_block_is_a_registered_operator(V):
    """torch.ops.tamgcn.tcn_gcn_unit_eval_vg: schema and fake-tensor checks on a stride-1 identity block and a stride-2 block with
    convolutional residuals; the second output holds the frame sums of the first over tiles of four frames, pad joints zero."""
    VP = (V + 3) & ~3
    blocks = f2g.FusedEvalG(M.Model(**_margs(V, 1)).to(DEV).eval())._packed(torch.device(DEV))
    x = make_input((2, 64, 11, V), seed=3).to(DEV)
    op = torch.ops.tamgcn.tcn_gcn_unit_eval_vg
    for b in (blocks[1], blocks[4]):
        torch.library.opcheck(op.default, (x, None, b.params, b.geom), test_utils=('test_schema', 'test_faketensor'))
    for b, shp in ((blocks[1], (2, 64, 11, V)), (blocks[4], (2, 128, 6, V))):
        out, xp = op(x, None, b.params, b.geom)
        T2 = shp[2]
        assert tuple(out.shape) == shp and tuple(xp.shape) == (2, (T2 + 3) // 4, shp[1], VP)
        assert VP == V or float(xp[..., V:].abs().max()) == 0.0
        pad = torch.zeros(2, shp[1], (-T2) % 4, V, device=DEV)
        want = torch.cat((out, pad), 2).view(2, shp[1], -1, 4, V).sum(3).permute(0, 2, 1, 3)
        assert float((xp[..., :V] - want).abs().max()) <= 1e-6 * float(out.abs().max()) * 4
        nb = blocks[2] if b is blocks[1] else blocks[5]
        o1, _ = op(out, xp, nb.params, nb.geom)
        o2, _ = op(out, None, nb.params, nb.geom)
        assert _rel(o1, o2) <= 1e-5
    with pytest.raises(RuntimeError, match='8 <= V <= 28'):
        op(make_input((2, 64, 11, 7), seed=3).to(DEV), None, blocks[1].params, blocks[1].geom)


@pytest.mark.parametrize('V', [17, 20, 25])
def test_the_engine_serves_the_dedicated_joint_counts_too(V):
    """Not routed, but accepted: the run-time-V kernels against the general path at the joint counts f2 / f2v are built for."""
    m = _model(V, 1)
    x = make_input((1, 3, 13, V, 1), seed=4).to(DEV)
    with torch.no_grad():
        assert m._f2g(x) is None and '_tamgcn_f2g' not in m.__dict__
        a = f2g.FusedEvalG(m)(x)
        with _general():
            b = m(x)
    assert _rel(a, b) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# StreamEnsemble: no grouped pass for these joint counts -- the models' own routed forwards
# ---------------------------------------------------------------------------------------------------------------------
def test_stream_ensemble_equals_the_weighted_sum_of_the_routed_forwards(monkeypatch):
    V, P, G = 21, 2, 3
    base = _model(V)
    models = []
    for g in range(G):
        mg = copy.deepcopy(base)
        gen = torch.Generator().manual_seed(g)
        with torch.no_grad():
            for p in mg.parameters():
                p.mul_((1 + 0.02 * (2 * torch.rand(p.shape, generator=gen) - 1)).to(DEV))
        models.append(mg.eval())
    streams, weights = ['joint', 'bone', 'motion'], [1.0, 0.7, 0.4]
    ens = StreamEnsemble(models, streams, weights=weights)
    assert ens._eng is None                                  # f2.GroupedEval stays as it is: Unsupported for 21 joints
    parent = torch.tensor(default_parent(models[0].graph), dtype=torch.int32, device=DEV)
    x = make_input((1, 3, 16, V, P), seed=1).to(DEV)
    calls = _spy(monkeypatch)
    (fused, pred, scores), cnt = _counted(lambda: ens.predict(x))
    assert len(calls) == G and sum(n.startswith('tamgcn_f2g_') for n in cnt.names) == 50 * G
    assert all(isinstance(m.__dict__.get('_tamgcn_f2g'), f2g.FusedEvalG) for m in models)
    with torch.no_grad():
        own = torch.stack([m(ops.stream_derive(x, parent, s)) for m, s in zip(models, streams)])
    assert torch.equal(scores, own)
    want = sum(w * o for w, o in zip(weights, own))
    assert _rel(fused, want) <= 1e-6 and torch.equal(fused, ops.score_fuse(own, ens.weights, False)[0])
    assert torch.equal(pred.long(), fused.argmax(1))
