"""-m gpu: models on skeletons CTRGC has no dedicated kernels for (route 'vgen', csrc/vgen.hip): COCO's 17 joints, OpenPose's
18, a 7-joint synthetic tree -- blocks teacher-forced against the fp64 oracle at tests/test_gpu_blocks.py's bars, whole models
against the fp64 oracle at tests/test_gpu_model.py's bars, the captured paths (GraphedForward, CapturedStep, CapturedEval)
against their eager forms, ST-GCN on OpenPose against oracle/stgcn_oracle.py, and the routes of V = 20 / 25 unmoved.

The oracle is pinned to the reference at V = 17 by tests/test_oracle_vs_golden_vgen.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evalmeter_ref as ER                                                        # noqa: E402
import test_gpu_blocks as TB                                                      # noqa: E402
from cases import tag_seed                                                        # noqa: E402
from params import fill_state_, make_input, make_labels                           # noqa: E402
from tam_gcn_amd.graph import coco, openpose                                       # noqa: E402
from tam_gcn_amd.models import ctrgcn as M                                          # noqa: E402
from oracle import ctrgcn_oracle as O                                               # noqa: E402

DEV = torch.device('cuda:0')
COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
OPENPOSE = dict(num_class=12, num_point=18, num_person=2, graph='tam_gcn_amd.graph.openpose.Graph', graph_args=dict(labeling_mode='spatial'))
TREE7 = dict(num_class=6, num_point=7, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=7, arity=2))
MODEL_CASES = [('coco_t13', COCO, (4, 3, 13, 17, 1)), ('openpose_t20', OPENPOSE, (2, 3, 20, 18, 2)), ('tree7_t8', TREE7, (2, 3, 8, 7, 1))]
PARAM_SEED, X_SEED, LABEL_SEED = 42, 21, 22


# ---------------------------------------------------------------------------------------------------------------------
# blocks, teacher-forced (tests/test_gpu_blocks.py's teacher, margins and bars)
# ---------------------------------------------------------------------------------------------------------------------
# (tag, index of the model block with this stride / residual in the oracle's layout, Cin, Cout)
BLOCKS = [('vblk_3_64_nores', 1, 3, 64), ('vblk_64_64', 2, 64, 64), ('vblk_64_128_s2', 5, 64, 128)]
_TEACHERS = {}


def _teacher(tag, i, cin, cout, training):
    key = (tag, training)
    if key not in _TEACHERS:
        blk = M.TCN_GCN_unit(cin, cout, coco.Graph().A, stride=O._STRIDES.get(i, 1), residual=(i != 1))
        fill_state_(blk.state_dict(), seed=tag_seed(tag))
        sd = {f'l{i}.{k}': (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in blk.state_dict().items()}
        x = make_input((2, cin, 13, 17), seed=16).double()
        T_out = 13 if i != 5 else 7
        cot = make_input((2, cout, T_out, 17), seed=777).double()
        assert x.shape[0] == TB.N_TEACH
        _TEACHERS[key] = (blk, sd, cot, TB._block_teacher(i, x, cot, sd, training))
    return _TEACHERS[key]


@pytest.mark.parametrize('bn', ['train', 'eval'])
@pytest.mark.parametrize('mode', [1, 0], ids=['split_bf16_bwd', 'exact_f32'])
@pytest.mark.parametrize('tag,i,cin,cout', BLOCKS, ids=[b[0] for b in BLOCKS])
def test_block_teacher_forced(tag, i, cin, cout, mode, bn):
    from tam_gcn_amd import _lib
    training = bn == 'train'
    blk0, sd, cot, (tx, ty, tdx, tgrads, tries) = _teacher(tag, i, cin, cout, training)
    blk = M.TCN_GCN_unit(cin, cout, coco.Graph().A, stride=O._STRIDES.get(i, 1), residual=(i != 1))
    blk.load_state_dict(blk0.state_dict())
    blk = blk.to(DEV).train(training)
    before = {k: b.detach().clone() for k, b in blk.named_buffers()}
    lib = _lib.load()
    prev = lib.tamgcn_get_split_mode()
    lib.tamgcn_set_split_mode(mode)
    failures = []
    try:
        xi = tx.float().to(DEV).contiguous().requires_grad_(True)
        out = blk(xi)
        out.backward(cot.float().to(DEV).contiguous())
        torch.cuda.synchronize()
    finally:
        lib.tamgcn_set_split_mode(prev)
    e = TB._rel(out, ty)
    print(f'{tag} mode {mode} bn {bn}: teacher nudges {tries}; out {e:.2e} dx {TB._rel(xi.grad, tdx):.2e}')
    if e > TB.REL_Y:
        failures.append(f'out {e:.2e}')
    e = TB._rel(xi.grad, tdx)
    if e > TB.REL_G[mode]:
        failures.append(f'dx {e:.2e}')
    for k, p in blk.named_parameters():
        ref = tgrads[k]
        assert p.grad is not None, f'{k}: no gradient'
        if k.endswith('bias') and float(ref.abs().max()) < 1e-9:                  # bias in front of a train-mode BatchNorm
            wk = k[:-4] + 'weight'
            scale = float(tgrads[wk].abs().max()) if wk in tgrads else 1.0
            if float(p.grad.abs().max()) > 1e-4 * max(scale, 1e-3):
                failures.append(f'{k} should be ~0, is {float(p.grad.abs().max()):.2e}')
            continue
        e = TB._rel(p.grad, ref)
        bar = TB.REL_G[mode]
        if mode == 1 and p.dim() == 1:
            bar = TB.REL_VEC_SPLIT
        if p.numel() == 1:
            bar = TB.REL_SCALAR
        elif k == 'tcn1.branches.2.1.weight':
            bar = TB.REL_SCALE_INV
        if e > bar:
            failures.append(f'{k} {e:.2e} > {bar:g}')
    assert not failures, f'{tag} mode {mode} bn {bn}: ' + '; '.join(failures[:40])
    if not training:
        assert all(torch.equal(b, before[k]) for k, b in blk.named_buffers()), 'running statistics changed in eval mode'


# ---------------------------------------------------------------------------------------------------------------------
# whole models against the fp64 oracle (tests/test_gpu_model.py's bars)
# ---------------------------------------------------------------------------------------------------------------------
def _flip_robust(name, got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    if float(ref.abs().max()) < 1e-12:
        assert float(got.abs().max()) < 1e-6, name
        return
    if got.numel() < 4:                                                           # a scalar (alpha): one heavily cancelling sum
        assert float((got - ref).abs().max()) <= 0.25 * float(ref.abs().max()) + 1e-12, f'{name}: {got} vs {ref}'
        return
    l2 = float((got - ref).norm() / (ref.norm() + 1e-30))
    cos = float((got * ref).sum() / (got.norm() * ref.norm() + 1e-30))
    assert l2 <= 5e-2 and cos >= 0.999, f'{name}: relative L2 {l2:.3e}, cosine {cos:.5f}'


def _model(margs):
    m = M.Model(**margs)
    fill_state_(m.state_dict(), seed=PARAM_SEED)
    return m


def _tree(V):
    return dict(num_class=5, num_point=V, num_person=1, graph='tam_gcn_amd.graph.synthetic.Graph', graph_args=dict(num_node=V, arity=2))


# the joint counts the three graphs above leave out: the ends of the range, both sides of the 16-joint tile, every residue mod 4
# (the pointwise / k x 1 GEMMs, tconv, BatchNorm, stem and head had only met V = 20, 25, 32 and 64)
OTHER_V = [(f'tree{V}_t8', _tree(V), (2, 3, 8, V, 1)) for V in (2, 3, 6, 15, 16, 23, 31)]


@pytest.mark.parametrize('case', MODEL_CASES, ids=lambda c: c[0])
def test_model_parity_against_the_fp64_oracle(case):
    _parity(*case)


@pytest.mark.parametrize('case', OTHER_V, ids=lambda c: c[0])
def test_model_parity_at_the_other_joint_counts(case):
    _parity(*case)


def _parity(tag, margs, shape):
    from tam_gcn_amd import ops
    V = margs['num_point']
    assert ops.ctrgc_route(V) == 'vgen'
    m = _model(margs)
    sd = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    pkeys = [k for k, _ in m.named_parameters()]
    for k in pkeys:
        sd[k].requires_grad_(True)
    xo = make_input(shape, seed=X_SEED).double().requires_grad_(True)
    lab = make_labels(shape[0], margs['num_class'], seed=LABEL_SEED)
    lo = O.model_forward(xo, sd, V, training=True)
    loss_o = torch.nn.functional.cross_entropy(lo, lab)
    loss_o.backward()

    m = m.to(DEV).train()
    x = make_input(shape, seed=X_SEED).to(DEV).requires_grad_(True)
    logits = m(x)
    loss = torch.nn.functional.cross_entropy(logits, lab.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    err = float((logits.detach().cpu().double() - lo.detach()).abs().max())
    print(f'{tag}: train logits max-abs err {err:.3e}, loss {float(loss.detach()):.6f} vs {float(loss_o.detach()):.6f}')
    assert err <= 1e-3
    assert torch.equal(logits.argmax(1).cpu(), lo.argmax(1))
    assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-3
    _flip_robust('dx', x.grad, xo.grad)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        _flip_robust(k, p.grad, sd[k].grad)
    for k, b in m.named_buffers():                                               # running statistics after the step
        if 'running_' in k:
            r = sd[k].detach()
            assert float((b.cpu().double() - r).abs().max()) <= 2e-4 * float(r.abs().max()) + 1e-6, k
        else:
            assert int(b) == int(sd[k]), k

    # eval mode under no_grad at batch 1, on running statistics that belong to these inputs (one momentum-1 pass)
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m(x.detach())
    for b in bns:
        b.momentum = 0.1
    sde = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}
    m.eval()
    x1 = x.detach()[:1].contiguous()
    with torch.no_grad():
        le = m(x1)
        ref = O.model_forward(x1.cpu().double(), sde, V, training=False)
    assert not m.__dict__.get('_tamgcn_f2') and not m.__dict__.get('_tamgcn_f2v'), 'a small-batch engine took a model outside its family'
    err = float((le.cpu().double() - ref).abs().max())
    print(f'{tag}: eval logits (batch 1) max-abs err {err:.3e}')
    assert err <= 1e-3 and torch.equal(le.argmax(1).cpu(), ref.argmax(1))


# ---------------------------------------------------------------------------------------------------------------------
# captured paths at V = 17
# ---------------------------------------------------------------------------------------------------------------------
B17, T17 = 4, 16


def _batches(k, seed=3):
    return [(make_input((B17, 3, T17, 17, 1), seed + i).to(DEV), make_labels(B17, 10, seed + 100 + i).to(DEV)) for i in range(k)]


def _setup():
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD
    m = _model(COCO).to(DEV).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    return m, arena, bucket, FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)


def _bn_state(m):
    return [t.clone() for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)
            for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]


def _settled_eval_model():
    """The COCO model in eval mode with running statistics of its own inputs (one momentum-1 pass)."""
    m = _model(COCO).to(DEV).train()
    bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m(make_input((8, 3, T17, 17, 1), seed=5).to(DEV))
    for b in bns:
        b.momentum = 0.1
    return m.eval()


def test_graphed_forward_equals_the_eager_forward():
    from tam_gcn_amd.inference import GraphedForward
    m = _settled_eval_model()
    fast = GraphedForward(m)
    for seed in (1, 2):
        for nb in (B17, 1):
            x = make_input((nb, 3, T17, 17, 1), seed=seed).to(DEV)
            with torch.no_grad():
                ref = m(x)
            got = fast(x).clone()
            assert torch.isfinite(ref).all() and torch.equal(got, ref), (seed, nb, float((got - ref).abs().max()))
    assert len(fast._graphs) == 2


def test_captured_step_equals_the_eager_sequence():
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    batches = _batches(3)
    runs = {}
    for mode in ('graph', 'plain'):
        m, arena, bucket, opt = _setup()
        ce = CrossEntropyLoss()
        start = arena.flat.clone()
        step = CapturedStep(m, ce, opt, arena, bucket, *batches[0]) if mode == 'graph' else None
        losses = []
        for x, y in batches:
            if step is not None:
                losses.append(step.step(x, y).clone())
            else:
                bucket.zero()
                loss = ce(m(x), y)
                loss.backward()
                bucket.pack()
                opt.step()
                losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        assert not torch.equal(arena.flat, start) and bool(torch.isfinite(arena.flat).all())
        runs[mode] = (torch.stack(losses).cpu(), arena.flat.cpu(), [t.cpu() for t in _bn_state(m)], opt.state_dict()['step'])
    g, r = runs['graph'], runs['plain']
    assert g[3] == r[3] == 3
    assert torch.equal(g[0], r[0]), (g[0], r[0])
    assert torch.equal(g[1], r[1]), float((g[1] - r[1]).abs().max())
    assert len(g[2]) == len(r[2]) > 0 and all(torch.equal(a, b) for a, b in zip(g[2], r[2]))


def test_captured_step_with_accumulation_equals_its_eager_form():
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    batches = _batches(4, seed=20)
    runs = {}
    for mode in ('graph', 'eager'):
        m, arena, bucket, opt = _setup()
        step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, *batches[0], eager=(mode == 'eager'), accum_steps=2)
        start = arena.flat.clone()
        losses, pend = [], []
        for k, (x, y) in enumerate(batches):
            losses.append(step.step(x, y).clone())
            pend.append(step.pending)
            torch.cuda.synchronize()
            if k == 0:
                assert torch.equal(arena.flat, start), mode
        assert pend == [1, 0, 1, 0] and opt.state_dict()['step'] == 2, (mode, pend)
        assert not torch.equal(arena.flat, start)
        runs[mode] = (torch.stack(losses).cpu(), arena.flat.cpu(), [t.cpu() for t in _bn_state(m)])
    g, e = runs['graph'], runs['eager']
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1]) and all(torch.equal(a, b) for a, b in zip(g[2], e[2]))


def test_captured_eval_on_a_synthetic_ten_clip_set():
    from tam_gcn_amd.evaluation import CapturedEval
    m = _settled_eval_model()
    n, B, K = 10, 4, 10
    xs = make_input((n, 3, T17, 17, 1), seed=31).to(DEV)
    labs = make_labels(n, K, seed=32).to(DEV)
    ev = CapturedEval(m, None, B, example_x=xs[:B].contiguous(), num_samples=n)
    ev.reset()
    ref = ER.Meter(K, num_samples=n, topk=(1, 5))
    scores = np.full((n, K), np.nan, dtype=np.float32)
    for b in range(0, n, B):
        idx = [i if i < n else 0 for i in range(b, b + B)]                       # the last batch padded with sample 0
        valid = min(B, n - b)
        it = torch.tensor(idx, device=DEV)
        x, y = xs[it].contiguous(), labs[it].contiguous()
        ev.update(x, y, index=it, valid=valid)
        with torch.no_grad():
            out = m(x).cpu().numpy()
        scores[b:b + valid] = out[:valid]
        ref.update(out, y.cpu().numpy(), index=np.asarray(idx), valid=valid)
    res = ev.meter.compute()
    assert np.isfinite(scores).all() and np.array_equal(res['scores'], scores), float(np.abs(res['scores'] - scores).max())
    ER.assert_same_metrics(res, ref.compute())
    assert res['count'] == n and res['bad_labels'] == 0 and res['bad_index'] == 0


# ---------------------------------------------------------------------------------------------------------------------
# ST-GCN on OpenPose
# ---------------------------------------------------------------------------------------------------------------------
def test_stgcn_on_openpose_against_its_oracle():
    """tests/test_gpu_stgcn.py::test_model_parity's bars with the oracle in place of the golden vectors."""
    from oracle import stgcn_oracle as SO
    from tam_gcn_amd.models import stgcn as SM
    from test_stgcn_oracle import fill_stgcn_
    margs = dict(in_channels=3, num_class=4, num_point=18, num_person=1, graph='tam_gcn_amd.graph.openpose.Graph',
                 graph_args=dict(labeling_mode='spatial'))
    shape = (2, 3, 20, 18, 1)
    m = SM.Model(**margs)
    fill_stgcn_(m.state_dict(), seed=77)
    assert tuple(m.state_dict()['A'].shape) == (3, 18, 18)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point() and 'running' not in k and k != 'A') for k, v in m.state_dict().items()}
    xo = make_input(shape, seed=21).requires_grad_(True)
    lab = make_labels(shape[0], margs['num_class'], seed=22)
    lo = SO.model_forward(xo, sd, 18, True)
    loss_o = torch.nn.functional.cross_entropy(lo, lab)
    loss_o.backward()
    m = m.to(DEV).train()
    x = make_input(shape, seed=21).to(DEV).requires_grad_(True)
    logits = m(x)
    loss = torch.nn.functional.cross_entropy(logits, lab.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    lg, ref = logits.detach().cpu().numpy(), lo.detach().numpy()
    assert np.abs(lg - ref).max() <= 1e-3 and np.array_equal(lg.argmax(1), ref.argmax(1))
    assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-3
    for k, p in m.named_parameters():
        if k.startswith('fcn.') or k.startswith('edge_importance'):
            g, r = p.grad.detach().cpu().double().numpy(), sd[k].grad.double().numpy()
            l2 = np.sqrt(((g - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + 1e-30)
            assert l2 <= (2e-3 if k.startswith('fcn.') else 5e-2), f'{k}: relative L2 {l2:.3e}'
    dx, rdx = x.grad.cpu().double().numpy(), xo.grad.double().numpy()
    assert np.sqrt(((dx - rdx) ** 2).sum()) / np.sqrt((rdx ** 2).sum()) <= 5e-2
    m.eval()
    with torch.no_grad():
        le = m(x.detach()).cpu().numpy()
        sde = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        re = SO.model_forward(x.detach().cpu(), sde, 18, False).numpy()
    assert np.abs(le - re).max() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# routes that must not have moved
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,want', [(25, 'ctrgc_agg_fwd_kernel<25, 3>'), (20, 'ctrgc_fwd')])
def test_dedicated_routes_keep_their_kernels(V, want):
    from tam_gcn_amd import _lib, ops
    g = torch.Generator().manual_seed(V)
    N, Cin, Cout, T, S, R = 2, 16, 16, 9, 3, 8
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(DEV)                  # noqa: E731
    x = ops.S(ops.with_slack(r(N, Cin, T, V)))
    y, part, x3 = ops.ctrgc_fwd(x, r(S * 2 * R, N, V), r(S * Cout, Cin) * 0.2, r(S, Cout) * 0.1, r(S, Cout, R) * 0.3, r(S, Cout) * 0.1,
                                r(S, V, V) * 0.3, torch.tensor([0.7], device=DEV), Cin, Cout, S, R, stats=True)
    torch.cuda.synchronize()
    sym = _lib.load().tamgcn_last_kernel().decode()
    assert sym.startswith(want), sym
    assert bool(torch.isfinite(y).all())
