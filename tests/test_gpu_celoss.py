"""-m gpu: the cross-entropy with torch's options (csrc/celoss.hip; torch.ops.tamgcn.cross_entropy_opts) against its fp64
restatement (tests/celoss_ref.py, itself held to torch.nn.functional.cross_entropy by tests/test_celoss_ref_cpu.py) at the bars
derived there: every option combination at the smallest shapes where the launch geometry changes, shifted logits, bad labels,
all rows ignored, the exact facts (bit-zero rows, K = 1, one-product backward), two runs bit-equal, the registration, and a
CapturedStep whose replays follow labels that change the normaliser.

Run with -s to see the largest err / bound ratio of every shape."""
import os
import sys

import pytest
import torch

import celoss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(p, backward=None):
    """(loss, g [, dlogits for the upstream gradient `backward`]) of problem p through the registered op"""
    from tam_gcn_amd import torch_ops  # noqa: F401
    logits = _dev(p['logits'])
    target = _dev(p['labels'] if p.get('labels') is not None else p['probs'])
    args = (target, _dev(p.get('weight')), p['ignore_index'], p['eps'], p['reduction'])
    if backward is None:
        return torch.ops.tamgcn.cross_entropy_opts(logits, *args)
    logits.requires_grad_(True)
    loss, g = torch.ops.tamgcn.cross_entropy_opts(logits, *args)
    loss.backward(_dev(backward))
    return loss.detach(), g, logits.grad


def _hold(shape, options, worst, **kw):
    for o in options:
        p = R.problem(*shape, **o, **kw)
        loss, g = _run(p)
        rat = R.verify(f'{shape} {R.option_name(o)} {kw}', p, dict(loss=loss, g=g))
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: f'N{s[0]}_K{s[1]}')
def test_every_option_against_the_restatement(shape):
    worst = {}
    _hold(shape, R.options_of(shape), worst)
    print(f'\n  {shape}: {len(R.options_of(shape))} option combinations, max err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('shape', [(5, 10), (257, 65), (4, 400), (1025, 3)], ids=lambda s: f'N{s[0]}_K{s[1]}')
def test_shifted_logits(shape):
    """+60 and one row spanning -80 .. 80: the max-shift (most of that row's exponentials underflow to 0)"""
    worst = {}
    _hold(shape, R.OPTIONS if shape == (5, 10) else R.options_of(shape), worst, logits='shifted')
    print(f'\n  {shape} shifted: max err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('labels', ['bad', 'allign'])
@pytest.mark.parametrize('shape', [(5, 3), (257, 10), (4, 130)], ids=lambda s: f'N{s[0]}_K{s[1]}')
def test_bad_label_and_all_rows_ignored(shape, labels):
    """bad: the reduced loss is NaN, with 'none' only that row's; its row of g is bit-zero and the other rows are held as ever
    (they divide by a W without it).  allign: mean NaN, sum 0, none all zeros, g all zeros -- all exact."""
    index = [o for o in R.OPTIONS if o['target'] == 'index']
    _hold(shape, index, {}, labels=labels)
    for red in R.REDUCTIONS:
        p = R.problem(*shape, eps=0.1, weight='uniform', reduction=red, labels=labels)
        loss, g = _run(p)
        if labels == 'allign':
            assert bool((g == 0).all())
            assert bool(torch.isnan(loss)) if red == 'mean' else bool((loss == 0).all())
        else:
            bad = min(2, shape[0] - 1)
            assert bool((g[bad] == 0).all()) and bool(torch.isnan(loss[bad] if red == 'none' else loss))
            if red == 'none':
                assert int(torch.isnan(loss).sum()) == 1


def test_all_kept_weights_zero_is_nan_as_torch():
    for eps in (0.0, 0.1):
        p = R.problem(257, 10, weight='allzero', eps=eps)
        loss, g = _run(p)
        assert bool(torch.isnan(loss))
        R.verify('allzero', p, dict(loss=loss, g=g))
        p = R.problem(257, 10, weight='zeros', eps=eps, labels='valid')      # kept rows of weight 0 among classes that have one
        p['labels'] = p['labels'] // 3 * 3
        loss, g = _run(p)
        assert bool(torch.isnan(loss)) and R.ce_opts(p).w_zero
        R.verify('kept weights zero', p, dict(loss=loss, g=g))
        p = R.problem(257, 10, weight='allzero', eps=eps, reduction='sum')
        loss, g = _run(p)
        assert float(loss) == 0.0 and bool((g == 0).all())


def test_eps_zero_never_forms_zero_times_infinity():
    p = R.problem(6, 5, weight='zeros', labels='valid')
    p['logits'] = p['logits'].clone()
    p['logits'][:, 0] = float('-inf')                                        # w_0 = 0 and -logp_0 = inf
    p['labels'] = p['labels'].clamp_min(1)
    for red in R.REDUCTIONS:
        p['reduction'] = red
        loss, g = _run(p)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
        R.verify('-inf logit', p, dict(loss=loss, g=g))


@pytest.mark.parametrize('reduction', R.REDUCTIONS)
def test_entry_point_writes_its_outputs_and_nothing_else(reduction):
    """tamgcn_ce_opts_fwd on the library directly, a bad label and ignored rows among the labels: loss, g and the workspace sit
    inside buffers pre-filled with a sentinel whose floats behind the outputs must keep it; the launched kernel is reported."""
    import ctypes as C
    from tam_gcn_amd import _lib
    lib = _lib.load()
    GUARD, SENT = 8, -7.25
    for shape in ((5, 3), (257, 65), (1025, 3)):
        N, K = shape
        p = R.problem(N, K, weight='uniform', eps=0.1, reduction=reduction, labels='bad')
        nl = N if reduction == 'none' else 1
        loss = torch.full((nl + GUARD,), SENT, device=DEV)
        g = torch.full((N * K + GUARD,), SENT, device=DEV)
        ws = torch.full((N + GUARD,), SENT, device=DEV, dtype=torch.float64)
        logits, labels, w = _dev(p['logits']), _dev(p['labels']), _dev(p['weight'])
        d = _lib.CeDesc()
        d.logits, d.labels, d.weight = logits.data_ptr(), labels.data_ptr(), w.data_ptr()
        d.ignore_index, d.label_smoothing, d.reduction, d.N, d.K = -100, 0.1, R.REDUCTIONS.index(reduction), N, K
        assert lib.tamgcn_ce_opts_workspace_bytes(C.byref(d)) == (0 if reduction == 'none' else 8 * N)
        rc = lib.tamgcn_ce_opts_fwd(C.byref(d), loss.data_ptr(), g.data_ptr(), ws.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.tamgcn_last_error()
        assert lib.tamgcn_last_kernel() == (b'ce_opts_rows_kernel' if reduction == 'none' else b'ce_opts_finish_kernel')
        torch.cuda.synchronize()
        assert bool((loss[nl:] == SENT).all()) and bool((g[N * K:] == SENT).all()) and bool((ws[N:] == SENT).all())
        if reduction == 'none':
            assert bool((ws == SENT).all())                                  # no workspace use at all
        R.verify(f'direct {shape} {reduction}', p, dict(loss=loss[:nl].view(nl if reduction == 'none' else ()).clone(), g=g[:N * K].view(N, K)))


@pytest.mark.parametrize('reduction', R.REDUCTIONS)
def test_backward_is_one_product(reduction):
    gen = torch.Generator().manual_seed(7)
    for shape in ((5, 3), (257, 10), (3, 130)):
        for target in ('index', 'prob'):
            p = R.problem(*shape, target=target, weight='uniform', eps=0.1, reduction=reduction)
            dloss = torch.randn((shape[0],) if reduction == 'none' else (), generator=gen)
            _, g, dl = _run(p, backward=dloss)
            R.verify_bwd(f'{shape} {target} {reduction}', reduction, g, dloss, dl)
    from tam_gcn_amd import ops
    g = torch.randn(51, 5, generator=gen).to(DEV)                            # the entry point itself, N K = 255: a partly empty workgroup
    dloss = torch.randn(51, generator=gen).to(DEV)
    R.verify_bwd('rows', 'none', g, dloss, ops.ce_opts_bwd_rows(g, dloss))


def test_default_arguments_keep_the_existing_op_bit_for_bit():
    from tam_gcn_amd.functional import CrossEntropyLoss
    for shape in ((257, 10), (5, 65)):
        p = R.problem(*shape)
        ref_l = _dev(p['logits']).requires_grad_(True)
        ref, _ = torch.ops.tamgcn.cross_entropy(ref_l, _dev(p['labels']))
        ref.backward()
        l = _dev(p['logits']).requires_grad_(True)
        loss = CrossEntropyLoss()(l, _dev(p['labels']))
        loss.backward()
        assert torch.equal(loss, ref) and torch.equal(l.grad, ref_l.grad)
        # the new op on the same arguments is another summation order: equal within the bars, not bit for bit
        lo, g = _run(p)
        R.verify('default options', p, dict(loss=lo, g=g))
        assert abs(float(lo) - float(ref.detach())) <= 2 * float(R.ce_opts(p).loss_tol)


def test_two_runs_are_bit_equal():
    for shape, o in (((1025, 3), dict(weight='uniform', eps=0.1)), ((257, 400), dict(weight='zeros', eps=0.1, reduction='sum')),
                     ((257, 400), dict(target='prob', weight='uniform', eps=0.1)), ((256, 65), dict(reduction='none', ignore=0))):
        p = R.problem(*shape, **o)
        a = [t.clone() for t in _run(p)]
        torch.empty(1 << 20, device=DEV).normal_()                           # other work in between
        b = _run(p)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), (shape, o)


def test_module_follows_its_arguments_and_moves_its_weight():
    from tam_gcn_amd.functional import CrossEntropyLoss
    p = R.problem(257, 10, weight='uniform', eps=0.1, ignore=0)
    ce = CrossEntropyLoss(weight=p['weight'], ignore_index=0, label_smoothing=0.1)
    with pytest.raises(RuntimeError, match='weight must be'):
        ce(_dev(p['logits']), _dev(p['labels']))                             # the buffer is still on the CPU
    ce = ce.to(DEV)
    l = _dev(p['logits']).requires_grad_(True)
    loss = ce(l, _dev(p['labels']))
    loss.backward()
    R.verify('module', p, dict(loss=loss.detach(), g=l.grad))
    with pytest.raises(RuntimeError, match='weight must be'):
        ce(_dev(R.problem(5, 65)['logits']), _dev(R.problem(5, 65)['labels']))            # K = 65 against 10 weights
    pp = R.problem(257, 10, target='prob', reduction='none')
    with pytest.raises(RuntimeError, match='no gradient'):
        CrossEntropyLoss(reduction='none')(_dev(pp['logits']), _dev(pp['probs']).requires_grad_(True))
    out = CrossEntropyLoss(reduction='none')(_dev(pp['logits']), _dev(pp['probs']))
    assert tuple(out.shape) == (257,)


def test_registration():
    from tam_gcn_amd import torch_ops  # noqa: F401
    from tam_gcn_amd.functional import CrossEntropyLoss
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    p = R.problem(5, 10, weight='uniform', eps=0.1)
    for red in R.REDUCTIONS:
        logits = _dev(p['logits']).requires_grad_(True)
        torch.library.opcheck(torch.ops.tamgcn.cross_entropy_opts.default, (logits, _dev(p['labels']), _dev(p['weight']), -100, 0.1, red),
                              test_utils=utils)
    pp = R.problem(5, 10, target='prob')
    torch.library.opcheck(torch.ops.tamgcn.cross_entropy_opts.default,
                          (_dev(pp['logits']).requires_grad_(True), _dev(pp['probs']), None, -100, 0.0, 'mean'), test_utils=utils)
    g = torch.ops.tamgcn.cross_entropy_opts(_dev(p['logits']), _dev(p['labels']), None, -100, 0.0, 'none')[1]
    torch.library.opcheck(torch.ops.tamgcn.cross_entropy_opts_backward.default, (g, torch.ones(5, device=DEV), 'none'),
                          test_utils=('test_schema', 'test_faketensor'))
    ce = CrossEntropyLoss(weight=p['weight'], label_smoothing=0.1).to(DEV)

    def f(x, lab):
        return ce(x * 2.0, lab)                                              # torch.ops.tamgcn.cross_entropy_opts

    x = _dev(p['logits']).requires_grad_(True)
    eager = f(x, _dev(p['labels']))
    compiled = torch.compile(f, backend='eager', fullgraph=True)(x, _dev(p['labels']))       # fullgraph: any graph break raises
    assert torch.equal(eager, compiled)
    compiled.backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


# ---------------------------------------------------------------------------------------------------------------------
# the captured step
# ---------------------------------------------------------------------------------------------------------------------
MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
SHAPE = (8, 3, 16, 20, 1)                                                    # a short N-UCLA clip batch


def _setup():
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    return m, arena, bucket, FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)


def _batches():
    """four batches whose kept count and W all differ: 8, 5, 2 and 6 kept rows"""
    from params import make_input, make_labels
    out = []
    for i, ignored in enumerate(((), (0, 3, 6), (0, 1, 2, 3, 4, 5), (2, 7))):
        y = make_labels(SHAPE[0], 10, 200 + i)
        y[list(ignored)] = -100
        out.append((make_input(SHAPE, 30 + i).to(DEV), y.to(DEV)))
    return out


@pytest.mark.parametrize('accum', [1, 2])
def test_captured_step_equals_eager_and_follows_the_labels(accum):
    """CapturedStep with label smoothing, class weights and ignored rows, graphs against eager=True, bit for bit after every
    step: losses, parameters, optimiser steps.  The labels of every replay keep another number of rows, so the normaliser W the
    graph divides by has to be the replay's own, read on the device: the eager form computes it from the labels at hand."""
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    batches = _batches()
    w = R.problem(8, 10, weight='uniform')['weight']
    runs = {}
    for mode in ('graph', 'eager'):
        m, arena, bucket, opt = _setup()
        ce = CrossEntropyLoss(weight=w, label_smoothing=0.1).to(DEV)
        step = CapturedStep(m, ce, opt, arena, bucket, *batches[0], eager=(mode == 'eager'), accum_steps=accum)
        losses, flats = [], []
        for x, y in batches:
            losses.append(step.step(x, y).clone())
            flats.append(arena.flat.clone())
        torch.cuda.synchronize()
        runs[mode] = (torch.stack(losses).cpu(), [f.cpu() for f in flats], opt.state_dict()['step'])
    g, e = runs['graph'], runs['eager']
    assert g[2] == e[2] == len(batches) // accum
    assert torch.equal(g[0], e[0]), (g[0], e[0])
    assert len(set(g[0].tolist())) == len(batches)                           # the loss followed the labels
    assert all(torch.equal(a, b) for a, b in zip(g[1], e[1]))
    assert not torch.equal(g[1][-1], g[1][0])                                # and the parameters moved

