"""CapturedStep on the MI355X: graph replays equal the eager step bit for bit (losses, parameters, BatchNorm running
statistics) with a learning-rate change between steps; eval caches stay valid after replays; a wrong batch is refused
before anything is launched."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
B, T, V = 8, 52, 20


def _setup(kind='sgd', seed=0):
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD, FusedAdam
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=seed)
    m = m.to(DEV).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    if kind == 'sgd':
        opt = FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
    else:
        opt = FusedAdam(arena, bucket, lr=1e-3, weight_decay=1e-4)
    return m, arena, bucket, opt


def _batches(k, seed=3):
    from params import make_input, make_labels
    return [(make_input((B, 3, T, V, 1), seed + i).to(DEV), make_labels(B, 10, seed + 100 + i).to(DEV)) for i in range(k)]


def _bn_state(m):
    return [t.clone() for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)
            for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]


LR2 = {'sgd': 0.01, 'adam': 2e-4}          # the learning rate from step 3 on


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_captured_step_equals_eager_bit_for_bit(kind):
    """4 CapturedStep replays with opt.lr changed after step 2 == CapturedStep(eager=True) == a plain eager loop
    (model -> functional.CrossEntropyLoss -> backward -> bucket.pack() -> opt.step()): losses, arena.flat and every
    BatchNorm running statistic, bit for bit."""
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    batches = _batches(4)
    runs = {}
    for mode in ('graph', 'eager_step', 'plain'):
        m, arena, bucket, opt = _setup(kind)
        ce = CrossEntropyLoss()
        before = (arena.flat.clone(), _bn_state(m))
        step = None
        if mode != 'plain':
            step = CapturedStep(m, ce, opt, arena, bucket, *batches[0], eager=(mode == 'eager_step'))
            torch.cuda.synchronize()
            # building the step (warm-up steps included) leaves the model and the optimiser as they were
            assert torch.equal(arena.flat, before[0]), mode
            assert all(torch.equal(a, b) for a, b in zip(_bn_state(m), before[1])), mode
            assert opt.state_dict()['step'] == 0
        losses = []
        for k, (x, y) in enumerate(batches):
            if k == 2:
                opt.lr = LR2[kind]
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
        assert not torch.equal(arena.flat, before[0])
        runs[mode] = (torch.stack(losses).cpu(), arena.flat.cpu(), [t.cpu() for t in _bn_state(m)], opt.state_dict()['step'])
    ref = runs['plain']
    assert ref[3] == 4
    for mode in ('graph', 'eager_step'):
        got = runs[mode]
        assert torch.equal(got[0], ref[0]), (mode, got[0], ref[0])
        assert torch.equal(got[1], ref[1]), (mode, float((got[1] - ref[1]).abs().max()))
        assert len(got[2]) == len(ref[2]) > 0
        for i, (a, b) in enumerate(zip(got[2], ref[2])):
            assert torch.equal(a, b), (mode, i)
        assert got[3] == 4


def _eval2(m, x):
    m.eval()
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    return out.clone()


def test_eval_after_replayed_steps_is_not_stale():
    """Replays run no Python: CapturedStep bumps the arena epoch and the BatchNorm update counters itself, so the folded
    eval caches (f2.FusedEval here: 2 clips) are rebuilt.  The eval forward after 3 more replayed steps equals that of a
    freshly built model loaded with the trained state, bit for bit."""
    from tam_gcn_amd import f2
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.training import CapturedStep
    m, arena, bucket, opt = _setup('sgd', seed=1)
    batches = _batches(4, seed=40)
    step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, *batches[0])
    step.step(*batches[0])
    xe = batches[1][0][:2].contiguous()
    first = _eval2(m, xe)
    assert isinstance(m.__dict__.get('_tamgcn_f2'), f2.FusedEval)        # the small-batch eval engine served it
    m.train()
    for x, y in batches[1:]:
        step.step(x, y)
    out = _eval2(m, xe)
    fresh = Model(**MARGS)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    fresh = fresh.to(DEV).eval()
    ParamArena(fresh)
    ref = _eval2(fresh, xe)
    assert not torch.equal(first, ref)                                 # the steps changed the model
    assert torch.equal(out, ref), float((out - ref).abs().max())


def test_wrong_batch_is_refused_before_any_launch():
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    m, arena, bucket, opt = _setup('sgd', seed=2)
    (x, y), = _batches(1, seed=60)
    step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y)
    torch.cuda.synchronize()
    flat, xs, bn = arena.flat.clone(), step.x.clone(), _bn_state(m)
    epoch = arena.epoch
    bad = [(x[:4], y[:4]), (x[:, :, :40].contiguous(), y), (x.double(), y), (x, y.int()), (x, y[:4])]
    for bx, by in bad:
        with pytest.raises(ValueError, match='CapturedStep'):
            step.step(bx, by)
    torch.cuda.synchronize()
    assert torch.equal(arena.flat, flat) and torch.equal(step.x, xs) and arena.epoch == epoch
    assert all(torch.equal(a, b) for a, b in zip(_bn_state(m), bn))
    assert opt.state_dict()['step'] == 0
    step.step(x, y)                                                    # the right batch still runs
    torch.cuda.synchronize()
    assert opt.state_dict()['step'] == 1 and not torch.equal(arena.flat, flat)
