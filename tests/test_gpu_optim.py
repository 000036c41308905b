"""tamgcn_optim_step and the fused optimisers on the MI355X: the kernel against float64 torch.optim, FusedSGD against
SGDNesterov on a real arena, graph replay with a learning rate changed between replays, and exact resume."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
STEPS = 10
BAR = 1e-6          # max |p - p64| <= BAR * max |p64|


def _flat_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.rand(n, generator=g) * 2 - 1
    grads = [torch.randn(n, generator=g) for _ in range(STEPS)]
    return p0, grads


def _kernel_run(p0, grads, mode, lr, **hyper):
    """STEPS updates through ops.optim_step on flat device buffers; returns p."""
    from tam_gcn_amd import ops
    n = p0.numel()
    p = p0.to(DEV)
    s0 = torch.zeros(n, device=DEV) if mode == 1 or hyper.get('momentum', 0) else None
    s1 = torch.zeros(n, device=DEV) if mode == 1 else None
    lr_t = torch.tensor([lr], device=DEV)
    step = torch.zeros(1, device=DEV, dtype=torch.int32)
    scal = torch.zeros(2, device=DEV)
    g = torch.empty(n, device=DEV)
    for k in range(STEPS):
        g.copy_(grads[k])
        ops.optim_step(p, g, s0, s1, lr_t, step, scal, mode, **hyper)
    torch.cuda.synchronize()
    assert int(step.item()) == STEPS
    return p.cpu()


def _torch64(p0, grads, opt_fn):
    p = torch.nn.Parameter(p0.double())
    opt = opt_fn([p])
    for k in range(STEPS):
        p.grad = grads[k].double()
        opt.step()
    return p.detach()


def _assert_bar(p, p64, what):
    err = float((p.double() - p64).abs().max())
    assert err <= BAR * float(p64.abs().max()), (what, err)


@pytest.mark.parametrize('n', [1_000_003, 4096], ids=['n1000003_tail', 'n4096'])
@pytest.mark.parametrize('nesterov,momentum,wd', [(True, 0.9, 0.0), (True, 0.9, 1e-4), (False, 0.9, 0.0), (False, 0.9, 1e-4),
                                                  (False, 0.0, 0.0), (False, 0.0, 1e-4)],
                         ids=['nesterov_wd0', 'nesterov_wd1e-4', 'plain_m0.9_wd0', 'plain_m0.9_wd1e-4', 'plain_m0_wd0', 'plain_m0_wd1e-4'])
def test_sgd_kernel_against_float64_torch(n, nesterov, momentum, wd):
    p0, grads = _flat_case(n, seed=n + int(momentum * 10) + int(nesterov))
    lr = 0.05
    p = _kernel_run(p0, grads, 0, lr, momentum=momentum, nesterov=nesterov, weight_decay=wd)
    p64 = _torch64(p0, grads, lambda ps: torch.optim.SGD(ps, lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=wd,
                                                         foreach=False))
    _assert_bar(p, p64, 'sgd')
    assert not torch.equal(p, p0)


def test_sgd_kernel_dampening_against_float64_torch():
    p0, grads = _flat_case(4099, seed=5)
    p = _kernel_run(p0, grads, 0, 0.05, momentum=0.9, dampening=0.3, weight_decay=1e-4)
    p64 = _torch64(p0, grads, lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9, dampening=0.3, weight_decay=1e-4,
                                                         foreach=False))
    _assert_bar(p, p64, 'sgd dampening')


@pytest.mark.parametrize('n', [1_000_003, 4096], ids=['n1000003_tail', 'n4096'])
@pytest.mark.parametrize('wd', [0.0, 1e-4], ids=['wd0', 'wd1e-4'])
def test_adam_kernel_against_float64_torch(n, wd):
    p0, grads = _flat_case(n, seed=n + 7 + int(wd * 1e4))
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    p = _kernel_run(p0, grads, 1, lr, weight_decay=wd, beta1=betas[0], beta2=betas[1], eps=eps)
    p64 = _torch64(p0, grads, lambda ps: torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False))
    _assert_bar(p, p64, 'adam')
    assert float((p - p0).abs().max()) > 2 * lr               # it moved (up to about lr per step)


# ---------------------------------------------------------------------------------------------------------------------
# on a real model arena
# ---------------------------------------------------------------------------------------------------------------------
def _arena(seed=0):
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    m = Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
    fill_state_(m.state_dict(), seed=seed)
    m = m.to(DEV).train()
    arena = ParamArena(m)
    return m, arena, arena.grad_bucket()


def _grads(total, k, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(total, generator=g) * 0.05).to(DEV) for _ in range(k)]


def test_fused_sgd_matches_sgdnesterov_on_the_model_arena():
    from tam_gcn_amd.distributed import SGDNesterov
    from tam_gcn_amd.optim import FusedSGD
    _, a1, b1 = _arena()
    _, a2, b2 = _arena()
    assert torch.equal(a1.flat, a2.flat)
    ref = SGDNesterov(a1.params, lr=0.05, momentum=0.9, weight_decay=1e-4, arena=a1, bucket=b1)
    opt = FusedSGD(a2, b2, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
    for g in _grads(a1.total, 5):
        b1.flat.copy_(g)
        b2.flat.copy_(g)
        ref.step()
        opt.step()
    torch.cuda.synchronize()
    err = float((a2.flat - a1.flat).abs().max())
    assert err <= BAR * float(a1.flat.abs().max()), err
    assert float((opt.momentum_buffer - ref.flat_buf).abs().max()) <= BAR * float(ref.flat_buf.abs().max())


def _make_opt(kind, arena, bucket, lr):
    from tam_gcn_amd.optim import FusedSGD, FusedAdam
    if kind == 'sgd':
        return FusedSGD(arena, bucket, lr=lr, momentum=0.9, nesterov=True, weight_decay=1e-4)
    return FusedAdam(arena, bucket, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


LRS = [0.05, 0.05, 0.05, 0.005, 0.005, 0.005]          # the learning rate of steps 1..6: set once, between steps 3 and 4


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_replayed_step_follows_the_learning_rate_bit_for_bit(kind):
    """opt.step() captured ONCE, replayed 3x, opt.lr changed on the host, replayed 3x more: equal bit for bit to the
    eager sequence with the same learning-rate change (the rate and the step count are read on the device)."""
    _, ae, be = _arena()
    _, ag, bg = _arena()
    grads = _grads(ae.total, 6)
    eager = _make_opt(kind, ae, be, LRS[0])
    for k, g in enumerate(grads):
        eager.lr = LRS[k]
        be.flat.copy_(g)
        eager.step()
    opt = _make_opt(kind, ag, bg, LRS[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    scratch = torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError, match='outside graph capture'):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch.add_(1.0)
            opt.lr = 1.0
    assert opt.lr == LRS[0]
    for k, g in enumerate(grads):
        if k == 3:
            opt.lr = LRS[3]
        bg.flat.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(ag.flat, _arena()[1].flat)
    assert torch.equal(ag.flat, ae.flat)
    sd, sde = opt.state_dict(), eager.state_dict()
    assert sd['step'] == sde['step'] == 6
    assert sd['lr'] == LRS[3]
    for s, t in zip(sd['state'], sde['state']):
        assert torch.equal(s, t)


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_resume_from_state_dict_is_exact(kind):
    """state_dict after 3 steps, loaded into a fresh optimiser (whose step() was already captured: the load copies into
    the existing storages), 3 more steps: equal bit for bit to 6 uninterrupted steps."""
    _, a6, b6 = _arena()
    _, ar, br = _arena()
    grads = _grads(a6.total, 6, seed=23)
    run6 = _make_opt(kind, a6, b6, LRS[0])
    for k, g in enumerate(grads):
        run6.lr = LRS[k]
        b6.flat.copy_(g)
        run6.step()
    first = _make_opt(kind, ar, br, LRS[0])
    for k in range(3):
        br.flat.copy_(grads[k])
        first.step()
    sd = first.state_dict()
    assert sd['step'] == 3
    fresh = _make_opt(kind, ar, br, 1.0)                      # its own (zero) buffers, another learning rate
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fresh.step()
    fresh.load_state_dict(sd)
    assert fresh.lr == LRS[0]
    fresh.lr = LRS[3]
    for k in range(3, 6):
        br.flat.copy_(grads[k])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ar.flat, a6.flat)
    assert fresh.state_dict()['step'] == 6
    for s, t in zip(fresh.state_dict()['state'], run6.state_dict()['state']):
        assert torch.equal(s, t)
    bad = dict(sd)
    bad['weight_decay'] = 0.5
    with pytest.raises(ValueError, match='weight_decay'):
        fresh.load_state_dict(bad)
