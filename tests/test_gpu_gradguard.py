"""The gradient guard (tamgcn_optim_step_guarded) and gradient accumulation on the MI355X: the fp64 norm reduction against
torch.linalg.vector_norm, clipped SGD / Adam against float64 clip_grad_norm_ + torch.optim, bit equality with the plain
update when nothing clips, the non-finite skip, and all of it through CapturedStep (replay == eager, accum_steps, one bad
batch, exact resume)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
BAR = 1e-6                  # max |p - p64| <= BAR * max |p64|, the bar of tests/test_gpu_optim.py
EPS24 = 2.0 ** -24
N_ARENA = 1_693_260         # the floats of the N-UCLA model's parameters


class _Flat:
    """Flat device buffers for one optimiser driven through ops.optim_step / ops.optim_step_guarded."""

    def __init__(self, p0, mode, **hyper):
        n = p0.numel()
        self.mode, self.hyper = mode, hyper
        self.p = p0.to(DEV).clone()
        self.s0 = torch.zeros(n, device=DEV) if mode == 1 or hyper.get('momentum', 0) else None
        self.s1 = torch.zeros(n, device=DEV) if mode == 1 else None
        self.lr = torch.tensor([hyper.pop('lr')], device=DEV)
        self.step = torch.zeros(1, device=DEV, dtype=torch.int32)
        self.scal = torch.zeros(2, device=DEV)
        self.g = torch.zeros(n, device=DEV)
        self.partial = torch.zeros(2048, device=DEV, dtype=torch.float64)
        self.stat = torch.zeros(3, device=DEV)
        self.skipped = torch.zeros(1, device=DEV, dtype=torch.int32)

    def plain(self, g):
        from tam_gcn_amd import ops
        self.g.copy_(g)
        ops.optim_step(self.p, self.g, self.s0, self.s1, self.lr, self.step, self.scal, self.mode, **self.hyper)

    def guarded(self, g, max_norm, skip_nonfinite=False):
        from tam_gcn_amd import ops
        self.g.copy_(g)
        ops.optim_step_guarded(self.p, self.g, self.s0, self.s1, self.lr, self.step, self.scal, self.mode, self.partial,
                               self.stat, self.skipped, max_norm=max_norm, skip_nonfinite=skip_nonfinite, **self.hyper)

    def state(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.p, self.s0, self.s1, self.step) if t is not None]


def _same(a, b):
    """bit for bit, NaN payloads included"""
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


HYPER = {
    'sgd_nesterov': (0, dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)),
    'sgd_plain': (0, dict(lr=0.05, momentum=0.0, nesterov=False, weight_decay=1e-4)),
    'adam': (1, dict(lr=1e-3, weight_decay=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)),
}


def _make(kind, p0):
    mode, hyper = HYPER[kind]
    return _Flat(p0, mode, **dict(hyper))


# ---------------------------------------------------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, N_ARENA, 4 * 256 * 2048 + 4 * 256 * 3 + 2])
def test_norm_against_fp64_vector_norm(n):
    """stat[0] against torch.linalg.vector_norm(g.double()) on values spanning 1e-20 ... 1e25 (an fp32 square overflows
    above 1.8e19): |norm - norm64| <= 4 * 2^-24 * norm64 (the fp64 sum contributes about n * 2^-53, the cast to fp32
    2^-24).  Two runs on the same buffer give identical bits, in stat and in every fp64 partial.  The largest n is more
    than 4 * 256 * 2048 elements, so the grid stride is exercised, and has a tail."""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 45.0 - 20.0)
    g[n // 2] = 1e25 if n > 1 else 3e21                                # the span's upper end is present
    assert torch.isfinite(g).all() and float(g.abs().max()) > 1.8e19
    norm64 = float(torch.linalg.vector_norm(g.double()))
    f = _Flat(torch.zeros(n), 0, lr=0.0, momentum=0.0, weight_decay=0.0)
    f.guarded(g, 0.0)
    torch.cuda.synchronize()
    stat1, part1 = f.stat.clone(), f.partial.clone()
    f.partial.fill_(-1.0)
    f.stat.zero_()
    f.guarded(g, 0.0)
    torch.cuda.synchronize()
    norm = float(f.stat[0].double())
    print(f'n = {n}: norm {norm!r}, fp64 {norm64!r}, rel err {abs(norm - norm64) / norm64:.3e} (bar {4 * EPS24:.3e})')
    assert abs(norm - norm64) <= 4 * EPS24 * norm64
    assert float(f.stat[1]) == 1.0 and float(f.stat[2]) == 1.0          # measure only, finite
    blocks = min(2048, max(1, ((n >> 2) + 255) // 256))
    assert torch.equal(f.stat.view(torch.int32), stat1.view(torch.int32))
    assert torch.equal(f.partial[:blocks].view(torch.int64), part1[:blocks].view(torch.int64))
    assert bool((f.partial[blocks:] == -1.0).all())                    # nothing written past the grid
    assert int(f.step.item()) == 2 and torch.equal(f.p.cpu(), torch.zeros(n))      # lr = 0


# ---------------------------------------------------------------------------------------------------------------------
# clipping against float64 torch
# ---------------------------------------------------------------------------------------------------------------------
SCALES = (1e-3, 3e-3, 1e-2, 1e-4, 5e-3, 2e-3)          # x randn over N_ARENA: norms about 1.3, 3.9, 13.0, 0.13, 6.5, 2.6
MAX_NORM = 4.0


def _clip_case(seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.rand(N_ARENA, generator=gen) * 2 - 1
    return p0, [torch.randn(N_ARENA, generator=gen) * s for s in SCALES]


@pytest.mark.parametrize('kind', ['sgd_nesterov', 'adam'])
def test_clipped_update_against_float64_torch(kind):
    """Six steps on the arena-sized vector with max_norm = 4: steps 3 and 5 clip, the others do not.  The reference is
    float64 clip_grad_norm_(foreach=False) + torch.optim (foreach=False); stat[1] equals min(1, 4 / (norm64 + 1e-6)) to
    8 * 2^-24 relative (the norm's 4 * 2^-24 plus one rounding each for the add, the divide and the store)."""
    p0, grads = _clip_case(seed=31 if kind == 'adam' else 30)
    f = _make(kind, p0)
    p64 = torch.nn.Parameter(p0.double())
    if kind == 'adam':
        ref = torch.optim.Adam([p64], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, foreach=False)
    else:
        ref = torch.optim.SGD([p64], lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4, foreach=False)
    clipped = []
    for k, g in enumerate(grads):
        f.guarded(g, MAX_NORM, skip_nonfinite=True)
        torch.cuda.synchronize()
        p64.grad = g.double()
        norm64 = float(torch.nn.utils.clip_grad_norm_([p64], MAX_NORM, foreach=False))
        ref.step()
        coef64 = min(1.0, MAX_NORM / (norm64 + 1e-6))
        norm, coef, finite = (float(v) for v in f.stat.double())
        print(f'{kind} step {k + 1}: norm {norm:.7g} (fp64 {norm64:.7g}), coef {coef:.7g} (fp64 {coef64:.7g})')
        assert abs(norm - norm64) <= 4 * EPS24 * norm64, k
        assert abs(coef - coef64) <= 8 * EPS24 * coef64, k
        assert finite == 1.0
        clipped.append(coef < 1.0)
        assert torch.equal(f.g.cpu(), g)                                # the bucket keeps the unclipped values
    assert clipped == [False, False, True, False, True, False]
    assert int(f.step.item()) == 6 and int(f.skipped.item()) == 0
    err = float((f.p.cpu().double() - p64.detach()).abs().max())
    print(f'{kind}: max |p - p64| = {err:.3e}, bar {BAR * float(p64.detach().abs().max()):.3e}')
    assert err <= BAR * float(p64.detach().abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# coef == 1: the plain update's bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [4099, 4096], ids=['n4099_tail', 'n4096'])
@pytest.mark.parametrize('max_norm', [1e30, 0.0, -1.0], ids=['above_every_norm', 'zero', 'negative'])
@pytest.mark.parametrize('kind', ['sgd_nesterov', 'sgd_plain', 'adam'])
def test_unclipped_guarded_steps_equal_plain_steps_bit_for_bit(kind, max_norm, n):
    from tam_gcn_amd import _lib
    gen = torch.Generator().manual_seed(n + len(kind))
    p0 = torch.rand(n, generator=gen) * 2 - 1
    grads = [torch.randn(n, generator=gen) for _ in range(6)]
    a, b = _make(kind, p0), _make(kind, p0)
    lib = _lib.load()
    for g in grads:
        a.plain(g)
        plain_kernel = lib.tamgcn_last_kernel().decode()
        b.guarded(g, max_norm, skip_nonfinite=True)
        guarded_kernel = lib.tamgcn_last_kernel().decode()
    assert plain_kernel.startswith('optim_update_kernel<') and guarded_kernel == plain_kernel.replace('update', 'update_guarded')
    sa, sb = a.state(), b.state()
    assert int(sb[-1].item()) == 6 and float(b.stat[1]) == 1.0 and int(b.skipped.item()) == 0
    assert not torch.equal(sa[0].cpu(), p0)
    assert _same(sa, sb)


# ---------------------------------------------------------------------------------------------------------------------
# non-finite gradients
# ---------------------------------------------------------------------------------------------------------------------
N_BAD = 4099                                            # 1024 vectors and a 3-element tail
POSITIONS = {'first': 0, 'middle': N_BAD // 2, 'last_tail': N_BAD - 1}


def _bad_case(kind):
    gen = torch.Generator().manual_seed(77 + len(kind))
    p0 = torch.rand(N_BAD, generator=gen) * 2 - 1
    return p0, [torch.randn(N_BAD, generator=gen) for _ in range(3)]


@pytest.mark.parametrize('pos', list(POSITIONS))
@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('kind', ['sgd_nesterov', 'adam'])
def test_nonfinite_gradient_is_skipped(kind, value, pos):
    """One NaN / +inf in the bucket with skip_nonfinite: p, s0, s1 and *step unchanged bit for bit, *skipped + 1,
    stat[2] == 0; good, bad, good equals good, good, and so does bad, good, good (SGD's first-step rule, Adam's bias
    correction: the skipped call does not count as a step)."""
    p0, (g1, g2, g3) = _bad_case(kind)
    bad = g3.clone()
    bad[POSITIONS[pos]] = value
    ref = _make(kind, p0)
    ref.guarded(g1, MAX_NORM, True)
    ref.guarded(g2, MAX_NORM, True)
    want = ref.state()
    assert int(ref.skipped.item()) == 0
    for order in ('good_bad_good', 'bad_good_good'):
        f = _make(kind, p0)
        if order == 'good_bad_good':
            f.guarded(g1, MAX_NORM, True)
        before = f.state()
        f.guarded(bad, MAX_NORM, True)
        after = f.state()
        assert _same(before, after), order
        assert int(f.skipped.item()) == 1 and float(f.stat[2]) == 0.0, order
        assert not bool(torch.isfinite(f.stat[0])), order
        if order == 'bad_good_good':
            f.guarded(g1, MAX_NORM, True)
        f.guarded(g2, MAX_NORM, True)
        assert float(f.stat[2]) == 1.0 and int(f.skipped.item()) == 1, order
        assert _same(f.state(), want), order
        assert int(f.step.item()) == 2


@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_nonfinite_without_skip_propagates_as_in_torch(value):
    """skip_nonfinite off is clip_grad_norm_(error_if_nonfinite=False): a NaN norm gives a NaN coefficient and so NaN
    everywhere; an inf norm gives coefficient 0, so 0 * inf = NaN at the bad element and a zero gradient elsewhere."""
    p0, (g1, _, _) = _bad_case('sgd_plain')
    g1[POSITIONS['middle']] = value
    f = _make('sgd_plain', p0)
    f.guarded(g1, MAX_NORM, False)
    torch.cuda.synchronize()
    p64 = torch.nn.Parameter(p0.double())
    ref = torch.optim.SGD([p64], lr=0.05, weight_decay=1e-4, foreach=False)
    p64.grad = g1.double()
    torch.nn.utils.clip_grad_norm_([p64], MAX_NORM, error_if_nonfinite=False, foreach=False)
    ref.step()
    p = f.p.cpu()
    assert torch.equal(torch.isnan(p), torch.isnan(p64.detach())) and bool(torch.isnan(p).any())
    ok = ~torch.isnan(p)
    if bool(ok.any()):
        assert float((p[ok].double() - p64.detach()[ok]).abs().max()) <= BAR
    assert int(f.step.item()) == 1 and int(f.skipped.item()) == 0 and float(f.stat[2]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# through FusedSGD / FusedAdam / CapturedStep on a small N-UCLA shape
# ---------------------------------------------------------------------------------------------------------------------
MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
B, T, V = 8, 52, 20
LR = {'sgd': (0.05, 0.01), 'adam': (1e-3, 2e-4)}


def _setup(kind='sgd', seed=0, **guard):
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
        opt = FusedSGD(arena, bucket, lr=LR[kind][0], momentum=0.9, nesterov=True, weight_decay=1e-4, **guard)
    else:
        opt = FusedAdam(arena, bucket, lr=LR[kind][0], weight_decay=1e-4, **guard)
    return m, arena, bucket, opt


def _batches(k, seed=3):
    from params import make_input, make_labels
    return [(make_input((B, 3, T, V, 1), seed + i).to(DEV), make_labels(B, 10, seed + 100 + i).to(DEV)) for i in range(k)]


def _bn_state(m):
    return [t.clone() for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)
            for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]


def test_default_optimiser_is_the_plain_one():
    """Without the new arguments: today's state_dict keys, no guard buffers, tamgcn_optim_step's kernel."""
    from tam_gcn_amd import _lib
    _, arena, bucket, opt = _setup('sgd')
    assert set(opt.state_dict()) == {'optimizer', 'momentum', 'dampening', 'nesterov', 'weight_decay', 'lr', 'step', 'state'}
    assert not hasattr(opt, 'grad_norm') and not hasattr(opt, '_partial')
    with pytest.raises(AttributeError):
        opt.skipped_steps
    bucket.flat.normal_(0, 0.01)
    opt.step()
    assert _lib.load().tamgcn_last_kernel().decode() == 'optim_update_kernel<0, true>'
    _, _, _, adam = _setup('adam')
    assert set(adam.state_dict()) == {'optimizer', 'betas', 'eps', 'weight_decay', 'lr', 'step', 'state'}
    _, _, _, g = _setup('sgd', skip_nonfinite=True)
    assert set(g.state_dict()) - set(opt.state_dict()) == {'max_grad_norm', 'skip_nonfinite', 'skipped'}
    assert g.state_dict()['max_grad_norm'] is None and g.skipped_steps == 0
    assert g.grad_norm.shape == g.clip_coef.shape == (1,) and g.grad_norm.is_cuda


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_guarded_captured_step_equals_eager_bit_for_bit(kind):
    """Six steps, the learning rate changed after step 3, max_grad_norm in the middle of the norms a measuring run saw
    (so some steps clip and some do not): replay == eager=True in losses, parameters, BatchNorm statistics, grad_norm
    and clip_coef."""
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    batches = _batches(6)

    def run(eager, **guard):
        m, arena, bucket, opt = _setup(kind, **guard)
        step = CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, *batches[0], eager=eager)
        losses, norms, coefs = [], [], []
        for k, (x, y) in enumerate(batches):
            if k == 3:
                opt.lr = LR[kind][1]
            losses.append(step.step(x, y).clone())
            norms.append(opt.grad_norm.clone())
            coefs.append(opt.clip_coef.clone())
        torch.cuda.synchronize()
        return (torch.stack(losses).cpu(), torch.cat(norms).cpu(), torch.cat(coefs).cpu(), arena.flat.cpu(),
                [t.cpu() for t in _bn_state(m)], opt.state_dict()['step'], opt.skipped_steps)

    measured = run(True, skip_nonfinite=True)[1].sort().values
    max_norm = float(measured[2] + measured[3]) / 2                     # three of the measured norms on either side
    got, ref = run(False, max_grad_norm=max_norm, skip_nonfinite=True), run(True, max_grad_norm=max_norm, skip_nonfinite=True)
    print(f'{kind}: max_grad_norm {max_norm:.5g}, norms {ref[1].tolist()}, coefficients {ref[2].tolist()}')
    assert bool((ref[2] < 1).any()) and bool((ref[2] == 1).any())
    assert got[5] == ref[5] == 6 and got[6] == ref[6] == 0
    for i in range(4):
        assert torch.equal(got[i], ref[i]), (i, got[i], ref[i])
    assert len(got[4]) == len(ref[4]) > 0 and all(torch.equal(a, b) for a, b in zip(got[4], ref[4]))


K = 4


def _eval2(m, x):
    m.eval()
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    m.train()
    return out.clone()


def test_accumulated_steps():
    """accum_steps = 4 over two cycles: parameters untouched by calls 1-3 and changed by call 4, pending 1, 2, 3, 0, one
    optimiser step per cycle, captured == eager bit for bit, the bucket before the update within
    (k + 2) * 2^-24 * sum_j |g_j| / k of the fp64 mean of the four micro-gradients (each obtained alone with a plain
    pack(); batch statistics make them independent of the running buffers), and an eval() forward after the cycle sees
    the new parameters."""
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.training import CapturedStep
    batches = _batches(2 * K, seed=20)
    ce = CrossEntropyLoss()
    # the micro-gradients of the first cycle, one at a time
    m, arena, bucket, _ = _setup('sgd')
    micro, micro_loss = [], []
    for x, y in batches[:K]:
        bucket.zero()
        loss = ce(m(x), y)
        loss.backward()
        micro.append(bucket.pack().double().cpu())
        micro_loss.append(loss.detach().cpu())
    ref = sum(micro) / K
    bound = (K + 2) * EPS24 * sum(g.abs() for g in micro) / K

    runs = {}
    for mode in ('graph', 'eager'):
        m, arena, bucket, opt = _setup('sgd', max_grad_norm=1e9, skip_nonfinite=True)
        step = CapturedStep(m, ce, opt, arena, bucket, *batches[0], eager=(mode == 'eager'), accum_steps=K)
        assert step.pending == 0
        start = arena.flat.clone()
        xe = batches[0][0][:2].contiguous()
        out0 = _eval2(m, xe)
        epoch0 = arena.epoch
        losses, pend = [], []
        for k, (x, y) in enumerate(batches):
            losses.append(step.step(x, y).clone())
            pend.append(step.pending)
            torch.cuda.synchronize()
            if k < K - 1:
                assert torch.equal(arena.flat, start), (mode, k)
                assert opt.state_dict()['step'] == 0 and arena.epoch == epoch0
            if k == K - 1:
                assert not torch.equal(arena.flat, start), mode
                assert opt.state_dict()['step'] == 1
                err = (bucket.flat.double().cpu() - ref).abs()
                print(f'{mode}: accumulated bucket, worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}')
                assert bool((err <= bound).all()), mode
                for j in range(K):
                    assert torch.equal(losses[j].cpu(), micro_loss[j]), (mode, j)       # the micro-batch's own, unscaled
                out = _eval2(m, xe)
                fresh = Model(**MARGS)
                fresh.load_state_dict({k_: v.cpu() for k_, v in m.state_dict().items()})
                fresh = fresh.to(DEV)
                ParamArena(fresh)
                want = _eval2(fresh, xe)
                assert not torch.equal(out0, want)
                assert torch.equal(out, want), (mode, float((out - want).abs().max()))
        assert pend == [1, 2, 3, 0, 1, 2, 3, 0], (mode, pend)
        assert opt.state_dict()['step'] == 2 and opt.skipped_steps == 0
        runs[mode] = (torch.stack(losses).cpu(), arena.flat.cpu(), opt.momentum_buffer.cpu(), [t.cpu() for t in _bn_state(m)],
                      opt.grad_norm.cpu())
    g, e = runs['graph'], runs['eager']
    for i in (0, 1, 2, 4):
        assert torch.equal(g[i], e[i]), i
    assert all(torch.equal(a, b) for a, b in zip(g[3], e[3]))


@pytest.mark.parametrize('eager', [False, True], ids=['graph', 'eager'])
def test_one_bad_batch_is_skipped(eager):
    """The loss is multiplied by a 1-element device tensor set to inf for one step (the forward, and so the BatchNorm
    statistics, stay finite): that step leaves the arena and the momentum buffer bit-identical and skipped_steps == 1;
    the next clean step lands where a run that never saw the bad batch lands."""
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    batches = _batches(3, seed=50)
    ce = CrossEntropyLoss()

    def run(with_bad):
        m, arena, bucket, opt = _setup('sgd', max_grad_norm=1e9, skip_nonfinite=True)
        scale = torch.ones(1, device=DEV)
        step = CapturedStep(m, lambda out, y: ce(out, y) * scale, opt, arena, bucket, *batches[0], eager=eager)
        step.step(*batches[0])
        if with_bad:
            torch.cuda.synchronize()
            before = (arena.flat.clone(), opt.momentum_buffer.clone())
            scale.fill_(float('inf'))
            step.step(*batches[1])
            scale.fill_(1.0)
            torch.cuda.synchronize()
            assert torch.equal(arena.flat, before[0]) and torch.equal(opt.momentum_buffer, before[1])
            assert opt.skipped_steps == 1 and opt.state_dict()['step'] == 1
            assert not bool(torch.isfinite(opt.grad_norm))
        loss = step.step(*batches[2]).clone()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t.float()).all()) for t in _bn_state(m))
        assert bool(torch.isfinite(arena.flat).all())
        return loss.cpu(), arena.flat.cpu(), opt.momentum_buffer.cpu(), opt.state_dict()['step'], opt.skipped_steps

    bad, clean = run(True), run(False)
    assert bad[3] == clean[3] == 2 and bad[4] == 1 and clean[4] == 0
    for i in range(3):
        assert torch.equal(bad[i], clean[i]), i


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_guarded_resume_from_state_dict_is_exact(kind):
    """state_dict after three guarded steps, one of them skipped, loaded into a fresh optimiser whose step() is already
    captured; three more steps equal six uninterrupted ones bit for bit.  Another max_grad_norm is refused."""
    from tam_gcn_amd.optim import FusedSGD
    guard = dict(max_grad_norm=2.0, skip_nonfinite=True)
    _, a6, b6, run6 = _setup(kind, **guard)
    _, ar, br, first = _setup(kind, **guard)
    gen = torch.Generator().manual_seed(23)
    grads = [(torch.randn(a6.total, generator=gen) * s).to(DEV) for s in (1e-3, 1e-3, 5e-3, 1e-3, 5e-3, 1e-3)]
    grads[1][a6.total // 3] = float('inf')                              # step 2 is skipped
    for g in grads:
        b6.flat.copy_(g)
        run6.step()
    for g in grads[:3]:
        br.flat.copy_(g)
        first.step()
    sd = first.state_dict()
    assert sd['step'] == 2 and sd['skipped'] == 1 and sd['max_grad_norm'] == 2.0 and sd['skip_nonfinite'] is True
    _, _, _, other = _setup(kind, max_grad_norm=3.0, skip_nonfinite=True)
    with pytest.raises(ValueError, match='max_grad_norm'):
        other.load_state_dict(sd)
    _, _, _, plain = _setup(kind)
    with pytest.raises(ValueError, match='built without'):
        plain.load_state_dict(sd)                                       # a plain optimiser would drop the guard silently
    fresh = type(first)(ar, br, lr=1.0, weight_decay=1e-4, **guard) if kind == 'adam' else \
        FusedSGD(ar, br, lr=1.0, momentum=0.9, nesterov=True, weight_decay=1e-4, **guard)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fresh.step()
    fresh.load_state_dict(sd)
    assert fresh.lr == LR[kind][0] and fresh.skipped_steps == 1
    for g in grads[3:]:
        br.flat.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ar.flat, a6.flat)
    sf, s6 = fresh.state_dict(), run6.state_dict()
    assert sf['step'] == s6['step'] == 5 and sf['skipped'] == s6['skipped'] == 1
    assert all(torch.equal(s, t) for s, t in zip(sf['state'], s6['state']))
    assert torch.equal(fresh.grad_norm, run6.grad_norm) and torch.equal(fresh.clip_coef, run6.clip_coef)
