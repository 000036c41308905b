"""The gradient guard and gradient accumulation without a GPU: the argument checks of tamgcn_optim_step_guarded (they run
before any HIP call), FlatGradBucket.pack(accumulate=True) against an fp64 sum, and the constructor checks of
FusedSGD / FusedAdam (max_grad_norm) and CapturedStep (accum_steps)."""
import ctypes as C

import pytest
import torch


def _lib():
    from tam_gcn_amd import build, _lib
    build.build()
    return _lib.load(), _lib


def _desc(_l, **kw):
    d = _l.OptimDesc()
    d.n = kw.get('n', 8)
    for k in ('p', 'g', 's0', 's1', 'lr', 'step', 'scal'):
        setattr(d, k, kw[k])
    d.mode = kw.get('mode', 0)
    d.nesterov = kw.get('nesterov', 1)
    d.momentum, d.dampening, d.weight_decay, d.eps = kw.get('momentum', 0.9), 0.0, 1e-4, 1e-8
    d.beta1, d.beta2 = kw.get('beta1', 0.9), 0.999
    return d


def _guard(_l, **kw):
    g = _l.GradGuard()
    g.max_norm = kw.get('max_norm', 4.0)
    g.skip_nonfinite = kw.get('skip_nonfinite', 1)
    g.partial, g.n_partial = kw['partial'], kw.get('n_partial', 2048)
    g.stat, g.skipped = kw['stat'], kw['skipped']
    return g


def test_optim_step_guarded_rejects_bad_arguments_without_touching_the_gpu():
    """Everything tamgcn_optim_step refuses, plus the guard's own arguments: a negative status and a message that names
    the entry point, before any HIP call (host memory stands in for the device buffers; nothing is launched)."""
    lib, _l = _lib()
    arr = (C.c_float * 64)()
    scratch = (C.c_double * 2050)()
    a16 = (C.addressof(arr) + 15) // 16 * 16
    p8 = (C.addressof(scratch) + 7) // 8 * 8
    good = dict(p=a16, g=a16 + 64, s0=a16 + 128, s1=a16 + 192, lr=a16 + 224, step=a16 + 228, scal=a16 + 240)
    ggood = dict(partial=p8, stat=a16 + 208, skipped=a16 + 232)

    def call(gkw=None, **kw):
        d = _desc(_l, **{**good, **kw})
        g = _guard(_l, **{**ggood, **(gkw or {})})
        return lib.tamgcn_optim_step_guarded(C.byref(d), C.byref(g), None), lib.tamgcn_last_error()

    g0 = _guard(_l, **ggood)
    assert lib.tamgcn_optim_step_guarded(None, C.byref(g0), None) < 0
    assert b'tamgcn_optim_step_guarded' in lib.tamgcn_last_error()
    d0 = _desc(_l, **good)
    assert lib.tamgcn_optim_step_guarded(C.byref(d0), None, None) < 0
    assert b'tamgcn_optim_step_guarded' in lib.tamgcn_last_error() and b'guard' in lib.tamgcn_last_error()
    cases = [
        # the checks shared with tamgcn_optim_step
        (dict(p=None), None, b'NULL'),
        (dict(g=None), None, b'NULL'),
        (dict(lr=None), None, b'NULL'),
        (dict(step=None), None, b'NULL'),
        (dict(s0=None), None, b's0'),
        (dict(mode=1, s1=None), None, b's1'),
        (dict(p=a16 + 4), None, b'aligned'),
        (dict(g=a16 + 68), None, b'aligned'),
        (dict(mode=2), None, b'mode 2'),
        (dict(n=0), None, b'n = 0'),
        (dict(momentum=0.0), None, b'Nesterov'),
        (dict(mode=1, beta1=1.0), None, b'betas'),
        # the guard's own
        ({}, dict(partial=None), b'NULL partial or stat'),
        ({}, dict(stat=None), b'NULL partial or stat'),
        ({}, dict(skipped=None), b'skipped'),
        ({}, dict(partial=p8 + 4), b'8-byte aligned'),
        ({}, dict(max_norm=float('nan')), b'NaN'),
        ({}, dict(n_partial=0), b'n_partial 0'),
        (dict(n=4 * 256 * 7), dict(n_partial=6), b'n_partial 6'),            # 7 workgroups
        (dict(n=1 << 30), dict(n_partial=2047), b'n_partial 2047'),          # the grid is capped at 2048
    ]
    for kw, gkw, msg in cases:
        rc, err = call(gkw, **kw)
        assert rc < 0, (kw, gkw)
        assert b'tamgcn_optim_step_guarded' in err and msg in err, (kw, gkw, err)


def test_guarded_entry_point_is_declared_and_bound():
    import os
    from tam_gcn_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'tamgcn.h')).read()
    assert 'int tamgcn_optim_step_guarded(const tamgcn_optim_desc* d, const tamgcn_grad_guard* g, void* stream);' in header
    assert 'tamgcn_optim_step_guarded' in _lib.SIGNATURES and callable(ops.optim_step_guarded)
    assert C.sizeof(_lib.GradGuard) == 40                 # float, int, double*, int (+pad), float*, int* on LP64


K = 4


def test_pack_accumulate_against_fp64_sum():
    """k = 4 micro-gradients over 1.69 M elements, each added with alpha = 1/k: every element within
    (k + 2) * 2^-24 * sum_j |g_j| / k of the fp64 sum (one rounding per scaled add plus one per product).  A parameter
    without a gradient keeps what the bucket held; pack() with defaults still equals the copy."""
    from tam_gcn_amd.distributed import FlatGradBucket
    gen = torch.Generator().manual_seed(7)
    shapes = [(1300, 1300), (3257,), (5, 7, 11), (1,), (2,)]          # 1,693,645 elements; the last never gets a gradient
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    bucket = FlatGradBucket(params)
    assert bucket.flat.numel() >= 1_690_000
    micro = [[torch.randn(s, generator=gen) for s in shapes[:-1]] for _ in range(K)]
    bucket.flat.zero_()
    bucket.views[-1].fill_(3.0)
    for grads in micro:
        bucket.zero()
        for p, g in zip(params, grads):
            p.grad = g.clone()
        out = bucket.pack(accumulate=True, alpha=1.0 / K)
        assert out is bucket.flat
        assert all(p.grad is v for p, v in zip(params, bucket.views))
    worst = 0.0
    for i in range(len(shapes) - 1):
        ref = sum(m[i].double() for m in micro) / K
        mag = sum(m[i].double().abs() for m in micro) / K
        bound = (K + 2) * 2.0 ** -24 * mag
        err = (bucket.views[i].double() - ref).abs()
        assert bool((err <= bound).all()), (i, float((err / bound).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f'accumulated bucket: worst error / bound = {worst:.3f}')
    assert torch.equal(bucket.views[-1], torch.full((2,), 3.0))       # no gradient: left alone
    # a second accumulating pack with nothing new (p.grad still the views) adds nothing
    before = bucket.flat.clone()
    bucket.pack(accumulate=True, alpha=0.25)
    assert torch.equal(bucket.flat, before)
    # defaults: the plain copy, parameters without a gradient zeroed as before
    bucket.zero()
    for p, g in zip(params, micro[0]):
        p.grad = g.clone()
    bucket.pack()
    for i in range(len(shapes) - 1):
        assert torch.equal(bucket.views[i], micro[0][i])
    assert torch.equal(bucket.views[-1], torch.zeros(2))


def _cpu_model():
    from tam_gcn_amd.models.ctrgcn import Model
    torch.manual_seed(0)
    return Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


@pytest.mark.parametrize('cls', ['FusedSGD', 'FusedAdam'])
@pytest.mark.parametrize('bad', [-1, 0, float('nan')])
def test_bad_max_grad_norm_is_refused_before_any_device_work(cls, bad):
    from tam_gcn_amd import optim
    from tam_gcn_amd.distributed import ParamArena
    arena = ParamArena(_cpu_model())
    with pytest.raises(ValueError, match='max_grad_norm'):
        getattr(optim, cls)(arena, arena.grad_bucket(), lr=0.1, max_grad_norm=bad)


@pytest.mark.parametrize('bad', [0, -2, 2.0, 1.5, '4', True])
def test_bad_accum_steps_is_refused_before_any_device_work(bad):
    from tam_gcn_amd.training import CapturedStep
    m = _cpu_model().train()
    with pytest.raises(ValueError, match='accum_steps'):
        CapturedStep(m, None, None, None, None, torch.zeros(1), torch.zeros(1), accum_steps=bad)
