"""Fused optimisers without a GPU: the learning-rate schedule against the reference's two schedules, the argument checks
of tamgcn_optim_step (they run before any HIP call) and the arena / bucket checks of FusedSGD / FusedAdam."""
import ctypes as C

import numpy as np
import pytest
import torch

from tam_gcn_amd.optim import lr_at


def test_lr_at_is_adjust_learning_rate():
    """processor/recognition_cross_modal.py:34-39: base_lr * lr_decay_rate ** sum(epoch >= step)."""
    base_lr, decay, step = 0.1, 0.1, [30, 40, 60]
    for epoch in range(81):
        ref = base_lr * (decay ** np.sum(epoch >= np.array(step)))
        assert lr_at(epoch, base_lr, steps=step, decay=decay) == ref, epoch
    assert lr_at(0, 0.05) == 0.05 and lr_at(80, 0.05, steps=(), decay=0.5) == 0.05


def test_lr_at_is_warmup_then_multisteplr():
    """tools/train_stgcn_group.py:182-192, 244-245: 5 warm-up epochs set lr = BASE_LR * (epoch + 1) / 5 by hand, then
    MultiStepLR(milestones=[50, 65], gamma=0.1) is stepped at the end of every later epoch.  The scheduler starts
    counting after the warm-up, so its milestones fall 5 epochs later: lr_at(steps=[m + warmup for m in milestones])."""
    base_lr, warmup, milestones, gamma = 0.1, 5, [50, 65], 0.1
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=base_lr, momentum=0.9, nesterov=True, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=gamma)
    steps = [m + warmup for m in milestones]
    seen = []
    for epoch in range(80):
        if epoch < warmup:
            for g in opt.param_groups:
                g['lr'] = base_lr * (epoch + 1) / warmup
        lr = opt.param_groups[0]['lr']
        seen.append(lr)
        assert lr_at(epoch, base_lr, steps=steps, decay=gamma, warmup=warmup) == pytest.approx(lr, rel=1e-12, abs=0), epoch
        opt.step()
        if epoch >= warmup:
            sched.step()
    assert len(set(round(v, 12) for v in seen[warmup:])) == 3       # both milestones were crossed


def _lib():
    from tam_gcn_amd import build, _lib
    build.build()
    return _lib.load(), _lib


def _desc(_lib, **kw):
    d = _lib.OptimDesc()
    d.n = kw.get('n', 8)
    for k in ('p', 'g', 's0', 's1', 'lr', 'step', 'scal'):
        setattr(d, k, kw[k])
    d.mode = kw.get('mode', 0)
    d.nesterov = kw.get('nesterov', 1)
    d.momentum, d.dampening, d.weight_decay, d.eps = kw.get('momentum', 0.9), 0.0, 1e-4, 1e-8
    d.beta1, d.beta2 = kw.get('beta1', 0.9), 0.999
    return d


def test_optim_step_rejects_bad_arguments_without_touching_the_gpu():
    """NULL / misaligned pointers, a bad mode and impossible hyperparameters: a negative status and a message, before
    any HIP call (host memory stands in for the device buffers; nothing is launched)."""
    lib, _l = _lib()
    arr = (C.c_float * 64)()
    base = C.addressof(arr)
    a16 = (base + 15) // 16 * 16
    good = dict(p=a16, g=a16 + 64, s0=a16 + 128, s1=a16 + 192, lr=a16 + 224, step=a16 + 228, scal=a16 + 240)

    def call(**kw):
        d = _desc(_l, **{**good, **kw})
        return lib.tamgcn_optim_step(C.byref(d), None), lib.tamgcn_last_error()

    assert lib.tamgcn_optim_step(None, None) < 0 and b'tamgcn_optim_step' in lib.tamgcn_last_error()
    cases = [
        (dict(p=None), b'NULL'),
        (dict(g=None), b'NULL'),
        (dict(lr=None), b'NULL'),
        (dict(step=None), b'NULL'),
        (dict(s0=None), b's0'),                          # SGD with momentum needs its buffer
        (dict(mode=1, s1=None), b's1'),                  # Adam needs exp_avg_sq
        (dict(p=a16 + 4), b'aligned'),
        (dict(g=a16 + 68), b'aligned'),
        (dict(mode=1, s1=a16 + 200), b'aligned'),
        (dict(mode=2), b'mode 2'),
        (dict(mode=-1), b'mode -1'),
        (dict(n=0), b'n = 0'),
        (dict(momentum=0.0), b'Nesterov'),              # Nesterov without momentum (torch refuses it too)
        (dict(mode=1, beta1=1.0), b'betas'),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc < 0, kw
        assert b'tamgcn_optim_step' in err and msg in err, (kw, err)


def _cpu_model():
    from tam_gcn_amd.models.ctrgcn import Model
    torch.manual_seed(0)
    return Model(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


@pytest.mark.parametrize('cls', ['FusedSGD', 'FusedAdam'])
def test_fused_optimisers_refuse_a_bucket_of_another_layout(cls):
    from tam_gcn_amd import optim
    from tam_gcn_amd.distributed import ParamArena, FlatGradBucket
    Opt = getattr(optim, cls)
    m = _cpu_model()
    arena = ParamArena(m)
    with pytest.raises(ValueError, match='same order and offsets'):
        Opt(arena, FlatGradBucket(arena.params), lr=0.1)            # packed offsets, not the arena's aligned ones
    with pytest.raises(ValueError, match='same order and offsets'):
        Opt(arena, FlatGradBucket(list(reversed(arena.params))), lr=0.1)
    other = ParamArena(_cpu_model())
    with pytest.raises(ValueError, match='same order and offsets'):
        Opt(arena, other.grad_bucket(), lr=0.1)
    m.fc.weight.data = m.fc.weight.data.clone()                    # detached from the arena
    with pytest.raises(ValueError, match='no longer backs'):
        Opt(arena, arena.grad_bucket(), lr=0.1)
