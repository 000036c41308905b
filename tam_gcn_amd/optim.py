"""Fused optimisers on the flat ParamArena / FlatGradBucket pair, safe to capture in a HIP graph.

``FusedSGD`` (torch.optim.SGD) and ``FusedAdam`` (torch.optim.Adam, coupled weight decay) update ``arena.flat`` from
``bucket.flat`` with ONE streaming kernel (tamgcn_optim_step) after a one-thread launch that advances the step count.
The learning rate and the step count live in device memory, so a graph that holds ``step()`` uses the learning rate
set on the host between replays and counts its own replays: SGD's first-step rule and Adam's bias corrections stay
right however the step is launched.  The reference's optimisers: processor/recognition_rgb.py:23-33,
processor/recognition_cross_modal.py:20-32.

Gradient guard.  ``max_grad_norm=`` and ``skip_nonfinite=`` put what a hand-written loop does between ``backward()`` and
``step()`` on the device (tamgcn_optim_step_guarded, three launches, still capture-safe): the L2 norm of the whole bucket
is reduced in fp64 in a fixed order, the update uses ``g * min(1, max_grad_norm / (norm + 1e-6))``
(torch.nn.utils.clip_grad_norm_) and, with ``skip_nonfinite``, a step whose norm is inf or NaN leaves the parameters, the
state buffers and the step count untouched and is counted in ``skipped_steps``.  The bucket is NOT rewritten: ``p.grad``
keeps the unclipped values, the coefficient is in ``opt.clip_coef``.  The guard sees the gradients only: BatchNorm
running statistics that a forward pass already overflowed are not rolled back.

``lr_at`` is the reference's learning-rate schedule as a pure function of the epoch; the host sets
``opt.lr = lr_at(epoch, ...)`` once per epoch, outside any capture.
"""
import torch

from . import ops


def lr_at(epoch, base_lr, steps=(), decay=0.1, warmup=0):
    """Learning rate of ``epoch`` (0-based): ``base_lr * (epoch + 1) / warmup`` during the first ``warmup`` epochs, then
    ``base_lr * decay ** (number of steps <= epoch)`` (processor/recognition_cross_modal.py:34-39)."""
    if epoch < warmup:
        return base_lr * (epoch + 1) / warmup
    return base_lr * decay ** sum(epoch >= s for s in steps)


class _FusedFlat:
    MODE = None
    _HYPER = ()

    N_PARTIAL = 2048                    # one fp64 partial per workgroup of the norm reduction (the kernel's largest grid)

    def __init__(self, arena, bucket, lr, max_grad_norm=None, skip_nonfinite=False):
        name = type(self).__name__
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:                         # refuses NaN too
                raise ValueError(f'{name}: max_grad_norm {max_grad_norm} must be > 0 (None: no clipping)')
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self.guarded = max_grad_norm is not None or self.skip_nonfinite
        if [id(p) for p in arena.params] != [id(p) for p in bucket.params] or list(arena.offsets) != list(bucket.offsets):
            raise ValueError(f'{name}: build the bucket with arena.grad_bucket() (same order and offsets)')
        if bucket.flat.numel() != arena.flat.numel():
            raise ValueError(f'{name}: the bucket and the arena differ in size')
        if not arena.intact():
            raise ValueError(f'{name}: the ParamArena no longer backs the parameters')
        if arena.flat.dtype != torch.float32 or not arena.flat.is_cuda:
            raise ValueError(f'{name}: the update runs on fp32 arenas on the GPU')
        self.arena, self.bucket = arena, bucket
        dev = arena.flat.device
        self._lr = torch.empty(1, device=dev, dtype=torch.float32)
        self._step = torch.zeros(1, device=dev, dtype=torch.int32)
        self._scal = torch.zeros(2, device=dev, dtype=torch.float32)
        if self.guarded:
            self._partial = torch.zeros(self.N_PARTIAL, device=dev, dtype=torch.float64)
            self._stat = torch.zeros(3, device=dev, dtype=torch.float32)      # norm before clipping, coefficient, finite
            self._skipped = torch.zeros(1, device=dev, dtype=torch.int32)
            self.grad_norm, self.clip_coef = self._stat[0:1], self._stat[1:2]
        self.lr = lr

    @property
    def lr(self):
        return self._lr_host

    @lr.setter
    def lr(self, value):
        """Written on the current stream; a graph that holds step() reads it on its next replay."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{type(self).__name__}.lr: set the learning rate outside graph capture '
                               '(a captured write would replay the value of capture time)')
        value = float(value)
        if not value >= 0.0:
            raise ValueError(f'{type(self).__name__}: learning rate {value} < 0')
        self._lr.fill_(value)
        self._lr_host = value

    def _buffers(self):
        raise NotImplementedError

    def _args(self):
        """(s0, s1, keyword hyperparameters) of ops.optim_step / ops.optim_step_guarded"""
        raise NotImplementedError

    def _launch(self):
        s0, s1, hyper = self._args()
        if not self.guarded:
            ops.optim_step(self.arena.flat, self.bucket.flat, s0, s1, self._lr, self._step, self._scal, self.MODE, **hyper)
        else:
            ops.optim_step_guarded(self.arena.flat, self.bucket.flat, s0, s1, self._lr, self._step, self._scal, self.MODE,
                                   self._partial, self._stat, self._skipped, max_norm=self.max_grad_norm or 0.0,
                                   skip_nonfinite=self.skip_nonfinite, **hyper)

    @property
    def skipped_steps(self):
        """Steps skipped for a non-finite gradient norm so far (reads the device counter: a host sync)."""
        if not self.guarded:
            raise AttributeError(f'{type(self).__name__}: built without max_grad_norm / skip_nonfinite')
        return int(self._skipped.item())

    @torch.no_grad()
    def step(self):
        """One update of arena.flat from bucket.flat (two launches on the current stream, three with the gradient guard;
        capture-safe).  With the guard, ``grad_norm`` and ``clip_coef`` (1-element device tensors) hold this step's norm
        before clipping and the coefficient applied; reading them later needs no sync of its own."""
        self.arena.touch()                  # eval caches key on the arena's state_version(); the kernel writes behind torch
        self._launch()

    def _hyper(self):
        keys = self._HYPER + (('max_grad_norm', 'skip_nonfinite') if self.guarded else ())
        return {k: getattr(self, k) for k in keys}

    def state_dict(self):
        """Hyperparameters, learning rate, step count and cloned flat state buffers (reads the step count: a host sync)."""
        sd = {'optimizer': type(self).__name__, **self._hyper(), 'lr': self._lr_host,
              'step': int(self._step.item()), 'state': [b.clone() for b in self._buffers()]}
        if self.guarded:
            sd['skipped'] = self.skipped_steps
        return sd

    def load_state_dict(self, sd):
        """Copies into the existing device storages: a graph already captured around step() keeps working.  The
        hyperparameters other than the learning rate, max_grad_norm and skip_nonfinite among them, are fixed at
        construction (they are launch arguments inside a captured graph) and must match."""
        name = type(self).__name__
        if sd.get('optimizer') != name:
            raise ValueError(f'{name}.load_state_dict: a state of {sd.get("optimizer")!r}')
        if not self.guarded and (sd.get('max_grad_norm') is not None or sd.get('skip_nonfinite')):
            raise ValueError(f'{name}.load_state_dict: the state was saved with max_grad_norm = {sd.get("max_grad_norm")!r}, '
                             f'skip_nonfinite = {sd.get("skip_nonfinite")!r}; this optimiser was built without them')
        for k, v in self._hyper().items():
            got = sd.get(k)
            if (tuple(got) if isinstance(got, (list, tuple)) else got) != v:
                raise ValueError(f'{name}.load_state_dict: {k} = {sd.get(k)!r} in the state, {v!r} here')
        bufs, src = self._buffers(), sd['state']
        if len(src) != len(bufs) or any(s.shape != b.shape for s, b in zip(src, bufs)):
            raise ValueError(f'{name}.load_state_dict: state buffers of another arena')
        self.lr = sd['lr']
        with torch.no_grad():
            for b, s in zip(bufs, src):
                b.copy_(s)
            self._step.fill_(int(sd['step']))
            if self.guarded:
                self._skipped.fill_(int(sd.get('skipped', 0)))


class FusedSGD(_FusedFlat):
    """torch.optim.SGD (momentum, dampening, Nesterov, coupled weight decay) on the flat arena; the defaults are the
    reference's recipe (SGD, momentum 0.9, Nesterov, weight decay 1e-4)."""
    MODE = 0
    _HYPER = ('momentum', 'dampening', 'nesterov', 'weight_decay')

    def __init__(self, arena, bucket, lr, momentum=0.9, nesterov=True, weight_decay=1e-4, dampening=0,
                 max_grad_norm=None, skip_nonfinite=False):
        if momentum < 0 or weight_decay < 0:
            raise ValueError('FusedSGD: momentum and weight_decay must be >= 0')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('FusedSGD: Nesterov momentum needs momentum > 0 and zero dampening')
        self.momentum, self.dampening, self.nesterov = float(momentum), float(dampening), bool(nesterov)
        self.weight_decay = float(weight_decay)
        super().__init__(arena, bucket, lr, max_grad_norm, skip_nonfinite)
        self.momentum_buffer = torch.zeros_like(arena.flat) if self.momentum != 0 else None

    def _buffers(self):
        return [self.momentum_buffer] if self.momentum_buffer is not None else []

    def _args(self):
        return self.momentum_buffer, None, dict(momentum=self.momentum, dampening=self.dampening, nesterov=self.nesterov,
                                                weight_decay=self.weight_decay)


class FusedAdam(_FusedFlat):
    """torch.optim.Adam (L2 weight decay added to the gradient, no amsgrad) on the flat arena."""
    MODE = 1
    _HYPER = ('betas', 'eps', 'weight_decay')

    def __init__(self, arena, bucket, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None,
                 skip_nonfinite=False):
        b1, b2 = (float(b) for b in betas)
        if not (0 <= b1 < 1 and 0 <= b2 < 1) or eps < 0 or weight_decay < 0:
            raise ValueError(f'FusedAdam: betas {betas} outside [0, 1), or eps / weight_decay < 0')
        self.betas, self.eps, self.weight_decay = (b1, b2), float(eps), float(weight_decay)
        super().__init__(arena, bucket, lr, max_grad_norm, skip_nonfinite)
        self.exp_avg = torch.zeros_like(arena.flat)
        self.exp_avg_sq = torch.zeros_like(arena.flat)

    def _buffers(self):
        return [self.exp_avg, self.exp_avg_sq]

    def _args(self):
        return self.exp_avg, self.exp_avg_sq, dict(weight_decay=self.weight_decay, beta1=self.betas[0], beta2=self.betas[1],
                                                   eps=self.eps)
