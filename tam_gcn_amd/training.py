"""A training step captured into two HIP graphs, for training loops written by the user (INTEGRATION.md
"Training loop").

    opt = FusedSGD(arena, bucket, lr=0.1)
    train = CapturedStep(model, CrossEntropyLoss(), opt, arena, bucket, x0, y0)
    for epoch in range(E):
        opt.lr = lr_at(epoch, 0.1, steps=(30, 40))
        for x, y in loader:
            loss = train.step(x, y)             # no host sync; loss is overwritten by the next call

Graph 1 holds ``bucket.zero()``, the forward, the loss, the backward and ``bucket.pack()``; graph 2 holds
``optimizer.step()`` (a FusedSGD / FusedAdam: learning rate and step count are read on the device, so both may change
between replays).  With torch.distributed initialised and more than one rank, ``bucket.all_reduce_mean(group)`` runs
between the two replays: bench.py's sequence.

What a hand-written loop does between ``backward()`` and ``step()`` is available as options, since the step is closed:

    opt = FusedSGD(arena, bucket, lr=0.1, max_grad_norm=4.0, skip_nonfinite=True)
    train = CapturedStep(model, loss_fn, opt, arena, bucket, x0, y0, accum_steps=4)
    for x, y in loader:                         # micro-batches: every 4th call updates the parameters
        loss = train.step(x, y)
    print(float(opt.grad_norm), opt.skipped_steps)

``accum_steps=k`` makes every ``step`` a micro-batch: graph 1 then ends in ``bucket.pack(accumulate=True, alpha=1/k)``,
the bucket is zeroed on the stream before the first micro-batch of a cycle, and only every k-th call runs the all-reduce
and graph 2.  The gradient guard (norm clipping, non-finite skip) needs nothing here: it is part of ``optimizer.step()``,
which graph 2 holds.  After the all-reduce every rank holds the same bucket, so every rank computes the same norm and
takes the same skip decision (not run on more than one GPU so far).  BatchNorm running statistics update on every
micro-batch, as in the usual PyTorch accumulation loop, and the guard does not protect them: a forward pass that itself
overflowed has already written them when the optimiser sees the gradient.

A replay executes no Python, so the host-side counters that invalidate the folded-BatchNorm eval caches
(``ParamArena.epoch`` and the per-BatchNorm update counters of functional.py) are bumped here after every replay;
``model.eval()`` inference after any number of steps sees the current parameters and running statistics.
"""
import torch

from . import dropout as _dropout
from . import functional as Fn


class CapturedStep:
    """One model, one loss, one FusedSGD / FusedAdam over ``arena`` / ``bucket``.  ``example_x`` / ``example_y`` fix the
    shapes and dtypes every later batch must have.  Construction runs WARMUP eager steps on a side stream (graph
    capture needs the allocator and the kernels warmed up) and then restores the parameters, the model's buffers and the
    optimiser's state -- and the (seed, call) of a DropoutStream attached by ``dropout.enable`` -- : building the step does not
    train the model or consume draws; the capture records the stream's advance launch, so every replay draws a new mask.  ``eager=True`` runs the same sequence without
    graphs (debugging; equality tests).  ``accum_steps=k > 1``: ``step`` accumulates k micro-batch gradients, each scaled
    by 1/k, and updates on every k-th call; ``pending`` is the number accumulated since the last update."""
    WARMUP = 2                                                  # eager steps before capture, as bench.py

    def __init__(self, model, loss_fn, optimizer, arena, bucket, example_x, example_y, group=None, eager=False,
                 accum_steps=1):
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
            raise ValueError(f'CapturedStep: accum_steps = {accum_steps!r} must be an integer >= 1')
        if getattr(optimizer, 'arena', None) is not arena or getattr(optimizer, 'bucket', None) is not bucket:
            raise ValueError('CapturedStep: the optimiser must be a FusedSGD / FusedAdam over this arena and bucket')
        if not arena.intact():
            raise ValueError('CapturedStep: the ParamArena no longer backs the parameters')
        if not model.training:
            raise ValueError('CapturedStep: put the model in train() mode first (the step is captured in that mode)')
        self.model, self.loss_fn, self.optimizer = model, loss_fn, optimizer
        self.arena, self.bucket, self.group, self.eager = arena, bucket, group, eager
        self.accum_steps, self.pending = accum_steps, 0
        dev = arena.flat.device
        self.x = example_x.detach().to(dev).contiguous().clone()
        self.y = example_y.detach().to(dev).contiguous().clone()
        self._bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        self.loss = None
        self._graphs = None
        if eager:
            return
        saved = (arena.flat.clone(), [b.detach().clone() for b in model.buffers()], optimizer.state_dict())
        drops = [(s, s.tensor.clone()) for s in _dropout.streams_under(model)]      # the warm-up forwards advance `call`
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(self.WARMUP):
                if accum_steps > 1:
                    bucket.flat.zero_()
                self._fwd_bwd()
                self._reduce()
                optimizer.step()
        cur.wait_stream(side)
        with torch.no_grad():
            arena.flat.copy_(saved[0])
            for b, v in zip(model.buffers(), saved[1]):
                b.copy_(v)
            for s, v in drops:                                  # building the step consumes no draws
                s.tensor.copy_(v)
        optimizer.load_state_dict(saved[2])
        arena.touch()
        torch.cuda.synchronize(dev)
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g1):
                self.loss = self._fwd_bwd()
            with torch.cuda.graph(g2):
                optimizer.step()
        except Exception as e:                                  # noqa: BLE001  -- no silent eager fall-back
            raise RuntimeError(f'CapturedStep: HIP graph capture failed ({type(e).__name__}: {e})') from e
        self._graphs = (g1, g2)

    def _fwd_bwd(self):
        self.bucket.zero()
        loss = self.loss_fn(self.model(self.x), self.y)
        loss.backward()
        if self.accum_steps > 1:
            self.bucket.pack(accumulate=True, alpha=1.0 / self.accum_steps)
        else:
            self.bucket.pack()
        return loss.detach()

    def _reduce(self):
        self.bucket.all_reduce_mean(self.group)                 # no-op unless torch.distributed runs > 1 rank

    def _check(self, x, y):
        for name, got, want in (('x', x, self.x), ('y', y, self.y)):
            if tuple(got.shape) != tuple(want.shape) or got.dtype != want.dtype:
                raise ValueError(f'CapturedStep: {name} is {tuple(got.shape)} {got.dtype}, the step was built for '
                                 f'{tuple(want.shape)} {want.dtype}')
        if not self.model.training:
            raise RuntimeError('CapturedStep: the model is in eval() mode; call model.train() before a training step')

    def step(self, x, y):
        """One training step on the batch (x, y); returns the loss tensor (on the device, no host sync).  With
        ``accum_steps=k > 1`` the batch is a micro-batch: its gradient / k is added to the bucket, the parameters change
        on every k-th call only, and the loss returned is the micro-batch's own, unscaled."""
        self._check(x, y)
        self.x.copy_(x)
        self.y.copy_(y)
        if self.accum_steps > 1:
            return self._micro_step()
        if self.eager:
            loss = self._fwd_bwd()
            self._reduce()
            self.optimizer.step()
            return loss
        g1, g2 = self._graphs
        g1.replay()
        self._reduce()
        g2.replay()
        # what the replayed Python would have bumped: the eval caches key on these (functional._eval_cached, f2.FusedEval)
        self.arena.touch()
        for m in self._bns:
            Fn._bn_epoch(m)[0] += 1
        return self.loss

    def _micro_step(self):
        if self.pending == 0:
            self.bucket.flat.zero_()                            # on the stream, before the cycle's first accumulating pack
        if self.eager:
            loss = self._fwd_bwd()
        else:
            self._graphs[0].replay()
            loss = self.loss
            for m in self._bns:                                 # running statistics move on every micro-batch
                Fn._bn_epoch(m)[0] += 1
        self.pending += 1
        if self.pending == self.accum_steps:
            self.pending = 0
            self._reduce()
            if self.eager:
                self.optimizer.step()
            else:
                self._graphs[1].replay()
                self.arena.touch()                              # only now did the parameters change
        return loss
