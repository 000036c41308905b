"""The evaluation epoch without the host in it (reference processor/recognition_rgb.py:71-101: per batch loss.item(),
output.cpu().numpy(), label.cpu().numpy(), then np.argmax on the host; ensemble/ensemble_ctrgcn_resnet_eval.py:217-234, :267:
per-class accuracy and confusion matrix from the stored scores).

``EvalMeter`` keeps the epoch's state on the device -- batch and sample counts, top-k hits, the two loss sums, the confusion
matrix and, if asked, every sample's scores -- and adds a batch to it in ONE launch (tamgcn_eval_accumulate) that neither
synchronises nor copies; ``compute()`` is the only call that reads the device.

``CapturedEval`` runs a whole val split through it: the batch from ``GraphedBatch``, the forward from ``GraphedForward``, the
meter launch behind them on the same stream.

    train = CapturedStep(model, loss_fn, opt, arena, bucket, x0, y0)
    val = CapturedEval(model.eval(), val_feeder, 64); model.train()
    for epoch in range(epochs):
        for i in range(0, len(perm) - B + 1, B):
            train.step(*gb(perm[i:i + B]))
        model.eval()
        res = val.run().compute()              # the epoch's one synchronisation: res['loss'], res['top1'], res['confusion'], ...
        model.train()

``run()`` compares the model's state key (tensor versions, BatchNorm update counters, ParamArena.state_version(): what
f2.FusedEval and functional._eval_cached key their folded coefficients on) with the one its forward graph was captured under and
captures again when it moved, so a run always evaluates the CURRENT parameters and running statistics.
"""
import torch

from . import ops
from . import functional as Fn
from .inference import GraphedForward

__all__ = ['EvalMeter', 'CapturedEval']


class EvalMeter:
    """num_class K; num_samples: keep a (num_samples, K) score table (rows never written are NaN); topk: up to four k.

    update(logits, labels, index=None, valid=None)   one launch, no synchronisation, capturable by torch.cuda.graph.  Only the
        first `valid` rows count (None: all; an int, or a 0-d int32 tensor on the device that a graph replay may change).
        Row n's scores go to row index[n] of the table, or to the next free row when index is None (rows are then numbered
        by the host: every update takes `valid` rows, or the whole batch where valid is a tensor).
    reset()                                          zeroes the state (on the stream, no synchronisation)
    state()                                          the raw device tensors (a multi-rank user all-reduces them)
    compute()                                        the one device read -> dict, see there
    Conventions (include/tamgcn.h, tamgcn_eval_accumulate): label -100 is skipped, any other label outside [0, K) is
    counted in bad_labels and makes that batch's mean loss NaN; an index outside the table stores nothing and is counted."""

    def __init__(self, num_class, num_samples=None, topk=(1, 5), device='cuda'):
        topk = tuple(int(k) for k in topk)
        if not 0 < int(num_class) or len(topk) > ops.EVAL_MAX_TOPK or any(k < 1 for k in topk):
            raise ValueError(f'EvalMeter: num_class {num_class!r} must be >= 1 and topk {topk!r} at most {ops.EVAL_MAX_TOPK} entries >= 1')
        if num_samples is not None and int(num_samples) < 1:
            raise ValueError(f'EvalMeter: num_samples = {num_samples!r} must be >= 1 (None: keep no scores)')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('EvalMeter: the state lives on the GPU; there is no CPU path')
        self.num_class, self.topk = int(num_class), topk
        self.counts = torch.zeros(ops.EVAL_COUNTS, dtype=torch.int64, device=dev)
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.confusion = torch.zeros(self.num_class, self.num_class, dtype=torch.int32, device=dev)
        self.scores = None if num_samples is None else torch.full((int(num_samples), self.num_class), float('nan'), dtype=torch.float32, device=dev)
        self._base = 0

    def reset(self):
        self.counts.zero_()
        self.sums.zero_()
        self.confusion.zero_()
        if self.scores is not None:
            self.scores.fill_(float('nan'))
        self._base = 0

    def state(self):
        return {'counts': self.counts, 'sums': self.sums, 'confusion': self.confusion, 'scores': self.scores}

    def update(self, logits, labels, index=None, valid=None):
        if not torch.is_tensor(logits) or logits.dim() != 2 or logits.shape[1] != self.num_class:
            raise ValueError(f'EvalMeter.update: logits must be (B, {self.num_class}), got {tuple(getattr(logits, "shape", ()))}')
        ops.eval_accumulate(logits, labels, self.counts, self.sums, self.confusion, self.topk, index=index, valid=valid,
                            scores=self.scores, base=self._base)
        self._base += logits.shape[0] if valid is None or torch.is_tensor(valid) else int(valid)

    def compute(self):
        """-> dict: loss (mean of the batch means, the reference's np.mean(loss_value)), sample_loss (mean over the samples),
        count (samples kept), top1, topk {k: ratio}, confusion int64 (K, K) numpy [label, prediction], class_acc {class:
        (correct, total, ratio)} with (0, 0, 0.0) for an empty class, scores numpy (num_samples, K) | None, bad_labels,
        bad_index, batches.  Ratios of an empty meter are NaN."""
        counts = self.counts.cpu().tolist()
        sums = self.sums.cpu().tolist()
        conf = self.confusion.cpu().numpy().astype('int64')
        batches, count = counts[0], counts[1]
        nan = float('nan')
        diag, tot = conf.diagonal(), conf.sum(axis=1)
        cls = {c: ((int(diag[c]), int(tot[c]), diag[c] / tot[c]) if tot[c] > 0 else (0, 0, 0.0)) for c in range(self.num_class)}
        return {'loss': sums[0] / batches if batches else nan, 'sample_loss': sums[1] / count if count else nan,
                'count': count, 'batches': batches, 'top1': int(diag.sum()) / count if count else nan,
                'topk': {k: (counts[4 + i] / count if count else nan) for i, k in enumerate(self.topk)},
                'confusion': conf, 'class_acc': cls, 'scores': None if self.scores is None else self.scores.cpu().numpy(),
                'bad_labels': counts[2], 'bad_index': counts[3]}


def _state_key(model):
    """What the eval path's folded coefficients are keyed on (f2.FusedEval._state_key, functional._eval_cached), for a whole model."""
    watch = list(model.parameters()) + list(model.buffers())
    arenas = {}
    for t in watch:
        a = getattr(t, '_tamgcn_arena', None)
        if a is not None:
            arenas[id(a)] = a
    mods = list(model.modules())
    return (tuple((t.data_ptr(), t._version) for t in watch),
            tuple(Fn._bn_epoch(m)[0] for m in mods if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)),
            tuple(v for a in arenas.values() for v in a.state_version()), tuple(id(m) for m in mods))


class CapturedEval:
    """model: a models.ctrgcn.Model or an inference.StreamEnsemble in eval() mode; feeder: a val-split Feeder (or None);
    batch_size B; topk as EvalMeter's.

    run() -> the EvalMeter after one pass over the split in file order, ceil(len / B) batches: per batch a GraphedBatch replay,
    a GraphedForward replay and the meter's launch, all on the current stream -- no host synchronisation and no device-to-host
    copy (run().compute() is the one).  The last batch is padded to B with sample 0; the meter is told how many rows count
    (eval-mode samples do not influence each other).  The scores of sample i are row i of compute()['scores'].

    Without a feeder -- CapturedEval(model, None, B, example_x=x0, num_samples=n) -- the caller brings the batches:
    reset(), update(x, y, index=None, valid=None) per batch (x of example_x's shape), then meter.compute().

    The forward graph is captured when this object is built and again by the first run() / update() after the model's state key
    moved (an optimiser step on the arena, a CapturedStep replay, load_state_dict, an in-place edit); such a capture
    synchronises, a run on unchanged parameters does not.  run() and update() raise while the model is in train() mode."""

    def __init__(self, model, feeder, batch_size, topk=(1, 5), example_x=None, num_samples=None):
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f'CapturedEval: batch_size = {batch_size!r} must be an integer >= 1')
        if model.training:
            raise ValueError('CapturedEval: put the model in eval() mode first (CapturedStep refuses the converse)')
        self.model, self.feeder, self.batch_size = model, feeder, batch_size
        if feeder is not None:
            from .feeder.feeder_nucla_gcn import GraphedBatch
            if feeder.train_val != 'val':
                raise ValueError('CapturedEval: the feeder is a train split (its batches are augmented); build it with a val label_path')
            n = len(feeder)
            if n < 1:
                raise ValueError('CapturedEval: the split is empty')
            self._gb = GraphedBatch(feeder, batch_size)
            example_x, num_samples = self._gb.x, n
            dev = example_x.device
            nb = -(-n // batch_size)
            idx = torch.zeros(nb * batch_size, dtype=torch.int64)
            idx[:n] = torch.arange(n)
            self._idx = idx.view(nb, batch_size).to(dev)             # every batch's indices, made once
            self._valid = [min(batch_size, n - b * batch_size) for b in range(nb)]
        else:
            if not torch.is_tensor(example_x) or not example_x.is_cuda or example_x.shape[0] != batch_size:
                raise ValueError('CapturedEval: without a feeder pass example_x, a HIP tensor of one batch (batch_size rows)')
            self._gb = None
        if getattr(model, 'arrangement', None) == 'streams':
            raise ValueError("CapturedEval: a StreamEnsemble with arrangement='streams' forks HIP streams inside the captured graph; "
                             "the evaluation pass stays on one stream (arrangement None, 'grouped' or 'serial')")
        self._shape, self._dtype = tuple(example_x.shape), example_x.dtype
        self._fwd = GraphedForward(model)
        self._key = _state_key(model)
        out = self._forward(example_x)                               # captures now; K from the logits
        if out.dim() != 2 or out.shape[0] != batch_size:
            raise ValueError(f'CapturedEval: the model returned {tuple(out.shape)}, expected ({batch_size}, num_class)')
        self.meter = EvalMeter(out.shape[1], num_samples, topk, device=out.device)
        self.captures = 1

    def _current(self):
        if self.model.training:
            raise RuntimeError('CapturedEval: the model is in train() mode; call model.eval() before an evaluation pass')
        key = _state_key(self.model)
        if key != self._key:
            self._fwd.reset()                                        # the next call captures under the current state
            self._key = key
            self.captures += 1

    def _forward(self, x):
        m = self.model
        if getattr(m, 'arrangement', 0) is not None:
            return self._fwd(x)
        # A StreamEnsemble left to choose would put its models on side streams when GraphedForward captures it; here the graph
        # stays one chain of launches: the grouped sequence where it applies, the models one after the other elsewhere.
        m.arrangement = 'grouped'
        try:
            return self._fwd(x)
        finally:
            m.arrangement = None

    def reset(self):
        self.meter.reset()

    def update(self, x, y, index=None, valid=None):
        if not torch.is_tensor(x) or tuple(x.shape) != self._shape or x.dtype != self._dtype or not x.is_cuda:
            raise ValueError(f'CapturedEval.update: x must be a {self._dtype} HIP tensor of shape {self._shape}')
        self._current()
        self.meter.update(self._forward(x), y, index=index, valid=valid)

    def run(self):
        if self._gb is None:
            raise RuntimeError('CapturedEval.run: built without a feeder; feed batches through update()')
        self._current()
        self.meter.reset()
        for idx, valid in zip(self._idx, self._valid):
            x, y = self._gb(idx)
            self.meter.update(self._forward(x), y, index=idx, valid=valid)
        return self.meter
