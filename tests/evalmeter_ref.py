"""numpy restatement, in fp64, of what tamgcn_eval_accumulate adds to an evaluation state (include/tamgcn.h; not a test file).
Shared by tests/test_evalmeter_cpu.py (held against the reference's own three formulas) and the GPU tests.

    prediction   np.argmax                                                      (processor/recognition_rgb.py:94)
    top-k        label in np.argsort(row, kind='stable')[-k:]                   (feeder/feeder_nucla_gcn.py top_k, ties stable)
    confusion    np.add.at(conf, (label, prediction), 1)                        (sklearn.metrics.confusion_matrix orientation)
    loss         logsumexp(row) - row[label] by max-shift; batch mean over the kept rows; epoch loss = mean of batch means

A row is kept when its label is in [0, K); label -100 is skipped silently, any other label outside [0, K) is counted as bad
and makes that batch's mean NaN; a batch without a kept row adds nothing.  Scores: row index[n] (or the next free row) of a
NaN-filled table gets logits[n]; an index outside the table stores nothing and is counted."""
import numpy as np

IGNORE = -100


def row_losses(logits, labels):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
    return lse - x[np.arange(len(x)), labels]


def topk_hits(logits, labels, k):
    rank = np.argsort(np.asarray(logits), axis=1, kind='stable')
    return np.array([l in rank[i, -k:] for i, l in enumerate(labels)], dtype=bool)


class Meter:
    def __init__(self, K, num_samples=None, topk=(1, 5)):
        self.K, self.topk = K, tuple(topk)
        self.batches = self.count = self.bad_labels = self.bad_index = 0
        self.hits = [0] * len(self.topk)
        self.sum_mean = self.sum_rows = 0.0
        self.confusion = np.zeros((K, K), dtype=np.int64)
        self.scores = None if num_samples is None else np.full((num_samples, K), np.nan, dtype=np.float32)
        self.base = 0
        self.batch_means = []

    def update(self, logits, labels, index=None, valid=None):
        logits, labels = np.asarray(logits), np.asarray(labels)
        B = len(logits)
        valid = B if valid is None else int(valid)
        lg, lab = logits[:valid], labels[:valid]
        if self.scores is not None:
            rows = np.asarray(index)[:valid] if index is not None else self.base + np.arange(valid)
            for n, r in enumerate(rows):
                if 0 <= r < len(self.scores):
                    self.scores[r] = lg[n]
                else:
                    self.bad_index += 1
        self.base += valid
        keep = (lab >= 0) & (lab < self.K)
        nbad = int(((~keep) & (lab != IGNORE)).sum())
        self.bad_labels += nbad
        if not keep.any():
            return
        lg, lab = lg[keep], lab[keep]
        losses = row_losses(lg, lab)
        mean = np.nan if nbad else losses.sum() / len(lab)
        self.batch_means.append(mean)
        self.batches += 1
        self.count += len(lab)
        self.sum_mean += mean
        self.sum_rows += losses.sum()
        np.add.at(self.confusion, (lab, np.argmax(lg, axis=1)), 1)
        for i, k in enumerate(self.topk):
            self.hits[i] += int(topk_hits(lg, lab, k).sum())

    def compute(self):
        nan = float('nan')
        diag, tot = self.confusion.diagonal(), self.confusion.sum(axis=1)
        return {'loss': self.sum_mean / self.batches if self.batches else nan,
                'sample_loss': self.sum_rows / self.count if self.count else nan,
                'count': self.count, 'batches': self.batches, 'top1': int(diag.sum()) / self.count if self.count else nan,
                'topk': {k: (h / self.count if self.count else nan) for k, h in zip(self.topk, self.hits)},
                'confusion': self.confusion,
                'class_acc': {c: ((int(diag[c]), int(tot[c]), diag[c] / tot[c]) if tot[c] > 0 else (0, 0, 0.0)) for c in range(self.K)},
                'scores': self.scores, 'bad_labels': self.bad_labels, 'bad_index': self.bad_index}


def assert_same_metrics(got, ref, loss_rtol=2e-6):
    """Everything integer exactly; the two losses within loss_rtol * max(1, |ref|) (NaN where the restatement's is NaN)."""
    for k in ('count', 'batches', 'bad_labels', 'bad_index'):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.array_equal(got['confusion'], ref['confusion']), (got['confusion'], ref['confusion'])
    assert got['confusion'].dtype == np.int64
    assert got['class_acc'] == ref['class_acc']
    for k in ref['topk']:
        assert got['topk'][k] == ref['topk'][k] or (np.isnan(got['topk'][k]) and np.isnan(ref['topk'][k])), (k, got['topk'], ref['topk'])
    assert got['top1'] == ref['top1'] or (np.isnan(got['top1']) and np.isnan(ref['top1']))
    for k in ('loss', 'sample_loss'):
        if np.isnan(ref[k]):
            assert np.isnan(got[k]), (k, got[k])
        else:
            assert abs(got[k] - ref[k]) <= loss_rtol * max(1.0, abs(ref[k])), (k, got[k], ref[k])
