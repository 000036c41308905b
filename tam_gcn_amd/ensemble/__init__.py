"""Score-level ensemble of the evaluation scripts on the GPU.

Mirrors what the reference's two ensemble scripts compute once every model has produced its per-sample class scores:

    ensemble/ensemble_resnet_ctrgcn.py:42-61          final = score_a + alpha * score_b on the RAW scores, samples matched by
                                                      name, names missing from either file skipped, top-1 accuracy
    ensemble/ensemble_ctrgcn_resnet_eval.py:99-108    the same on softmax-normalised scores
    ensemble/ensemble_ctrgcn_resnet_eval.py:217-234   compute_accuracy: overall + per-class (correct, total, ratio)
    ensemble/ensemble_ctrgcn_resnet_eval.py:421-438   the accuracy of score_a + alpha * score_b over a list of alphas, best alpha

Only the arithmetic runs on the device (one launch of tamgcn_score_fuse for any number of score sets); matching names is
host bookkeeping, as in the reference.  Reading / writing the score pickles, the models' inference loops and the plots are
the scripts' own business (out of scope)."""
import numpy as np
import torch

from .. import ops

__all__ = ['fuse', 'compute_accuracy', 'ensemble_by_name', 'sweep', 'REFERENCE_ALPHAS']

REFERENCE_ALPHAS = (0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 1.5, 2.0, 3.0)      # ensemble_ctrgcn_resnet_eval.py:428


def fuse(scores, weights, softmax=False, labels=None):
    """scores: sequence of S (N, K) arrays / tensors (one per model or stream), weights: S floats.
    -> fused (N, K) f32, pred (N,) int64, class_stats (K, 2) int32 [correct, total] or None -- HIP tensors."""
    dev = torch.device('cuda', torch.cuda.current_device())
    st = torch.stack([torch.as_tensor(np.asarray(s) if not torch.is_tensor(s) else s, dtype=torch.float32).to(dev) for s in scores]).contiguous()
    if st.dim() != 3 or len(weights) != st.shape[0]:
        raise ValueError('fuse: need S score sets of one (N, K) shape and S weights')
    w = torch.tensor([float(a) for a in weights], dtype=torch.float32, device=dev)
    lab = None
    if labels is not None:
        lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(dev, torch.int64).contiguous()
        if lab.shape != (st.shape[1],):
            raise ValueError('fuse: one label per sample')
        if bool(((lab < 0) | (lab >= st.shape[2])).any()):         # the kernel would leave it out of every class row, while
            raise ValueError('fuse: label outside [0, K)')         # the scripts' accuracy divides by len(labels)
    return ops.score_fuse(st, w, softmax, lab)


def compute_accuracy(scores, labels):
    """(acc, correct, total, {class: (correct, total, ratio)}) of one score set -- the reference's compute_accuracy."""
    scores = scores if torch.is_tensor(scores) else np.asarray(scores)
    _, _, stats = fuse([scores], [1.0], softmax=False, labels=labels)
    st = stats.cpu().numpy()
    correct, total = int(st[:, 0].sum()), int(st[:, 1].sum())
    cls = {c: ((int(st[c, 0]), int(st[c, 1]), st[c, 0] / st[c, 1]) if st[c, 1] > 0 else (0, 0, 0.0)) for c in range(st.shape[0])}
    return correct / total, correct, total, cls


def ensemble_by_name(score_dicts, weights, names, labels, softmax=False):
    """score_dicts: S mappings name -> (K,) scores; names / labels: the label file's two lists.  Samples missing from any
    mapping are skipped (the reference prints a warning and continues, ensemble_resnet_ctrgcn.py:46-48).
    -> dict(acc, correct, total, pred {name: class}, skipped [names], class_acc)"""
    keep = [i for i, n in enumerate(names) if all(n in d for d in score_dicts)]
    skipped = [n for n in names if not all(n in d for d in score_dicts)]
    if not keep:
        raise ValueError('ensemble_by_name: no sample is present in every score set')
    mats = [np.stack([np.asarray(d[names[i]], dtype=np.float32) for i in keep]) for d in score_dicts]
    lab = np.asarray([int(labels[i]) for i in keep], dtype=np.int64)
    _, pred, stats = fuse(mats, weights, softmax=softmax, labels=lab)
    pred = pred.cpu().numpy()
    st = stats.cpu().numpy()
    correct, total = int(st[:, 0].sum()), int(st[:, 1].sum())
    cls = {c: ((int(st[c, 0]), int(st[c, 1]), st[c, 0] / st[c, 1]) if st[c, 1] > 0 else (0, 0, 0.0)) for c in range(st.shape[0])}
    return dict(acc=correct / total, correct=correct, total=total, pred={names[i]: int(p) for i, p in zip(keep, pred)},
                skipped=skipped, class_acc=cls)


def best_alpha(alphas, accs, start_alpha=None, start_acc=None):
    """The reference's choice (ensemble_ctrgcn_resnet_eval.py:425-436): begin with (start_alpha, start_acc) and move to a
    later alpha only when its accuracy is STRICTLY greater.  Without a start the first alpha is the start."""
    alphas, accs = list(alphas), list(accs)
    if start_alpha is None:
        best, best_acc = alphas[0], accs[0]
    else:
        best, best_acc = start_alpha, start_acc
    for a, acc in zip(alphas, accs):
        if acc > best_acc:
            best, best_acc = a, acc
    return best, best_acc


def sweep(score_a, score_b, alphas=REFERENCE_ALPHAS, labels=None, softmax=False, start_alpha=None):
    """Top-1 accuracy of score_a + alpha * score_b for every alpha in ONE launch (tamgcn_score_sweep), fused exactly as
    ``fuse([score_a, score_b], [1.0, alpha], softmax)`` fuses: -> (accs [len(alphas)] floats, best alpha, its accuracy).
    start_alpha: the reference's args.alpha, whose accuracy the search starts from (best_alpha()).  Accuracies divide by
    len(labels), as the script's do; labels must lie in [0, K)."""
    if labels is None:
        raise ValueError('sweep: labels are needed')
    dev = torch.device('cuda', torch.cuda.current_device())
    a, b = (torch.as_tensor(np.asarray(s) if not torch.is_tensor(s) else s, dtype=torch.float32).to(dev).contiguous() for s in (score_a, score_b))
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError('sweep: need two score sets of one (N, K) shape')
    lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(dev, torch.int64).contiguous()
    if lab.shape != (a.shape[0],):
        raise ValueError('sweep: one label per sample')
    if bool(((lab < 0) | (lab >= a.shape[1])).any()):
        raise ValueError('sweep: label outside [0, K)')
    alphas = [float(x) for x in alphas]
    if not alphas:
        raise ValueError('sweep: no alphas')
    todo = alphas + ([float(start_alpha)] if start_alpha is not None else [])
    correct = []
    for i in range(0, len(todo), ops.SWEEP_MAX_ALPHAS):
        correct += ops.score_sweep(a, b, todo[i:i + ops.SWEEP_MAX_ALPHAS], lab, softmax).tolist()
    accs = [c / a.shape[0] for c in correct]
    best, best_acc = best_alpha(alphas, accs[:len(alphas)], start_alpha, accs[-1] if start_alpha is not None else None)
    return accs[:len(alphas)], best, best_acc
