"""No GPU: the fp64 restatement of the evaluation meter (tests/evalmeter_ref.py) against the reference's own formulas, the
argument checks of the two new entry points, and ensemble.sweep's best-alpha rule."""
import ctypes as C
import types

import numpy as np
import pytest

import evalmeter_ref as R

SHAPES = [(1, 3), (7, 60), (256, 10), (300, 10)]
TOPK = (1, 2, 5, 70)


def _tie_free(B, K, seed):
    rng = np.random.default_rng(seed)
    x = (3 * rng.standard_normal((B, K))).astype(np.float32)
    assert all(len(np.unique(r)) == K for r in x)              # no ties: plain argsort() and the stable one agree
    return x, rng.integers(0, K, size=B)


@pytest.mark.parametrize('B,K', SHAPES)
def test_restatement_equals_the_reference_formulas(B, K):
    from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder
    x, lab = _tie_free(B, K, seed=B + K)
    m = R.Meter(K, num_samples=B, topk=TOPK)
    m.update(x, lab)
    res = m.compute()
    # processor/recognition_rgb.py:94-95
    predict_label = np.argmax(x, axis=1)
    assert res['top1'] == np.sum(predict_label == lab) / len(lab)
    # feeder/feeder_nucla_gcn.py top_k (the mirror keeps the reference's two lines), plain argsort()
    fd = types.SimpleNamespace(label=list(lab))
    for k in TOPK:
        assert res['topk'][k] == Feeder.top_k(fd, x, k)
    assert res['topk'][70] == 1.0                              # k >= K always hits
    assert res['topk'][1] == res['top1']                       # tie-free rows: the two rules meet
    # nn.CrossEntropyLoss (mean) in fp64, and np.mean(loss_value) over one batch
    import torch
    ref = float(torch.nn.functional.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(lab)))
    assert abs(res['loss'] - ref) <= 1e-12 * max(1.0, abs(ref)) and abs(res['sample_loss'] - ref) <= 1e-12 * max(1.0, abs(ref))
    assert np.array_equal(res['scores'], x)
    # ensemble/__init__.py compute_accuracy's per-class triple
    for c in range(K):
        tot = int((lab == c).sum())
        cor = int(((lab == c) & (predict_label == c)).sum())
        assert res['class_acc'][c] == ((cor, tot, cor / tot) if tot else (0, 0, 0.0))


@pytest.mark.parametrize('B,K', SHAPES)
def test_confusion_orientation_is_sklearns(B, K):
    skm = pytest.importorskip('sklearn.metrics')
    x, lab = _tie_free(B, K, seed=B + K)
    m = R.Meter(K)
    m.update(x, lab)
    assert np.array_equal(m.confusion, skm.confusion_matrix(lab, np.argmax(x, axis=1), labels=np.arange(K)))


def test_counting_rule_for_ties_is_the_stable_argsort():
    """The kernel's hit rule, #{j : s_j > s_l} + #{j > l : s_j == s_l} < k, on integer-valued rows full of ties."""
    rng = np.random.default_rng(3)
    for B, K in SHAPES:
        x = rng.integers(-2, 3, size=(B, K)).astype(np.float32)
        lab = rng.integers(0, K, size=B)
        sl = x[np.arange(B), lab][:, None]
        above = (x > sl).sum(axis=1) + ((x == sl) & (np.arange(K)[None, :] > lab[:, None])).sum(axis=1)
        for k in TOPK:
            assert np.array_equal(above < k, R.topk_hits(x, lab, k)), (B, K, k)


def test_conventions_of_labels_batches_and_indices():
    K = 5
    rng = np.random.default_rng(9)
    x = rng.standard_normal((6, K)).astype(np.float32)
    m = R.Meter(K, num_samples=4, topk=(1,))
    m.update(x, np.array([0, -100, 1, 2, 3, 4]), index=np.array([3, -1, 4, 0, 1, 2]), valid=4)     # rows 4, 5 do not count
    assert (m.count, m.batches, m.bad_labels, m.bad_index) == (3, 1, 0, 2)
    assert np.array_equal(m.scores[3], x[0]) and np.array_equal(m.scores[0], x[3]) and np.isnan(m.scores[1:3]).all()
    m.update(x, np.array([-100] * 6))                                                             # nothing kept: not a batch
    assert (m.count, m.batches) == (3, 1) and not np.isnan(m.compute()['loss'])
    m.update(x, np.array([0, K + 3, 1, 1, 1, 1]))                                                 # a bad label: this batch's mean is NaN
    res = m.compute()
    assert (res['count'], res['batches'], res['bad_labels']) == (8, 2, 1)
    assert np.isnan(res['loss']) and np.isfinite(res['sample_loss'])
    assert R.Meter(K).compute()['class_acc'][0] == (0, 0, 0.0)


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from tam_gcn_amd import build, _lib
    build.build()
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    tk = (C.c_int * 5)(1, 2, 3, 4, 5)

    def acc(logits=p, labels=p, B=4, K=3, nk=2, counts=p, sums=p, conf=p, topk=tk):
        return lib.tamgcn_eval_accumulate(logits, labels, None, B, K, B, None, topk, nk, 0, 0, counts, sums, conf, None, None)
    bad = [dict(logits=None), dict(labels=None), dict(counts=None), dict(sums=None), dict(conf=None), dict(B=0), dict(B=-3), dict(K=0),
           dict(nk=5), dict(nk=-1), dict(nk=2, topk=None)]
    for kw in bad:
        assert acc(**kw) < 0, kw
        assert b'tamgcn_eval_accumulate' in lib.tamgcn_last_error(), (kw, lib.tamgcn_last_error())
    # scores without a table size
    assert lib.tamgcn_eval_accumulate(p, p, None, 4, 3, 4, None, tk, 2, 0, 0, p, p, p, p, None) < 0
    assert b'tamgcn_eval_accumulate' in lib.tamgcn_last_error()

    al = (C.c_float * 20)(*([0.5] * 20))

    def sweep(a=p, b=p, alphas=al, A=9, N=4, K=3, labels=p, correct=p):
        return lib.tamgcn_score_sweep(a, b, alphas, A, N, K, 0, labels, correct, None)
    for kw in [dict(a=None), dict(b=None), dict(alphas=None), dict(labels=None), dict(correct=None), dict(A=0), dict(A=17), dict(N=0), dict(K=0)]:
        assert sweep(**kw) < 0, kw
        assert b'tamgcn_score_sweep' in lib.tamgcn_last_error(), (kw, lib.tamgcn_last_error())
    assert lib.tamgcn_version() == 401


def test_best_alpha_moves_only_on_strictly_greater():
    from tam_gcn_amd.ensemble import best_alpha, REFERENCE_ALPHAS
    assert REFERENCE_ALPHAS == (0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 1.5, 2.0, 3.0)
    accs = [0.50, 0.60, 0.60, 0.55, 0.70, 0.70, 0.65, 0.70, 0.10]
    # from the start alpha's accuracy: a tie with the start does not replace it, the FIRST strictly greater one does
    assert best_alpha(REFERENCE_ALPHAS, accs, start_alpha=1.0, start_acc=0.70) == (1.0, 0.70)
    assert best_alpha(REFERENCE_ALPHAS, accs, start_alpha=0.25, start_acc=0.60) == (0.7, 0.70)
    assert best_alpha(REFERENCE_ALPHAS, accs, start_alpha=0.25, start_acc=0.95) == (0.25, 0.95)
    # no start: the first alpha is the start; later equal accuracies never replace an earlier one
    assert best_alpha(REFERENCE_ALPHAS, accs) == (0.7, 0.70)
    assert best_alpha([1.0, 2.0], [0.3, 0.3]) == (1.0, 0.3)
