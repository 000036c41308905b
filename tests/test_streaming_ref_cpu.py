"""tests/streaming_ref.py (the restatement the GPU tests of csrc/streaming.hip lean on) against plain slicing and brute force, and
tam_gcn_amd.streaming's host-side plan against it.  No GPU."""
import numpy as np
import pytest

import streaming_ref as R
from tam_gcn_amd import streaming


def test_ring_model_equals_slicing_across_the_wrap():
    seq = np.random.default_rng(0).normal(size=(38, 4, 3))
    ring = R.Ring(16)
    at = 0
    for n in (5, 7, 9, 1, 16):
        ring.push(seq[at:at + n])
        at += n
        assert ring.count == at
        for L in (1, 9, 16):
            for start in range(max(0, at - 16), at - L + 1):
                assert np.array_equal(np.stack(ring.window(start, L)), seq[start:start + L]), (at, start, L)
    assert ring.pushes == 5
    with pytest.raises(AssertionError):
        ring.window(at - 17, 3)                    # overwritten


def test_plan_live_marks_what_is_gone_or_not_there_yet():
    assert R.plan_live(5, 16, 3, 9, 4).tolist() == [[0, 0], [0, 0], [0, 0]]
    assert R.plan_live(12, 16, 3, 9, 4).tolist() == [[0, 0], [0, 0], [3, 9]]
    assert R.plan_live(17, 16, 3, 9, 4).tolist() == [[0, 0], [4, 9], [8, 9]]        # frame 0 is overwritten
    assert R.plan_live(16, 16, 3, 9, 4).tolist() == [[0, 0], [3, 9], [7, 9]]        # would start at -1
    assert R.plan_live(40, 16, 3, 9, 4).tolist() == [[0, 0], [27, 9], [31, 9]]       # 23 < 40 - 16: overwritten


@pytest.mark.parametrize('length,window,hop', [(70, 20, 8), (20, 20, 8), (21, 20, 8), (68, 20, 8), (7, 20, 8), (1, 1, 1),
                                               (2000, 40, 8), (53, 9, 4)])
def test_plan_offline_covers_every_frame_and_stays_inside(length, window, hop):
    plan = R.plan_offline(length, window, hop)
    assert plan.tolist() == [list(r) for r in streaming.plan_offline(length, window, hop)]
    covered = np.zeros(length, dtype=int)
    for start, L in plan:
        assert 0 <= start and start + L <= length and L == min(window, length)
        covered[start:start + L] += 1
    assert covered.min() >= 1
    assert len({tuple(r) for r in plan.tolist()}) == len(plan)                         # no window twice
    if length < window:
        assert plan.tolist() == [[0, length]]
    else:
        regular = [r for r in plan.tolist() if r[0] % hop == 0]
        assert len(regular) == (length - window) // hop + 1 and len(plan) - len(regular) <= 1


@pytest.mark.parametrize('name', sorted(R.VOTE_CASES))
def test_vote_equals_the_double_loop_and_no_frame_is_a_near_tie(name):
    logits, plan, frames = R.vote_case(name)
    B, K = logits.shape
    probs, scores, label, cover = R.vote(logits, plan, frames)
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-14) and (probs > 0).all()
    p32 = probs.astype(np.float32)
    uncovered = 0
    for f in range(frames):
        rows = [j for j in range(B) if plan[j, 1] >= 1 and plan[j, 0] <= f < plan[j, 0] + plan[j, 1]]
        assert cover[f] == len(rows)
        if not rows:
            uncovered += 1
            assert label[f] == -1 and not scores[f].any()
            continue
        want = [sum(float(p32[j, k]) for j in rows) / len(rows) for k in range(K)]
        assert np.allclose(scores[f], want, rtol=0, atol=1e-15)
        assert label[f] == int(np.argmax(scores[f]))
    assert uncovered >= 2
    if R.VOTE_CASES[name][5] is not None:
        assert (plan[R.VOTE_CASES[name][5]] == 0).all()
    # the GPU test compares labels on every frame whose two largest scores differ by more than twice the bound: that is all of them
    cov = cover > 0
    bound = R.score_bound(np.sort(scores, axis=1)[:, -1], K, cover)
    assert (R.top2_gap(scores)[cov] > 2 * bound[cov]).all()


def test_the_label_is_the_first_of_tied_maxima():
    assert R.first_argmax(np.array([0.1, 0.4, 0.4, 0.1])) == 1
    assert R.first_argmax(np.array([0.25, 0.25, 0.25, 0.25])) == 0
    logits = np.zeros((2, 4), dtype=np.float32)
    logits[:, 1] = logits[:, 3] = 2.0                                                   # classes 1 and 3 tie in every window
    _, scores, label, _ = R.vote(logits, np.array([(0, 3), (2, 3)]), 6)
    assert label.tolist() == [1, 1, 1, 1, 1, -1] and scores[0, 1] == scores[0, 3]
    steps = R.ema(np.array([[0.5, 0.5], [0.2, 0.8]], dtype=np.float32), [False, True], 0.5)
    assert steps[0][1:] == (0, -1) and steps[1][1:] == (1, 1)
    tie = R.ema(np.array([[0.5, 0.5]], dtype=np.float32), [True], 0.0)
    assert tie[0][2] == 0


def test_ema_first_valid_step_sets_and_invalid_steps_hold():
    rng = np.random.default_rng(3)
    rows = R.softmax(rng.uniform(-3, 3, size=(6, 5))).astype(np.float32)
    valid = [False, True, True, False, True, True]
    for beta in (0.0, 0.8):
        steps = R.ema(rows, valid, beta)
        assert not steps[0][0].any() and steps[0][1] == 0
        assert np.array_equal(steps[1][0], rows[1].astype(np.float64))
        assert np.array_equal(steps[3][0], steps[2][0]) and steps[3][1] == steps[2][1] == 2
        assert np.allclose(steps[2][0], beta * rows[1].astype(np.float64) + (1 - beta) * rows[2].astype(np.float64), rtol=0, atol=1e-16)
        assert steps[-1][1] == 4
        if beta == 0.0:
            assert np.array_equal(steps[-1][0], rows[-1].astype(np.float64))


def test_window_builders_are_the_feeders_references():
    from oracle import feeder_oracle
    import clip_resize_ref
    rng = np.random.default_rng(4)
    frames = rng.normal(size=(9, 20, 3))
    got = R.window_nucla(frames, 'bone', 8)
    want = feeder_oracle.transform(frames, 0, 0, 1.0, np.linspace(0, 8, 8).astype(int), 'bone', 8)
    assert got.shape == (3, 8, 20, 1) and got.dtype == np.float32 and np.array_equal(got, want)
    one = R.window_nucla(frames[:1], 'joint', 52)
    assert np.isfinite(one).all()                                                       # hi == lo: the 1e-6 carries the division
    seq = rng.uniform(-1, 1, size=(3, 23, 17, 1)).astype(np.float32)
    out, bound = R.window_clip(seq, 4, 8, 8)
    assert np.array_equal(out, seq[:, 4:12].astype(np.float64)) and out.shape == bound.shape
    want, _ = clip_resize_ref.resize(seq, 2, 13, 8)
    assert np.array_equal(R.window_clip(seq, 2, 13, 8)[0], want)
