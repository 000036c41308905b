"""tests/streambank_ref.py against hand-written cases: a bank's feed is a single ring that saw only its own ticks, a restart is a
fresh ring, and the decision log's edges."""
import numpy as np

import streaming_ref as R
import streambank_ref as BR


def _frames(S, n, tick):
    """feed s, frame i of tick t is the tuple (s, t, i): whatever is pushed can be told apart."""
    return [[(s, tick, i) for i in range(n)] for s in range(S)]


def test_a_feed_that_skips_ticks_is_a_ring_that_was_not_pushed_on_them():
    bank, alone = BR.Bank(3, 5), R.Ring(5)
    pattern = [(2, 1, 0), (2, 0, 2), (1, 0, 0), (2, 2, 1), (0, 0, 2), (2, 1, 0), (2, 0, 1)]
    for t, counts in enumerate(pattern):
        fr = _frames(3, 2, t)
        before = (list(bank.rings[1].slots), bank.rings[1].count, bank.rings[1].pushes)
        bank.push(fr, counts)
        if counts[1]:
            alone.push(fr[1][:counts[1]])
        else:
            assert (bank.rings[1].slots, bank.rings[1].count, bank.rings[1].pushes) == before     # nothing of it moved
        assert bank.rings[1].slots == alone.slots and bank.rings[1].count == alone.count and bank.rings[1].pushes == alone.pushes
    assert bank.state().tolist() == [[11, 6], [4, 3], [6, 4]]
    assert bank.rings[0].count > 5 and bank.rings[2].count > 5                                        # they wrapped
    # counts are clamped into 0..n, and None takes everything
    b2 = BR.Bank(2, 5)
    b2.push(_frames(2, 2, 0), (-3, 7))
    assert b2.state().tolist() == [[0, 0], [2, 1]]
    b2.push(_frames(2, 2, 1))
    assert b2.state().tolist() == [[2, 1], [4, 2]]


def test_a_restart_is_a_fresh_ring():
    bank = BR.Bank(2, 5)
    for t in range(4):
        bank.push(_frames(2, 2, t))
    bank.push(_frames(2, 2, 4), counts=(1, 2), restart=(1, 0))                     # restarts and pushes on the same tick
    fresh = R.Ring(5)
    fresh.push([(0, 4, 0)])
    assert bank.rings[0].slots == fresh.slots and bank.state().tolist() == [[1, 1], [10, 5]]
    bank.push(_frames(2, 2, 5), counts=(0, 0), restart=(0, 1))                     # restarts and takes nothing
    assert bank.state().tolist() == [[1, 1], [0, 0]] and bank.rings[1].slots == [None] * 5
    # the plan: a feed that takes nothing has no window; a restarted feed has none until `window` frames are in again
    assert bank.plan(2, 1, 1, counts=(1, 0)).tolist() == [[0, 0], [0, 1], [0, 0], [0, 0]]
    assert bank.plan(1, 1, 1).tolist() == [[0, 1], [0, 0]]


def test_the_averages_follow_ema_per_feed_and_forget_on_restart():
    rows = R.softmax(R.vote_logits(12, 10, 7)).astype(np.float32)
    av = BR.Averages(2, 10, 0.8)
    alone_rows, alone_valid = [], []
    for t in range(6):
        valid = [[t != 2, True], [t % 2 == 0, False]]
        got = av.tick([[rows[2 * t], rows[2 * t + 1]], [rows[2 * t], rows[2 * t + 1]]], valid, restart=(0, 1) if t == 4 else None)
        alone_rows += [rows[2 * t], rows[2 * t + 1]]
        alone_valid += valid[0]
        e, seen, lab = R.ema(np.stack(alone_rows), alone_valid, 0.8)[-1]
        assert np.array_equal(got[0][0], e) and got[0][1:] == (seen, lab, True)
        assert got[1][3] == (t % 2 == 0)
    assert av.seen == [11, 1] and np.array_equal(av.e[1], rows[8].astype(np.float64))          # feed 1 forgot ticks 0 and 2 at tick 4
    fresh = BR.Averages(1, 10, 0.8).tick([[rows[0]]], [[False]], restart=(1,))
    assert fresh[0][1:] == (0, -1, False) and not fresh[0][0].any()


def test_the_log_fills_and_counts_the_drops():
    ticks, S = 3, 4
    labels = np.array([[1, 2, 3, 4], [5, 2, 6, 4], [5, 7, 6, 8]])
    confs = np.full((ticks, S), 0.9, dtype=np.float32)
    adv = np.ones((ticks, S), dtype=bool)
    stable, rows, rc, dropped = BR.decide(labels, confs, adv, threshold=0.5, hold=1, capacity=5)
    assert stable.tolist() == labels.tolist()                                       # hold = 1: every confident label is stable at once
    assert rows.tolist() == [[0, 0, 1], [1, 0, 2], [2, 0, 3], [3, 0, 4], [0, 1, 5]]     # tick, then feed ascending; never overwritten
    assert dropped == 3 and rc.dtype == np.float32 and rc.tolist() == [np.float32(0.9)] * 5
    _, rows, _, dropped = BR.decide(labels, confs, adv, threshold=0.5, hold=1)
    assert len(rows) == 8 and dropped == 0
    assert rows[5:].tolist() == [[2, 1, 6], [1, 2, 7], [3, 2, 8]]


def test_hold_and_threshold_edges():
    thr = 0.6
    at = np.float32(thr)                                                             # conf == float32(threshold) counts
    below = np.nextafter(at, np.float32(0))
    # feed 0: label 3 three times at exactly the threshold -> stable at the third tick (hold = 3), one event
    # feed 1: 3, 3, then a flip to 4 resets the run: 4 needs three ticks of its own
    # feed 2: one tick below the threshold in between clears the candidate
    labels = np.zeros((6, 3), dtype=np.int64)
    labels[:, 0] = 3
    labels[:, 1] = [3, 3, 4, 4, 4, 4]
    labels[:, 2] = [3, 3, 3, 3, 3, 3]
    confs = np.full((6, 3), at, dtype=np.float32)
    confs[2, 2] = below
    adv = np.ones((6, 3), dtype=bool)
    stable, rows, rc, dropped = BR.decide(labels, confs, adv, threshold=thr, hold=3)
    assert stable[:, 0].tolist() == [-1, -1, 3, 3, 3, 3]
    assert stable[:, 1].tolist() == [-1, -1, -1, -1, 4, 4]
    assert stable[:, 2].tolist() == [-1, -1, -1, -1, -1, 3]
    assert rows.tolist() == [[0, 2, 3], [1, 4, 4], [2, 5, 3]] and dropped == 0 and (rc == at).all()
    # a feed that does not advance keeps its run; a restart clears stable without an event
    adv2 = adv.copy()
    adv2[1, 0] = False
    restarts = np.zeros((6, 3), dtype=int)
    restarts[4, 0] = 1
    stable, rows, _, _ = BR.decide(labels, confs, adv2, threshold=thr, hold=3, restarts=restarts)
    assert stable[:, 0].tolist() == [-1, -1, -1, 3, -1, -1]
    assert [r for r in rows.tolist() if r[0] == 0] == [[0, 3, 3]]
    # a stable label is logged once, not every tick; the same label after a dip is no new event
    lab1 = np.full((7, 1), 2)
    c1 = np.array([[.9], [.9], [.1], [.9], [.9], [.9], [.9]], dtype=np.float32)
    stable, rows, _, _ = BR.decide(lab1, c1, np.ones((7, 1), dtype=bool), threshold=0.5, hold=2)
    assert stable[:, 0].tolist() == [-1, 2, 2, 2, 2, 2, 2] and rows.tolist() == [[0, 1, 2]]
