"""numpy restatement of the bank of frame rings (tam_gcn_amd.streaming.RingBank / LiveBank, the tamgcn_bank_* entry points of
csrc/streaming.hip; include/tamgcn.h has the contract; not a test file): S copies of streaming_ref.Ring / plan_live / ema with
`counts` and `restart` applied per tick, and the debounced decision with its log.  tests/test_streambank_ref_cpu.py holds it to
hand-written cases, tests/test_gpu_streambank.py holds the kernels to it."""
import numpy as np

import streaming_ref as R


def take(counts, s, n):
    """What feed s takes of a tick's n frames: all without counts, else counts[s] clamped into 0..n."""
    return n if counts is None else min(max(int(counts[s]), 0), n)


class Bank:
    """S streaming_ref.Ring objects.  push(frames, counts, restart): frames[s] is feed s's list of n frames; a restarted feed
    becomes a fresh ring first; a feed takes the first take(counts, s, n) frames, and with 0 nothing of it moves."""

    def __init__(self, feeds, cap):
        self.cap, self.rings = cap, [R.Ring(cap) for _ in range(feeds)]

    def push(self, frames, counts=None, restart=None):
        for s in range(len(self.rings)):
            if restart is not None and restart[s]:
                self.rings[s] = R.Ring(self.cap)
            t = take(counts, s, len(frames[s]))
            if t:
                self.rings[s].push(list(frames[s][:t]))

    def state(self):
        return np.array([(r.count, r.pushes) for r in self.rings], dtype=np.int64)

    def plan(self, B, L, hop, counts=None):
        """int64 (S B, 2): plan_live per feed; (0, 0) rows for a feed that takes nothing this tick."""
        rows = []
        for s, r in enumerate(self.rings):
            idle = counts is not None and int(counts[s]) <= 0
            rows.append(np.zeros((B, 2), dtype=np.int64) if idle else R.plan_live(r.count, self.cap, B, L, hop))
        return np.concatenate(rows)


class Averages:
    """S moving averages, each streaming_ref.ema's recurrence fed window by window.  tick(probs (S, B, K), valid (S, B), restart)
    -> per feed (ema fp64 [K], seen, label, advanced) after the tick's B windows, oldest first."""

    def __init__(self, feeds, K, beta):
        self.beta, self.e, self.seen = beta, np.zeros((feeds, K)), [0] * feeds

    def tick(self, probs, valid, restart=None):
        out = []
        for s in range(len(self.seen)):
            if restart is not None and restart[s]:
                self.e[s], self.seen[s] = 0.0, 0
            before = self.seen[s]
            for p, v in zip(np.asarray(probs[s], dtype=np.float32).astype(np.float64), valid[s]):
                if v:
                    self.e[s] = p.copy() if self.seen[s] == 0 else self.beta * self.e[s] + (1.0 - self.beta) * p
                    self.seen[s] += 1
            out.append((self.e[s].copy(), self.seen[s], R.first_argmax(self.e[s]) if self.seen[s] else -1, self.seen[s] > before))
        return out


class Decider:
    """The debounce state (stable, cand, run) of S feeds and the log of `capacity` rows."""

    def __init__(self, feeds, threshold, hold, capacity):
        self.threshold, self.hold, self.capacity = np.float32(threshold), hold, capacity
        self.stable, self.cand, self.run = [-1] * feeds, [-1] * feeds, [0] * feeds
        self.rows, self.confs, self.dropped = [], [], 0

    def tick(self, labels, confs, advanced, counts, restart=None):
        """labels, confs (fp32), advanced per feed after the tick's average update; counts: every feed's frame count after the
        tick's push.  -> the feeds' stable labels after the tick."""
        for s in range(len(self.stable)):
            if restart is not None and restart[s]:
                self.stable[s], self.cand[s], self.run[s] = -1, -1, 0
            if not advanced[s]:
                continue
            lab, conf = int(labels[s]), np.float32(confs[s])
            if conf >= self.threshold and lab == self.cand[s]:
                self.run[s] += 1
            elif conf >= self.threshold:
                self.cand[s], self.run[s] = lab, 1
            else:
                self.cand[s], self.run[s] = -1, 0
            if self.run[s] >= self.hold and self.cand[s] != self.stable[s]:
                self.stable[s] = self.cand[s]
                if len(self.rows) < self.capacity:
                    self.rows.append((s, int(counts[s]) - 1, lab))
                    self.confs.append(conf)
                else:
                    self.dropped += 1
        return list(self.stable)

    def clear(self):
        self.rows, self.confs, self.dropped = [], [], 0


def decide(labels, confs, advanced, threshold, hold, counts=None, restarts=None, capacity=4096):
    """Over ticks: labels, confs, advanced (ticks, S); counts (ticks, S) the frame counts after each tick's push (default: the
    tick number + 1, one frame per tick); restarts (ticks, S) | None.  -> (stable int64 (ticks, S), rows int64 (n, 3) =
    (feed, frame, label) in the order tick then feed, confs fp32 [n], dropped)."""
    labels = np.asarray(labels)
    ticks, S = labels.shape
    d = Decider(S, threshold, hold, capacity)
    stable = np.zeros((ticks, S), dtype=np.int64)
    for t in range(ticks):
        c = counts[t] if counts is not None else [t + 1] * S
        stable[t] = d.tick(labels[t], confs[t], advanced[t], c, None if restarts is None else restarts[t])
    return stable, np.array(d.rows, dtype=np.int64).reshape(-1, 3), np.array(d.confs, dtype=np.float32), d.dropped
