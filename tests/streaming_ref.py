"""numpy restatement of the streaming path (csrc/streaming.hip, tam_gcn_amd/streaming.py; include/tamgcn.h has the contract; not
a test file): the plans, the ring as a python list indexed modulo its capacity, the two window builders through the feeders' own
references, and the score post-processing in fp64 with its rounding bounds.  tests/test_streaming_ref_cpu.py holds it to plain
slicing and brute force, tests/test_gpu_streaming.py holds the kernels to it.

Bounds.  A probability or a frame score is one fp32 rounding (2^-24 relative) of an fp64 chain on magnitudes <= 1: K
exponentials and additions for the softmax denominator, n_cover additions for the mean, the shifts, divisions and the
exponential's own ulp in the 8 --

    |got - ref| <= 2^-24 |ref| + (K + n_cover + 8) 2^-52

-- and the moving average after `steps` valid updates the same with 3 steps in place of n_cover (two products and one sum per
update; the device may contract the update to an FMA, which is inside that)."""
import numpy as np

from oracle import feeder_oracle
import clip_resize_ref

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -52
STREAMS = ('joint', 'bone', 'motion', 'bone_motion')


def plan_live(count, cap, B, L, hop):
    """int64 (B, 2): window j ends (B - 1 - j) hop frames before frame `count`; (0, 0) before frame 0 or overwritten."""
    plan = np.zeros((B, 2), dtype=np.int64)
    for j in range(B):
        start = count - (B - 1 - j) * hop - L
        if start >= 0 and start >= count - cap:
            plan[j] = (start, L)
    return plan


def plan_offline(length, window, hop):
    """SlidingWindow's plan: starts j hop while the window fits, one last window at length - window when frames are left
    uncovered, one window (0, length) for a sequence shorter than the window."""
    if length < window:
        return np.array([(0, length)], dtype=np.int64)
    rows, j = [], 0
    while j * hop + window <= length:
        rows.append((j * hop, window))
        j += 1
    if rows[-1][0] + window < length:
        rows.append((length - window, window))
    return np.array(rows, dtype=np.int64)


class Ring:
    """cap slots; frame f of everything pushed so far lives in slot f % cap.  Frames are whatever the caller pushes."""

    def __init__(self, cap):
        self.cap, self.slots, self.count, self.pushes = cap, [None] * cap, 0, 0

    def push(self, frames):
        assert 1 <= len(frames) <= self.cap
        for f in frames:
            self.slots[self.count % self.cap] = f
            self.count += 1
        self.pushes += 1

    def window(self, start, L):
        """The frames start .. start + L - 1; they must still be in the ring."""
        assert 0 <= start and start + L <= self.count and start >= self.count - self.cap and L >= 1
        return [self.slots[(start + i) % self.cap] for i in range(L)]


def window_nucla(frames, stream='joint', time_steps=52):
    """frames (L, 20, 3) fp64 -> (3, time_steps, 20, 1) fp32: the feeder's val path (identity view, linspace indices)."""
    frames = np.asarray(frames, dtype=np.float64)
    return feeder_oracle.transform(frames, 0, 0, 1.0, feeder_oracle.val_indices(len(frames), time_steps), stream, time_steps)


def window_clip(seq, start, L, W):
    """seq (C, T, V, M) -> (out fp64 (C, W, V, M), bound): clip_resize_ref.resize of the crop without rotation."""
    return clip_resize_ref.resize(seq, start, L, W)


def softmax(logits):
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def score_bound(ref, K, n):
    return EPS32 * np.abs(ref) + (K + n + 8) * EPS64


def first_argmax(row):
    """The first index of the largest value (np.argmax's rule, restated)."""
    best = 0
    for k in range(1, len(row)):
        if row[k] > row[best]:
            best = k
    return best


def vote(logits, plan, n_frames):
    """-> probs fp64 (B, K), frame_scores fp64 (n_frames, K), frame_label int64 (n_frames,), cover int64 (n_frames,).
    The mean is taken over the fp32-rounded probabilities, as the device takes it over what it stored."""
    probs = softmax(logits)
    p32 = probs.astype(np.float32).astype(np.float64)
    plan = np.asarray(plan, dtype=np.int64)
    B, K = probs.shape
    f = np.arange(n_frames)[:, None]
    covers = (plan[None, :, 1] >= 1) & (plan[None, :, 0] <= f) & (f < plan[None, :, 0] + plan[None, :, 1])     # (n_frames, B)
    cover = covers.sum(axis=1)
    scores = np.zeros((n_frames, K))
    label = np.full(n_frames, -1, dtype=np.int64)
    for i in range(n_frames):
        if cover[i]:
            acc = np.zeros(K)
            for j in np.nonzero(covers[i])[0]:
                acc += p32[j]
            scores[i] = acc / cover[i]
            label[i] = first_argmax(scores[i])
    return probs, scores, label, cover


def top2_gap(scores):
    s = np.sort(scores, axis=-1)
    return s[..., -1] - s[..., -2]


def ema(prob_rows, valid, beta):
    """The moving average over steps: prob_rows (S, K) (fp32 values), valid bool [S] -> per step (ema fp64 [K], seen, label)."""
    e, seen, out = np.zeros(np.asarray(prob_rows).shape[1]), 0, []
    for p, v in zip(np.asarray(prob_rows, dtype=np.float32).astype(np.float64), valid):
        if v:
            e = p.copy() if seen == 0 else beta * e + (1.0 - beta) * p
            seen += 1
        out.append((e.copy(), seen, first_argmax(e) if seen else -1))
    return out


def ema_bound(ref, K, steps):
    return score_bound(ref, K, 3 * steps)


def vote_logits(B, K, seed):
    """The seeded U(-3, 3) logits of the vote cases, fp32 (B, K)."""
    return np.random.default_rng(seed).uniform(-3.0, 3.0, size=(B, K)).astype(np.float32)


# the two vote cases of tests/test_gpu_streaming.py: (B, K, L, hop, frames, invalid window, seed).  The seeds are chosen so that
# no frame's two largest fp64 scores lie within twice the bound (tests/test_streaming_ref_cpu.py asserts it).
VOTE_CASES = {'b6_k10': (6, 10, 9, 4, 27, 2, 5), 'b40_k60': (40, 60, 9, 4, 170, None, 6)}


def vote_case(name):
    B, K, L, hop, frames, invalid, seed = VOTE_CASES[name]
    plan = np.array([(2 + j * hop, L) for j in range(B)], dtype=np.int64)      # frames 0, 1 and the tail: uncovered
    if invalid is not None:
        plan[invalid] = (0, 0)
    return vote_logits(B, K, seed), plan, frames
