"""Live and untrimmed inference: a stream of skeleton frames from a pose estimator, or one long recording, instead of clips a
feeder cut from a dataset split (the reference ships the pose extraction for this use, tools/gen_ucla_yolo_ske.py; graph.coco
and graph.openpose are its skeletons).

``FrameRing`` holds the last ``capacity`` frames in HBM and is pushed to without the host.  The model's input windows are built
straight from it by the val path of either feeder -- ``prep='nucla'``: feeder_nucla_gcn's centring, min-max normalisation and
resampling to ``time_steps`` frames on raw (V, 3) fp64 joints; ``prep='clip'``: clip_feeder's linear time-resize to
``window_size`` frames on (C, V, M) fp32 frames -- by the kernels those feeders run (csrc/streaming.hip shares their bodies), so
a window is bit-equal to what the feeder makes of a clip with the same frames.

``LiveClassifier`` is the frame-by-frame use: push -> plan -> window -> stream derivation -> forward -> softmax -> moving
average as one HIP graph that never synchronises:

    ring = FrameRing(128, prep='nucla', V=20)
    live = LiveClassifier(model.eval(), ring, window=40, beta=0.8)
    for frame in camera:                                   # (1, 20, 3) on the device
        label, conf, smoothed, logits = live.step(frame)   # device tensors, overwritten by the next step
        ...                                                # read them when a decision is due: that read is the only sync

``SlidingWindow`` is the offline use, one dense pass over a long sequence with per-frame votes:

    sw = SlidingWindow(model.eval(), window=40, hop=8, prep='nucla')
    res = sw.run(recording)                                # (len, 20, 3)
    res.frame_label                                        # (len,) int64 on the device

``RingBank`` and ``LiveBank`` are the frame-by-frame use for many feeds at once -- several cameras, or several tracked persons of
one camera -- S rings in one allocation and one graph replay per tick for all of them:

    bank = RingBank(feeds=32, capacity=128, prep='nucla', V=20)
    live = LiveBank(model.eval(), bank, window=40, beta=0.8, threshold=0.6, hold=3)
    for frames, counts, restart in ticks:                  # (32, 1, 20, 3); int32 [32] on the device or None
        out = live.step(frames, counts, restart)           # out.label, out.conf, out.smoothed, out.logits, out.stable: no sync
    live.events()                                          # the debounced label changes logged on the device: the only sync

The plan rule of ``SlidingWindow``: windows start at j * hop while j * hop + window <= len; one more window at len - window
when that leaves frames uncovered; a sequence shorter than the window is one window (0, len).  A frame's scores are the mean
of the softmax rows of the windows that cover it.  ``LiveClassifier``: per step `hop_windows` windows, window j ending
(hop_windows - 1 - j) * hop frames before the newest frame; a window that reaches before frame 0, or into frames the ring has
overwritten, is invalid: its input is zeros, it does not move the average, and until the first valid window the label is -1."""
import collections

import torch

from . import ops
from .evaluation import _state_key
from .inference import ENGINE_SLOTS, GraphedForward, default_parent

__all__ = ['FrameRing', 'RingBank', 'SlidingWindow', 'LiveClassifier', 'LiveBank', 'plan_offline']

PREPS = ('nucla', 'clip')
NUCLA_CENTER_JOINT = 1         # feeder_nucla_gcn centres on joint 1 of the first frame


def _int(name, v, lo, who):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError(f'{who}: {name} = {v!r} must be an integer >= {lo}')
    return v


def _device(device, who):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError(f'{who}: the frames live on the GPU; there is no CPU path')
    return dev


def _ring_frames(ring, n):
    """The push form of n frames for one ring of a FrameRing or a RingBank."""
    return (n, ring.V, 3) if ring.prep == 'nucla' else (ring.C, n, ring.V, ring.M)


def _feed_flags(who, name, t, S):
    """counts / restart of a bank call: None, or S integers in a tensor."""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dim() != 1 or t.numel() != S or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f'{who}: {name} must be None or an integer tensor [{S}], got {getattr(t, "dtype", type(t))} '
                         f'{tuple(getattr(t, "shape", ()))}')
    return t


class RingBank:
    """S = feeds independent rings in one allocation, one per camera or tracked person: frame f of feed s (counted from 0, the
    first frame the feed was ever pushed) lives in slot f % capacity, and feed(s) returns views (buf[s], state[s]) the
    single-ring ops accept.

    prep='nucla': buf fp64 (S, capacity, V, 3), push((S, n, V, 3)) in any float dtype (cast to fp64 on the device).
    prep='clip':  buf fp32 (S, C, capacity, V, M), push((S, C, n, V, M)) fp32.
    state int64 (S, 2) = (count, pushes) per feed lives on the device.  1 <= S <= 1024 (ops.BANK_MAX_FEEDS), 1 <= n <= capacity.

    push(frames, counts=None, restart=None), no host synchronisation, capturable: counts int32 [S] on the device (None: every
    feed takes all n frames): feed s takes the first min(max(counts[s], 0), n) frames of its slice; with 0 nothing of feed s
    moves, and what is not taken is never read (it may hold NaN).  restart int32 [S]: a non-zero entry forgets feed s before the
    push: its count goes to 0 and its frames are numbered from 0 again (the buffer is not cleared: no valid window reaches
    before frame 0).  reset(feeds=None) is the host-side call for all feeds or a list of them; it clears the buffers too."""

    def __init__(self, feeds, capacity, prep='nucla', V=None, C=3, M=1, device='cuda', _who='RingBank'):
        who = _who                                                    # FrameRing: the refusals carry the front's name
        self.feeds = _int('feeds', feeds, 1, who)
        if feeds > ops.BANK_MAX_FEEDS:
            raise ValueError(f'{who}: feeds = {feeds} above {ops.BANK_MAX_FEEDS}')
        self.capacity = _int('capacity', capacity, 1, who)
        if prep not in PREPS:
            raise ValueError(f'{who}: prep {prep!r} (one of {PREPS})')
        self.V, self.C, self.M = _int('V', V, 1, who), _int('C', C, 1, who), _int('M', M, 1, who)
        if prep == 'nucla' and (C != 3 or M != 1):
            raise ValueError(f"{who}: prep='nucla' holds one person's (V, 3) joints per feed; C = {C}, M = {M}")
        self.prep = prep
        dev = _device(device, who)
        self.buf = torch.zeros(self.frames_shape(capacity), dtype=torch.float64 if prep == 'nucla' else torch.float32, device=dev)
        self.state = torch.zeros(feeds, 2, dtype=torch.int64, device=dev)

    def frames_shape(self, n):
        return (self.feeds,) + _ring_frames(self, n)

    def push(self, frames, counts=None, restart=None):
        self._push('RingBank.push', (self.feeds,), frames, counts, restart)

    def _push(self, who, lead, frames, counts=None, restart=None):
        """frames in the form lead + one ring's: lead = (feeds,) for the bank's own push, () for a FrameRing's."""
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise RuntimeError(f'{who}: expected a HIP (cuda) tensor; there is no CPU path')
        t = len(lead) + (0 if self.prep == 'nucla' else 1)
        form = lambda n: lead + _ring_frames(self, n)                  # noqa: E731
        if frames.dim() != len(form(0)) or tuple(frames.shape) != form(frames.shape[t]) or not frames.is_floating_point():
            raise ValueError(f'{who}: frames must be {form("n")} floats, got {tuple(frames.shape)} {frames.dtype}')
        if not 1 <= frames.shape[t] <= self.capacity:
            raise ValueError(f'{who}: {frames.shape[t]} frames outside 1..capacity = {self.capacity}')
        if self.prep == 'clip' and frames.dtype != torch.float32:
            raise ValueError(f"{who}: prep='clip' takes fp32 frames, got {frames.dtype}")
        dev = self.buf.device
        counts, restart = (None if f is None else f.to(device=dev, dtype=torch.int32).contiguous()
                           for f in (_feed_flags(who, 'counts', counts, self.feeds), _feed_flags(who, 'restart', restart, self.feeds)))
        frames = frames.to(self.buf.dtype).contiguous()
        ops.bank_push(frames.view(self.frames_shape(frames.shape[t])), self.buf, self.state, counts, restart)

    def reset(self, feeds=None):
        if feeds is None:
            self.buf.zero_()
            self.state.zero_()
            return
        for s in self._feeds('RingBank.reset', feeds):
            self.buf[s].zero_()
            self.state[s].zero_()

    def _feeds(self, who, feeds):
        feeds = [feeds] if isinstance(feeds, int) else list(feeds)
        for s in feeds:
            if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.feeds:
                raise ValueError(f'{who}: feed {s!r} outside 0..{self.feeds - 1}')
        return feeds

    def feed(self, s):
        """(buf[s], state[s]): feed s as the ring and state tensors ops.ring_push, ring_plan, window_nucla and window_clip take."""
        s, = self._feeds('RingBank.feed', s)
        return self.buf[s], self.state[s]

    @property
    def counts(self):
        """The frames every feed has taken, as a list (a synchronisation)."""
        return self.state[:, 0].tolist()


class FrameRing:
    """capacity frames in HBM; frame f (counted from 0, the first frame ever pushed) lives in slot f % capacity.  A FrameRing is a
    RingBank of one feed: buf and state are feed 0's views, and every check and launch is the bank's.

    prep='nucla': buf fp64 (capacity, V, 3), push((n, V, 3)) in any float dtype (cast to fp64 on the device).
    prep='clip':  buf fp32 (C, capacity, V, M), push((C, n, V, M)) fp32.
    push() makes no host synchronisation and is capturable; 1 <= n <= capacity.  state int64 [2] = (frames, pushes) lives on
    the device; `count` reads it (a synchronisation).  reset() forgets every frame."""

    def __init__(self, capacity, prep='nucla', V=None, C=3, M=1, device='cuda'):
        bank = self._bank = RingBank(1, capacity, prep, V, C, M, device, _who='FrameRing')
        self.capacity, self.prep, self.V, self.C, self.M = bank.capacity, bank.prep, bank.V, bank.C, bank.M
        self.buf, self.state = bank.feed(0)

    def frames_shape(self, n):
        return _ring_frames(self, n)

    def push(self, frames):
        self._bank._push('FrameRing.push', (), frames)

    def reset(self):
        self._bank.reset()

    @property
    def count(self):
        return int(self.state[0])


def plan_offline(length, window, hop):
    """[(start, L)] of SlidingWindow's pass over `length` frames (the rule in the module docstring)."""
    if length < 1:
        return []
    if length < window:
        return [(0, length)]
    plan = [(s, window) for s in range(0, length - window + 1, hop)]
    if plan[-1][0] + window < length:
        plan.append((length - window, window))
    return plan


def _family_batch(model, frames_per_window, V, M):
    """Windows per call that keep `model` on its small-batch eval family (Model.forward's routing bounds)."""
    from . import f2, f2g, f2s, f2v
    G = len(model.models) if hasattr(model, 'models') else 1        # a StreamEnsemble's grouped pass counts G N M
    one = model.models[0] if hasattr(model, 'models') else model     # a StreamEnsemble's models are of one architecture
    if type(one).__module__.endswith('stgcn'):
        return max(1, f2s.F2S_MAX_FRAMES // (G * M * frames_per_window))
    if V == 20:
        return max(1, f2.F2_MAX_CLIPS // (G * M))
    bound = f2v.F2V_MAX_FRAMES if V == 25 else f2v.F2J_MAX_FRAMES if V in f2v.JOINTS else f2g.F2G_MAX_FRAMES
    return max(1, bound // (G * M * frames_per_window))


class _StateWatch:
    """evaluation._state_key(model) at the price a per-frame caller can pay.  The whole key walks the module tree (about a
    millisecond of host time for a ten-block model: twice the forward it guards); most of that is the walk, not the reading.  So
    the walk's result -- the tensors, the BatchNorm counters, the arenas -- is kept, and a call reads only what can move under
    an unchanged tree: every tensor's address and version, the counters, the arenas' state versions.  That sees what
    CapturedEval's key sees of an optimiser step, a CapturedStep replay, load_state_dict, an in-place edit, a train-mode
    forward or model.to().  Replacing a parameter or sub-module OBJECT changes the tree itself: the whole key is compared
    every `recheck` calls to catch that late, and invalidate() makes the next call catch it at once."""

    def __init__(self, model, recheck=256):
        self.model, self.recheck = model, recheck
        self.walk()

    def walk(self):
        from . import functional as Fn
        m = self.model
        self.full = _state_key(m)
        self.watch = list(m.parameters()) + list(m.buffers())
        self.epochs = [Fn._bn_epoch(b) for b in m.modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]
        arenas = {}
        for t in self.watch:
            a = getattr(t, '_tamgcn_arena', None)
            if a is not None:
                arenas[id(a)] = a
        self.arenas = list(arenas.values())
        self.fast = self.read()
        self.calls = 0

    def read(self):
        return (tuple((t.data_ptr(), t._version) for t in self.watch), tuple(e[0] for e in self.epochs),
                tuple(v for a in self.arenas for v in a.state_version()))

    def invalidate(self):
        self.calls = self.recheck

    def moved(self):
        """True once per change: the watch then stands on the current state."""
        self.calls += 1
        if self.calls >= self.recheck:
            before = self.full
            self.walk()
            return self.full != before
        fast = self.read()
        if fast == self.fast:
            return False
        self.walk()
        return True


class _Windows:
    """What SlidingWindow and the live chain share: the checked arguments and plan -> model input."""

    def __init__(self, who, model, prep, time_steps, window_size, stream, parent, V, C, M):
        if prep not in PREPS:
            raise ValueError(f'{who}: prep {prep!r} (one of {PREPS})')
        if stream not in ops.STREAM_MODES:
            raise ValueError(f'{who}: unknown stream {stream!r} (one of {sorted(ops.STREAM_MODES)})')
        if getattr(model, 'training', False):
            raise ValueError(f'{who}: put the model in eval() mode first')
        if getattr(model, 'arrangement', None) == 'streams':
            raise ValueError(f"{who}: a StreamEnsemble with arrangement='streams' forks HIP streams inside the captured graph; "
                             "the chain stays on one stream (arrangement None, 'grouped' or 'serial')")
        if hasattr(model, 'streams') and stream != 'joint':
            raise ValueError(f"{who}: a StreamEnsemble derives its own streams from the joint windows; stream = {stream!r}")
        if prep == 'nucla':
            if window_size is not None:
                raise ValueError(f"{who}: prep='nucla' resamples to time_steps frames; window_size belongs to prep='clip'")
            self.T = _int('time_steps', 52 if time_steps is None else time_steps, 1, who)
            if self.T > ops.STREAM_MAX_TS:
                raise ValueError(f'{who}: time_steps = {self.T} above {ops.STREAM_MAX_TS}')
        else:
            if time_steps is not None:
                raise ValueError(f"{who}: prep='clip' resizes to window_size frames; time_steps belongs to prep='nucla'")
            self.T = _int('window_size', window_size, 1, who)
        self.model, self.prep, self.stream = model, prep, stream
        self.V, self.C, self.M = V, C, M
        self._parent_arg, self.parent = parent, None

    def bind(self, dev):
        """The bone-parent table on the device (once)."""
        if self.parent is not None and self.parent.device == dev:
            return
        parent = self._parent_arg
        if parent is None:
            if self.prep == 'nucla' and self.V == 20:
                from .feeder.feeder_nucla_gcn import BONE_PARENT
                parent = BONE_PARENT
            else:
                first = self.model.models[0] if hasattr(self.model, 'models') else self.model
                parent = default_parent(first.graph)
        parent = [int(p) for p in (parent.tolist() if torch.is_tensor(parent) else parent)]
        if len(parent) != self.V or any(p < 0 or p >= self.V for p in parent):
            raise ValueError(f'parent must hold {self.V} joint indices in [0, {self.V})')
        self.parent = torch.tensor(parent, dtype=torch.int32, device=dev)

    def build(self, bank, plan, B):
        """bank tensor of S rings, plan int64 (rows >= S B, 2) -> the model's input (rows, C, T, V, M) of the configured stream."""
        if self.prep == 'nucla':
            return ops.bank_window_nucla(bank, plan, B, self.parent, self.T, NUCLA_CENTER_JOINT, self.stream)
        return ops.stream_derive(ops.bank_window_clip(bank, plan, B, self.T), self.parent, self.stream)

    def forward_one_stream(self, fn, x):
        """fn(x) with a StreamEnsemble that was left to choose kept on the grouped, one-stream arrangement (CapturedEval's rule)."""
        m = self.model
        if getattr(m, 'arrangement', 0) is not None:
            return fn(x)
        m.arrangement = 'grouped'
        try:
            return fn(x)
        finally:
            m.arrangement = None


SlidingResult = collections.namedtuple('SlidingResult', 'window_logits window_probs frame_scores frame_label plan')


class SlidingWindow:
    """model in eval() mode (a Model or a one-stream-arrangement StreamEnsemble); window, hop in frames; prep and its
    time_steps (default 52) or window_size; stream of ops.STREAM_MODES; parent: bone parents (default: the N-UCLA feeder's
    table for prep='nucla' at V = 20, else the model graph's); batch_windows: windows per forward call (default: what keeps the
    model on its small-batch eval family).

    run(seq) -> SlidingResult(window_logits (n, K), window_probs (n, K), frame_scores (len, K), frame_label (len,), plan (n, 2)),
    all on the device.  seq is the whole sequence, (len, V, 3) for 'nucla', (C, len, V, M) fp32 for 'clip', on the device or the
    host.  The plan is made on the host from len alone; the windows run in fixed-shape chunks of batch_windows, the last padded
    with invalid (all-zero) windows, through GraphedForward under torch.no_grad()."""

    def __init__(self, model, window, hop, prep='nucla', time_steps=None, window_size=None, stream='joint', parent=None,
                 batch_windows=None):
        who = 'SlidingWindow'
        self.window, self.hop = _int('window', window, 1, who), _int('hop', hop, 1, who)
        if batch_windows is not None:
            _int('batch_windows', batch_windows, 1, who)
        first = model.models[0] if hasattr(model, 'models') else model
        V = getattr(first, 'num_point', None)
        if not isinstance(V, int):
            raise ValueError(f'{who}: the model has no num_point (a models.ctrgcn.Model, models.stgcn.Model or StreamEnsemble is expected)')
        self._w = _Windows(who, model, prep, time_steps, window_size, stream, parent, V, None, None)
        self.batch_windows = batch_windows
        self._fwd = GraphedForward(model)
        self._watch = _StateWatch(model)

    def _seq(self, seq):
        w = self._w
        if not torch.is_tensor(seq):
            seq = torch.as_tensor(seq)
        if w.prep == 'nucla':
            ok = seq.dim() == 3 and seq.shape[1:] == (w.V, 3) and seq.is_floating_point()
        else:
            ok = seq.dim() == 4 and seq.shape[2] == w.V and seq.dtype == torch.float32
        if not ok or seq.numel() == 0:
            form = f'(len, {w.V}, 3) floats' if w.prep == 'nucla' else f'(C, len, {w.V}, M) fp32'
            raise ValueError(f'SlidingWindow.run: the sequence must be a non-empty {form} tensor, got {tuple(seq.shape)} {seq.dtype}')
        if not seq.is_cuda:
            seq = seq.to(next(self._w.model.parameters()).device)
            if not seq.is_cuda:
                raise RuntimeError('SlidingWindow.run: the model is not on the GPU; there is no CPU path')
        return seq.to(torch.float64 if w.prep == 'nucla' else torch.float32).contiguous()

    def run(self, seq):
        w = self._w
        seq = self._seq(seq)
        dev = seq.device
        w.bind(dev)
        length = seq.shape[0] if w.prep == 'nucla' else seq.shape[1]
        M = 1 if w.prep == 'nucla' else seq.shape[3]
        rows = plan_offline(length, self.window, self.hop)
        n = len(rows)
        bw = self.batch_windows or _family_batch(w.model, w.T, w.V, M)
        chunks = -(-n // bw)
        plan = torch.zeros(chunks * bw, 2, dtype=torch.int64)
        plan[:n] = torch.tensor(rows, dtype=torch.int64)
        plan = plan.to(dev)
        if w.model.training:
            raise RuntimeError('SlidingWindow.run: the model is in train() mode; call model.eval() first')
        if self._watch.moved():                                     # the forward graph holds the folded coefficients of one state
            self._fwd.reset()
        logits = None
        with torch.no_grad():
            for c in range(chunks):
                rows_c = plan[c * bw:(c + 1) * bw]
                out = w.forward_one_stream(self._fwd, w.build(seq[None], rows_c, bw))     # the sequence: one ring that never wraps
                if logits is None:
                    if out.dim() != 2 or out.shape[0] != bw:
                        raise ValueError(f'SlidingWindow: the model returned {tuple(out.shape)}, expected ({bw}, num_class)')
                    logits = torch.empty(chunks * bw, out.shape[1], dtype=torch.float32, device=dev)
                logits[c * bw:(c + 1) * bw].copy_(out)              # out is the graph's own tensor
        logits, plan = logits[:n], plan[:n]
        probs, scores, label = ops.window_vote(logits, plan, n_frames=length)
        return SlidingResult(logits, probs, scores, label, plan)


BankStep = collections.namedtuple('BankStep', 'label conf smoothed logits stable')
BankEvents = collections.namedtuple('BankEvents', 'rows conf dropped')


class LiveBank:
    """The live chain for S feeds at once: one graph replay pushes a tick's frames to every feed of a RingBank and classifies
    them all.  model in eval() mode; bank: the RingBank the frames go to (its prep decides the window form); window frames per
    window; per step and feed hop_windows windows `hop` frames apart (default hop = window), the newest last; beta in [0, 1): the
    moving average ema = beta ema + (1 - beta) probs over a feed's valid windows in the order they are seen (0: the newest
    window's softmax); time_steps / window_size, stream, parent as SlidingWindow's; frames_per_step (default 1): the n frames per
    feed every step takes; eager=True runs the chain launch by launch instead of replaying a graph (the same bits).

    step(frames, counts=None, restart=None) -> BankStep(label int64 [S], conf fp32 [S], smoothed fp32 (S, K), logits fp32
    (S, hop_windows, K), stable int64 [S] | None): frames in the bank's push form with n = frames_per_step; counts, restart:
    integer tensors [S] or None, copied like the frames into the chain's own device tensors (changing them never captures again).
    The chain is push -> plan -> window -> stream derivation -> forward -> softmax -> average -> decision; its outputs are device
    tensors, the graph's own, overwritten by the next step (clone to keep them).  Per feed the semantics are those of a feed
    that was stepped only on the ticks where counts[s] > 0, with that many frames, and reset() where restart[s] was set.  A feed
    with counts[s] == 0: no window of the tick is valid, its average and `seen` do not move, label, conf, smoothed and stable
    repeat its state, its logits rows are unspecified.  A feed with restart[s]: average, seen and debounce state are cleared on
    the device before the tick's push; label is -1 until its first valid window.  No synchronisation.

    CapturedEval's rules: step() raises while the model is in train() mode; the model's state key (evaluation._state_key, read
    per step through _StateWatch: see there for what a step sees at once) is compared per step and the chain is captured again
    when it moved (`captures` counts; such a step synchronises); a StreamEnsemble stays on one stream.  invalidate() makes the
    next step compare the whole key (after replacing a parameter object).

    The S hop_windows windows go through the model in chunks of chunk_windows (default: the fewest chunks that keep the model on
    its small-batch eval family, as in SlidingWindow, made equal in size; the last chunk padded with invalid windows), all inside
    the one graph.  Past the family's bound one pass of all windows (chunk_windows = S hop_windows) measured faster, with the
    general path's bits instead of the family's (profiles/stream_bank_bench.txt).

    threshold (None: no decisions, stable is None): the debounced decision per feed, updated after the average for every feed
    whose `seen` moved this tick, feeds ascending -- conf >= float32(threshold) and label == cand: run += 1; else conf >=
    float32(threshold): cand = label, run = 1; else cand = -1, run = 0; then, when run >= hold and cand != stable: stable = cand
    and one event (feed, frame = count - 1, label) with its conf is appended to a log of log_capacity rows on the device (a
    full log drops the event and counts it).  events() -> BankEvents(rows int64 (n, 3), conf fp32 [n], dropped) on the host: the
    only synchronisation.  clear_events() empties the log on the device.  reset() clears the bank, the averages, their counts,
    the debounce state and the log.  state_dict() / load_state_dict() carry the bank's buffers and states, the averages, the
    debounce state and the log."""

    def __init__(self, model, bank, window, hop_windows=1, hop=None, beta=0.0, time_steps=None, window_size=None, stream='joint',
                 parent=None, frames_per_step=1, eager=False, chunk_windows=None, threshold=None, hold=1, log_capacity=4096, _front=None):
        who = self._who = _front or 'LiveBank'                        # LiveClassifier: `bank` is its FrameRing, the refusals carry its name
        kind, noun = (FrameRing, 'ring') if _front else (RingBank, 'bank')
        if not isinstance(bank, kind):
            raise ValueError(f'{who}: {noun} must be a {kind.__name__}')
        self.window, self.B = _int('window', window, 1, who), _int('hop_windows', hop_windows, 1, who)
        self.hop = _int('hop', window if hop is None else hop, 1, who)
        self.n = _int('frames_per_step', frames_per_step, 1, who)
        if not (isinstance(beta, (int, float)) and not isinstance(beta, bool) and 0.0 <= beta < 1.0):
            raise ValueError(f'{who}: beta = {beta!r} outside [0, 1)')
        if threshold is not None and not (isinstance(threshold, (int, float)) and not isinstance(threshold, bool) and threshold == threshold):
            raise ValueError(f'{who}: threshold = {threshold!r} must be None or a number')
        self.hold = _int('hold', hold, 1, who)
        self.log_capacity = _int('log_capacity', log_capacity, 1, who)
        if chunk_windows is not None:
            _int('chunk_windows', chunk_windows, 1, who)
        need = self.window + (self.B - 1) * self.hop
        if bank.capacity < need:
            raise ValueError(f'{who}: a ring holds {bank.capacity} frames, window + (hop_windows - 1) hop = {need} are needed')
        if self.n > bank.capacity:
            raise ValueError(f'{who}: frames_per_step = {self.n} above the rings\' capacity {bank.capacity}')
        first = model.models[0] if hasattr(model, 'models') else model
        if getattr(first, 'num_point', None) != bank.V:
            raise ValueError(f'{who}: the model has {getattr(first, "num_point", None)} joints, the {noun} {bank.V}')
        self._w = _Windows(who, model, bank.prep, time_steps, window_size, stream, parent, bank.V, bank.C, bank.M)
        self._form = tuple(bank.frames_shape(self.n))                 # what step() takes: the caller's push form
        if _front:
            bank = bank._bank
        self.model, self.bank, self.beta, self.eager = model, bank, float(beta), bool(eager)
        self.threshold = None if threshold is None else float(threshold)
        S = self.S = bank.feeds
        if chunk_windows is None:                                     # as few family-sized passes as it takes, of equal size
            self.chunks = -(-S * self.B // _family_batch(model, self._w.T, bank.V, bank.M))
            self.chunk = -(-S * self.B // self.chunks)
        else:
            self.chunk = min(chunk_windows, S * self.B)
            self.chunks = -(-S * self.B // self.chunk)
        dev = self._dev = bank.buf.device
        self._w.bind(dev)
        self._frames = torch.zeros(bank.frames_shape(self.n), dtype=bank.buf.dtype, device=dev)
        # a LiveClassifier's step has no counts or restart: None, and the kernels load neither (four dependent loads less per step)
        self._counts = None if _front else torch.full((S,), self.n, dtype=torch.int32, device=dev)
        self._restart = None if _front else torch.zeros(S, dtype=torch.int32, device=dev)
        self._all, self._none = True, True                            # _counts holds n everywhere; _restart holds zeros
        with torch.no_grad():
            K = self._warm().shape[1]
        if K > ops.STREAM_MAX_K:
            raise ValueError(f'{who}: {K} classes above {ops.STREAM_MAX_K}')
        self.num_class = K
        self.ema = torch.zeros(S, K, dtype=torch.float64, device=dev)
        self.seen = torch.zeros(S, dtype=torch.int64, device=dev)
        self.deb = torch.tensor([-1, -1, 0], dtype=torch.int64, device=dev).repeat(S, 1)       # (stable, cand, run)
        self.log_rows = torch.zeros(self.log_capacity, 3, dtype=torch.int64, device=dev)
        self.log_conf = torch.zeros(self.log_capacity, dtype=torch.float32, device=dev)
        self.log_count = torch.zeros(2, dtype=torch.int64, device=dev)                          # (written, dropped)
        self._graph = self._out = self._keep = None
        self._watch = _StateWatch(model)
        self.captures = 0
        if not self.eager:
            self._capture()

    def _capture(self):
        """self._chain() as one HIP graph, after self._warm() ran on a side stream."""
        dev = self._dev
        told = hasattr(self.model, '_tamgcn_graphed')                 # GraphedForward's note to a StreamEnsemble
        if told:
            before, self.model._tamgcn_graphed = self.model._tamgcn_graphed, True
        try:
            with torch.no_grad():
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(2):
                        self._warm()
                torch.cuda.current_stream(dev).wait_stream(side)
                g = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(g):
                        out = self._chain()
                except Exception as e:                                # noqa: BLE001  -- no silent eager fall-back
                    raise RuntimeError(f'{self._who}: HIP graph capture failed ({type(e).__name__}: {e})') from e
        finally:
            if told:
                self.model._tamgcn_graphed = before
        # what the graph reads through pointers and the eval caches own (GraphedForward._capture_told has the reasons)
        keep = [dict(m.__dict__['_tamgcn_eval_cache']) for m in self.model.modules() if '_tamgcn_eval_cache' in m.__dict__]
        for slot in ENGINE_SLOTS:
            eng = self.model.__dict__.get(slot)
            if eng:
                keep.append(eng._blocks)
        hook = getattr(self.model, '_tamgcn_keep_alive', None)
        if hook is not None:
            keep.append(hook())
        self._graph, self._out, self._keep = g, out, keep
        self.captures += 1

    def _logits(self):
        """plan -> windows -> derive -> forward, chunk by chunk, on the bank as it stands: (plan (S B, 2), logits (S B, K))."""
        w, bank, S, B = self._w, self.bank, self.S, self.B
        rows = self.chunks * self.chunk
        plan = ops.bank_plan(bank.state, bank.capacity, B, self.window, self.hop, self._counts, rows=rows)
        x = w.build(bank.buf, plan, B)
        logits = None
        for c in range(self.chunks):
            out = w.forward_one_stream(self.model, x[c * self.chunk:(c + 1) * self.chunk])
            if out.dim() != 2 or out.shape[0] != self.chunk:
                raise ValueError(f'{self._who}: the model returned {tuple(out.shape)}, expected ({self.chunk}, num_class)')
            if self.chunks == 1:
                logits = out
                break
            if logits is None:
                logits = torch.empty(rows, out.shape[1], dtype=torch.float32, device=out.device)
            logits[c * self.chunk:(c + 1) * self.chunk].copy_(out)       # out may be the family's own buffer
        return plan[:S * B], logits[:S * B]

    def _warm(self):
        """The read-only part of the chain (nothing of the bank, the averages or the log moves)."""
        return self._logits()[1]

    def _chain(self):
        bank = self.bank
        ops.bank_push(self._frames, bank.buf, bank.state, self._counts, self._restart)
        plan, logits = self._logits()
        probs, _, _ = ops.window_vote(logits, plan)
        smoothed, label, conf, advanced = ops.bank_ema(probs, plan, self.beta, self.ema, self.seen, self._restart)
        stable = None
        if self.threshold is not None:
            ops.bank_decide(label, conf, advanced, bank.state, self.threshold, self.hold, self.deb, self.log_rows, self.log_conf, self.log_count,
                            self._restart)
            stable = self.deb[:, 0]
        return BankStep(label, conf, smoothed, logits.view(self.S, self.B, -1), stable)

    def _flags(self, name, given, own, default, is_default):
        """Copy counts / restart into the chain's tensor; None fills the default once.  -> whether `own` now holds the default."""
        given = _feed_flags(f'{self._who}.step', name, given, self.S)
        if given is None:
            if not is_default:
                own.fill_(default)
            return True
        own.copy_(given)
        return False

    def step(self, frames, counts=None, restart=None):
        who = self._who
        if self.model.training:
            raise RuntimeError(f'{who}: the model is in train() mode; call model.eval() before a step')
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise RuntimeError(f'{who}.step: expected a HIP (cuda) tensor; there is no CPU path')
        if tuple(frames.shape) != self._form or not frames.is_floating_point():
            raise ValueError(f'{who}.step: frames must be {self._form} floats, got {tuple(frames.shape)} {frames.dtype}')
        moved = self._watch.moved()
        self._frames.copy_(frames)                                    # a FrameRing's form lacks only the feed axis of one
        self._all = self._flags('counts', counts, self._counts, self.n, self._all)
        self._none = self._flags('restart', restart, self._restart, 0, self._none)
        with torch.no_grad():
            if self.eager:                                            # an eager chain folds a new state by itself
                return self._chain()
            if moved or self._graph is None:
                self._capture()
        self._graph.replay()
        return self._out

    def invalidate(self):
        self._watch.invalidate()

    def events(self):
        """BankEvents(rows int64 (n, 3) = (feed, frame, label), conf fp32 [n], dropped) on the host, in the order tick, then feed."""
        written, dropped = self.log_count.tolist()                    # the synchronisation
        return BankEvents(self.log_rows[:written].cpu(), self.log_conf[:written].cpu(), dropped)

    def clear_events(self):
        self.log_count.zero_()

    def reset(self):
        self.bank.reset()
        self.ema.zero_()
        self.seen.zero_()
        self.deb.copy_(torch.tensor([-1, -1, 0], dtype=torch.int64, device=self._dev).repeat(self.S, 1))
        self.clear_events()

    def _resumable(self):
        return dict(buf=self.bank.buf, state=self.bank.state, ema=self.ema, seen=self.seen, deb=self.deb, log_rows=self.log_rows,
                    log_conf=self.log_conf, log_count=self.log_count)

    def state_dict(self):
        """Copies of what a service needs to resume: the bank's buffers and states, the averages, the debounce state, the log."""
        return {k: v.detach().clone() for k, v in self._resumable().items()}

    def load_state_dict(self, sd):
        own = self._resumable()
        if set(sd) != set(own):
            raise ValueError(f'LiveBank.load_state_dict: keys {sorted(sd)} are not {sorted(own)}')
        for k, v in own.items():
            if not torch.is_tensor(sd[k]) or tuple(sd[k].shape) != tuple(v.shape) or sd[k].dtype != v.dtype:
                raise ValueError(f'LiveBank.load_state_dict: {k} must be {tuple(v.shape)} {v.dtype}')
        for k, v in own.items():
            v.copy_(sd[k])                                            # in place: the graph holds these addresses


class LiveClassifier:
    """The frame-by-frame use on one FrameRing: a thin front on LiveBank's chain at S = 1, all hop_windows windows in one pass
    through the model, no decisions.  model, ring (its prep decides the window form), window, hop_windows, hop, beta, time_steps /
    window_size, stream, parent, frames_per_step, eager as LiveBank's, and its rules: eval mode only, the state key compared per
    step with a re-capture when it moved (`captures` counts), a StreamEnsemble on one stream, eager=True the same bits.

    step(frames) takes the same n frames per call -- frames_per_step, default 1 -- in the ring's push form, copies them into
    the chain's input and runs push -> plan -> window -> derive -> forward -> softmax -> average.  -> (label int64 [1], conf
    fp32 [1], smoothed fp32 [K], logits fp32 (hop_windows, K)): device tensors, no synchronisation; they are the graph's own
    outputs, overwritten by the next step (clone to keep them).  label is -1 until the first valid window.

    ema fp64 [K] and seen int64 [1] are the average and the number of valid windows it has seen.  reset() clears the ring, the
    average and its count; invalidate() makes the next step compare the whole key (after replacing a parameter object)."""

    def __init__(self, model, ring, window, hop_windows=1, hop=None, beta=0.0, time_steps=None, window_size=None, stream='joint',
                 parent=None, frames_per_step=1, eager=False):
        live = self._live = LiveBank(model, ring, window, hop_windows, hop, beta, time_steps, window_size, stream, parent, frames_per_step,
                                     eager, chunk_windows=hop_windows, _front='LiveClassifier')
        self.model, self.ring, self.eager, self.num_class = model, ring, live.eager, live.num_class
        self.ema, self.seen = live.ema[0], live.seen

    @property
    def captures(self):
        return self._live.captures

    def step(self, frames):
        out = self._live.step(frames)
        return out.label, out.conf, out.smoothed[0], out.logits[0]

    def invalidate(self):
        self._live.invalidate()

    def reset(self):
        self._live.reset()
