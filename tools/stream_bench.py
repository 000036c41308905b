"""GPU-box tool: what live and sliding-window inference cost on the streaming path and on a host-driven one (one MI355X;
profiles/stream_infer_bench.txt).

    python tools/stream_bench.py time [rounds] [steps]
        (a) LiveClassifier.step, one frame per step, against a host-driven leg on the same tree -- a torch ring (torch.roll),
            the val normalisation in torch on the device, GraphedForward, softmax -- on N-UCLA (window 40, time_steps 52) and
            on COCO (17 joints, window 64 -> W = 64); ms per step over `steps` steps.
        (b) SlidingWindow.run on a 2000-frame sequence, hop 8, against a Python loop over windows through ops.feeder_transform /
            ops.clip_resize and GraphedForward; ms per pass (10 passes per timed window).
        Legs alternate inside one process, `rounds` rounds (default 7); medians with the spread (min .. max) of each leg.
        Every shape is warmed before it is timed; every timed window ends with a device synchronise.
    python tools/stream_bench.py trace [steps]
        `steps` live steps per dataset and one sliding pass each -- run it under rocprofv3 --kernel-trace --stats
    python tools/stream_bench.py report <kernel_trace.csv>
        the streaming kernels' times from that run, and the window kernels' bytes per second with the bytes computed from shapes
    python tools/stream_bench.py bank [rounds] [ticks]                        (profiles/stream_bank_bench.txt)
        S feeds at once, S = 1 4 8 16 32 64, one frame per feed and tick, on N-UCLA CTR-GCN (window 40 -> 52 steps), COCO CTR-GCN
        (window 64) and N-UCLA ST-GCN: (a) LiveBank.step, one graph replay for all feeds; (b) S LiveClassifier graph replays one
        after another (S one-feed chains: the baseline); (c) LiveBank with chunk_windows = S, one forward of
        all windows, where S is past the small-batch family's bound (elsewhere (c) is (a)).  ms per tick and feeds per 33 ms.
    python tools/stream_bench.py bank-trace [ticks]
        `ticks` LiveBank ticks per model at S = 32 with the decision log on -- run it under rocprofv3 --kernel-trace --stats
    python tools/stream_bench.py bank-report <kernel_trace.csv>
        the bank kernels' times from that run

One ring is a bank of one feed, so `trace` and `report` show the bank_* kernels at S = 1; profiles recorded before that carry the
former ring_*, window_* and score_ema kernel names.  The models carry seeded parameters (tests/golden/params.py); their accuracy is not the subject."""
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

DEV = 'cuda:0'
UCLA = dict(num_class=10, num_point=20, num_person=1, graph='tam_gcn_amd.graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
COCO = dict(num_class=10, num_point=17, num_person=1, graph='tam_gcn_amd.graph.coco.Graph', graph_args=dict(labeling_mode='spatial'))
# name -> (model arguments, prep, window, time_steps | window_size)
SETS = {'nucla': (UCLA, 'nucla', 40, 52), 'coco': (COCO, 'clip', 64, 64)}
SEQ_LEN, HOP = 2000, 8
PASSES = 10                    # sliding passes per timed window
BANK_FEEDS = (1, 4, 8, 16, 32, 64)
BANK_KERNELS = ('bank_push_kernel', 'bank_advance_kernel', 'bank_plan_kernel', 'bank_window_nucla_kernel', 'bank_window_clip_kernel',
                'window_softmax_kernel', 'bank_ema_kernel', 'bank_decide_kernel')
KERNELS = BANK_KERNELS[:-1] + ('window_vote_kernel',)      # one ring is a one-feed bank: the same kernels, and the per-frame vote


def _model(margs):
    import torch
    from params import fill_state_
    from tam_gcn_amd.models.ctrgcn import Model
    m = Model(**margs)
    fill_state_(m.state_dict(), seed=0)
    return m.to(DEV).eval()


def _bank_sets():
    """name -> (model, prep, V, window, LiveClassifier / LiveBank keywords)"""
    from params import fill_state_
    from tam_gcn_amd.models import stgcn
    st = stgcn.Model(**UCLA)
    fill_state_(st.state_dict(), seed=0)
    return {'nucla ctrgcn': (_model(UCLA), 'nucla', 20, 40, dict(time_steps=52)),
            'coco ctrgcn': (_model(COCO), 'clip', 17, 64, dict(window_size=64)),
            'nucla stgcn': (st.to(DEV).eval(), 'nucla', 20, 40, dict(time_steps=52))}


def _bank_frames(prep, V, S, n, seed=0):
    """n ticks of one frame per feed, in the bank's push form: [(S, 1, V, 3) fp64] or [(S, 3, 1, V, 1) fp32]"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    if prep == 'nucla':
        seq = rng.normal(size=(S, 1, V, 3)) + 0.05 * np.cumsum(rng.normal(size=(S, n, V, 3)), axis=1)
        return [torch.from_numpy(np.ascontiguousarray(seq[:, i:i + 1])).to(DEV) for i in range(n)]
    seq = rng.uniform(-1.0, 1.0, size=(S, 3, n, V, 1)).astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(seq[:, :, i:i + 1])).to(DEV) for i in range(n)]


def cmd_bank(rounds, ticks):
    import torch
    from tam_gcn_amd import streaming
    assert torch.cuda.is_available(), 'stream_bench: no GPU'
    print(f'# {torch.cuda.get_device_name(0)}; {rounds} rounds, legs alternated in one process; {ticks} ticks per timed window; '
          'one frame per feed and tick, beta 0.8, decision log on (threshold 0.6, hold 3)')
    for name, (model, prep, V, window, kw) in _bank_sets().items():
        kw = dict(kw, window=window, beta=0.8)
        bound = streaming._family_batch(model, kw.get('time_steps') or kw['window_size'], V, 1)
        alone = [streaming.LiveClassifier(model, streaming.FrameRing(128, prep=prep, V=V, device=DEV), **kw) for _ in range(max(BANK_FEEDS))]
        print(f'\n{name}: window {window}, the small-batch family takes {bound} windows per forward')
        print(f'{"S":>3s}  {"leg":<52s} {"ms / tick":>10s}  {"spread":>19s}  {"feeds / 33 ms":>13s}')
        for S in BANK_FEEDS:
            frames = _bank_frames(prep, V, S, window + ticks)
            mk = lambda **more: streaming.LiveBank(model, streaming.RingBank(S, 128, prep=prep, V=V, device=DEV), threshold=0.6, hold=3,     # noqa: E731
                                                   **kw, **more)
            bank = mk()
            legs = {f'(a) LiveBank.step, {bank.chunks} forward(s) of {bank.chunk}': lambda: [bank.step(f) for f in frames[window:]],
                    f'(b) {S} LiveClassifier replays': lambda: [[alone[s].step(f[s]) for s in range(S)] for f in frames[window:]]}
            one = mk(chunk_windows=S) if S > bound else None
            if one is not None:
                legs[f'(c) LiveBank, one forward of {S}'] = lambda: [one.step(f) for f in frames[window:]]
            with torch.no_grad():
                for a in alone[:S]:
                    a.reset()
                for f in frames[:window]:                                    # fill every ring, warm every shape
                    bank.step(f)
                    if one is not None:
                        one.step(f)
                    for s in range(S):
                        alone[s].step(f[s])
                res = {k: [] for k in legs}
                for _ in range(rounds):
                    for k, fn in legs.items():
                        res[k].append(_timed(fn) / ticks)
            for k, v in res.items():
                med = statistics.median(v)
                print(f'{S:>3d}  {k:<52s} {med:>10.3f}  {min(v):>8.3f} .. {max(v):>7.3f}  {S * 33.0 / med:>13.0f}')
            meds = [statistics.median(v) for v in res.values()]
            print(f'     (b) / (a) = {meds[1] / meds[0]:.2f}x' + (f'   (c) / (a) = {meds[2] / meds[0]:.2f}x' if one is not None else '')
                  + f'   captures {bank.captures}')
            del bank, one, legs


def cmd_bank_trace(ticks):
    import torch
    from tam_gcn_amd import streaming
    S = 32
    for name, (model, prep, V, window, kw) in _bank_sets().items():
        live = streaming.LiveBank(model, streaming.RingBank(S, 128, prep=prep, V=V, device=DEV), window=window, beta=0.8, threshold=0.6, hold=3, **kw)
        for f in _bank_frames(prep, V, S, window + ticks):
            live.step(f)
        torch.cuda.synchronize()


def cmd_bank_report(path):
    by = {}
    for r in csv.DictReader(open(path)):
        n = r['Kernel_Name']
        if any(k in n for k in BANK_KERNELS):
            short = n.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            grid = int(r.get('Grid_Size_X') or r.get('Grid_Size') or 0)
            by.setdefault((short, grid), []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('# kernel times of the bank path at S = 32 (rocprofv3 --kernel-trace, a run of its own), per kernel and grid (threads)')
    print(f'{"kernel":<56s} {"grid":>8s} {"calls":>6s} {"median us":>10s} {"min us":>8s} {"max us":>8s}')
    for (short, grid), t in sorted(by.items()):
        print(f'{short:<56s} {grid:>8d} {len(t):>6d} {statistics.median(t):>10.2f} {min(t):>8.2f} {max(t):>8.2f}')


def _sequence(prep, V, n, seed=0):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    if prep == 'nucla':
        return torch.from_numpy(rng.normal(size=(1, V, 3)) + 0.05 * np.cumsum(rng.normal(size=(n, V, 3)), axis=0)).to(DEV)
    return torch.from_numpy(rng.uniform(-1.0, 1.0, size=(3, n, V, 1)).astype(np.float32)).to(DEV)


def window_bytes(prep, L, T, V, C=3, M=1):
    """Bytes one window needs: read the L source frames once (the N-UCLA transform reads them twice: min / max, then the gather of
    T frames -- counted once, the second pass hits the cache), write the (C, T, V, M) fp32 window."""
    if prep == 'nucla':
        return L * V * 3 * 8 + 3 * T * V * 4
    return C * min(L, 2 * T) * V * M * 4 + C * T * V * M * 4


class HostLive:
    """The host-driven leg: what a user writes today.  A torch ring rolled by one frame per step, the feeder's val normalisation
    restated in torch on the device (no synchronisation either, but a dozen launches), GraphedForward, softmax."""

    def __init__(self, model, prep, window, T, V):
        import numpy as np
        import torch
        from tam_gcn_amd.inference import GraphedForward
        self.prep, self.T = prep, T
        self.fwd = GraphedForward(model)
        if prep == 'nucla':
            self.ring = torch.zeros(window, V, 3, dtype=torch.float64, device=DEV)
            self.idx = torch.from_numpy(np.linspace(0, window - 1, T).astype(int)).to(DEV)
        else:
            self.ring = torch.zeros(3, window, V, 1, dtype=torch.float32, device=DEV)

    def step(self, frame):
        import torch
        if self.prep == 'nucla':
            self.ring = torch.roll(self.ring, -1, 0)
            self.ring[-1:] = frame
            v = self.ring - self.ring[0, 1]
            flat = v.reshape(-1, 3)
            lo, hi = flat.min(0).values, flat.max(0).values
            v = (v - lo) / (hi - lo + 1e-6) * 2 - 1
            x = v[self.idx].permute(2, 0, 1).unsqueeze(0).unsqueeze(-1).float().contiguous()
        else:
            self.ring = torch.roll(self.ring, -1, 1)
            self.ring[:, -1:] = frame
            x = self.ring.unsqueeze(0)                                   # window == W: the resize is the identity
            if x.shape[2] != self.T:
                x = torch.nn.functional.interpolate(x.squeeze(-1), size=(self.T, x.shape[3]), mode='bilinear', align_corners=False).unsqueeze(-1)
        logits = self.fwd(x.contiguous())
        return torch.softmax(logits, 1)


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _host_sliding(model_fwd, prep, seq, rows, T, parent, bw):
    """A Python loop over the windows, bw per forward: gather the frames, ops.feeder_transform / ops.clip_resize, GraphedForward."""
    import numpy as np
    import torch
    from tam_gcn_amd import ops
    out = []
    for c in range(0, len(rows), bw):
        chunk = rows[c:c + bw]
        chunk = chunk + [chunk[-1]] * (bw - len(chunk))                     # fixed shape: pad with the last window
        if prep == 'nucla':
            raw = torch.cat([seq[s:s + L] for s, L in chunk])
            offs = torch.from_numpy(np.concatenate([[0], np.cumsum([L for _, L in chunk])]).astype(np.int64)).to(DEV)
            rot = torch.eye(3, dtype=torch.float64, device=DEV).repeat(bw, 1, 1)
            idx = torch.from_numpy(np.stack([np.linspace(0, L - 1, T).astype(int) for _, L in chunk]).astype(np.int32)).to(DEV)
            x = ops.feeder_transform(raw, offs, rot, idx, parent, seq.shape[1], T, 1, 'joint')
        else:
            crop = torch.tensor(chunk, dtype=torch.int32, device=DEV)
            x = ops.clip_resize(seq.unsqueeze(0), torch.zeros(bw, dtype=torch.int64, device=DEV), crop, T)
        out.append(model_fwd(x).clone())
    return torch.softmax(torch.cat(out)[:len(rows)], 1)


def _summary(name, times):
    med = statistics.median(times)
    return f'{name:<44s} median {med:9.3f} ms   spread {min(times):9.3f} .. {max(times):9.3f}  ({len(times)} rounds)', med


def cmd_time(rounds, steps):
    import torch
    from tam_gcn_amd import streaming
    from tam_gcn_amd.feeder.feeder_nucla_gcn import BONE_PARENT
    from tam_gcn_amd.inference import GraphedForward, default_parent
    assert torch.cuda.is_available(), 'stream_bench: no GPU'
    print(f'# {torch.cuda.get_device_name(0)}; {rounds} rounds, legs alternated in one process; live: {steps} steps per timed window')
    for name, (margs, prep, window, T) in SETS.items():
        model = _model(margs)
        V = margs['num_point']
        kw = dict(time_steps=T) if prep == 'nucla' else dict(window_size=T)
        seq = _sequence(prep, V, SEQ_LEN)
        frame = (lambda i: seq[i:i + 1]) if prep == 'nucla' else (lambda i: seq[:, i:i + 1])
        # (a) live
        ring = streaming.FrameRing(128, prep=prep, V=V, device=DEV)
        live = streaming.LiveClassifier(model, ring, window=window, beta=0.8, **kw)
        host = HostLive(model, prep, window, T, V)
        frames = [frame(i % SEQ_LEN) for i in range(window + steps)]
        with torch.no_grad():
            for i in range(window):                                         # fill both rings, warm every shape
                live.step(frames[i])
                host.step(frames[i])
            legs = {'LiveClassifier.step (one graph replay)': lambda: [live.step(f) for f in frames[window:]],
                    'host-driven (torch ring + norm, GraphedForward)': lambda: [host.step(f) for f in frames[window:]]}
            res = {k: [] for k in legs}
            for _ in range(rounds):
                for k, fn in legs.items():
                    res[k].append(_timed(fn) / steps)
        print(f'\n(a) live, {name}: window {window}, one frame per step, ms per step')
        meds = [print(s) or m for s, m in (_summary(k, v) for k, v in res.items())]
        print(f'    host-driven / LiveClassifier = {meds[1] / meds[0]:.2f}x')
        # (b) sliding
        sw = streaming.SlidingWindow(model, window=window, hop=HOP, prep=prep, **kw)
        rows = streaming.plan_offline(SEQ_LEN, window, HOP)
        bw = streaming._family_batch(model, T, V, 1)
        parent = torch.tensor(BONE_PARENT if prep == 'nucla' else default_parent(model.graph), dtype=torch.int32, device=DEV)
        fwd = GraphedForward(model)
        with torch.no_grad():
            a = sw.run(seq).window_probs.clone()
            b = _host_sliding(fwd, prep, seq, rows, T, parent, bw)
            print(f'\n(b) sliding, {name}: {SEQ_LEN} frames, window {window}, hop {HOP}: {len(rows)} windows, {bw} per forward; '
                  f'max |probs - host loop| = {float((a - b).abs().max()):.3g}')
            legs = {'SlidingWindow.run': lambda: sw.run(seq), 'python loop (ops.* + GraphedForward)': lambda: _host_sliding(fwd, prep, seq, rows, T, parent, bw)}
            res = {k: [] for k in legs}
            for _ in range(rounds):
                for k, fn in legs.items():
                    res[k].append(_timed(lambda: [fn() for _ in range(PASSES)]) / PASSES)
        meds = [print(s) or m for s, m in (_summary(k, v) for k, v in res.items())]
        print(f'    python loop / SlidingWindow.run = {meds[1] / meds[0]:.2f}x   (ms per pass)')


def cmd_trace(steps):
    import torch
    from tam_gcn_amd import streaming
    for name, (margs, prep, window, T) in SETS.items():
        model = _model(margs)
        V = margs['num_point']
        kw = dict(time_steps=T) if prep == 'nucla' else dict(window_size=T)
        seq = _sequence(prep, V, SEQ_LEN)
        live = streaming.LiveClassifier(model, streaming.FrameRing(128, prep=prep, V=V, device=DEV), window=window, beta=0.8, **kw)
        for i in range(window + steps):
            live.step(seq[i:i + 1] if prep == 'nucla' else seq[:, i:i + 1])
        streaming.SlidingWindow(model, window=window, hop=HOP, prep=prep, **kw).run(seq)
        torch.cuda.synchronize()


def cmd_report(path):
    from tam_gcn_amd import streaming
    by = {}
    for r in csv.DictReader(open(path)):
        n = r['Kernel_Name']
        if any(k in n for k in KERNELS):
            short = n.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            grid = int(r.get('Grid_Size_X') or r.get('Grid_Size') or 0)
            by.setdefault((short, grid), []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('# kernel times of the streaming path (rocprofv3 --kernel-trace, a run of its own), per kernel and grid (threads)')
    print(f'{"kernel":<40s} {"grid":>8s} {"calls":>6s} {"median us":>10s} {"min us":>8s} {"max us":>8s}')
    for (short, grid), t in sorted(by.items()):
        print(f'{short:<40s} {grid:>8d} {len(t):>6d} {statistics.median(t):>10.2f} {min(t):>8.2f} {max(t):>8.2f}')
    print('\n# bytes per second of the window kernels: bytes computed from shapes (window_bytes in this file) over the median kernel time')
    for name, (margs, prep, window, T) in SETS.items():
        V = margs['num_point']
        bw = streaming._family_batch(_Shape(margs), T, V, 1)
        vec = 4 if V % 4 == 0 else 1
        per_window = 256 if prep == 'nucla' else 256 * 3 * -(-T * V // (256 * vec))      # threads of the grid per window
        for what, nwin in (('one live window', 1), (f'a sliding chunk of {bw} windows', bw)):
            key = next((k for k in by if ('window_nucla' if prep == 'nucla' else 'window_clip') in k[0] and k[1] == nwin * per_window), None)
            if key is None:
                print(f'{name:<6s} {what:<32s} not in the trace')
                continue
            b, us = nwin * window_bytes(prep, window, T, V), statistics.median(by[key])
            print(f'{name:<6s} {what:<32s} {b:>9d} bytes / launch, median {us:7.2f} us: {b / us / 1e3:8.2f} GB/s')


class _Shape:
    """Stands in for a model where only its family is asked for."""
    def __init__(self, margs):
        self.num_point = margs['num_point']


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if what == 'time':
        cmd_time(int(sys.argv[2]) if len(sys.argv) > 2 else 7, int(sys.argv[3]) if len(sys.argv) > 3 else 1000)
    elif what == 'trace':
        cmd_trace(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    elif what == 'report':
        cmd_report(sys.argv[2])
    elif what == 'bank':
        cmd_bank(int(sys.argv[2]) if len(sys.argv) > 2 else 7, int(sys.argv[3]) if len(sys.argv) > 3 else 100)
    elif what == 'bank-trace':
        cmd_bank_trace(int(sys.argv[2]) if len(sys.argv) > 2 else 100)
    elif what == 'bank-report':
        cmd_bank_report(sys.argv[2])
    else:
        sys.exit(__doc__)
