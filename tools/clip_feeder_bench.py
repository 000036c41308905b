"""GPU-box tool: what a batch of the clip feeder costs on each path (profiles/clip_feeder_bench.txt).

    python tools/clip_feeder_bench.py time [batches]
        per configuration -- 256 x (3, 64, 20, 1); 128 x (3, 300, 25, 2) with W = 300 and W = 64; all random flags on and
        all off -- ms per batch of (a) the numpy restatement tests/clip_feeder_ref.py on the host plus the copy to the
        device, (b) Feeder.batch_device() launched eagerly, (c) a GraphedBatch replay; legs alternated, three repeats.
        Then the transform alone: `batches` launches held in one HIP graph between two device events, and the bytes the
        gather needs (read: the copied spans; written: the whole batch) over that time.
    python tools/clip_feeder_bench.py trace [batches]
        `batches` eager batch_device calls per configuration -- run it under rocprofv3 --kernel-trace
    python tools/clip_feeder_bench.py report <kernel_trace.csv> [batches]
        kernel time per batch of the clip feeder's kernels from that trace

Every timed window starts and ends with a device synchronise; every leg is warmed up before it is timed.  The splits are
seeded: 2048 clips of the larger shape are 368 MB, above the 256 MiB Infinity Cache.
"""
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DEV = 'cuda:0'
# (batch, clips in the split, (C, T, V, M), window_size)
SHAPES = [(256, 4096, (3, 64, 20, 1), -1), (128, 2048, (3, 300, 25, 2), -1), (128, 2048, (3, 300, 25, 2), 64)]
CONFIGS = [(s, flags) for s in SHAPES for flags in (7, 0)]
HOST_BATCHES = 3


def _data(n, shape, seed=0):
    """Seeded clips with a zero tail of 0 .. T/2 frames, as padded NTU clips have."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(n,) + shape).astype(np.float32)
    for i, tail in enumerate(rng.integers(0, shape[1] // 2 + 1, size=n)):
        if tail:
            x[i][:, shape[1] - tail:] = 0
    return x


def _feeder(data, ws, flags):
    import numpy as np
    from tam_gcn_amd.feeder.clip_feeder import Feeder
    return Feeder(None, None, data=data, labels=np.arange(len(data)) % 60, random_shift=bool(flags & 1), random_choose=bool(flags & 2),
                  random_move=bool(flags & 4), window_size=ws, device=DEV, seed=1)


def _name(batch, shape, ws, flags):
    return f'{batch} x {shape}, W = {ws if ws > 0 else shape[1]}, flags {"on" if flags else "off"}'


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def _gather_bytes(plan, C, T, W, VM):
    """Bytes one transform launch has to move: the copied spans read, the whole batch written."""
    import numpy as np
    src0, lo, hi = (plan[:, k].astype(np.int64) for k in range(3))
    lo, hi = np.maximum(np.maximum(lo, 0), -src0), np.minimum(np.minimum(hi, W), T - src0)
    frames = int(np.maximum(hi - lo, 0).sum())
    return 4 * C * VM * (frames + len(plan) * W)


def _host_batch(R, data, ext, ids, call, W, flags, node, cand):
    """The restatement's batch, on the host, and its copy to the device."""
    import numpy as np
    import torch
    T = data.shape[2]
    pl, _, move = R.device_draws(1, call, ext[ids], T, W, flags, len(node), tuple(len(c) for c in cand))
    out = np.empty((len(ids), data.shape[1], W) + data.shape[3:], dtype=np.float32)
    for b, i in enumerate(ids):
        keys = None
        if flags & 4:
            keys = np.stack([c[move[b][:, q]] for q, c in enumerate((cand[0], cand[1], cand[2], cand[2]))], axis=1)
        out[b] = R.apply(data[i], pl[b], W, node if flags & 4 else None, keys)[0]
    return torch.from_numpy(out).to(DEV)


def time_batches(batches=200):
    import numpy as np
    import torch
    import clip_feeder_ref as R
    from tam_gcn_amd import ops
    from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch
    torch.manual_seed(0)
    cand = R.default_candidates()
    print(f'{batches} batches per device leg, {HOST_BATCHES} per host leg, 3 repeats, legs alternated')
    cache = {}
    for (batch, n, shape, ws), flags in CONFIGS:
        if (n, shape) not in cache:
            cache.clear()
            cache[(n, shape)] = _data(n, shape)
        data = cache[(n, shape)]
        fd = _feeder(data, ws, flags)
        gb = GraphedBatch(fd, batch)
        ext, node = fd._extent_cpu.astype(np.int64), R.node_table(fd.W, 1)
        perm = torch.randperm(n, device=DEV)
        perm_host = perm.cpu().numpy()
        n_pos = n - batch + 1
        legs = {'numpy restatement + copy': lambda i: _host_batch(R, data, ext, perm_host[(i * batch) % n_pos:][:batch], i, fd.W, flags, node, cand),
                'batch_device eager': lambda i: fd.batch_device(perm[(i * batch) % n_pos:][:batch]),
                'GraphedBatch replay': lambda i: gb(perm[(i * batch) % n_pos:][:batch])}
        print(_name(batch, shape, ws, flags))
        ms = {name: [] for name in legs}
        for rep in range(3):
            for name, fn in legs.items():
                k = HOST_BATCHES if name.startswith('numpy') else batches
                _timed(fn, 1 if name.startswith('numpy') else 5)
                ms[name].append(1e3 * _timed(fn, k))
                print(f'  repeat {rep}: {name:26s} {ms[name][-1]:10.4f} ms/batch')
        for name in list(legs)[1:]:
            print(f'  {name}: slowest repeat {max(ms[name]):.4f} ms against the host leg\'s fastest {min(ms["numpy restatement + copy"]):.3f} ms')
        # the transform alone, on the draws of one batch
        ids = perm[:batch].contiguous()
        plan, _, _, keys, _ = ops.clip_draw(fd._extent, ids, fd._rng.clone(), flags, fd.T, fd.W, len(fd.node), fd._cand if flags & 4 else None)
        nd = fd._node if flags & 4 else None
        for _ in range(3):
            ops.clip_transform(fd._raw, ids, plan, fd.W, nd, keys)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(batches):
                ops.clip_transform(fd._raw, ids, plan, fd.W, nd, keys)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / batches
        nbytes = _gather_bytes(plan.cpu().numpy(), shape[0], fd.T, fd.W, shape[2] * shape[3])
        print(f'  transform alone, {batches} launches in one graph: {us:.2f} us per launch, {nbytes / 1e6:.2f} MB needed -> {nbytes / us / 1e6:.3f} TB/s '
              f'(launch gaps included; the kernel trace has the kernel\'s own time)')


def trace(batches=50):
    import torch
    cache = {}
    for (batch, n, shape, ws), flags in CONFIGS:
        if (n, shape) not in cache:
            cache.clear()
            cache[(n, shape)] = _data(n, shape)
        fd = _feeder(cache[(n, shape)], ws, flags)
        perm = torch.randperm(n, device=DEV)
        n_pos = n - batch + 1
        nbytes = 0
        torch.cuda.synchronize()
        for i in range(batches):
            fd.batch_device(perm[(i * batch) % n_pos:][:batch])
            if i == 0:
                nbytes = _gather_bytes(fd.last_draws['plan'].cpu().numpy(), shape[0], fd.T, fd.W, shape[2] * shape[3])
        torch.cuda.synchronize()
        print(f'trace: {batches} x {_name(batch, shape, ws, flags)}: first batch needs {nbytes} bytes')


def report(path, batches=50):
    rows = [r for r in csv.DictReader(open(path)) if 'clip_' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    by = {}
    for r in rows:
        short = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        by.setdefault('transform' if 'clip_transform' in short else short, []).append((short, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3))
    for kind, ds in by.items():
        if kind == 'transform' or len(ds) == batches * len(CONFIGS):
            for leg, ((batch, n, shape, ws), flags) in enumerate(CONFIGS):          # the trace runs the configurations in this order
                d = ds[leg * batches:(leg + 1) * batches]
                if d:
                    t = [v for _, v in d]
                    print(f'  {_name(batch, shape, ws, flags):52s} {len(t):4d} x {sum(t) / len(t):8.2f} us (min {min(t):.2f}, max {max(t):.2f})  {d[0][0]}')
        else:
            t = [v for _, v in ds]
            print(f'  all configurations: {len(t):5d} x {sum(t) / len(t):8.2f} us (min {min(t):.2f}, max {max(t):.2f})  {kind}')


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        time_batches(*(int(a) for a in sys.argv[2:3]))
    elif mode == 'trace':
        trace(*(int(a) for a in sys.argv[2:3]))
    elif mode == 'report':
        report(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        raise SystemExit(__doc__)
