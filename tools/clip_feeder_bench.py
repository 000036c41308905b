"""GPU-box tool: what a batch of the clip feeder costs on each path (profiles/clip_feeder_bench.txt).

    python tools/clip_feeder_bench.py time [batches]
        per configuration -- 256 x (3, 64, 20, 1); 128 x (3, 300, 25, 2) with W = 300 and W = 64; all random flags on and
        all off -- ms per batch of (a) the numpy restatement tests/clip_feeder_ref.py on the host plus the copy to the
        device, (b) Feeder.batch_device() launched eagerly, (c) a GraphedBatch replay; legs alternated, three repeats.
        Then the transform alone: `batches` launches held in one HIP graph between two device events, and the bytes the
        gather needs (read: the copied spans; written: the whole batch) over that time.
    python tools/clip_feeder_bench.py resize [batches] [steps]
        the crop-and-resize mode (profiles/clip_resize_bench.txt): 128 x (3, 300, 25, 2) at W = 64, p_interval = [0.5, 1], with
        and without the rotation -- ms per batch of (a) the published pipeline's own host operations (per sample the crop, torch's
        F.interpolate and the matrix product, with the draws of tests/clip_resize_ref.py) plus the copy, (b) batch_device() eagerly, (c) a GraphedBatch replay; then the resize kernel alone in one HIP graph and the bytes
        it needs (read: the source frames its taps name; written: the whole batch), beside clip_transform's centre crop of the
        same split to the same window measured the same way; then one CapturedStep of the NTU model fed by a GraphedBatch at
        W = 64 (this mode) and at W = 300 (the padded clips), `steps` steps per leg, legs alternated.
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


def _alone(launch, batches):
    """us per launch of `launch()`, `batches` of them held in one HIP graph between two device events."""
    import torch
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(batches):
            launch()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / batches


def _resize_bytes(R, crop, C, W, VM):
    """Bytes one resize launch has to move: the distinct source frames its taps name read once, the whole batch written."""
    import numpy as np
    frames = 0
    for _, L in crop:
        i0, i1, _ = R.taps(int(L), W)
        frames += len(np.union1d(i0, i1))
    return 4 * C * VM * (frames + len(crop) * W)


def _host_resize_batch(R, data, ext, ids, call, W, flags, p, min_crop, theta):
    """The published pipeline's own operations on the host -- per sample the crop, F.interpolate(bilinear) over time, the fp32
    matrix product -- with the restatement's draws, and the batch's copy to the device."""
    import numpy as np
    import torch
    crop, drawn = R.crop_draws(1, call, ext[ids], flags, p[0], p[-1], min_crop, theta)
    C, _, V, M = data.shape[1:]
    out = torch.empty((len(ids), C, W, V, M), dtype=torch.float32)
    for b, i in enumerate(ids):
        x = torch.from_numpy(data[i][:, crop[b, 0]:crop[b, 0] + crop[b, 1]])
        x = x.permute(0, 2, 3, 1).contiguous().view(C * V * M, -1)[None, None]
        y = torch.nn.functional.interpolate(x, size=(C * V * M, W), mode='bilinear', align_corners=False).squeeze()
        y = y.contiguous().view(C, V, M, W).permute(0, 3, 1, 2).contiguous()
        if flags & R.ROT:
            rot = torch.from_numpy(R.rot_matrix(drawn[b, 1:]).astype(np.float32))
            y = torch.matmul(rot, y.view(C, -1)).view(C, W, V, M)
        out[b] = y
    return out.to(DEV)


def _ntu_step(batch, W):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    m = Model(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    opt = FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    x, y = make_input((batch, 3, W, 25, 2), 4).to(DEV), make_labels(batch, 60, 5).to(DEV)
    return CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y)


def time_resize(batches=200, steps=10):
    import numpy as np
    import torch
    import clip_resize_ref as R
    from tam_gcn_amd import ops
    from tam_gcn_amd.feeder.clip_feeder import Feeder
    from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch
    torch.manual_seed(0)
    batch, n, shape, W, p, min_crop, theta = 128, 2048, (3, 300, 25, 2), 64, (0.5, 1.0), 64, 0.3
    data = _data(n, shape)
    labels = np.arange(n) % 60
    perm = torch.randperm(n, device=DEV)
    perm_host = perm.cpu().numpy()
    n_pos = n - batch + 1
    print(f'{batch} x {shape} of a split of {n} clips, W = {W}, p_interval = {list(p)}, min_crop = {min_crop}; {batches} batches per device leg, '
          f'{HOST_BATCHES} per host leg, 3 repeats, legs alternated')
    feeders = {}
    for rot in (True, False):
        fd = Feeder(None, None, data=data, labels=labels, window_size=W, p_interval=list(p), min_crop=min_crop, random_rot=rot,
                    rot_theta=theta, device=DEV, seed=1)
        feeders[rot] = fd
        gb = GraphedBatch(fd, batch)
        ext, flags = fd._extent_cpu.astype(np.int64), fd.crop_flags
        legs = {'host torch pipeline + copy': lambda i: _host_resize_batch(R, data, ext, perm_host[(i * batch) % n_pos:][:batch], i, W, flags, p, min_crop, theta),
                'batch_device eager': lambda i: fd.batch_device(perm[(i * batch) % n_pos:][:batch]),
                'GraphedBatch replay': lambda i: gb(perm[(i * batch) % n_pos:][:batch])}
        print(f'rotation {"on" if rot else "off"}')
        ms = {name: [] for name in legs}
        for rep in range(3):
            for name, fn in legs.items():
                k = HOST_BATCHES if name.startswith('host') else batches
                _timed(fn, 1 if name.startswith('host') else 5)
                ms[name].append(1e3 * _timed(fn, k))
                print(f'  repeat {rep}: {name:26s} {ms[name][-1]:10.4f} ms/batch')
        for name in list(legs)[1:]:
            print(f'  {name}: slowest repeat {max(ms[name]):.4f} ms against the host leg\'s fastest {min(ms["host torch pipeline + copy"]):.3f} ms')
        ids = perm[:batch].contiguous()
        crop, _, rmat, _ = ops.clip_crop_draw(fd._extent, ids, fd._rng.clone(), flags, p[0], p[1], min_crop, theta)
        us = _alone(lambda: ops.clip_resize(fd._raw, ids, crop, W, rmat), batches)
        nbytes = _resize_bytes(R, crop.cpu().numpy(), shape[0], W, shape[2] * shape[3])
        print(f'  resize alone, {batches} launches in one graph: {us:.2f} us per launch, {nbytes / 1e6:.2f} MB needed -> {nbytes / us / 1e6:.3f} TB/s '
              f'(launch gaps included)')
    # the yardstick: clip_transform's centre crop of the same split to the same window, measured the same way
    fc = _feeder(data, W, 0)
    ids = perm[:batch].contiguous()
    plan, _, _, _, _ = ops.clip_draw(fc._extent, ids, fc._rng.clone(), 0, fc.T, fc.W, len(fc.node), None)
    us = _alone(lambda: ops.clip_transform(fc._raw, ids, plan, fc.W, None, None), batches)
    nbytes = _gather_bytes(plan.cpu().numpy(), shape[0], fc.T, fc.W, shape[2] * shape[3])
    print(f'clip_transform (centre crop, no flags) alone, {batches} launches in one graph: {us:.2f} us per launch, {nbytes / 1e6:.2f} MB needed -> '
          f'{nbytes / us / 1e6:.3f} TB/s (launch gaps included)')
    # one captured training step of the NTU model fed by a GraphedBatch: this mode's 64-frame windows beside the padded 300 frames
    fd300 = _feeder(data, -1, 0)
    sets = {64: (_ntu_step(batch, 64), GraphedBatch(feeders[True], batch)), 300: (_ntu_step(batch, 300), GraphedBatch(fd300, batch))}
    print(f'CapturedStep of the NTU model (CTR-GCN, 25 joints, 2 persons, batch {batch}, FusedSGD) fed by GraphedBatch; {steps} steps per leg, 3 repeats, legs alternated')
    loss = {}
    for rep in range(3):
        for w, (train, gb) in sets.items():
            def step(i, train=train, gb=gb):
                loss[w] = train.step(*gb(perm[(i * batch) % n_pos:][:batch]))
            _timed(step, 2)
            print(f'  repeat {rep}: W = {w:3d}  {1e3 * _timed(step, steps):9.3f} ms/step (batch + step), last loss {float(loss[w]):.4f}')


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
    elif mode == 'resize':
        time_resize(*(int(a) for a in sys.argv[2:4]))
    elif mode == 'trace':
        trace(*(int(a) for a in sys.argv[2:3]))
    elif mode == 'report':
        report(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        raise SystemExit(__doc__)
