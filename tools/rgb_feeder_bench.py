"""GPU-box tool: what a batch of the RGB modality costs on each path (profiles/rgb_feeder_bench.txt).

    python tools/rgb_feeder_bench.py time [rounds]
        640 x 480 sources generated from a seed, S = 224, F = 5, at B = 16 (the reference's batch) and B = 64: ms per batch of
          (a) the reference-shaped host loop: per sample PIL resize of the decoded image, ToTensor, Normalize, tile, then stack
              and .to(device)                                           (needs PIL; "not measured" without it)
          (b) a host leg given the feeder's advantage: pre-resized uint8 on the host, torch normalise, tile and copy
          (c) RGBFeeder.batch_device() launched eagerly
          (d) a GraphedBatch replay
        legs alternated in one process, median of `rounds` (>= 5) rounds with the spread (min .. max).  Then the one-off cost of
        the load-time resize of 1020 such images and the store's size, and the row_scale path against batch_device() followed
        by the guidance's multiplication (torch.ops.tamgcn.guidance_apply, what SkeletonGuidance.apply launches).
    python tools/rgb_feeder_bench.py trace [batches]
        `batches` eager batch_device calls at B = 16, then at B = 64 -- run it under rocprofv3 --kernel-trace
    python tools/rgb_feeder_bench.py report <kernel_trace.csv or a directory holding one> [batches]
        tamgcn_rgb_batch's kernel time per batch from that trace, and the bytes it needs, B S^2 (3 + 12 F), over that time

Every timed window starts and ends with a device synchronise; every leg is warmed up before it is timed.
"""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = 'cuda:0'
H0, W0, S, F = 480, 640, 224, 5
BATCHES = (16, 64)
N_BENCH, N_SPLIT = 64, 1020            # images behind the timed batches; images of the load-time resize (the N-UCLA train split)


def _sources(n, seed=0):
    """Seeded uint8 (n, 480, 640, 3): a low-frequency pattern plus noise, so neither constant nor white."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H0, 0:W0]
    base = (127.5 + 100.0 * np.sin(x / 37.0) * np.cos(y / 23.0)).astype(np.int16)[:, :, None]
    out = np.empty((n, H0, W0, 3), dtype=np.uint8)
    for i in range(n):
        out[i] = np.clip(base + rng.integers(-40, 41, size=(H0, W0, 3), dtype=np.int16), 0, 255)
    return out


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def _line(name, ts):
    return f'    {name:<58} {statistics.median(ts):9.4f} ms   ({min(ts):.4f} .. {max(ts):.4f})'


def time_batches(rounds=7):
    import numpy as np
    import torch
    from tam_gcn_amd import torch_ops  # noqa: F401
    from tam_gcn_amd.feeder import rgb_feeder as R
    from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch
    try:
        from PIL import Image
    except ImportError:
        Image = None
    rounds = max(5, rounds)
    src = _sources(N_BENCH)
    fd = R.RGBFeeder(src, np.arange(N_BENCH) % 10, size=S, temporal_rgb_frames=F, device=DEV)
    store_host = fd._raw.cpu()
    mean, std = (torch.tensor(v, dtype=torch.float32) for v in (R.IMAGENET_MEAN, R.IMAGENET_STD))
    pil = [Image.fromarray(im) for im in src] if Image is not None else None
    rng = np.random.default_rng(1)
    print(f'sources {W0} x {H0}, S = {S}, F = {F}; {rounds} rounds, legs alternated, median (min .. max)')
    for B in BATCHES:
        ids_host = [rng.integers(0, N_BENCH, size=B) for _ in range(64)]
        ids_dev = [torch.from_numpy(v).to(DEV) for v in ids_host]
        gb = GraphedBatch(fd, B)

        def ref_loop(i):
            out = []
            for j in ids_host[i % 64]:
                a = np.asarray(pil[j].resize((S, S), Image.BILINEAR))
                t = torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
                t = t.sub_(mean[:, None, None]).div_(std[:, None, None]).numpy()
                out.append(np.concatenate([t] * F, axis=0))
            return torch.from_numpy(np.stack(out)).to(DEV)

        def host_resized(i):
            t = store_host[torch.from_numpy(ids_host[i % 64])].permute(0, 3, 1, 2).to(torch.float32).div(255)
            t = t.sub_(mean[None, :, None, None]).div_(std[None, :, None, None])
            return t.repeat(1, F, 1, 1).to(DEV)

        legs = [('(b) host, pre-resized uint8: normalise, tile, copy', host_resized, 3),
                ('(c) batch_device, eager', lambda i: fd.batch_device(ids_dev[i % 64]), 200),
                ('(d) GraphedBatch replay', lambda i: gb(ids_dev[i % 64]), 200)]
        if pil is not None:
            legs.insert(0, ('(a) reference-shaped host loop: PIL resize .. .to(device)', ref_loop, 2))
        same = torch.equal(host_resized(0), fd.batch_device(ids_dev[0])[0])
        if pil is not None:
            same = same and torch.equal(ref_loop(0), fd.batch_device(ids_dev[0])[0])
        for _, fn, k in legs:
            _timed(fn, min(k, 20))
        ts = {name: [] for name, _, _ in legs}
        for _ in range(rounds):
            for name, fn, k in legs:
                ts[name].append(_timed(fn, k))
        print(f'B = {B}: out {B * 3 * F * S * S * 4 / 1e6:.1f} MB per batch; host legs and device legs give the same bits: {same}')
        if pil is None:
            print('    (a) reference-shaped host loop: not measured (PIL is not installed)')
        for name, _, _ in legs:
            print(_line(name, ts[name]))
        del gb
    # ---- the row_scale path against batch_device + the guidance's multiplication -----------------------------------------------
    B = 16
    ids = torch.from_numpy(rng.integers(0, N_BENCH, size=B)).to(DEV)
    w = torch.rand(B, 5, device=DEV) * 2.0                       # joint weights as SkeletonGuidance.joint_weights gives them: (N, J)
    wmap = torch.ops.tamgcn.guidance_apply(w, None, F, S, S, True)[1]
    rows = wmap[:, 0, :, 0].contiguous()
    constant = torch.equal(wmap, rows[:, None, :, None].expand_as(wmap))
    two = lambda i: torch.ops.tamgcn.guidance_apply(w, fd.batch_device(ids)[0], F, S, S, False)[0]      # noqa: E731
    one = lambda i: fd.batch_device(ids, row_scale=torch.ops.tamgcn.guidance_apply(w, None, F, S, S, True)[1][:, 0, :, 0].contiguous())[0]   # noqa: E731
    same = torch.equal(one(0), two(0))
    for fn in (one, two):
        _timed(fn, 20)
    t1, t2 = [], []
    for _ in range(rounds):
        t1.append(_timed(one, 200))
        t2.append(_timed(two, 200))
    print(f'guidance, B = {B}: the weight map is constant along x: {constant}; the two paths give the same bits: {same}')
    print(_line('weight_map rows + batch_device(row_scale=)', t1))
    print(_line('batch_device + guidance_apply', t2))
    del fd
    # ---- the one-off cost at load ---------------------------------------------------------------------------------------------------
    big = _sources(60, seed=2)[np.arange(N_SPLIT) % 60]          # 60 distinct images, repeated: the resize does not care
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fd = R.RGBFeeder(big, np.arange(N_SPLIT) % 10, size=S, temporal_rgb_frames=F, device=DEV)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    up = torch.from_numpy(big[:256]).to(DEV)
    R.resize(up, (S, S))
    t = _timed(lambda i: R.resize(up, (S, S)), 3)
    print(f'load: RGBFeeder of {N_SPLIT} decoded {W0} x {H0} images (upload + resize + tables): {total:.2f} s once; '
          f'the two resize launches alone: {t / 256 * N_SPLIT:.1f} ms for {N_SPLIT} images ({t / 256 * 1e3:.1f} us per image)')
    print(f'store: {fd._raw.numel() / 1e6:.1f} MB of HBM ({N_SPLIT} x {S} x {S} x 3 uint8)')
    print('a cross-modal training step fed by this feeder (needs a real ResNet trunk): not measured')


def trace(batches=50):
    import numpy as np
    import torch
    from tam_gcn_amd.feeder import rgb_feeder as R
    fd = R.RGBFeeder(_sources(N_BENCH), np.arange(N_BENCH) % 10, size=S, temporal_rgb_frames=F, device=DEV)
    rng = np.random.default_rng(1)
    for B in BATCHES:
        for _ in range(batches):
            fd.batch_device(torch.from_numpy(rng.integers(0, N_BENCH, size=B)).to(DEV))
        torch.cuda.synchronize()


def report(path, batches=50):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True))
        if not found:
            raise SystemExit(f'no *kernel_trace.csv under {path}')
        path = found[0]
    rows = [r for r in csv.DictReader(open(path)) if 'rgb_batch' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    if len(rows) != batches * len(BATCHES):
        raise SystemExit(f'{len(rows)} rgb_batch launches in {path}, expected {batches * len(BATCHES)}')
    print(f'tamgcn_rgb_batch from a kernel trace, {batches} launches per batch size (the first 5 dropped), S = {S}, F = {F}')
    for k, B in enumerate(BATCHES):
        d = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows[k * batches:(k + 1) * batches]][5:]
        need = B * S * S * (3 + 12 * F)
        med = statistics.median(d)
        short = rows[k * batches]['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        print(f'    B = {B:<3} {short:<22} median {med:8.2f} us  ({min(d):.2f} .. {max(d):.2f});  '
              f'{need / 1e6:.1f} MB needed -> {need / med / 1e6:.2f} TB/s')


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        time_batches(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
    elif mode == 'trace':
        trace(int(sys.argv[2]) if len(sys.argv) > 2 else 50)
    elif mode == 'report':
        report(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 50)
    else:
        raise SystemExit(__doc__)
