"""GPU-box tool: what a training batch costs on each of the feeder's two paths (profiles/feeder_device_draw.txt).

    python tools/feeder_bench.py time [batch] [batches] [steps]
        per clip length (40 and 200 frames, seeded synthetic clips): ms per batch of Feeder.batch() (host draws), of
        Feeder.batch_device() launched eagerly and of a GraphedBatch replay, legs alternated, three repeats; then ms per
        training step of CapturedStep (N-UCLA model) fed by batch() and fed by GraphedBatch, alternated, three repeats;
        and the largest difference of batch_device's data to the feeder oracle fed the device's own draws
    python tools/feeder_bench.py trace [batch] [batches]
        `batches` eager batch_device calls per clip length -- run it under rocprofv3 --kernel-trace --stats
    python tools/feeder_bench.py report <kernel_trace.csv> [batches]
        kernel time per batch of the feeder's kernels from that trace

Every timed window starts and ends with a device synchronise; every leg is warmed up before it is timed.
"""
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

MARGS = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
LENGTHS = (40, 200)
N_FILES, N_CLIPS = 64, 1024                    # 64 distinct clips on disk, listed 16 times each: an N-UCLA-sized split
DEV = 'cuda:0'


def _split(root, length, seed=0):
    """data_dict of N_CLIPS entries over N_FILES seeded clips of `length` frames written under root."""
    import numpy as np
    rng = np.random.default_rng(seed + length)
    names = []
    for k in range(N_FILES):
        name = f'a{1 + k % 6:02d}_s{k:02d}_e00_v01'
        clip = rng.normal(size=(1, 20, 3)) + 0.05 * np.cumsum(rng.normal(size=(length, 20, 3)), axis=0)
        os.makedirs(os.path.join(root, name), exist_ok=True)
        with open(os.path.join(root, name, name + '.json'), 'w') as f:
            json.dump({'skeletons': clip.tolist()}, f)
        names.append(name)
    return [{'file_name': names[i % N_FILES], 'label': 1 + i % 10} for i in range(N_CLIPS)]


def _feeder(length, seed=1):
    from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder
    with tempfile.TemporaryDirectory() as root:
        return Feeder(root, 'train', data_dict=_split(root, length), device=DEV, seed=seed)


def _timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def _oracle_diff(fd, batch):
    import numpy as np
    import torch
    from oracle import feeder_oracle as FO
    ids = torch.randperm(len(fd), device=DEV)[:batch]
    out, _ = fd.batch_device(ids)
    v, ix = fd.last_draws['view'].cpu().numpy(), fd.last_draws['idx'].cpu().numpy()
    got, ids = out.cpu().numpy(), ids.tolist()
    return max(float(np.abs(got[b] - FO.transform(fd.data[i], int(v[b, 0]), int(v[b, 1]), float(v[b, 2]), ix[b], fd.stream)).max())
               for b, i in enumerate(ids))


def _step(batch):
    from params import fill_state_, make_input, make_labels
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.functional import CrossEntropyLoss
    from tam_gcn_amd.training import CapturedStep
    m = Model(**MARGS)
    fill_state_(m.state_dict(), seed=0)
    m = m.to(DEV).train()
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    opt = FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    x, y = make_input((batch, 3, 52, 20, 1), 4).to(DEV), make_labels(batch, 10, 5).to(DEV)
    return CapturedStep(m, CrossEntropyLoss(), opt, arena, bucket, x, y)


def time_batches(batch=256, batches=200, steps=40):
    import random
    import torch
    from tam_gcn_amd.feeder.feeder_nucla_gcn import GraphedBatch
    random.seed(0)
    torch.manual_seed(0)
    train = _step(batch)
    print(f'{batch}-clip training batches, joint stream, a split of {N_CLIPS} clips; {batches} batches per leg, 3 repeats, '
          f'legs alternated; N-UCLA model, captured step, FusedSGD, {steps} steps per leg')
    for length in LENGTHS:
        fd = _feeder(length)
        gb = GraphedBatch(fd, batch)
        n_pos = len(fd) - batch + 1
        perm = torch.randperm(len(fd), device=DEV)
        perm_host = perm.tolist()

        def host(i):
            lo = (i * batch) % n_pos
            return fd.batch(perm_host[lo:lo + batch])

        def device(i):
            lo = (i * batch) % n_pos
            return fd.batch_device(perm[lo:lo + batch])

        def graphed(i):
            lo = (i * batch) % n_pos
            return gb(perm[lo:lo + batch])
        legs = {'batch() (host draws)': host, 'batch_device eager': device, 'GraphedBatch replay': graphed}
        ms = {name: [] for name in legs}
        print(f'clips of {length} frames')
        for rep in range(3):
            for name, fn in legs.items():
                _timed(fn, 5)
                ms[name].append(1e3 * _timed(fn, batches))
                print(f'  repeat {rep}: {name:22s} {ms[name][-1]:9.4f} ms/batch')
        base = ms['batch() (host draws)']
        spread = max(base) - min(base)
        for name in list(legs)[1:]:
            gain = min(base) - max(ms[name])
            print(f'  {name}: slowest repeat {max(ms[name]):.4f} ms against batch()\'s fastest {min(base):.4f} ms: '
                  f'{gain:+.3f} ms, spread of the batch() repeats {spread:.3f} ms '
                  f'({"faster by more than" if gain > spread else "NOT faster by more than"} the spread)')
        fed = {'step fed by batch()': lambda i: train.step(*host(i)[:2]), 'step fed by GraphedBatch': lambda i: train.step(*graphed(i))}
        sms = {name: [] for name in fed}
        for rep in range(3):
            for name, fn in fed.items():
                _timed(fn, 3)
                sms[name].append(1e3 * _timed(fn, steps))
                print(f'  repeat {rep}: {name:26s} {sms[name][-1]:9.3f} ms/step')
        a, b = sms['step fed by batch()'], sms['step fed by GraphedBatch']
        print(f'  fed step: mean {sum(b) / 3:.3f} ms against {sum(a) / 3:.3f} ms fed by batch() '
              f'(spread of the batch()-fed repeats {max(a) - min(a):.3f} ms)')
        print(f'  batch_device against the feeder oracle on its own draws, {batch} clips: largest difference {_oracle_diff(fd, batch):.3e}')


def trace(batch=256, batches=200):
    import torch
    for length in LENGTHS:
        fd = _feeder(length)
        perm = torch.randperm(len(fd), device=DEV)
        n_pos = len(fd) - batch + 1
        torch.cuda.synchronize()
        for i in range(batches):
            lo = (i * batch) % n_pos
            fd.batch_device(perm[lo:lo + batch])
        torch.cuda.synchronize()
    print(f'trace: {batches} eager batch_device calls of {batch} clips at each of {LENGTHS} frames (in that order)')


def report(path, batches=200):
    rows = [r for r in csv.DictReader(open(path)) if 'feeder_' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    names = []
    for r in rows:
        short = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        r['short'] = short
        if short not in names:
            names.append(short)
    for short in names:
        ds = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if r['short'] == short]
        for leg, length in enumerate(LENGTHS):                  # the trace runs the lengths one after the other
            d = ds[leg * batches:(leg + 1) * batches]
            if d:
                print(f'  {length:4d} frames: {len(d):5d} x {sum(d) / len(d):8.2f} us  (min {min(d):.2f}, max {max(d):.2f})  {short}')


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        time_batches(*(int(a) for a in sys.argv[2:5]))
    elif mode == 'trace':
        trace(*(int(a) for a in sys.argv[2:4]))
    elif mode == 'report':
        report(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        raise SystemExit(__doc__)
