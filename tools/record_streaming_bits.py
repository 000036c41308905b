"""GPU-box tool: the outputs of the single-ring streaming ops on small seeded inputs, as arrays (tests/golden/streaming_parent.npz;
tests/test_gpu_streaming_bits.py compares every array bit for bit).

    python tools/record_streaming_bits.py <out.npz>

Only the public names of tam_gcn_amd.ops are used -- ring_push, ring_plan, window_nucla, window_clip, score_ema -- so the same
file runs on any commit that keeps them: record on the commit whose bits are the standard, compare on every later one.  No model
is involved; every input is seeded numpy data."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = 'cuda:0'
CAP = 16
PUSHES = (3, 1, 16, 3, 16, 1, 3)                       # 43 frames through 16 slots: the ring wraps more than twice
# name -> ring shape; rows of 144 bytes (16-byte units), 120 bytes (8-byte), 68 bytes (4-byte), 48 bytes (16-byte)
RINGS = {'nucla_v6': (CAP, 6, 3), 'nucla_v5': (CAP, 5, 3), 'clip_v17': (3, CAP, 17, 1), 'clip_v6x2': (2, CAP, 6, 2)}
PARENTS = {'nucla_v6': (0, 0, 1, 2, 1, 4), 'nucla_v5': (0, 0, 1, 1, 3)}
# after the pushes frames 27 .. 42 remain: a window that wraps (slots 14 .. 22), one frame, an invalid row, W = L = 8, the whole ring
WINDOWS = ((30, 9), (42, 1), (0, 0), (34, 8), (27, 16))
STREAMS = ('joint', 'bone', 'motion', 'bone_motion')
EMA_VALID = (0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1)       # 12 steps, two invalid: before the first valid window and between two


def record():
    import torch
    from tam_gcn_amd import ops
    dev = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)     # noqa: E731
    out = {}
    rings = {}
    for k, (name, shape) in enumerate(RINGS.items()):
        rng = np.random.default_rng(100 + k)
        fp64 = len(shape) == 3
        ring = torch.zeros(shape, dtype=torch.float64 if fp64 else torch.float32, device=DEV)
        state = torch.zeros(2, dtype=torch.int64, device=DEV)
        for i, n in enumerate(PUSHES):
            fshape = (n,) + shape[1:] if fp64 else (shape[0], n) + shape[2:]
            frames = rng.normal(size=fshape)
            ops.ring_push(dev(frames if fp64 else frames.astype(np.float32)), ring, state)
            out[f'push/{name}/{i}/ring'], out[f'push/{name}/{i}/state'] = ring.cpu().numpy(), state.cpu().numpy()
        rings[name] = ring
    for count in (5, 16, 40):                          # not yet; valid; the oldest row overwritten
        state = torch.tensor([count, 1], dtype=torch.int64, device=DEV)
        out[f'plan/{count}'] = ops.ring_plan(state, CAP, 3, 9, 4).cpu().numpy()
    plan = dev(WINDOWS, torch.int64)
    for name, ring in rings.items():
        if name in PARENTS:
            for stream in STREAMS:
                out[f'window_nucla/{name}/{stream}'] = ops.window_nucla(ring, plan, dev(PARENTS[name], torch.int32), 8, 1, stream).cpu().numpy()
        else:
            for W in (8, 16):
                out[f'window_clip/{name}/W{W}'] = ops.window_clip(ring, plan, W).cpu().numpy()
    K = 10
    for beta in (0.0, 0.8):
        rng = np.random.default_rng(7)
        ema = torch.zeros(K, dtype=torch.float64, device=DEV)
        seen = torch.zeros(1, dtype=torch.int64, device=DEV)
        for i, valid in enumerate(EMA_VALID):
            e = np.exp(rng.normal(size=K))
            probs = (e / e.sum()).astype(np.float32)
            row = torch.tensor([i, 9 * valid], dtype=torch.int64, device=DEV)
            smoothed, label, conf = ops.score_ema(dev(probs), row, beta, ema, seen)
            for what, t in (('ema', ema), ('seen', seen), ('out', smoothed), ('label', label), ('conf', conf)):
                out[f'score_ema/beta{beta}/{i}/{what}'] = t.cpu().numpy()
    return out


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    arrays = record()
    np.savez_compressed(sys.argv[1], **arrays)
    print(f'{len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)')
