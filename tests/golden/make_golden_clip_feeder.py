"""Golden vectors for the clip feeder (tam_gcn_amd/feeder/clip_feeder.py).  Runs ONLY in the build container.

The reference's feeder/tools.py imports torchvision.transforms and PIL for its RGB loader only; both are stubbed in
sys.modules for the import, as make_golden_feeder.py does.  Small synthetic clips (C, T, V, M) of fp32-representable values go,
as fp64, through the reference's own functions in the order of feeder/feeder_nucla_fusion.py:95-106 -- random_shift,
random_choose or auto_pading + centre crop, random_move -- under random.seed(s) / np.random.seed(s).  The draws are recorded by
seeding again and repeating the reference's RNG calls in their order.  What is stored is data only: the clips, and per case
its configuration, the draws and the reference's output.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clip_feeder.py
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

tv = types.ModuleType('torchvision')
tvt = types.ModuleType('torchvision.transforms')
for name in ('Compose', 'Resize', 'ToTensor', 'Normalize'):
    setattr(tvt, name, lambda *a, **k: None)
tv.transforms = tvt
pil = types.ModuleType('PIL')
pil.Image = types.ModuleType('PIL.Image')
for mod_name, mod in (('torchvision', tv), ('torchvision.transforms', tvt), ('PIL', pil), ('PIL.Image', pil.Image)):
    sys.modules.setdefault(mod_name, mod)

from feeder import tools      # noqa: E402  (reference's)

SHIFT, CHOOSE, MOVE = 1, 2, 4
ANGLES, SCALES, TRANS = (list(tools.random_move.__defaults__[k]) for k in (0, 1, 2))


def clips(seed, C, T, V, M):
    """Five clips: leading and trailing zero frames; no zero frame; all zeros; a frame holding only -0.0 at the end of the valid
    range (and zero frames before); a frame holding one NaN between zero frames."""
    r = np.random.RandomState(seed)
    x = r.uniform(-1.0, 1.0, size=(5, C, T, V, M)).astype(np.float32)
    x[0][:, :max(1, T // 4)] = 0
    x[0][:, T - max(1, T // 6):] = 0
    x[2][:] = 0
    x[3][:, 0] = 0
    x[3][:, T - 2:] = 0
    x[3][:, T - 2] = -0.0
    x[4][:, 1:] = 0
    x[4][:, 0] = 0
    x[4][0, T // 2, V - 1, 0] = np.nan
    x[4][:, T // 2 + 1] = r.uniform(-1.0, 1.0, size=(C, V, M)).astype(np.float32)
    return x


def reference(clip, W, flags, move_time):
    data = np.array(clip, dtype=np.float64)
    if flags & SHIFT:
        data = tools.random_shift(data)
    if flags & CHOOSE:
        data = tools.random_choose(data, W)
    elif W > 0:
        data = tools.auto_pading(data, W)
        T = data.shape[1]
        if T > W:
            begin = (T - W) // 2
            data = data[:, begin:begin + W, :, :]
    if flags & MOVE:
        data = tools.random_move(np.array(data), move_time_candidate=[move_time])
    return np.asarray(data, dtype=np.float64)


def draws(clip, W, flags, move_time, seed):
    """The reference's RNG calls, in its order, on generators seeded like the run above."""
    random.seed(seed)
    np.random.seed(seed)
    T = clip.shape[1]
    bias = d = 0
    if flags & SHIFT:
        valid = (clip != 0).sum(axis=3).sum(axis=2).sum(axis=0) > 0
        begin, end = valid.argmax(), len(valid) - valid[::-1].argmax()
        bias = random.randint(0, T - (end - begin))
    if flags & CHOOSE:
        if T > W:
            d = random.randint(0, T - W)
        elif T < W:
            d = -random.randint(0, W - T)
    elif T > W:
        d = (T - W) // 2
    move = np.zeros((0, 4), dtype=np.int32)
    if flags & MOVE:
        random.choice([move_time])
        n = len(np.arange(0, W, W * 1.0 / move_time)) + 1
        state = np.random.get_state()
        vals = [np.random.choice(c, n) for c in (ANGLES, SCALES, TRANS, TRANS)]
        move = np.stack([[list(c).index(v) for v in col] for col, c in zip(vals, (ANGLES, SCALES, TRANS, TRANS))], axis=1).astype(np.int32)
        np.random.set_state(state)                 # choice(list, n) is list[randint(0, len(list), n)] on the same stream
        again = np.stack([np.random.randint(0, len(c), n) for c in (ANGLES, SCALES, TRANS, TRANS)], axis=1)
        assert np.array_equal(again, move)
    return np.array([bias, d], dtype=np.int32), move


def main():
    out = {'angles': np.array(ANGLES, dtype=np.float64), 'scales': np.array(SCALES, dtype=np.float64), 'trans': np.array(TRANS, dtype=np.float64)}
    sets = {'A': clips(1, 3, 12, 5, 2), 'B': clips(2, 2, 7, 3, 1)}
    for k, v in sets.items():
        out[f'{k}/clips'] = v
    # (set, window_size, flags, move_time)
    configs = [('A', 8, f, 1) for f in range(8)] + [('A', 16, 7, 1), ('A', 16, 2, 1), ('A', 16, 0, 1), ('A', 12, 7, 1), ('A', -1, 5, 1),
                                                    ('A', 8, 7, 3), ('A', 16, 4, 3), ('B', 1, 7, 1), ('B', 1, 0, 1), ('B', 9, 6, 3), ('B', 9, 1, 1)]
    cases = []
    for ci, (s, ws, flags, mt) in enumerate(configs):
        n = len(sets[s])
        for j in ((ci % n, (ci + 2) % n) if s == 'A' else range(n)):        # two clips per configuration of the larger set
            clip = sets[s][j]
            W = ws if ws > 0 else clip.shape[1]
            seed = 100 * ci + j
            random.seed(seed)
            np.random.seed(seed)
            got = reference(clip, ws if (flags & CHOOSE) == 0 else W, flags, mt)
            shift, move = draws(clip.astype(np.float64), W, flags, mt, seed)
            k = len(cases)
            cases.append([ord(s), j, ws, flags, mt, seed])
            out[f'case{k}/out'] = got
            out[f'case{k}/shift'] = shift
            out[f'case{k}/move'] = move
            assert got.shape[1] == W, (got.shape, W)
    out['cases'] = np.array(cases, dtype=np.int64)
    path = os.path.join(HERE, 'clip_feeder.npz')
    np.savez_compressed(path, **out)
    print('clip_feeder.npz', len(cases), 'cases', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
