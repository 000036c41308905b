"""GPU-side mirror of the reference's skeleton feeder, ``feeder/feeder_nucla_gcn.py``.

Same constructor arguments, same ``__getitem__`` contract -- ``(data float32 (3, 52, 20, 1), rgb_tensor, label, index)``
(reference :154) -- and the same consumption of Python's ``random`` on the train path (:89-91, :112), but the per-sample
numpy arithmetic (:98-130: centre on joint 1 of frame 0, view rotation and scale, per-coordinate min-max to [-1, 1],
resampling to 52 frames, bone / motion streams) runs as ONE workgroup per clip on the MI355X
(``tamgcn_feeder_transform``, csrc/feeder.hip) over raw skeletons that stay resident in HBM, in fp64 like numpy.
``batch(indices)`` transforms a whole batch in one launch and returns tensors on the device: that is the form the
data-parallel step uses (at >= 10 k clips/s per GPU a per-sample Python feeder is the bottleneck).

Differences, stated:
  * the two split lists the reference carries as 28 kB / 61 kB source literals (:22, :25) are dataset metadata, not code:
    pass ``data_dict=[{'file_name': ..., 'label': ...}, ...]`` (or ``split_file=`` a JSON file holding that list) to fix
    the sample order; without either, ``data_path`` is scanned and split by the N-UCLA cross-view rule those lists follow
    (camera view 3 = val, views 1 and 2 = train), sorted by name, label from the action id (a01..a06, a08, a09, a11,
    a12 -> 1..10);
  * the RGB part (:131-152: last ``*rgb.jpg`` frame through a torchvision transform) is the other modality and out of
    scope: ``rgb_tensor`` is the zeros tensor the reference returns when a sample has no image (:132);
  * label paths containing both 'bone' and 'motion' select the bone stream in the reference (the ``elif`` at :124); the same
    here by default, ``stream='bone_motion'`` asks for motion-of-bone explicitly (upstream CTR-GCN's fourth stream).

A second way to ask for a batch, with no host work per sample: ``batch_device(indices)`` takes the sample indices as a
tensor on the device and draws the train path's view angles, scale and 52 frames per clip in a HIP kernel
(``tamgcn_feeder_draw``: Philox4x32-10 keyed by ``seed``, counted by a call counter that lives on the device) --
the reference's distributions, not its Python ``random`` stream, which ``batch()`` / ``__getitem__`` keep mirroring call
for call.  It makes no host-to-device copy and no synchronisation, so ``GraphedBatch`` can hold it in a HIP graph:

    fd = Feeder(path, 'train', data_dict=split, seed=1234)          # data-parallel: seed=base + rank, see below
    gb = GraphedBatch(fd, 256)
    perm = torch.randperm(len(fd), device=dev)
    for i in range(0, len(fd) - 255, 256):
        loss = train.step(*gb(perm[i:i + 256]))                    # training.CapturedStep

Slot b of call c with seed s always gets the same draws, whatever the other slots hold.  Ranks of a data-parallel run
must pass different seeds (``seed=base + rank``): with equal seeds every rank would apply the same views to its slots.
``rng_state()`` / ``set_rng_state()`` carry (seed, call) through a checkpoint.
"""
import json
import math
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import ops

ACTION_TO_LABEL = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 8: 7, 9: 8, 11: 9, 12: 10}
# reference :27-28, pair (v1, v2) at list position v1 - 1 -> 0-based parent of joint v
BONE_PARENT = (1, 2, 2, 2, 2, 4, 5, 6, 2, 8, 9, 10, 0, 12, 13, 14, 0, 16, 17, 18)


def _scan_split(data_path, val):
    out = []
    for name in sorted(os.listdir(data_path)):
        parts = name.split('_')
        if len(parts) != 4 or not (parts[0][:1] == 'a' and parts[3][:1] == 'v'):
            continue
        view, action = int(parts[3][1:]), int(parts[0][1:])
        if (view == 3) == val and action in ACTION_TO_LABEL:
            out.append({'file_name': name, 'label': ACTION_TO_LABEL[action]})
    return out


def view_matrix(agx, agy, s):
    """Ry . Rx . S of reference :75-83 (degrees in, row-vector convention: p' = p . R), float64."""
    agx, agy = math.radians(agx), math.radians(agy)
    Rx = np.asarray([[1, 0, 0], [0, math.cos(agx), math.sin(agx)], [0, -math.sin(agx), math.cos(agx)]])
    Ry = np.asarray([[math.cos(agy), 0, -math.sin(agy)], [0, 1, 0], [math.sin(agy), 0, math.cos(agy)]])
    Ss = np.asarray([[s, 0, 0], [0, s, 0], [0, 0, s]])
    return np.dot(Ry, np.dot(Rx, Ss))


class Feeder(Dataset):
    def __init__(self, data_path, label_path, repeat=1, random_choose=False, random_shift=False, random_move=False,
                 window_size=-1, normalization=False, debug=False, use_mmap=True, data_dict=None, split_file=None,
                 device='cuda', stream=None, seed=0):
        self.data_path, self.label_path = data_path, label_path
        self.train_val = 'val' if 'val' in label_path else 'train'
        if data_dict is None and split_file is not None:
            with open(split_file) as f:
                data_dict = json.load(f)
        self.data_dict = list(data_dict) if data_dict is not None else _scan_split(data_path, self.train_val == 'val')
        self.time_steps = 52
        self.bone = [(v + 1, p + 1) for v, p in enumerate(BONE_PARENT)]
        self.label = [int(info['label']) - 1 for info in self.data_dict]
        self.debug, self.random_choose, self.random_shift, self.random_move = debug, random_choose, random_shift, random_move
        self.window_size, self.normalization, self.use_mmap, self.repeat = window_size, normalization, use_mmap, repeat
        if stream is None:                                   # reference :119-127
            stream = 'bone' if 'bone' in label_path else ('motion' if 'motion' in label_path else 'joint')
        if stream not in ops.STREAM_MODES:
            raise ValueError(f'unknown stream {stream!r}')
        self.stream = stream
        self.device = torch.device(device)
        self.seed, self.last_draws = self._check_seed(seed, 'seed'), None
        self.load_data()
        if normalization:
            self.get_mean_map()

    # ---- reference :52-64: every clip of the split, JSON {"skeletons": [[[x, y, z] x 20] x length]} ----------------
    def load_data(self):
        self.data = []
        for info in self.data_dict:
            name = info['file_name']
            with open(os.path.join(self.data_path, name, name + '.json'), 'r') as f:
                self.data.append(np.array(json.load(f)['skeletons'], dtype=np.float64))
        lens = [len(v) for v in self.data]
        for info, n in zip(self.data_dict, lens):               # the device-side draw indexes 100 * length positions
            if n < 1 or 100 * n >= 2 ** 24:
                raise ValueError(f"clip {info['file_name']!r} has {n} frames: the feeder takes 1 .. {(2 ** 24 - 1) // 100}")
        self._offsets_cpu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        raw = np.concatenate(self.data, axis=0) if self.data else np.zeros((0, 20, 3))
        if raw.shape[1:] != (20, 3):
            raise ValueError(f'expected (length, 20, 3) skeletons, got {raw.shape}')
        # the whole split stays resident in HBM (N-UCLA: 1484 clips x ~40 frames x 60 doubles = 28 MB)
        self._raw = torch.from_numpy(np.ascontiguousarray(raw)).to(self.device)
        self._parent = torch.tensor(BONE_PARENT, dtype=torch.int32, device=self.device)
        # what batch_device() reads, resident once: frame offsets, labels, the host libm's cos / sin of -60 .. 60 degrees
        # (so that the device's view matrix is built from view_matrix()'s own values) and the generator state
        self._offsets = torch.from_numpy(self._offsets_cpu).to(self.device)
        self._labels = torch.tensor(self.label, dtype=torch.int64, device=self.device)
        self._cossin = torch.tensor([[math.cos(math.radians(a)), math.sin(math.radians(a))] for a in range(-60, 61)],
                                    dtype=torch.float64, device=self.device)
        self._rng = torch.tensor([self.seed, 0], dtype=torch.int64, device=self.device)

    def get_mean_map(self):
        raise NotImplementedError('normalization=True: the reference computes it over a 5-D array its own loader never '
                                  'produces (feeder_nucla_gcn.py:66-70 would fail on ragged clips); unsupported here too')

    def __len__(self):
        return len(self.data_dict) * self.repeat

    # ---- host side of one sample: exactly the reference's RNG consumption (:88-93, :110-117) ----------------------
    def _draw(self, index):
        length = len(self.data[index])
        if self.train_val == 'train':
            agx = random.randint(-60, 60)
            agy = random.randint(-60, 60)
            s = random.uniform(0.5, 1.5)
            idx = random.sample(list(np.arange(length)) * 100, self.time_steps)
            idx.sort()
            idx = np.asarray(idx, dtype=np.int32)
        else:
            agx, agy, s = 0, 0, 1.0
            idx = np.linspace(0, length - 1, self.time_steps).astype(int).astype(np.int32)
        return view_matrix(agx, agy, s), idx

    def batch(self, indices):
        """(data (B, 3, 52, 20, 1) float32 on the device, labels (B,) int64 on the device, indices) in ONE launch."""
        indices = [int(i) % len(self.data_dict) for i in indices]
        rots, idxs = zip(*(self._draw(i) for i in indices))
        offs = np.zeros(len(indices) + 1, dtype=np.int64)
        sel = []
        for b, i in enumerate(indices):                     # gather the clips' frame ranges (device-side, one index_select)
            lo, hi = self._offsets_cpu[i], self._offsets_cpu[i + 1]
            sel.append(np.arange(lo, hi))
            offs[b + 1] = offs[b] + (hi - lo)
        sel = torch.from_numpy(np.concatenate(sel)).to(self.device)
        raw = self._raw.index_select(0, sel).contiguous()
        out = ops.feeder_transform(raw, torch.from_numpy(offs).to(self.device),
                                   torch.from_numpy(np.ascontiguousarray(np.stack(rots))).to(self.device),
                                   torch.from_numpy(np.ascontiguousarray(np.stack(idxs))).to(self.device),
                                   self._parent, 20, self.time_steps, 1, self.stream)
        lab = torch.tensor([self.label[i] for i in indices], dtype=torch.int64, device=self.device)
        return out, lab, indices

    # ---- the same batch without the host: draws on the device, the resident split read in place --------------------
    def batch_device(self, indices):
        """(data (B, 3, 52, 20, 1) float32, labels (B,) int64), both on the device, for ``indices`` an int64 tensor [B] on
        the device (taken modulo the split's size, as ``batch()`` does for ``repeat``).  Train or val by ``label_path``,
        stream by ``stream``, exactly as ``batch()``; the train path's draws come from the device-resident generator
        (module docstring), whose call counter moves on by one.  Three launches on the current stream, no host loop, no
        copy from the host, no synchronisation: capturable (``GraphedBatch``).  ``last_draws`` keeps what the launch
        drew: ``view`` (B, 3) = (agx, agy, s), ``rot`` (B, 3, 3), ``idx`` (B, 52)."""
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int64 and indices.dim() == 1
                and indices.device == self._raw.device and indices.numel() > 0):
            raise ValueError('Feeder.batch_device: indices must be a non-empty 1-D int64 tensor on the feeder\'s device '
                             '(batch() takes host indices)')
        if not self.data_dict:
            raise ValueError('Feeder.batch_device: the split is empty')
        indices = indices.contiguous()
        view, rot, idx, lab = ops.feeder_draw(self._offsets, indices, self._rng, self._cossin, self.time_steps,
                                              self.train_val == 'train', labels=self._labels)
        out = ops.feeder_transform_indexed(self._raw, self._offsets, indices, rot, idx, self._parent, 20, self.time_steps, 1,
                                           self.stream)
        self.last_draws = {'view': view, 'rot': rot, 'idx': idx}
        return out, lab

    @staticmethod
    def _check_seed(v, what):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 63:
            raise ValueError(f'Feeder: {what} = {v!r} must be an integer in [0, 2^63)')
        return v

    def manual_seed(self, seed, call=0):
        """Write (seed, call) into the device-resident generator state on the current stream.  Graphs captured earlier
        read the state on every replay, so this takes effect on them too."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('Feeder.manual_seed: set the seed outside graph capture (a captured write would replay '
                               'the value of capture time)')
        self.seed = self._check_seed(seed, 'seed')
        self._rng.copy_(torch.tensor([self.seed, self._check_seed(call, 'call')], dtype=torch.int64))

    def rng_state(self):
        """(seed, call): the next batch_device() call draws call number ``call`` (reads the device: a host sync)."""
        seed, call = self._rng.tolist()
        return seed, call

    def set_rng_state(self, state):
        seed, call = state
        self.manual_seed(int(seed), int(call))

    def __getitem__(self, index):
        index = index % len(self.data_dict)
        out, _, _ = self.batch([index])
        rgb_tensor = torch.zeros(3, 299, 299)              # reference :132 (no image / RGB modality out of scope)
        return out[0].cpu().numpy().astype(np.float32), rgb_tensor, self.label[index], index

    def top_k(self, score, top_k):
        rank = score.argsort()
        hit_top_k = [l in rank[i, -top_k:] for i, l in enumerate(self.label)]
        return sum(hit_top_k) * 1.0 / len(hit_top_k)


class GraphedBatch:
    """One ``feeder.batch_device`` call of ``batch_size`` samples held in a HIP graph.  ``x, y = gb(indices)`` copies the
    indices (int64 [batch_size], on the device) into the graph's input and replays it: new draws every time, because the
    generator state is read and advanced on the device.  ``x`` and ``y`` are the graph's own output tensors, overwritten by
    the next call (``CapturedStep.step`` copies them into its inputs); ``feeder.last_draws`` are the replay's draws.
    Building it warms the kernels up on a side stream and puts the generator state back: it consumes no draws."""

    def __init__(self, feeder, batch_size):
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f'GraphedBatch: batch_size = {batch_size!r} must be an integer >= 1')
        self.feeder, self.batch_size = feeder, batch_size
        dev = feeder._raw.device
        self.indices = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            saved = feeder._rng.clone()
            feeder.batch_device(self.indices)
            feeder._rng.copy_(saved)
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        self._graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self._graph):
                self.x, self.y = feeder.batch_device(self.indices)
        except Exception as e:                                  # noqa: BLE001  -- no silent eager fall-back
            raise RuntimeError(f'GraphedBatch: HIP graph capture failed ({type(e).__name__}: {e})') from e
        self.draws = feeder.last_draws

    def __call__(self, indices):
        if not isinstance(indices, torch.Tensor) or tuple(indices.shape) != (self.batch_size,) or indices.dtype != torch.int64:
            raise ValueError(f'GraphedBatch: indices must be an int64 tensor of {self.batch_size} elements, got '
                             f'{tuple(getattr(indices, "shape", ()))} {getattr(indices, "dtype", type(indices))}')
        self.indices.copy_(indices)
        self._graph.replay()
        self.feeder.last_draws = self.draws
        return self.x, self.y


def import_class(name):
    components = name.split('.')
    mod = __import__(components[0])
    for comp in components[1:]:
        mod = getattr(mod, comp)
    return mod
