"""Device-resident feeder for fixed-shape skeleton arrays ``(N, C, T, V, M)``: NTU, Kinetics-skeleton, COCO / OpenPose
keypoints, anything the ST-GCN / CTR-GCN data tools write.  It restates the reference's second feeder,
``feeder/feeder_nucla_fusion.py:84-106``, which takes a clip ``(C, T, V, M)`` through ``feeder/tools.py``:

  1. ``random_shift`` (:118-130): the clip's valid frames -- ``begin`` = first frame with a non-zero element, ``end`` = last
     such frame + 1, ``(0, T)`` when there is none -- are moved to start at ``bias``, uniform on ``0 .. T - size``.
  2. the window ``W`` (``window_size``, or ``T`` when it is <= 0): with ``random_choose`` (:39-62) a crop at ``d`` uniform on
     ``0 .. T - W`` or, for ``T < W``, zero padding with the clip at ``p`` uniform on ``0 .. W - T`` (``d = -p``); without it
     padding at the front or the centre crop ``(T - W) // 2`` (feeder_nucla_fusion.py:99-104).
  3. ``random_move`` (:65-115): angle, scale and two translations drawn per node from candidate lists, interpolated over the
     frames with ``np.linspace``, and ``[x'; y'] = s R(a) [x; y] + [t_x; t_y]`` in fp64 on every frame of the window.  As in
     the reference the padded (zero) frames are moved too and come out as ``(t_x, t_y, 0, ...)``.
  4. ``stream``: 'bone' / 'motion' / 'bone_motion' through ``ops.stream_derive`` (needs ``parent``), last.

Steps 1 and 2 compose to three integers per batch slot -- output frame ``t`` is raw frame ``src0 + t`` for ``lo <= t < hi``
and zero elsewhere (``make_plan``) -- so the kernels (csrc/clipfeeder.hip) build no intermediate clip.  The whole split
stays in HBM as one fp32 array; the clips' extents are computed there once, at load.

``batch(indices)`` draws on the host with ``random`` / ``np.random`` in the reference's call order (seeding both reproduces
the reference's draws).  ``batch_device(indices)`` takes the indices as an int64 tensor on the device and draws there
(``tamgcn_clip_draw``: Philox4x32-10 keyed by ``seed``, counted by a call counter that lives on the device; the stream is
defined in include/tamgcn.h and INTEGRATION.md): no host work, no synchronisation, capturable -- ``GraphedBatch``,
``CapturedEval`` and ``CapturedStep`` take this feeder as they take the N-UCLA one.  ``normalization=True`` is accepted and
does nothing, as in the reference (``get_mean_map`` at :34-35 is empty).  RGB loading is the other modality: it lives in
``feeder/rgb_feeder.py`` (``RGBFeeder``), and ``FusionFeeder`` there pairs this feeder with it for the fusion batch.

``p_interval=`` switches to a second pipeline, the one CTR-GCN was published with for NTU-style arrays (its
``feeders/tools.py``: ``valid_crop_resize`` and ``random_rot``), in place of steps 1 to 3:

  a. crop a share ``p`` of the clip's valid frames: ``p_interval=[p]`` the centre crop (evaluation), ``p_interval=[p0, p1]``
     a share drawn per sample at a drawn place, at least ``min_crop`` frames long (training);
  b. resize the crop linearly in time to ``window_size`` frames (``F.interpolate(mode='bilinear', align_corners=False)`` on
     the time axis alone);
  c. ``random_rot``: one rotation per clip, ``Rz Ry Rx`` with the three angles uniform on ``[-rot_theta, rot_theta)``.

``stream`` is derived last, as above.  The valid frames are those of the clip's extent, ``begin .. end``: this is the published
pipeline wherever a clip's valid frames are a prefix without all-zero gaps, which is how the NTU data tools write them.
include/tamgcn.h has the arithmetic.  ``batch()`` draws as the published code does -- per sample ``np.random.rand(1)`` then
``np.random.randint(0, valid - L + 1)`` for a two-element interval, then ``torch.zeros(3).uniform_(-theta, theta)`` for the
rotation -- and ``batch_device()`` on the device; ``last_draws`` then holds ``crop`` int32 (B, 2) = (start, L), ``drawn`` fp64
(B, 4) = (p, a_x, a_y, a_z) and ``rot`` fp32 (B, 3, 3) or None.
"""
import pickle
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import ops

MAX_MOVE_TIME = 8


def default_candidates():
    """(angles in degrees, scales, translations) of the reference's random_move (tools.py:72-74)."""
    angles = [float(a) for a in range(-175, 185, 5) if abs(a) not in (105, 110)]
    return angles, [k / 10 for k in (9, 10, 11)], [k / 10 for k in range(-2, 3)]


def node_table(W, move_time):
    """The frames at which random_move draws (tools.py:79-80): arange(0, W, W / move_time) rounded half to even, W appended."""
    return np.append(np.arange(0, W, W * 1.0 / move_time).round().astype(int), W).astype(np.int32)


def make_plan(begin, end, T, W, bias, d):
    """(src0, lo, hi) of a slot whose clip has extent (begin, end), shifted to ``bias`` and windowed at ``d``."""
    return d - bias + begin, max(0, bias - d), min(W, bias + (end - begin) - d)


def crop_of(valid, p):
    """(bias, L) of the centre crop of share ``p`` out of ``valid`` frames (CTR-GCN feeders/tools.py valid_crop_resize, the
    one-element p_interval), kept to L >= 1."""
    bias = min(int((1.0 - p) * valid / 2), (valid - 1) // 2)
    return bias, valid - 2 * bias


def rot_matrix(angles):
    """R = (Rz(a_z) . Ry(a_y)) . Rx(a_x) of CTR-GCN's random_rot for angles = (a_x, a_y, a_z) in radians: fp64, every entry of a
    product summed over k = 0, 1, 2 left to right (what the draw kernel does), rounded to fp32 once."""
    ax, ay, az = (np.float64(a) for a in angles)
    one, zero = np.float64(1.0), np.float64(0.0)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = [[one, zero, zero], [zero, cx, sx], [zero, -sx, cx]]
    ry = [[cy, zero, -sy], [zero, one, zero], [sy, zero, cy]]
    rz = [[cz, sz, zero], [-sz, cz, zero], [zero, zero, one]]

    def mul(a, b):
        return [[a[r][0] * b[0][c] + a[r][1] * b[1][c] + a[r][2] * b[2][c] for c in range(3)] for r in range(3)]
    return np.array(mul(mul(rz, ry), rx), dtype=np.float64).astype(np.float32)


def _candidates(values, default, what):
    v = np.asarray(default if values is None else values, dtype=np.float64)
    if v.ndim != 1 or v.size < 1 or not np.isfinite(v).all():
        raise ValueError(f'Feeder: {what} must be a non-empty list of finite numbers')
    return v


class Feeder(Dataset):
    def __init__(self, data_path, label_path, random_choose=False, random_shift=False, random_move=False, window_size=-1,
                 normalization=False, debug=False, use_mmap=True, split='train', stream='joint', parent=None, move_time=1,
                 angle_candidate=None, scale_candidate=None, transform_candidate=None, data=None, labels=None, device='cuda',
                 seed=0, p_interval=None, min_crop=64, random_rot=False, rot_theta=0.3):
        self.data_path, self.label_path, self.split = data_path, label_path, split
        self.random_choose, self.random_shift, self.random_move = bool(random_choose), bool(random_shift), bool(random_move)
        self.normalization, self.debug, self.use_mmap = normalization, debug, use_mmap
        if isinstance(window_size, bool) or not isinstance(window_size, (int, np.integer)):
            raise ValueError(f'Feeder: window_size = {window_size!r} must be an integer (<= 0: the clips\' own length)')
        self.window_size = int(window_size)
        if isinstance(move_time, bool) or not isinstance(move_time, (int, np.integer)) or not 1 <= move_time <= MAX_MOVE_TIME:
            raise ValueError(f'Feeder: move_time = {move_time!r} must be an integer in 1 .. {MAX_MOVE_TIME}')
        self.move_time = int(move_time)
        if stream not in ops.STREAM_MODES:
            raise ValueError(f'unknown stream {stream!r}')
        self.stream = stream
        da, ds, dt = default_candidates()
        self.angle_candidate = _candidates(angle_candidate, da, 'angle_candidate')
        self.scale_candidate = _candidates(scale_candidate, ds, 'scale_candidate')
        self.transform_candidate = _candidates(transform_candidate, dt, 'transform_candidate')
        self.seed, self.last_draws = self._check_seed(seed, 'seed'), None
        self.flags = ((ops.CLIP_SHIFT if self.random_shift else 0) | (ops.CLIP_CHOOSE if self.random_choose else 0)
                      | (ops.CLIP_MOVE if self.random_move else 0))
        self._check_crop_mode(p_interval, min_crop, random_rot, rot_theta)
        # CapturedEval asks for 'val': a feeder whose batches are a function of the indices alone
        self.train_val = 'train' if self.flags or self.crop_flags else 'val'
        self.device = torch.device(device)
        self.load_data(data, labels)
        N, C, T, V, M = self.data.shape
        if self.random_rot and C != 3:
            raise ValueError(f'Feeder: random_rot maps three channels; the clips have C = {C}')
        self.T, self.W = T, (self.window_size if self.window_size > 0 else T)
        if max(T, self.W) * V * M > 2 ** 30:
            raise ValueError(f'Feeder: a channel plane of {max(T, self.W)} x {V} x {M} elements is above 2^30')
        if self.random_move and C < 2:
            raise ValueError(f'Feeder: random_move maps channels 0 and 1; the clips have C = {C}')
        self.node = node_table(self.W, self.move_time)
        if ops.STREAM_MODES[stream] != 0:
            p = None if parent is None else np.asarray(parent)
            if p is None or p.shape != (V,) or not np.issubdtype(p.dtype, np.integer) or p.min() < 0 or p.max() >= V:
                raise ValueError(f'Feeder: stream {stream!r} needs parent=, {V} integers in 0 .. {V - 1} (the root its own parent)')
            parent = p.astype(np.int32)
        else:
            parent = None
        self._upload(parent)
        if normalization:
            self.get_mean_map()

    def _check_crop_mode(self, p_interval, min_crop, random_rot, rot_theta):
        self.random_rot = bool(random_rot)
        if isinstance(min_crop, bool) or not isinstance(min_crop, (int, np.integer)) or min_crop < 1:
            raise ValueError(f'Feeder: min_crop = {min_crop!r} must be an integer >= 1')
        self.min_crop = int(min_crop)
        if isinstance(rot_theta, bool) or not isinstance(rot_theta, (int, float, np.integer, np.floating)) \
                or not np.isfinite(rot_theta) or rot_theta < 0:
            raise ValueError(f'Feeder: rot_theta = {rot_theta!r} must be a finite number >= 0')
        self.rot_theta = float(rot_theta)
        if p_interval is not None:
            try:
                p = [float(v) for v in p_interval]
            except (TypeError, ValueError):
                p = []
            if len(p) not in (1, 2) or not 0 < p[0] <= p[-1] <= 1:                     # NaN fails the comparison too
                raise ValueError(f'Feeder: p_interval = {p_interval!r} must be one or two numbers, 0 < p0 <= p1 <= 1')
            if self.window_size <= 0:
                raise ValueError('Feeder: p_interval resizes the crop to window_size frames: window_size must be > 0')
            if self.flags:
                raise ValueError('Feeder: p_interval excludes random_shift, random_choose and random_move')
            p_interval = tuple(p)
        elif self.random_rot:
            raise ValueError('Feeder: random_rot needs p_interval (the rotation follows the resize)')
        self.p_interval = p_interval
        self.crop_flags = 0
        if p_interval is not None:
            self.crop_flags = (ops.CLIP_CROP_RANDOM if len(p_interval) == 2 else 0) | (ops.CLIP_ROT if self.random_rot else 0)

    # ---- reference :37-38, and the ST-GCN / CTR-GCN data tools' files ---------------------------------------------------
    def load_data(self, data=None, labels=None):
        if data is None:
            data = np.load(self.data_path, mmap_mode='r' if self.use_mmap else None)
        if labels is None:
            if str(self.label_path).endswith('.npy'):
                names, labels = None, np.load(self.label_path)
            else:
                with open(self.label_path, 'rb') as f:
                    try:
                        names, labels = pickle.load(f)
                    except UnicodeDecodeError:                     # a Python 2 pickle, as the ST-GCN tools wrote them
                        f.seek(0)
                        names, labels = pickle.load(f, encoding='latin1')
        else:
            names = None
        if np.ndim(data) != 5 or 0 in np.shape(data):
            raise ValueError(f'Feeder: data must be a non-empty (N, C, T, V, M) array, got {np.shape(data)}')
        labels = np.asarray(labels)
        if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer) or len(labels) != len(data):
            raise ValueError(f'Feeder: labels must be {len(data)} integers, got {labels.dtype} {labels.shape}')
        if self.debug:
            data, labels, names = data[:100], labels[:100], (None if names is None else names[:100])
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        self.label = [int(v) for v in labels]
        self.sample_name = list(names) if names is not None else [str(i) for i in range(len(self.label))]

    def _upload(self, parent):
        dev = self.device
        self._raw = torch.from_numpy(self.data).to(dev)
        self._labels = torch.tensor(self.label, dtype=torch.int64, device=dev)
        self._extent = ops.clip_extent(self._raw)
        self._extent_cpu = self._extent.cpu().numpy()               # what batch() plans with: copied back once
        self._node = torch.from_numpy(self.node).to(dev)
        self._cand = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                           for v in (self.angle_candidate, self.scale_candidate, self.transform_candidate))
        self._parent = None if parent is None else torch.from_numpy(parent).to(dev)
        self._rng = torch.tensor([self.seed, 0], dtype=torch.int64, device=dev)

    def get_mean_map(self):
        pass                                                        # reference :34-35: empty there too

    def __len__(self):
        return len(self.label)

    # ---- host side of one sample: the reference's RNG consumption, call for call ------------------------------------------
    def _draw(self, index):
        T, W = self.T, self.W
        begin, end, bias, d = 0, T, 0, 0
        if self.random_shift:                                       # tools.py:127
            begin, end = (int(v) for v in self._extent_cpu[index])
            bias = random.randint(0, T - (end - begin))
        if self.random_choose:                                      # tools.py:42, :61
            if T > W:
                d = random.randint(0, T - W)
            elif T < W:
                d = -random.randint(0, W - T)
        elif T > W:
            d = (T - W) // 2
        move = None
        if self.random_move:                                        # tools.py:78, :83-86
            random.choice([self.move_time])
            n = len(self.node)
            move = np.stack([np.random.randint(0, len(c), n) for c in (self.angle_candidate, self.scale_candidate,
                                                                       self.transform_candidate, self.transform_candidate)], axis=1)
        return make_plan(begin, end, T, W, bias, d), (bias, d), move

    def _keys(self, move):
        cand = (self.angle_candidate, self.scale_candidate, self.transform_candidate, self.transform_candidate)
        return np.stack([c[move[..., q]] for q, c in enumerate(cand)], axis=-1)

    def _draw_crop(self, index):
        """(start, L), (p, a_x, a_y, a_z), R | None of one sample in the crop-and-resize mode: the published pipeline's RNG
        consumption, call for call."""
        begin, end = (int(v) for v in self._extent_cpu[index])
        valid = max(end - begin, 1)
        p = self.p_interval[0]
        if len(self.p_interval) == 2:
            p = float(np.random.rand(1)[0] * (self.p_interval[1] - self.p_interval[0]) + self.p_interval[0])
            L = min(max(int(np.floor(valid * p)), self.min_crop), valid)
            bias = int(np.random.randint(0, valid - L + 1))
        else:
            bias, L = crop_of(valid, p)
        ang, rot = (0.0, 0.0, 0.0), None
        if self.random_rot:
            ang = tuple(float(a) for a in torch.zeros(3).uniform_(-self.rot_theta, self.rot_theta))
            rot = rot_matrix(ang)
        return (begin + bias, L), (p,) + ang, rot

    def _batch_crop(self, indices):
        crops, drawn, rots = zip(*(self._draw_crop(i) for i in indices))
        dev = self.device
        crop = torch.tensor(crops, dtype=torch.int32, device=dev)
        rot = torch.from_numpy(np.stack(rots)).to(dev) if self.random_rot else None
        out = ops.clip_resize(self._raw, torch.tensor(indices, dtype=torch.int64, device=dev), crop, self.W, rot)
        self.last_draws = {'crop': crop, 'drawn': torch.tensor(drawn, dtype=torch.float64, device=dev), 'rot': rot}
        return out

    def _finish(self, out):
        return ops.stream_derive(out, self._parent, self.stream) if self._parent is not None else out

    def batch(self, indices):
        """(data (B, C, W, V, M) float32 on the device, labels (B,) int64 on the device, indices): the draws on the host,
        the gather in one launch."""
        indices = [int(i) % len(self.label) for i in indices]
        if not indices:
            raise ValueError('Feeder.batch: no indices')
        dev = self.device
        if self.p_interval is not None:
            out = self._batch_crop(indices)
            return self._finish(out), torch.tensor([self.label[i] for i in indices], dtype=torch.int64, device=dev), indices
        plans, shifts, moves = zip(*(self._draw(i) for i in indices))
        plan = torch.tensor(plans, dtype=torch.int32, device=dev)
        node = keys = move = None
        if self.random_move:
            move = np.stack(moves).astype(np.int32)
            node, keys = self._node, torch.from_numpy(np.ascontiguousarray(self._keys(move))).to(dev)
            move = torch.from_numpy(move).to(dev)
        out = ops.clip_transform(self._raw, torch.tensor(indices, dtype=torch.int64, device=dev), plan, self.W, node, keys)
        self.last_draws = {'plan': plan, 'shift': torch.tensor(shifts, dtype=torch.int32, device=dev), 'move': move}
        lab = torch.tensor([self.label[i] for i in indices], dtype=torch.int64, device=dev)
        return self._finish(out), lab, indices

    # ---- the same batch without the host ------------------------------------------------------------------------------------
    def batch_device(self, indices):
        """(data (B, C, W, V, M) float32, labels (B,) int64), both on the device, for ``indices`` an int64 tensor [B] on the
        device (taken modulo the split's size).  The draws come from the device-resident generator, whose call counter moves
        on by one iff a random flag is set.  Two launches (three with a counter advance, one more for a derived stream) on
        the current stream, no copy from the host, no synchronisation: capturable.  ``last_draws`` keeps what the launch
        drew: ``plan`` int32 (B, 3) = (src0, lo, hi), ``shift`` int32 (B, 2) = (bias, d), ``move`` int32 (B, num_node, 4) =
        indices into the angle, scale, translation and translation candidates (None without random_move).  With p_interval:
        ``crop`` int32 (B, 2) = (start, L), ``drawn`` fp64 (B, 4) = (p, a_x, a_y, a_z), ``rot`` fp32 (B, 3, 3) or None; the
        counter moves on iff the interval has two elements or random_rot is set."""
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int64 and indices.dim() == 1
                and indices.device == self._raw.device and indices.numel() > 0):
            raise ValueError('Feeder.batch_device: indices must be a non-empty 1-D int64 tensor on the feeder\'s device '
                             '(batch() takes host indices)')
        indices = indices.contiguous()
        if self.p_interval is not None:
            crop, drawn, rot, lab = ops.clip_crop_draw(self._extent, indices, self._rng, self.crop_flags, self.p_interval[0],
                                                       self.p_interval[-1], self.min_crop, self.rot_theta, labels=self._labels)
            out = ops.clip_resize(self._raw, indices, crop, self.W, rot)
            self.last_draws = {'crop': crop, 'drawn': drawn, 'rot': rot}
            return self._finish(out), lab
        plan, shift, move, keys, lab = ops.clip_draw(self._extent, indices, self._rng, self.flags, self.T, self.W, len(self.node),
                                                     self._cand if self.random_move else None, labels=self._labels)
        out = ops.clip_transform(self._raw, indices, plan, self.W, self._node if self.random_move else None, keys)
        self.last_draws = {'plan': plan, 'shift': shift, 'move': move}
        return self._finish(out), lab

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
        index = index % len(self.label)
        out, _, _ = self.batch([index])
        return out[0].cpu().numpy(), self.label[index], index

    def top_k(self, score, top_k):
        rank = score.argsort()
        hit_top_k = [l in rank[i, -top_k:] for i, l in enumerate(self.label)]
        return sum(hit_top_k) * 1.0 / len(hit_top_k)
