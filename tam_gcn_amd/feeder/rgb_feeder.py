"""Device-resident feeder of the RGB modality.  It restates the reference's RGB path, ``feeder/tools.py:216-246``
(``load_rgb_images``, what the fusion feeder calls) and ``feeder/feeder_nucla_resnet.py:24-35, :50-64`` (the ResNet feeder):

  1. ``Resize((size, size))``: PIL's bilinear filter on 8-bit pixels, which is integer arithmetic on fixed-point coefficients
     (``pil_bilinear_tables``; include/tamgcn_rgb.h has the formula) -- horizontal pass first, rounded to uint8, vertical second;
  2. ``ToTensor`` + ``Normalize(mean, std)``: a function of (channel, byte), so a table of 3 x 256 floats that torch fills on
     the host with the reference's own operations (``normalise_table``);
  3. ``temporal_rgb_frames`` copies along the channel axis (tools.py:236-238; 5 copies give 15 channels);
  4. on the ResNet feeder's train path a left-right flip with probability 1/2 (feeder_nucla_resnet.py:61-62), before the resize
     there and after it here: the two are the same bytes iff the horizontal table is mirror symmetric
     (``tables_mirror_symmetric``), which the constructor checks for every source width;
  5. a missing or unreadable file: float zeros in the fusion feeder (tools.py:246, ``missing_as='zeros'``), a black image that is
     then normalised in the ResNet feeder (feeder_nucla_resnet.py:59-60, ``missing_as='black'``).

Decoding stays on the host and happens once (``load_images``).  The deterministic step 1 runs once per split, at construction
(``tamgcn_rgb_resize``), into a uint8 store ``(n, size, size, 3)`` in HBM: 1020 images at 224 x 224 are 154 MB.  A batch is one
launch (``tamgcn_rgb_batch``) that reads 3 bytes per pixel and writes ``3 * temporal_rgb_frames`` floats per pixel.  Every step is
bit for bit the reference's: there is no tolerance anywhere.

``batch(indices)`` draws the flips on the host, ``np.random.random() < 0.5`` per sample in order.  ``batch_device(indices)`` takes
int64 indices on the device and draws there (``tamgcn_rgb_draw``: Philox4x32-10 keyed by ``seed``, counted by a call counter on
the device): no copy from the host, no synchronisation, capturable -- ``GraphedBatch`` takes this feeder unmodified.
``FusionFeeder`` pairs it with a skeleton feeder for ``crossmodal.ResNet_GCN_Attention``.
"""
import math
import os

import numpy as np
import torch

from .. import _rgb_lib, ops

PRECISION_BITS = 22                 # Pillow's fixed point for 8-bit pixels: 32 - 8 - 2
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MISSING_MODES = {'zeros': 0, 'black': 1}
_CHUNK_BYTES = 256 << 20            # source images uploaded and resized per call, at construction


def pil_bilinear_tables(n_in, n_out):
    """(coef int32 (n_out, K), bounds int32 (n_out, 2) = (first tap, tap count)) of Pillow's bilinear resample of one axis from
    n_in to n_out 8-bit samples, in Python floats (fp64) and Pillow's operation order."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f'pil_bilinear_tables: sizes {n_in} -> {n_out} must be >= 1')
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs                                        # bilinear: support 1.0, times the filter scale
    ss = 1.0 / fs
    K = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((n_out, K), dtype=np.int32)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        n = hi - lo
        w = []
        for j in range(n):
            a = abs((j + lo - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for j in range(n):
            v = w[j] / ww if ww != 0.0 else w[j]
            coef[o, j] = int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS))
        bounds[o] = (lo, n)
    return coef, bounds


def dense_table(coef, bounds, n_in):
    """The (n_out, n_in) int64 matrix the tables stand for."""
    n_out = len(bounds)
    D = np.zeros((n_out, n_in), dtype=np.int64)
    for o in range(n_out):
        lo, n = (int(v) for v in bounds[o])
        D[o, lo:lo + n] = coef[o, :n]
    return D


def tables_mirror_symmetric(coef, bounds, n_in):
    """True iff the resample commutes with reversing the axis: the dense matrix equals itself reversed on both axes.  A flip
    after the resize equals the reference's flip before it iff this holds for the horizontal table."""
    D = dense_table(coef, bounds, n_in)
    return bool(np.array_equal(D, D[::-1, ::-1]))


def normalise_table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """fp32 (3, 256): ToTensor (byte / 255 in fp32) then Normalize (sub mean, div std, both fp32 tensors), in torch on the host
    with the reference's operations in their order."""
    mean, std = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    if mean.shape != (3,) or std.shape != (3,) or not bool((std != 0).all()):
        raise ValueError('normalise_table: mean and std are three numbers each, std non-zero')
    x = torch.arange(256, dtype=torch.float32).div(255)
    return torch.stack([x.clone().sub_(mean[c]).div_(std[c]) for c in range(3)]).contiguous()


def load_images(rgb_root, names):
    """(list of uint8 (H, W, 3) arrays, missing bool [n]) for ``names`` under ``rgb_root``: name + '.png', else '.jpg', then
    ``convert('RGB')`` (tools.py:225-233).  An absent or unreadable file is flagged missing and stands as a 1 x 1 black image, as
    the reference's ``except`` replaces it.  Host only; needs PIL."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError('rgb_feeder.load_images decodes with PIL (Pillow), which is not installed; decode the images '
                          'elsewhere and give RGBFeeder uint8 (H, W, 3) arrays') from e
    images, missing = [], np.zeros(len(names), dtype=bool)
    for i, name in enumerate(names):
        path = os.path.join(rgb_root, name + '.png')
        if not os.path.exists(path):
            path = os.path.join(rgb_root, name + '.jpg')
        try:
            with Image.open(path) as im:
                images.append(np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8)))
        except Exception:                                   # noqa: BLE001  -- the reference's `except Exception`, tools.py:244
            images.append(np.zeros((1, 1, 3), dtype=np.uint8))
            missing[i] = True
    return images, missing


def _lib():
    return _rgb_lib.load()


def resize(src, size, tables_h=None, tables_v=None):
    """src uint8 (n, H0, W0, 3) on the device -> uint8 (n, Ho, Wo, 3), PIL's bilinear resample (tamgcn_rgb_resize).  size =
    (Ho, Wo); the tables default to pil_bilinear_tables of the two axes and a pass between equal sizes is skipped."""
    ops._want(src, 'src', torch.uint8)
    if src.dim() != 4 or src.shape[3] != 3 or src.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: resize takes a non-empty uint8 (n, H0, W0, 3), got {tuple(src.shape)}')
    n, H0, W0, _ = src.shape
    Ho, Wo = (int(v) for v in size)
    dev = src.device

    def up(tables, n_in, n_out):
        if tables is None:
            if n_in == n_out:
                return None, None, 0
            tables = pil_bilinear_tables(n_in, n_out)
        coef, bounds = (np.ascontiguousarray(t, dtype=np.int32) for t in tables)
        if coef.ndim != 2 or coef.shape[0] != n_out or bounds.shape != (n_out, 2):
            raise RuntimeError(f'tam_gcn_amd: resize tables are {coef.shape} and {bounds.shape}, expected ({n_out}, K) and ({n_out}, 2)')
        return torch.from_numpy(coef).to(dev), torch.from_numpy(bounds).to(dev), coef.shape[1]
    ch, bh, Kh = up(tables_h, W0, Wo)
    cv, bv, Kv = up(tables_v, H0, Ho)
    tmp = torch.empty(n, H0, Wo, 3, dtype=torch.uint8, device=dev) if ch is not None and cv is not None else None
    dst = torch.empty(n, Ho, Wo, 3, dtype=torch.uint8, device=dev)
    p = ops._ptr
    _rgb_lib.check(_lib().tamgcn_rgb_resize(p(src), n, H0, W0, Ho, Wo, p(ch), p(bh), Kh, p(cv), p(bv), Kv, p(tmp), p(dst), ops._stream()),
                   'tamgcn_rgb_resize')
    return dst


def draw(state, B):
    """flip int32 [B] of call state[1] under seed state[0] (tamgcn_rgb_draw); state int64 [2] on the device moves on by one."""
    ops._want(state, 'state', torch.int64, (2,))
    flip = torch.empty(B, dtype=torch.int32, device=state.device)
    _rgb_lib.check(_lib().tamgcn_rgb_draw(ops._ptr(state), B, ops._ptr(flip), ops._stream()), 'tamgcn_rgb_draw')
    return flip


def batch(store, ids, lut, F=1, flip=None, missing=None, missing_mode=0, row_scale=None, labels=None):
    """out fp32 (B, 3 F, S, S) from store uint8 (n, S, S, 3) (tamgcn_rgb_batch, include/tamgcn_rgb.h), and labels[ids] when
    labels int64 [n] is given (else None)."""
    ops._want(store, 'store', torch.uint8)
    if store.dim() != 4 or store.shape[1] != store.shape[2] or store.shape[3] != 3 or store.numel() == 0:
        raise RuntimeError(f'tam_gcn_amd: batch takes a non-empty uint8 store (n, S, S, 3), got {tuple(store.shape)}')
    n, S = store.shape[0], store.shape[1]
    ops._want(ids, 'ids', torch.int64)
    if ids.dim() != 1 or ids.numel() == 0:
        raise RuntimeError('tam_gcn_amd: batch takes non-empty 1-D ids')
    B, F = ids.numel(), int(F)
    ops._want(lut, 'lut', torch.float32, (3, 256))
    if flip is not None:
        ops._want(flip, 'flip', torch.int32, (B,))
    if missing is not None:
        ops._want(missing, 'missing', torch.uint8, (n,))
    if row_scale is not None:
        ops._want(row_scale, 'row_scale', torch.float32, (B, S))
    lab = None
    if labels is not None:
        ops._want(labels, 'labels', torch.int64, (n,))
        lab = torch.empty(B, dtype=torch.int64, device=store.device)
    if F < 1:
        raise RuntimeError(f'tam_gcn_amd: batch: F = {F}')
    out = torch.empty(B, 3 * F, S, S, dtype=torch.float32, device=store.device)
    p = ops._ptr
    _rgb_lib.check(_lib().tamgcn_rgb_batch(p(store), n, S, p(ids), B, p(lut), p(flip), p(missing), int(missing_mode), p(row_scale), F,
                                           p(labels), p(lab), p(out), ops._stream()), 'tamgcn_rgb_batch')
    return out, lab


class RGBFeeder:
    """``images``: one uint8 array (n, H0, W0, 3) or a list of (H, W, 3) arrays of differing sizes (``load_images`` gives one);
    ``labels``: n integers.  ``missing``: bool [n] or None.  The flip is drawn only when ``train and random_flip``;
    ``random_crop`` is accepted and does nothing, as in the reference (feeder_nucla_resnet.py:11: never read)."""

    def __init__(self, images, labels, size=224, temporal_rgb_frames=1, random_flip=False, random_crop=False, train=True,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, missing=None, missing_as='black', seed=0, device='cuda'):
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
            raise ValueError(f'RGBFeeder: size = {size!r} must be an integer >= 1')
        if isinstance(temporal_rgb_frames, bool) or not isinstance(temporal_rgb_frames, (int, np.integer)) or temporal_rgb_frames < 1:
            raise ValueError(f'RGBFeeder: temporal_rgb_frames = {temporal_rgb_frames!r} must be an integer >= 1')
        if missing_as not in MISSING_MODES:
            raise ValueError(f'RGBFeeder: missing_as = {missing_as!r} must be one of {sorted(MISSING_MODES)}')
        self.size, self.temporal_rgb_frames = int(size), int(temporal_rgb_frames)
        self.random_flip, self.random_crop, self.train = bool(random_flip), random_crop, bool(train)
        self.missing_as, self.missing_mode = missing_as, MISSING_MODES[missing_as]
        self.draws_flip = self.train and self.random_flip
        self.train_val = 'train' if self.draws_flip else 'val'   # 'val': a batch is a function of the indices alone
        self.seed, self.last_draws = self._check_seed(seed, 'seed'), None
        self.device = torch.device(device)
        images = [images[i] for i in range(len(images))]
        n = len(images)
        if n == 0:
            raise ValueError('RGBFeeder: no images')
        for i, im in enumerate(images):
            if not (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.size > 0):
                raise ValueError(f'RGBFeeder: image {i} must be a non-empty uint8 (H, W, 3) array, got '
                                 f'{getattr(im, "dtype", type(im))} {getattr(im, "shape", "")}')
        labels = np.asarray(labels)
        if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer) or len(labels) != n:
            raise ValueError(f'RGBFeeder: labels must be {n} integers, got {labels.dtype} {labels.shape}')
        self.label = [int(v) for v in labels]
        miss = np.zeros(n, dtype=bool) if missing is None else np.asarray(missing)
        if miss.shape != (n,) or miss.dtype != np.bool_:
            raise ValueError(f'RGBFeeder: missing must be {n} booleans, got {miss.dtype} {miss.shape}')
        self.missing = miss
        groups = {}
        for i, im in enumerate(images):
            if not miss[i]:
                groups.setdefault(im.shape[:2], []).append(i)
        if self.draws_flip:
            bad = sorted({W0 for (_, W0) in groups if W0 != self.size and not tables_mirror_symmetric(*pil_bilinear_tables(W0, self.size), W0)})
            if bad:
                raise ValueError(f'RGBFeeder: random_flip flips after the resize, which equals the reference\'s flip before it only for a '
                                 f'mirror-symmetric table; the tables of source widths {bad} -> {self.size} are not')
        self.lut = normalise_table(mean, std)
        self._upload(images, groups)

    def _upload(self, images, groups):
        dev, S = self.device, self.size
        self._raw = torch.zeros(len(images), S, S, 3, dtype=torch.uint8, device=dev)       # a missing image's rows are never read
        for (H0, W0), members in groups.items():
            th = None if W0 == S else pil_bilinear_tables(W0, S)
            tv = None if H0 == S else pil_bilinear_tables(H0, S)
            step = max(1, _CHUNK_BYTES // (H0 * W0 * 3))
            for k in range(0, len(members), step):
                part = members[k:k + step]
                src = torch.from_numpy(np.stack([images[i] for i in part])).to(dev)
                self._raw.index_copy_(0, torch.tensor(part, dtype=torch.int64, device=dev), resize(src, (S, S), th, tv))
                del src
        self._labels = torch.tensor(self.label, dtype=torch.int64, device=dev)
        self._lut = self.lut.to(dev)
        self._missing = torch.from_numpy(self.missing.astype(np.uint8)).to(dev) if self.missing.any() else None
        self._rng = torch.tensor([self.seed, 0], dtype=torch.int64, device=dev)

    def __len__(self):
        return len(self.label)

    def _make(self, ids, flip, row_scale):
        if row_scale is not None and flip is not None:
            raise ValueError('RGBFeeder: row_scale with a drawn flip is refused (the weights belong to the unflipped image\'s rows '
                             'and columns; construct the feeder with random_flip=False)')
        out, lab = batch(self._raw, ids, self._lut, self.temporal_rgb_frames, flip, self._missing, self.missing_mode, row_scale, self._labels)
        self.last_draws = {'flip': flip}
        return out, lab

    def batch(self, indices):
        """(x_rgb (B, 3 F, size, size) float32, labels (B,) int64, both on the device, indices): the flips drawn on the host,
        ``np.random.random() < 0.5`` per sample in order (feeder_nucla_resnet.py:61)."""
        indices = [int(i) % len(self.label) for i in indices]
        if not indices:
            raise ValueError('RGBFeeder.batch: no indices')
        flip = None
        if self.draws_flip:
            flip = torch.tensor([1 if np.random.random() < 0.5 else 0 for _ in indices], dtype=torch.int32, device=self.device)
        out, lab = self._make(torch.tensor(indices, dtype=torch.int64, device=self.device), flip, None)
        return out, lab, indices

    def batch_device(self, indices, row_scale=None):
        """(x_rgb (B, 3 F, size, size) float32, labels (B,) int64), both on the device, for ``indices`` an int64 tensor [B] on the
        device (taken modulo the split's size).  With ``train and random_flip`` the flips come from the device-resident
        generator, whose call counter then moves on by one (three launches); otherwise nothing is drawn (one launch).  No copy
        from the host, no synchronisation: capturable.  ``row_scale`` fp32 (B, size) multiplies row y of slot b, e.g.
        ``SkeletonGuidance.weight_map(x, (size, size))[:, 0, :, 0]``.  ``last_draws = {'flip': int32 [B] | None}``."""
        if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int64 and indices.dim() == 1
                and indices.device == self._raw.device and indices.numel() > 0):
            raise ValueError('RGBFeeder.batch_device: indices must be a non-empty 1-D int64 tensor on the feeder\'s device '
                             '(batch() takes host indices)')
        if row_scale is not None:
            if self.draws_flip:
                raise ValueError('RGBFeeder.batch_device: row_scale with a drawn flip is refused (construct the feeder with random_flip=False)')
            if not (isinstance(row_scale, torch.Tensor) and row_scale.dtype == torch.float32 and row_scale.device == self._raw.device
                    and tuple(row_scale.shape) == (indices.numel(), self.size)):
                raise ValueError(f'RGBFeeder.batch_device: row_scale must be fp32 ({indices.numel()}, {self.size}) on the feeder\'s device')
            row_scale = row_scale.contiguous()
        indices = indices.contiguous()
        flip = draw(self._rng, indices.numel()) if self.draws_flip else None
        return self._make(indices, flip, row_scale)

    @staticmethod
    def _check_seed(v, what):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 63:
            raise ValueError(f'RGBFeeder: {what} = {v!r} must be an integer in [0, 2^63)')
        return v

    def manual_seed(self, seed, call=0):
        """Write (seed, call) into the device-resident generator state on the current stream.  Graphs captured earlier read the
        state on every replay, so this takes effect on them too."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('RGBFeeder.manual_seed: set the seed outside graph capture (a captured write would replay the value '
                               'of capture time)')
        self.seed = self._check_seed(seed, 'seed')
        self._rng.copy_(torch.tensor([self.seed, self._check_seed(call, 'call')], dtype=torch.int64))

    def rng_state(self):
        """(seed, call): the next drawing batch_device() call draws call number ``call`` (reads the device: a host sync)."""
        seed, call = self._rng.tolist()
        return seed, call

    def set_rng_state(self, state):
        seed, call = state
        self.manual_seed(int(seed), int(call))

    def __getitem__(self, index):
        index = index % len(self.label)
        out, _, _ = self.batch([index])
        return out[0].cpu().numpy(), self.label[index], index


class FusionFeeder:
    """The reference's fusion batch ``[data_numpy, data_rgb], label`` (feeder_nucla_fusion.py:113) from a skeleton feeder
    (feeder_nucla_gcn.Feeder or clip_feeder.Feeder) and an RGBFeeder over the same samples: ``batch`` and ``batch_device`` return
    ``((x_gcn, x_rgb), y)``.  The two generator states move into one int64 [4] tensor, ``_rng`` = (skeleton seed, call, RGB seed,
    call), of which the two feeders hold views from then on: ``GraphedBatch(fusion, B)`` saves and restores both with it.
    Construct it before capturing either feeder.  The skeleton half is what the skeleton feeder alone gives from the same state."""

    def __init__(self, skeleton_feeder, rgb_feeder):
        if not isinstance(rgb_feeder, RGBFeeder):
            raise TypeError(f'FusionFeeder: rgb_feeder is a {type(rgb_feeder).__name__}, not an RGBFeeder')
        for a in ('batch', 'batch_device', '_rng', '_raw', 'label'):
            if not hasattr(skeleton_feeder, a):
                raise TypeError(f'FusionFeeder: {type(skeleton_feeder).__name__} has no {a} (a device-resident skeleton feeder is needed)')
        if len(skeleton_feeder) != len(rgb_feeder):
            raise ValueError(f'FusionFeeder: {len(skeleton_feeder)} skeleton samples, {len(rgb_feeder)} images')
        if [int(v) for v in skeleton_feeder.label] != rgb_feeder.label:
            raise ValueError('FusionFeeder: the two feeders\' labels differ')
        if skeleton_feeder._raw.device != rgb_feeder._raw.device:
            raise ValueError(f'FusionFeeder: the feeders are on {skeleton_feeder._raw.device} and {rgb_feeder._raw.device}')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusionFeeder: construct it outside graph capture')
        self.skeleton, self.rgb = skeleton_feeder, rgb_feeder
        self.label = rgb_feeder.label
        self._raw = skeleton_feeder._raw
        self._rng = torch.cat([skeleton_feeder._rng, rgb_feeder._rng])
        skeleton_feeder._rng, rgb_feeder._rng = self._rng[0:2], self._rng[2:4]
        self.train_val = 'val' if (getattr(skeleton_feeder, 'train_val', 'train') == 'val' and rgb_feeder.train_val == 'val') else 'train'
        self.last_draws = None

    def __len__(self):
        return len(self.label)

    def batch(self, indices):
        """((x_gcn, x_rgb), labels): the draws on the host, the skeleton's first, as feeder_nucla_fusion.py:95-111 orders them."""
        indices = [int(i) for i in indices]
        x, y, _ = self.skeleton.batch(indices)
        r, _, _ = self.rgb.batch(indices)
        self.last_draws = {'skeleton': self.skeleton.last_draws, 'rgb': self.rgb.last_draws}
        return (x, r), y

    def batch_device(self, indices):
        """((x_gcn, x_rgb), labels) for int64 indices on the device: the two feeders' batch_device on the current stream, no copy
        from the host, no synchronisation, capturable."""
        x, y = self.skeleton.batch_device(indices)
        r, _ = self.rgb.batch_device(indices)
        self.last_draws = {'skeleton': self.skeleton.last_draws, 'rgb': self.rgb.last_draws}
        return (x, r), y

    def manual_seed(self, seed, call=0):
        """Seed both generators: the skeleton's with ``seed``, the RGB feeder's with ``seed + 1`` (two streams, not one twice)."""
        self.skeleton.manual_seed(seed, call)
        self.rgb.manual_seed((seed + 1) % 2 ** 63, call)

    def rng_state(self):
        return tuple(self._rng.tolist())

    def set_rng_state(self, state):
        s0, c0, s1, c1 = (int(v) for v in state)
        self.skeleton.manual_seed(s0, c0)
        self.rgb.manual_seed(s1, c1)
