"""numpy restatement of the RGB feeder (include/tamgcn_rgb.h, tam_gcn_amd/feeder/rgb_feeder.py): Pillow's 8-bit bilinear
resample as tables and two integer passes, the normalisation table lookup, tiling, flip, the two missing modes, row_scale and the
Philox flip draws.  Test infrastructure: tests/test_rgb_feeder_ref_cpu.py holds it to Pillow byte for byte and to the recorded
fixture, tests/test_gpu_rgb_feeder.py holds the kernels to it bit for bit."""
import math

import numpy as np

from feeder_draws import philox4x32_10

BITS = 22
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (H, W, S): the shapes the restatement was checked on against Pillow
PIL_SHAPES = [(37, 53, 16), (480, 640, 224), (60, 80, 224), (224, 300, 224), (100, 224, 224), (7, 9, 24), (500, 333, 224), (225, 223, 224),
              (24, 24, 24)]


def tables(n_in, n_out):
    """coef int32 (n_out, K), bounds int32 (n_out, 2) = (first tap, tap count); everything in Python floats."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    K = int(math.ceil(support)) * 2 + 1
    coef, bounds = np.zeros((n_out, K), dtype=np.int32), np.zeros((n_out, 2), dtype=np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = []
        for j in range(hi - lo):
            a = abs((j + lo - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        tot = 0.0
        for v in w:
            tot += v
        for j, v in enumerate(w):
            coef[o, j] = int(0.5 + v / tot * (1 << BITS))
        bounds[o] = (lo, hi - lo)
    return coef, bounds


def resample_axis(x, axis, coef, bounds):
    """One pass over `axis` of a uint8 array: clip((2^21 + sum c * in) >> 22, 0, 255), int64 sums (they stay below 2^31)."""
    x = np.moveaxis(np.asarray(x), axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + x.shape[1:], dtype=np.int64)
    for o, (lo, n) in enumerate(bounds):
        c = coef[o, :n].astype(np.int64).reshape((n,) + (1,) * (x.ndim - 1))
        acc = (1 << (BITS - 1)) + (c * x[lo:lo + n]).sum(axis=0)
        assert acc.max() < 2 ** 31 and acc.min() >= 0
        out[o] = acc >> BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img, S, tables_h=None, tables_v=None):
    """uint8 (..., H, W, 3) -> (..., S, S, 3): horizontal pass first, rounded to uint8, vertical second; a pass between equal
    sizes is skipped."""
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape[-3], img.shape[-2]
    if W != S or tables_h is not None:
        img = resample_axis(img, img.ndim - 2, *(tables_h or tables(W, S)))
    if H != S or tables_v is not None:
        img = resample_axis(img, img.ndim - 3, *(tables_v or tables(H, S)))
    return img


def lut(mean=MEAN, std=STD):
    """fp32 (3, 256) in numpy: byte / 255, minus mean, over std, every step rounded to fp32 (IEEE: what torch's fp32 kernels give)."""
    x = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.stack([(x - np.float32(m)) / np.float32(s) for m, s in zip(mean, std)]).astype(np.float32)


def batch(store, ids, table, F=1, flip=None, missing=None, missing_mode=0, row_scale=None):
    """out fp32 (B, 3 F, S, S); store uint8 (n, S, S, 3); ids any integers, taken modulo n."""
    n, S = store.shape[0], store.shape[1]
    out = np.zeros((len(ids), 3 * F, S, S), dtype=np.float32)
    for b, i in enumerate(ids):
        i = int(i) % n
        gone = missing is not None and bool(missing[i])
        px = np.zeros((S, S, 3), dtype=np.uint8) if gone else store[i]
        if flip is not None and flip[b]:
            px = px[:, ::-1]
        v = np.stack([table[c][px[:, :, c]] for c in range(3)])                    # (3, S, S)
        if row_scale is not None:
            v = (v * np.asarray(row_scale[b], dtype=np.float32)[None, :, None]).astype(np.float32)
        if gone and missing_mode == 0:
            v = np.zeros_like(v)
        out[b] = np.tile(v, (F, 1, 1))
    return out


def flips(seed, call, B):
    """int32 [B]: slot b flips iff word 0 of philox4x32_10((call_lo, call_hi, b, 0), key (seed_lo, seed_hi)) < 2^31."""
    slot, zero = np.arange(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    counter = (zero + np.uint64(call & 0xFFFFFFFF), zero + np.uint64((call >> 32) & 0xFFFFFFFF), slot, zero)
    w = philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (w[0] < np.uint64(1 << 31)).astype(np.int32)


def smooth_images(seed, n, H, W):
    """Smooth synthetic uint8 (n, H, W, 3): a few low-frequency waves per channel (they compress, and exercise every byte range)."""
    r = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        for c in range(3):
            fy, fx, ph = r.uniform(0.5, 3.0) / H, r.uniform(0.5, 3.0) / W, r.uniform(0, 2 * np.pi)
            v = 127.5 + 140.0 * np.sin(2 * np.pi * (fy * y + fx * x) + ph) * np.cos(2 * np.pi * fx * x * 0.5)
            out[i, :, :, c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out
