"""numpy / fp64 restatement of the device dropout (include/tamgcn.h, tamgcn_drop_add_act_fwd; tam_gcn_amd/dropout.py) -- no GPU
code.  Test infrastructure: tests/test_dropout_ref_cpu.py holds it to the distribution it must have and to the existing fp64
teacher, tests/test_gpu_dropout.py holds the kernels, the block, the models and CapturedStep to it.

mask() is the draw, word for word as the header states it (Philox4x32-10 from tests/feeder_draws.py).  The block is
tests/stgcn_block_ref.py's fp64 st_gcn with `z * mask * scale` where the reference has nn.Dropout (models/stgcn.py:77-99), its
teacher loop (ReLU margin) and its bars: the teachers made here are entered into stgcn_block_ref's caches under keys of their
own, so that its judge() / verify() serve them unchanged."""
import numpy as np
import torch
import torch.nn.functional as F

import stgcn_block_ref as R
from cases import COT_SEED, tag_seed
from feeder_draws import philox4x32_10
from oracle import stgcn_oracle as SO
from oracle.ctrgcn_oracle import _bn
from params import fill_state_, make_input
from test_gpu_blocks import _Monitor, MARGIN, MAX_TRIES

MAX_ROW, MAX_SITES = 2 ** 22, 4096
_U64 = 2 ** 64 - 1


def consts(p):
    """(thr, scale): floor(p 2^32) and float32(1 / (1 - p)), both from fp64; the scale as a numpy float32."""
    assert 0.0 < p < 1.0
    return int(np.float64(p) * np.float64(4294967296.0)), np.float32(np.float64(1.0) / (np.float64(1.0) - np.float64(p)))


def mask(seed, call, site, rows, L, p):
    """bool [rows, L]: element i of row r is KEPT iff word (i & 3) of
    Philox4x32-10(key = (seed low, seed high), counter = (call low, call high, r, (site << 20) | (i >> 2))) >= floor(p 2^32)."""
    assert L <= MAX_ROW and 0 <= site < MAX_SITES
    seed, call = int(seed) & _U64, int(call) & _U64
    thr = consts(p)[0]
    G = (L + 3) // 4
    r = np.repeat(np.arange(rows, dtype=np.uint64), G)
    g = np.tile(np.arange(G, dtype=np.uint64), rows)
    zero = np.zeros(rows * G, dtype=np.uint64)
    counter = (zero + np.uint64(call & 0xFFFFFFFF), zero + np.uint64(call >> 32), r, g | np.uint64(site << 20))
    w = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
    keep = np.stack([x >= np.uint64(thr) for x in w], axis=1)             # [rows * G, 4]
    return keep.reshape(rows, 4 * G)[:, :L].copy()


def mask_nctv(seed, call, site, shape, p):
    """The mask of a site tensor (N, C, T, V) as a bool torch tensor of that shape: row n * C + c, position t * V + v."""
    N, C, T, V = shape
    return torch.from_numpy(mask(seed, call, site, N * C, T * V, p).reshape(N, C, T, V))


def nibbles(bits, L):
    """(sign, keep) bool [rows, L] out of a bits array (.., ceil(L / 4)) uint8: low nibble sign, high nibble keep."""
    b = bits.reshape(-1, bits.shape[-1]).astype(np.uint8)
    e = np.arange(4, dtype=np.uint8)
    sign = ((b[:, :, None] >> e) & 1).reshape(b.shape[0], -1)[:, :L].astype(bool)
    keep = ((b[:, :, None] >> (e + 4)) & 1).reshape(b.shape[0], -1)[:, :L].astype(bool)
    return sign, keep


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 st_gcn block with the mask where the reference has nn.Dropout
# ---------------------------------------------------------------------------------------------------------------------
def block_forward(keep, scale):
    """stgcn_block_ref.forward's signature (tail is ignored: this IS the tail form) with z * keep * scale between the second
    BatchNorm and the residual add.  keep: bool (N, Cout, T2, V); scale: the fp32 scale as a float."""
    def fwd(x, sd, Ae, stride, rmode, training, tail=True):
        sd = {'m.' + k: v for k, v in sd.items()}
        if rmode == 'zero':
            res = 0
        elif rmode == 'identity':
            res = x
        else:
            res = _bn(F.conv2d(x, sd['m.residual.0.weight'], sd['m.residual.0.bias'], stride=(stride, 1)), sd, 'm.residual.1', training)
        y = torch.relu(_bn(SO.conv_temporal_graphical(x, sd, 'm.gcn', Ae), sd, 'm.tcn.0', training))
        w = sd['m.tcn.2.weight']
        y = F.conv2d(y, w, sd['m.tcn.2.bias'], stride=(stride, 1), padding=((w.shape[2] - 1) // 2, 0))
        y = _bn(y, sd, 'm.tcn.3', training)
        if rmode == 'zero':
            # a dropped element is relu(+0) = 0 with gradient 0 in every arithmetic: it has no ReLU decision to protect, so the
            # margin monitor (which patches torch.relu) is shown the kept values only in spirit -- y * scale everywhere
            return torch.where(keep, torch.relu(y * scale), torch.zeros((), dtype=y.dtype))
        y = y * keep.to(y.dtype) * scale
        return torch.relu(y + res)
    return fwd


# tag -> (temporal kernel, Cin, Cout, stride, residual, frames T, joints V); N = 2.  The first three are stgcn_block_ref's own
# isolated blocks (V = 20), the last one a 25-joint block on the NTU graph with rows of 175 floats: a row tail of 3.
BLOCK_CASES = {
    'k9 64->64 s1': (9, 64, 64, 1, True, 13, 20),
    'k5 64->128 s2': (5, 64, 128, 2, True, 13, 20),
    'k3 3->64 nores': (3, 3, 64, 1, False, 13, 20),
    'k9 64->64 v25 t7': (9, 64, 64, 1, True, 7, 25),
}
DROP_P, DROP_SEED, DROP_CALL, DROP_SITE = 0.5, 20240611, 5, 3


def _block(tag):
    kt, cin, cout, stride, residual, T, V = BLOCK_CASES[tag]
    if V == R.ISO_V:
        return R.block('isolated', tag)
    from tam_gcn_amd.graph import ntu_rgb_d
    from tam_gcn_amd.models import stgcn as M
    build = lambda: M.st_gcn(cin, cout, (kt, 3), stride, residual=residual)      # noqa: E731
    blk = build()
    fill_state_(blk.state_dict(), seed=tag_seed(tag))
    sd = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in blk.state_dict().items()}
    A = torch.tensor(ntu_rgb_d.Graph(labeling_mode='spatial').A, dtype=torch.float32)
    Ae = (A * (1 + 0.1 * make_input((3, V, V), seed=R.ISO_IMP_SEED))).double()
    x = make_input((R.ISO_N, cin, T, V), R.ISO_X_SEED).double()
    cot = make_input((R.ISO_N, cout, (T - 1) // stride + 1, V), seed=COT_SEED).double()
    return R.Block(tag, sd, Ae, x, cot, stride, R.rmode_of(cin, cout, stride, residual), build)


def out_shape(tag):
    kt, cin, cout, stride, residual, T, V = BLOCK_CASES[tag]
    return (R.ISO_N, cout, (T - 1) // stride + 1, V)


_CACHE = {}


def block_teacher(tag, keep=None, scale=None):
    """(Block, Teacher) of the dropout form of block `tag` in train mode.  keep None: the mask of (DROP_SEED, DROP_CALL, DROP_SITE,
    DROP_P) with its scale; otherwise the given bool mask and scale.  The teacher and its fp32 twin (the bars' ref32) go into
    stgcn_block_ref's caches under the key ('dropout', id, True, True)."""
    ident = (tag, 'drawn' if keep is None else 'given')
    if ident in _CACHE:
        return _CACHE[ident]
    b = _block(tag)
    if keep is None:
        keep, scale = mask_nctv(DROP_SEED, DROP_CALL, DROP_SITE, out_shape(tag), DROP_P), float(consts(DROP_P)[1])
    fwd = block_forward(keep, scale)
    xs = float(b.x.abs().max())
    for t in range(MAX_TRIES):
        x = b.x if t == 0 else b.x + 1e-3 * xs * make_input(tuple(b.x.shape), seed=9000 + tag_seed(b.tag) + t).double()
        with torch.no_grad(), _Monitor() as mon:
            fwd(x, {k: v.detach().clone() for k, v in b.sd.items()}, b.Ae, b.stride, b.rmode, True)
        if mon.relu_min >= MARGIN:
            break
    else:
        raise AssertionError(f'{tag}: no dropout teacher with ReLU margin >= {MARGIN} in {MAX_TRIES} tries')
    key = ('dropout', ident, True, True)
    teacher = R.Teacher((x.detach(),) + R.evaluate(b, x, True, True, fwd=fwd) + (t,))
    teacher.key = key
    r32 = R.Teacher((x.float(),) + R.evaluate(b, x, True, True, torch.float32, fwd=fwd) + (t,))
    r32.key = key
    R._TEACHERS[key], R._REF32[key] = teacher, r32
    _CACHE[ident] = (b, teacher)
    return _CACHE[ident]


# ---------------------------------------------------------------------------------------------------------------------
# the two kernels alone: seeded problems, the fp64 restatement of the forward, the fp32 products and fp64 sums of the backward
# ---------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24
EXCLUDE_CAP = 1e-3
# tag -> ((N, C, T, V), residual: None | 'plain' | 'coef', coefficient source for a, relu)
KERNEL_CASES = {
    'identity L260': ((2, 64, 13, 20), 'plain', True, True),       # L % 4 = 0, 16 lanes per row
    'tail3 L175': ((2, 64, 7, 25), 'coef', True, True),            # a row tail of 3, rows 4-byte aligned only; the conv residual's form
    'short L2': ((3, 5, 1, 2), 'plain', False, True),              # L < 4; 15 rows in a workgroup of 16
    'wide L7500': ((1, 4, 300, 25), 'plain', True, True),          # 1875 steps: the whole workgroup walks one row
    'nores L260': ((2, 64, 13, 20), None, True, True),             # res = NULL: a block built with residual=False
    'plain L256': ((4, 1, 1, 256), None, False, False),            # functional.dropout's form: no source, no residual, no ReLU
}
K_SEED, K_CALL, K_SITE, K_P = 2 ** 40 + 7, 2 ** 33 + 1, 9, 0.5


def _coef(C, seed, x2=False):
    r = np.random.RandomState(seed)
    c = np.zeros((3, C), dtype=np.float32)
    c[0] = (0.5 + r.random_sample(C)) * np.where(r.random_sample(C) < 0.5, -1, 1)
    c[2] = r.random_sample(C) - 0.5
    return torch.from_numpy(c)


def kernel_problem(tag, p=K_P):
    """Seeded O(1) fp32 inputs of one case: a (z, coef | None), res (r, coef | None) | None, dout, the BatchNorm saves, a sign
    pattern for the backward alone, the mask and the constants."""
    shape, res, coef, relu = KERNEL_CASES[tag]
    N, C, T, V = shape
    s = tag_seed(tag)
    thr, scale = consts(p)
    q = dict(tag=tag, shape=shape, relu=relu, p=p, thr=thr, scale=scale, seed=K_SEED, call=K_CALL, site=K_SITE)
    q['z'] = make_input(shape, s + 1)
    q['acoef'] = _coef(C, s + 2) if coef else None
    q['r'] = make_input(shape, s + 3) if res else None
    q['rcoef'] = _coef(C, s + 4) if res == 'coef' else None
    q['dout'] = make_input(shape, s + 5)
    q['a_save'] = make_input((2, C), s + 6, -0.5, 0.5)
    q['r_save'] = make_input((2, C), s + 7, -0.5, 0.5)
    q['sign'] = torch.from_numpy(np.random.RandomState(s + 8).random_sample(shape) < 0.6)
    q['keep'] = mask_nctv(K_SEED, K_CALL, K_SITE, shape, p)
    return q


def _affine(x, coef, dt, absval=False):
    x = x.to(dt)
    if coef is None:
        return x.abs() if absval else x
    c = coef.to(dt)
    if absval:
        return c[0].abs()[None, :, None, None] * x.abs() + c[2].abs()[None, :, None, None]
    return c[0][None, :, None, None] * x + c[2][None, :, None, None]


def fwd_ref(q):
    """(out64, bar, pre64): out = act(keep * a * scale + res) in fp64 on the fp32 inputs and the fp32 scale; the element-wise
    bar of a correct fp32 evaluation: the fma of a (on |a|), the product with the scale (both scaled: 2 eps |a| scale), the
    residual's own fma and the add (2 eps on |a scale| + |res|) -- three roundings on |a scale| and |a scale + res|, the bound
    taken on magnitudes: 3 eps (|a| scale + |res|)."""
    F64 = torch.float64
    sc = float(q['scale'])
    a, am = _affine(q['z'], q['acoef'], F64), _affine(q['z'], q['acoef'], F64, True)
    pre = torch.where(q['keep'], a * sc, torch.zeros((), dtype=F64))
    mag = torch.where(q['keep'], am * sc, torch.zeros((), dtype=F64))
    if q['r'] is not None:
        pre = pre + _affine(q['r'], q['rcoef'], F64)
        mag = mag + _affine(q['r'], q['rcoef'], F64, True)
    out = torch.relu(pre) if q['relu'] else pre
    return out, 3 * EPS32 * mag, pre


def pack_bits(sign, keep):
    """uint8 (N, C, ceil(L / 4)) of bool (N, C, T, V) sign and keep: low nibble sign, high nibble keep"""
    N, C = sign.shape[:2]
    L = sign[0, 0].numel()
    G = (L + 3) // 4
    out = np.zeros((N, C, G * 4), dtype=np.uint8)
    out[:, :, :L] = sign.reshape(N, C, L).numpy().astype(np.uint8) | (keep.reshape(N, C, L).numpy().astype(np.uint8) << 4)
    out = out.reshape(N, C, G, 4)
    return torch.from_numpy((out[..., 0] | (out[..., 1] << 1) | (out[..., 2] << 2) | (out[..., 3] << 3)).astype(np.uint8))


def bwd_ref(q, with_a=True, with_r=True):
    """d, dza as the fp32 values the kernel must deliver bit for bit, and the Bars (tests/ew_ref.py's conventions, add_act_bwd's
    sums) of part: s0, s1 over dza against a_pre = z (one rounding in the element: k = 1), s2, s3 over d against r_pre = r."""
    import ew_ref as E
    F64 = torch.float64
    d32 = torch.where(q['sign'], q['dout'], torch.zeros(())) if q['relu'] else q['dout'].clone()
    za32 = torch.where(q['keep'], torch.from_numpy(d32.numpy() * np.float32(q['scale'])), torch.zeros(()))
    sc = float(q['scale'])
    d64 = d32.to(F64)
    za64 = torch.where(q['keep'], d64 * sc, torch.zeros((), dtype=F64))
    dm = q['dout'].to(F64).abs()
    bars = {}
    if with_a:
        bars['s0'], bars['s1'] = E._moment(za64, dm * sc, q['z'], q['a_save'][0], 1, F64)
    if with_r and q['r'] is not None:
        bars['s2'], bars['s3'] = E._moment(d64, dm, q['r'], q['r_save'][0], 0, F64)
    return d32, za32, bars
