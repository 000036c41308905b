"""-m gpu: the ledger of the GEMM-family kernel forms of csrc/conv.hip.  Every case is one tamgcn_conv / tamgcn_wgrad /
reduction descriptor, the kernel symbol the host dispatch must pick for it (tamgcn_last_kernel), and an fp64 reference the
result is held to at fp32-rounding bars (tests/fp64_bars.py).  Operands are channel slices of wider tensors, outputs land
in channel / frame windows of wider tensors whose other elements must come back bit-identical.

tests/test_gemm_ledger.py (CPU) checks that every instantiation conv.hip dispatches to is pinned here, pinned by another
test (ELSEWHERE) or listed in UNREACHABLE with the planner condition that excludes it."""
import ctypes as C

import pytest
import torch

import fp64_bars as B

GLDS8 = 'conv1x1_glds_kernel<{}, {}, {}, 8>'
G_PLAIN, G_PRO, G_TWO = GLDS8.format(1, 16, 'false'), GLDS8.format(1, 16, 'true'), GLDS8.format(2, 8, 'true')
G_SPLIT = 'conv1x1_glds_split_kernel<2, false, 4>'


def vec(bk, mt, cw):
    return f'conv_kernel_vec<{bk}, {mt}, {cw}>'


def conv(cid, sym, N, K, M, T, V, **kw):
    """sym: the symbol in both split modes, or {mode: symbol}.  kw: KT dil stride pad up wmode T_out ostride ty (extra output
    frames) src ('plain' | 'coef' | 'relu' | 'two') kx (extra source channels in front) ycoff yx (extra output channels
    behind) bias add1 ('y': the output itself) add2 bcast mask aux stats post (None | post_act)."""
    return cid, dict(kind='conv', sym=sym, N=N, K=K, M=M, T=T, V=V, **kw)


def wg(cid, sym, N, M, K, T, V, **kw):
    """sym: {mode: symbol} (LDS-DMA kernel) or one symbol (register-staged, exact in both modes).  kw: KT dil stride pad
    gy ('coef' | 'two') x ('relu' | 'two') empty (the case's nsplit leaves the last split without work)."""
    return cid, dict(kind='wgrad', sym=sym, N=N, M=M, K=K, T=T, V=V, **kw)


def wglds(wmt, wkt, ny, nx, nst, taps=False):
    t = ' taps' if taps else ''
    return {0: f'wgrad_glds_kernel<{wmt}, {wkt}, {ny}, {nx}, f32, {nst[0]}>{t}',
            1: f'wgrad_glds_kernel<{wmt}, {wkt}, {ny}, {nx}, split, {nst[1]}>{t}'}


def wreg(kt, wmt, wkt, v, ps=False):
    return f'wgrad_kernel<{kt}, {wmt}, {wkt}, {"true" if v else "false"}{", p-split" if ps else ""}>'


CASES = dict([
    # ---- 1x1 LDS-DMA GEMM, eight waves (TG_GLDS_CASE(*, *, *, 8)); its four-wave form: ELSEWHERE
    conv('glds_plain_bias_adds_bcast_ty', G_PLAIN, 2, 48, 64, 16, 20, kx=8, ycoff=8, yx=4, ty=3, add1=True, add2=True,
         bcast=True),
    conv('glds_coef_nobias_mask_aux_stats_ragged', G_PRO, 2, 32, 40, 37, 20, src='coef', kx=16, ycoff=24, bias=False,
         mask=True, aux=True, stats=True),
    conv('glds_relu_post1_addy_stats_v25', G_PRO, 2, 48, 64, 30, 25, src='relu', kx=8, ycoff=16, post=1, add1='y',
         stats=True),
    conv('glds_two_post0_stats_v64', G_TWO, 1, 32, 48, 9, 64, src='two', ycoff=8, yx=8, post=0, stats=True, add2=True),
    conv('glds_two_dx_ostride2', G_TWO, 2, 48, 64, 16, 20, src='two', wmode=1, ostride=2, ty=1, bias=False, add1='y',
         ycoff=4),
    conv('glds_strided_plain_stats', G_PLAIN, 2, 32, 64, 33, 20, stride=2, kx=16, ycoff=8, stats=True, add1=True),
    conv('glds_strided_relu_post1_v64', G_PRO, 1, 48, 40, 9, 64, stride=2, src='relu', ycoff=8, post=1, bcast=True),
    # ---- data gradients into >= 128 channels: the split-bf16 GEMM in mode 1, the exact one in mode 0
    conv('split_dx_two_mask_addy', {0: G_TWO, 1: G_SPLIT}, 2, 64, 128, 16, 20, src='two', wmode=1, bias=False, mask=True,
         add1='y', ycoff=8, ty=2),
    conv('split_dx_plain_v25_ostride2', {0: G_PLAIN, 1: G_SPLIT}, 2, 64, 132, 13, 25, wmode=1, ostride=2, ty=1,
         add2=True, bcast=True, kx=8),
    # ---- register-pipelined kernel, BK = 32 (1x1 off the LDS-DMA GEMM: K % 16 != 0, too few columns)
    conv('vec32_4_5_post1_stats', vec(32, 4, 5), 2, 24, 64, 16, 20, src='coef', ycoff=8, post=1, stats=True, add1=True),
    conv('vec32_3_5_mask_aux', vec(32, 3, 5), 2, 20, 48, 16, 20, src='relu', mask=True, aux=True, stats=True, ycoff=16,
         bias=False),
    conv('vec32_2_5_dx_ostride2', vec(32, 2, 5), 2, 24, 32, 16, 20, src='two', wmode=1, ostride=2, ty=2, add1='y',
         ycoff=8),
    conv('vec32_1_5_post0_bcast', vec(32, 1, 5), 2, 20, 16, 17, 20, post=0, ycoff=8, bcast=True, add2=True, ty=3),
    conv('vec32_4_3_short_T', vec(32, 4, 3), 3, 24, 64, 9, 20, src='coef', add1=True, add2=True, stats=True, ycoff=4),
    conv('vec32_3_3_two', vec(32, 3, 3), 2, 40, 96, 5, 20, src='two', bias=False, ycoff=8),
    conv('vec32_2_3_short_T', vec(32, 2, 3), 2, 40, 24, 5, 20, src='relu', post=1, ycoff=8, stats=True),
    conv('vec32_1_3_up2', vec(32, 1, 3), 2, 24, 8, 4, 20, up=2, T_out=7, wmode=1, src='coef', add1=True),
    # ---- register-pipelined kernel, BK = 16 (k x 1)
    conv('vec16_3_5_kt5', vec(16, 3, 5), 2, 32, 48, 18, 20, KT=5, pad=2, src='relu', ycoff=8, stats=True, add1=True),
    conv('vec16_3_3_kt5_dil2_post1', vec(16, 3, 3), 2, 16, 48, 9, 20, KT=5, dil=2, pad=4, post=1, ycoff=16,
         stats=True),
    conv('vec16_2_5_kt3_mask_aux', vec(16, 2, 5), 2, 24, 64, 16, 20, KT=3, pad=1, src='coef', mask=True, aux=True,
         stats=True, ycoff=8),
    conv('vec16_2_3_kt9', vec(16, 2, 3), 1, 16, 32, 8, 20, KT=9, pad=4, src='two', bias=False, add2=True, ty=2),
    conv('vec16_2_3_kt5_v64_slices', vec(16, 2, 3), 1, 16, 32, 12, 64, KT=5, dil=2, pad=4, src='relu', post=0,
         ycoff=8, stats=True),
    conv('vec16_1_5_kt5_stride2', vec(16, 1, 5), 2, 16, 16, 37, 20, KT=5, stride=2, pad=2, bcast=True, add1='y',
         ycoff=16),
    conv('vec16_1_5_dx_up2', vec(16, 1, 5), 2, 32, 16, 7, 20, KT=5, pad=2, up=2, T_out=13, wmode=1, src='coef',
         bias=False, ycoff=8, stats=True),
    conv('vec16_1_3_kt5_v25', vec(16, 1, 3), 2, 16, 16, 7, 25, KT=5, pad=2, src='relu', mask=True, stats=True,
         post=1, ycoff=8),
    # 1x1 whose staged line buffer exceeds 320 floats (V % 4 != 0 with a temporal stride: Vp = V rounded up to 4) also
    # takes BK = 16, with 64-row tiles: NTU's strided 1x1 convs; cwt = 3 with such a buffer needs V <= 2
    conv('vec16_4_5_v25_strided', vec(16, 4, 5), 2, 48, 64, 25, 25, stride=2, src='coef', ycoff=8, stats=True,
         add1=True, post=1),
    conv('vec16_4_3_v2_strided', vec(16, 4, 3), 1, 16, 64, 191, 2, stride=2, src='two', mask=True, aux=True,
         stats=True, ycoff=4, bcast=True),
    # ---- scalar kernel: K > 1024, a tile too small to stage the vector epilogue in, or a flat V = 25 tile of fewer than
    # 4 frames (line buffer not whole 16-byte slots)
    conv('scalar_tiny_T_no_room_for_staged_epilogue', 'conv_kernel', 2, 40, 24, 2, 20, src='relu', post=1, ycoff=8,
         stats=True),
    conv('scalar_bigK_post1_addy', 'conv_kernel', 1, 1040, 16, 4, 20, ycoff=8, post=1, add1='y', stats=True),
    conv('scalar_v25_T3_two_mask_aux', 'conv_kernel', 2, 32, 40, 3, 25, src='two', mask=True, aux=True, stats=True,
         bcast=True, ty=2, add2=True, ycoff=8, bias=False),
    conv('scalar_v25_T3_post0_dx_ostride2', 'conv_kernel', 2, 48, 24, 3, 25, wmode=1, ostride=2, post=0, ycoff=4),
    conv('scalar_bigK_dx_up2', 'conv_kernel', 1, 1040, 8, 2, 20, up=2, T_out=3, wmode=1, add1=True),
    # ---- weight gradient, LDS-DMA kernel: (WMT, WKT) tile x (NY, NX) two-source pairs x f32 / split; 1x1, strided, taps
    wg('wg_2_1_1_1', wglds(2, 1, 1, 1, (3, 3)), 2, 48, 40, 8, 20),
    wg('wg_2_1_2_1_strided', wglds(2, 1, 2, 1, (3, 3)), 2, 64, 64, 17, 20, stride=2, gy='two'),
    wg('wg_2_1_1_2', wglds(2, 1, 1, 2, (3, 3)), 3, 33, 40, 7, 25, x='two'),
    wg('wg_2_1_2_2', wglds(2, 1, 2, 2, (2, 2)), 2, 64, 32, 8, 25, gy='two', x='two'),
    wg('wg_2_1_2_2_taps', wglds(2, 1, 2, 2, (2, 2), taps=True), 2, 48, 40, 12, 20, KT=5, gy='two', x='two'),
    wg('wg_4_1_1_1', wglds(4, 1, 1, 1, (3, 3)), 2, 80, 64, 8, 20),
    wg('wg_4_1_2_1', wglds(4, 1, 2, 1, (2, 2)), 2, 128, 48, 9, 64, gy='two'),
    wg('wg_4_1_1_2_taps_v25', wglds(4, 1, 1, 2, (2, 2), taps=True), 2, 80, 24, 13, 25, KT=5, x='two'),
    wg('wg_4_1_2_2', wglds(4, 1, 2, 2, (3, 3)), 2, 80, 40, 8, 20, gy='two', x='two'),
    wg('wg_2_2_1_1_taps_dil2', wglds(2, 2, 1, 1, (3, 3), taps=True), 2, 40, 72, 16, 20, KT=5, dil=2),
    wg('wg_2_2_2_1', wglds(2, 2, 2, 1, (2, 2)), 2, 40, 72, 8, 20, gy='two'),
    wg('wg_2_2_1_2_strided_v64', wglds(2, 2, 1, 2, (2, 2)), 1, 40, 72, 9, 64, stride=2, x='two'),
    wg('wg_2_2_2_2', wglds(2, 2, 2, 2, (3, 3)), 2, 40, 72, 8, 20, gy='two', x='two'),
    wg('wg_4_2_1_1_strided', wglds(4, 2, 1, 1, (2, 2)), 2, 80, 72, 17, 20, stride=2),
    wg('wg_4_2_2_1', wglds(4, 2, 2, 1, (3, 3)), 2, 80, 72, 8, 20, gy='two'),
    wg('wg_4_2_1_2_taps', wglds(4, 2, 1, 2, (3, 3), taps=True), 1, 80, 72, 10, 20, KT=3, x='two'),
    # (4, 2, 2, 2) does not fit three stages: the planner shrinks the tile to (2, 2) -- UNREACHABLE below
    wg('wg_4_2_2_2_shrinks', wglds(2, 2, 2, 2, (3, 3)), 2, 80, 72, 8, 20, gy='two', x='two'),
    wg('wg_glds_empty_split', wglds(2, 1, 1, 1, (3, 3)), 2, 32, 32, 71, 20, nsplit=11, empty=True),
    # ---- weight gradient, register-staged kernel (every launch_wgrad<KT, ...> branch; vec = V % 4 == 0, else ragged)
    wg('wr_1_2_2_short_rows', wreg(1, 2, 2, True), 2, 48, 40, 3, 20),
    wg('wr_1_4_2_v25_strided', wreg(1, 4, 2, False), 2, 80, 40, 13, 25, stride=2, gy='two'),
    wg('wr_1_2_4_short_rows', wreg(1, 2, 4, True), 3, 48, 72, 3, 20, x='two'),
    wg('wr_1_4_4_v25_strided', wreg(1, 4, 4, False), 1, 80, 72, 9, 25, stride=2),
    wg('wr_1_4_2_short_rows', wreg(1, 4, 2, True), 2, 80, 40, 3, 20, gy='two'),
    wg('wr_1_4_4_short_rows', wreg(1, 4, 4, True), 2, 80, 72, 3, 20),
    wg('wr_1_2_2_v25_strided', wreg(1, 2, 2, False), 2, 48, 40, 13, 25, stride=2, x='two'),
    wg('wr_1_2_4_v25_strided', wreg(1, 2, 4, False), 2, 48, 72, 11, 25, stride=2),
    wg('wr_3_2_2_strided', wreg(3, 2, 2, True), 2, 48, 40, 13, 20, KT=3, stride=2, pad=1),
    wg('wr_3_1_1_v25_strided', wreg(3, 1, 1, False), 2, 24, 24, 13, 25, KT=3, stride=2, pad=1, gy='two'),
    wg('wr_5_ps', wreg(5, 1, 1, True, ps=True), 2, 16, 16, 13, 20, KT=5),
    wg('wr_5_ps_v25', wreg(5, 1, 1, True, ps=True), 3, 16, 12, 11, 25, KT=5, dil=2),
    wg('wr_5_2_2_strided', wreg(5, 2, 2, True), 2, 64, 48, 13, 20, KT=5, stride=2, pad=2),
    wg('wr_5_1_1_v25_strided', wreg(5, 1, 1, False), 2, 16, 16, 13, 25, KT=5, stride=2, pad=2),
    wg('wr_5_1_1_strided', wreg(5, 1, 1, True), 2, 24, 24, 12, 20, KT=5, stride=2, pad=2, gy='two'),
    wg('wr_9', wreg(9, 1, 1, True), 2, 24, 24, 13, 20, KT=9),
    wg('wr_9_v25_strided', wreg(9, 1, 1, False), 2, 16, 16, 12, 25, KT=9, stride=2),
    wg('wr_empty_split', wreg(1, 2, 2, True), 5, 32, 32, 3, 20, nsplit=4, empty=True),
])

# instantiations pinned by another test of the suite (TAMGCN_CONV_WAVES is read once per process)
ELSEWHERE = {
    ('TG_GLDS_CASE', ('2', '8', 'true', '4')): 'tests/test_gpu_primitives.py::test_pointwise_gemm_four_wave_layout',
    ('TG_GLDS_CASE', ('1', '16', 'true', '4')): 'tests/test_gpu_primitives.py::test_pointwise_gemm_four_wave_layout',
    ('TG_GLDS_CASE', ('1', '16', 'false', '4')): 'tests/test_gpu_primitives.py::test_pointwise_gemm_four_wave_layout',
}

# instantiations no legal descriptor reaches, with the planner condition that excludes them
UNREACHABLE = {}
UNREACHABLE_SYMBOLS = {
    'wgrad_glds_kernel<4, 2, 2, 2, f32, 3>': 'wgrad_glds_plan: three stages of 128 + 128 two-source rows exceed 160 KB; '
                                              'fits() shrinks wmt 4 -> 2',
    'wgrad_glds_kernel<4, 2, 2, 2, split, 3>': 'wgrad_glds_plan: as the f32 form',
}


def symbols(case):
    s = case['sym']
    return set(s.values()) if isinstance(s, dict) else {s}


def source_key(sym):
    """The (dispatch macro / launcher, template arguments) tuple of conv.hip that launches kernel `sym`."""
    if '<' not in sym:
        return sym, ()
    name, args = sym.split('<', 1)
    args = [a.strip() for a in args.split('>', 1)[0].split(',')]
    if name == 'conv1x1_glds_kernel':
        return 'TG_GLDS_CASE', tuple(args)
    if name == 'conv_kernel_vec':
        return 'TG_CONV_CASE', tuple(args)
    if name == 'wgrad_glds_kernel':
        return 'launch_wgrad_glds_src', (args[0], args[1])
    if name == 'wgrad_kernel':
        return 'launch_wgrad', tuple(args[:3]) + (('true',) if args[-1] == 'p-split' else ())
    return name, tuple(args)


PINNED = set().union(*(symbols(c) for c in CASES.values())) | {'conv_kernel', 'reduce_sum_kernel', 'reduce_multi_kernel'}
PINNED_ELSEWHERE = {f'conv1x1_glds_kernel<{", ".join(k[1])}>' for k in ELSEWHERE}


# ---------------------------------------------------------------------------------------------------------------------
# GPU runners
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rnd(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _src(kind, N, ctot, T, V, g):
    s = dict(x1=_rnd((N, ctot, T, V), g))
    if kind in ('coef', 'relu', 'two'):
        s['coef'] = _rnd((3, ctot), g, 0.5, 1.5) * torch.where(_rnd((3, ctot), g) < 0, -1.0, 1.0)
    if kind == 'two':
        s['x2'] = _rnd((N, ctot, T, V), g)
    if kind == 'relu':
        s['act'] = 1
    return s


def _dev(t):
    """A device copy with 16 readable bytes behind it (ops.empty): the 16-byte kernels' contract for V % 4 != 0 rows."""
    from tam_gcn_amd import ops
    if t is None or isinstance(t, str):
        return t
    out = ops.empty(*t.shape, like=torch.empty(0, device='cuda:0'))
    return out.copy_(t)


def _sdev(s):
    from tam_gcn_amd.ops import S
    return S(_dev(s['x1']), _dev(s.get('x2')), _dev(s.get('coef')), s.get('coff', 0), s.get('act', 0))


class split_mode:
    def __init__(self, mode):
        from tam_gcn_amd import _lib
        self.lib, self.mode = _lib.load(), mode

    def __enter__(self):
        self.prev = self.lib.tamgcn_get_split_mode()
        assert self.lib.tamgcn_set_split_mode(self.mode) == 0
        return self

    def __exit__(self, *exc):
        self.lib.tamgcn_set_split_mode(self.prev)
        return False


def _conv_problem(c, seed):
    g = _gen(seed)
    N, K, M, T, V = c['N'], c['K'], c['M'], c['T'], c['V']
    KT, dil, stride, pad, up = c.get('KT', 1), c.get('dil', 1), c.get('stride', 1), c.get('pad', 0), c.get('up', 1)
    T_out = c.get('T_out') or (T + 2 * pad - dil * (KT - 1) - 1) // stride + 1
    ostride, ycoff = c.get('ostride', 1), c.get('ycoff', 0)
    yctot = ycoff + M + c.get('yx', 0)
    T_y = (T_out - 1) * ostride + 1 + c.get('ty', 0)
    kx = c.get('kx', 0)
    src = _src(c.get('src', 'plain'), N, K + kx + 4, T, V, g)
    src['coff'] = kx
    w = _rnd((K, M, KT) if c.get('wmode', 0) == 1 else (M, K, KT), g) * 0.25
    p = dict(src=src, K=K, M=M, KT=KT, dil=dil, stride=stride, pad=pad, up=up, wmode=c.get('wmode', 0), w=w,
             y0=_rnd((N, yctot, T_y, V), g, -2.0, 2.0), ycoff=ycoff, T_out=T_out, ostride=ostride,
             bias=_rnd((M,), g) if c.get('bias', True) else None, stats=c.get('stats', False))
    if c.get('add1'):
        p['add1'] = 'y' if c['add1'] == 'y' else _rnd((N, yctot, T_y, V), g)
    if c.get('add2'):
        p['add2'] = _rnd((N, yctot, T_y, V), g)
    if c.get('bcast'):
        p['bcast'], p['bcast_scale'] = _rnd((M, N, V), g), 0.375
    if c.get('mask'):
        p['mask'] = dict(x1=_rnd((N, yctot + 8, T_y, V), g), coff=ycoff + 8)
    if c.get('aux'):
        p['aux'], p['auxcoff'] = _rnd((N, yctot + 4, T_y, V), g), ycoff + 4
        p['aux_center'] = _rnd((yctot + 4,), g, -0.5, 0.5)
    if c.get('post') is not None:
        p['post_coef'], p['post_act'] = _rnd((3, yctot), g, 0.5, 1.5), c['post']
        p['post_coef'][1] = 0.0
    return p


def run_conv(c, p, mode):
    """One tamgcn_conv launch of problem p in split mode `mode`: returns (y, stats partials or None, symbol)."""
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    d = _lib.ConvDesc()
    s = _sdev(p['src'])
    d.src = s.c()
    N, _, T_in, V = p['src']['x1'].shape
    d.N, d.K, d.T_in, d.V = N, p['K'], T_in, V
    w, bias = _dev(p['w']), _dev(p.get('bias'))
    d.w, d.bias = w.data_ptr(), (bias.data_ptr() if bias is not None else None)
    d.M, d.KT, d.dil, d.stride, d.pad, d.wmode, d.up = p['M'], p['KT'], p['dil'], p['stride'], p['pad'], p['wmode'], p['up']
    y = _dev(p['y0'])
    d.y, d.yctot, d.ycoff, d.T_out, d.T_y, d.ostride = y.data_ptr(), y.shape[1], p['ycoff'], p['T_out'], y.shape[2], p['ostride']
    keep = []
    for k in ('add1', 'add2'):
        a = p.get(k)
        t = y if a == 'y' else _dev(a)
        keep.append(t)
        setattr(d, k, None if t is None else t.data_ptr())
    if p.get('bcast') is not None:
        bc = _dev(p['bcast'])
        keep.append(bc)
        d.bcast, d.bcast_scale = bc.data_ptr(), p['bcast_scale']
    mc = None
    if p.get('mask') is not None:
        ms = _sdev(p['mask'])
        keep.append(ms)
        mc = ms.c()
        d.mask = C.pointer(mc)
    if p.get('aux') is not None:
        aux, ctr = _dev(p['aux']), _dev(p['aux_center'])
        keep += [aux, ctr]
        d.aux, d.aux_center, d.auxctot, d.auxcoff = aux.data_ptr(), ctr.data_ptr(), aux.shape[1], p['auxcoff']
    if p.get('post_coef') is not None:
        pc = _dev(p['post_coef'])
        keep.append(pc)
        d.post_coef, d.post_ctot = pc.data_ptr(), pc.shape[1]
    d.post_act = int(p.get('post_act', 0))
    part = None
    if p['stats']:
        nparts = lib.tamgcn_conv_nparts(C.byref(d))
        assert nparts > 0
        part = torch.full((2, y.shape[1], nparts), -7.25, device='cuda:0')
        d.stats_part, d.stats_ctot, d.stats_coff = part.data_ptr(), y.shape[1], p['ycoff']
    with split_mode(mode):
        _lib.check(lib.tamgcn_conv(C.byref(d), ops._stream()), 'tamgcn_conv')
        sym = lib.tamgcn_last_kernel().decode()
    torch.cuda.synchronize()
    return y, part, sym


def check_conv(cid, p, y, part, mode, sym):
    split = sym == G_SPLIT
    L = p['K'] * p['KT']
    ref, r1, r2 = B.conv_eval(p)
    mag, m1, m2 = B.conv_eval(p, absval=True)
    M, ycoff = p['M'], p['ycoff']
    tsel = torch.arange(p['T_out']) * p['ostride']
    written = torch.zeros(ref.shape, dtype=torch.bool)
    written[:, ycoff:ycoff + M, tsel] = True
    B.check_untouched(f'{cid}: y outside the written window', y, p['y0'], ~written)
    yw = y.cpu()[:, ycoff:ycoff + M][:, :, tsel]
    B.check(f'{cid} [mode {mode}]: y', yw, ref[:, ycoff:ycoff + M][:, :, tsel], mag[:, ycoff:ycoff + M][:, :, tsel], L,
            split=split)
    if part is not None:
        sentinel = torch.full_like(part.cpu(), -7.25)
        rows = torch.zeros(part.shape, dtype=torch.bool)
        rows[:, ycoff:ycoff + M] = True
        B.check_untouched(f'{cid}: stats rows outside stats_coff..+M', part, sentinel, ~rows)
        P = ref.shape[0] * p['T_out'] * ref.shape[3]           # elements per channel
        got = part.cpu().double()[:, ycoff:ycoff + M].sum(-1)
        B.check(f'{cid}: stats sum', got[0], r1, m1, L + P, global_bound=False)
        B.check(f'{cid}: stats sum of products', got[1], r2, m2, 2 * L + P + 4, global_bound=False)


def _wgrad_problem(c, seed):
    g = _gen(seed)
    N, M, K, T, V = c['N'], c['M'], c['K'], c['T'], c['V']
    KT, dil, stride = c.get('KT', 1), c.get('dil', 1), c.get('stride', 1)
    pad = c.get('pad', dil * (KT - 1) // 2)
    T_out = (T + 2 * pad - dil * (KT - 1) - 1) // stride + 1
    gy = _src('two' if c.get('gy') == 'two' else 'coef', N, M + 24, T_out, V, g)
    gy['coff'] = 16
    x = _src(c.get('x', 'relu'), N, K + 12, T, V, g)
    x['coff'] = 8
    return dict(gy=gy, src=x, N=N, M=M, K=K, KT=KT, dil=dil, stride=stride, pad=pad, T_in=T, T_out=T_out, V=V)


def wgrad_desc(p):
    from tam_gcn_amd import _lib
    d = _lib.WgradDesc()
    gs, xs = _sdev(p['gy']), _sdev(p['src'])
    d.gy, d.src = gs.c(), xs.c()
    d.N, d.M, d.K, d.T_in, d.T_out, d.V = p['N'], p['M'], p['K'], p['T_in'], p['T_out'], p['V']
    d.KT, d.dil, d.stride, d.pad = p['KT'], p['dil'], p['stride'], p['pad']
    return d, (gs, xs)


def run_wgrad(d, p, nsplit, mode):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    part = torch.full((nsplit, p['M'], p['K'], p['KT']), float('nan'), device='cuda:0')
    d.part, d.nsplit = part.data_ptr(), nsplit
    with split_mode(mode):
        _lib.check(lib.tamgcn_wgrad(C.byref(d), ops._stream()), 'tamgcn_wgrad')
        sym = lib.tamgcn_last_kernel().decode()
    torch.cuda.synchronize()
    return part, sym


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('cid', [k for k, c in CASES.items() if c['kind'] == 'conv'])
def test_conv_form(cid):
    c = CASES[cid]
    p = _conv_problem(c, seed=sum(map(ord, cid)))
    modes = sorted(c['sym']) if isinstance(c['sym'], dict) else [0]
    for mode in modes:
        want = c['sym'][mode] if isinstance(c['sym'], dict) else c['sym']
        y, part, sym = run_conv(c, p, mode)
        assert sym == want, f'{cid} [mode {mode}]: dispatched {sym}, ledger says {want}'
        check_conv(cid, p, y, part, mode, sym)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [k for k, c in CASES.items() if c['kind'] == 'wgrad'])
def test_wgrad_form(cid):
    from tam_gcn_amd import _lib
    lib = _lib.load()
    c = CASES[cid]
    p = _wgrad_problem(c, seed=sum(map(ord, cid)))
    L = p['N'] * p['T_out'] * p['V']
    ref = B.wgrad_eval(p['gy'], p['src'], p['M'], p['K'], p['KT'], p['dil'], p['stride'], p['pad'])
    mag = B.wgrad_eval(p['gy'], p['src'], p['M'], p['K'], p['KT'], p['dil'], p['stride'], p['pad'], absval=True)
    d, keep = wgrad_desc(p)
    mx = lib.tamgcn_wgrad_max_split(C.byref(d))
    assert mx >= 1
    splits = [c['nsplit']] if c.get('nsplit') else sorted({1, mx})
    modes = sorted(c['sym']) if isinstance(c['sym'], dict) else [0, 1]
    for mode in modes:
        want = c['sym'][mode] if isinstance(c['sym'], dict) else c['sym']
        for ns in splits:
            assert ns <= mx, (cid, ns, mx)
            part, sym = run_wgrad(d, p, ns, mode)
            assert sym == want, f'{cid} [mode {mode}, nsplit {ns}]: dispatched {sym}, ledger says {want}'
            B.check(f'{cid} [mode {mode}, nsplit {ns}/{mx}]', part.cpu().double().sum(0), ref, mag, L,
                    split=', split,' in sym)
            if c.get('empty'):          # the case leaves its last split without work: that slab must be zeros, not garbage
                assert float(part[-1].abs().max()) == 0.0, f'{cid}: empty split slab not zero'
            again, _ = run_wgrad(d, p, ns, mode)
            assert torch.equal(part, again), f'{cid} [mode {mode}, nsplit {ns}]: two identical launches differ'
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize('nsplit,count,scale,accumulate', [(37, 1000, 0.5, 1), (128, 333, 1.0, 0), (300, 517, -0.25, 1),
                                                           (1000, 70, 3.0, 0)])
def test_reduce_sum_forms(nsplit, count, scale, accumulate):
    """tamgcn_reduce_sum: one stage (nsplit <= 128) and reduce_group_kernel + reduce_sum_kernel (> 128, in place on the
    slabs); slabs strided wider than `count`; scale != 1 and accumulate; bit-identical on a second run."""
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    g = _gen(nsplit + count)
    stride = count + 11
    part0 = _rnd((nsplit, stride), g)
    out0 = _rnd((count,), g)
    ref = scale * part0[:, :count].double().sum(0) + (out0.double() if accumulate else 0)
    mag = abs(scale) * part0[:, :count].double().abs().sum(0) + (out0.double().abs() if accumulate else 0)
    res = []
    for _ in range(2):
        part, out = part0.to('cuda:0'), out0.to('cuda:0')
        _lib.check(lib.tamgcn_reduce_sum(part.data_ptr(), nsplit, stride, count, scale, accumulate, out.data_ptr(),
                                         ops._stream()), 'tamgcn_reduce_sum')
        assert lib.tamgcn_last_kernel().decode() == 'reduce_sum_kernel'
        torch.cuda.synchronize()
        res.append(out.cpu())
    B.check(f'reduce_sum nsplit={nsplit}', res[0], ref, mag, nsplit)
    assert torch.equal(res[0], res[1])


@pytest.mark.gpu
def test_reduce_multi_more_than_one_launch():
    """tamgcn_reduce_multi with 30 descriptors (> RM_MAX = 24: two launches) of unequal counts and split counts, the 8- and
    4-wide load loops and their tails, accumulate and scale; bit-identical on a second run."""
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    g = _gen(7)
    specs = [(1 + (5 * i) % 67, 1 + (97 * i) % 500, (0.5, 1.0, -2.0)[i % 3], i % 2) for i in range(30)]
    parts0 = [_rnd((ns, cnt + 3), g) for ns, cnt, _, _ in specs]
    outs0 = [_rnd((cnt,), g) for _, cnt, _, _ in specs]
    res = []
    for _ in range(2):
        parts = [t.to('cuda:0') for t in parts0]
        outs = [t.to('cuda:0') for t in outs0]
        arr = (_lib.ReduceDesc * len(specs))()
        for i, (ns, cnt, sc, acc) in enumerate(specs):
            arr[i] = _lib.ReduceDesc(parts[i].data_ptr(), outs[i].data_ptr(), ns, acc, cnt + 3, cnt, sc)
        _lib.check(lib.tamgcn_reduce_multi(arr, len(specs), ops._stream()), 'tamgcn_reduce_multi')
        assert lib.tamgcn_last_kernel().decode() == 'reduce_multi_kernel'
        torch.cuda.synchronize()
        res.append([o.cpu() for o in outs])
    for i, (ns, cnt, sc, acc) in enumerate(specs):
        p = parts0[i][:, :cnt].double()
        ref = sc * p.sum(0) + (outs0[i].double() if acc else 0)
        mag = abs(sc) * p.abs().sum(0) + (outs0[i].double().abs() if acc else 0)
        B.check(f'reduce_multi descriptor {i} (nsplit {ns}, count {cnt})', res[0][i], ref, mag, ns)
        assert torch.equal(res[0][i], res[1][i]), i


# ---------------------------------------------------------------------------------------------------------------------
# what the models actually dispatch
# ---------------------------------------------------------------------------------------------------------------------
CONV_HIP_ABI = ('tamgcn_conv', 'tamgcn_wgrad', 'tamgcn_reduce_sum', 'tamgcn_reduce_multi')
_UCLA = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
_NTU = dict(num_class=60, num_point=25, num_person=2, graph='graph.ntu_rgb_d.Graph', graph_args=dict(labeling_mode='spatial'))
_SYN = dict(num_class=10, num_point=64, num_person=1, graph='graph.synthetic.Graph', graph_args=dict(labeling_mode='spatial'))


@pytest.mark.gpu
@pytest.mark.parametrize('margs,shape', [(_UCLA, (2, 3, 64, 20, 1)), (_NTU, (1, 3, 300, 25, 2)), (_SYN, (1, 3, 512, 64, 1))],
                         ids=['ucla_t64', 'ntu_t300', 'config4_t512'])
def test_models_dispatch_only_pinned_forms(margs, shape, monkeypatch):
    """Every conv.hip kernel an eager train step (both split modes) and a general-path eval forward launch is a ledger entry."""
    from helpers import record_kernels
    from tam_gcn_amd.models.ctrgcn import Model
    torch.manual_seed(0)
    m = Model(**margs).to('cuda:0')
    g = _gen(3)
    x = _rnd(shape, g).to('cuda:0')
    lab = torch.randint(0, margs['num_class'], (shape[0],), generator=g).to('cuda:0')
    monkeypatch.setenv('TAMGCN_F2', '0')
    with record_kernels() as rec:
        for mode in (0, 1):
            with split_mode(mode):
                m.train()
                m.zero_grad(set_to_none=True)
                torch.nn.functional.cross_entropy(m(x), lab).backward()
                torch.cuda.synchronize()
        m.eval()
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
    seen = {sym for name, sym in rec.seen if name in CONV_HIP_ABI}
    assert seen, 'no conv.hip launch recorded'
    assert not seen - PINNED, f'conv.hip kernels dispatched by the model but not pinned by the ledger: {sorted(seen - PINNED)}'
