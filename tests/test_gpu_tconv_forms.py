"""-m gpu: the ledger of the temporal-convolution kernel forms of csrc/tconv.hip.  Every case is one MS-TCN second-stage
shape run through tamgcn_tconv_fwd, _bwd and _wgrad with the descriptor built directly (_lib.TconvDesc), the kernel symbol
each host dispatch must pick (tamgcn_last_kernel), the planners' answers (tamgcn_tconv_nparts, _wgrad_max_split) and an fp64
reference (tests/tconv_ref.py) the results are held to at derived rounding bars: outputs element by element, the moment
partials per sample and over all slots, the weight-gradient slabs, NaN sentinels in every slot and slab, and bit-identical
channels around the written slices.  Sources and outputs are channel slices of wider tensors at different offsets.

tests/test_tconv_ledger_cpu.py (CPU) checks that every instantiation tconv.hip dispatches to is pinned here, pinned by
tests/test_gpu_primitives.py (ELSEWHERE) or listed in UNREACHABLE, that the reference and the bars are right, and that the
bars reject planted faults.  Run with -s for the measured err / bar ratios (profiles/tconv_bars.txt records one run)."""
import ctypes as C

import pytest
import torch

import fp64_bars as B
import tconv_ref as R

NAN = float('nan')


def sym_tc(mt, ct, kt, bwd):
    return f'tconv_kernel<{mt}, {ct}, {kt}, {"true" if bwd else "false"}>'


def sym_tw(tl, kt):
    return f'tconv_wgrad_kernel<{tl}, {tl}, {kt}>'


def case(shape, fwd, bwd, wg, counts, *opts):
    """shape = (N, Cb, T_in, V, KT, dils, stride); fwd / bwd = (MT, CT) of tconv_kernel<MT, CT, KT, dir>; wg = KTL = MTL of
    tconv_wgrad_kernel; counts = (nparts fwd, nparts bwd, max_split); opts: descriptor variants and sharper checks run on top
    of the default descriptor form (see VARIANTS; 'dead', 'splits', 'multi')."""
    KT = shape[4]
    cid = 'x'.join(str(x).replace(' ', '') for x in shape)
    return cid, dict(shape=shape, fwd=sym_tc(*fwd, KT, False), bwd=sym_tc(*bwd, KT, True), wgrad=sym_tw(wg, KT), counts=counts,
                     opts=opts)


CASES = dict([
    case((2, 16, 9, 20, 5, (1, 2), 1), (1, 3), (1, 3), 1, (2, 2, 4), 'dead', 'splits', 'bias_null', 'gy_one'),
    case((2, 32, 9, 20, 3, (1, 2), 1), (2, 3), (2, 3), 2, (2, 2, 4), 'nopool', 'gy_nocoef'),
    case((2, 32, 23, 20, 3, (1,), 2), (2, 5), (2, 5), 2, (2, 4, 4), 'splits', 'nostats', 'wg_act0'),     # stride 2, odd T_in
    case((1, 64, 9, 20, 3, (1, 2), 1), (4, 3), (4, 3), 2, (1, 1, 2), 'bias_null', 'center_null'),
    case((1, 64, 25, 20, 3, (2,), 2), (4, 5), (4, 5), 2, (2, 2, 3), 'dead', 'src_nocoef'),               # ragged last tiles
    # mh = 2 (two workgroups per branch), V = 17: partial group of 1 column, wgrad's 512-float line buffer
    case((1, 128, 9, 17, 5, (1, 2), 2), (4, 3), (4, 3), 2, (1, 1, 1), 'dead', 'nopool', 'gy_one'),
    case((2, 16, 9, 3, 5, (1, 2), 2), (1, 3), (1, 3), 1, (2, 2, 2), 'src_nocoef', 'center_null'),        # one 16-column tile
    case((2, 32, 5, 31, 5, (1, 2), 1), (2, 3), (2, 3), 2, (2, 2, 2), 'nostats', 'gy_nocoef'),            # Vp = 32
    case((2, 32, 11, 18, 3, (1, 2, 3), 2), (2, 3), (2, 5), 2, (2, 2, 2), 'bias_null', 'wg_act0'),
    # nb = TAMGCN_TCONV_MAXB, span 12, ragged tile, partial group of 3
    case((2, 16, 33, 17, 3, (1, 2, 3, 4, 5, 6), 1), (1, 5), (1, 5), 1, (6, 6, 8), 'dead', 'splits', 'nostats', 'gy_one'),
    case((3, 16, 13, 25, 5, (1, 2), 2), (1, 3), (1, 5), 1, (6, 6, 6), 'dead', 'nopool', 'center_null'),
    case((2, 64, 19, 25, 5, (1, 2), 2), (4, 3), (4, 5), 2, (4, 4, 4), 'splits', 'bias_null', 'src_nocoef', 'wg_act0'),
    case((1, 16, 11, 48, 5, (1, 2), 2), (1, 3), (1, 3), 1, (3, 3, 3), 'dead', 'nopool', 'gy_nocoef'),    # nsl = 3
    case((1, 16, 1, 64, 3, (1,), 1), (1, 3), (1, 3), 1, (4, 4, 4), 'gy_one'),                            # T = 1, sliced
    case((1, 16, 2, 25, 5, (1, 2), 2), (1, 3), (1, 3), 1, (1, 1, 1), 'center_null'),                     # BT = 1
    case((1, 32, 1, 20, 5, (1, 2), 1), (2, 3), (2, 3), 2, (1, 1, 1)),             # every tap but the centre is padding
    case((2, 16, 300, 1, 5, (1, 2), 1), (1, 3), (1, 3), 1, (6, 6, 10), 'splits', 'wg_act0'),             # V = 1: BT = 120
    # ---- more than one frame tile per workgroup (tpw >= 2): the cross-tile part of the software pipeline
    case((80, 16, 77, 20, 5, (1, 2), 1), (1, 5), (1, 5), 1, (240, 240, 800), 'multi'),                   # groups of 2, 2, 1
    case((16, 32, 100, 20, 3, (1, 2, 3, 4, 5, 6), 2), (2, 3), (2, 5), 2, (64, 64, 128), 'multi'),
    case((16, 64, 104, 20, 3, (1, 2, 3, 4, 5, 6), 1), (4, 5), (4, 5), 2, (64, 64, 208), 'multi'),
    case((40, 16, 60, 25, 5, (1, 2, 3), 2), (1, 3), (1, 3), 1, (200, 200, 400), 'multi'),                # partial groups
    case((24, 16, 123, 64, 5, (1, 2), 1), (1, 5), (1, 5), 1, (288, 288, 1248), 'multi'),                 # tpw = 3, nsl = 4
])

# (TC_CASE / TW_CASE tuple, direction) pinned by tests/test_gpu_primitives.py::test_tconv_fused_branches_fwd_bwd: the
# TCONV_CASES entry that runs it (tests/test_tconv_ledger_cpu.py checks the claim against the planner mirror)
ELSEWHERE = {
    ('TC_CASE', ('2', '5', '5'), 'false'): (2, 32, 32, 20, 5, (1, 2), 1),
    ('TC_CASE', ('2', '5', '5'), 'true'): (2, 32, 32, 20, 5, (1, 2), 1),
    ('TC_CASE', ('4', '5', '5'), 'false'): (2, 64, 16, 20, 5, (1, 2), 1),
}
# instantiations no supported shape reaches, with the planner condition that excludes them
UNREACHABLE = {}

# descriptor options the Python wrappers hide: name -> (entry points rerun, what changes)
VARIANTS = {
    'bias_null': ('f', 'bias[1] (one-branch cases: bias[0]) = NULL'),
    'nopool': ('f', 'pool = 0'),
    'nostats': ('fb', 'stats_part = NULL'),
    'src_nocoef': ('f', 'forward source without coef'),
    'gy_one': ('bw', 'gradient with x2 = NULL'),
    'gy_nocoef': ('bw', 'gradient without coef'),
    'center_null': ('b', 'center = NULL'),
    'wg_act0': ('w', 'weight gradient with mask.act = 0'),
}
DEAD_K = 3                        # the source channel of branch 0 whose prologue is negative everywhere in the 'dead' cases


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rnd(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _coef(ctot, g):
    return _rnd((3, ctot), g, 0.5, 1.5) * torch.where(_rnd((3, ctot), g) < 0, -1.0, 1.0)


SRC_LEAD, MASK_LEAD, GY_LEAD, Y_LEAD, DH_LEAD = 16, 4, 12, 8, 20


def problem(shape, seed, dead=False):
    """The default descriptor form of a shape: every option present (biases, pool, moments, coefficients, two-source gradient,
    center).  The mask of the backward holds the forward's source values in a tensor of another width at another offset."""
    N, Cb, T, V, KT, dils, s = shape
    g = _gen(seed)
    nb, T2 = len(dils), (T - 1) // s + 1
    sct = SRC_LEAD + (nb + 1) * Cb + 8
    src = dict(x1=_rnd((N, sct, T, V), g), coef=_coef(sct, g), coff=SRC_LEAD, act=1)
    src['coef'][1] = 0.0
    if dead:
        src['coef'][0, SRC_LEAD + DEAD_K], src['coef'][2, SRC_LEAD + DEAD_K] = 0.25, -2.0
    mct = MASK_LEAD + nb * Cb + 4
    mx, mc = _rnd((N, mct, T, V), g), _coef(mct, g)
    mx[:, MASK_LEAD:MASK_LEAD + nb * Cb] = src['x1'][:, SRC_LEAD:SRC_LEAD + nb * Cb]
    mc[:, MASK_LEAD:MASK_LEAD + nb * Cb] = src['coef'][:, SRC_LEAD:SRC_LEAD + nb * Cb]
    gct = GY_LEAD + nb * Cb + 4
    gy = dict(x1=_rnd((N, gct, T2, V), g), x2=_rnd((N, gct, T2, V), g), coef=_coef(gct, g), coff=GY_LEAD, act=0)
    return dict(N=N, Cb=Cb, T_in=T, T_out=T2, V=V, KT=KT, dils=tuple(dils), stride=s, pool=1, src=src,
                w=[_rnd((Cb, Cb, KT), g) * 0.25 for _ in dils], bias=[_rnd((Cb,), g) for _ in dils],
                y0=_rnd((N, Y_LEAD + (nb + 1) * Cb + 8, T2, V), g, -2.0, 2.0), ycoff=Y_LEAD, gy=gy,
                mask=dict(x1=mx, coef=mc, coff=MASK_LEAD), center=_rnd((mct,), g, -0.5, 0.5),
                dh0=_rnd((N, DH_LEAD + nb * Cb + 4, T, V), g, -2.0, 2.0), dcoff=DH_LEAD, wsrc=src)


def variant(p, name):
    q = dict(p)
    if name == 'bias_null':
        q['bias'] = list(p['bias'])
        q['bias'][min(1, len(p['dils']) - 1)] = None
    elif name == 'nopool':
        q['pool'] = 0
    elif name == 'src_nocoef':
        q['src'] = dict(p['src'], coef=None)
    elif name == 'gy_one':
        q['gy'] = dict(p['gy'], x2=None)
    elif name == 'gy_nocoef':
        q['gy'] = dict(p['gy'], coef=None)
    elif name == 'center_null':
        q['center'] = None
    elif name == 'wg_act0':
        q['wsrc'] = dict(p['src'], act=0)
    else:
        assert name == 'nostats', name
    return q


def first_samples(p, n):
    """the same problem on samples 0:n alone"""
    def cut(s):
        return {k: (v[:n].contiguous() if k in ('x1', 'x2') and v is not None else v) for k, v in s.items()}
    q = dict(p, N=n, src=cut(p['src']), gy=cut(p['gy']), mask=cut(p['mask']), y0=p['y0'][:n].contiguous(),
             dh0=p['dh0'][:n].contiguous())
    q['wsrc'] = q['src']
    return q


def seed_of(cid):
    return sum(map(ord, cid))


def supported(shape):
    from tam_gcn_amd import _lib
    N, Cb, T, V, KT, dils, s = shape
    arr = (C.c_int * max(1, len(dils)))(*dils)
    return _lib.load().tamgcn_tconv_supported(V, Cb, KT, len(dils), arr, s, T)


def query_desc(shape):
    """a descriptor that carries the shape alone: what the planners' queries read"""
    from tam_gcn_amd import _lib
    N, Cb, T, V, KT, dils, s = shape
    d = _lib.TconvDesc()
    d.N, d.T_in, d.T_out, d.V, d.Cb, d.nb, d.KT, d.stride = N, T, (T - 1) // s + 1, V, Cb, len(dils), KT, s
    for b, dl in enumerate(dils):
        d.dil[b] = dl
    return d


def planner_counts(shape):
    from tam_gcn_amd import _lib
    lib, d = _lib.load(), query_desc(shape)
    return (lib.tamgcn_tconv_nparts(C.byref(d), 0), lib.tamgcn_tconv_nparts(C.byref(d), 1),
            lib.tamgcn_tconv_wgrad_max_split(C.byref(d)))


# ---------------------------------------------------------------------------------------------------------------------
# GPU runners
# ---------------------------------------------------------------------------------------------------------------------
def _dev(t):
    """A device copy with 16 readable bytes behind it (ops.empty): the 16-byte kernels' contract for V % 4 != 0 rows."""
    from tam_gcn_amd import ops
    if t is None:
        return None
    return ops.empty(*t.shape, like=torch.empty(0, device='cuda:0')).copy_(t)


def _sdev(s):
    from tam_gcn_amd.ops import S
    return S(_dev(s['x1']), _dev(s.get('x2')), _dev(s.get('coef')), s.get('coff', 0), s.get('act', 0))


def _base_desc(p, src):
    from tam_gcn_amd import _lib
    d = _lib.TconvDesc()
    d.src = src.c()
    d.N, d.T_in, d.T_out, d.V, d.Cb, d.nb, d.KT, d.stride = (p['N'], p['T_in'], p['T_out'], p['V'], p['Cb'], len(p['dils']),
                                                              p['KT'], p['stride'])
    for b, dl in enumerate(p['dils']):
        d.dil[b] = dl
    return d


def _nan(*shape):
    return torch.full(shape, NAN, device='cuda:0')


def fwd_desc(p, stats=True):
    """(descriptor, y, part, tensors to keep alive)"""
    from tam_gcn_amd import _lib
    lib = _lib.load()
    s = _sdev(p['src'])
    d = _base_desc(p, s)
    ws, bs = [_dev(w) for w in p['w']], [_dev(b) for b in p['bias']]
    for b in range(len(ws)):
        d.w[b], d.bias[b] = ws[b].data_ptr(), (bs[b].data_ptr() if bs[b] is not None else None)
    d.pool = int(p['pool'])
    y = _dev(p['y0'])
    d.y, d.yctot, d.ycoff = y.data_ptr(), y.shape[1], p['ycoff']
    nparts = lib.tamgcn_tconv_nparts(C.byref(d), 0)
    assert nparts > 0
    part = _nan(2, y.shape[1], nparts)
    if stats:
        d.stats_part, d.stats_ctot = part.data_ptr(), y.shape[1]
    return d, y, part, (s, ws, bs)


def run_fwd(p, stats=True):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    d, y, part, keep = fwd_desc(p, stats)
    _lib.check(lib.tamgcn_tconv_fwd(C.byref(d), ops._stream()), 'tamgcn_tconv_fwd')
    sym = lib.tamgcn_last_kernel().decode()
    torch.cuda.synchronize()
    del keep
    return y, part, sym


def bwd_desc(p, stats=True):
    from tam_gcn_amd import _lib
    lib = _lib.load()
    s, ms = _sdev(p['gy']), _sdev(p['mask'])
    d = _base_desc(p, s)
    ws = [_dev(w) for w in p['w']]
    for b in range(len(ws)):
        d.w[b] = ws[b].data_ptr()
    dh = _dev(p['dh0'])
    d.y, d.yctot, d.ycoff = dh.data_ptr(), dh.shape[1], p['dcoff']
    mc = ms.c()
    ctr = _dev(p['center'])
    d.mask, d.center = C.pointer(mc), (ctr.data_ptr() if ctr is not None else None)
    nparts = lib.tamgcn_tconv_nparts(C.byref(d), 1)
    assert nparts > 0
    part = _nan(2, dh.shape[1], nparts)
    if stats:
        d.stats_part, d.stats_ctot = part.data_ptr(), dh.shape[1]
    return d, dh, part, (s, ms, mc, ws, ctr)


def run_bwd(p, stats=True):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    d, dh, part, keep = bwd_desc(p, stats)
    _lib.check(lib.tamgcn_tconv_bwd(C.byref(d), ops._stream()), 'tamgcn_tconv_bwd')
    sym = lib.tamgcn_last_kernel().decode()
    torch.cuda.synchronize()
    del keep
    return dh, part, sym


def wgrad_desc(p):
    s, xs = _sdev(p['gy']), _sdev(p['wsrc'])
    d = _base_desc(p, s)
    mc = xs.c()
    d.mask = C.pointer(mc)
    return d, (s, xs, mc)


def launch_wgrad(d, p, nsplit, alloc=None):
    """rc, slabs (pre-filled with NaN; `alloc` slabs where nsplit itself is not a legal size), symbol"""
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    slabs = _nan(alloc or nsplit, len(p['dils']), p['Cb'], p['Cb'], p['KT'])
    d.y, d.yctot, d.ycoff = slabs.data_ptr(), nsplit, 0
    rc = lib.tamgcn_tconv_wgrad(C.byref(d), ops._stream())
    sym = lib.tamgcn_last_kernel().decode()
    torch.cuda.synchronize()
    return rc, slabs, sym


def wrapper_nsplit(p, mx):
    """what ops.tconv_wgrad chooses"""
    from tam_gcn_amd import ops
    blocks = len(p['dils']) * (1 if p['Cb'] == 16 else (p['Cb'] // 32) ** 2)
    return max(1, min(mx, ops.WGRAD_BLOCKS * 2 // blocks))


def run_wgrad(name, p, d, nsplit, want, key=None):
    from tam_gcn_amd import ops
    rc, slabs, sym = launch_wgrad(d, p, nsplit)
    assert rc == 0, f'{name}: tamgcn_tconv_wgrad failed'
    assert sym == want, f'{name}: dispatched {sym}, ledger says {want}'
    red = ops.reduce_sum(slabs.clone(), nsplit, immediate=True)
    torch.cuda.synchronize()
    return R.check_wgrad(name, p, slabs, red, key=key)


def report(cid, what, rat):
    print(f'TCONV_BAR {cid} [{what}] ' + ' '.join(f'{k}={v:.4f}' for k, v in rat.items()))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(CASES))
def test_tconv_form(cid):
    c = CASES[cid]
    shape, opts = c['shape'], c['opts']
    assert supported(shape) == 1
    assert planner_counts(shape) == c['counts'], f'{cid}: the planners answer {planner_counts(shape)}, ledger says {c["counts"]}'
    p = problem(shape, seed_of(cid), dead='dead' in opts)
    assert R.min_abs_prologue(p) > 1e-30
    nb, Cb = len(p['dils']), p['Cb']
    # ---- the default descriptor form
    y, part, sym = run_fwd(p)
    assert sym == c['fwd'], f'{cid}: forward dispatched {sym}, ledger says {c["fwd"]}'
    assert part.shape[2] == c['counts'][0]
    rat = R.check_fwd(f'{cid} fwd', p, y, part)
    dh, bpart, sym = run_bwd(p)
    assert sym == c['bwd'], f'{cid}: backward dispatched {sym}, ledger says {c["bwd"]}'
    assert bpart.shape[2] == c['counts'][1]
    rat.update(R.check_bwd(f'{cid} bwd', p, dh, bpart))
    wd, wkeep = wgrad_desc(p)
    mx = c['counts'][2]
    ns0 = wrapper_nsplit(p, mx)
    rat.update(run_wgrad(f'{cid} wgrad nsplit={ns0}', p, wd, ns0, c['wgrad'], key=cid))
    report(cid, 'default', rat)

    if 'dead' in opts:
        # the dead channel's prologue is negative everywhere: the output does not depend on its data, its gradient and its
        # two backward moments are exactly zero
        q = dict(p, src=dict(p['src'], x1=p['src']['x1'].clone()))
        q['src']['x1'][:, SRC_LEAD + DEAD_K] = _rnd(q['src']['x1'][:, 0].shape, _gen(1))
        y2, part2, _ = run_fwd(q)
        assert torch.equal(y2, y) and torch.equal(part2.view(torch.int32), part.view(torch.int32)), \
            f'{cid}: the forward depends on a channel whose ReLU is off everywhere'
        ch = DH_LEAD + DEAD_K
        assert float(dh[:, ch].abs().max()) == 0.0, f'{cid}: dh of the dead channel is not exactly zero'
        assert float(bpart[:, ch].abs().max()) == 0.0, f'{cid}: backward moments of the dead channel are not exactly zero'

    if 'splits' in opts:
        for ns in sorted({1, mx, ns0} | ({mx - 1} if mx > 2 else set())):
            if ns != ns0:
                report(cid, f'nsplit={ns}/{mx}', run_wgrad(f'{cid} wgrad nsplit={ns}/{mx}', p, wd, ns, c['wgrad'], key=cid))
        from tam_gcn_amd import _lib
        for ns in (0, mx + 1):
            rc, slabs, _ = launch_wgrad(wd, p, ns, alloc=mx + 1)
            assert rc != 0, f'{cid}: nsplit = {ns} of {mx} was accepted'
            assert b'nsplit' in _lib.load().tamgcn_last_error()
            assert bool(torch.isnan(slabs).all()), f'{cid}: a refused nsplit wrote a slab'
    del wkeep

    for v in [o for o in opts if o in VARIANTS]:
        q, which, rat = variant(p, v), VARIANTS[v][0], {}
        stats = v != 'nostats'
        if 'f' in which:
            yv, pv, sym = run_fwd(q, stats)
            assert sym == c['fwd']
            rat.update(R.check_fwd(f'{cid} fwd [{v}]', q, yv, pv, stats))
            if v == 'nopool':               # the pooled branch's channels and moment slots stay what they were
                lo = Y_LEAD + nb * Cb
                assert torch.equal(yv[:, lo:lo + Cb].cpu(), p['y0'][:, lo:lo + Cb])
                assert bool(torch.isnan(pv[:, lo:lo + Cb]).all())
        if 'b' in which:
            dv, pv, sym = run_bwd(q, stats)
            assert sym == c['bwd']
            rat.update(R.check_bwd(f'{cid} bwd [{v}]', q, dv, pv, stats))
        if 'w' in which:
            wq, keep = wgrad_desc(q)
            rat.update(run_wgrad(f'{cid} wgrad [{v}]', q, wq, ns0, c['wgrad']))
            del keep
        report(cid, v, rat)

    if 'multi' in opts:
        # independence from the tile grouping: samples 0:2 alone run with one tile per workgroup, and an element's products
        # are added in the same order whatever the grouping
        pl = R.plan(shape)
        assert pl['tpw_fwd'] >= 2 and pl['tpw_bwd'] >= 2, pl
        q = first_samples(p, 2)
        small = R.plan((2,) + tuple(shape[1:]))
        assert small['tpw_fwd'] == 1 and small['tpw_bwd'] == 1 and (small['fwd'], small['bwd']) == (c['fwd'], c['bwd'])
        y2, _, sym = run_fwd(q)
        assert sym == c['fwd']
        assert torch.equal(y2, y[:2]), f'{cid}: y depends on the number of frame tiles per workgroup'
        d2, _, sym = run_bwd(q)
        assert sym == c['bwd']
        assert torch.equal(d2, dh[:2]), f'{cid}: dh depends on the number of frame tiles per workgroup'


# ---------------------------------------------------------------------------------------------------------------------
# refused descriptors: host checks in front of any launch
# ---------------------------------------------------------------------------------------------------------------------
def _refused(fn, d, out, before, word):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    rc = getattr(lib, fn)(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0, f'{fn}: accepted a descriptor with {word}'
    msg = lib.tamgcn_last_error().decode()
    assert fn in msg, (fn, word, msg)
    assert torch.equal(out.cpu(), before), f'{fn}: wrote although it refused ({word})'
    return msg


@pytest.mark.gpu
def test_refused_descriptors_launch_nothing():
    from tam_gcn_amd import _lib
    shape = (2, 16, 9, 20, 5, (1, 2), 1)
    p = problem(shape, 5)

    def f(edit, word):
        d, y, part, keep = fwd_desc(p)
        edit(d, keep)
        msg = _refused('tamgcn_tconv_fwd', d, y, p['y0'], word)
        assert bool(torch.isnan(part).all())
        return msg

    def b(edit, word):
        d, dh, part, keep = bwd_desc(p)
        edit(d, keep)
        msg = _refused('tamgcn_tconv_bwd', d, dh, p['dh0'], word)
        assert bool(torch.isnan(part).all())
        return msg

    def set_(**kw):
        def edit(d, keep):
            for k, v in kw.items():
                obj = d
                *path, last = k.split('__')
                for a in path:
                    obj = getattr(obj, a)
                setattr(obj, last, v)
        return edit

    assert 'ReLU' in f(set_(src__act=0), 'src.act = 0')
    assert 'single-source' in f(lambda d, keep: setattr(d.src, 'x2', keep[0].x1.data_ptr()), 'a second source')
    assert 'act = 0' in b(set_(src__act=1), 'src.act = 1')
    assert 'T_out' in f(set_(T_out=p['T_out'] + 1), 'T_out inconsistent')
    assert 'T_out' in b(set_(T_out=p['T_out'] - 1), 'T_out inconsistent')
    assert 'out of range' in f(set_(src__ctot=SRC_LEAD + 3 * 16 - 1), 'a source slice past ctot')
    assert 'out of range' in f(set_(yctot=Y_LEAD + 3 * 16 - 1), 'an output slice past yctot')
    assert 'out of range' in b(set_(yctot=DH_LEAD + 2 * 16 - 1), 'an output slice past yctot')
    assert 'out of range' in b(lambda d, keep: setattr(keep[2], 'ctot', MASK_LEAD + 2 * 16 - 1), 'a mask slice past ctot')
    assert 'even' in f(set_(KT=4), '(KT-1)*dil odd')
    assert 'even' in b(set_(KT=4), '(KT-1)*dil odd')
    # the weight gradient: T_out, slices, (KT-1)*dil
    for edit, word, txt in ((set_(T_out=p['T_out'] + 1), 'T_out inconsistent', 'T_out'),
                            (set_(src__ctot=GY_LEAD + 2 * 16 - 1), 'a gradient slice past ctot', 'out of range'),
                            (set_(KT=4), '(KT-1)*dil odd', 'even')):
        d, keep = wgrad_desc(p)
        edit(d, keep)
        slabs = _nan(2, 2, 16, 16, 5)
        d.y, d.yctot, d.ycoff = slabs.data_ptr(), 2, 0
        rc = _lib.load().tamgcn_tconv_wgrad(C.byref(d), None)
        torch.cuda.synchronize()
        assert rc != 0 and txt in _lib.load().tamgcn_last_error().decode(), word
        assert bool(torch.isnan(slabs).all()), word
