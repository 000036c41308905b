"""CPU: the temporal-convolution ledger (tests/test_gpu_tconv_forms.py) stays complete, its table agrees with the host planners,
the fp64 reference (tests/tconv_ref.py) is right, and the bars admit correct fp32 arithmetic and reject planted faults."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fp64_bars as B
import tconv_ref as R
import test_gpu_tconv_forms as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')
F32, F64 = torch.float32, torch.float64
SMALL = [cid for cid, c in L.CASES.items() if 'multi' not in c['opts']]


def source_tuples():
    """{macro: set of literal argument tuples} of the TC_CASE / TW_CASE dispatch sites of tconv.hip"""
    src = open(os.path.join(CSRC, 'tconv.hip')).read()
    found = {'TC_CASE': set(), 'TW_CASE': set()}
    for name in found:
        for m in re.finditer(r'\b' + name + r'\s*\(([^()]*)\)', src):
            args = tuple(a.strip() for a in m.group(1).split(','))
            if all(re.fullmatch(r'\d+', a) for a in args):                  # the macro's definition has parameter names
                found[name].add(args)
    return found


def source_key(sym):
    name, args = sym.split('<', 1)
    args = [a.strip() for a in args.split('>', 1)[0].split(',')]
    return ('TC_CASE', tuple(args[:3]), args[3]) if name == 'tconv_kernel' else ('TW_CASE', tuple(args), None)


def primitives_cases():
    import test_gpu_primitives as P
    return P.TCONV_CASES


def test_every_dispatch_site_is_pinned_or_unreachable():
    found = source_tuples()
    assert len(found['TC_CASE']) == 12 and len(found['TW_CASE']) == 4, found
    want = {('TC_CASE', t, d) for t in found['TC_CASE'] for d in ('false', 'true')} | {('TW_CASE', t, None) for t in found['TW_CASE']}
    pinned = {source_key(c[k]) for c in L.CASES.values() for k in ('fwd', 'bwd', 'wgrad')}
    missing = sorted((k for k in want if k not in pinned and k not in L.ELSEWHERE and k not in L.UNREACHABLE), key=str)
    assert not missing, f'tconv.hip instantiations without a ledger case, ELSEWHERE or UNREACHABLE entry: {missing}'
    stale = sorted((k for k in list(L.ELSEWHERE) + list(L.UNREACHABLE) if k not in want), key=str)
    assert not stale, f'ledger entries for instantiations tconv.hip no longer has: {stale}'
    both = sorted((k for k in L.UNREACHABLE if k in pinned or k in L.ELSEWHERE), key=str)
    assert not both, f'instantiations listed as unreachable but pinned: {both}'
    assert all(isinstance(v, str) and v for v in L.UNREACHABLE.values())
    # an ELSEWHERE entry names a TCONV_CASES shape of tests/test_gpu_primitives.py that the planner sends to that form
    for key, shape in L.ELSEWHERE.items():
        assert shape in primitives_cases(), f'{key}: {shape} is no case of test_tconv_fused_branches_fwd_bwd'
        pl = R.plan(shape)
        assert source_key(pl['bwd' if key[2] == 'true' else 'fwd']) == key, (key, shape, pl)


def test_table_agrees_with_the_planner_mirror_and_the_library():
    """Symbols, nparts and max_split of every ledger row as the mirrored planners compute them, and the mirror's counts as
    the library's own queries answer them (the ledger rows and the shapes of test_tconv_fused_branches_fwd_bwd)."""
    for cid, c in L.CASES.items():
        pl = R.plan(c['shape'])
        assert pl is not None and L.supported(c['shape']) == 1, cid
        assert (pl['fwd'], pl['bwd'], pl['wgrad']) == (c['fwd'], c['bwd'], c['wgrad']), (cid, pl)
        assert (pl['nparts_fwd'], pl['nparts_bwd'], pl['max_split']) == c['counts'], (cid, pl)
        assert L.planner_counts(c['shape']) == c['counts'], cid
        assert (pl['tpw_fwd'] >= 2 and pl['tpw_bwd'] >= 2) == ('multi' in c['opts']), cid
    for shape in primitives_cases():
        pl = R.plan(shape)
        assert L.supported(shape) == 1
        assert L.planner_counts(shape) == (pl['nparts_fwd'], pl['nparts_bwd'], pl['max_split']), shape
    assert sum('multi' in c['opts'] for c in L.CASES.values()) == 5


def test_supported_says_what_the_header_says():
    """Cb = 16, 32 or a multiple of 64; KT in {3, 5}; V <= 32 or V % 16 == 0; stride 1 or 2; at most TAMGCN_TCONV_MAXB branches"""
    ok = (2, 32, 9, 20, 5, (1, 2), 1)
    assert L.supported(ok) == 1

    def but(**kw):
        d = dict(zip(('N', 'Cb', 'T', 'V', 'KT', 'dils', 's'), ok))
        d.update(kw)
        return tuple(d.values())
    for shape in (but(Cb=96), but(Cb=48), but(Cb=8), but(V=40), but(KT=7), but(s=3), but(dils=(1, 1, 1, 1, 1, 1, 1))):
        assert L.supported(shape) == 0, shape
        assert R.plan(shape) is None, shape
    for shape in (but(Cb=64), but(Cb=128), but(V=48), but(V=32), but(KT=3), but(s=2), but(dils=(1, 2, 3, 4, 5, 6))):
        assert L.supported(shape) == 1, shape
    hdr = open(os.path.join(os.path.dirname(CSRC), os.pardir, 'include', 'tamgcn.h')).read()
    assert 'Built for Cb = 16, 32 or a multiple of 64' in hdr


def test_options_and_sharper_checks_are_spread_over_the_forms():
    for v in L.VARIANTS:
        forms = {(c['fwd'], c['bwd'], c['wgrad']) for c in L.CASES.values() if v in c['opts']}
        assert len(forms) >= 2, f'{v}: on {len(forms)} forms'
    assert sum('dead' in c['opts'] for c in L.CASES.values()) >= 4
    assert {c['wgrad'] for c in L.CASES.values() if 'splits' in c['opts']} == {c['wgrad'] for c in L.CASES.values()}
    assert all(len(c['shape'][5]) >= 2 for c in L.CASES.values() if 'bias_null' in c['opts'])


# ---------------------------------------------------------------------------------------------------------------------
# the reference is right
# ---------------------------------------------------------------------------------------------------------------------
AUTOGRAD_CASES = ['2x16x9x20x5x(1,2)x1', '2x32x23x20x3x(1,)x2', '1x128x9x17x5x(1,2)x2', '2x16x33x17x3x(1,2,3,4,5,6)x1',
                  '3x16x13x25x5x(1,2)x2', '1x16x11x48x5x(1,2)x2', '1x16x2x25x5x(1,2)x2', '2x16x300x1x5x(1,2)x1']


@pytest.mark.parametrize('cid', AUTOGRAD_CASES)
def test_reference_agrees_with_float64_autograd(cid):
    """conv2d + max_pool2d + ReLU and their autograd in float64 (stride 2 with even and odd T_in, V = 17, V = 48, V = 1)"""
    p = L.problem(L.CASES[cid]['shape'], L.seed_of(cid), dead='dead' in L.CASES[cid]['opts'])
    Cb, KT, s, dils, nb = p['Cb'], p['KT'], p['stride'], p['dils'], len(p['dils'])
    src, gy = p['src'], p['gy']
    c = src['coef'].double()
    z = (c[0][None, :, None, None] * src['x1'].double() + c[2][None, :, None, None]).requires_grad_(True)
    hv = torch.relu(z)
    ws = [w.double()[..., None].clone().requires_grad_(True) for w in p['w']]
    outs = []
    for b, dil in enumerate(dils):
        lo = src['coff'] + b * Cb
        outs.append(F.conv2d(hv[:, lo:lo + Cb], ws[b], p['bias'][b].double(), stride=(s, 1), padding=((KT - 1) * dil // 2, 0),
                             dilation=(dil, 1)))
    lo = src['coff'] + nb * Cb
    outs.append(F.max_pool2d(hv[:, lo:lo + Cb], kernel_size=(3, 1), stride=(s, 1), padding=(1, 0)))
    out = torch.cat(outs, 1)
    g = gy['coef'].double()
    gv = (g[0][None, :, None, None] * gy['x1'].double() + g[1][None, :, None, None] * gy['x2'].double() +
          g[2][None, :, None, None])[:, gy['coff']:gy['coff'] + nb * Cb]
    (out[:, :nb * Cb] * gv).sum().backward()

    def close(name, a, b):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-12 * max(scale, 1e-300), name
    y, s1, s2 = R.fwd(p)
    yw = y[:, p['ycoff']:p['ycoff'] + (nb + 1) * Cb]
    close('y', yw, out.detach())
    assert torch.equal(y[:, :p['ycoff']], p['y0'].double()[:, :p['ycoff']])
    close('s1', s1, out.detach().sum((2, 3)))
    close('s2', s2, (out.detach() ** 2).sum((2, 3)))
    dh, b1, b2 = R.bwd(p)
    d = z.grad[:, src['coff']:src['coff'] + nb * Cb]
    close('dh', dh[:, p['dcoff']:p['dcoff'] + nb * Cb], d)
    m0 = p['mask']['coff']
    hc = p['mask']['x1'].double()[:, m0:m0 + nb * Cb] - p['center'].double()[None, m0:m0 + nb * Cb, None, None]
    close('b1', b1, d.sum((2, 3)))
    close('b2', b2, (d * hc).sum((2, 3)))
    close('dW', R.wgrad(p), torch.stack([w.grad[..., 0] for w in ws]))


# ---------------------------------------------------------------------------------------------------------------------
# float32 torch as the kernel: the bars admit correct arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def slots(sums, ctot, ch0, nparts):
    """[2][ctot][nparts] moment partials as a kernel would leave them: NaN, and for the written channels each sample's sum
    spread over that sample's slots"""
    s = torch.stack(sums).to(F32)                                     # [2][N][nch]
    N, nch = s.shape[1], s.shape[2]
    per = nparts // N
    part = torch.full((2, ctot, nparts), float('nan'))
    w = (s / per).permute(0, 2, 1)[..., None].expand(2, nch, N, per)
    part[:, ch0:ch0 + nch] = w.reshape(2, nch, nparts)
    return part


def emulate(p, counts, nsplit=3):
    """(y, fwd part, dh, bwd part, slabs) of problem p from float32 torch"""
    y, s1, s2 = R.fwd(p, F32)
    dh, b1, b2 = R.bwd(p, F32)
    dw = R.wgrad(p, F32)
    slabs = torch.stack([dw * 0.5, dw * 0.25, dw * 0.25][:nsplit])
    return (y, slots((s1, s2), y.shape[1], p['ycoff'], counts[0]), dh, slots((b1, b2), dh.shape[1], p['dcoff'], counts[1]),
            slabs)


def check_all(name, p, got, **kw):
    y, part, dh, bpart, slabs = got
    R.check_fwd(name, p, y, part, **kw)
    R.check_bwd(name, p, dh, bpart, **kw)
    R.check_wgrad(name, p, slabs, slabs.sum(0))


@pytest.mark.parametrize('cid', SMALL)
def test_bars_admit_float32_torch(cid):
    c = L.CASES[cid]
    p = L.problem(c['shape'], L.seed_of(cid), dead='dead' in c['opts'])
    check_all(cid, p, emulate(p, c['counts']))
    for v in [o for o in c['opts'] if o in L.VARIANTS]:
        q = L.variant(p, v)
        check_all(f'{cid} [{v}]', q, emulate(q, c['counts']))


def test_input_condition_holds_for_every_case():
    """min |c1*x + c0| > 1e-30 over every operand a ReLU or the mask decides on: no fp32 prologue value is subnormal, so the
    float64 expression decides exactly as the kernel's fmaf"""
    for cid, c in L.CASES.items():
        p = L.problem(c['shape'], L.seed_of(cid), dead='dead' in c['opts'])
        assert R.min_abs_prologue(p) > 1e-30, cid
        for v in ('src_nocoef', 'wg_act0'):
            if v in c['opts']:
                assert R.min_abs_prologue(L.variant(p, v)) > 1e-30, (cid, v)


# ---------------------------------------------------------------------------------------------------------------------
# the bars have teeth
# ---------------------------------------------------------------------------------------------------------------------
TEETH = '2x16x33x17x3x(1,2,3,4,5,6)x1'          # three frame tiles per sample (the last one partial), groups of 1 to 3 columns
TEETH_S2 = '3x16x13x25x5x(1,2)x2'               # stride 2, two frame tiles per sample
FAULTS = ['drop_channel', 'swap_taps', 'dilation_of_branch_1', 'shift_frame', 'last_tile_not_written', 'last_group_not_written',
          'bias_of_neighbour', 'mask_from_m', 'upsampling_off_by_one', 'slot_doubled_slot_zeroed', 'bf16_operands',
          'wgrad_item_twice']


def _written(p, t):
    return t[:, p['ycoff']:p['ycoff'] + R.nbr(p) * p['Cb']]


@pytest.mark.parametrize('how', FAULTS)
def test_bars_reject_planted_faults(how):
    cid = TEETH_S2 if how == 'upsampling_off_by_one' else TEETH
    c = L.CASES[cid]
    p = L.problem(c['shape'], L.seed_of(cid))
    pl = R.plan(c['shape'])
    assert pl['plan_fwd']['ntt'] >= 2 and pl['plan_bwd']['ntt'] >= 2
    Cb, KT, V = p['Cb'], p['KT'], p['V']
    if how == 'slot_doubled_slot_zeroed':       # two samples with the same data: their slots hold the same sums
        for s in (p['src'], p['mask'], p['gy']):
            for k in ('x1', 'x2'):
                if s.get(k) is not None:
                    s[k][1] = s[k][0]
    y, part, dh, bpart, slabs = emulate(p, c['counts'])
    check_all(cid, p, (y, part, dh, bpart, slabs))                          # the unspoiled emulation passes
    q = dict(p)
    if how == 'drop_channel':
        q['w'] = [w.clone() for w in p['w']]
        q['w'][0][:, 5] = 0
        y = R.fwd(q, F32)[0]
    elif how == 'swap_taps':
        q['w'] = [p['w'][0][:, :, [1, 0, 2]].contiguous()] + list(p['w'][1:])
        y = R.fwd(q, F32)[0]
    elif how == 'dilation_of_branch_1':
        q['dils'] = (p['dils'][1],) + p['dils'][1:]
        y = R.fwd(q, F32)[0]
    elif how == 'shift_frame':
        w = _written(p, y)
        w[:, :, 1:] = w[:, :, :-1].clone()
    elif how == 'last_tile_not_written':
        t0 = pl['plan_fwd']['BT'] * (pl['plan_fwd']['ntt'] - 1)
        _written(p, y)[:, :, t0:] = _written(p, p['y0'])[:, :, t0:]
    elif how == 'last_group_not_written':                                   # the final V*BT % 4 columns of the first tile
        BT = pl['plan_fwd']['BT']
        n = (BT * V) % 4
        assert 1 <= n <= 3
        _written(p, y)[:, :, BT - 1, V - n:] = _written(p, p['y0'])[:, :, BT - 1, V - n:]
    elif how == 'bias_of_neighbour':
        q['bias'] = [p['bias'][1]] + list(p['bias'][1:])
        y = R.fwd(q, F32)[0]
    elif how == 'mask_from_m':
        q['mask'] = dict(p['mask'], coff=0)
        dh = R.bwd(q, F32)[0]
    elif how == 'upsampling_off_by_one':
        dh = R.bwd(p, F32, up_shift=1)[0]
    elif how == 'slot_doubled_slot_zeroed':
        per = c['counts'][0] // p['N']
        part = part.clone()
        ch = p['ycoff'] + 2
        assert torch.equal(part[:, ch, 0], part[:, ch, per])
        part[:, ch, 0] *= 2
        part[:, ch, per] = 0
        R.check_fwd(cid, p, y, part, per_sample=False)                      # the sum over all slots does not see it
    elif how == 'bf16_operands':
        q['src'] = dict(p['src'], x1=p['src']['x1'].bfloat16().float())
        q['w'] = [w.bfloat16().float() for w in p['w']]
        y = R.fwd(q, F32)[0]
    else:                                                                   # item (sample 0, frame tile 0) counted twice
        p = L.variant(p, 'gy_nocoef')
        y, part, dh, bpart, slabs = emulate(p, c['counts'])
        check_all(cid, p, (y, part, dh, bpart, slabs))
        BT = pl['plan_wgrad']['BT']
        one = L.first_samples(p, 1)
        one['gy'] = dict(one['gy'], x1=one['gy']['x1'].clone())
        one['gy']['x1'][:, :, BT:] = 0
        slabs = slabs.clone()
        slabs[1] += R.wgrad(one, F32)
    with pytest.raises(B.BarError):
        check_all(cid, p, (y, part, dh, bpart, slabs))


def test_bars_reject_touched_sentinels_and_nan_slots():
    cid = TEETH
    c = L.CASES[cid]
    p = L.problem(c['shape'], L.seed_of(cid))
    got = emulate(p, c['counts'])
    for i, idx in ((0, (0, 0, 0, 0)), (0, (1, -1, 3, 3)), (2, (0, 0, 0, 0)), (2, (1, -1, 5, 16))):      # y / dh beside the slices
        bad = [t.clone() for t in got]
        bad[i][idx] += 1e-6
        with pytest.raises(B.BarError):
            check_all(cid, p, bad)
    for i, ch in ((1, p['ycoff'] - 1), (3, p['dcoff'] + len(p['dils']) * p['Cb'])):                  # a slot of another channel
        bad = [t.clone() for t in got]
        bad[i][1, ch, 2] = 0.0
        with pytest.raises(B.BarError):
            check_all(cid, p, bad)
    for i, ch in ((1, p['ycoff'] + 1), (3, p['dcoff'])):                                             # a slot never written
        bad = [t.clone() for t in got]
        bad[i][0, ch, 4] = float('nan')
        with pytest.raises(B.BarError):
            check_all(cid, p, bad)
    bad = [t.clone() for t in got]
    bad[4][2, 1, 3, 3, 1] = float('nan')                                                              # a slab element
    with pytest.raises(B.BarError):
        check_all(cid, p, bad)
    q = L.variant(p, 'nopool')                          # pool = 0: the pooled channels' output and slots must not be written
    with pytest.raises(B.BarError):
        check_all(cid, q, got)
    q = L.variant(p, 'nostats')
    R.check_fwd(cid, q, got[0], torch.full_like(got[1], float('nan')), stats=False)
    with pytest.raises(B.BarError):
        R.check_fwd(cid, q, got[0], got[1], stats=False)
