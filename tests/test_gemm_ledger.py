"""CPU: the GEMM-form ledger (tests/test_gpu_gemm_forms.py) stays complete, and the fp64 bars it holds kernels to
(tests/fp64_bars.py) have teeth."""
import os
import re

import pytest
import torch

import fp64_bars as B
import test_gpu_gemm_forms as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')
GEMM_HIP = ('conv.hip', 'wgrad.hip')                                    # the files that hold the GEMM family's dispatch
LAUNCHERS = ('TG_GLDS_CASE', 'TG_CONV_CASE', 'launch_wgrad', 'launch_wgrad_glds_src')


def source_tuples():
    """(launcher, literal template / macro arguments) of every dispatch site in conv.hip and wgrad.hip."""
    src = ''.join(open(os.path.join(CSRC, f)).read() for f in GEMM_HIP)
    found = set()
    for name in LAUNCHERS:
        for m in re.finditer(r'\b' + name + r'\s*[(<]([^()<>]*)[)>]', src):
            args = tuple(a.strip() for a in m.group(1).split(','))
            if all(re.fullmatch(r'-?\d+|true|false', a) for a in args):   # the macro's definition has parameter names
                found.add((name, args))
    return found


def test_every_dispatch_site_is_pinned_or_unreachable():
    found = source_tuples()
    assert len(found) >= 35, sorted(found)                                # the extraction itself still works
    pinned = {L.source_key(s) for c in L.CASES.values() for s in L.symbols(c)}
    missing = sorted(k for k in found if k not in pinned and k not in L.ELSEWHERE and k not in L.UNREACHABLE)
    assert not missing, f'conv.hip instantiations without a ledger case, ELSEWHERE or UNREACHABLE entry: {missing}'
    stale = sorted(k for k in list(L.UNREACHABLE) + list(L.ELSEWHERE) if k not in found)
    assert not stale, f'ledger entries for instantiations conv.hip no longer has: {stale}'
    both = sorted(k for k in L.UNREACHABLE if k in pinned)
    assert not both, f'instantiations listed as unreachable but pinned by a case: {both}'
    src = open(os.path.join(CSRC, 'conv.hip')).read()
    assert 'tamgcn_note_kernel("conv_kernel")' in src and 'conv1x1_glds_split_kernel<2, false, 4>' in src


def test_every_weight_gradient_dma_form_is_pinned():
    """Every (WMT, WKT) tile x (NY, NX) source pair x f32 / split of wgrad_glds_kernel is a case or unreachable."""
    pinned = {re.sub(r' taps$', '', s) for c in L.CASES.values() for s in L.symbols(c) if s.startswith('wgrad_glds')}
    forms = {re.sub(r', \d+>$', '', s) for s in pinned | set(L.UNREACHABLE_SYMBOLS)}
    want = {f'wgrad_glds_kernel<{a}, {b}, {y}, {x}, {s}' for a in (2, 4) for b in (1, 2) for y in (1, 2) for x in (1, 2)
            for s in ('f32', 'split')}
    assert forms == want, sorted(want ^ forms)
    taps = {s for c in L.CASES.values() for s in L.symbols(c) if s.endswith(' taps')}
    assert any(', f32, ' in s for s in taps) and any(', split, ' in s for s in taps)
    forms = {L.source_key(s) for c in L.CASES.values() for s in L.symbols(c)}
    assert ('launch_wgrad', ('5', '1', '1', 'true')) in forms                 # the p-split branch


# ---------------------------------------------------------------------------------------------------------------------
# the checker rejects what a subtly wrong kernel would deliver
# ---------------------------------------------------------------------------------------------------------------------
def _problem():
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.rand(s, generator=g) * 2 - 1                      # noqa: E731
    N, K, M, T, V, KT, ycoff = 2, 24, 16, 13, 20, 5, 8
    yctot = ycoff + M + 4
    src = dict(x1=r(N, K + 8, T, V), coef=r(3, K + 8), act=1, coff=4)
    src['x2'] = r(N, K + 8, T, V)
    pc = torch.rand(3, yctot, generator=g) + 0.5
    return dict(src=src, K=K, M=M, KT=KT, dil=1, stride=1, pad=2, up=1, wmode=0, w=r(M, K, KT) * 0.25, bias=r(M),
                y0=r(N, yctot, T, V), ycoff=ycoff, T_out=T, ostride=1, add1=r(N, yctot, T, V), post_coef=pc, post_act=0,
                stats=False)


def _check(p, got):
    ref, _, _ = B.conv_eval(p)
    mag, _, _ = B.conv_eval(p, absval=True)
    B.check('conv', got, ref, mag, p['K'] * p['KT'])


def _fp32(p, **over):
    q = dict(p, **over)
    y, _, _ = B.conv_eval(q, dt=torch.float32)
    return y


def test_checker_accepts_fp32_torch():
    p = _problem()
    _check(p, _fp32(p))
    B.check_untouched('untouched', _fp32(p), p['y0'], torch.zeros(p['y0'].shape, dtype=torch.bool))


@pytest.mark.parametrize('how', ['drop_channel', 'shift_frame', 'zero_last_tile', 'swap_taps', 'bf16_operands',
                                 'post_coef_from_m'])
def test_checker_rejects_subtly_wrong_results(how):
    p = _problem()
    M, ycoff = p['M'], p['ycoff']
    if how == 'drop_channel':                                   # one input channel missing from the contraction
        w = p['w'].clone()
        w[:, 5] = 0
        got = _fp32(p, w=w)
    elif how == 'shift_frame':                                  # output written one frame late
        got = _fp32(p)
        got[:, ycoff:ycoff + M, 1:] = got[:, ycoff:ycoff + M, :-1].clone()
    elif how == 'zero_last_tile':                               # the last, partial frame tile never written
        got = _fp32(p)
        got[:, ycoff:ycoff + M, 8:] = 0
    elif how == 'swap_taps':
        got = _fp32(p, w=p['w'][:, :, [1, 0, 2, 3, 4]].contiguous())
    elif how == 'bf16_operands':                                # split arithmetic where exact is promised
        src = dict(p['src'])
        src['x1'] = src['x1'].bfloat16().float()
        src['x2'] = src['x2'].bfloat16().float()
        got = _fp32(p, src=src, w=p['w'].bfloat16().float())
    else:                                                       # post-coefficient read at m instead of ycoff + m
        pc = p['post_coef'].clone()
        pc[:, ycoff + 3] = p['post_coef'][:, 3]
        got = _fp32(p, post_coef=pc)
    with pytest.raises(B.BarError):
        _check(p, got)


def test_checker_rejects_a_touched_sentinel_and_nan():
    p = _problem()
    got = _fp32(p)
    keep = torch.ones(got.shape, dtype=torch.bool)
    keep[:, p['ycoff']:p['ycoff'] + p['M']] = False
    B.check_untouched('untouched', got, _fp32(p), keep)
    bad = got.clone()
    bad[0, 0, 0, 0] += 1e-7
    with pytest.raises(B.BarError):
        B.check_untouched('untouched', bad, got, keep)
    ref, _, _ = B.conv_eval(p)
    mag, _, _ = B.conv_eval(p, absval=True)
    got[1, p['ycoff'], 3, 3] = float('nan')
    with pytest.raises(B.BarError):
        B.check('conv', got, ref, mag, p['K'] * p['KT'])


def test_split_bar_is_wider_but_still_catches_a_dropped_channel():
    p = _problem()
    ref, _, _ = B.conv_eval(p)
    mag, _, _ = B.conv_eval(p, absval=True)
    L_ = p['K'] * p['KT']
    src = dict(p['src'])                                        # bf16 hi/lo split of every operand: within the split bar
    for k in ('x1', 'x2'):
        hi = src[k].bfloat16().float()
        src[k] = hi + (src[k] - hi).bfloat16().float()
    B.check('split', _fp32(p, src=src), ref, mag, L_, split=True)
    w = p['w'].clone()
    w[:, 5] = 0
    with pytest.raises(B.BarError):
        B.check('split', _fp32(p, w=w), ref, mag, L_, split=True)
