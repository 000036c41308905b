"""-m gpu: the raw guidance ABI (csrc/guidance.hip: tamgcn_guidance_reduce, _weights, _apply) on the seeded features of
tests/guidance_cases.py against the fp64 restatement tests/guidance_ref.py.  Every output lies inside a poisoned margin that must
come back untouched.

Bars -- derived, not picked (tests/guidance_ref.py has the derivation in full):
  intensity  fp64_bars.check with L = C, mag = I:            |dI| <= (C + 4) 2^-24 I
  pooled     fp64_bars.check with L = T' V M, mag = mean|h|
  weights    the intensity bar E = (C + 4) 2^-24 max I moves I, min and max, so f = 255 (I - min) / (max - min) moves by
             <= 255 * 4 E / (max - min - 2 E) + 4 * 2^-24 * 255: the intensity bar amplified by 255 / (max - min).  The mean of the k
             largest is 1-Lipschitz in that, summed in fp64 on the device; one rounding to fp32 and one for / 127:
             |dw| <= (|df| + 2 * 2^-24 * 255) / 127.   With max == min: |dw| <= (E + 2 * 2^-24 max) / 127, and the intensities
             themselves must be bit-equal for that branch to be taken at all.
  map, out   apply is fed the reference weights rounded to fp32, so only its own arithmetic is measured: the fp32 row position is
             within 3 * 2^-24 * 225 of the exact one and the profile is continuous piecewise linear:  |dmap| <= 3 * 2^-24 * 225 *
             (largest step between neighbouring rows around the position) + 4 * 2^-24 (|a| + |b|);  |dout| <= |rgb| |dmap| +
             2 * 2^-24 |out|.
Two discontinuities are conditions on the INPUTS, asserted on the fp64 reference before a device result is looked at
(guidance_cases.assert_conditions; tests/test_guidance_ref_cpu.py checks them for every case without a GPU): max - min >= max / 4,
and the two persons' means >= 100 |df| apart unless person 1 is a bitwise copy.
profiles/guidance_stage_bars.txt keeps the measured maxima of one run (pytest -s prints them)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_bars as B                                   # noqa: E402
import guidance_cases as S                              # noqa: E402
import guidance_ref as R                                # noqa: E402
from tam_gcn_amd import _lib                            # noqa: E402

DEV = 'cuda:0'
PAD = 64                      # floats of poisoned margin on either side of an output (256 bytes: the payload stays 16-byte aligned)
POISON = -7777.25


class Guarded:
    """an output of `shape` inside a poisoned buffer; `shift` floats of extra offset move the payload off its 16-byte alignment"""

    def __init__(self, shape, shift=0):
        self.shape, self.n, self.off = tuple(shape), int(np.prod(shape)), PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 4,), POISON, device=DEV, dtype=torch.float32)
        self.before = self.buf.clone()
        self.keep = torch.ones(self.buf.numel(), dtype=torch.bool)
        self.keep[self.off:self.off + self.n] = False

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def get(self, name):
        B.check_untouched(name, self.buf, self.before, self.keep)
        got = self.buf[self.off:self.off + self.n].view(self.shape)
        assert not bool((got == POISON).any()), f'{name}: elements were not written'
        return got


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ratio(got, ref, bar):
    err = np.abs(got.double().cpu().numpy() - ref)
    assert np.all(err <= bar), f'{float(np.max(err / np.maximum(bar, 1e-300))):.3g} bars'
    return float(np.max(err / np.maximum(bar, 1e-300)))


@pytest.fixture(scope='module')
def problems():
    return {cid: S.problem(c) for cid, c in S.CASES.items()}


@pytest.mark.parametrize('cid', list(S.CASES))
def test_stages_against_the_fp64_reference(cid, problems):
    c, p = S.CASES[cid], problems[cid]
    S.assert_conditions(cid, p)                                           # on the reference, before any device result
    lib = _lib.load()
    N, M, Cc, T, V = c['N'], c['M'], c['C'], c['T'], c['V']
    H, W = p['size']
    h = p['h'].to(DEV)
    parts = lib.tamgcn_guidance_parts(N, M, T, V)
    assert parts == N * M * -(-T * V // 64)
    # ---- reduce
    inten, pooled, csum, minmax = Guarded((N, T, V, M)), Guarded((N, Cc)), Guarded((parts, Cc)), Guarded((parts, 2))
    _lib.check(lib.tamgcn_guidance_reduce(h.data_ptr(), N, M, Cc, T, V, inten.ptr, pooled.ptr, csum.ptr, minmax.ptr, _stream()), 'reduce')
    Ig = inten.get('intensity')
    csum.get('csum')
    mm = minmax.get('minmax')
    I64 = torch.from_numpy(p['I'])
    r_i = B.check(f'{cid}: intensity', Ig, I64, I64, Cc) / float(I64.max())
    r_p = B.check(f'{cid}: pooled', pooled.get('pooled'), torch.from_numpy(p['pooled']), torch.from_numpy(p['pooled_mag']), T * V * M)
    assert float(mm[:, 0].min()) == float(Ig.min()) and float(mm[:, 1].max()) == float(Ig.max())
    if p['special'] == 'const':
        assert float(Ig.min()) == float(Ig.max()), 'a constant feature map must give bit-equal intensities'
    if p['special'] == 'copy':
        assert torch.equal(Ig[1, :, :, 0], Ig[1, :, :, 1])
    # ---- weights, from the device's own intensity and partials
    J = len(p['targets'])
    joints = torch.tensor(p['targets'], dtype=torch.int32, device=DEV)
    wg = Guarded((N, J))
    _lib.check(lib.tamgcn_guidance_weights(inten.ptr, minmax.ptr, parts, N, T, V, M, joints.data_ptr(), J, p['k'], wg.ptr, _stream()), 'weights')
    E = R.intensity_bar_max(p['I'], Cc)
    r_w = _ratio(wg.get('weights'), p['w'], R.weights_bar(p['I'], E))
    for j, v in enumerate(p['targets']):
        if v >= V:
            assert bool((wg.get('weights')[:, j] == 0).all())
    # ---- apply, from the reference weights in fp32: out and map, then the map alone
    w32 = torch.from_numpy(p['w'].astype(np.float32)).to(DEV)
    w64 = w32.double().cpu().numpy()
    map_ref = R.weight_map(w64, p['frames'], (H, W))
    out_ref = p['rgb'].double().numpy() * map_ref
    mbar = R.map_bar(w64, p['frames'], H)[:, None, :, None]
    obar = np.abs(p['rgb'].double().numpy()) * mbar + 2 * R.U * np.abs(out_ref)
    shifts = ((1, 0), (1, 1)) if p['misaligned'] else ((0, 0),)          # rgb only 4-byte aligned: out aligned, then out alike
    r_m = r_o = 0.0
    for rs, os_ in shifts:
        rgb_buf = torch.zeros(p['rgb'].numel() + 8, device=DEV)
        rgb = rgb_buf[rs:rs + p['rgb'].numel()].view(p['rgb'].shape)
        rgb.copy_(p['rgb'])
        assert rgb.data_ptr() % 16 == 4 * rs
        out, wm = Guarded(p['rgb'].shape, os_), Guarded((N, 1, H, W))
        _lib.check(lib.tamgcn_guidance_apply(w32.data_ptr(), N, J, p['frames'], rgb.data_ptr(), c['Crgb'], H, W, out.ptr, wm.ptr, _stream()), 'apply')
        r_m = max(r_m, _ratio(wm.get('map'), map_ref, mbar))
        r_o = max(r_o, _ratio(out.get('out'), out_ref, obar))
        only = Guarded((N, 1, H, W))
        _lib.check(lib.tamgcn_guidance_apply(w32.data_ptr(), N, J, p['frames'], None, 0, H, W, None, only.ptr, _stream()), 'apply (map)')
        assert torch.equal(only.get('map alone'), wm.get('map'))
    if p['frames'] < J:                                                   # a stripe beyond 45 * frames stays 0
        assert float(wm.get('map')[:, :, -1].abs().max()) == 0.0
    print(f'\nguidance_stage_bars {cid:20s} intensity {r_i:9.3e} of max (bar {(Cc + 4) * R.U:9.3e})  pooled max|err| {r_p:9.3e}  '
          f'weights {r_w:6.3f}  map {r_m:6.3f}  out {r_o:6.3f}  (err / bar)')


def test_two_runs_are_bit_equal_and_bad_arguments_are_refused(problems):
    lib = _lib.load()
    p = problems['ntu_t16_2p']
    c = S.CASES['ntu_t16_2p']
    N, M, Cc, T, V = c['N'], c['M'], c['C'], c['T'], c['V']
    h = p['h'].to(DEV)
    parts = lib.tamgcn_guidance_parts(N, M, T, V)
    runs = []
    for _ in range(2):
        bufs = [torch.empty(s, device=DEV) for s in ((N, T, V, M), (N, Cc), (parts, Cc), (parts, 2))]
        _lib.check(lib.tamgcn_guidance_reduce(h.data_ptr(), N, M, Cc, T, V, *[b.data_ptr() for b in bufs], _stream()), 'reduce')
        runs.append(bufs)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    one = torch.zeros(4, device=DEV)
    q = one.data_ptr()
    assert lib.tamgcn_guidance_reduce(q, 1, 1, 1, 1, 33, q, q, q, q, None) < 0 and b'tamgcn_guidance_reduce' in lib.tamgcn_last_error()
    assert lib.tamgcn_guidance_reduce(q, 1, 1, 1, 1, 1, q, q, q, q, None) < 0
    assert lib.tamgcn_guidance_weights(q, q, 1, 1, 1025, 2, 1, q, 1, 15, q, None) < 0 and b'tamgcn_guidance_weights' in lib.tamgcn_last_error()
    assert lib.tamgcn_guidance_apply(q, 1, 1, 5, q, 1, 1, 1, None, None, None) < 0 and b'tamgcn_guidance_apply' in lib.tamgcn_last_error()
    assert lib.tamgcn_guidance_apply(q, 1, 1, 5, None, 1, 1, 1, q, None, None) < 0
    assert lib.tamgcn_guidance_parts(0, 1, 1, 2) == -1
