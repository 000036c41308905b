"""-m gpu: every entry point of include/tamgcn_xmodal.h alone against the fp64 restatement tests/crossmodal_ref.py, teacher-forced:
each stage gets fp32 inputs on the device -- the device's own results of the stage before -- and the reference is evaluated in
fp64 on exactly those.  Bars: fp64_bars.check with the contraction length of the stage and the allowances derived in
crossmodal_ref's docstring (BatchNorm statistics from their own N-term sums; the sigmoid a quarter of its pre-activation's bar plus
SIGMOID_ALLOW, twice the error of the device's 1 / (1 + expf(-z)) measured on a dense grid below).  Every output lies in a
poisoned buffer that must come back untouched outside the payload.  profiles/xmodal_stage_bars.txt keeps one run's maxima
(pytest -s prints them)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crossmodal_ref as R                              # noqa: E402
import fp64_bars as B                                   # noqa: E402
from tam_gcn_amd import _xm_lib                         # noqa: E402

DEV = 'cuda:0'
PAD = 64
POISON = -7777.25
MOM, EPS = 0.1, 1e-5


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


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    _xm_lib.check(rc, what)


def run_chain(shape, seed, training, shift=0, want_df=True, want_dfrgb=True, rgb_shift=0):
    """every stage once, each fed the device results of the one before; returns the problem and {name: device tensor}"""
    lib = _xm_lib.load()
    N, D, Hd, Rr, P, K = shape
    p, f, f_rgb, _ = R.make_problem(shape, seed)
    gen = torch.Generator().manual_seed(seed + 100)
    dg = (torch.randn(N, Rr, generator=gen) / N).to(DEV)
    d = {k: v.to(DEV) for k, v in p.items()}
    fd = f.to(DEV)
    rgb_buf = torch.zeros(f_rgb.numel() + 8, device=DEV)
    rgb = rgb_buf[rgb_shift:rgb_shift + f_rgb.numel()].view(f_rgb.shape)
    rgb.copy_(f_rgb)
    assert rgb.data_ptr() % 16 == 4 * rgb_shift
    o = {k: Guarded(s) for k, s in dict(a1=(N, Hd), xhat=(N, Hd), mean=(Hd,), invstd=(Hd,), att=(N, Rr), m=(N, Rr), g=(N, Rr), dz2=(N, Rr),
                                         dW2=(Rr, Hd), db2=(Rr,), da1=(N, Hd), dgamma=(Hd,), dbeta=(Hd,), dW1=(Hd, D), db1=(Hd,),
                                         dz1=(N, Hd), df=(N, D)).items()}
    o['df_rgb'] = Guarded((N, Rr, P, 1), shift)
    rm, rv, nbt = d['rmean'].clone(), d['rvar'].clone(), d['nbt'].clone()
    _ok(lib.tamgcn_xm_hidden_fwd(fd.data_ptr(), d['W1'].data_ptr(), d['b1'].data_ptr(), d['gamma'].data_ptr(), d['beta'].data_ptr(), rm.data_ptr(),
                                 rv.data_ptr(), nbt.data_ptr(), N, D, Hd, int(training), MOM, EPS, o['a1'].ptr, o['xhat'].ptr, o['mean'].ptr,
                                 o['invstd'].ptr, _st()), 'hidden_fwd')
    _ok(lib.tamgcn_xm_gate_fwd(o['a1'].ptr, d['W2'].data_ptr(), d['b2'].data_ptr(), N, Hd, Rr, o['att'].ptr, _st()), 'gate_fwd')
    _ok(lib.tamgcn_xm_pool_fwd(rgb.data_ptr(), o['att'].ptr, N, Rr, P, o['m'].ptr, o['g'].ptr, _st()), 'pool_fwd')
    _ok(lib.tamgcn_xm_pool_bwd(dg.data_ptr(), o['m'].ptr, o['att'].ptr, N, Rr, P, o['dz2'].ptr, o['df_rgb'].ptr if want_dfrgb else None, _st()),
        'pool_bwd')
    _ok(lib.tamgcn_xm_gate_bwd(o['dz2'].ptr, o['a1'].ptr, d['W2'].data_ptr(), N, Hd, Rr, o['dW2'].ptr, o['db2'].ptr, o['da1'].ptr, _st()), 'gate_bwd')
    _ok(lib.tamgcn_xm_hidden_bwd(o['da1'].ptr, o['a1'].ptr, o['xhat'].ptr, o['invstd'].ptr, d['gamma'].data_ptr(), fd.data_ptr(), d['W1'].data_ptr(),
                                 N, D, Hd, int(training), o['dgamma'].ptr, o['dbeta'].ptr, o['dW1'].ptr, o['db1'].ptr, o['dz1'].ptr,
                                 o['df'].ptr if want_df else None, _st()), 'hidden_bwd')
    torch.cuda.synchronize()
    skip = ([] if want_df else ['df']) + ([] if want_dfrgb else ['df_rgb'])
    got = {k: g.get(k) for k, g in o.items() if k not in skip}
    for k in skip:                                             # not asked for: not one element written
        assert torch.equal(o[k].buf, o[k].before), k
    got.update(running_mean=rm, running_var=rv, num_batches_tracked=nbt, dg=dg, f=fd, f_rgb=rgb)
    return (p, f, f_rgb), got


def check_chain(shape, seed, training, tag):
    N, D, Hd, Rr, P, K = shape
    (p, f, f_rgb), g = run_chain(shape, seed, training)
    worst = {}

    def chk(name, ref, L, gb=True):
        r, mag = ref[0], ref[1]
        allow = ref[2] if len(ref) > 2 else 0.0
        e = B.check(f'{tag}: {name}', g[name], r, mag, L, global_bound=gb and len(ref) == 2, allow=allow)
        lim = B.elementwise_bar(L, mag) + allow
        worst[name] = float(((g[name].double().cpu() - r).abs() / lim.clamp_min(1e-300)).max()) if torch.is_tensor(lim) and lim.dim() else e
    h = R.hidden_fwd(f, p['W1'], p['b1'], p['gamma'], p['beta'], p['rmean'], p['rvar'], p['nbt'], training, MOM, EPS)
    chk('mean', h['mean'], N)
    for k in ('invstd', 'xhat', 'a1', 'running_mean', 'running_var'):
        chk(k, h[k], 0)
    assert int(g['num_batches_tracked']) == h['num_batches_tracked'] == 3 + int(training)
    if not training:
        assert torch.equal(g['running_mean'].cpu(), p['rmean']) and torch.equal(g['running_var'].cpu(), p['rvar'])
    chk('att', R.gate_fwd(g['a1'], p['W2'], p['b2'])['att'], 0)
    pf = R.pool_fwd(g['f_rgb'], g['att'])
    chk('m', pf['m'], P)
    chk('g', pf['g'], P)
    pb = R.pool_bwd(g['dg'], g['m'], g['att'], P, (N, Rr, P, 1))
    chk('dz2', pb['dz2'], 1)
    chk('df_rgb', pb['df_rgb'], 1)
    gbw = R.gate_bwd(g['dz2'], g['a1'], p['W2'])
    chk('dW2', gbw['dW2'], N)
    chk('db2', gbw['db2'], N)
    chk('da1', gbw['da1'], Rr)
    hb = R.hidden_bwd(g['da1'], g['a1'], g['xhat'], g['invstd'], p['gamma'], f, p['W1'], training, dz1_dev=g['dz1'])
    chk('dbeta', hb['dbeta'], N)
    chk('dgamma', hb['dgamma'], N)
    chk('dz1', hb['dz1'], 4)
    chk('dW1', hb['dW1'], N)
    chk('db1', hb['db1'], N, gb=False)                       # the batch formula centres dz1: its sum is rounding noise around 0
    chk('df', hb['df'], Hd)
    print(f'\nxmodal_stage_bars {tag:34s} ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()) + '   (largest err / bar)')


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('shape', R.STAGE_SHAPES[:4], ids=lambda s: 'x'.join(map(str, s)))
def test_stages_against_the_fp64_reference(shape, training):
    check_chain(shape, seed=21, training=training, tag=f'{"x".join(map(str, shape))} {"train" if training else "eval"}')


def test_stages_at_the_configured_workload():
    check_chain(R.STAGE_SHAPES[4], seed=22, training=True, tag='16x256x1024x2048x49x10 train')


def test_eval_at_one_clip_and_train_at_one_clip_is_refused():
    check_chain((1, 8, 20, 40, 49, 3), seed=23, training=False, tag='1x8x20x40x49x3 eval')
    lib = _xm_lib.load()
    q = torch.zeros(64, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    a = q.data_ptr()
    assert lib.tamgcn_xm_hidden_fwd(a, a, a, a, a, a, a, nbt.data_ptr(), 1, 4, 4, 1, MOM, EPS, a, a, a, a, None) == -1
    assert b'N >= 2' in lib.tamgcn_xm_last_error()
    assert lib.tamgcn_xm_hidden_bwd(a, a, a, a, a, a, a, 1, 4, 4, 1, a, a, a, a, a, None, None) == -1
    torch.cuda.synchronize()
    assert float(q.abs().max()) == 0.0 and int(nbt) == 0


@pytest.mark.parametrize('shape', [(17, 64, 36, 72, 49, 10), (33, 256, 128, 256, 50, 10), (3, 8, 20, 40, 3, 3)], ids=lambda s: f'P{s[4]}')
def test_optional_outputs_alignment_and_repeatability(shape):
    """df_rgb = NULL and df = NULL leave every other result bit-equal; df_rgb written at a dword-aligned address (a payload one float
    off its 16-byte alignment) and f_rgb read from one give the bits of the aligned call; two runs are bit-equal.  run_chain checks
    the poisoned margins of every output of every one of these calls."""
    _, a = run_chain(shape, 31, True)
    _, b = run_chain(shape, 31, True)
    for k in a:
        assert torch.equal(a[k], b[k]), f'{k}: two runs differ'
    _, c = run_chain(shape, 31, True, want_df=False, want_dfrgb=False)
    assert set(a) - set(c) == {'df', 'df_rgb'}
    for k in c:
        assert torch.equal(a[k], c[k]), f'{k} changes when df / df_rgb are not asked for'
    for shift, rgb_shift in ((1, 0), (0, 1), (3, 3), (2, 1)):
        _, s = run_chain(shape, 31, True, shift=shift, rgb_shift=rgb_shift)
        for k in a:
            assert torch.equal(a[k], s[k]), f'{k}: differs with df_rgb {shift} and f_rgb {rgb_shift} floats off 16-byte alignment'


def test_the_device_sigmoid_on_a_dense_grid():
    """1 / (1 + expf(-z)) of tamgcn_xm_gate_fwd against fp64 on 2^20 points of [-30, 30]: z = 1 * W2[r][0] + 0 is exact, so the
    error is the sigmoid's alone.  SIGMOID_ALLOW is twice the largest error this prints (profiles/xmodal_stage_bars.txt)."""
    lib = _xm_lib.load()
    Rr = 1 << 20
    z = torch.linspace(-30, 30, Rr, dtype=torch.float64).to(torch.float32)
    W2 = torch.zeros(Rr, 4)
    W2[:, 0] = z
    W2, b2 = W2.to(DEV), torch.zeros(Rr, device=DEV)
    a1 = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV)
    att = Guarded((1, Rr))
    _ok(lib.tamgcn_xm_gate_fwd(a1.data_ptr(), W2.data_ptr(), b2.data_ptr(), 1, 4, Rr, att.ptr, _st()), 'gate_fwd')
    got = att.get('att')[0].double().cpu()
    ref = 1.0 / (1.0 + torch.exp(-z.double()))
    err = (got - ref).abs()
    i = int(err.argmax())
    rel = float((err / ref).max())
    print(f'\nxmodal_stage_bars device sigmoid: max |err| {float(err.max()):.3e} at z = {float(z[i]):.4f}; max relative {rel:.3e}; '
          f'SIGMOID_ALLOW {R.SIGMOID_ALLOW:.3e}')
    assert 2 * float(err.max()) <= R.SIGMOID_ALLOW
    assert bool((got[1:] >= got[:-1]).all()) or float((got[:-1] - got[1:]).max()) <= 2 * R.U       # monotone up to one rounding
