"""-m gpu: ReLU sign bits through the raw ops layer -- every comparison is exact (bit for bit).

  forward    tamgcn_gcn_tail_fwd_bits / tamgcn_add_act_fwd_bits (plain, row-mean and frame-mean forms): the bits equal
             `out > 0` in the layout of tests/test_signbits_cpu.py, and every other output holds the bits of the call without
             the bit pointer;
  backward   tamgcn_gcn_tail_bwd_bits form (a) (fed an already masked dsum) and form (b) (dg + bits), tamgcn_add_act_bwd_bits:
             outputs and moment slabs equal today's entry points on the same data;
  epilogue   tamgcn_conv_signmask == tamgcn_conv followed by where(bit, y, 0);
  defects    a bit array one group late, `>= 0` for `> 0`, a mask applied before add1: each built in this file's reference,
             each must break at least one comparison.

Geometries (N, C, T, V):
  (2, 5, 2, 20)    10 rows of 10 sixteen-byte steps: 16 lanes a row, the rows do not fill a workgroup
  (2, 24, 4, 20)   whole groups of four, three workgroups
  (3, 7, 3, 25)    L = 75: a scalar tail of three and a partial last byte; rows that are not 16-byte aligned
  (2, 3, 90, 20)   450 steps: the whole workgroup walks one row"""
import numpy as np
import pytest
import torch

from test_signbits_cpu import pack_bits, unpack_bits, shift_one_group, special_values, row_bytes

pytestmark = pytest.mark.gpu

GEOS = [(2, 5, 2, 20), (2, 24, 4, 20), (3, 7, 3, 25), (2, 3, 90, 20)]
GIDS = ['rows_short_of_a_workgroup', 'whole_groups', 'L75_tail', 'whole_workgroup_rows']
DEV = 'cuda:0'


def same(a, b):
    """bit equality (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(t):
    from tam_gcn_amd import ops
    out = ops.empty(*t.shape, like=torch.empty(0, device=DEV)) if t.dim() == 4 else torch.empty(t.shape, device=DEV, dtype=t.dtype)
    out.copy_(t)
    return out


def _special_input(gen, shape):
    """Ordinary values of both signs with the edge values of the mask planted in every row (start, middle, the row's tail)."""
    x = torch.randn(shape, generator=gen)
    N, C, T, V = shape
    L = T * V
    flat = x.view(N, C, L)
    sp = torch.from_numpy(special_values())
    for r, pos in enumerate((0, L // 2, L - 1, L - 2, 1, L // 3, L - 3, 2)):
        flat[:, :, pos % L] = sp[r]
    return x


@pytest.fixture(scope='module', params=GEOS, ids=GIDS)
def geo(request):
    N, C, T, V = request.param
    gen = torch.Generator().manual_seed(31 + T * V)
    c = dict(shape=request.param)
    c['a'] = _special_input(gen, request.param)
    c['r'] = torch.zeros(request.param)                    # a residual of exact zeros keeps the planted values
    c['r'].view(N, C, -1)[:, :, 5::7] = torch.randn(N, C, len(range(5, T * V, 7)), generator=gen)
    c['rand'] = [torch.randn(request.param, generator=gen) for _ in range(4)]
    c['coef'] = torch.stack([torch.rand(C, generator=gen) + 0.5, torch.zeros(C), torch.randn(C, generator=gen) * 0.1])
    c['save'] = torch.randn(2, C, generator=gen)
    # value = 1 * a + 1 * (-0.0) + (-0.0) = a bit for bit, -0.0 included (the one-source prologue adds a +0.0, which loses that sign)
    c['negz'] = torch.full(request.param, -0.0)
    c['coef_id'] = torch.stack([torch.ones(C), torch.ones(C), torch.full((C,), -0.0)])
    c['dev'] = {k: _dev(v) for k, v in c.items() if isinstance(v, torch.Tensor)}
    c['dev']['rand'] = [_dev(t) for t in c['rand']]
    return c


def _exact(d):
    from tam_gcn_amd.ops import S
    return S(d['a'], d['negz'], d['coef_id'])


def _check_bits(bits, out, T, V):
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    b = bits.cpu().numpy()
    assert b.shape == (o.shape[0], o.shape[1], row_bytes(T * V))
    assert np.array_equal(b, pack_bits(o)), 'bits != (out > 0) in the layout'
    with np.errstate(invalid='ignore'):
        assert np.array_equal(unpack_bits(b, T, V), o > 0)
    return o, b


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('has_res', [0, 1])
def test_gcn_tail_fwd_bits(geo, has_res):
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    d = geo['dev']
    N, C, T, V = geo['shape']
    zero = torch.zeros_like(d['a'])                        # tanh(0) = 0: g = relu(a + res) keeps the planted values
    res = S(d['r']) if has_res else None
    g0 = ops.gcn_tail_fwd(S(d['a']), S(zero), res)
    sign = []
    g1 = ops.gcn_tail_fwd(S(d['a']), S(zero), res, sign=sign)
    assert len(sign) == 1 and sign[0].dtype == torch.uint8
    o, b = _check_bits(sign[0], g1, T, V)
    assert same(g0, g1)
    assert (o == 0).any() and (o > 0).any()
    # an ordinary operand pair too (prologue coefficients, tanh at work)
    sign2 = []
    y, ob = S(d['rand'][0], coef=d['coef']), S(d['rand'][1], coef=d['coef'])
    g2 = ops.gcn_tail_fwd(y, ob, res, sign=sign2)
    _check_bits(sign2[0], g2, T, V)
    assert same(g2, ops.gcn_tail_fwd(y, ob, res))
    # defects: each reference variant must differ from what the kernel wrote
    assert not np.array_equal(b, pack_bits(o, ge=True)), '`>= 0` would pass'
    assert not np.array_equal(b, shift_one_group(pack_bits(o))), 'a bit array one group late would pass'


@pytest.mark.parametrize('has_res', [0, 1])
@pytest.mark.parametrize('form', ['plain', 'rowmean', 'xbar'])
def test_add_act_fwd_bits(geo, form, has_res):
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    d = geo['dev']
    N, C, T, V = geo['shape']
    kw = dict(rowmean=True) if form == 'rowmean' else dict(xbar=True) if form == 'xbar' else {}
    res = S(d['r']) if has_res else None

    def run(a, relu, sign):
        r = ops.add_act_fwd(a, res, relu, C, sign=sign, **kw)
        return r if isinstance(r, tuple) else (r,)
    for a in (_exact(d), S(d['rand'][0], coef=d['coef'])):
        ref = run(a, 1, None)
        sign = []
        got = run(a, 1, sign)
        assert len(sign) == 1
        o, b = _check_bits(sign[0], got[0], T, V)
        assert len(got) == len(ref) and all((x is None and y is None) or same(x, y) for x, y in zip(got, ref)), form
        if form == 'xbar':                                 # V % 4 != 0: no frame means, the plain kernel (ops.add_act_fwd)
            assert (got[1] is None) if V % 4 else tuple(got[1].shape) == (C, N, V)
    assert not np.array_equal(b, shift_one_group(pack_bits(o)))
    # relu = 0 produces no bits and is the call it was
    sign = []
    got = run(S(d['a']), 0, sign)
    assert sign == []
    assert all((x is None and y is None) or same(x, y) for x, y in zip(got, run(S(d['a']), 0, None)))
    torch.cuda.synchronize()
    assert (got[0].cpu().view(-1)[~torch.isnan(got[0].cpu().view(-1))] < 0).any()


def test_zero_signs_denormal_and_nan_reach_the_output(geo):
    """relu = 0 passes the planted values through: the bits of THAT tensor, taken by the relu = 1 kernel's test `> 0`, are what
    the numpy layout says for +0.0, -0.0, a denormal and a NaN (the relu form itself maps NaN and -0.0 to a zero)."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    d = geo['dev']
    N, C, T, V = geo['shape']
    out = ops.add_act_fwd(_exact(d), None, 0, C)
    torch.cuda.synchronize()
    o = out.cpu()
    nan = torch.isnan(geo['a'])
    assert torch.equal(torch.isnan(o), nan) and same(o.masked_fill(nan, 0.0), geo['a'].masked_fill(nan, 0.0))
    v = o.view(N, C, -1)[0, 0]
    assert torch.isnan(v).any() and (v == 0).any() and ((v > 0) & (v < 1e-38)).any() and torch.signbit(v[v == 0]).any()
    sign = []
    out1 = ops.add_act_fwd(_exact(d), None, 1, C, sign=sign)
    o1, b = _check_bits(sign[0], out1, T, V)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(unpack_bits(b, T, V), geo['a'].numpy() > 0)      # relu keeps exactly the elements > 0


# ---------------------------------------------------------------------------------------------------------------------
# backward forms
# ---------------------------------------------------------------------------------------------------------------------
def _relu_like(geo):
    """An activation as a forward leaves it (zeros where the ReLU cut) and its bits."""
    g = torch.clamp(geo['a'].nan_to_num(0.0), min=0.0)
    return g, torch.from_numpy(pack_bits(g.numpy()))


def test_gcn_tail_bwd_forms(geo):
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    d = geo['dev']
    N, C, T, V = geo['shape']
    g, bits = _relu_like(geo)
    gd, bd = _dev(g), bits.to(DEV)
    dg, o_pre = d['rand'][0], d['rand'][1]
    o = S(o_pre, coef=d['coef'])
    dsum0, doz0, part0 = ops.gcn_tail_bwd(dg, gd, o, d['save'])
    # (b): dg + bits
    dsum_b, doz_b, part_b = ops.gcn_tail_bwd_bits(dg, bd, o, d['save'])
    assert same(dsum_b, dsum0) and same(doz_b, doz0) and same(part_b, part0)
    # (a): an already masked dsum; g is not read, dsum is not written
    pre = _dev(torch.where(g > 0, geo['rand'][0], torch.zeros(())))
    dsum_a, doz_a, part_a = ops.gcn_tail_bwd_bits(pre, None, o, d['save'])
    assert dsum_a is pre and same(doz_a, doz0) and same(part_a, part0)
    torch.cuda.synchronize()
    assert same(pre, dsum0)
    # defects in the reference: bits one group late / `>= 0` would change dsum
    late = torch.from_numpy(shift_one_group(bits.numpy())).to(DEV)
    ge = torch.from_numpy(pack_bits(g.numpy(), ge=True)).to(DEV)
    assert not same(ops.gcn_tail_bwd_bits(dg, late, o, d['save'])[0], dsum0)
    assert not same(ops.gcn_tail_bwd_bits(dg, ge, o, d['save'])[0], dsum0)


@pytest.mark.parametrize('with_r', [False, True])
@pytest.mark.parametrize('want_dz', [False, True])
def test_add_act_bwd_bits(geo, with_r, want_dz):
    from tam_gcn_amd import ops
    d = geo['dev']
    g, bits = _relu_like(geo)
    gd, bd = _dev(g), bits.to(DEV)
    dout, a_pre = d['rand'][0], d['rand'][1]
    r_pre = d['rand'][2] if with_r else None
    r_save = d['save'] if with_r else None
    dz0, part0 = ops.add_act_bwd(dout, gd, 1, a_pre, d['save'], r_pre, r_save, want_dz=want_dz)
    dz1, part1 = ops.add_act_bwd_bits(dout, bd, a_pre, d['save'], r_pre, r_save, want_dz=want_dz)
    assert part1.shape[0] == (4 if with_r else 2) and same(part1, part0)
    assert (dz1 is None and dz0 is None) if not want_dz else same(dz1, dz0)
    late = torch.from_numpy(shift_one_group(bits.numpy())).to(DEV)
    assert not same(ops.add_act_bwd_bits(dout, late, a_pre, d['save'], r_pre, r_save, want_dz=False)[1], part0)


# ---------------------------------------------------------------------------------------------------------------------
# the 1x1 GEMM's epilogue
# ---------------------------------------------------------------------------------------------------------------------
def _last_kernel():
    from tam_gcn_amd import _lib
    return _lib.load().tamgcn_last_kernel().decode()


EPI = [(K, M, T, coff) for K in (16, 64) for M in (64, 48) for T in (16, 20) for coff in (0, 8)]


@pytest.fixture(scope='module')
def epi_rand():
    gen = torch.Generator().manual_seed(77)
    N, V, Kmax, Mmax, Tmax = 2, 20, 64, 64, 20
    return dict(dz=torch.randn(N, Kmax + 16, Tmax, V, generator=gen), cat=torch.randn(N, Kmax + 16, Tmax, V, generator=gen),
                coef=torch.randn(3, Kmax + 16, generator=gen), w=torch.randn(Kmax, Mmax, 1, 1, generator=gen) * 0.25,
                dg0=torch.randn(N, Mmax, Tmax, V, generator=gen), m=torch.randn(N, Mmax + 8, Tmax, V, generator=gen))


def _epi_run(r, K, M, T, coff, bits=None, kind='random'):
    """(masked launch, plain launch, the bits used, on-mask): y = add1 in place, two-source prologue, source slice at channel 16."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, V = 2, 20
    dz, cat = _dev(r['dz'][:, :K + 16, :T].contiguous()), _dev(r['cat'][:, :K + 16, :T].contiguous())
    coef = r['coef'][:, :K + 16].contiguous().to(DEV)
    w = r['w'][:K, :M].contiguous().to(DEV)
    src = S(dz, cat, coef, coff=16)
    mref = r['m'][:, :M + coff, :T].contiguous()
    if kind == 'zeros':
        mref = -mref.abs()
    elif kind == 'ones':
        mref = mref.abs() + 1.0
    if bits is None:
        bits = torch.from_numpy(pack_bits(mref.numpy()))
    y_plain = _dev(r['dg0'][:, :M, :T].contiguous())
    ops.conv(src, K=K, w=w, bias=None, M=M, wmode=1, y=y_plain, add1=y_plain)
    assert _last_kernel() == 'conv1x1_glds_kernel<2, 8, true, 8>'
    y_mask = _dev(r['dg0'][:, :M, :T].contiguous())
    ops.conv(src, K=K, w=w, bias=None, M=M, wmode=1, y=y_mask, add1=y_mask, sign=bits.to(DEV), sign_coff=coff)
    assert _last_kernel() == 'conv1x1_glds_kernel<2, 8, true, 8, 2>'
    torch.cuda.synchronize()
    on = (mref > 0)[:, coff:coff + M]
    return y_mask.cpu(), y_plain.cpu(), bits, on


@pytest.mark.parametrize('K,M,T,coff', EPI, ids=[f'K{k}_M{m}_T{t}_off{c}' for k, m, t, c in EPI])
def test_epilogue_sign_mask(epi_rand, K, M, T, coff):
    y_mask, y_plain, bits, on = _epi_run(epi_rand, K, M, T, coff)
    assert on.any() and not on.all()
    assert same(y_mask, torch.where(on, y_plain, torch.zeros(())))
    # defect: the mask applied before add1 leaves add1 where the bit is 0
    before = torch.where(on, y_plain, epi_rand['dg0'][:, :M, :T])
    assert not same(y_mask, before)
    # defect: a bit array one group late
    late_on = torch.from_numpy(unpack_bits(shift_one_group(bits.numpy()), T, 20))[:, coff:coff + M]
    assert not same(y_mask, torch.where(late_on, y_plain, torch.zeros(())))


@pytest.mark.parametrize('kind', ['zeros', 'ones'])
def test_epilogue_all_bits_equal(epi_rand, kind):
    y_mask, y_plain, bits, on = _epi_run(epi_rand, 16, 48, 20, 8, kind=kind)
    if kind == 'zeros':
        assert not on.any() and not y_mask.any()
    else:
        assert on.all() and same(y_mask, y_plain)


def test_epilogue_refuses_what_it_does_not_serve():
    """One source, V % 4 != 0, a strided output: the library refuses, it does not run another kernel."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    gen = torch.Generator().manual_seed(5)
    N, K, M, T = 2, 16, 64, 8
    for V, two, ostride in ((20, False, 1), (25, True, 1), (20, True, 2)):
        x1, x2 = _dev(torch.randn(N, K, T, V, generator=gen)), _dev(torch.randn(N, K, T, V, generator=gen))
        coef = torch.randn(3, K, generator=gen).to(DEV)
        w = torch.randn(K, M, 1, 1, generator=gen).to(DEV)
        y = ops.zeros_like(_dev(torch.zeros(N, M, T * ostride, V)))
        bits = torch.zeros(N, M, row_bytes(T * ostride * V), dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError, match='tamgcn_conv_signmask'):
            ops.conv(S(x1, x2 if two else None, coef if two else None), K=K, w=w, bias=None, M=M, wmode=1, y=y, T_out=T,
                     ostride=ostride, add1=y, sign=bits)
    torch.cuda.synchronize()
