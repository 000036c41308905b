"""-m gpu: the paired GEMM forms of MS-TCN's entry convolutions and plain 1x1 branch (tamgcn_conv_pair, tamgcn_wgrad_pair).

  forward         the row split is bit-identical to the two tamgcn_conv launches (outputs and moment partials), writes nothing
                  else, and meets the fp64 rounding bar of L = Cin;
  weight gradient per parameter tensor against the fp64 reference, L = N T V, with one and with several splits; bit-identical
                  to the two tamgcn_wgrad launches at their common split count;
  module          one MultiScale_TemporalConv forward + backward with the switch on and off: it dispatches the bit-identical
                  forms only (the data gradient stays two launches), so everything is bit-equal.

Shapes (N, Cin, Cb, T, V), two dilated branches (Ch = 3 Cb stacked entry rows, Cout = 4 Cb):
  (3, 64, 16, 20, 20)   split inside a 64-row tile (48 | 16), two frame tiles with a partial last one (400 columns > 320),
                        N * ntt = 6: the plain workgroup mapping
  (8, 128, 32, 9, 20)   N * ntt = 8: the XCD mapping; odd T; two channel tiles, the split inside the second (96 = 64 + 32)
  (2, 256, 64, 16, 20)  four channel tiles, the split on a tile boundary; 16 chunks of the contraction, beyond the
                        three-stage ring"""
import copy
import ctypes as C

import pytest
import torch

import fp64_bars as B

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64, 16, 20, 20), (8, 128, 32, 9, 20), (2, 256, 64, 16, 20)]
IDS = ['n3_c64_t20', 'n8_c128_t9', 'n2_c256_t16']


def _rand(gen, *shape, scale=1.0):
    return (torch.rand(shape, generator=gen) * 2 - 1) * scale


@pytest.fixture(scope='module', params=SHAPES, ids=IDS)
def prob(request):
    """Seeded operands of one shape on the CPU (references) and on the GPU; shared by the tests, never written."""
    from tam_gcn_amd import ops
    N, Cin, Cb, T, V = request.param
    Ch, Cout = 3 * Cb, 4 * Cb
    gen = torch.Generator().manual_seed(1000 + Cin + T)
    c = dict(N=N, Cin=Cin, Cb=Cb, T=T, V=V, Ch=Ch, Cout=Cout)
    c['g'] = _rand(gen, N, Cin, T, V)
    c['Win'], c['Wl'] = _rand(gen, Ch, Cin, 1, 1, scale=0.25), _rand(gen, Cb, Cin, 1, 1, scale=0.25)
    c['bin'], c['bl'] = _rand(gen, Ch), _rand(gen, Cb)
    c['cat0'] = _rand(gen, N, Cout, T, V)                       # what cat_pre holds before the launch
    # the backward's operands: two-source BatchNorm-backward prologues with their own coefficient tables
    c['dh'], c['h_pre'], c['coefb_h'] = _rand(gen, N, Ch, T, V), _rand(gen, N, Ch, T, V), _rand(gen, 3, Ch)
    c['dz'], c['cat_pre'], c['coefb_c'] = _rand(gen, N, Cout, T, V), _rand(gen, N, Cout, T, V), _rand(gen, 3, Cout)
    dev = torch.device('cuda:0')
    d = {}
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            d[k] = ops.empty(*v.shape, like=torch.empty(0, device=dev)) if v.dim() == 4 else torch.empty(v.shape, device=dev)
            d[k].copy_(v)
    c['dev'] = d
    c['gyh'] = dict(x1=c['dh'], x2=c['h_pre'], coef=c['coefb_h'], coff=0)
    c['gcat'] = dict(x1=c['dz'], x2=c['cat_pre'], coef=c['coefb_c'], coff=Ch)
    return c


@pytest.fixture
def mode(request):
    from tam_gcn_amd import _lib
    lib = _lib.load()
    before = lib.tamgcn_get_split_mode()
    lib.tamgcn_set_split_mode(request.param)
    yield request.param
    lib.tamgcn_set_split_mode(before)


def _last_kernel():
    from tam_gcn_amd import _lib
    return _lib.load().tamgcn_last_kernel().decode()


def test_forward_row_split_is_bit_identical_to_two_launches(prob):
    from tam_gcn_amd import ops, _lib
    from tam_gcn_amd.ops import S
    p, d = prob, prob['dev']
    N, Cin, Cb, T, V, Ch, Cout = (p[k] for k in ('N', 'Cin', 'Cb', 'T', 'V', 'Ch', 'Cout'))
    gs = S(d['g'])
    # the two launches of the parent path
    cat_t = ops.empty_like(d['cat0']); cat_t.copy_(d['cat0'])
    h_t, hpart_t = ops.conv(gs, K=Cin, w=d['Win'], bias=d['bin'], M=Ch, stats=True)
    assert _last_kernel() == 'conv1x1_glds_kernel<1, 16, false, 8>'
    _, lpart_t = ops.conv(gs, K=Cin, w=d['Wl'], bias=d['bl'], M=Cb, y=cat_t, ycoff=Ch, stats=True)
    # one launch
    cat_p = ops.empty_like(d['cat0']); cat_p.copy_(d['cat0'])
    h_p, hpart_p, y1, lpart_p = ops.conv_pair(gs, d['Win'], d['Wl'], bias0=d['bin'], bias1=d['bl'], y1=cat_p, ycoff1=Ch,
                                              stats=True)
    assert _last_kernel() == 'conv1x1_glds_kernel<1, 16, false, 8, 1>'
    torch.cuda.synchronize()
    assert y1 is cat_p
    # the partial count is that of the single descriptor with the stacked rows, and of each of the two launches
    cd = _lib.ConvDesc()
    cd.src = gs.c()
    cd.N, cd.K, cd.T_in, cd.V, cd.M, cd.KT, cd.dil, cd.stride, cd.up = N, Cin, T, V, Cout, 1, 1, 1, 1
    cd.T_out, cd.T_y, cd.ostride = T, T, 1
    nparts = _lib.load().tamgcn_conv_nparts(C.byref(cd))
    assert nparts == hpart_p.shape[2] == lpart_p.shape[2] == hpart_t.shape[2] == lpart_t.shape[2]
    assert tuple(hpart_p.shape) == (2, Ch, nparts) and tuple(lpart_p.shape) == (2, Cout, nparts)
    assert torch.equal(h_p, h_t), 'h_pre differs from the single launch'
    assert torch.equal(cat_p, cat_t), 'cat_pre differs from the single launch'
    assert torch.equal(hpart_p, hpart_t), 'entry moment partials differ'
    assert torch.equal(lpart_p[:, Ch:], lpart_t[:, Ch:]), 'plain-branch moment partials differ'
    keep = torch.ones(p['cat0'].shape, dtype=torch.bool)
    keep[:, Ch:] = False
    B.check_untouched('cat_pre[:, :Ch]', cat_p, p['cat0'], keep)
    # fp64
    src = dict(x1=p['g'])
    q0 = dict(src=src, K=Cin, M=Ch, w=p['Win'], bias=p['bin'], y0=torch.zeros(N, Ch, T, V), T_out=T)
    q1 = dict(src=src, K=Cin, M=Cb, w=p['Wl'], bias=p['bl'], y0=p['cat0'], ycoff=Ch, T_out=T)
    for name, q, got in (('h_pre', q0, h_p), ('cat_pre', q1, cat_p)):
        ref, _, _ = B.conv_eval(q)
        mag, _, _ = B.conv_eval(q, absval=True)
        err = B.check(name, got, ref, mag, Cin)
        print(f'{name}: max |err| {err:.3g}')


@pytest.mark.parametrize('mode', [0, 1], indirect=True)
@pytest.mark.parametrize('nsplit', [1, None], ids=['nsplit1', 'nsplit_auto'])
def test_weight_gradient_row_split_meets_the_fp64_bar(prob, mode, nsplit):
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    p, d = prob, prob['dev']
    N, Cin, Cb, T, V, Ch = (p[k] for k in ('N', 'Cin', 'Cb', 'T', 'V', 'Ch'))
    gyh = S(d['dh'], d['h_pre'], d['coefb_h'])
    gcat = S(d['dz'], d['cat_pre'], d['coefb_c'], coff=Ch)
    seen = {}
    real = ops.reduce_sum

    def spy(part, ns, *a, **kw):
        seen['nsplit'], seen['sym'] = ns, _last_kernel()           # the launch that filled `part`
        return real(part, ns, *a, **kw)
    ops.reduce_sum = spy
    try:
        outs = ops.wgrad_pair(gyh, gcat, S(d['g']), Ch, Cb, Cin, rows=[Cb] * 4, nsplit=nsplit)
    finally:
        ops.reduce_sum = real
    sym = seen['sym']
    torch.cuda.synchronize()
    assert (seen['nsplit'] == 1) if nsplit == 1 else (seen['nsplit'] > 1), seen
    assert len(outs) == 4 and all(tuple(o.shape) == (Cb, Cin, 1, 1) for o in outs)
    src = dict(x1=p['g'])
    refs = torch.cat([B.wgrad_eval(p['gyh'], src, Ch, Cin), B.wgrad_eval(p['gcat'], src, Cb, Cin)])
    mags = torch.cat([B.wgrad_eval(p['gyh'], src, Ch, Cin, absval=True), B.wgrad_eval(p['gcat'], src, Cb, Cin, absval=True)])
    for i, o in enumerate(outs):
        sl = slice(i * Cb, (i + 1) * Cb)
        err = B.check(f'dW[{i}]', o.view(Cb, Cin, 1), refs[sl], mags[sl], N * T * V, split=(mode == 1))
        print(f'dW[{i}] ({sym}): max |err| {err:.3g}')
    assert sym.startswith('wgrad_glds_kernel<') and sym.endswith(' pair') and (', split, ' in sym) == (mode == 1)


def _run_module(m, x, dout):
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), xg.grad, {k: v.grad for k, v in m.named_parameters()}, {k: v.clone() for k, v in m.named_buffers()}


def test_module_forward_and_backward_with_the_switch_on_and_off(monkeypatch):
    """The module dispatches only the paired forms that reproduce the two launches bit for bit (the forward row split and the
    weight-gradient row split at an equal split count; the data gradient stays two launches): outputs, running statistics
    and EVERY gradient are bit-equal with the switch on and off -- zero, inside any sum of fp64 bars."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.models import ctrgcn as M
    N, Cin, Cb, T, V = SHAPES[0]
    dev = torch.device('cuda:0')
    torch.manual_seed(7)
    m_on = M.MultiScale_TemporalConv(Cin, 4 * Cb, kernel_size=5, dilations=[1, 2], residual=False).to(dev).train()
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for prm in m_on.parameters():                            # biases and norms off their initial constants
            prm.add_(_rand(gen, *prm.shape, scale=0.1).to(dev))
    m_off = copy.deepcopy(m_on)
    x = _rand(gen, N, Cin, T, V).to(dev)
    dout = _rand(gen, N, 4 * Cb, T, V).to(dev)

    rec = []
    real_conv_pair, real_wgrad_pair = ops.conv_pair, ops.wgrad_pair

    def conv_pair(*a, **kw):
        rec.append(('conv', None))
        return real_conv_pair(*a, **kw)

    def wgrad_pair(*a, **kw):
        rec.append(('wgrad', kw.get('nsplit')))
        return real_wgrad_pair(*a, **kw)
    monkeypatch.setattr(ops, 'TCN_PAIR', True)
    monkeypatch.setattr(ops, 'conv_pair', conv_pair)
    monkeypatch.setattr(ops, 'wgrad_pair', wgrad_pair)
    out_on, dx_on, g_on, b_on = _run_module(m_on, x, dout)
    assert [r[0] for r in rec] == ['conv', 'wgrad'] and rec[1][1], f'paired launches of the run: {rec}'
    monkeypatch.setattr(ops, 'TCN_PAIR', False)
    out_off, dx_off, g_off, b_off = _run_module(m_off, x, dout)
    assert len(rec) == 2, 'TCN_PAIR = 0 still took a paired path'

    assert torch.equal(out_on, out_off)
    for k in b_on:
        assert torch.equal(b_on[k], b_off[k]), k
    assert torch.equal(dx_on, dx_off), 'dg differs'
    for k in g_on:
        assert torch.equal(g_on[k], g_off[k]), f'{k}: gradient differs from the two-launch run'


def test_weight_gradient_pair_is_bit_identical_at_the_single_launches_split_count(prob):
    """wgrad_pair_nsplit() names the split count all three launches share (or None); at it every parameter tensor of the
    paired launch holds the bits of its single launch -- also where the tile heights differ (128 rows against 64 at Cb = 32)."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    p, d = prob, prob['dev']
    Cin, Cb, Ch = p['Cin'], p['Cb'], p['Ch']
    gyh = S(d['dh'], d['h_pre'], d['coefb_h'])
    gcat = S(d['dz'], d['cat_pre'], d['coefb_c'], coff=Ch)
    gs = S(d['g'])
    ns = ops.wgrad_pair_nsplit(gyh, gcat, gs, Ch, Cb, Cin)
    assert ns is not None and ns >= 1, 'the three launches of this shape cut the contraction alike'
    outs = ops.wgrad_pair(gyh, gcat, gs, Ch, Cb, Cin, rows=[Cb] * 4, nsplit=ns)
    win = ops.wgrad(gyh, gs, M=Ch, K=Cin, rows=[Cb] * 3)
    wl = ops.wgrad(gcat, gs, M=Cb, K=Cin)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(outs[i], win[i]), f'entry branch {i}'
    assert torch.equal(outs[3], wl), 'plain branch'
