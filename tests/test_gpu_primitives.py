"""-m gpu: each C-ABI primitive against a stock-PyTorch fp32 expression of the same
arithmetic (computed on the CPU), on small ragged shapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from params import make_input          # noqa: E402


def dev():
    return torch.device('cuda:0')


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return make_input(shape, seed, lo, hi)


def close(a, b, rtol=1e-4, atol=1e-5, msg=''):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=msg)


CONV_CASES = [
    # N, K, M, T, V, KT, dil, stride
    (2, 3, 64, 13, 20, 1, 1, 1),
    (2, 20, 24, 13, 20, 1, 1, 1),
    (3, 64, 192, 64, 20, 1, 1, 1),
    (2, 16, 16, 13, 20, 5, 1, 1),
    (2, 16, 16, 13, 20, 5, 2, 1),
    (2, 32, 32, 12, 20, 5, 2, 2),
    (2, 16, 16, 13, 20, 5, 1, 2),
    (2, 64, 128, 13, 20, 1, 1, 2),
    (3, 128, 256, 32, 20, 1, 1, 2),    # strided 1x1 on the LDS-DMA GEMM (round 4): one full 16-frame tile per clip
    (2, 64, 64, 35, 20, 1, 1, 2),      # ... 18 output frames: a full tile and a 2-frame one
    (2, 32, 48, 9, 64, 1, 1, 2),       # ... V = 64: 5 frames per tile
    (1, 70, 40, 9, 25, 1, 1, 1),
    (1, 16, 16, 12, 20, 9, 1, 1),
    (1, 12, 12, 11, 20, 3, 3, 1),
    (2, 64, 96, 40, 20, 1, 1, 1),      # two 48-row channel tiles, three frame tiles (staged epilogue overshoot)
    (2, 192, 64, 33, 20, 1, 1, 1),     # K = 6 chunks, ragged last frame tile
    (2, 48, 144, 16, 20, 1, 1, 1),
    # k x 1 weight gradients as tap windows of the LDS-DMA kernel (more than 16 channels, stride 1); rows whose windows
    # are not multiples of the 32-element chunk (overlapping last chunk), V = 25 (dword-aligned windows), V = 64
    (3, 32, 32, 16, 20, 5, 1, 1),
    (3, 64, 64, 16, 20, 5, 2, 1),
    (2, 64, 32, 13, 20, 5, 2, 1),
    (2, 64, 64, 11, 25, 5, 1, 1),
    (2, 32, 64, 9, 25, 5, 2, 1),
    (1, 64, 64, 12, 64, 5, 2, 1),
    (2, 40, 24, 14, 20, 3, 1, 1),
    (2, 24, 24, 10, 20, 9, 1, 1),
    (2, 64, 64, 5, 25, 5, 2, 1),       # T - pad = 1 frame: too short for a window, stays on the register-staged kernel
    (2, 48, 80, 7, 25, 1, 1, 1),       # 1x1, rows of 175 = 5 * 32 + 15 floats
    # 16-channel k x 1 at V = 25: the p-split weight-gradient kernel with 16-byte slots on dword-aligned rows (slots
    # straddling two frames, rows cut at both ends), chunk lengths 8 and 4 frames, T not a multiple of either
    (2, 64, 128, 13, 25, 1, 1, 2),     # strided 1x1 at V = 25: its data gradient writes every second frame from the LDS-DMA GEMM
    (3, 32, 128, 16, 20, 1, 1, 2),
    (2, 16, 16, 13, 25, 5, 1, 1),
    (2, 16, 16, 11, 25, 5, 2, 1),
    (3, 16, 12, 7, 25, 5, 1, 1),
    (1, 16, 16, 3, 25, 5, 2, 1),
]


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv_fwd_bwd_wgrad(case):
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, K, M, T, V, KT, dil, stride = case
    pad = (KT + (KT - 1) * (dil - 1) - 1) // 2
    x = rnd((N, K, T, V), 1).requires_grad_(True)
    w = (rnd((M, K, KT, 1), 2) * 0.2).requires_grad_(True)
    b = rnd((M,), 3).requires_grad_(True)
    y = F.conv2d(x, w, b, stride=(stride, 1), padding=(pad, 0), dilation=(dil, 1))
    cot = rnd(tuple(y.shape), 4)
    (y * cot).sum().backward()
    xd, wd, bd, cd = (t.detach().to(dev()) for t in (x, w, b, cot))
    yg, part = ops.conv(S(xd), K=K, w=wd, bias=bd, M=M, KT=KT, dil=dil, stride=stride, pad=pad, stats=True)
    close(yg, y, 1e-4, 1e-4, 'conv fwd')
    s1 = part[0].sum(-1)
    s2 = part[1].sum(-1)
    close(s1, y.sum((0, 2, 3)), 1e-3, 1e-2, 'stats sum')
    close(s2, (y * y).sum((0, 2, 3)), 1e-3, 1e-2, 'stats sumsq')
    T2 = y.shape[2]
    # data gradient
    if KT == 1:
        dx = torch.zeros_like(xd)
        ops.conv(S(cd), K=M, w=wd, bias=None, M=K, wmode=1, y=dx, T_out=T2, ostride=stride)
    else:
        dx, _ = ops.conv(S(cd), K=M, w=wd, bias=None, M=K, KT=KT, dil=dil, stride=1, pad=(KT - 1) * dil - pad,
                         wmode=1, up=stride, T_out=T)
    close(dx, x.grad, 1e-4, 1e-4, 'conv bwd data')
    dw = ops.wgrad(S(cd), S(xd), M=M, K=K, KT=KT, dil=dil, stride=stride, pad=pad)
    close(dw, w.grad, 1e-4, 2e-4, 'conv wgrad')


@pytest.mark.parametrize('shape', [(3, 96, 64, 8, 20, True, False), (2, 192, 128, 16, 20, True, True),
                                   (2, 64, 192, 32, 20, False, False), (5, 48, 40, 16, 20, False, True),
                                   (2, 160, 160, 8, 20, True, True), (1, 48, 64, 72, 20, True, False)])
def test_pointwise_dma_gemms_with_prologue(shape):
    """The LDS-DMA forms of the 1x1 conv and of its weight gradient (T*V % 32 == 0, K % 16 == 0) with
    two-source BatchNorm(-backward)-apply operands, ReLU and channel slices; fp64 torch reference."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, M, K, T, V, ytwo, xtwo = shape
    d = dev()
    ap = lambda c, a, b: c[0][None, :, None, None] * a + (c[1][None, :, None, None] * b if b is not None else 0) + c[2][None, :, None, None]
    Kt, Mt = K + 16, M + 32                                  # operands are channel slices of wider tensors
    x1, x2 = rnd((N, Kt, T, V), 1), (rnd((N, Kt, T, V), 2) if xtwo else None)
    cx = rnd((3, Kt), 3)
    g1, g2 = rnd((N, Mt, T, V), 4), (rnd((N, Mt, T, V), 5) if ytwo else None)
    cg = rnd((3, Mt), 6)
    xv = torch.relu(ap(cx.double(), x1.double(), None if x2 is None else x2.double()))[:, 16:16 + K]
    gv = ap(cg.double(), g1.double(), None if g2 is None else g2.double())[:, 32:32 + M]
    t = lambda z: None if z is None else z.to(d)
    xs = S(t(x1), t(x2), t(cx), coff=16, act=1)
    gs = S(t(g1), t(g2), t(cg), coff=32)
    dw = ops.wgrad(gs, xs, M=M, K=K)
    ref = torch.einsum('nmtv,nktv->mk', gv, xv)
    close(dw.view(M, K).double(), ref, 1e-4, 2e-4 * float(ref.abs().max()), 'wgrad (DMA)')
    # forward conv on the prologue'd x, and the data-gradient form on the prologue'd gy
    w = rnd((M, K, 1, 1), 7) * 0.1
    b = rnd((M,), 8)
    y, part = ops.conv(xs, K=K, w=t(w), bias=t(b), M=M, stats=True)
    yr = torch.einsum('mk,nktv->nmtv', w[:, :, 0, 0].double(), xv) + b.double()[None, :, None, None]
    close(y.double(), yr, 1e-4, 2e-4 * float(yr.abs().max()), 'conv fwd (DMA)')
    close(part[0].sum(-1).double(), yr.sum((0, 2, 3)), 1e-3, 1e-2, 'stats')
    a1 = rnd((N, K, T, V), 9)
    dx, _ = ops.conv(gs, K=M, w=t(w), bias=None, M=K, wmode=1, add1=t(a1))
    dxr = torch.einsum('mk,nmtv->nktv', w[:, :, 0, 0].double(), gv) + a1.double()
    close(dx.double(), dxr, 1e-4, 2e-4 * float(dxr.abs().max()), 'conv bwd-data (DMA)')


@pytest.mark.parametrize('shape', [(2, 768, 256, 16, 20, 1), (3, 384, 128, 16, 20, 0), (2, 192, 64, 24, 25, 1), (2, 400, 96, 12, 25, 0), (1, 64, 16, 16, 20, 1)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_plain_source_gemm_without_prologue_table(shape):
    """Round 4: a plain source tensor (no coefficients, second source or ReLU) takes the GEMM instantiation WITHOUT the [3][K]
    coefficient table (two workgroups per CU also at K >= 384) -- the dx <- dx3 GEMMs (reference models/ctrgcn.py:252-254 backward).
    Both weight layouts, broadcast term + two residual adds, V = 20 / 25, K up to 768 and not a multiple of 64; fp64 reference."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, K, M, T, V, wmode = shape
    d = dev()
    x = rnd((N, K + 8, T, V), 1)
    w = (rnd((K, M, 1, 1), 2) if wmode else rnd((M, K, 1, 1), 2)) * 0.1
    a1, a2, bc = rnd((N, M, T, V), 3), rnd((N, M, T, V), 4), rnd((M, N, V), 5)
    t = lambda z: z.to(d)
    y, _ = ops.conv(S(t(x), coff=8), K=K, w=t(w), bias=None, M=M, wmode=wmode, bcast=t(bc), bcast_scale=0.25, add1=t(a1), add2=t(a2))
    assert ops._lib_().tamgcn_last_kernel().decode().startswith('conv1x1_glds_kernel<1, 16, false'), ops._lib_().tamgcn_last_kernel()
    wm = w[:, :, 0, 0].double()
    ref = torch.einsum('km,nktv->nmtv' if wmode else 'mk,nktv->nmtv', wm, x[:, 8:].double())
    ref = ref + 0.25 * bc.double().permute(1, 0, 2)[:, :, None, :] + a1.double() + a2.double()
    close(y.double(), ref, 1e-4, 2e-4 * float(ref.abs().max()), 'plain-source GEMM')


def test_coef_diff_kernel():
    """tamgcn_coef_diff: the two-source prologue coefficients of unit_gcn's offset_conv input (reference models/ctrgcn.py:256-258,
    diff = down(x) - bn(y)) -- bit-identical to the torch expressions it replaced, all three residual modes."""
    from tam_gcn_amd import ops
    d = dev()
    cd, cy = rnd((3, 72), 1).to(d), rnd((3, 72), 2).to(d)
    assert torch.equal(ops.coef_diff(cd, cy, 0), torch.stack((cd[0], -cy[0], cd[2] - cy[2])))
    assert torch.equal(ops.coef_diff(None, cy, 1), torch.stack((torch.ones_like(cy[0]), -cy[0], -cy[2])))
    assert torch.equal(ops.coef_diff(None, cy, 2), torch.stack((-cy[0], torch.zeros_like(cy[0]), -cy[2])))


def test_conv_prologue_slices_mask_aux():
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, Ct, T, V = 2, 48, 13, 20
    x1, x2 = rnd((N, Ct, T, V), 1), rnd((N, Ct, T, V), 2)
    coef = rnd((3, Ct), 3)
    w = rnd((16, 16, 5, 1), 4) * 0.2
    val = torch.relu(coef[0][None, :, None, None] * x1 + coef[1][None, :, None, None] * x2 + coef[2][None, :, None, None])
    ref = F.conv2d(val[:, 16:32], w, None, padding=(2, 0))
    y = torch.full((N, 64, T, V), 7.0, device=dev())
    add1 = rnd((N, 64, T, V), 5)
    msk = rnd((N, 64, T, V), 6)
    aux = rnd((N, 64, T, V), 7)
    yg, part = ops.conv(S(x1.to(dev()), x2.to(dev()), coef.to(dev()), coff=16, act=1), K=16, w=w.to(dev()), bias=None,
                        M=16, KT=5, pad=2, y=y, ycoff=32, add1=add1.to(dev()), mask=S(msk.to(dev()), coff=32),
                        aux=aux.to(dev()), aux_center=torch.zeros(64, device=dev()), auxcoff=32, stats=True)
    exp = (ref + add1[:, 32:48]) * (msk[:, 32:48] > 0)
    close(yg[:, 32:48], exp, 1e-4, 1e-4)
    assert float(yg[:, :32].min()) == 7.0 and float(yg[:, 48:].max()) == 7.0
    close(part[0, 32:48].sum(-1), exp.sum((0, 2, 3)), 1e-3, 1e-2)
    close(part[1, 32:48].sum(-1), (exp * aux[:, 32:48]).sum((0, 2, 3)), 1e-3, 1e-2)


def test_bn_finalize_fwd_bwd():
    import ew_ref as R
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, C_, T, V = 3, 24, 7, 20
    x = (rnd((N, C_, T, V), 1) * 2 + 0.5).requires_grad_(True)
    g = (1 + 0.1 * rnd((C_,), 2)).requires_grad_(True)
    b = rnd((C_,), 3).requires_grad_(True)
    rm, rv = rnd((C_,), 4), rnd((C_,), 5, 0.5, 1.5)
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm, rv, g, b, training=True, momentum=0.1, eps=1e-5)
    cot = rnd(tuple(y.shape), 6)
    (y * cot).sum().backward()
    d = dev()
    xd = x.detach().to(d)
    part = torch.stack((xd.sum(3).sum(2).t().contiguous(), (xd * xd).sum(3).sum(2).t().contiguous()))   # [2][C][N]
    coef = torch.empty(3, C_, device=d); save = torch.empty(2, C_, device=d)
    rmd, rvd = rm0.to(d), rv0.to(d)
    nbt = torch.zeros((), dtype=torch.int64, device=d)
    ops.bn_fwd_finalize(part, 0, N * T * V, g.detach().to(d), b.detach().to(d), rmd, rvd, nbt, 0.1, 1e-5, True,
                        coef, save, 0, C_)
    yg = ops.apply(S(xd, coef=coef), C_)
    close(yg, y, 1e-4, 1e-5)
    close(rmd, rm, 1e-5, 1e-6); close(rvd, rv, 1e-5, 1e-6)
    assert int(nbt) == 1
    # the finaliser against its fp64 evaluation on the partial sums it was given, to fp32 rounding (tests/ew_ref.py)
    fd = dict(C=C_, part=part.cpu(), count=N * T * V, training=1, gamma=g.detach(), beta=b.detach(), running_mean=rm0, running_var=rv0,
              momentum=0.1, eps=1e-5)
    cf, sv = coef.cpu(), save.cpu()
    R.bn_check('bn_fwd_finalize', dict(c1=cf[0], c2=cf[1], c0=cf[2], mean=sv[0], invstd=sv[1], running_mean=rmd.cpu(), running_var=rvd.cpu()),
               R.bn_fwd(fd))
    cd = cot.to(d)
    _, bpart = ops.add_act_bwd(cd, None, 0, xd, save, None, None, want_dz=False)
    R.verify('add_act_bwd', 'add_act_bwd', dict(dout=cot, relu=0, a_pre=x.detach(), a_save=sv, want_dz=0), dict(s0=bpart[0].cpu(), s1=bpart[1].cpu()))
    coefb = torch.empty(3, C_, device=d)
    dg = torch.empty(C_, device=d); db = torch.empty(C_, device=d); dbias = torch.empty(C_, device=d)
    ops.bn_bwd_finalize(bpart, 0, N * T * V, g.detach().to(d), save, 0, True, dg, db, dbias, coefb, 0, C_)
    close(dg, g.grad, 1e-4, 1e-4); close(db, b.grad, 1e-4, 1e-4)
    cb = coefb.cpu()
    R.bn_check('bn_bwd_finalize', dict(c1=cb[0], c2=cb[1], c0=cb[2], dgamma=dg.cpu(), dbeta=db.cpu(), dbias_conv=dbias.cpu()),
               R.bn_bwd(dict(C=C_, part=bpart.cpu(), count=N * T * V, training=1, gamma=g.detach(), save=sv)))
    dx = ops.apply(S(cd, xd, coefb), C_)
    close(dx, x.grad, 1e-3, 1e-5)
    assert float(dbias.abs().max()) < 1e-3


@pytest.mark.parametrize('shape', [(2, 3, 64, 9, 20, 3), (2, 64, 64, 20, 20, 3), (1, 128, 128, 5, 25, 3),
                                   (2, 256, 256, 16, 20, 3), (2, 64, 32, 8, 20, 1), (2, 256, 64, 40, 20, 3), (3, 128, 48, 33, 20, 3)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_ctrgc_fused_fwd_bwd(shape):
    """Fused CTRGC (S subsets summed) against the einsum formulation on the CPU."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, Cin, Cout, T, V, S_ = shape
    R = 8 if Cin in (3, 9) else Cin // 8
    x = rnd((N, Cin, T, V), 1).requires_grad_(True)
    W12 = (rnd((S_ * 2 * R, Cin), 2) * (1.0 / Cin ** 0.5)).requires_grad_(True)
    B12 = (rnd((S_ * 2 * R,), 3) * 0.1).requires_grad_(True)
    W3 = (rnd((S_ * Cout, Cin), 4) * (1.0 / Cin ** 0.5)).requires_grad_(True)
    B3 = (rnd((S_ * Cout,), 5) * 0.1).requires_grad_(True)
    W4 = (rnd((S_, Cout, R), 6) * (1.0 / R ** 0.5)).requires_grad_(True)
    B4 = (rnd((S_, Cout), 7) * 0.1).requires_grad_(True)
    A = (rnd((S_, V, V), 8) * 0.3).requires_grad_(True)
    alpha = torch.tensor([0.7], requires_grad=True)
    xbar = x.mean(2)                                                      # N,Cin,V
    pqr = torch.einsum('jc,ncv->jnv', W12, xbar) + B12[:, None, None]      # (S2R, N, V)
    y = 0
    for s in range(S_):
        p = pqr[(2 * s) * R:(2 * s + 1) * R].permute(1, 0, 2)              # N,R,V
        q = pqr[(2 * s + 1) * R:(2 * s + 2) * R].permute(1, 0, 2)
        D = torch.tanh(p.unsqueeze(-1) - q.unsqueeze(-2))
        E = alpha * (torch.einsum('cr,nruv->ncuv', W4[s], D) + B4[s][None, :, None, None]) + A[s][None, None]
        x3 = torch.einsum('oc,nctv->notv', W3[s * Cout:(s + 1) * Cout], x) + B3[s * Cout:(s + 1) * Cout][None, :, None, None]
        y = y + torch.einsum('ncuv,nctv->nctu', E, x3)
    cot = rnd(tuple(y.shape), 9)
    (y * cot).sum().backward(retain_graph=True)
    d = dev()
    t = lambda z: z.detach().to(d).contiguous()
    xs = S(t(x))
    xb = ops.tmean(xs, Cin)
    close(xb, xbar.permute(1, 0, 2), 1e-5, 1e-6, 'tmean')
    pq, _ = ops.conv(S(xb.view(1, Cin, N, V)), K=Cin, w=t(W12), bias=t(B12), M=S_ * 2 * R)
    pq = pq.view(S_ * 2 * R, N, V)
    close(pq, pqr, 1e-4, 1e-5, 'pq')
    yg, part, x3k = ops.ctrgc_fwd(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R, stats=True,
                                  keep_x3=True)
    x3r = torch.einsum('oc,nctv->notv', W3, x) + B3[None, :, None, None]
    if V != 20:                                                           # the streaming route: x3 from the pointwise GEMM, its own ledgers
        close(yg, y, 2e-4, 2e-4, 'ctrgc fwd')
        close(x3k, x3r, 2e-4, 2e-4, 'x3 kept for the backward')
    yg0, _, none = ops.ctrgc_fwd(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R, stats=False)
    assert none is None and torch.equal(yg0, yg)
    # E, built once per layer in HBM and loaded by the kernels, against its definition
    Eg = ops.ctrgc_build_E(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R)
    Er = torch.stack([alpha * (torch.einsum('cr,nruv->ncuv', W4[s], torch.tanh(
        pqr[(2 * s) * R:(2 * s + 1) * R].permute(1, 0, 2).unsqueeze(-1) - pqr[(2 * s + 1) * R:(2 * s + 2) * R].permute(1, 0, 2).unsqueeze(-2)))
        + B4[s][None, :, None, None]) + A[s][None, None] for s in range(S_)], 1)
    close(Eg, Er, 2e-4, 2e-5, 'E')
    yg1, _, _ = ops.ctrgc_fwd(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R, stats=False, E=Eg)
    assert torch.equal(yg1, yg)                                           # E handed in == E built inside the call
    if V == 20:
        # the fused forward: y, x3 and every moment slot at the forward ledger's derived bars (tests/ctrgc_fwd_ref.py), against
        # the E the call built, read back above -- tanh stays out of the bound
        import ctrgc_fwd_ref as FR
        FR.verify('x'.join(map(str, shape)), dict(x=x.detach(), w3=W3.detach(), b3=B3.detach(), E=Eg.cpu().view(N, S_, Cout, V, V),
                                                  coff=0, Cin=Cin, Cout=Cout, S=S_), dict(y=yg, x3=x3k, part=part))
    else:
        close(part[0].sum(-1), y.sum((0, 2, 3)), 1e-3, 1e-2, 'stats')
        close(part[1].sum(-1), (y * y).sum((0, 2, 3)), 1e-3, 1e-2, 'stats2')
    dx3, db3, dA, dW4, db4, dal, dpq = ops.ctrgc_bwd(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha),
                                                     Cin, Cout, S_, R, S(t(cot)), x3=x3k, E=Eg)
    dx3e, db3e = ops.ctrgc_bwd_dx3(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R, S(t(cot)))
    assert torch.equal(dx3e, dx3)                                         # E rebuilt inside the call
    gpq, = torch.autograd.grad((y * cot).sum(), pqr, retain_graph=True)
    sc = lambda g: 2e-4 * (float(g.abs().max()) + 1e-3)
    # the dE chain without the kept x3 (one more pointwise GEMM) against the one that reads it
    for got, ref, nm in zip(ops.ctrgc_bwd_de(xs, pq, t(W3), t(B3), t(W4), t(B4), t(A), t(alpha), Cin, Cout, S_, R,
                                             S(t(cot))), (dA, dW4, db4, dal, dpq), ('dA', 'dW4', 'db4', 'dalpha', 'dpq')):
        close(got, ref.cpu(), 1e-4, 0.25 * sc(ref.cpu()), nm + ' (x3 recomputed)')
    close(dA, A.grad, 1e-3, sc(A.grad), 'dA')
    close(dW4, W4.grad, 1e-3, sc(W4.grad), 'dW4')
    close(db4, B4.grad, 1e-3, sc(B4.grad), 'db4')
    close(dal, alpha.grad, 1e-3, sc(alpha.grad), 'dalpha')
    close(db3, B3.grad, 1e-3, sc(B3.grad), 'db3')
    close(dpq, gpq, 1e-3, sc(gpq), 'dpq')
    dW3 = ops.wgrad(S(dx3), xs, M=S_ * Cout, K=Cin)
    close(dW3.view(S_ * Cout, Cin), W3.grad, 1e-3, sc(W3.grad), 'dW3')
    dpq4 = S(dpq.view(1, S_ * 2 * R, N, V))
    dxbar, _ = ops.conv(dpq4, K=S_ * 2 * R, w=t(W12), bias=None, M=Cin, wmode=1)
    dx, _ = ops.conv(S(dx3), K=S_ * Cout, w=t(W3), bias=None, M=Cin, wmode=1, bcast=dxbar.view(Cin, N, V),
                     bcast_scale=1.0 / T)
    close(dx, x.grad, 1e-3, sc(x.grad), 'dx')
    dW12 = ops.wgrad(dpq4, S(xb.view(1, Cin, N, V)), M=S_ * 2 * R, K=Cin)
    close(dW12.view(S_ * 2 * R, Cin), W12.grad, 1e-3, sc(W12.grad), 'dW12')


def test_elementwise_kernels():
    import ew_ref as R
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, C_, T, V = 2, 20, 13, 20
    d = dev()
    y, o, r = rnd((N, C_, T, V), 1), rnd((N, C_, T, V), 2), rnd((N, C_, T, V), 3)
    cy, co = rnd((3, C_), 4), rnd((3, C_), 5)
    ap = lambda c, z: c[0][None, :, None, None] * z + c[2][None, :, None, None]
    g = torch.relu(ap(cy, y) + torch.tanh(ap(co, o)) + r)
    gg = ops.gcn_tail_fwd(S(y.to(d), coef=cy.to(d)), S(o.to(d), coef=co.to(d)), S(r.to(d)))
    close(gg, g, 1e-5, 1e-5)
    dg = rnd((N, C_, T, V), 6)
    osave = rnd((2, C_), 11).to(d)
    dsum, doz, part = ops.gcn_tail_bwd(dg.to(d), gg, S(o.to(d), coef=co.to(d)), osave)
    e_dsum = dg * (g > 0)
    e_doz = e_dsum * (1 - torch.tanh(ap(co, o)) ** 2)
    close(dsum, e_dsum, 1e-5, 1e-5); close(doz, e_doz, 1e-4, 1e-5)
    # every output against fp64, the moments slot by slot (tests/ew_ref.py; tests/test_gpu_ew_forms.py walks the kernel forms)
    R.verify('gcn_tail_bwd', 'gcn_tail_bwd', dict(C=C_, dg=dg, g=gg.cpu(), o=dict(x1=o, coef=co), o_save=osave.cpu()),
             dict(dsum=dsum.cpu(), doz=doz.cpu(), s0=part[0].cpu(), s1=part[1].cpu()))
    # max-pool fwd/bwd, stride 1 and 2, vs autograd
    for s in (1, 2):
        h = rnd((N, C_, T, V), 7).requires_grad_(True)
        ch = rnd((3, C_), 8)
        a = torch.relu(ap(ch, h))
        mp = F.max_pool2d(a, (3, 1), (s, 1), (1, 0))
        cot = rnd(tuple(mp.shape), 9)
        (mp * cot).sum().backward()
        # reference gradient wrt the BN output (before ReLU): autograd through relu
        hb = ap(ch, h.detach()).requires_grad_(True)
        (F.max_pool2d(torch.relu(hb), (3, 1), (s, 1), (1, 0)) * cot).sum().backward()
        T2 = mp.shape[2]
        yb = torch.zeros(N, C_ + 4, T2, V, device=d)
        src = S(h.detach().to(d), coef=ch.to(d), act=1)
        part = ops.maxpool_fwd(src, C_, s, yb, 4, stats=True)
        close(yb[:, 4:], mp, 1e-5, 1e-6)
        hs = dict(x1=h.detach(), coef=ch, act=1)
        R.verify(f'maxpool_fwd s={s}', 'maxpool_fwd', dict(C=C_, src=hs, stride=s, stats=1),
                 dict(y=yb[:, 4:].cpu(), s0=part[0, 4:].cpu(), s1=part[1, 4:].cpu()))
        dd = torch.zeros(N, C_ + 2, T, V, device=d)
        hsave = rnd((2, C_), 12).to(d)
        bp = ops.maxpool_bwd(S(cot.to(d)), src, hsave, C_, s, dd, 2)
        close(dd[:, 2:], hb.grad, 1e-5, 1e-6, f'maxpool bwd s={s}')
        R.verify(f'maxpool_bwd s={s}', 'maxpool_bwd', dict(C=C_, src=hs, gy=dict(x1=cot), stride=s, src_save=hsave.cpu()),
                 dict(d=dd[:, 2:].cpu(), s0=bp[0, 2:].cpu(), s1=bp[1, 2:].cpu()))


@pytest.mark.parametrize('mode,bar', [('0', 2e-6), ('1', 3e-5)])
def test_split_fp32_modes_against_fp64(mode, bar):
    """TAMGCN_SPLIT_BF16 is read once per process: run the GEMM kernels in a child process per mode and bound their
    error against an fp64 reference.  0 = exact fp32-input MFMA (rounding noise only); 1 = split-fp32 on the bf16 matrix
    cores in the weight-gradient and wide data-gradient GEMMs (~4.5e-6), forward GEMMs exact in both."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TAMGCN_SPLIT_BF16=mode)
    out = subprocess.run([sys.executable, os.path.join(root, 'tools', 'split_accuracy.py')], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    errs = {}
    for line in out.stdout.splitlines():
        m = re.match(r'\s+(wgrad|conv fwd|conv bwd-data|x3 \(kept\)|y)\s+max\|err\|/max\|ref\| ([0-9.e+-]+)', line)
        if m:
            errs.setdefault(m.group(1), []).append(float(m.group(2)))
    assert set(errs) == {'wgrad', 'conv fwd', 'conv bwd-data', 'x3 (kept)', 'y'}, out.stdout[-2000:]
    for k in ('conv fwd', 'x3 (kept)', 'y'):                     # activations: exact fp32 in every default mode
        assert max(errs[k]) <= 2e-6, (k, errs[k])
    for k in ('wgrad', 'conv bwd-data'):
        assert max(errs[k]) <= bar, (k, errs[k])
    if mode == '1':                                              # and the split really is in use where it should be
        assert max(errs['wgrad']) > 1e-6


def test_pointwise_gemm_four_wave_layout():
    """TAMGCN_CONV_WAVES=4 (read once per process): the 1x1 LDS-DMA GEMM with 1 x 4 waves of four row tiles instead of the default
    2 x 4 waves of two -- the A/B arm of tools/conv_knockout.py (half the prologue / address VALU per MFMA, but its epilogue is
    slower: measured behind the default at every signature of the step).  The conv / pointwise primitive tests of this file, in a child
    process with the switch on."""
    import os
    import subprocess
    import sys
    if os.environ.get('TAMGCN_CONV_WAVES') == '4':
        pytest.skip('already inside the child run')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-x', '-q', '-k',
                          'conv_fwd_bwd_wgrad or pointwise_dma or prologue_slices'], cwd=root,
                         env=dict(os.environ, TAMGCN_CONV_WAVES='4'), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]


@pytest.mark.parametrize('mode', ['0', '2', '3'])
def test_ctrgc_forward_forms(mode):
    """TAMGCN_CTRGC_FWD2 (read once per process) selects the form of the fused forward at 16-channel tiles: 0 = the E tile resident in
    LDS (one workgroup per CU), 2 = ctrgc_fwd2_kernel wherever it applies (E fragments from L2, operands by LDS-DMA: frame chunks
    16 + 16 + 8 at Cin = 256 and 16 + 4 at Cin = 64), 3 = E from L2 with register-staged operands everywhere; the default (1) picks
    by Cin.  The fused-CTRGC test of this file in a child process per form."""
    import os
    import subprocess
    import sys
    if os.environ.get('TAMGCN_CTRGC_FWD2') is not None:
        pytest.skip('already inside a child run')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-m', 'gpu', '-x', '-q', '-k', 'ctrgc_fused_fwd_bwd'],
                         cwd=root, env=dict(os.environ, TAMGCN_CTRGC_FWD2=mode), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]


@pytest.mark.parametrize('shape,training', [((3, 3, 7, 25, 2), True), ((4, 3, 13, 20, 1), True), ((3, 3, 7, 25, 2), False)])
def test_stem_and_head_against_torch(shape, training):
    """data_bn + permutes (reference models/ctrgcn.py:328-332) and mean-pool + fc (:343-348) against the
    stock ops they replace, forward, backward, running statistics."""
    import copy
    from tam_gcn_amd import functional as Fn
    N, C_, T, V, M = shape
    d = dev()
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm1d(M * V * C_)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(M * V * C_)); bn.bias.copy_(0.1 * torch.randn(M * V * C_))
        bn.running_mean.copy_(0.1 * torch.randn(M * V * C_)); bn.running_var.copy_(0.5 + torch.rand(M * V * C_))
    bn.train(training)
    bng = copy.deepcopy(bn).to(d)
    x = rnd(shape, 1).requires_grad_(True)
    y = bn(x.permute(0, 4, 3, 1, 2).contiguous().view(N, M * V * C_, T))
    y = y.view(N, M, V, C_, T).permute(0, 1, 3, 4, 2).contiguous().view(N * M, C_, T, V)
    cot = rnd(tuple(y.shape), 2)
    (y * cot).sum().backward()
    xg = x.detach().to(d).requires_grad_(True)
    yg = Fn.StemFn.apply(bng, xg, bng.weight, bng.bias)
    (yg * cot.to(d)).sum().backward()
    close(yg, y, 1e-4, 1e-5, 'stem forward')
    close(xg.grad, x.grad, 1e-3, 2e-5, 'stem dx')
    close(bng.weight.grad, bn.weight.grad, 1e-3, 1e-4, 'data_bn dgamma'); close(bng.bias.grad, bn.bias.grad, 1e-3, 1e-4, 'data_bn dbeta')
    close(bng.running_mean, bn.running_mean, 1e-5, 1e-6); close(bng.running_var, bn.running_var, 1e-5, 1e-6)
    assert int(bng.num_batches_tracked) == int(bn.num_batches_tracked)
    # head
    Cf, K = 32, 10
    h = rnd((N * M, Cf, T, V), 3).requires_grad_(True)
    W, b = (rnd((K, Cf), 4) * 0.2).requires_grad_(True), rnd((K,), 5).requires_grad_(True)
    lo = F.linear(h.view(N, M, Cf, -1).mean(3).mean(1), W, b)
    cl = rnd((N, K), 6)
    (lo * cl).sum().backward()
    hg, Wg, bg = (t.detach().to(d).requires_grad_(True) for t in (h, W, b))
    lg = Fn.HeadFn.apply(hg, Wg, bg, M)
    (lg * cl.to(d)).sum().backward()
    close(lg, lo, 1e-4, 1e-5, 'logits')
    close(hg.grad, h.grad, 1e-4, 1e-7, 'head dx'); close(Wg.grad, W.grad, 1e-4, 1e-6, 'dW'); close(bg.grad, b.grad, 1e-4, 1e-6, 'db')


def test_cross_entropy_against_torch():
    """tamgcn_ce_fwd / _bwd against torch's CrossEntropyLoss on the same logits: loss and gradient."""
    from tam_gcn_amd.functional import CrossEntropyLoss
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(5)
    for N, K in [(256, 10), (7, 60), (1, 3), (1000, 10)]:
        logits = (torch.randn(N, K, generator=g) * 3).to(dev).requires_grad_(True)
        lab = torch.randint(0, K, (N,), generator=g).to(dev)
        loss = CrossEntropyLoss()(logits, lab)
        (loss * 1.7).backward()
        ref_l = logits.detach().double().clone().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(ref_l, lab)
        (ref * 1.7).backward()
        assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
        assert (logits.grad.double() - ref_l.grad).abs().max() <= 2e-7
    # nn.CrossEntropyLoss's default ignore_index = -100: skipped rows, mean over the kept ones
    N, K = 37, 10
    logits = (torch.randn(N, K, generator=g) * 3).to(dev).requires_grad_(True)
    lab = torch.randint(0, K, (N,), generator=g)
    lab[::5] = -100
    lab = lab.to(dev)
    loss = CrossEntropyLoss()(logits, lab)
    loss.backward()
    ref_l = logits.detach().double().clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(ref_l, lab)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    assert (logits.grad.double() - ref_l.grad).abs().max() <= 2e-7 and float(logits.grad[::5].abs().max()) == 0.0
    assert torch.isnan(CrossEntropyLoss()(logits.detach(), torch.full((N,), -100, device=dev)))       # nothing kept: NaN, as torch
    # a label outside [0, K) (torch: device assert): NaN loss, that row's gradient zero, no out-of-bounds read
    for badv in (K, -1, 10 ** 12):
        lab2 = lab.clone()
        lab2[3] = badv
        lg = logits.detach().clone().requires_grad_(True)
        loss = CrossEntropyLoss()(lg, lab2)
        loss.backward()
        assert torch.isnan(loss) and float(lg.grad[3].abs().max()) == 0.0


@pytest.mark.parametrize('shape', [(3, 64, 64, 16, 20, 5, 1), (2, 32, 64, 13, 25, 5, 2), (2, 64, 48, 10, 64, 5, 2)])
def test_kx1_weight_gradient_taps_with_prologue(shape, monkeypatch):
    """k x 1 weight gradient on the LDS-DMA kernel with the operands the temporal branches hand it: gy a two-source
    BatchNorm-backward apply, x a BatchNorm apply + ReLU, both channel slices of wider tensors; fp64 torch reference.
    Both arithmetic modes (split-bf16 default, exact fp32)."""
    from tam_gcn_amd import ops, _lib
    from tam_gcn_amd.ops import S
    N, M, K, T, V, KT, dil = shape
    pad = dil * (KT - 1) // 2
    d = dev()
    ap = lambda c, a, b: c[0][None, :, None, None] * a + (c[1][None, :, None, None] * b if b is not None else 0) + c[2][None, :, None, None]
    Kt, Mt = K + 16, M + 32
    x1, cx = rnd((N, Kt, T, V), 1), rnd((3, Kt), 3)
    g1, g2, cg = rnd((N, Mt, T, V), 4), rnd((N, Mt, T, V), 5), rnd((3, Mt), 6)
    xv = torch.relu(ap(cx.double(), x1.double(), None))[:, 16:16 + K]
    gv = ap(cg.double(), g1.double(), g2.double())[:, 32:32 + M]
    w = torch.zeros(M, K, KT, 1, dtype=torch.float64, requires_grad=True)
    xv = xv.clone().requires_grad_(False)
    y = F.conv2d(xv, w, None, padding=(pad, 0), dilation=(dil, 1))
    (y * gv).sum().backward()
    ref = w.grad
    t = lambda z: z.to(d)
    xs = S(t(x1), None, t(cx), coff=16, act=1)
    gs = S(t(g1), t(g2), t(cg), coff=32)
    lib = _lib.load()
    prev = lib.tamgcn_get_split_mode()
    seen, orig = [], ops.reduce_sum

    def spy(*a, **k):                                  # the kernel that filled the partial slabs
        seen.append(lib.tamgcn_last_kernel().decode())
        return orig(*a, **k)
    monkeypatch.setattr(ops, 'reduce_sum', spy)
    try:
        for mode, bar in ((1, 2e-5), (0, 2e-6)):
            lib.tamgcn_set_split_mode(mode)
            del seen[:]
            dw = ops.wgrad(gs, xs, M=M, K=K, KT=KT, dil=dil, stride=1, pad=pad)
            torch.cuda.synchronize()
            name = seen[0] if seen else lib.tamgcn_last_kernel().decode()
            assert name.startswith('wgrad_glds_kernel') and name.endswith('taps'), name
            err = float((dw.double().cpu() - ref).abs().max() / ref.abs().max())
            assert err <= bar, (mode, err)
    finally:
        lib.tamgcn_set_split_mode(prev)


# N, Cb, T, V, KT, dilations, stride  (the MS-TCN second stage: temporal branches + pooled branch in one launch)
TCONV_CASES = [
    (2, 16, 64, 20, 5, (1, 2), 1),        # l1-l4
    (3, 16, 13, 20, 5, (1, 2), 1),        # ragged T: one partial frame tile
    (2, 32, 33, 20, 5, (1, 2), 2),        # l5: strided, odd T
    (2, 32, 32, 20, 5, (1, 2), 1),
    (2, 64, 32, 20, 5, (1, 2), 2),        # l8: two 32-row output halves, strided
    (2, 64, 16, 20, 5, (1, 2), 1),
    (2, 16, 20, 20, 3, (1, 2, 3, 4), 1),  # MultiScale_TemporalConv's constructor defaults
    (2, 32, 14, 25, 5, (1, 2), 1),        # NTU: rows of 25 joints (Vp = 28, dword-aligned 16-byte accesses)
    (2, 32, 15, 25, 5, (1, 2), 2),
    (1, 64, 40, 64, 5, (1, 2), 1),        # V = 64: four joint slices
    (1, 16, 9, 64, 3, (2,), 2),
    (2, 64, 4, 20, 5, (1, 2), 1),         # the model cases' last layers at T = 13: 4 frames, fewer column tiles than waves
    (2, 64, 7, 20, 5, (1, 2), 2),
    (2, 32, 13, 20, 5, (1, 2), 2),
    (2, 32, 7, 20, 5, (1, 2), 1),
]


@pytest.mark.parametrize('case', TCONV_CASES, ids=lambda c: 'x'.join(str(x).replace(' ', '') for x in c))
def test_tconv_fused_branches_fwd_bwd(case):
    """tamgcn_tconv_fwd / _bwd (csrc/tconv.hip) against fp64 torch: conv2d per branch + max_pool2d on relu(bn(h)) slices
    of a wider tensor, written into slices of a wider output; the BatchNorm moment partials; the data gradient with the
    ReLU mask and the entry BatchNorm's backward moments."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, Cb, T, V, KT, dils, s = case
    nb = len(dils)
    d = dev()
    assert ops.tconv_supported(V, Cb, [KT] * nb, list(dils), s, T)
    T2 = (T - 1) // s + 1
    lead, tail = 16, 8                                  # channels in front of / behind the branch slices
    Ch = lead + (nb + 1) * Cb + tail
    Co = 8 + (nb + 1) * Cb + 8
    h1 = rnd((N, Ch, T, V), 1)
    ch = torch.stack((1 + 0.3 * rnd((Ch,), 2), torch.zeros(Ch), 0.2 * rnd((Ch,), 3)))
    ws = [rnd((Cb, Cb, KT, 1), 10 + b) * (1.0 / (Cb * KT)) ** 0.5 for b in range(nb)]
    bs = [0.1 * rnd((Cb,), 20 + b) for b in range(nb)]
    hv = torch.relu(ch[0].double()[None, :, None, None] * h1.double() + ch[2].double()[None, :, None, None])
    hv.requires_grad_(True)
    outs = []
    for b in range(nb):
        pad = (KT - 1) * dils[b] // 2
        outs.append(F.conv2d(hv[:, lead + b * Cb: lead + (b + 1) * Cb], ws[b].double(), bs[b].double(), stride=(s, 1),
                             padding=(pad, 0), dilation=(dils[b], 1)))
    outs.append(F.max_pool2d(hv[:, lead + nb * Cb: lead + (nb + 1) * Cb], kernel_size=(3, 1), stride=(s, 1), padding=(1, 0)))
    ref = torch.cat(outs, 1)
    assert ref.shape[2] == T2
    t = lambda z: z.to(d)
    y = torch.full((N, Co, T2, V), 7.0, device=d)
    part = ops.tconv_fwd(S(t(h1), None, t(ch), coff=lead, act=1), Cb, KT, list(dils), s, [t(w) for w in ws], [t(b_) for b_ in bs],
                         True, y, 8, stats=True)
    torch.cuda.synchronize()
    got = y[:, 8:8 + (nb + 1) * Cb].double().cpu()
    scale = float(ref.abs().max())
    assert float((got - ref.detach()).abs().max()) <= 2e-6 * scale
    assert float((y[:, :8] - 7).abs().max()) == 0 and float((y[:, 8 + (nb + 1) * Cb:] - 7).abs().max()) == 0    # neighbours untouched
    sums = part.double().sum(2).cpu()[:, 8:8 + (nb + 1) * Cb]
    cnt = N * T2 * V
    assert float((sums[0] - ref.detach().sum((0, 2, 3))).abs().max()) <= 2e-6 * scale * cnt
    assert float((sums[1] - (ref.detach() ** 2).sum((0, 2, 3))).abs().max()) <= 4e-6 * scale * scale * cnt
    # ---- data gradient of the temporal branches: gy = c1*g1 + c2*g2 + c0 on slices of wider tensors
    Cg = 4 + nb * Cb + 4
    g1, g2 = rnd((N, Cg, T2, V), 30), rnd((N, Cg, T2, V), 31)
    cg = torch.stack((1 + 0.2 * rnd((Cg,), 32), 0.3 * rnd((Cg,), 33), 0.1 * rnd((Cg,), 34)))
    gv = (cg[0].double()[None, :, None, None] * g1.double() + cg[1].double()[None, :, None, None] * g2.double() +
          cg[2].double()[None, :, None, None])[:, 4:4 + nb * Cb]
    (ref[:, :nb * Cb] * gv).sum().backward()
    # d relu(bn(h)) -> d (bn(h)) by the mask; the product's contract stops there (the BatchNorm backward is the consumer's prologue)
    dref = (hv.grad * (hv.detach() > 0))[:, lead: lead + nb * Cb]
    mu = 0.1 * rnd((Ch,), 40)
    dh = torch.full((N, Ch, T, V), 3.0, device=d)
    bpart = ops.tconv_bwd(S(t(g1), t(g2), t(cg), coff=4), Cb, KT, list(dils), s, [t(w) for w in ws],
                          S(t(h1), None, t(ch), coff=lead), t(mu), dh, lead)
    torch.cuda.synchronize()
    gotd = dh[:, lead: lead + nb * Cb].double().cpu()
    dscale = float(dref.abs().max())
    assert float((gotd - dref).abs().max()) <= 2e-6 * dscale
    assert float((dh[:, :lead] - 3).abs().max()) == 0 and float((dh[:, lead + nb * Cb:] - 3).abs().max()) == 0
    bs_ = bpart.double().sum(2).cpu()[:, lead: lead + nb * Cb]
    cnt1 = N * T * V
    hc = (h1.double() - mu.double()[None, :, None, None])[:, lead: lead + nb * Cb]
    assert float((bs_[0] - dref.sum((0, 2, 3))).abs().max()) <= 2e-6 * dscale * cnt1
    assert float((bs_[1] - (dref * hc).sum((0, 2, 3))).abs().max()) <= 4e-6 * dscale * float(hc.abs().max()) * cnt1
    # ---- weight gradients of every branch in one launch (tamgcn_tconv_wgrad)
    wd = [w.double().clone().requires_grad_(True) for w in ws]
    hv2 = hv.detach()
    outs2 = []
    for b in range(nb):
        pad = (KT - 1) * dils[b] // 2
        outs2.append(F.conv2d(hv2[:, lead + b * Cb: lead + (b + 1) * Cb], wd[b], None, stride=(s, 1), padding=(pad, 0), dilation=(dils[b], 1)))
    (torch.cat(outs2, 1) * gv).sum().backward()
    dws = ops.tconv_wgrad(S(t(g1), t(g2), t(cg), coff=4), S(t(h1), None, t(ch), coff=lead, act=1), Cb, KT, list(dils), s)
    torch.cuda.synchronize()
    for b in range(nb):
        wr = wd[b].grad
        assert tuple(dws[b].shape) == (Cb, Cb, KT, 1)
        assert float((dws[b].double().cpu() - wr).abs().max()) <= 3e-6 * float(wr.abs().max()), b


def test_tconv_wgrad_without_forward_source_is_an_error():
    """tamgcn_tconv_wgrad with mask = NULL (the forward's source is missing) returns an error that says so -- a host-side
    check in front of any device work -- instead of reading through the null pointer."""
    import ctypes as C
    from tam_gcn_amd import _lib
    from tam_gcn_amd.ops import S
    N, Cb, T, V, KT, dils = 2, 16, 13, 20, 5, (1, 2)
    gy = torch.zeros(N, len(dils) * Cb, T, V, device=dev())
    part = torch.zeros(1, len(dils), Cb, Cb, KT, device=dev())
    d = _lib.TconvDesc()
    d.src = S(gy).c()
    d.N, d.T_in, d.T_out, d.V, d.Cb, d.nb, d.KT, d.stride = N, T, T, V, Cb, len(dils), KT, 1
    for b, dl in enumerate(dils):
        d.dil[b] = dl
    d.y, d.yctot, d.ycoff = part.data_ptr(), 1, 0
    assert not d.mask                                              # a null pointer
    rc = _lib.load().tamgcn_tconv_wgrad(C.byref(d), None)
    assert rc != 0
    assert 'forward source' in _lib.load().tamgcn_last_error().decode()
    assert float(part.abs().max()) == 0


def test_de_tail_r16_bit_identical_beside_other_streams_in_a_graph():
    """VERDICT r03 item 6 / ADVICE r03: the captured multi-stream step of round 3 was once ~1e-4 off in ONE model's
    gradients.  The records (gpurun_out r03c/r03d/r03e logs, quoted in DESIGN.md section 3) localise every occurrence to a
    128-input-channel block (l7 or l8: R = 16 rel-channels) with exactly two of that block's own tensors affected -- one
    subset's dp or dq -- i.e. to the dE chain of the R = 16 shape, whose tail is still ctrgc_de_tail_reg_kernel.  This test
    puts that chain (dE accumulation + tail + slab reductions) for FOUR independent problems on four streams inside ONE HIP
    graph, beside each other and beside a bandwidth-heavy neighbour, and requires every replay to be bit-identical to the
    same four problems run one after the other eagerly."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    d = dev()
    N, Cin, Cout, T, V, S_, R = 16, 128, 128, 32, 20, 3, 16
    probs = []
    for i in range(4):
        t = lambda z: z.to(d).contiguous()
        x = t(rnd((N, Cin, T, V), 100 + i))
        pq = t(rnd((S_ * 2 * R, N, V), 110 + i))
        W3, B3 = t(rnd((S_ * Cout, Cin), 120 + i) * (1.0 / Cin ** 0.5)), t(rnd((S_ * Cout,), 130 + i) * 0.1)
        W4, B4 = t(rnd((S_, Cout, R), 140 + i) * (1.0 / R ** 0.5)), t(rnd((S_, Cout), 150 + i) * 0.1)
        A, alpha = t(rnd((S_, V, V), 160 + i) * 0.3), torch.tensor([0.7], device=d)
        dy = t(rnd((N, Cout, T, V), 170 + i))
        x3 = t(rnd((N, S_ * Cout, T, V), 180 + i))
        probs.append((x, pq, W3, B3, W4, B4, A, alpha, dy, x3))

    def chain(p):
        x, pq, W3, B3, W4, B4, A, alpha, dy, x3 = p
        return ops.ctrgc_bwd_de(S(x), pq, W3, B3, W4, B4, A, alpha, Cin, Cout, S_, R, S(dy), x3)

    ref = [[o.clone() for o in chain(p)] for p in probs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(d) for _ in range(4)]
    big = torch.randn(64 * 1024 * 1024 // 4, device=d)

    def step():
        cur = torch.cuda.current_stream()
        outs = []
        for st, p in zip(streams, probs):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                outs.append(chain(p))
        junk = big * 1.0001 + 1.0                                               # a streaming neighbour on the origin stream
        for st in streams:
            cur.wait_stream(st)
        return outs, junk

    s0 = torch.cuda.Stream(d)
    s0.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s0):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs, _ = step()
    for rep in range(3):
        g.replay()
        torch.cuda.synchronize()
        for i, (got, want) in enumerate(zip(outs, ref)):
            for nm, a_, b_ in zip(('dA', 'dW4', 'db4', 'dalpha', 'dpq'), got, want):
                assert torch.equal(a_, b_), f'replay {rep}, problem {i}: {nm} differs by {float((a_ - b_).abs().max()):.3e}'


@pytest.mark.parametrize('shape', [(2, 16, 13, 20, 1), (3, 32, 12, 20, 2), (2, 16, 7, 20, 2), (2, 64, 5, 64, 1), (1, 16, 1, 20, 1), (2, 16, 2, 20, 2),
                                   (2, 16, 13, 25, 1), (3, 8, 6, 25, 1), (2, 8, 3, 25, 1), (1, 8, 1, 25, 1), (2, 8, 2, 25, 1), (2, 8, 5, 7, 1), (2, 8, 9, 3, 1)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_maxpool_bwd_vector_kernel(shape):
    """The LDS-free max-pool gradients (V % 4 == 0: groups of four joints of a frame, both strides; any V at stride 1: groups of
    four flat positions of a row -- NTU's 25 joints, rows whose length is not a multiple of four): two-source gradient prologue, channel slices of wider tensors, ragged and
    tiny T, both strides, exact ties between window candidates (zeros behind the ReLU and planted equal positives: aten routes
    the gradient to the FIRST maximum) -- against autograd in fp64."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, C_, T, V, s = shape
    d = dev()
    T2 = (T - 1) // s + 1
    Ch, Cg = C_ + 8, C_ + 4
    h = rnd((N, Ch, T, V), 1)
    h[:, :, ::3] = h[:, :, :1].clone()                   # exact ties between frames 0, 3, 6, ... (and their neighbours' windows)
    ch = torch.stack((1 + 0.3 * rnd((Ch,), 2), torch.zeros(Ch), 0.2 * rnd((Ch,), 3)))
    g1, g2 = rnd((N, Cg, T2, V), 4), rnd((N, Cg, T2, V), 5)
    cg = torch.stack((1 + 0.2 * rnd((Cg,), 6), 0.3 * rnd((Cg,), 7), 0.1 * rnd((Cg,), 8)))
    ap = lambda c, a, b=None: c[0][None, :, None, None] * a + (c[1][None, :, None, None] * b if b is not None else 0) + c[2][None, :, None, None]
    hb = ap(ch.double(), h.double())[:, 8:].clone().requires_grad_(True)
    gv = ap(cg.double(), g1.double(), g2.double())[:, 4:]
    (F.max_pool2d(torch.relu(hb), (3, 1), (s, 1), (1, 0)) * gv).sum().backward()
    mu = 0.1 * rnd((2, Ch), 9)
    dd = torch.full((N, Ch, T, V), 5.0, device=d)
    t = lambda z: z.to(d)
    bp = ops.maxpool_bwd(S(t(g1), t(g2), t(cg), coff=4), S(t(h), None, t(ch), coff=8, act=1), t(mu), C_, s, dd, 8)
    torch.cuda.synchronize()
    assert ('vec' if V % 4 == 0 else 'flat') in ops._lib_().tamgcn_last_kernel().decode()
    got = dd[:, 8:].double().cpu()
    assert float((got - hb.grad).abs().max()) <= 2e-6 * (float(hb.grad.abs().max()) + 1e-6)
    assert float((dd[:, :8] - 5).abs().max()) == 0
    hc = (h.double() - mu[0].double()[None, :, None, None])[:, 8:]
    sums = bp.double().sum(2).cpu()[:, 8:]
    cnt = N * T * V
    assert float((sums[0] - hb.grad.sum((0, 2, 3))).abs().max()) <= 2e-6 * cnt
    assert float((sums[1] - (hb.grad * hc).sum((0, 2, 3))).abs().max()) <= 4e-6 * cnt


@pytest.mark.parametrize('shape', [(3, 24, 13, 20), (2, 16, 64, 20), (2, 8, 9, 64), (1, 5, 1, 20), (2, 6, 7, 12)], ids=lambda s: 'x'.join(map(str, s)))
def test_add_act_fwd_emits_the_next_blocks_frame_means(shape):
    """tamgcn_add_act_fwd with the xbar output: out = relu(bn(a) + bn(res)) and the (C, N, V) means over t of out in one pass,
    against torch; the means must equal tamgcn_tmean of the written tensor to fp32 rounding (they replace it)."""
    from tam_gcn_amd import ops
    from tam_gcn_amd.ops import S
    N, C_, T, V = shape
    d = dev()
    a, r = rnd((N, C_ + 3, T, V), 1), rnd((N, C_, T, V), 2)
    ca, cr = rnd((3, C_ + 3), 3), rnd((3, C_), 4)
    ap = lambda c, x: c[0][None, :, None, None] * x + c[2][None, :, None, None]
    ref = torch.relu(ap(ca.double(), a.double())[:, 3:] + ap(cr.double(), r.double()))
    t = lambda z: z.to(d)
    out, xb = ops.add_act_fwd(S(t(a), None, t(ca), coff=3), S(t(r), None, t(cr)), True, C_, xbar=True)
    assert xb is not None and tuple(xb.shape) == (C_, N, V)
    assert float((out.double().cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    want = ref.mean(2).permute(1, 0, 2)
    assert float((xb.double().cpu() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    close(xb, ops.tmean(S(out), C_), 1e-5, 1e-6, 'against tamgcn_tmean')
    out2 = ops.add_act_fwd(S(t(a), None, t(ca), coff=3), S(t(r), None, t(cr)), True, C_)
    assert torch.equal(out2, out)                                      # the same values as the plain pass
