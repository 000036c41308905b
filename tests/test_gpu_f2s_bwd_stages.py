"""-m gpu: every case of tests/f2s_bwd_ref.py's tables as ONE launch of tamgcn_f2s_tcn_bwd / tamgcn_f2s_gcn_bwd /
tamgcn_saliency_joints through the raw ABI against the fp64 restatement of the header's formulas, held to the derived rounding
bars (fp64_bars.check; tcn_bwd L = KT Cout, gcn_bwd L = 3 (Cout + V) + Cres, saliency_joints L = C T M -- tests/f2s_bwd_ref.py says
why).  Around every launch: the output is NaN-filled beforehand, a NaN canary sits in the slack behind every operand the kernel
streams (a read past an operand poisons the result), a guard region behind the output must stay untouched, and a second launch
must give the same bits.  Cases flagged `off` place every operand one float past a 16-byte boundary: the dword-aligned path of
the weight loads.  h and out are relu of seeded normals: about half of each mask is zero.  tamgcn_saliency_accumulate must equal
its restatement exactly in the counts and to fp64 rounding in the sums."""
import ctypes as C

import pytest
import torch

import f2s_bwd_ref as RB
import fp64_bars as B

pytestmark = pytest.mark.gpu

from tam_gcn_amd import _lib, f2s                                                  # noqa: E402,F401  (the family under test)

DEV = 'cuda:0'
SLACK, GUARD = 8, 64


def _place(t, off):
    """t on the device at `off` floats into a buffer of its own, NaN everywhere else (front and SLACK floats behind)."""
    buf = torch.full((off + t.numel() + SLACK,), float('nan'), device=DEV)
    buf[off:off + t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf[off:off + t.numel()]


def _operands(stage, c, p):
    """the kernel's own operands: the weights transposed as the host folds them"""
    if stage == 'tcn_bwd':
        return dict(gout=p['gout'], out=p['out'], h=p['h'], wtb=p['Wt'].permute(1, 0, 2).contiguous())
    if stage == 'gcn_bwd':
        return dict(dh=p['dh'], Ae=p['Ae'], wgb=p['Wg'].permute(0, 2, 1).contiguous(), gout=p['gout'], out=p['out'],
                    wrb=None if p['Wr'] is None else p['Wr'].t().contiguous())
    return dict(dx0=p['dx0'], c1=p['c1'])


def _run(stage, c, p, outputs):
    """outputs: [(name, shape)]; returns the list of result tensors"""
    lib = _lib.load()
    off = 1 if c.get('off') else 0
    keep, ptr = [], {}
    for k, t in _operands(stage, c, p).items():
        if t is None:
            ptr[k] = None
            continue
        buf, view = _place(t.float().contiguous(), off)
        keep.append((k, buf, view, t))
        ptr[k] = view.data_ptr()
    outs = []
    for name, shape in outputs:
        n = 1
        for d in shape:
            n *= d
        o = torch.full((off + n + GUARD,), float('nan'), device=DEV)
        outs.append((name, shape, n, o, o.clone()))
    op = [o.data_ptr() + 4 * off for _, _, _, o, _ in outs]
    if stage == 'tcn_bwd':
        d = _lib.F2sTcnBwdDesc(N=c['N'], Cout=c['Cout'], T=c['T'], V=c['V'], KT=RB.KT, stride=c['stride'], gout=ptr['gout'], out=ptr['out'],
                               h=ptr['h'], wtb=ptr['wtb'], dh=op[0])
        name = 'tamgcn_f2s_tcn_bwd'
        call = lambda st: lib.tamgcn_f2s_tcn_bwd(C.byref(d), st)                      # noqa: E731
    elif stage == 'gcn_bwd':
        d = _lib.F2sGcnBwdDesc(N=c['N'], Cin=c['Cin'], Cout=c['Cout'], T=c['T'], V=c['V'], K=c['K'], stride=c['stride'], res_mode=c['rmode'],
                               dh=ptr['dh'], Ae=ptr['Ae'], wgb=ptr['wgb'], gout=ptr['gout'], out=ptr['out'], wrb=ptr['wrb'], dx=op[0])
        name = 'tamgcn_f2s_gcn_bwd'
        call = lambda st: lib.tamgcn_f2s_gcn_bwd(C.byref(d), st)                      # noqa: E731
    else:
        name = 'tamgcn_saliency_joints'
        call = lambda st: lib.tamgcn_saliency_joints(ptr['dx0'], ptr['c1'], c['N'], c['C'], c['T'], c['V'], c['M'], op[0], op[1], st)   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(call(st), name)
    torch.cuda.synchronize()
    first = [o.clone() for _, _, _, o, _ in outs]
    for _, _, _, o, before in outs:
        o.copy_(before)
    _lib.check(call(st), name)
    torch.cuda.synchronize()
    res = []
    for (oname, shape, n, o, before), f in zip(outs, first):
        assert torch.equal(f[off:off + n].view(torch.int32), o[off:off + n].view(torch.int32)), f'{oname}: second launch differs'
        mask = torch.ones(o.numel(), dtype=torch.bool)
        mask[off:off + n] = False
        B.check_untouched(f'guard of {oname}', o.view(torch.int32), before.view(torch.int32), mask)
        res.append(o[off:off + n].view(shape))
    for k, buf, view, t in keep:                                  # the operands and their canaries are as they were
        assert torch.equal(view.cpu(), t.float().reshape(-1)), k
        assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + t.numel():]).all()), k
    return res


def _case(stage, cid):
    c = {'tcn_bwd': RB.TCN_BWD_CASES, 'gcn_bwd': RB.GCN_BWD_CASES}[stage][cid]
    p = RB.problem(stage, c)
    ref, mag = RB.evaluate(stage, c, p), RB.evaluate(stage, c, p, absval=True)
    (got,) = _run(stage, c, p, [('dh' if stage == 'tcn_bwd' else 'dx', tuple(ref.shape))])
    assert 0.2 < float((p['out'] > 0).float().mean() if p['out'] is not None else 0.5) < 0.8
    err = B.check(f'{stage} {cid}', got, ref, mag, RB.bar_L(stage, c))
    print(f'\n{stage} {cid}: max|err| {err:.3e} (max|ref| {float(ref.abs().max()):.3e}, L = {RB.bar_L(stage, c)})')


@pytest.mark.parametrize('cid', list(RB.TCN_BWD_CASES))
def test_tcn_bwd(cid):
    _case('tcn_bwd', cid)


@pytest.mark.parametrize('cid', list(RB.GCN_BWD_CASES))
def test_gcn_bwd(cid):
    _case('gcn_bwd', cid)


@pytest.mark.parametrize('cid', list(RB.SAL_CASES))
@pytest.mark.parametrize('off', (0, 1))
def test_saliency_joints(cid, off):
    c = dict(RB.SAL_CASES[cid], off=off)
    p = RB.problem('sal', RB.SAL_CASES[cid])
    N, Cc, T, V, M = c['N'], c['C'], c['T'], c['V'], c['M']
    (sal, dxin), (smag, dmag) = RB.saliency_joints(p['dx0'], p['c1'], M), RB.saliency_joints(p['dx0'], p['c1'], M, absval=True)
    got_sal, got_dxin = _run('sal', c, p, [('sal', (N, V)), ('dxin', (N, Cc, T, V, M))])
    e1 = B.check(f'sal {cid}', got_sal, sal, smag, RB.bar_L('sal', c))
    e2 = B.check(f'dxin {cid}', got_dxin, dxin, dmag, 1)
    print(f'\nsaliency_joints {cid}: sal max|err| {e1:.3e} (max|ref| {float(sal.max()):.3e}), dxin max|err| {e2:.3e}')
    # without the optional output: the same saliency bits
    lib = _lib.load()
    alone = torch.full((N, V), float('nan'), device=DEV)
    dx0, c1 = p['dx0'].to(DEV), p['c1'].to(DEV)
    _lib.check(lib.tamgcn_saliency_joints(dx0.data_ptr(), c1.data_ptr(), N, Cc, T, V, M, alone.data_ptr(), None,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'tamgcn_saliency_joints')
    assert torch.equal(alone.view(torch.int32), got_sal.contiguous().view(torch.int32))


def test_saliency_accumulate_equals_its_restatement():
    lib = _lib.load()
    K, V, cap = 5, 20, 3
    parts = [list(v) for v in RB.UCLA_PARTS.values()] + [[0], [1, 19, 7]]
    P = len(parts)
    off = [0]
    for js in parts:
        off.append(off[-1] + len(js))
    d_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    d_j = torch.tensor([j for js in parts for j in js], dtype=torch.int32, device=DEV)
    count = torch.zeros(K, dtype=torch.int32, device=DEV)
    total = torch.zeros(K, P, dtype=torch.float64, device=DEV)
    rc, rt = [0] * K, [[0.0] * P for _ in range(K)]
    g = torch.Generator().manual_seed(5)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, labels in ((7, [0, 0, 1, 0, 0, 3, 1]), (1, [3]), (6, [3, 3, 3, 9, -1, 1]), (300, None)):   # class 2 stays empty until the last batch; 4 never seen
        lab = torch.tensor(labels) if labels is not None else torch.randint(0, 4, (n,), generator=g)
        sal = torch.rand(n, V, generator=g) * 3
        if labels is None:
            sal[::7] = 0
        RB.part_accumulate(rc, rt, sal.double().tolist(), lab.tolist(), parts, cap)
        ds, dl = sal.to(DEV), lab.to(DEV)
        _lib.check(lib.tamgcn_saliency_accumulate(ds.data_ptr(), dl.data_ptr(), n, V, d_off.data_ptr(), d_j.data_ptr(), P, K, cap,
                                                  count.data_ptr(), total.data_ptr(), st), 'tamgcn_saliency_accumulate')
        assert count.cpu().tolist() == rc
        want = torch.tensor(rt, dtype=torch.float64)
        assert float((total.cpu() - want).abs().max()) <= 8 * 2.0 ** -53 * float(want.abs().max())   # sums of <= 3 samples x <= 4 joints
    assert rc == [3, 3, 3, 3, 0]
    for bad in ((0, V, P), (4097, V, P), (4, V, 257)):
        assert lib.tamgcn_saliency_accumulate(ds.data_ptr(), dl.data_ptr(), bad[0], bad[1], d_off.data_ptr(), d_j.data_ptr(), bad[2], K, cap,
                                              count.data_ptr(), total.data_ptr(), st) < 0
        assert b'tamgcn_saliency_accumulate' in lib.tamgcn_last_error()
