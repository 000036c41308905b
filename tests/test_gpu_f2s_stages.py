"""-m gpu: every case of tests/f2s_ref.py's table as ONE launch of tamgcn_f2s_gcn / tamgcn_f2s_tcn through the raw ABI against
the fp64 restatement of the header's formulas, held to the derived rounding bars (fp64_bars.check; gcn L = 3 (Cin + V), tcn
L = KT Cout + Cres -- tests/f2s_ref.py says why).  Around every launch: the output is NaN-filled beforehand, a NaN canary sits
in the slack behind every operand the kernel streams (a read past an operand poisons the result), a guard region behind the
output must stay untouched, and a second launch must give the same bits.  Cases flagged `off` place every operand one float
past a 16-byte boundary: the dword-aligned path of the weight loads."""
import ctypes as C

import pytest
import torch

import f2s_ref as R
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


def _run(stage, c, p):
    lib = _lib.load()
    off = 1 if c['off'] else 0
    keep, ptr = [], {}
    for k, t in p.items():
        if t is None:
            ptr[k] = None
            continue
        buf, view = _place(t.float().contiguous(), off)
        keep.append((k, buf, view, t))
        ptr[k] = view.data_ptr()
    N, Cout, T, V = c['N'], c['Cout'], c['T'], c['V']
    T2 = T if stage == 'gcn' else (T - 1) // c['stride'] + 1
    n_out = N * Cout * T2 * V
    out = torch.full((off + n_out + GUARD,), float('nan'), device=DEV)
    before = out.clone()
    if stage == 'gcn':
        d = _lib.F2sGcnDesc(N=N, Cin=c['Cin'], Cout=Cout, T=T, V=V, K=c['K'], x=ptr['x'], Ae=ptr['Ae'], wg=ptr['Wg'], bg=ptr['bg'],
                            h=out.data_ptr() + 4 * off)
        fn, name = lib.tamgcn_f2s_gcn, 'tamgcn_f2s_gcn'
    else:
        d = _lib.F2sTcnDesc(N=N, Cin=c['Cin'], Cout=Cout, T=T, V=V, KT=R.KT, stride=c['stride'], res_mode=c['rmode'], h=ptr['h'],
                            wt=ptr['Wt'], bt=ptr['bt'], x=ptr['x'], wr=ptr['Wr'], br=ptr['br'], out=out.data_ptr() + 4 * off)
        fn, name = lib.tamgcn_f2s_tcn, 'tamgcn_f2s_tcn'
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fn(C.byref(d), st), name)
    torch.cuda.synchronize()
    first = out.clone()
    out.copy_(before)
    _lib.check(fn(C.byref(d), st), name)
    torch.cuda.synchronize()
    assert torch.equal(first[off:off + n_out].view(torch.int32), out[off:off + n_out].view(torch.int32)), 'second launch differs'
    mask = torch.ones(out.numel(), dtype=torch.bool)
    mask[off:off + n_out] = False
    B.check_untouched('guard', out.view(torch.int32), before.view(torch.int32), mask)
    for k, buf, view, t in keep:                                  # the operands and their canaries are as they were
        assert torch.equal(view.cpu(), t.float().reshape(-1)), k
        assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + t.numel():]).all()), k
    return out[off:off + n_out].view(N, Cout, T2, V)


def _case(stage, cid):
    c = (R.GCN_CASES if stage == 'gcn' else R.TCN_CASES)[cid]
    p = R.problem(stage, c)
    ref, mag = R.evaluate(stage, c, p), R.evaluate(stage, c, p, absval=True)
    got = _run(stage, c, p)
    err = B.check(f'{stage} {cid}', got, ref, mag, R.bar_L(stage, c))
    print(f'\n{stage} {cid}: max|err| {err:.3e} (max|ref| {float(ref.abs().max()):.3e}, L = {R.bar_L(stage, c)})')


@pytest.mark.parametrize('cid', list(R.GCN_CASES))
def test_gcn(cid):
    _case('gcn', cid)


@pytest.mark.parametrize('cid', list(R.TCN_CASES))
def test_tcn(cid):
    _case('tcn', cid)
