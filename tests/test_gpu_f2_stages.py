"""-m gpu: the ledger of the small-batch eval kernels (csrc/f2.hip, csrc/f2v.hip): every stage of both families, launched
through its descriptor on the tables of tests/f2_ref.py, the kernel symbol pinned, every output held element by element to
the derived rounding bar of its fp64 reference (f2_ref's docstring), no element excluded.

Around every launch: each operand lives inside its own NaN-filled buffer (guards in front and behind; the 12 bytes the V = 25
family may read past a contiguous input are NaN too); outputs are pre-filled with NaN, so an element the kernel leaves out
fails its bar; afterwards every guard and every input must hold the bits it held before.  For V = 25 the pad joints
(columns 25..27) of every INPUT in 28-float frames hold NaN (gemm's x / add, tcn's h, gcn's E, e's xpart): every joint
column must still be finite and inside its bar, and the pad joints of E, sum, diff and xpart must come out exactly zero
(include/tamgcn.h).  An `off` case runs a second time with its weight arrays one float past a 16-byte boundary (scalar
A-fragment path): bit-equal.  A grouped case runs the plain entry point per group, then the grouped twin: bit-equal slices.

`pytest -s` prints one line per case, family and output: worst err / bar and the tanh-attributable error
(profiles/f2_stage_bars.txt keeps one run)."""
import zlib

import pytest
import torch

import fp64_bars as B
import f2_ref as R

pytestmark = pytest.mark.gpu

from tam_gcn_amd import _lib                                                       # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')
GUARD = 8                                                          # floats in front of and behind every operand (32 bytes)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Bufs:
    """device operands, each inside a NaN-filled allocation of its own"""

    def __init__(self):
        self.items = []

    def put(self, name, t, off=0, out=False):
        """t: a CPU tensor (its values are the input; out=True: only its shape counts, the buffer stays NaN).  off: floats
        past the 16-byte boundary."""
        if t is None:
            return None
        n = t.numel()
        whole = torch.full((GUARD + off + n + GUARD,), NAN, device=DEV)
        assert whole.data_ptr() % 16 == 0
        view = whole[GUARD + off:GUARD + off + n].view(t.shape)
        if not out:
            view.copy_(t)
        keep = torch.ones(whole.numel(), dtype=torch.bool)
        if out:
            keep[GUARD + off:GUARD + off + n] = False
        self.items.append((name, whole, _bits(whole), keep))
        return view

    def check(self, what):
        for name, whole, before, keep in self.items:
            B.check_untouched(f'{what}: {name} (inputs and the guards around every operand)', _bits(whole), before, keep)


def _seed(cid):
    return zlib.crc32(cid.encode()) & 0xffff


def _fr(t, V):
    """logical -> the family's frames, NaN in the pad joints"""
    return None if t is None else R.to_frames(t, V, NAN)


def _zero_pads(what, pads):
    if pads.numel() and not bool((pads == 0).all()):
        raise B.BarError(f'{what}: {int((pads != 0).sum())} pad-joint elements are not exactly zero')


def _shape(*s):
    return torch.empty(*s, device='meta')


# ---------------------------------------------------------------------------------------------------------------------
# one launch per stage: operands -> descriptor -> (rc, outputs in the logical layout)
# ---------------------------------------------------------------------------------------------------------------------
def prepare(stage, fam, p, off=False):
    """-> (Bufs, descriptor, dict of the device views)"""
    V, P = R.FAMILIES[fam], R.vp(R.FAMILIES[fam])
    N, T, o = p['N'], p['T'], 1 if off else 0
    bufs, t = Bufs(), {}
    if stage in ('e', 'gcn'):
        Cout = p['Cout']
        for k in ('w12', 'w4', 'w3', 'wd'):
            t[k] = bufs.put(k, p[k], off=o)
        for k in ('b12', 'b4', 'A', 'alpha', 'b3', 'sy', 'ty', 'bd'):
            t[k] = bufs.put(k, p[k])
        t['x'] = bufs.put('x', p['x'])
        t['xpart'] = bufs.put('xpart', _fr(p['xpart'], V))
        if stage == 'e':
            t['E'] = bufs.put('E', _shape(N, R.S, Cout, V, P), out=True)
            t['sum'] = bufs.put('sum', torch.full((N, Cout, T, P), NAN))          # not touched by the e stage
            t['diff'] = bufs.put('diff', torch.full((N, Cout, T, P), NAN))
        else:
            t['E'] = bufs.put('E', _fr(p['E'], V))
            t['sum'] = bufs.put('sum', _shape(N, Cout, T, P), out=True)
            t['diff'] = bufs.put('diff', _shape(N, Cout, T, P), out=True)
    elif stage == 'gemm':
        t['x'] = bufs.put('x', _fr(p['x'], V))
        t['add'] = bufs.put('add', _fr(p['add'], V) if p['mode'] == 0 else None)
        t['w'], t['b'] = bufs.put('w', p['w'], off=o), bufs.put('b', p['b'])
        t['out'] = bufs.put('out', _shape(N, p['M'], T, P), out=True)
    else:
        T2 = (T - 1) // p['stride'] + 1
        t['h'] = bufs.put('h', _fr(p['h'], V))
        t['x'] = bufs.put('x', p['x'])
        t['wt'] = [bufs.put(f'wt{i}', w, off=o) for i, w in enumerate(p['wt'])]
        t['bt'] = [bufs.put(f'bt{i}', b) for i, b in enumerate(p['bt'])]
        t['sp'], t['tp'] = bufs.put('sp', p['sp']), bufs.put('tp', p['tp'])
        t['wr'], t['br'] = bufs.put('wr', p['wr'], off=o), bufs.put('br', p['br'])
        t['out'] = bufs.put('out', _shape(N, p['Cout'], T2, V), out=True)
        t['xpart'] = bufs.put('xpart', _shape(N, -(-T2 // R.BT), p['Cout'], P), out=True) if p['xpart'] else None
    return bufs, R.DESC[stage](_lib, p, V, t), t


def run(stage, fam, p, off=False, groups=None):
    """launch and collect: {output: CPU tensor in the logical layout}; the symbol, the guards and the zero pad joints checked"""
    lib = _lib.load()
    V = R.FAMILIES[fam]
    what = f'{fam}_{stage}{"_grouped" if groups else ""}'
    bufs, d, t = prepare(stage, fam, p, off)
    rc = R.launch(lib, fam, stage, d, groups, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (what, lib.tamgcn_last_error())
    assert lib.tamgcn_last_kernel() == f'{what}_kernel'.encode(), lib.tamgcn_last_kernel()
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                                    # a device fault: nothing more is launched in this session
        pytest.exit(f'{what}: {err}', returncode=3)
    bufs.check(what)
    out = {}
    if stage == 'e':
        out['E'], pads = R.from_frames(t['E'].cpu(), V)
        _zero_pads(f'{what}: E', pads)
    elif stage == 'gcn':
        for k in ('sum', 'diff'):
            out[k], pads = R.from_frames(t[k].cpu(), V)
            _zero_pads(f'{what}: {k}', pads)
    elif stage == 'gemm':
        out['out'], _ = R.from_frames(t['out'].cpu(), V)        # its pad joints hold the epilogue of the inputs' pad joints
    else:
        out['out'] = t['out'].cpu()
        if t['xpart'] is not None:
            out['xpart'], pads = R.from_frames(t['xpart'].cpu(), V)
            _zero_pads(f'{what}: xpart', pads)
    return out


def check(stage, name, p, out):
    if stage == 'e':
        return R.check_e(name, p, out['E'])
    if stage == 'gcn':
        return R.check_gcn(name, p, out['sum'], out['diff'], p['V'])
    if stage == 'gemm':
        return R.check_gemm(name, p, out['out'])
    return R.check_tcn(name, p, out['out'], out.get('xpart'))


def ledger_case(stage, cid, fam):
    c = R.STAGES[stage][cid]
    V, G = R.FAMILIES[fam], c['G']
    p = R.problem(stage, c, V, _seed(cid))
    npg = c['N'] // G
    plain, worst = [], {}
    for g in range(G):
        q = R.sub(stage, p, g)
        out = run(stage, fam, q)
        for k, (r, ta) in check(stage, f'{fam}_{stage} {cid}' + (f' group {g}' if G > 1 else ''), q, out).items():
            w = worst.get(k, (0.0, None))
            worst[k] = (max(w[0], r), ta if w[1] is None else max(w[1], ta))
        if c['off']:
            shifted = run(stage, fam, q, off=True)
            for k in out:
                assert torch.equal(shifted[k], out[k]), f'{cid}: {k}: weights one float off the boundary change the result'
        plain.append(out)
    if G > 1:
        whole = run(stage, fam, p, groups=G)
        for g in range(G):
            for k in whole:
                assert torch.equal(whole[k][g * npg:(g + 1) * npg], plain[g][k]), f'{cid}: {k}: group {g} differs from the plain launch'
    for k, (r, ta) in worst.items():
        print(f'\nF2BARS {stage:4s} {cid:32s} {fam:3s} {k:8s} err/bar {r:.3f}' + ('' if ta is None else f'  tanh-attributable {ta:.3e}'), end='')


def _params(stage):
    return [(cid, fam) for cid in R.STAGES[stage] for fam in R.FAMILIES]


@pytest.mark.parametrize('cid, fam', _params('e'))
def test_e(cid, fam):
    ledger_case('e', cid, fam)


@pytest.mark.parametrize('cid, fam', _params('gcn'))
def test_gcn(cid, fam):
    ledger_case('gcn', cid, fam)


@pytest.mark.parametrize('cid, fam', _params('gemm'))
def test_gemm(cid, fam):
    ledger_case('gemm', cid, fam)


@pytest.mark.parametrize('cid, fam', _params('tcn'))
def test_tcn(cid, fam):
    ledger_case('tcn', cid, fam)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: on the host, before any launch.  Every pointer is a real buffer sized for the descriptor that is refused.
# (case overrides before the operands are made, descriptor edits after, message fragment, groups)
# ---------------------------------------------------------------------------------------------------------------------
def _misalign(field):
    def f(d):
        setattr(d, field, getattr(d, field) + 4)
    return f


def _set(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


_GCN_BASE = dict(R.GCN_CASES['cin16_res2_t9'], G=1, N=2)
_GCN_REFUSED = {
    'wrong_V': ({}, lambda d: setattr(d, 'V', 45 - d.V), b'V=', None),
    'wrong_S': ({}, _set(S=2), b'S=2', None),
    'cin257': (dict(Cin=257), None, b'bad shape', None),
    'cout24': (dict(Cout=24), None, b'bad shape', None),
    'r0': ({}, _set(R=0), b'R=0 outside 1..32', None),            # (an array of no elements has no address: the R = 8 operands stay)
    'r33': (dict(R=33), None, b'R=33 outside 1..32', None),
    'identity_cin_ne_cout': (dict(res_mode=1), None, b'identity residual', None),
    'conv_without_weights': ({}, _set(wd=None, bd=None), b'convolutional residual without weights', None),
    'misaligned_E': ({}, _misalign('E'), b'aligned', None),
    'groups_do_not_divide': (dict(N=3), None, b'not a multiple of groups', 2),
}
_GEMM_BASE = dict(R.GEMM_CASES['k48_m48_mode0_t9'], G=1, N=2)
_GEMM_REFUSED = {
    'wrong_V': ({}, lambda d: setattr(d, 'V', 45 - d.V), b'V=', None),
    'k257': (dict(K=257), None, b'bad shape', None),
    'm24': (dict(M=24), None, b'bad shape', None),
    'mode0_without_add': ({}, _set(add=None), b'mode 0 needs the addend', None),
    'misaligned_x': ({}, _misalign('x'), b'aligned', None),
    'groups_do_not_divide': (dict(N=3), None, b'not a multiple of groups', 2),
}


def _tcn_case(cout=None, cin=None, **kw):
    c = dict(R.TCN_CASES['nb2_cb16_k5_s2_res2_cin3_t8'], G=1, N=2)
    c.update(kw)
    c['Cout'] = cout or (c['nb'] + 2) * c['Cb']
    if cin is not None or c['res_mode'] == 1:
        c['Cin'] = cin or c['Cout']
    return c


_TCN_REFUSED = {
    'wrong_V': (_tcn_case(), lambda d: setattr(d, 'V', 45 - d.V), b'V=', None),
    'nb5': (_tcn_case(nb=5, dils=(1, 1, 1, 1, 1)), None, b'nb=5', None),
    'cb80': (_tcn_case(Cb=80), None, b'Cb=80', None),
    'cout_mismatch': (_tcn_case(cout=80), None, b'(nb + 2) Cb == Cout', None),
    'even_ks': (_tcn_case(ks=4), None, b'kernel size 4', None),
    'identity_cin_ne_cout': (_tcn_case(res_mode=1, stride=1, cin=48), None, b'identity residual', None),
    'identity_stride2': (_tcn_case(res_mode=1, stride=2), None, b'identity residual', None),
    'conv_without_weights': (_tcn_case(), _set(wr=None, br=None), b'convolutional residual', None),
    'conv_cin257': (_tcn_case(cin=257), None, b'Cin=257', None),
    'misaligned_h': (_tcn_case(), _misalign('h'), b'aligned', None),
    'groups_do_not_divide': (_tcn_case(N=3), None, b'not a multiple of groups', 2),
}
for _s, _pairs in R.AT_LIMIT.items():
    for _ks, _d in _pairs:                                         # one dilation step past every at-limit pair of the table
        _TCN_REFUSED[f'halo_k{_ks}d{_d + 1}_s{_s}'] = (_tcn_case(ks=_ks, dils=(1, _d + 1), stride=_s, res_mode=0), None, b'halo of', None)

_REFUSED = {'e': (_GCN_BASE, _GCN_REFUSED), 'gcn': (_GCN_BASE, dict(_GCN_REFUSED, misaligned_sum=({}, _misalign('sum'), b'misaligned output', None))),
            'gemm': (_GEMM_BASE, _GEMM_REFUSED), 'tcn': (None, _TCN_REFUSED)}


@pytest.mark.parametrize('fam', list(R.FAMILIES))
@pytest.mark.parametrize('stage', list(_REFUSED))
def test_refusals(stage, fam):
    lib = _lib.load()
    V = R.FAMILIES[fam]
    # a launch of ANOTHER stage first: the symbol it leaves must still be the last one after every refusal
    other = 'gemm' if stage != 'gemm' else 'tcn'
    oc = next(iter(R.STAGES[other]))
    run(other, fam, R.sub(other, R.problem(other, R.STAGES[other][oc], V, 1), 0))
    before = lib.tamgcn_last_kernel()
    base, table = _REFUSED[stage]
    for rid, (over, edit, frag, groups) in table.items():
        c = dict(base, **over) if base is not None else over
        if groups:                                                 # the grouped layout: every parameter array `groups` times
            p = R.problem(stage, dict(c, G=groups), V, 2)
        else:
            p = R.sub(stage, R.problem(stage, c, V, 2), 0)
        bufs, d, _ = prepare(stage, fam, p)
        if edit is not None:
            edit(d)
        rc = R.launch(lib, fam, stage, d, groups, torch.cuda.current_stream().cuda_stream)
        msg = lib.tamgcn_last_error()
        assert rc != 0, f'{fam}_{stage} {rid}: accepted'
        assert frag in msg, (rid, msg)
        assert lib.tamgcn_last_kernel() == before, (rid, lib.tamgcn_last_kernel())
        torch.cuda.synchronize()
        bufs.check(f'{fam}_{stage} {rid} (refused)')
        for name, whole, was, keep in bufs.items:                  # nothing was written anywhere, outputs included
            assert torch.equal(_bits(whole), was), (rid, name)
