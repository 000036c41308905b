"""-m gpu: the ledger of the fused V = 20 CTRGC forward (tamgcn_ctrgc_fwd, csrc/ctrgc.hip): ctrgc_fwd_kernel in its five
instantiations and ctrgc_fwd2_kernel.  Table, fp64 reference and bars: tests/ctrgc_fwd_ref.py.

Every case calls tamgcn_ctrgc_fwd through the raw ABI on operands the test made (a seeded random E; every input in ops.empty
storage with NaN in the slack behind it) and asserts
  * the kernel symbol tamgcn_last_kernel() reports after every launch;
  * y, x3_out and every moment slot part[.][c][n] inside the derived fp64 bars, no element excluded;
  * the write region: outputs pre-filled with NaN are entirely finite afterwards, the sentinel floats behind y, x3_out and
    part are unchanged, every input holds the bits it held before;
  * the four (stats_part, x3_out) pointer combinations: y bit-equal in all four, part and x3 bit-equal wherever produced;
  * A, then other operands B of the same shape, then A again: the two A results bit-equal, B different and inside its own bars;
  * where the case says so, x as channels coff .. coff + Cin of Cin + 8 (the others NaN), x or w3 one float into its storage.

TAMGCN_CTRGC_FWD2 is read once per process, so every case declares its mode: this process runs the cases of its own mode (1
unless the environment says otherwise), test_other_modes_in_children runs this file once per other mode in a child and compares
the digests of the shapes every mode serves (the three 16-channel S = 3 forms promise the same bits).

Run with -s to see the measured err / bound ratios (profiles/ctrgc_fwd_bars.txt records one run)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest
import torch

import ctrgc_fwd_ref as FR
import fp64_bars as B
import test_gpu_ctrgc_routes as L

pytestmark = pytest.mark.gpu

_ENV = os.environ.get('TAMGCN_CTRGC_FWD2')
MODE = int(_ENV) if _ENV is not None else FR.DEFAULT_MODE
DIGEST_DIR = 'TAMGCN_TEST_FWD_DIGEST_DIR'
GUARD, SENT = 64, 12345.0
V = FR.V
DIGESTS = {}                                                       # shape key -> digest of (y, x3, part), this process's mode


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _storage_bits(t):
    """Every float of t's allocation (offset and slack included) as integers, copied."""
    return _bits(torch.empty(0, device=t.device).set_(t.untyped_storage())).clone()


def _buf(n):
    """n NaN floats followed by GUARD sentinel floats, from ops.empty"""
    whole = L._out(n + GUARD)
    whole[n:] = SENT
    return whole


def _operands(c, p):
    d = dict(x=L._dev(p['x'], c.get('xoff', 0)), w3=L._dev(p['w3'], c.get('w3off', 0)), b3=L._dev(p['b3']), E=L._dev(p['E']))
    assert (d['x'].data_ptr() % 16 != 0) == bool(c.get('xoff')) and (d['w3'].data_ptr() % 16 != 0) == bool(c.get('w3off'))
    return d


def _desc(p, dev, N, T, V_=V):
    from tam_gcn_amd import _lib
    d = _lib.CtrgcDesc()
    d.N, d.Cin, d.Cout, d.S, d.R, d.T, d.V = N, p['Cin'], p['Cout'], p['S'], 0, T, V_
    d.x = _lib.Src(dev['x'].data_ptr(), None, None, p['x'].shape[1], p['coff'], 0)
    d.w3, d.b3, d.E = dev['w3'].data_ptr(), dev['b3'].data_ptr(), dev['E'].data_ptr()
    return d


def run(name, sym, p, dev, stats, x3):
    """One launch: {y, x3 or None, part or None} as device tensors.  Symbol, written region and sentinels are asserted here."""
    N, _, T, _ = p['x'].shape
    Cout, S = p['Cout'], p['S']
    shapes = dict(y=(N, Cout, T, V), x3=(N, S * Cout, T, V) if x3 else None, part=(2, Cout, N) if stats else None)
    whole = {k: _buf(torch.Size(s).numel()) for k, s in shapes.items() if s is not None}
    before = {k: w.clone() for k, w in whole.items()}
    ptr = {k: (whole[k].data_ptr() if k in whole else None) for k in shapes}
    L._launch('tamgcn_ctrgc_fwd', sym, C.byref(_desc(p, dev, N, T)), ptr['y'], ptr['part'], ptr['x3'])
    torch.cuda.synchronize()
    out = {k: None for k in shapes}
    for k, w in whole.items():
        n = w.numel() - GUARD
        keep = torch.zeros(w.numel(), dtype=torch.bool)
        keep[n:] = True
        B.check_untouched(f'{name}: floats behind {k}', w, before[k], keep)
        assert bool(torch.isfinite(w[:n]).all()), f'{name}: {k}: {int((~torch.isfinite(w[:n])).sum())} elements not written (or not finite)'
        out[k] = w[:n].view(shapes[k])
    return out


def _same(name, a, b):
    assert torch.equal(_bits(a), _bits(b)), f'{name}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ in their bits'


def ledger_case(cid):
    c = FR.CASES[cid]
    assert c['mode'] == MODE, f'{cid} is a case of mode {c["mode"]}, this process dispatches in mode {MODE}'
    sym = c['sym']
    pA, pB = FR.problem(cid, 0), FR.problem(cid, 1)
    dA, dB = _operands(c, pA), _operands(c, pB)
    was = {(w, k): _storage_bits(t) for w, d in (('A', dA), ('B', dB)) for k, t in d.items()}
    both = run(cid, sym, pA, dA, True, True)
    neither = run(cid + ' [y only]', sym, pA, dA, False, False)
    st = run(cid + ' [stats only]', sym, pA, dA, True, False)
    xo = run(cid + ' [x3 only]', sym, pA, dA, False, True)
    gotB = run(cid + ' [B]', sym, pB, dB, True, True)
    again = run(cid + ' [A again]', sym, pA, dA, True, True)
    for (w, k), bits in was.items():
        assert torch.equal(_storage_bits((dA if w == 'A' else dB)[k]), bits), f'{cid}: input {k} of {w} changed'
    ra = FR.verify(cid, pA, both)
    rb = FR.verify(cid + ' [B]', pB, gotB)
    print(f'FWD {cid} | {sym} | ' + ' '.join(f'{q}={max(ra[q], rb[q]):.3f}' for q in ra))
    for other, nm in ((neither, 'y only'), (st, 'stats only'), (xo, 'x3 only'), (again, 'A again')):
        _same(f'{cid}: y [{nm}] against y [both]', other['y'], both['y'])
    _same(f'{cid}: part [stats only]', st['part'], both['part'])
    _same(f'{cid}: x3 [x3 only]', xo['x3'], both['x3'])
    _same(f'{cid}: part [A again]', again['part'], both['part'])
    _same(f'{cid}: x3 [A again]', again['x3'], both['x3'])
    for k in ('y', 'x3', 'part'):
        assert not torch.equal(_bits(gotB[k]), _bits(both[k])), f'{cid}: {k} of operands B equals that of A'
    if c['xform']:
        h = hashlib.sha256()
        for k in ('y', 'x3', 'part'):
            h.update(both[k].contiguous().cpu().numpy().tobytes())
        DIGESTS[FR.shape_key(c)] = h.hexdigest()
        if os.environ.get(DIGEST_DIR):
            with open(os.path.join(os.environ[DIGEST_DIR], f'{FR.shape_key(c)}.m{MODE}'), 'w') as f:
                f.write(h.hexdigest())


@pytest.mark.parametrize('cid', FR.cases_of(MODE))
def test_fwd_case(cid):
    ledger_case(cid)


def test_other_modes_in_children(tmp_path):
    """The cases of every other dispatch mode, one child process per mode, one after the other; then the digests of the shapes
    every mode serves, across the processes."""
    here = os.path.abspath(__file__)
    root = os.path.dirname(os.path.dirname(here))
    for mode in (m for m in (0, 1, 2, 3) if m != MODE):
        n = len(FR.cases_of(mode))
        out = subprocess.run([sys.executable, '-m', 'pytest', here, '-m', 'gpu', '-x', '-q', '-s', '-k', 'test_fwd_case'], cwd=root,
                             env={**os.environ, 'TAMGCN_CTRGC_FWD2': str(mode), DIGEST_DIR: str(tmp_path)},
                             capture_output=True, text=True, timeout=90 + 10 * n)       # interpreter start-up + a few seconds per case at the very most
        print(''.join(ln[ln.index('FWD '):] + '\n' for ln in out.stdout.splitlines() if 'FWD ' in ln), end='')   # the children's record lines
        assert out.returncode == 0, f'mode {mode}: exit {out.returncode}\n' + out.stdout[-3000:] + out.stderr[-1000:]   # no further child after a failure
        assert f'{n} passed' in out.stdout and 'failed' not in out.stdout, f'mode {mode}: expected {n} passed\n' + out.stdout[-1000:]
    for cid in FR.cases_of(MODE):                                   # this process's own side (run here unless test_fwd_case already did)
        c = FR.CASES[cid]
        if c['xform'] and FR.shape_key(c) not in DIGESTS:
            ledger_case(cid)
    seen = set()
    for N, Cin, T in FR.XFORM:
        key = FR.shape_key(dict(N=N, Cin=Cin, Cout=48, T=T, S=3, sl=0, xoff=0, w3off=0))
        got = {MODE: DIGESTS[key]}
        for mode in (m for m in (0, 1, 2, 3) if m != MODE):
            with open(os.path.join(str(tmp_path), f'{key}.m{mode}')) as f:
                got[mode] = f.read()
        forms = {m: FR.form_key(m, Cin, 48, 3) for m in got}
        seen |= set(forms.values())
        assert len(set(got.values())) == 1, f'{key}: y / x3 / part differ between the forms {forms}: {got}'
    assert seen == {'res16_3', 'l2', 'fwd2'}


# ---------------------------------------------------------------------------------------------------------------------
# refused on the host: the last kernel symbol and every buffer unchanged
# ---------------------------------------------------------------------------------------------------------------------
REFUSALS = {
    'Cout=12': (dict(Cout=12), b'Cout=12 must be a multiple of 8'),
    'S=2': (dict(S=2), b'unsupported S=2 V=20'),
    'V=25': (dict(V=25), b'unsupported S=3 V=25'),
    'x with a prologue': (dict(coef=True), b'x must be a plain tensor'),
    'channel slice out of range': (dict(coff=5), b'x channel slice out of range'),
    'E=NULL': (dict(E=None), b'd->E is NULL'),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refused(what):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    kw, msg = REFUSALS[what]
    ok = FR.make_problem(1, 3, 16, 1, 3, 0, 7)                     # a served launch first: its symbol must survive the refusal
    run('before the refusal', FR.form(MODE, 3, 16, 3), ok, _operands({}, ok), True, True)
    before = lib.tamgcn_last_kernel()
    assert before == FR.form(MODE, 3, 16, 3).encode()
    N, Cin, T = 2, 16, 5
    Cout, S, V_ = kw.get('Cout', 16), kw.get('S', 3), kw.get('V', V)
    g = torch.Generator().manual_seed(11)
    p = dict(x=FR._rnd((N, Cin + 8, T, V_), g), w3=FR._rnd((S * Cout, Cin), g), b3=FR._rnd((S * Cout,), g),
             E=FR._rnd((N, S, Cout, V_, V_), g), coff=kw.get('coff', 4), Cin=Cin + (8 if 'coff' in kw else 0), Cout=Cout, S=S)
    dev = _operands({}, p)
    dev['coef'] = L._dev(FR._rnd((3, Cin + 8), g))
    d = _desc(p, dev, N, T, V_)
    if 'coef' in kw:
        d.x.coef = dev['coef'].data_ptr()
    if 'E' in kw:
        d.E = None
    outs = dict(y=_buf(N * Cout * T * V_), part=_buf(2 * Cout * N), x3=_buf(N * S * Cout * T * V_))
    was = {k: _storage_bits(t) for k, t in {**dev, **outs}.items()}
    rc = lib.tamgcn_ctrgc_fwd(C.byref(d), outs['y'].data_ptr(), outs['part'].data_ptr(), outs['x3'].data_ptr(), ops._stream())
    err = lib.tamgcn_last_error()
    assert rc != 0, f'{what}: accepted'
    assert b'tamgcn_ctrgc_fwd: ' in err and msg in err, err
    assert lib.tamgcn_last_kernel() == before, lib.tamgcn_last_kernel()
    torch.cuda.synchronize()
    for k, t in {**dev, **outs}.items():
        assert torch.equal(_storage_bits(t), was[k]), f'{what}: {k} changed'
