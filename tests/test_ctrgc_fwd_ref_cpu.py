"""CPU: the fused-forward ledger (tests/test_gpu_ctrgc_fwd_forms.py, tests/ctrgc_fwd_ref.py): the dispatch mirror is the source's
dispatch, the table reaches every forward instantiation and every path it promises, an fp32 torch evaluation of every case stays
inside every bar, and the bars have teeth."""
import itertools
import os
import re

import pytest
import torch

import ctrgc_fwd_ref as FR
import fp64_bars as B

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the mirror against the source text of tamgcn_ctrgc_fwd
# ---------------------------------------------------------------------------------------------------------------------
def _source():
    src = open(os.path.join(CSRC, 'ctrgc.hip')).read()
    body = src[src.index('extern "C" int tamgcn_ctrgc_fwd('):]
    return src, body[:body.index('\n}\n')]


def _py(expr):
    """A C condition over d->Cin, d->S, ct, mode, two, al16 as a Python expression"""
    expr = re.sub(r'(.+?) \? (.+?) : (.+)', r'((\2) if (\1) else (\3))', expr) if '?' in expr else expr
    return expr.replace('d->', '').replace('&&', ' and ').replace('||', ' or ')


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def source_dispatch():
    """form key by (mode, Cin, Cout, S, x_aligned, w3_aligned) as the SOURCE decides it, its default mode, its symbols"""
    src, body = _source()
    geo = {k: v for k, v in re.findall(r'using (G20W?) = (Geo<[^>]*>);', src)}
    assert geo == {'G20': FR.G20, 'G20W': FR.G20W}, geo
    ct_expr = _py(_one(r'static int fwd_ct\(int Cout\) \{ return (.*?); \}', src))
    assert 'const int ct = fwd_ct(d->Cout);' in body
    default = int(_one(r'getenv\("TAMGCN_CTRGC_FWD2"\); return e \? atoi\(e\) : (\d+);', body))
    assert 'const bool al16 = (((uintptr_t)d->x.x1 | (uintptr_t)d->w3) & 15) == 0;' in body
    two_expr = _py(_one(r'const bool two = (.*?);', body))
    # the chain: if (fwd2 condition) fwd2  else if (two) E from L2  else if (ct == 16) resident 16  else resident 8, each by S
    chain = re.findall(r'^    (if|\} else if|\} else) ?(?:\((.*)\) )?\{$', body, re.M)
    assert [k for k, _ in chain] == ['if', '} else if', '} else if', '} else'], chain
    fwd2_expr, two_only, ct16 = (_py(e) for _, e in chain[:3])
    assert two_only == 'two'
    blocks = re.split(r'^    (?:if|\} else if|\} else) ?(?:\(.*\) )?\{$', body, flags=re.M)[1:]
    assert len(blocks) == 4
    launched = []
    for blk in blocks:
        direct = re.findall(r'tg_launch_lds<(ctrgc_\w+)<([^<>()]*)>>', blk)
        macro = re.findall(r'if \(d->S == 3\) CTRGC_LAUNCH\((\w+), (G20W?), 3, .*\n\s*else CTRGC_LAUNCH\((\w+), (G20W?), 1, ', blk)
        assert len(direct) + len(macro) == 1, blk
        launched.append(direct[0] if direct else macro[0])
    assert launched == [('ctrgc_fwd2_kernel', 'G20W, 3, 2'), ('ctrgc_fwd_kernel', 'G20W, 3, false'),
                        ('ctrgc_fwd_kernel', 'G20W', 'ctrgc_fwd_kernel', 'G20W'), ('ctrgc_fwd_kernel', 'G20', 'ctrgc_fwd_kernel', 'G20')], launched
    # symbols: the two literal notes, and the macro's
    notes = re.findall(r'tamgcn_note_kernel\("([^"]*)", (G20W?)::V, \2::CT, \2::TB, \2::NTQ, \2::SBK\);', body)
    assert len(notes) == 2, notes
    sym = {k: fmt.replace('Geo<%d, %d, %d, %d, %d>', geo[g]) for k, (fmt, g) in zip(('fwd2', 'l2'), notes)}
    mfmt = _one(r'tamgcn_note_kernel\(#KERNEL "([^"]*)", GEO::V, GEO::CT, GEO::TB, GEO::NTQ, GEO::SBK, ST_\);', src)
    for g, tag in (('G20W', 'res16'), ('G20', 'res8')):
        for s in (3, 1):
            sym[f'{tag}_{s}'] = 'ctrgc_fwd_kernel' + mfmt.replace('Geo<%d, %d, %d, %d, %d>', geo[g]).replace('%d', str(s))

    def decide(mode, Cin, Cout, S, xa, wa):
        env = dict(mode=mode, Cin=Cin, S=S, al16=xa and wa, ct=eval(ct_expr, {}, dict(Cout=Cout)))
        env['two'] = bool(eval(two_expr, {}, env))
        if eval(fwd2_expr, {}, env):
            return 'fwd2'
        if env['two']:
            return 'l2'
        return ('res16_' if eval(ct16, {}, env) else 'res8_') + str(S)
    return decide, default, sym


def test_dispatch_mirror_is_the_source():
    decide, default, sym = source_dispatch()
    assert default == FR.DEFAULT_MODE
    assert sym == FR.SYM
    cins = [1, 3, 15, 16, 17, 31, 32, 48, 63, 64, 65, 72, 80, 128, 255, 256, 257, 260, 272, 512]
    for mode, Cin, Cout, S, xa, wa in itertools.product((0, 1, 2, 3), cins, (8, 16, 24, 32, 40, 48), (1, 3), (True, False), (True, False)):
        assert FR.form_key(mode, Cin, Cout, S, xa, wa) == decide(mode, Cin, Cout, S, xa, wa), (mode, Cin, Cout, S, xa, wa)
        assert FR.form(mode, Cin, Cout, S, xa, wa) == sym[decide(mode, Cin, Cout, S, xa, wa)]
    assert FR.fwd_ct(24) == 8 and FR.fwd_ct(48) == 16
    for cid, c in FR.CASES.items():                                # the table's symbols are the dispatch's
        assert c['sym'] == sym[decide(c['mode'], c['Cin'], c['Cout'], c['S'], not c['xoff'], not c['w3off'])], cid


def test_the_mirror_test_fails_when_the_dispatch_changes(monkeypatch):
    """The same comparison against a source whose fwd2 threshold moved: it must not pass."""
    src, _ = _source()
    assert src.count('mode == 1 && d->Cin >= 256') == 1
    changed = src.replace('mode == 1 && d->Cin >= 256', 'mode == 1 && d->Cin >= 128')
    real_open = open

    def fake(path, *a, **kw):
        if str(path).endswith('ctrgc.hip'):
            import io
            return io.StringIO(changed)
        return real_open(path, *a, **kw)
    monkeypatch.setattr('builtins.open', fake)
    decide, _, _ = source_dispatch()
    assert decide(1, 128, 16, 3, True, True) == 'fwd2' and FR.form_key(1, 128, 16, 3) == 'l2'


# ---------------------------------------------------------------------------------------------------------------------
# completeness
# ---------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_forward_instantiation_and_every_required_path():
    import test_ctrgc_ref_cpu as RC
    fwd = {k for k in RC.source_symbols() if k.startswith(('ctrgc_fwd_kernel<', 'ctrgc_fwd2_kernel<'))}
    assert fwd == set(FR.INSTANTIATION.values()), fwd
    reached = {c['form'] for c in FR.CASES.values()}
    assert reached == set(FR.SYM) == set(FR.INSTANTIATION) == set(FR.required_paths)
    for fk, need in FR.required_paths.items():
        have = set().union(*(FR.features(c) for c in FR.CASES.values() if c['form'] == fk))
        assert not [n for n in need if n not in have], (fk, [n for n in need if n not in have])
    assert {c['form'] for c in FR.CASES.values() if c['mode'] == FR.DEFAULT_MODE} == set(FR.SYM)     # all six in the pytest process itself


def test_table_holds_the_shapes_it_promises():
    m1 = [c for c in FR.CASES.values() if c['mode'] == 1 and not c['xform']]
    for fk in FR.SYM:                                               # every T, N and Cout of the lists at least twice per form
        cs = [c for c in m1 if c['form'] == fk]
        couts = FR.CO8 if fk.startswith('res8') else FR.CO16
        for key, vals in (('T', FR.TS), ('N', FR.NS), ('Cout', couts)):
            for v in vals:
                assert sum(c[key] == v for c in cs) >= 2, (fk, key, v)
        assert sum(c['sl'] for c in cs) >= 2, fk

    def cins(mode, fk, **kw):
        return sorted({c['Cin'] for c in FR.CASES.values() if c['mode'] == mode and c['form'] == fk and not c['xform']
                       and all(c[k] == v for k, v in kw.items())})
    assert cins(1, 'res16_3') == [3, 35, 48] and cins(1, 'res16_1') == [3, 80, 96]
    assert cins(1, 'l2') == [64, 72, 128, 256, 260] and cins(1, 'l2', w3off=1) == [256] and cins(1, 'l2', xoff=1) == [256]
    assert cins(1, 'fwd2') == [256, 272] and cins(1, 'res8_3') == cins(1, 'res8_1') == [3, 16, 20, 64]
    for sl in (0, 1):
        assert {c['T'] for c in m1 if c['form'] == 'fwd2' and c['Cin'] == 256 and c['sl'] == sl} == set(FR.TS)
    assert cins(2, 'fwd2') == [16, 32, 48, 80] and cins(2, 'fwd2', sl=1) == [32] and cins(2, 'l2') == [3, 16, 20] and cins(2, 'l2', w3off=1) == [16]
    assert {c['T'] for c in FR.CASES.values() if c['mode'] == 2 and c['form'] == 'fwd2'} == {1, 17, 33, 40}
    assert cins(3, 'l2') == [3, 16, 48, 256] and cins(0, 'res16_3') == [64, 256]
    assert all(c['T'] % 16 for c in FR.CASES.values() if c['mode'] == 3 and not c['xform'])
    assert {c['T'] for c in FR.CASES.values() if c['mode'] == 0 and not c['xform']} == {33}
    x = [c for c in FR.CASES.values() if c['xform']]
    assert {c['Cin'] for c in x} == {16, 64, 256} and {c['T'] for c in x} == {17, 40} and {c['Cout'] for c in x} == {48}
    for N, Cin, T in FR.XFORM:
        assert {FR.form_key(m, Cin, 48, 3) for m in (0, 1, 2, 3)} == {'res16_3', 'l2', 'fwd2'}
        assert sum(c['xform'] and (c['N'], c['Cin'], c['T']) == (N, Cin, T) for c in FR.CASES.values()) == 4
    assert all(c['N'] <= 9 and c['T'] <= 40 and c['Cout'] <= 48 and c['S'] in (1, 3) for c in FR.CASES.values())
    # the same shape in another mode has the same operands
    a, b = FR.problem('m0_res16_3_N1_Ci64_Co48_T40_S3_x'), FR.problem('m2_fwd2_N1_Ci64_Co48_T40_S3_x')
    assert all(torch.equal(a[k], b[k]) for k in ('w3', 'b3', 'E')) and torch.equal(a['x'].nan_to_num(7.0), b['x'].nan_to_num(7.0))
    assert not torch.equal(FR.problem('m2_fwd2_N1_Ci64_Co48_T40_S3_x', 1)['E'], b['E'])


# ---------------------------------------------------------------------------------------------------------------------
# the reference alone stays inside every bar
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _case(cid):
    if cid not in _CACHE:
        p = FR.problem(cid)
        _CACHE[cid] = (p, FR.evaluate(p, F32))
    return _CACHE[cid]


_UNIQUE = {}
for _cid, _c in FR.CASES.items():                                   # one evaluation per shape (the modes share operands)
    _UNIQUE.setdefault(FR.shape_key(_c), _cid)


@pytest.mark.parametrize('cid', list(_UNIQUE.values()))
def test_checker_accepts_fp32_torch(cid):
    p, got = _case(cid)
    rat = FR.verify(cid, p, got)
    assert set(rat) == {'x3', 'y', 'part'} and max(rat.values()) <= 1.0
    assert set(FR.verify(cid, p, dict(y=got['y'], x3=None, part=None))) == {'y'}


def test_reference_is_the_einsum_of_the_older_tests():
    p = FR.make_problem(2, 5, 16, 3, 3, 1, 3)
    x = p['x'][:, 4:9].double()
    x3 = torch.einsum('oc,nctv->notv', p['w3'].double(), x) + p['b3'].double()[None, :, None, None]
    y = sum(torch.einsum('ncuv,nctv->nctu', p['E'][:, s].double(), x3[:, s * 16:(s + 1) * 16]) for s in range(3))
    rx3, ry = FR.reference(p)
    assert float((rx3 - x3).abs().max()) <= 1e-14 and float((ry - y).abs().max()) <= 1e-13
    part = FR.moments(y)
    assert tuple(part.shape) == (2, 16, 2)
    assert float((part[0, 5, 1] - y[1, 5].sum()).abs()) <= 1e-13 and float((part[1, 5, 1] - (y[1, 5] ** 2).sum()).abs()) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# the bars reject what a subtly wrong kernel would deliver
# ---------------------------------------------------------------------------------------------------------------------
RAGGED = [cid for cid, c in FR.CASES.items() if c['form'] == 'res16_3' and c['T'] == 33 and c['N'] == 3 and c['mode'] != 1][0]   # chunks 16 + 16 + 1
KTAIL = [[cid for cid, c in FR.CASES.items() if c['mode'] == 1 and c['Cin'] == k][0] for k in (35, 72, 20, 260)]   # one per form with a tail
SLICED = [cid for cid, c in FR.CASES.items() if c['sl'] and c['mode'] == 1 and c['form'] in ('fwd2', 'res8_3', 'l2')]


def _rejects(cid, p, got, **over):
    FR.verify(cid, p, got)
    with pytest.raises(B.BarError):
        FR.verify(cid, p, dict(got, **over))


def _with(p, **kw):
    return FR.evaluate(dict(p, **kw), F32)


def test_rejects_the_last_chunk_taken_from_the_previous_one():
    p, got = _case(RAGGED)
    assert FR.CASES[RAGGED]['T'] == 33
    y = got['y'].clone()
    y[:, :, 32:] = got['y'][:, :, 16:17]
    _rejects(RAGGED, p, got, y=y, part=FR.moments(y, F32))
    x3 = got['x3'].clone()
    x3[:, :, 32:] = got['x3'][:, :, 16:17]
    _rejects(RAGGED, p, got, x3=x3)


def test_rejects_a_dropped_k_tail():
    for cid in KTAIL:
        p, got = _case(cid)
        full = p['Cin'] - p['Cin'] % FR.SBK[FR.CASES[cid]['form']]     # the whole stages only
        assert 0 < full < p['Cin']
        w3 = p['w3'].clone()
        w3[:, full:] = 0
        bad = _with(p, w3=w3)
        _rejects(cid, p, got, x3=bad['x3'])
        _rejects(cid, p, got, y=bad['y'], part=bad['part'])


def test_rejects_a_missing_subset_b3_left_out_and_E_transposed():
    for cid in (RAGGED, 'm1_fwd2_N3_Ci272_Co32_T33_S3'):
        p, got = _case(cid)
        E = p['E'].clone()
        E[:, 2] = 0
        _rejects(cid, p, got, y=_with(p, E=E)['y'])
        nob = _with(p, b3=torch.zeros_like(p['b3']))
        _rejects(cid, p, got, x3=nob['x3'])
        _rejects(cid, p, got, y=nob['y'], part=nob['part'])
        _rejects(cid, p, got, y=_with(p, E=p['E'].transpose(-1, -2).contiguous())['y'])


def test_rejects_subset_rows_of_x3_swapped():
    p, got = _case(RAGGED)
    N, SC, T, V = got['x3'].shape
    sw = got['x3'].view(N, 3, SC // 3, T, V)[:, [0, 2, 1]].reshape(N, SC, T, V)
    _rejects(RAGGED, p, got, x3=sw)
    y = torch.einsum('nscuv,nsctv->nctu', p['E'], sw.view(N, 3, SC // 3, T, V))
    _rejects(RAGGED, p, got, y=y, part=FR.moments(y, F32))


def test_rejects_moments_without_the_last_chunk_and_slots_transposed():
    p, got = _case(RAGGED)
    _rejects(RAGGED, p, got, part=FR.moments(got['y'][:, :, :32], F32))
    N, C = got['y'].shape[:2]
    assert N == 3
    t = torch.stack([got['part'][i].t().contiguous().view(C, N) for i in (0, 1)])      # written at [n][c], read as [c][n]
    _rejects(RAGGED, p, got, part=t)
    one = got['part'].clone()
    one[1, 7, 2] = got['part'][1, 7, 1]
    _rejects(RAGGED, p, got, part=one)


def test_rejects_a_nan_neighbour_channel_leaking():
    assert len(SLICED) >= 3
    for cid in SLICED[:3]:
        p, got = _case(cid)
        assert bool(torch.isnan(p['x'][:, p['coff'] - 1]).all() and torch.isnan(p['x'][:, p['coff'] + p['Cin']]).all())
        for coff in (p['coff'] - 1, p['coff'] + 1):                # the slice one channel early / late
            bad = _with(p, coff=coff)
            _rejects(cid, p, got, x3=bad['x3'])
            _rejects(cid, p, got, y=bad['y'])
        y = got['y'].clone()
        y[-1, -1, -1, -1] = float('nan')                          # into one output only
        _rejects(cid, p, got, y=y)
        x3 = got['x3'].clone()
        x3[0, 0, 0, 0] = float('nan')
        _rejects(cid, p, got, x3=x3)
        part = got['part'].clone()
        part[1, 0, 0] = float('nan')
        _rejects(cid, p, got, part=part)
