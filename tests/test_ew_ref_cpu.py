"""CPU: the ledger of the row-streaming kernels and BatchNorm finalisers (tests/test_gpu_ew_forms.py) stays complete, its
fp64 references (tests/ew_ref.py) are autograd's formulas on the composites they belong to, an fp32 torch evaluation of
every GPU case stays inside every bar (and the reference alone leaves out at most 0.1 % of a case's decisions), and the bars
reject what a subtly wrong kernel would deliver."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ew_ref as R
import fp64_bars as B
import test_gpu_ew_forms as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tam_gcn_amd', 'csrc')
F64, F32 = torch.float64, torch.float32
EPS = float(np.float32(1e-5))


# ---------------------------------------------------------------------------------------------------------------------
# ledger completeness
# ---------------------------------------------------------------------------------------------------------------------
def launched():
    """every kernel (with its literal template arguments) behind a hipLaunchKernelGGL( of elementwise.hip and bn.hip"""
    found = []
    for name in ('elementwise.hip', 'bn.hip'):
        src = open(os.path.join(CSRC, name)).read()
        found += [k + (a or '') for k, a in re.findall(r'hipLaunchKernelGGL\(\s*\(?\s*(\w+)\s*(<[^<>()]*>)?', src)]
    return found


def test_every_launched_kernel_is_named_by_a_case():
    found = launched()
    assert len(found) >= 20, found                                        # the extraction itself still works
    found = set(found)
    assert {'maxpool_bwd_kernel<0>', 'maxpool_bwd_kernel<1>', 'maxpool_bwd_vec_kernel<2>', 'gcn_mid_bwd_kernel', 'bn_fwd_finalize_multi_kernel'} <= found
    missing = sorted(k for k in found if k not in L.PINNED and k not in L.ELSEWHERE)
    assert not missing, f'kernels without a ledger case or an ELSEWHERE entry: {missing}'
    stale = sorted(k for k in list(L.PINNED) + list(L.ELSEWHERE) if k not in found)
    assert not stale, f'ledger entries for kernels the sources no longer launch: {stale}'
    assert not set(L.ELSEWHERE) & L.PINNED and all(L.ELSEWHERE.values())
    # the symbols the host reports are the launched ones: every tamgcn_note_kernel string of the two sources is a prefix form of one
    for name in ('elementwise.hip', 'bn.hip'):
        for note in re.findall(r'tamgcn_note_kernel\("([^"]+)"', open(os.path.join(CSRC, name)).read()):
            pat = re.escape(note).replace('%d', r'\d+')
            assert any(re.fullmatch(pat, k) for k in found), note


def test_lane_rule_and_what_the_table_promises():
    # row_geo: tpr = 16; while (tpr < 64 && tpr * 5 < steps) tpr <<= 1; steps >= 448 -> 256
    src = open(os.path.join(CSRC, 'elementwise.hip')).read()
    assert 'while (tpr < 64 && tpr * 5 < steps) tpr <<= 1;' in src and 'if (wide && steps >= 448) tpr = 256;' in src
    assert 'const int steps = vec_capable ? (L + 3) >> 2 : L;' in src

    def geo(steps):
        tpr = 16
        while tpr < 64 and tpr * 5 < steps:
            tpr <<= 1
        return 256 if steps >= 448 else tpr
    for steps in range(1, 600):
        assert R.lanes(steps, False) == geo(steps) and R.lanes(4 * steps, True) == geo(steps) and R.lanes(4 * steps - 3, True) == geo(steps)
    assert [R.lanes(s, False) for s in (80, 81, 160, 161, 447, 448)] == [16, 32, 32, 64, 64, 256]
    by = {}
    for c in L.CASES.values():
        by.setdefault(c['kind'] + ('_xbar' if c.get('xbar') else ''), []).append(c)
    for k in ('gcn_tail_fwd', 'gcn_tail_bwd', 'gcn_mid_bwd', 'add_act_fwd', 'add_act_bwd', 'maxpool_fwd', 'maxpool_post_fwd', 'maxpool_bwd', 'apply'):
        assert {c['lanes'] for c in by[k]} == {16, 32, 64, 256}, k
    for k in ('gcn_tail_fwd', 'gcn_tail_bwd', 'gcn_mid_bwd', 'add_act_fwd', 'add_act_bwd'):
        Ls = {c['T'] * c['V'] for c in by[k]}
        assert {3, 1788, 1789, 1875, 1040} <= Ls and {l % 4 for l in Ls} == {0, 1, 2, 3}
        assert any(c['N'] * c['C'] % (256 // c['lanes']) and c['N'] * c['C'] > 256 // c['lanes'] for c in by[k])     # a partly idle second workgroup
    for sym in ('maxpool_bwd_kernel<1>', 'maxpool_bwd_vec_kernel<1>', 'maxpool_bwd_vec_kernel<2>', 'maxpool_bwd_flat_kernel'):
        assert {c['lanes'] for c in by['maxpool_bwd'] if c['sym'] == sym} == {16, 32, 64, 256}, sym
    assert {c['lanes'] for c in by['maxpool_bwd'] if c['sym'] == 'maxpool_bwd_kernel<0>'} == {256}      # 64 KB of LDS: one long row per workgroup
    assert all(c['N'] * c['C'] * c['T'] * c['V'] <= (41000 if c.get('xbar') else 22000) for c in L.CASES.values())      # xbar: the five older shapes
    assert {c['T'] for c in by['tmean']} == {1, 7, 8, 9, 17} and {c['V'] for c in by['tmean']} == {25, 64, 100}
    assert {c['V'] for c in by['add_act_fwd_xbar']} >= {4, 12, 20, 24, 40, 64}
    assert {(C_, n) for C_, n, f in L.BN_FWD if f == 'full'} == {(C_, n) for C_ in (1, 3, 64, 256) for n in (1, 63, 64, 65, 200)}
    assert len(L.BN_MULTI) == len(L.BN_MULTI_BWD) == 11 and {s[0] for s in L.BN_MULTI} == {1, 3, 64, 256}


# ---------------------------------------------------------------------------------------------------------------------
# the references are autograd's formulas
# ---------------------------------------------------------------------------------------------------------------------
def _r(g, *s, lo=-1.0, hi=1.0):
    return torch.rand(s, generator=g, dtype=F64) * (hi - lo) + lo


def _same(name, a, b):
    a = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    assert float((a - b.detach()).abs().max()) <= 1e-12 * max(1.0, float(b.detach().abs().max())), name


def _part(x):
    """[2][C][N] moment slabs of a (N, C, T, V) tensor, as the producing kernels leave them"""
    return torch.stack((x.sum((2, 3)).t(), (x * x).sum((2, 3)).t()))


def _fwd(x, gamma, beta, **kw):
    """coef (3, C) and save (2, C) of train-mode BatchNorm from ew_ref.bn_fwd"""
    d = dict(C=x.shape[1], part=_part(x), count=x.numel() // x.shape[1], training=1, gamma=gamma, beta=beta, momentum=0.1, eps=1e-5, **kw)
    r = {k: torch.from_numpy(v[0]) for k, v in R.bn_fwd(d).items()}
    return torch.stack((r['c1'], r['c2'], r['c0'])), torch.stack((r['mean'], r['invstd'])), r


def _bwd(s0, s1, gamma, save, count, training=1):
    d = dict(C=s0.shape[0], part=torch.stack((s0, s1)), count=count, training=training, gamma=gamma, save=save)
    r = {k: torch.from_numpy(v[0]) for k, v in R.bn_bwd(d).items()}
    return torch.stack((r['c1'], r['c2'], r['c0'])), r


def _apply(coef, a, b=None):
    c = coef[:, None, :, None, None]
    return c[0] * a + c[2] + (c[1] * b if b is not None else 0)


def test_gcn_tail_and_mid_equal_autograd_of_the_fp64_unit():
    """g = relu(bn(y) + tanh(bn(o)) + bn(r)) with o = 0.7 (bn(r) - bn(y)) + const standing in for the offset conv of
    diff = down(x) - bn(y): the gradient reaches y through dsum and through ddiff, as in unit_gcn (models/ctrgcn.py:256-261)"""
    g_ = torch.Generator().manual_seed(11)
    N, C_, T, V = 3, 4, 5, 7
    y_pre, r_pre, noise, cot = (_r(g_, N, C_, T, V) for _ in range(4))
    gam = [(1 + 0.3 * _r(g_, C_)).requires_grad_(True) for _ in range(3)]
    bet = [_r(g_, C_).requires_grad_(True) for _ in range(3)]
    y_pre.requires_grad_(True), r_pre.requires_grad_(True)
    bn = lambda x, i: F.batch_norm(x, None, None, gam[i], bet[i], True, 0.0, EPS)          # noqa: E731
    yb, rb = bn(y_pre, 0), bn(r_pre, 1)
    o_pre = 0.7 * (rb - yb) + 0.2 * noise
    o_pre.retain_grad()
    out = torch.relu(yb + torch.tanh(bn(o_pre, 2)) + rb)
    (out * cot).sum().backward()
    cnt = N * T * V
    det = lambda t: t.detach()                                                           # noqa: E731
    cy, sy, _ = _fwd(det(y_pre), det(gam[0]), det(bet[0]))
    cr, sr, _ = _fwd(det(r_pre), det(gam[1]), det(bet[1]))
    co, so, _ = _fwd(det(o_pre), det(gam[2]), det(bet[2]))
    _same('bn(y) from the finalised coefficients', _apply(cy, det(y_pre)), yb)
    srcs = dict(y=dict(x1=det(y_pre), coef=cy), o=dict(x1=det(o_pre), coef=co), res=dict(x1=det(r_pre), coef=cr))
    g = R.gcn_tail_fwd(dict(C=C_, **srcs), F64)['g'].val
    _same('g', g, out)
    tb = R.gcn_tail_bwd(dict(C=C_, dg=cot, g=g, o=srcs['o'], o_save=so), F64)
    cob, ro = _bwd(tb['s0'].val, tb['s1'].val, det(gam[2]), so, cnt)
    _same('dgamma of bn(o)', ro['dgamma'], gam[2].grad), _same('dbeta of bn(o)', ro['dbeta'], bet[2].grad)
    do_pre = _apply(cob, tb['doz'].val, det(o_pre))
    _same('d o_pre', do_pre, o_pre.grad)
    mb = R.gcn_mid_bwd(dict(dsum=tb['dsum'].val, ddiff=0.7 * do_pre, y_pre=det(y_pre), y_save=sy, r_pre=det(r_pre), r_save=sr, want_dres=1), F64)
    cyb, ry = _bwd(mb['s0'].val, mb['s1'].val, det(gam[0]), sy, cnt)
    crb, rr = _bwd(mb['s2'].val, mb['s3'].val, det(gam[1]), sr, cnt)
    _same('d y_pre', _apply(cyb, mb['dyb'].val, det(y_pre)), y_pre.grad)
    _same('d r_pre', _apply(crb, mb['dres'].val, det(r_pre)), r_pre.grad)
    for nm, r, i in (('y', ry, 0), ('r', rr, 1)):
        _same(f'dgamma of bn({nm})', r['dgamma'], gam[i].grad), _same(f'dbeta of bn({nm})', r['dbeta'], bet[i].grad)
        assert float(r['dbias_conv'].abs().max()) <= 1e-12                               # a bias in front of a train-mode BatchNorm has no gradient


def test_add_act_equals_autograd_of_relu_bn_a_plus_bn_r():
    g_ = torch.Generator().manual_seed(12)
    N, C_, T, V = 2, 3, 4, 5
    a, r, cot = (_r(g_, N, C_, T, V) for _ in range(3))
    gam = [(1 + 0.3 * _r(g_, C_)).requires_grad_(True) for _ in range(2)]
    bet = [_r(g_, C_).requires_grad_(True) for _ in range(2)]
    a.requires_grad_(True), r.requires_grad_(True)
    out = torch.relu(F.batch_norm(a, None, None, gam[0], bet[0], True, 0.0, EPS) + F.batch_norm(r, None, None, gam[1], bet[1], True, 0.0, EPS))
    (out * cot).sum().backward()
    det = lambda t: t.detach()                                                           # noqa: E731
    ca, sa, _ = _fwd(det(a), det(gam[0]), det(bet[0]))
    cr, sr, _ = _fwd(det(r), det(gam[1]), det(bet[1]))
    f = R.add_act_fwd(dict(C=C_, a=dict(x1=det(a), coef=ca), res=dict(x1=det(r), coef=cr), relu=1, rowmean=1, xbar=True), F64)
    _same('out', f['out'].val, out), _same('rowmean', f['rowmean'].val, out.mean((2, 3))), _same('xbar', f['xbar'].val, out.mean(2).permute(1, 0, 2))
    b = R.add_act_bwd(dict(dout=cot, out=f['out'].val, relu=1, a_pre=det(a), a_save=sa, r_pre=det(r), r_save=sr, want_dz=1), F64)
    for x, s0, s1, i, save in ((a, 's0', 's1', 0, sa), (r, 's2', 's3', 1, sr)):
        cb, rb = _bwd(b[s0].val, b[s1].val, det(gam[i]), save, N * T * V)
        _same('dx', _apply(cb, b['dz'].val, det(x)), x.grad), _same('dgamma', rb['dgamma'], gam[i].grad), _same('dbeta', rb['dbeta'], bet[i].grad)


@pytest.mark.parametrize('stride,T', [(1, 7), (2, 7), (2, 6), (1, 1), (2, 2)])
def test_pools_equal_max_pool2d_and_its_autograd(stride, T):
    g_ = torch.Generator().manual_seed(13 + T)
    N, C_, V = 2, 3, 8
    src = dict(x1=_r(g_, N, C_, T, V), coef=_r(g_, 3, C_), act=1)
    L._plant_ties(src)
    hb = _apply(src['coef'], src['x1']).requires_grad_(True)
    mp = F.max_pool2d(torch.relu(hb), (3, 1), (stride, 1), (1, 0))
    To = mp.shape[2]
    assert To == R.pool_T_out(T, stride)
    gy = dict(x1=_r(g_, N, C_, To, V), x2=_r(g_, N, C_, To, V), coef=_r(g_, 3, C_))
    gv = _apply(gy['coef'], gy['x1'], gy['x2'])
    (mp * gv).sum().backward()
    f = R.maxpool_fwd(dict(C=C_, src=src, stride=stride, stats=1), F64)
    _same('max-pool', f['y'].val, mp), _same('sum', f['s0'].val, mp.sum((2, 3)).t()), _same('sum of squares', f['s1'].val, (mp * mp).sum((2, 3)).t())
    coef, add = _r(g_, 3, C_), _r(g_, N, C_, To, V)
    post = R.maxpool_post_fwd(dict(C=C_, src=src, stride=stride, ycoff=0, coef=coef, add=add, relu=1), F64)['y'].val
    _same('pooled branch in eval mode', post, torch.relu(_apply(coef, mp) + add))
    save = _r(g_, 2, C_)
    b = R.maxpool_bwd(dict(C=C_, src=src, gy=gy, stride=stride, src_save=save), F64)
    assert bool(b['d'].keep.all())
    _same('max-pool gradient (first maximum)', b['d'].val, hb.grad)
    _same('centred moment', b['s1'].val, (hb.grad * (src['x1'] - save[0][None, :, None, None])).sum((2, 3)).t())
    if T > 1:                                                               # the planted ties are there and decide something
        assert not torch.equal(R.maxpool_bwd(dict(C=C_, src=src, gy=gy, stride=stride, src_save=save), F64, last_max=True)['d'].val, b['d'].val)


@pytest.mark.parametrize('training', [True, False])
def test_finaliser_references_equal_batch_norm(training):
    g_ = torch.Generator().manual_seed(14)
    N, C_, T, V = 3, 5, 4, 6
    x = (_r(g_, N, C_, T, V) * 2 + 0.5).requires_grad_(True)
    gam, bet = (1 + 0.3 * _r(g_, C_)).requires_grad_(True), _r(g_, C_).requires_grad_(True)
    rm, rv = _r(g_, C_), _r(g_, C_, lo=0.5, hi=1.5)
    rm0, rv0 = rm.clone(), rv.clone()
    mom = float(np.float32(0.1))
    y = F.batch_norm(x, rm, rv, gam, bet, training, mom, EPS)
    cot = _r(g_, N, C_, T, V)
    (y * cot).sum().backward()
    d = dict(C=C_, part=_part(x.detach()), count=N * T * V, training=int(training), gamma=gam.detach(), beta=bet.detach(), momentum=0.1, eps=1e-5,
             running_mean=rm0, running_var=rv0)
    r = {k: torch.from_numpy(v[0]) for k, v in R.bn_fwd(d).items()}
    coef, save = torch.stack((r['c1'], r['c2'], r['c0'])), torch.stack((r['mean'], r['invstd']))
    _same('y', _apply(coef, x.detach()), y)
    if training:
        _same('running_mean', r['running_mean'], rm), _same('running_var', r['running_var'], rv)
    else:
        assert 'running_mean' not in r and torch.equal(rm, rm0)
    b = R.add_act_bwd(dict(dout=cot, relu=0, a_pre=x.detach(), a_save=save, want_dz=1), F64)
    cb, rb = _bwd(b['s0'].val, b['s1'].val, gam.detach(), save, N * T * V, int(training))
    _same('dx', _apply(cb, cot, x.detach()), x.grad), _same('dgamma', rb['dgamma'], gam.grad), _same('dbeta', rb['dbeta'], bet.grad)
    if not training:
        assert float(cb[1].abs().max()) == 0 and float(cb[2].abs().max()) == 0
        _same('bias gradient of the conv in front (eval)', rb['dbias_conv'], x.grad.sum((0, 2, 3)))


# ---------------------------------------------------------------------------------------------------------------------
# the bars admit correct fp32: an fp32 torch evaluation of every GPU case
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _case(cid):
    if cid not in _CACHE:
        p = L.problem(cid)
        _CACHE[cid] = (p, L.evaluate(cid, p, F32))
    return _CACHE[cid]


def _cpu_delta(cid):
    """the allowance per tanh for torch's CPU tanh in fp32 (the library routine of THIS evaluation): twice its largest error here"""
    kind = L.CASES[cid]['kind']
    worst = 0.0
    for p in _case(cid)[0].values():
        x = R.tanh_args(kind, p)
        if x is not None:
            worst = max(worst, float((torch.tanh(x).double() - torch.tanh(x.double())).abs().max()))
    assert worst <= R.TANHF_FINDING
    return 2 * worst


@pytest.mark.parametrize('cid', list(L.CASES))
def test_bars_admit_fp32_torch(cid):
    p, got = _case(cid)
    rat = L.verify(cid, p, got, _cpu_delta(cid))                            # raises above the 0.1 % exclusion cap, too
    assert rat and max(rat.values()) <= 1.0
    if L.CASES[cid]['kind'] == 'maxpool_bwd':                               # the planted ties stay in, and a win among them exists
        for v in p.values():
            b = R.maxpool_bwd(v, F64)
            assert int((~b['d'].keep).sum()) <= R.EXCLUDE_CAP * b['d'].keep.numel()


def _bn_other_order(p, fwd):
    """the finaliser's formulas in torch float64 with the partial sums added in reverse order, rounded to fp32 like the kernel's stores"""
    q = dict(p)
    q['part'] = None if p['part'] is None else p['part'].flip(2)
    ref = R.bn_fwd(q) if fwd else R.bn_bwd(q)
    return {n: torch.from_numpy(v[0]).float() for n, v in ref.items()}


@pytest.mark.parametrize('spec', L.BN_FWD + L.BN_MULTI, ids=str)
def test_bn_fwd_bars_admit_another_summation_order(spec):
    p = L.bn_fwd_problem(*spec, 7)
    rat = R.bn_check(str(spec), _bn_other_order(p, True), R.bn_fwd(p))
    assert rat and max(rat.values()) <= 1.0
    if p['training'] and spec[2] != 'count1':                               # the clamp is reached: var is exactly 0 there
        assert R.bn_fwd(p)['invstd'][0][0] == 1.0 / np.sqrt(float(np.float32(1e-5)))


@pytest.mark.parametrize('spec', L.BN_BWD + L.BN_MULTI_BWD, ids=str)
def test_bn_bwd_bars_admit_another_summation_order(spec):
    p = L.bn_bwd_problem(*spec, 7)
    rat = R.bn_check(str(spec), _bn_other_order(p, False), R.bn_bwd(p))
    assert rat and max(rat.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# teeth: each bar rejects each planted fault on the same inputs
# ---------------------------------------------------------------------------------------------------------------------
IDLE = '3x7x3x25_lanes16'                # 21 rows of L = 75 (L % 4 = 3) over two workgroups of 16 rows


def _rejects(cid, variant, **over):
    """the fp32 evaluation of one launch passes; with the outputs in `over` replaced it does not"""
    kind = L.CASES[cid]['kind']
    p, got = _case(cid)
    p, got = p[variant], got[variant]
    delta = _cpu_delta(cid)
    R.verify(cid, kind, p, got, delta)
    for n, v in over.items():
        assert not torch.equal(v, got[n]), n
        with pytest.raises(B.BarError):
            R.verify(cid, kind, p, dict(got, **{n: v}), delta)


def _moments(kind):
    return {'gcn_tail_bwd': ('s0', 's1'), 'gcn_mid_bwd': ('s0', 's1', 's2', 's3'), 'add_act_bwd': ('s0', 's1', 's2', 's3')}[kind]


FULL = {'gcn_tail_fwd': 'two.res', 'gcn_tail_bwd': 'two', 'gcn_mid_bwd': 'r1.dres1', 'add_act_fwd': 'two.relu0.res1.mean1', 'add_act_bwd': 'relu1.a1.r1.dz1'}
ELEMENTWISE = {'gcn_tail_fwd': ('g',), 'gcn_tail_bwd': ('dsum', 'doz'), 'gcn_mid_bwd': ('dyb', 'dres'), 'add_act_fwd': ('out',), 'add_act_bwd': ('dz',)}


@pytest.mark.parametrize('kind', list(FULL))
def test_rejects_a_row_without_its_scalar_tail(kind):
    """the last L % 4 elements of one row left unwritten (they hold what the buffer held: zero), in every output; and a row's
    moments and mean without the tail's terms"""
    cid = f'{kind}_{IDLE}'
    p, got = _case(cid)
    p, got = p[FULL[kind]], got[FULL[kind]]
    for n in ELEMENTWISE[kind]:
        v = got[n].clone()
        row = int(v[:, :, -1, -3:].abs().amin(-1).flatten().argmax())          # the row whose tail is farthest from zero
        v.view(-1, 75)[row, -3:] = 0
        _rejects(cid, FULL[kind], **{n: v})
    if kind in ('gcn_tail_bwd', 'gcn_mid_bwd', 'add_act_bwd'):
        short = R.evaluate(kind, {k: (_cut(v) if k in ('dg', 'dsum', 'ddiff', 'dout') else v) for k, v in p.items()}, F32)
        for n in _moments(kind):
            v = got[n].clone()
            v[2, 1] = short[n][2, 1]
            _rejects(cid, FULL[kind], **{n: v})
    if kind == 'add_act_fwd':
        v = got['rowmean'].clone()
        v[1, 2] = _cut(got['out'])[1, 2].sum() / 75
        _rejects(cid, FULL[kind], rowmean=v)


def _cut(x):
    """the last three elements of every row zeroed: with the gradient cut like this their terms drop out of every sum"""
    x = x.clone()
    x[:, :, -1, -3:] = 0
    return x


@pytest.mark.parametrize('kind', ['gcn_tail_bwd', 'gcn_mid_bwd', 'add_act_bwd'])
def test_rejects_a_moment_in_the_neighbouring_n_slot_and_row_0_overwritten_by_an_idle_lane(kind):
    cid = f'{kind}_{IDLE}'
    got = _case(cid)[1][FULL[kind]]
    for n in _moments(kind):
        v = got[n].clone()
        v[3, 1], v[3, 2] = got[n][3, 2], got[n][3, 1]                       # part[s][c][n] <-> part[s][c][n + 1]
        _rejects(cid, FULL[kind], **{n: v})
        v = got[n].clone()
        v[0, 0] = 0.0                                                       # an idle lane shadows row 0 with L = 0: its sums are 0
        _rejects(cid, FULL[kind], **{n: v})


def test_rejects_an_idle_lanes_row_mean_in_row_0():
    cid = f'add_act_fwd_{IDLE}'
    v = _case(cid)[1][FULL['add_act_fwd']]['rowmean'].clone()
    v[0, 0] = 0.0
    _rejects(cid, FULL['add_act_fwd'], rowmean=v)


@pytest.mark.parametrize('kind', ['gcn_tail_bwd', 'gcn_mid_bwd', 'add_act_bwd'])
@pytest.mark.parametrize('shape', [IDLE, '2x2x75x25_lanes256'])
def test_rejects_a_second_moment_centred_by_zero(kind, shape):
    cid = f'{kind}_{shape}'
    p, got = _case(cid)
    p, got = p[FULL[kind]], got[FULL[kind]]
    zero = {k: torch.zeros_like(v) for k, v in p.items() if k.endswith('_save')}
    wrong = R.evaluate(kind, dict(p, **zero), F32)
    for n in _moments(kind)[1::2]:
        _rejects(cid, FULL[kind], **{n: wrong[n]})


def test_rejects_dres_written_as_the_difference():
    for shape in (IDLE, '1x3x1x3_lanes16'):
        cid = f'gcn_mid_bwd_{shape}'
        got = _case(cid)[1]['r1.dres1']
        _rejects(cid, 'r1.dres1', dres=got['dyb'].clone())


def test_rejects_a_tie_resolved_to_the_last_maximum():
    for cid, c in L.CASES.items():
        if c['kind'] == 'maxpool_bwd' and c['T'] > 1:
            for v, p in _case(cid)[0].items():
                wrong = R.maxpool_bwd(p, F32, last_max=True)
                _rejects(cid, v, d=wrong['d'].val)


def test_rejects_a_descriptor_finalised_with_another_descriptors_count():
    for fwd, ps in ((True, L.multi_problems(True)), (False, L.multi_problems(False))):
        for i in (0, 3, 9):
            p = ps[i]
            if not p['training']:
                continue
            ref = R.bn_fwd(p) if fwd else R.bn_bwd(p)
            wrong = dict(p, count=ps[(i + 1) % len(ps)]['count'])
            assert wrong['count'] != p['count']
            bad = (R.bn_fwd if fwd else R.bn_bwd)(wrong)
            R.bn_check('own count', {n: torch.from_numpy(v[0]).float() for n, v in ref.items()}, ref)
            with pytest.raises(B.BarError):
                R.bn_check('another count', {n: torch.from_numpy(v[0]).float() for n, v in bad.items()}, ref)


def test_rejects_one_ulp_where_bit_equality_is_asked_and_nan_anywhere():
    cid = f'gcn_mid_bwd_{IDLE}'
    got = _case(cid)[1]['r1.dres1']
    v = got['dyb'].clone()
    v[1, 2, 1, 3] = torch.nextafter(v[1, 2, 1, 3], torch.tensor(9.0))
    _rejects(cid, 'r1.dres1', dyb=v)
    v = got['s1'].clone()
    v[4, 1] = float('nan')
    _rejects(cid, 'r1.dres1', s1=v)


def test_rejects_a_pool_gradient_that_ignores_the_activation_of_gy():
    """what the vector and flat kernels would deliver for a gy with act = 1 (coefficients applied, the ReLU not): the cases that
    send such a gy through tamgcn_maxpool_bwd reject it, in the gradient and in both moments"""
    cids = [cid for cid, c in L.CASES.items() if c.get('gyact')]
    assert len(cids) == 3 and all(L.CASES[cid]['sym'] == 'maxpool_bwd_kernel<1>' for cid in cids)
    staged = [cid for cid, c in L.CASES.items() if c['kind'] == 'maxpool_bwd' and c['sym'].startswith('maxpool_bwd_kernel')]
    assert all(any(p['gy'].get('act') == 1 for p in _case(cid)[0].values()) for cid in staged)      # every staged case has a two-source gy with act = 1
    for cid in cids:
        for v, p in _case(cid)[0].items():
            assert p['gy']['act'] == 1
            wrong = R.evaluate('maxpool_bwd', dict(p, gy=dict(p['gy'], act=0)), F32)
            _rejects(cid, v, **wrong)


def test_rejects_one_dropped_term_in_the_moments_of_the_longest_row():
    """the no-LDS case sums 11000 elements per slot: its bars still notice ONE element left out of a row's sums"""
    cid = 'maxpool_bwd_1x2x440x25_stride2_lanes256'
    p, got = _case(cid)
    v = 'gy-coef.src-plain'
    b = R.maxpool_bwd(p[v], F64)
    d = b['d'].val[0, 1].flatten()
    i = int(torch.nonzero(d.abs() > 0.25 * d.abs().max())[0])                     # an element of ordinary size
    c0 = p[v]['src']['coff']
    x = p[v]['src']['x1'][0, c0 + 1].flatten()[i].double() - p[v]['src_save'][0, c0 + 1].double()
    s0, s1 = got[v]['s0'].clone(), got[v]['s1'].clone()
    s0[1, 0] -= d[i].float()
    s1[1, 0] -= (d[i] * x).float()
    _rejects(cid, v, s0=s0)
    if abs(float(d[i] * x)) > 1e-3:
        _rejects(cid, v, s1=s1)
