"""CPU: the ledger of the stem, head, loss and score-fusion kernels (tests/test_gpu_stemhead_forms.py) stays complete, its fp64
references (tests/stemhead_ref.py) are autograd's formulas on the composites they replace, the frame index stem_apply_kernel takes
from a float reciprocal is the integer quotient for every legal row, an fp32 torch evaluation of every GPU case stays inside
every bar (and the reference alone leaves out at most 1 % of a softmax case's decisions), the bars reject what a subtly wrong
kernel would deliver, and the entry points refuse what they cannot run."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ew_ref as E
import fp64_bars as B
import stemhead_ref as R
import test_gpu_stemhead_forms as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tam_gcn_amd', 'csrc')
F64, F32 = torch.float64, torch.float32
EPS = float(np.float32(1e-5))
KERNELS = ['stem_stats_kernel', 'stem_apply_kernel', 'stem_streams_eval_kernel', 'pool_fwd_kernel', 'pool_bwd_kernel', 'fc_fwd_kernel',
           'fc_grouped_kernel', 'fc_bwd_kernel', 'ce_fwd_kernel', 'ce_bwd_kernel', 'score_fuse_kernel']


# ---------------------------------------------------------------------------------------------------------------------
# ledger completeness
# ---------------------------------------------------------------------------------------------------------------------
def launched():
    """every kernel (with its literal template arguments) behind a hipLaunchKernelGGL( of stemhead.hip"""
    src = open(os.path.join(CSRC, 'stemhead.hip')).read()
    return [k + (a or '') for k, a in re.findall(r'hipLaunchKernelGGL\(\s*\(?\s*(\w+)\s*(<[^<>()]*>)?', src)]


def test_every_launched_kernel_is_named_by_a_case():
    found = launched()
    assert len(found) >= 11, found                                        # the extraction itself still works
    found = set(found)
    assert set(KERNELS) <= found
    missing = sorted(k for k in found if k not in L.PINNED)
    assert not missing, f'kernels of stemhead.hip without a ledger case: {missing}'
    stale = sorted(k for k in list(L.PINNED) + list(L.ELSEWHERE) if k not in found)
    assert not stale, f'ledger entries for kernels the source no longer launches: {stale}'
    # ELSEWHERE: only the two grouped kernels, only in addition to their own cases, and the tests it names exist
    assert set(L.ELSEWHERE) <= {'stem_streams_eval_kernel', 'fc_grouped_kernel'} and set(L.ELSEWHERE) <= L.PINNED
    for where in L.ELSEWHERE.values():
        path, test = where.split('::')
        assert path == 'tests/test_gpu_stream_ensemble.py' and f'def {test}(' in open(os.path.join(ROOT, path)).read(), where
    src = open(os.path.join(CSRC, 'stemhead.hip')).read()
    notes = re.findall(r'tamgcn_note_kernel\("([^"]+)"', src)
    assert len(notes) >= 11
    for note in notes:
        assert note in found, note


def test_what_the_table_promises():
    by = {}
    for c in L.CASES.values():
        by.setdefault(c['kind'], []).append(c['shape'])
    J = lambda s: s[1] * s[3] * s[4]                                        # noqa: E731
    st = by['stem_stats']
    assert any(J(s) > 256 for s in st) and any(s[2] < 8 for s in st) and any(s[2] % 8 == 0 for s in st) and any(s[2] > 8 and s[2] % 8 for s in st)
    assert {s[4] for s in st} == {1, 2, 3} and set(st) <= set(by['stem_apply'])
    assert {s[2] * s[3] * s[4] for s in by['stem_apply']} >= {2 ** 20 - 1, 2 ** 20 - 26}                # the longest rows of whole 25-joint frames, M = 1 and 2
    assert all(s[2] * s[3] * s[4] < 2 ** 20 for s in by['stem_apply'])
    assert {s[2] * s[3] for s in by['pool_fwd']} == {1, 63, 64, 65, 300} and any(s[0] * s[1] % 4 for s in by['pool_fwd'])
    assert {s[4] for s in by['pool_bwd']} == {1, 2, 3}
    assert any(s[1] > 64 for s in by['fc_fwd']) and any(s[2] < 4 for s in by['fc_fwd']) and by['fc_fwd'] == by['fc_grouped']
    assert {s[0] for s in by['fc_bwd']} == {1, 15, 16, 17, 33} and any(s[1] > 256 for s in by['fc_bwd'])
    assert {s[0] for s in by['ce_fwd']} >= {1, 255, 256, 257} and (1, 1) in by['ce_fwd']
    assert sorted(s[0] * s[1] for s in by['ce_bwd']) == [1, 255, 256, 257, 2560]
    fu = by['score_fuse']
    assert {s[0] for s in fu} == {1, 2, 4} and {s[1] for s in fu} == {1, 255, 256, 257, 600} and {s[2] for s in fu} == {1, 10, 60}
    assert any(s[1] == 257 and s[2] == 60 for s in fu)


# ---------------------------------------------------------------------------------------------------------------------
# the references are autograd's formulas
# ---------------------------------------------------------------------------------------------------------------------
def _r(g, *s, lo=-1.0, hi=1.0):
    return torch.rand(s, generator=g, dtype=F64) * (hi - lo) + lo


def _same(name, a, b):
    a = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    assert tuple(a.shape) == tuple(b.shape), name
    assert float((a - b.detach()).abs().max()) <= 1e-12 * max(1.0, float(b.detach().abs().max())), name


@pytest.mark.parametrize('training', [True, False])
def test_stem_references_equal_batchnorm1d_between_the_two_permutes(training):
    g_ = torch.Generator().manual_seed(21)
    N, C_, T, V, M = 3, 2, 5, 4, 3
    J = C_ * V * M
    x = (_r(g_, N, C_, T, V, M) * 2 + 0.5).requires_grad_(True)
    gam, bet = (1 + 0.3 * _r(g_, J)).requires_grad_(True), _r(g_, J).requires_grad_(True)
    rm, rv = _r(g_, J), _r(g_, J, lo=0.5, hi=1.5)
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.batch_norm(x.permute(0, 4, 3, 1, 2).contiguous().view(N, J, T), rm, rv, gam, bet, training, float(np.float32(0.1)), EPS)
    y = y.view(N, M, V, C_, T).permute(0, 1, 3, 4, 2).contiguous().view(N * M, C_, T, V)
    cot = _r(g_, N * M, C_, T, V)
    (y * cot).sum().backward()
    xd = x.detach()
    part = None
    if training:
        st = R.stem_stats(dict(x=xd))
        part = torch.stack((st['s0'].val, st['s1'].val))
        _same('sum', st['s0'].val, xd.permute(4, 3, 1, 0, 2).reshape(J, N, T).sum(2))
    d = dict(C=J, part=part, count=N * T, training=int(training), gamma=gam.detach(), beta=bet.detach(), momentum=0.1, eps=1e-5,
             running_mean=rm0, running_var=rv0)
    r = {k: torch.from_numpy(v[0]) for k, v in E.bn_fwd(d).items()}
    coef, save = torch.stack((r['c1'], r['c2'], r['c0'])), torch.stack((r['mean'], r['invstd']))
    _same('stem forward', R.stem_apply(dict(x=xd, coef=coef))['out'].val, y)
    if training:
        _same('running_mean', r['running_mean'], rm), _same('running_var', r['running_var'], rv)
    sb = R.stem_stats(dict(x=xd, dout=cot, center=save[0]))
    db = dict(C=J, part=torch.stack((sb['s0'].val, sb['s1'].val)), count=N * T, training=int(training), gamma=gam.detach(), save=save)
    rb = {k: torch.from_numpy(v[0]) for k, v in E.bn_bwd(db).items()}
    coefb = torch.stack((rb['c1'], rb['c2'], rb['c0']))
    _same('stem dx', R.stem_apply(dict(x=xd, coef=coefb, dout=cot))['dx'].val, x.grad)
    _same('dgamma', rb['dgamma'], gam.grad), _same('dbeta', rb['dbeta'], bet.grad)


def test_head_references_equal_linear_of_the_two_means():
    g_ = torch.Generator().manual_seed(22)
    N, M, C_, T, V, K = 3, 2, 5, 4, 3, 7
    x = _r(g_, N * M, C_, T, V).requires_grad_(True)
    W, b = _r(g_, K, C_).requires_grad_(True), _r(g_, K).requires_grad_(True)
    lo = F.linear(x.view(N, M, C_, -1).mean(3).mean(1), W, b)
    cot = _r(g_, N, K)
    (lo * cot).sum().backward()
    pooled = R.pool_fwd(dict(x=x.detach(), M=M))['pooled'].val
    _same('logits', R.fc_fwd(dict(pooled=pooled, W=W.detach(), b=b.detach()))['logits'].val, lo)
    bw = R.fc_bwd(dict(dl=cot, pooled=pooled, W=W.detach()))
    _same('dW', bw['dW'].val, W.grad), _same('db', bw['db'].val, b.grad)
    _same('dx', R.pool_bwd(dict(dpooled=bw['dpooled'].val, M=M, T=T, V=V))['dx'].val, x.grad)
    G = 3
    pg, Wg, bg = _r(g_, G * N, C_), _r(g_, G, K, C_), _r(g_, G, K)
    sc = R.fc_grouped(dict(pooled=pg, W=Wg, b=bg))['scores'].val
    for g in range(G):
        _same(f'group {g}', sc[g], F.linear(pg[g * N:(g + 1) * N], Wg[g], bg[g]))


def test_cross_entropy_reference_equals_torch():
    g_ = torch.Generator().manual_seed(23)
    N, K = 37, 10
    for pat in ('valid', 'ign5'):
        lg = (torch.randn(N, K, generator=g_) * 3).double().requires_grad_(True)
        y = L.ce_labels(pat, N, K, g_)
        loss = F.cross_entropy(lg, y)                                       # default arguments: mean, ignore_index = -100
        (loss * 1.7).backward()
        r = R.ce_fwd(dict(logits=lg.detach(), labels=y))
        _same('loss', r['loss'].val, loss)
        _same('gradient', R.ce_bwd(dict(g=r['g'].val, dloss=torch.tensor(1.7, dtype=F64)))['dlogits'].val, lg.grad)
    lg = torch.randn(N, K, generator=g_).double()
    none = torch.full((N,), -100)
    assert torch.isnan(F.cross_entropy(lg, none)) and R.ce_fwd(dict(logits=lg, labels=none))['loss'].how == 'nan'
    for bad in (K, -1, 10 ** 12):                                           # torch raises here; the header says NaN and a zero row
        y = L.ce_labels('ign5', N, K, g_)
        y[3] = bad
        r = R.ce_fwd(dict(logits=lg, labels=y))
        ok = R.ce_fwd(dict(logits=lg, labels=torch.where(y == bad, torch.tensor(-100), y)))
        assert r['loss'].how == 'nan' and float(r['g'].val[3].abs().max()) == 0 and torch.equal(r['g'].val, ok['g'].val)


def test_score_fusion_reference_equals_the_numpy_loop():
    r_ = np.random.RandomState(24)
    N, K, alpha = 50, 10, 0.7
    a, b = r_.standard_normal((N, K)).astype(np.float32), r_.standard_normal((N, K)).astype(np.float32)
    p = dict(scores=torch.from_numpy(np.stack((a, b))), w=torch.tensor([1.0, alpha]), softmax=0, labels=None)
    fused = np.empty_like(a)
    for n in range(N):
        fused[n] = a[n] + np.float32(alpha) * b[n]
    got = R.evaluate('score_fuse', p, F32)
    assert np.array_equal(got['fused'].numpy(), fused) and np.array_equal(got['pred'].numpy(), np.argmax(fused, axis=1))
    _same('fp64', R.score_fuse(p)['fused'].val, torch.from_numpy(a.astype(np.float64) + float(np.float32(alpha)) * b.astype(np.float64)))
    sm = lambda z: np.exp(z - z.max(1, keepdims=True)) / np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)     # noqa: E731
    _same('softmax', R.score_fuse(dict(p, softmax=1))['fused'].val, torch.from_numpy(sm(a.astype(np.float64)) + float(np.float32(alpha)) * sm(b.astype(np.float64))))
    lab = torch.from_numpy(r_.randint(0, K, N))
    st = R.class_stats(got['pred'], lab, K)
    assert int(st[:, 1].sum()) == N and int(st[:, 0].sum()) == int((got['pred'] == lab).sum())


def test_fuse_add_cannot_be_contracted():
    """__fmul_rn / __fadd_rn are plain * and + in the HIP headers: inlined, the pair became one v_fmac_f32 and every raw score_fuse
    case with S >= 2 failed its bit-equality.  The body switches contraction off for its own operations."""
    src = open(os.path.join(CSRC, 'evalbody.h')).read()
    body = src[src.index('float fuse_add('):]
    body = body[:body.index('\n}') + 2]
    assert '#pragma clang fp contract(off)' in body and 'fmaf' not in body and '__fmul_rn' not in body
    assert body.index('#pragma clang fp contract(off)') < body.index('ws * term') < body.index('f + prod')


# ---------------------------------------------------------------------------------------------------------------------
# the frame index from a float reciprocal
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_index_from_the_reciprocal_is_the_quotient_below_2_to_20():
    src = open(os.path.join(CSRC, 'stemhead.hip')).read()
    assert 'const float rV = 1.0f / (float)V;' in src and 'const int t = (int)(((float)tv + 0.5f) * rV)' in src
    assert '(long long)T * V * M < (1LL << 20)' in src
    tv = np.arange(2 ** 20, dtype=np.int64)
    for V in list(range(1, 129)) + [150, 255, 256, 300, 511, 512, 1000]:
        assert np.array_equal(R.frame_index_f32(tv, V), tv // V), V


# ---------------------------------------------------------------------------------------------------------------------
# the bars admit correct fp32: an fp32 torch evaluation of every GPU case
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _case(cid):
    if cid not in _CACHE:
        p = L.problem(cid)
        _CACHE[cid] = (p, L.evaluate(cid, p, F32))
    return _CACHE[cid]


@pytest.mark.parametrize('cid', list(L.CASES))
def test_bars_admit_fp32_torch(cid):
    p, got = _case(cid)
    rat = L.verify(cid, p, got)                                             # raises above the 1 % exclusion cap, too
    assert rat and max(rat.values()) <= 1.0
    if L.CASES[cid]['kind'] == 'score_fuse':
        for v, q in p.items():
            if q['softmax']:
                out = R.fuse_excluded(q)
                assert int(out.sum()) <= R.FUSE_CAP * out.numel(), (cid, v)


# ---------------------------------------------------------------------------------------------------------------------
# teeth: each bar rejects each planted fault on the same inputs
# ---------------------------------------------------------------------------------------------------------------------
def _rejects(cid, variant, *alts):
    """the fp32 evaluation of one launch passes; with the outputs of any one dict of `alts` replaced it does not"""
    kind = L.CASES[cid]['kind']
    p, got = _case(cid)
    p, got = p[variant], got[variant]
    R.verify(cid, kind, p, got)
    assert alts
    for over in alts:
        assert any(not torch.equal(v, got[n]) for n, v in over.items())
        with pytest.raises(B.BarError):
            R.verify(cid, kind, p, dict(got, **over))


def test_rejects_stem_statistics_in_memory_order():
    for cid in ('stem_stats_2x3x7x25x2', 'stem_stats_3x3x17x5x3'):
        N, C_, T, V, M = L.CASES[cid]['shape']
        jmap = torch.tensor([(m * V + v) * C_ + c for c in range(C_) for v in range(V) for m in range(M)])      # slot i = (c, v, m) holds feature j
        for variant in ('fwd', 'bwd'):
            got = _case(cid)[1][variant]
            _rejects(cid, variant, dict(s0=got['s0'][jmap]), dict(s1=got['s1'][jmap]))


def test_rejects_a_backward_second_moment_centred_by_zero():
    for cid in ('stem_stats_2x3x7x25x2', 'stem_stats_1x1x1x1x1', 'stem_stats_2x6x13x25x2'):
        p = _case(cid)[0]['bwd']
        wrong = R.evaluate('stem_stats', dict(p, center=torch.zeros_like(p['center'])))
        _rejects(cid, 'bwd', dict(s1=wrong['s1']))


def test_rejects_statistics_without_the_tail_frames():
    for cid in ('stem_stats_2x6x13x25x2', 'stem_stats_2x3x7x25x2', 'stem_stats_3x3x17x5x3'):
        T = L.CASES[cid]['shape'][2]
        full = T - T % 8
        for variant, p in _case(cid)[0].items():
            q = {k: (v[:, :, :full] if k in ('x', 'dout') else v) for k, v in p.items()}
            wrong = R.evaluate('stem_stats', q) if full else {k: torch.zeros_like(v) for k, v in _case(cid)[1][variant].items()}
            _rejects(cid, variant, dict(s0=wrong['s0']), dict(s1=wrong['s1']))


def test_rejects_a_frame_boundary_element_with_the_previous_frames_index():
    """tv = t V decoded as (t - 1, V): the element is stored where it belongs, with the coefficients of feature (m, V, c) = (m + 1, 0, c)"""
    for cid, t in (('stem_apply_2x3x7x25x2', 1), ('stem_apply_1x1x20971x25x2', 20970), ('stem_apply_3x3x17x5x3', 16)):
        N, C_, T, V, M = L.CASES[cid]['shape']
        n, c, m = N - 1, C_ - 1, 0
        j = (m * V + V) * C_ + c
        ps, gots = _case(cid)
        cf = ps['fwd']['coef']
        x = ps['fwd']['x'][n, c, t, 0, m]
        out = gots['fwd']['out'].clone()
        out[n * M + m, c, t, 0] = cf[0, j] * x + cf[2, j]
        _rejects(cid, 'fwd', dict(out=out))
        dx = gots['bwd']['dx'].clone()
        dx[n, c, t, 0, m] = cf[0, j] * ps['bwd']['dout'][n * M + m, c, t, 0] + cf[1, j] * x + cf[2, j]
        _rejects(cid, 'bwd', dict(dx=dx))


def test_rejects_a_pool_that_divides_by_L_or_ignores_the_second_body():
    for cid in ('pool_fwd_2x6x12x25x2', 'pool_fwd_3x5x1x1x2', 'pool_fwd_1x3x13x5x3'):
        N, C_, T, V, M = L.CASES[cid]['shape']
        p, got = _case(cid)[0]['one'], _case(cid)[1]['one']
        first = p['x'].view(N, M, C_, T * V)[:, 0].sum(-1) / (M * T * V)
        _rejects(cid, 'one', dict(pooled=got['pooled'] * M), dict(pooled=first))
    for cid in ('pool_bwd_2x6x12x25x2', 'pool_bwd_1x3x13x5x3'):
        M = L.CASES[cid]['shape'][4]
        _rejects(cid, 'one', dict(dx=_case(cid)[1]['one']['dx'] * M))


def test_rejects_fc_faults():
    p, got = _case('fc_fwd_3x100x10')
    for v in ('bias', 'nobias'):
        q = p[v]
        wrong = q['pooled'][:, :64] @ q['W'][:, :64].t() + (q['b'] if q['b'] is not None else 0)      # channels >= 64 dropped
        _rejects('fc_fwd_3x100x10', v, dict(logits=wrong))
    _rejects('fc_fwd_3x100x10', 'nobias', dict(logits=got['bias']['logits']))                          # a bias where none is given
    for cid in ('fc_grouped_3x100x10', 'fc_grouped_1x32x3'):
        q, sc = _case(cid)[0]['G3'], _case(cid)[1]['G3']['scores']
        _rejects(cid, 'G3', dict(scores=sc - q['b'][:, None] + q['b'][0][None, None]))                  # group 0's bias everywhere
    for cid, full in (('fc_bwd_17x256x10', 16), ('fc_bwd_33x300x5', 32)):
        q = _case(cid)[0]['one']
        _rejects(cid, 'one', dict(dW=q['dl'][:full].t() @ q['pooled'][:full]), dict(db=q['dl'][:full].sum(0)))


def test_rejects_cross_entropy_faults():
    cid = 'ce_fwd_255x10'
    p, got = _case(cid)
    q, g = p['scale3.ign5'], got['scale3.ign5']
    N, K = q['logits'].shape
    kept = int(R.ce_rows(q['labels'], K)[0].sum())
    assert kept < N
    _rejects(cid, 'scale3.ign5', dict(loss=g['loss'] * kept / N), dict(g=g['g'] * kept / N))            # the mean over N
    leak = g['g'].clone()
    leak[5, 2] = 1e-30                                                                                 # row 5 is ignored
    assert int(q['labels'][5]) == R.IGNORE_INDEX
    _rejects(cid, 'scale3.ign5', dict(g=leak))
    for cid2 in (cid, 'ce_fwd_1x3', 'ce_fwd_600x60'):                                                  # no max-shift: expf(100 + ..) is inf
        q, g = _case(cid2)[0]['plus100.valid'], _case(cid2)[1]['plus100.valid']
        e = torch.exp(q['logits'])
        s = e.sum(1, keepdim=True)
        onehot = torch.zeros_like(e).scatter_(1, q['labels'][:, None], 1.0)
        term = torch.log(s)[:, 0] - q['logits'].gather(1, q['labels'][:, None])[:, 0]
        _rejects(cid2, 'plus100.valid', dict(loss=term.double().mean().float()), dict(g=(e / s - onehot) / q['logits'].shape[0]))
    q, g = _case(cid)[0]['scale3.badK'], _case(cid)[1]['scale3.badK']
    _rejects(cid, 'scale3.badK', dict(loss=torch.tensor(2.5)))                                          # a number where NaN is due
    _rejects('ce_fwd_1x1', 'plus100.valid', dict(loss=torch.tensor(2.0 ** -17)), dict(g=torch.full((1, 1), 2.0 ** -24)))


def _fuse_alt(p, fused, last=False):
    pred = R.first_argmax(fused, last)
    out = dict(fused=fused, pred=pred)
    if p['labels'] is not None:
        out['stats'] = R.class_stats(pred, p['labels'], p['scores'].shape[2])
    return out


def test_rejects_score_fusion_faults():
    for cid in ('score_fuse_2x255x10', 'score_fuse_2x257x60', 'score_fuse_2x1x60'):
        p, got = _case(cid)
        q, g = p['raw'], got['raw']
        two, three = L.tie_rows(q['scores'].shape[1])
        f = g['fused']
        assert all(f[n, 2] == f[n, 7] == f[n].max() for n in two) and all(f[n, 1] == f[n, 4] == f[n, 9] == f[n].max() for n in three)
        assert all(int(g['pred'][n]) == 2 for n in two) and all(int(g['pred'][n]) == 1 for n in three)
        _rejects(cid, 'raw', _fuse_alt(q, f, last=True))                                               # the last maximum wins a tie
        _rejects(cid, 'raw', _fuse_alt(q, R.score_fuse(q, F32, fma=True)['fused'].val))                 # one rounding where two are asked
        _rejects(cid, 'raw', dict(stats=g['stats'] + L.STALE))                                         # the statistics not reset
        _rejects(cid, 'softmax', dict(stats=got['softmax']['stats'] + L.STALE))
    cid = 'score_fuse_4x600x60'
    p, got = _case(cid)
    wrong = R.score_fuse(dict(p['softmax'], w=p['softmax']['w'].flip(0)), F32)['fused'].val            # the weights of the wrong score set
    _rejects(cid, 'softmax', _fuse_alt(p['softmax'], wrong))


def test_rejects_one_ulp_where_bit_equality_is_asked_and_nan_anywhere():
    up = lambda t, i: torch.nextafter(t[i], torch.tensor(9.0))               # noqa: E731
    v = _case('ce_bwd_51x5')[1]['one']['dlogits'].clone()
    v[50, 4] = up(v, (50, 4))
    _rejects('ce_bwd_51x5', 'one', dict(dlogits=v))
    p, got = _case('score_fuse_4x256x10')
    v = got['raw']['fused'].clone()
    v[255, 3] = up(v, (255, 3))
    _rejects('score_fuse_4x256x10', 'raw', _fuse_alt(p['raw'], v))
    for cid, variant, n in (('stem_stats_2x6x13x25x2', 'bwd', 's1'), ('stem_apply_3x3x17x5x3', 'fwd', 'out'), ('stem_streams_eval_1x3x5x7x3', 'modes0123', 'out'),
                            ('pool_fwd_1x5x9x7x1', 'one', 'pooled'), ('pool_bwd_2x2x8x8x1', 'one', 'dx'), ('fc_fwd_1x320x5', 'bias', 'logits'),
                            ('fc_grouped_2x64x4', 'G3', 'scores'), ('fc_bwd_16x100x10', 'one', 'db'), ('ce_fwd_257x10', 'scale30.valid', 'g'),
                            ('ce_fwd_257x10', 'minus100.ign5', 'loss'), ('ce_bwd_256x10', 'one', 'dlogits'), ('score_fuse_1x600x10', 'softmax.nolabels', 'fused')):
        v = _case(cid)[1][variant][n].clone()
        v.view(-1)[-1] = float('nan')
        over = dict({n: v})
        if n == 'fused':
            over['pred'] = _case(cid)[1][variant]['pred']
        _rejects(cid, variant, over)


def test_rejects_a_stream_taken_for_another_and_a_motion_that_reads_past_the_clip():
    cid = 'stem_streams_eval_1x3x5x7x3'
    p, got = _case(cid)
    q = p['modes0123']
    _rejects(cid, 'modes0123', dict(out=R.evaluate('stem_streams_eval', dict(q, modes=[0, 1, 3, 2]))['out']))
    N, C_, T, V, M = L.CASES[cid]['shape']
    v = got['modes0123']['out'].clone()
    g = 2                                                                    # motion: its last frame is c1 * 0 + c0, not c1 * (0 - x) + c0
    c1 = q['coef'][g, 0].view(M, V, C_).permute(0, 2, 1)
    blk = v[g * N * M:(g + 1) * N * M].view(N, M, C_, T, V)
    blk[:, :, :, T - 1] -= c1[None] * q['x'].permute(0, 4, 1, 2, 3)[:, :, :, T - 1]
    _rejects(cid, 'modes0123', dict(out=v))


# ---------------------------------------------------------------------------------------------------------------------
# argument errors (no GPU: a call that got past its checks would fail in the launch with another code)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_cannot_run():
    from tam_gcn_amd import _lib
    lib = _lib.load()
    p = 1 << 20
    assert lib.tamgcn_stem_apply(p, None, p, 1, 1, 1 << 18, 4, 1, p, None) == -1                       # T V M = 2^20
    err = lib.tamgcn_last_error()
    assert b'tamgcn_stem_apply' in err and b'2^20' in err and b'1048576' in err, err
    assert lib.tamgcn_stem_apply(p, None, p, 1, 1, 1 << 17, 4, 2, p, None) == -1 and b'2^20' in lib.tamgcn_last_error()
    assert lib.tamgcn_stem_stats(p, p, None, 1, 3, 8, 20, 1, p, None) == -1 and b'tamgcn_stem_stats' in lib.tamgcn_last_error()
