"""-m gpu: the ledger of the stem, head, loss and score-fusion kernels (csrc/stemhead.hip): the one source every training step
and every evaluation passes through.  Every case is the smallest shape that reaches one path of one kernel -- the second pass of
a thread loop, a round count with and without its tail, M = 1 / 2 / 3, a row of 2^20 - 2 floats, a partly empty last workgroup,
a thread's second row -- the kernel symbol the host must report for it (tamgcn_last_kernel()), and the fp64 reference of THAT
entry point (tests/stemhead_ref.py) at fp32-rounding bars (tests/fp64_bars.py) or, where the project already has an absolute
bar (the loss, the softmax scores), at that one.  Every entry point is called on the library directly; inputs are seeded, have
NaN floats behind them and coefficients that differ per feature; every output is pre-filled with a sentinel and has sentinel
floats (integers) behind it that must keep their value.

tests/test_stemhead_ref_cpu.py (CPU) checks that the references are autograd's formulas, that an fp32 torch evaluation of every
case passes its bars, that planted faults do not, and that every kernel the source launches is named by a case here.

Run with -s to see the measured err / bound ratios (profiles/stemhead_bars.txt records one run)."""
import numpy as np
import pytest
import torch

import fp64_bars as B
import stemhead_ref as R

NAN = float('nan')
SENTINEL = -7.25
GUARD = 8
INT_GUARD = -77
STALE = 12345                          # what the statistics buffer holds before tamgcn_score_fuse

# (N, C, T, V, M).  stem_stats: one element; T = 7: tail only; T = 8: one round of eight frames and no tail; J = C V M = 300: a
# second pass of the thread loop (and T = 13: a round and a tail); M = 3.  stem_apply also: the longest legal rows, tv up to 2^20 - 2
STEM = [(1, 1, 1, 1, 1), (2, 3, 7, 25, 2), (1, 3, 8, 20, 1), (2, 6, 13, 25, 2), (3, 3, 17, 5, 3)]
STEM_LONG = [(1, 1, 41943, 25, 1), (1, 1, 20971, 25, 2)]
# T = 1: every motion frame is the last one; M = 3
STREAMS = [(2, 3, 1, 20, 1), (1, 3, 5, 7, 3)]
# (N, C, T, V, M) of the pooled tensor: L = T V = 1 (the head_pooled route) / 63 / 64 / 65 / 300; N C = 5: a partly empty workgroup
POOL = [(3, 5, 1, 1, 2), (1, 5, 9, 7, 1), (2, 2, 8, 8, 1), (1, 3, 13, 5, 3), (2, 6, 12, 25, 2)]
# (N, C, K): C <= 64 one pass, > 64 two and more; K < 4 leaves waves idle
FC = [(1, 32, 3), (2, 64, 4), (3, 100, 10), (2, 256, 60), (1, 320, 5)]
# (N, C, K): N around the rounds of 16 samples; C > 256: a thread's second channel
FC_BWD = [(1, 32, 1), (15, 64, 3), (16, 100, 10), (17, 256, 10), (33, 300, 5)]
CE = [(1, 1), (1, 3), (255, 10), (256, 10), (257, 10), (600, 60)]
CE_LOGITS = dict(scale3=(3.0, 0.0), scale30=(30.0, 0.0), plus100=(3.0, 100.0), minus100=(3.0, -100.0))
CE_LABELS = ('valid', 'ign5', 'allign', 'badK', 'badneg', 'badbig')
CE_BWD = [(1, 1), (51, 5), (256, 1), (257, 1), (256, 10)]           # N K = 1, 255, 256, 257, 2560
# (S, N, K): every S of 1, 2, 4, every N of 1, 255, 256, 257, 600, every K of 1, 10, 60; N = 257 with K = 60
FUSE = [(1, 1, 1), (2, 1, 60), (2, 255, 10), (4, 256, 10), (2, 257, 60), (1, 600, 10), (4, 600, 60)]

CASES = {}


def _add(kind, sym, shape, **kw):
    cid = f'{kind}_' + 'x'.join(map(str, shape))
    assert cid not in CASES, cid
    CASES[cid] = dict(kind=kind, sym=sym, shape=tuple(shape), **kw)


for _s in STEM:
    _add('stem_stats', 'stem_stats_kernel', _s)
for _s in STEM + STEM_LONG:
    _add('stem_apply', 'stem_apply_kernel', _s)
for _s in STREAMS:
    _add('stem_streams_eval', 'stem_streams_eval_kernel', _s)
for _s in POOL:
    _add('pool_fwd', 'pool_fwd_kernel', _s)
    _add('pool_bwd', 'pool_bwd_kernel', _s)
for _s in FC:
    _add('fc_fwd', 'fc_fwd_kernel', _s)
    _add('fc_grouped', 'fc_grouped_kernel', _s)
for _s in FC_BWD:
    _add('fc_bwd', 'fc_bwd_kernel', _s)
for _s in CE:
    _add('ce_fwd', 'ce_fwd_kernel', _s)
for _s in CE_BWD:
    _add('ce_bwd', 'ce_bwd_kernel', _s)
for _s in FUSE:
    _add('score_fuse', 'score_fuse_kernel', _s)

PINNED = {c['sym'] for c in CASES.values()}
# held here AND, bit-equal to the single kernels, by the ensemble's tests
ELSEWHERE = {'stem_streams_eval_kernel': 'tests/test_gpu_stream_ensemble.py::test_fused_stem_equals_stream_derive_then_stem_apply',
             'fc_grouped_kernel': 'tests/test_gpu_stream_ensemble.py::test_grouped_head_equals_the_single_head'}


# ---------------------------------------------------------------------------------------------------------------------
# problems: CPU tensors from the case's seed (shared with the CPU test, which evaluates them in fp32 torch)
# ---------------------------------------------------------------------------------------------------------------------
def seed_of(cid):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(cid))


def _coef(shape, g):
    """0.5 .. 1.5 with a random sign: no two features alike, none near 0"""
    return (torch.rand(shape, generator=g) + 0.5) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def _randn(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g) * scale + shift


def tie_rows(N):
    """(two-way, three-way) rows of the planted ties of a raw score-fusion problem"""
    return [n for n in range(N) if n % 7 == 0], [n for n in range(N) if n % 7 == 3]


def ce_labels(pattern, N, K, g):
    y = torch.randint(0, K, (N,), generator=g)
    if pattern != 'valid':
        y[::5] = R.IGNORE_INDEX
    if pattern == 'allign':
        y[:] = R.IGNORE_INDEX
    if pattern.startswith('bad'):
        y[min(3, N - 1)] = dict(badK=K, badneg=-1, badbig=10 ** 12)[pattern]
    return y


def problem(cid):
    """{variant: problem dict of stemhead_ref} of case cid"""
    c = CASES[cid]
    k, sh = c['kind'], c['shape']
    g = torch.Generator().manual_seed(seed_of(cid))
    if k in ('stem_stats', 'stem_apply'):
        N, C_, T, V, M = sh
        J = C_ * V * M
        x = _randn(sh, g, 1.0, 3.0)                                          # a mean that a centring has to remove
        dout = _randn((N * M, C_, T, V), g)
        if k == 'stem_stats':
            center = R._rows(x).mean((1, 2))                                 # the saved mean of the forward
            return dict(fwd=dict(x=x), bwd=dict(x=x, dout=dout, center=center))
        coef = _coef((3, J), g)
        return dict(fwd=dict(x=x, coef=coef), bwd=dict(x=x, coef=coef, dout=dout))
    if k == 'stem_streams_eval':
        N, C_, T, V, M = sh
        J = C_ * V * M
        x = _randn(sh, g, 1.0, 3.0)
        parent = [(3 * v + 1) % V for v in range(V)]
        return {'modes0123': dict(x=x, parent=parent, modes=[0, 1, 2, 3], coef=_coef((4, 3, J), g)),
                'g1': dict(x=x, parent=parent, modes=[3], coef=_coef((1, 3, J), g))}
    if k in ('pool_fwd', 'pool_bwd'):
        N, C_, T, V, M = sh
        if k == 'pool_fwd':
            return dict(one=dict(x=_randn((N * M, C_, T, V), g, 1.0, 3.0), M=M))
        return dict(one=dict(dpooled=_randn((N, C_), g), M=M, T=T, V=V))
    if k == 'fc_fwd':
        N, C_, K = sh
        p = dict(pooled=_randn((N, C_), g, 1.0, 0.5), W=_randn((K, C_), g), b=_randn((K,), g))
        out = dict(bias=p)
        if sh == (3, 100, 10):
            out['nobias'] = dict(p, b=None)
        return out
    if k == 'fc_grouped':
        N, C_, K = sh
        out = {}
        for G in (1, 3):
            out[f'G{G}'] = dict(pooled=_randn((G * N, C_), g, 1.0, 0.5), W=_randn((G, K, C_), g), b=_randn((G, K), g))
        if sh == (3, 100, 10):
            out['G3.nobias'] = dict(out['G3'], b=None)
        return out
    if k == 'fc_bwd':
        N, C_, K = sh
        return dict(one=dict(dl=_randn((N, K), g), pooled=_randn((N, C_), g, 1.0, 0.5), W=_randn((K, C_), g)))
    if k == 'ce_fwd':
        N, K = sh
        base = torch.randn((N, K), generator=g)
        labels = {pat: ce_labels(pat, N, K, g) for pat in CE_LABELS}
        return {f'{ln}.{pat}': dict(logits=base * sc + shf, labels=labels[pat], shifted=shf != 0.0)
                for ln, (sc, shf) in CE_LOGITS.items() for pat in CE_LABELS}
    if k == 'ce_bwd':
        N, K = sh
        return dict(one=dict(g=_randn((N, K), g, 0.1), dloss=torch.tensor(1.7)))
    if k == 'score_fuse':
        S, N, K = sh
        scores = _randn((S, N, K), g, 3.0)
        w = torch.rand((S,), generator=g) + 0.3
        labels = torch.randint(0, K, (N,), generator=g)
        if N > 1:
            labels[1] = -1                                                   # counted nowhere
        raw = scores.clone()
        if K >= 10:                                                          # exact ties at the top: the same bits in every score set
            two, three = tie_rows(N)
            raw[:, two, 2] = raw[:, two, 7] = 20.0 + raw[:, two, 7].abs()
            raw[:, three, 1] = raw[:, three, 4] = raw[:, three, 9] = 20.0 + raw[:, three, 4].abs()
        return {'raw': dict(scores=raw, w=w, softmax=0, labels=labels), 'softmax': dict(scores=scores, w=w, softmax=1, labels=labels),
                'raw.nolabels': dict(scores=raw, w=w, softmax=0, labels=None), 'softmax.nolabels': dict(scores=scores, w=w, softmax=1, labels=None)}
    raise KeyError(k)


def evaluate(cid, probs, dt):
    """every output of every launch of case cid from stemhead_ref in dtype dt: {variant: {name: tensor}}"""
    return {v: R.evaluate(CASES[cid]['kind'], p, dt) for v, p in probs.items()}


def verify(cid, probs, got):
    """hold `got` (what evaluate() returns, from whatever computed it) to the bars: {output: largest err / bound over the launches}"""
    rat = {}
    for v, p in probs.items():
        for n, r in R.verify(f'{cid} [{v}]', CASES[cid]['kind'], p, got[v]).items():
            rat[n] = max(rat.get(n, 0.0), r)
    return rat


# ---------------------------------------------------------------------------------------------------------------------
# GPU runners
# ---------------------------------------------------------------------------------------------------------------------
class Dev:
    """device buffers of one launch: inputs with NaN around them, outputs pre-filled with a sentinel and GUARD elements behind them"""

    def __init__(self):
        self.outs, self.keep = [], []

    def put(self, t, lead=0, tail=GUARD):
        if t is None:
            return None
        if t.dtype != torch.float32:                                         # labels, parent, modes
            v = t.to('cuda:0')
            self.keep.append(v)
            return v
        flat = torch.full((lead + t.numel() + tail,), NAN, device='cuda:0')
        self.keep.append(flat)
        v = flat[lead:lead + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def out(self, *shape, dtype=torch.float32, fill=SENTINEL):
        n = int(np.prod(shape))
        flat = torch.full((n + GUARD,), fill, dtype=dtype, device='cuda:0')
        self.outs.append((flat, n, fill))
        return flat[:n].view(shape)

    def check_guards(self, name):
        for flat, n, fill in self.outs:
            f = flat.cpu()
            keep = torch.ones(f.numel(), dtype=torch.bool)
            keep[:n] = False
            B.check_untouched(f'{name}: elements behind an output', f, torch.full_like(f, fill), keep)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(name, sym, *args):
    from tam_gcn_amd import _lib, ops
    lib = _lib.load()
    _lib.check(getattr(lib, name)(*args, ops._stream()), name)
    got = lib.tamgcn_last_kernel().decode()
    assert got == sym, f'{name}: dispatched {got}, ledger says {sym}'


def run_variant(cid, vname, p):
    """one launch: the dict stemhead_ref.evaluate returns, as CPU tensors"""
    from tam_gcn_amd import ops
    c = CASES[cid]
    k, sym = c['kind'], c['sym']
    d = Dev()
    name = f'{cid} [{vname}]'
    out = {}
    if k in ('stem_stats', 'stem_apply', 'stem_streams_eval'):
        N, C_, T, V, M = c['shape']
        J = C_ * V * M
    if k == 'stem_stats':
        part = d.out(2, J, N)
        _launch('tamgcn_stem_stats', sym, _ptr(d.put(p['x'])), _ptr(d.put(p.get('dout'))), _ptr(d.put(p.get('center'))), N, C_, T, V, M, _ptr(part))
        out.update(s0=part[0], s1=part[1])
    elif k == 'stem_apply':
        bwd = p.get('dout') is not None
        o = d.out(N, C_, T, V, M) if bwd else d.out(N * M, C_, T, V)
        _launch('tamgcn_stem_apply', sym, _ptr(d.put(p['x'])), _ptr(d.put(p.get('dout'))), _ptr(d.put(p['coef'])), N, C_, T, V, M, _ptr(o))
        out['dx' if bwd else 'out'] = o
    elif k == 'stem_streams_eval':
        G = len(p['modes'])
        per = C_ * T * V * M
        x = d.put(p['x'], lead=per, tail=per)                                # a NaN sample on either side
        parent, modes = d.put(torch.tensor(p['parent'], dtype=torch.int32)), d.put(torch.tensor(p['modes'], dtype=torch.int32))
        coef = d.put(p['coef'])
        o = d.out(G * N * M, C_, T, V)
        _launch('tamgcn_stem_streams_eval', sym, _ptr(x), _ptr(parent), _ptr(modes), _ptr(coef), G, N, C_, T, V, M, _ptr(o))
        for g, mode in enumerate(p['modes']):                                # the pair of launches it replaces, bit for bit
            pair = ops.stem_apply(ops.stream_derive(x, parent, mode), coef[g])
            assert torch.equal(o[g * N * M:(g + 1) * N * M], pair), f'{name}: group {g} (mode {mode}) differs from stream_derive + stem_apply'
        out['out'] = o
    elif k == 'pool_fwd':
        N, C_, T, V, M = c['shape']
        o = d.out(N, C_)
        _launch('tamgcn_head_pool_fwd', sym, _ptr(d.put(p['x'])), N, C_, T, V, M, _ptr(o))
        out['pooled'] = o
    elif k == 'pool_bwd':
        N, C_, T, V, M = c['shape']
        o = d.out(N * M, C_, T, V)
        _launch('tamgcn_head_pool_bwd', sym, _ptr(d.put(p['dpooled'])), N, C_, T, V, M, _ptr(o))
        out['dx'] = o
    elif k in ('fc_fwd', 'fc_grouped'):
        N, C_, K = c['shape']
        x, W, b = d.put(p['pooled']), d.put(p['W']), d.put(p.get('b'))
        G = W.shape[0] if k == 'fc_grouped' else 1
        single = d.out(G, N, K)
        for g in range(G):
            _launch('tamgcn_head_fc_fwd', 'fc_fwd_kernel', _ptr(x[g * N:]), _ptr(W.view(G, K, C_)[g]), None if b is None else _ptr(b.view(G, K)[g]),
                    N, C_, K, _ptr(single[g]))
        grouped = d.out(G, N, K)
        _launch('tamgcn_head_fc_grouped', 'fc_grouped_kernel', _ptr(x), _ptr(W), _ptr(b), G, N, C_, K, _ptr(grouped))
        assert torch.equal(single, grouped), f'{name}: the grouped head differs from the single head'
        if k == 'fc_fwd':
            out['logits'] = single[0]
        else:
            out['scores'] = grouped
    elif k == 'fc_bwd':
        N, C_, K = c['shape']
        dW, db, dp = d.out(K, C_), d.out(K), d.out(N, C_)
        _launch('tamgcn_head_fc_bwd', sym, _ptr(d.put(p['dl'])), _ptr(d.put(p['pooled'])), _ptr(d.put(p['W'])), N, C_, K, _ptr(dW), _ptr(db), _ptr(dp))
        out.update(dW=dW, db=db, dpooled=dp)
    elif k == 'ce_fwd':
        N, K = c['shape']
        loss, g = d.out(1), d.out(N, K)
        _launch('tamgcn_ce_fwd', sym, _ptr(d.put(p['logits'])), _ptr(d.put(p['labels'])), N, K, _ptr(loss), _ptr(g))
        out.update(loss=loss.view(()), g=g)
    elif k == 'ce_bwd':
        N, K = c['shape']
        o = d.out(N, K)
        _launch('tamgcn_ce_bwd', sym, _ptr(d.put(p['g'])), _ptr(d.put(p['dloss'].view(1))), N, K, _ptr(o))
        out['dlogits'] = o
    elif k == 'score_fuse':
        S, N, K = c['shape']
        fused, pred = d.out(N, K), d.out(N, dtype=torch.int64, fill=INT_GUARD)
        stats = d.out(K, 2, dtype=torch.int32, fill=STALE) if p['labels'] is not None else None
        _launch('tamgcn_score_fuse', sym, _ptr(d.put(p['scores'])), _ptr(d.put(p['w'])), S, N, K, p['softmax'], _ptr(d.put(p['labels'])),
                _ptr(fused), _ptr(pred), _ptr(stats))
        out.update(fused=fused, pred=pred)
        if stats is not None:
            out['stats'] = stats
    else:
        raise KeyError(k)
    torch.cuda.synchronize()
    d.check_guards(name)
    return {n: v.cpu() for n, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('cid', list(CASES))
def test_stemhead_form(cid):
    c, probs = CASES[cid], problem(cid)
    got = {v: run_variant(cid, v, p) for v, p in probs.items()}
    rat = verify(cid, probs, got)
    print(f'SH {cid} | {c["sym"]} | launches={len(probs)} | ' + ' '.join(f'{n}={v:.3f}' for n, v in rat.items()))
