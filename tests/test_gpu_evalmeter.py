"""-m gpu: tamgcn_eval_accumulate behind tam_gcn_amd.evaluation.EvalMeter against the fp64 restatement tests/evalmeter_ref.py
(itself held against the reference's formulas by tests/test_evalmeter_cpu.py) and, for the loss, against tamgcn_ce_fwd bit for bit."""
import numpy as np
import pytest
import torch

import evalmeter_ref as R
import tam_gcn_amd.torch_ops  # noqa: F401  (registers torch.ops.tamgcn.cross_entropy)
from tam_gcn_amd.evaluation import EvalMeter

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SHAPES = [(1, 3), (7, 60), (256, 10), (300, 10)]            # 300: more rows than the workgroup has threads
TOPK = (1, 2, 5, 70)
GUARD = 4096


def _batch(B, K, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'ties':
        x = rng.integers(-2, 3, size=(B, K)).astype(np.float32)           # ties in nearly every row
    else:
        x = (3 * rng.standard_normal((B, K))).astype(np.float32)
        assert all(len(np.unique(r)) == K for r in x)
    return x, rng.integers(0, K, size=B).astype(np.int64)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(meter, ref, scores=True):
    got = meter.compute()
    want = ref.compute()
    R.assert_same_metrics(got, want)
    if scores and want['scores'] is not None:
        assert np.array_equal(got['scores'], want['scores'], equal_nan=True)
    return got, want


@pytest.mark.parametrize('kind', ['ties', 'free'])
@pytest.mark.parametrize('B,K', SHAPES)
def test_one_batch_equals_the_restatement_and_the_loss_kernel(B, K, kind):
    x, lab = _batch(B, K, kind, seed=B * K)
    xd, ld = _t(x), _t(lab)
    meter = EvalMeter(K, num_samples=B, topk=TOPK, device=DEV)
    for valid in sorted({B, B - 1, 1, 0}, reverse=True):
        meter.reset()
        meter.update(xd, ld, valid=valid)
        ref = R.Meter(K, num_samples=B, topk=TOPK)
        ref.update(x, lab, valid=valid)
        got, want = _check(meter, ref)
        print(f'B={B} K={K} {kind} valid={valid}: loss {got["loss"]!r} ref {want["loss"]!r}')
        assert got['count'] == valid and got['batches'] == (1 if valid else 0)
        if valid:
            ce = torch.ops.tamgcn.cross_entropy(xd[:valid].contiguous(), ld[:valid].contiguous())[0]
            assert meter.sums[0].item() == float(ce), (meter.sums[0].item(), float(ce))       # the batch mean, bit for bit
            assert got['loss'] == float(ce)
        else:
            assert np.isnan(got['loss']) and np.isnan(got['top1']) and int(meter.confusion.abs().sum()) == 0
    # valid = None is the whole batch
    meter.reset()
    meter.update(xd, ld)
    ref = R.Meter(K, num_samples=B, topk=TOPK)
    ref.update(x, lab)
    _check(meter, ref)


def test_three_updates_accumulate():
    K = 10
    parts = [_batch(B, K, kind, seed=70 + i) for i, (B, kind) in enumerate([(300, 'ties'), (7, 'free'), (256, 'ties')])]
    n = sum(len(x) for x, _ in parts)
    meter = EvalMeter(K, num_samples=n, topk=TOPK, device=DEV)
    ref = R.Meter(K, num_samples=n, topk=TOPK)
    valids = [None, 5, 255]
    for (x, lab), v in zip(parts, valids):
        meter.update(_t(x), _t(lab), valid=v)
        ref.update(x, lab, valid=v)
    got, want = _check(meter, ref)
    assert got['batches'] == 3 and got['count'] == 300 + 5 + 255
    # the integer state and the per-sample loss do not depend on where the batches were cut
    cat = R.Meter(K, topk=TOPK)
    cat.update(np.concatenate([x[:len(x) if v is None else v] for (x, _), v in zip(parts, valids)]),
               np.concatenate([l[:len(l) if v is None else v] for (_, l), v in zip(parts, valids)]))
    one = cat.compute()
    assert np.array_equal(got['confusion'], one['confusion']) and got['topk'] == one['topk'] and got['top1'] == one['top1']
    assert abs(got['sample_loss'] - one['sample_loss']) <= 2e-6 * max(1.0, abs(one['sample_loss']))
    assert got['loss'] != got['sample_loss']                  # the mean of batch means weighs the batches equally


def _guarded(shape, dtype, fill):
    """A tensor of `shape` in the middle of a buffer whose other elements hold `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def test_out_of_range_labels_and_indices_are_skipped_and_counted():
    B, K, NS = 300, 10, 310
    x, lab = _batch(B, K, 'free', seed=5)
    lab[[0, 17, 256, 299]] = -100
    lab[[3, 257]] = K + 3
    lab[40] = -1
    lab[41] = 10 ** 12
    rng = np.random.default_rng(6)
    idx = rng.permutation(NS)[:B].astype(np.int64)
    idx[[1, 258]] = -1
    idx[[2, 298]] = NS
    idx[5] = -10 ** 12
    idx[6] = 10 ** 12
    meter = EvalMeter(K, num_samples=NS, topk=TOPK, device=DEV)
    sbuf, meter.scores = _guarded((NS, K), torch.float32, 7.0)
    cbuf, meter.confusion = _guarded((K, K), torch.int32, -5)
    meter.reset()
    meter.update(_t(x), _t(lab), index=_t(idx))
    ref = R.Meter(K, num_samples=NS, topk=TOPK)
    ref.update(x, lab, index=idx)
    got, want = _check(meter, ref)
    assert got['bad_labels'] == 4 and got['bad_index'] == 6 and got['count'] == B - 8
    assert np.isnan(got['loss']) and np.isfinite(got['sample_loss'])            # tamgcn_ce_fwd's convention for a bad label
    ce = torch.ops.tamgcn.cross_entropy(_t(x), _t(lab))[0]
    assert torch.isnan(ce)
    stored = np.zeros(NS, dtype=bool)
    ok = (idx >= 0) & (idx < NS)
    stored[idx[ok]] = True
    assert np.array_equal(got['scores'][idx[ok]], x[ok]) and np.isnan(got['scores'][~stored]).all()
    for buf, n, fill in ((sbuf, NS * K, 7.0), (cbuf, K * K, -5)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())
    # rows past `valid` are not looked at: bad values there change nothing
    meter.reset()
    lab2, idx2 = lab.copy(), idx.copy()
    lab2[100:] = K + 3
    idx2[100:] = -1
    x2 = x.copy()
    x2[100:] = np.nan
    meter.update(_t(x2), _t(lab2), index=_t(idx2), valid=100)
    ref = R.Meter(K, num_samples=NS, topk=TOPK)
    ref.update(x, lab, index=idx, valid=100)
    _check(meter, ref)
    for buf, n, fill in ((sbuf, NS * K, 7.0), (cbuf, K * K, -5)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def test_permuted_index_and_running_rows():
    B, K = 7, 60
    x, lab = _batch(B, K, 'ties', seed=8)
    perm = np.random.default_rng(1).permutation(2 * B)[:B].astype(np.int64)
    meter = EvalMeter(K, num_samples=2 * B, topk=(1, 5), device=DEV)
    meter.update(_t(x), _t(lab), index=_t(perm))
    sc = meter.compute()['scores']
    assert np.array_equal(sc[perm], x) and np.isnan(np.delete(sc, perm, axis=0)).all()
    # without an index the rows are numbered as they come: `valid` rows per update
    meter.reset()
    meter.update(_t(x), _t(lab), valid=4)
    meter.update(_t(x), _t(lab))
    sc = meter.compute()['scores']
    assert np.array_equal(sc[:4], x[:4]) and np.array_equal(sc[4:4 + B], x) and np.isnan(sc[4 + B:]).all()


def test_update_replays_from_a_graph_with_valid_on_the_device():
    B, K = 300, 10
    batches = [_batch(B, K, kind, seed=90 + i) for i, kind in enumerate(['ties', 'free'])]
    valids = [300, 37]
    xs, ls = torch.zeros(B, K, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    vd = torch.zeros((), dtype=torch.int32, device=DEV)
    meter = EvalMeter(K, num_samples=2 * B, topk=TOPK, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        meter.update(xs, ls, index=idx, valid=vd)              # warm-up off the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        meter.update(xs, ls, index=idx, valid=vd)
    meter.reset()
    eager = EvalMeter(K, num_samples=2 * B, topk=TOPK, device=DEV)
    ref = R.Meter(K, num_samples=2 * B, topk=TOPK)
    for i, ((x, lab), v) in enumerate(zip(batches, valids)):
        xs.copy_(_t(x)); ls.copy_(_t(lab)); vd.fill_(v); idx.copy_(torch.arange(B, device=DEV) + i * B)
        g.replay()
        eager.update(_t(x), _t(lab), index=idx.clone(), valid=v)
        ref.update(x, lab, index=np.arange(B) + i * B, valid=v)
    _check(meter, ref)
    for a, b in zip(meter.state().values(), eager.state().values()):
        assert torch.equal(a, b) or (a.dtype == torch.float32 and torch.equal(a.nan_to_num(nan=-1e30), b.nan_to_num(nan=-1e30)))


def test_reset_and_argument_errors():
    K = 3
    x, lab = _batch(1, K, 'free', seed=2)
    meter = EvalMeter(K, num_samples=2, topk=(1,), device=DEV)
    meter.update(_t(x), _t(lab))
    assert meter.compute()['count'] == 1
    meter.reset()
    res = meter.compute()
    assert res['count'] == 0 and res['batches'] == 0 and int(res['confusion'].sum()) == 0 and np.isnan(res['scores']).all()
    assert np.isnan(res['loss']) and res['class_acc'] == {c: (0, 0, 0.0) for c in range(K)}
    assert set(meter.state()) == {'counts', 'sums', 'confusion', 'scores'}
    with pytest.raises(ValueError, match='EvalMeter'):
        meter.update(torch.zeros(1, K + 1, device=DEV), _t(lab))
    with pytest.raises(RuntimeError, match='tam_gcn_amd'):
        meter.update(_t(x), _t(lab).int())
    with pytest.raises(RuntimeError, match='valid'):
        meter.update(_t(x), _t(lab), valid=2)
    with pytest.raises(ValueError, match='EvalMeter'):
        EvalMeter(K, topk=(1, 2, 3, 4, 5), device=DEV)
    assert meter.compute()['count'] == 0                        # nothing was launched by the refused calls


@pytest.mark.parametrize('softmax', [False, True])
def test_score_sweep_equals_fuse_per_alpha(softmax):
    """tamgcn_score_sweep against tamgcn_score_fuse with weights (1, alpha), alpha by alpha: the same predictions, so the same
    counts -- on scores full of near and exact ties (integer-valued a, b in multiples of 1/8, so that a product's rounding can
    decide the arg max) and on continuous ones."""
    from tam_gcn_amd import ensemble
    alphas = list(ensemble.REFERENCE_ALPHAS)
    for (N, K), kind in (((300, 10), 'ties'), ((7, 60), 'free'), ((1, 3), 'free'), ((257, 60), 'ties')):
        a, lab = _batch(N, K, kind, seed=N + K)
        b = _batch(N, K, kind, seed=N + K + 1)[0] * (0.125 if kind == 'ties' else 1.0)
        accs, best, best_acc = ensemble.sweep(a, b, alphas, lab, softmax=softmax)
        want = []
        for alpha in alphas:
            _, pred, _ = ensemble.fuse([a, b], [1.0, alpha], softmax=softmax)
            want.append(int((pred.cpu().numpy() == lab).sum()) / N)
        assert accs == want, (N, K, kind, accs, want)
        assert (best, best_acc) == ensemble.best_alpha(alphas, want)
    with pytest.raises(ValueError, match='label outside'):
        ensemble.sweep(a, b, alphas, lab + K)
    # more alphas than one launch takes are cut into launches
    many = [0.05 * i for i in range(1, 21)]
    accs, _, _ = ensemble.sweep(a, b, many, lab, softmax=softmax, start_alpha=0.5)
    assert len(accs) == 20 and accs[9] == ensemble.sweep(a, b, [0.5], lab, softmax=softmax)[0][0]
