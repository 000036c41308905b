"""-m gpu: tam_gcn_amd.evaluation.CapturedEval -- a val split through GraphedBatch, GraphedForward and the device meter --
against an eager pass over the same padded batches (Feeder.batch, model(x) under no_grad) and the fp64 restatement
tests/evalmeter_ref.py applied to its scores.  The seeded N-UCLA model of tests/stream_ensemble_models.py with running statistics
settled on feeder clips (_model), a synthetic val split made like tests/test_gpu_feeder_draw.py::_synthetic."""
import json
import os

import numpy as np
import pytest
import torch

import evalmeter_ref as R
import stream_ensemble_models as SM
from tam_gcn_amd import ensemble
from tam_gcn_amd.distributed import ParamArena
from tam_gcn_amd.evaluation import CapturedEval
from tam_gcn_amd.feeder.feeder_nucla_gcn import Feeder
from tam_gcn_amd.inference import StreamEnsemble
from tam_gcn_amd.optim import FusedSGD

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
TAG = 'ucla_t52'
K = 10
LENGTHS = {11: [1, 60, 2, 52, 53, 17, 130, 5, 33, 71, 8],                        # lengths 1 and > 52 among them
           40: [1 + (7 * k) % 90 for k in range(40)]}


def _synthetic(path, lengths, seed=11):
    rng = np.random.default_rng(seed)
    dd = []
    for k, n in enumerate(lengths):
        name = f'a{1 + k % 6:02d}_s{k:02d}_e00_v03'
        clip = rng.normal(size=(1, 20, 3)) + 0.05 * np.cumsum(rng.normal(size=(n, 20, 3)), axis=0)
        os.makedirs(path / name, exist_ok=True)
        with open(path / name / (name + '.json'), 'w') as f:
            json.dump({'skeletons': clip.tolist()}, f)
        dd.append({'file_name': name, 'label': 1 + (3 * k) % 10})
    return dd


@pytest.fixture(scope='module')
def feeders(tmp_path_factory):
    out = {}
    for n, lengths in LENGTHS.items():
        path = tmp_path_factory.mktemp(f'val{n}')
        out[n] = Feeder(str(path), 'val', data_dict=_synthetic(path, lengths), device=DEV)
    return out


_CALIBRATED = {}


def _model(fd, g=None):
    """The seeded N-UCLA model (g: its perturbed copy number g) with running statistics that belong to its inputs.  The golden
    statistics the other GPU tests load are those of tests/golden/params.py's inputs; feeder clips are another distribution,
    under which the eval-mode activations grow from block to block (logits of 1e4).  So the statistics are settled here by 40
    train-mode forwards over the 11-clip split (momentum 0.1: 1 - 0.9^40 = 98.5 % of the way), once per model."""
    m = (SM.base_model(TAG) if g is None else SM.perturbed_model(TAG, g)).to(DEV)
    if g not in _CALIBRATED:
        m.train()
        x, _, _ = fd.batch(range(len(fd)))
        for _ in range(40):
            m(x)
        _CALIBRATED[g] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    else:
        m.load_state_dict(_CALIBRATED[g])
    return m.eval()


def _eager(model, fd, B, topk=(1, 5)):
    """Scores (n, K) of an eager pass over the padded batches and the restatement's metrics of them."""
    n = len(fd)
    scores = np.full((n, K), np.nan, dtype=np.float32)
    ref = R.Meter(K, num_samples=n, topk=topk)
    tail = None
    for b in range(0, n, B):
        idx = [i if i < n else 0 for i in range(b, b + B)]
        valid = min(B, n - b)
        x, lab, _ = fd.batch(idx)
        with torch.no_grad():
            out = model(x).cpu().numpy()
            if valid < B:
                tail = model(x[:valid].contiguous()).cpu().numpy()               # the unpadded tail
        scores[b:b + valid] = out[:valid]
        ref.update(out, lab.cpu().numpy(), index=np.asarray(idx), valid=valid)
    return scores, ref.compute(), tail


def _assert_run(res, model, fd, B, topk=(1, 5)):
    scores, want, tail = _eager(model, fd, B, topk)
    assert np.array_equal(res['scores'], scores), float(np.abs(res['scores'] - scores).max())
    R.assert_same_metrics(res, want)
    assert res['count'] == len(fd) and res['batches'] == -(-len(fd) // B) and res['bad_labels'] == 0 and res['bad_index'] == 0
    if tail is not None:
        err = float(np.abs(res['scores'][len(fd) - len(tail):] - tail).max())
        print(f'n={len(fd)} B={B}: max |logit| {float(np.abs(scores).max()):.3e}, padded vs unpadded tail max-abs-err {err:.3e}; loss {res["loss"]!r} ref {want["loss"]!r}')
        assert err <= 1e-3
    return scores


@pytest.mark.parametrize('n,B,tail', [(11, 4, 3), (40, 36, 4)])          # 4 clips: the small-batch route; 36 > 32: the general path
def test_run_equals_the_eager_pass(feeders, n, B, tail):
    fd, model = feeders[n], _model(feeders[11])
    ev = CapturedEval(model, fd, B)
    assert ev._valid[-1] == tail and len(ev._valid) == -(-n // B)
    meter = ev.run()
    state = [t.clone() for t in meter.state().values()]
    res = meter.compute()
    _assert_run(res, model, fd, B)
    assert 0.0 <= res['top1'] <= res['topk'][5] <= 1.0 and np.isfinite(res['loss'])
    # a second run is the first, bit for bit, from the same graphs, and the host never waits for the device in it
    torch.cuda.set_sync_debug_mode('error')                    # a synchronising call or a copy to the host inside run() raises
    try:
        again = ev.run()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert ev.captures == 1
    for a, b in zip(state, again.state().values()):
        assert torch.equal(a, b)


def test_run_sees_changed_parameters(feeders):
    fd, B = feeders[11], 4
    model = _model(fd)
    arena = ParamArena(model)
    bucket = arena.grad_bucket()
    opt = FusedSGD(arena, bucket, lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    ev = CapturedEval(model, fd, B)
    first = ev.run().compute()
    _assert_run(first, model, fd, B)
    # (a) one optimiser step through the arena: no parameter's _version moves, the arena's state_version() does
    gen = torch.Generator().manual_seed(3)
    bucket.flat.copy_(0.5 * torch.randn(bucket.flat.shape, generator=gen))
    opt.step()
    second = ev.run().compute()
    assert ev.captures == 2
    _assert_run(second, model, fd, B)
    assert not np.array_equal(second['scores'], first['scores'])
    # (b) load_state_dict of a perturbed copy
    sd = {k: (v * (1 + 0.02 * (2 * torch.rand(v.shape, generator=gen).to(v.device) - 1)) if v.is_floating_point() and 'running_var' not in k else v.clone())
          for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    third = ev.run().compute()
    assert ev.captures == 3
    _assert_run(third, model, fd, B)
    assert not np.array_equal(third['scores'], second['scores'])
    # unchanged parameters: no new capture
    ev.run()
    assert ev.captures == 3


def test_train_mode_is_refused(feeders):
    fd = feeders[11]
    model = _model(fd)
    with pytest.raises(ValueError, match='CapturedEval'):
        CapturedEval(model.train(), fd, 4)
    ev = CapturedEval(model.eval(), fd, 4)
    before = [t.clone() for t in ev.run().state().values()]
    model.train()
    with pytest.raises(RuntimeError, match='train'):
        ev.run()
    with pytest.raises(RuntimeError, match='train'):
        ev.update(ev._gb.x, ev._gb.y)
    for a, b in zip(before, ev.meter.state().values()):        # the refused calls launched nothing
        assert torch.equal(a, b)
    model.eval()
    with pytest.raises(ValueError, match='val'):
        CapturedEval(model, Feeder(fd.data_path, 'train', data_dict=fd.data_dict, device=DEV), 4)


def test_own_loader_form(feeders):
    fd, B = feeders[11], 4
    model = _model(fd)
    x0, _, _ = fd.batch([0] * B)
    ev = CapturedEval(model, None, B, example_x=x0, num_samples=len(fd))
    with pytest.raises(RuntimeError, match='feeder'):
        ev.run()
    ev.reset()
    n = len(fd)
    for b in range(0, n, B):
        idx = [i if i < n else 0 for i in range(b, b + B)]
        x, y, _ = fd.batch(idx)
        ev.update(x, y, valid=min(B, n - b))                   # rows numbered as they come
    _assert_run(ev.meter.compute(), model, fd, B)


def test_stream_ensemble_and_alpha_sweep(feeders):
    fd, B = feeders[11], 4
    models = [_model(fd, 0), _model(fd, 1)]
    ens = StreamEnsemble(models, ('joint', 'bone'))
    ev = CapturedEval(ens, fd, B)
    res = ev.run().compute()
    assert ens.arrangement is None                              # left as it was
    _assert_run(res, ens, fd, B)                                # bit-equal to ens(x), metrics from those scores
    # the alpha sweep on the stored scores of two single-model runs == ensemble.fuse per alpha
    sa = CapturedEval(models[0], fd, B).run().compute()['scores']
    sb = CapturedEval(models[1], fd, B).run().compute()['scores']
    assert not np.isnan(sa).any() and not np.array_equal(sa, sb)
    lab = np.asarray(fd.label)
    for softmax in (False, True):
        accs, best, best_acc = ensemble.sweep(sa, sb, ensemble.REFERENCE_ALPHAS, lab, softmax=softmax, start_alpha=1.0)
        want = []
        for alpha in ensemble.REFERENCE_ALPHAS:
            _, pred, _ = ensemble.fuse([sa, sb], [1.0, alpha], softmax=softmax)
            want.append(int((pred.cpu().numpy() == lab).sum()) / len(lab))
        assert accs == want, (softmax, accs, want)
        assert (best, best_acc) == ensemble.best_alpha(ensemble.REFERENCE_ALPHAS, want, 1.0, want[5])
