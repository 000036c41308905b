"""-m gpu: one ring is a bank of one feed, and nothing a caller sees moved with that.  The single-ring ops give the bits recorded
on the commit before the ring and bank kernels became one (tools/record_streaming_bits.py -> golden/streaming_parent.npz), and
LiveClassifier equals the chain its docstring describes, spelled out with the single-ring ops."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import stream_ensemble_models as SM
from tam_gcn_amd import ops
from tam_gcn_amd.feeder.feeder_nucla_gcn import BONE_PARENT
from tam_gcn_amd.streaming import FrameRing, LiveClassifier

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')


def test_the_single_ring_ops_give_the_recorded_bits():
    spec = importlib.util.spec_from_file_location('record_streaming_bits', os.path.join(ROOT, 'tools', 'record_streaming_bits.py'))
    recorder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recorder)
    want = np.load(os.path.join(ROOT, 'tests', 'golden', 'streaming_parent.npz'))
    got = recorder.record()
    assert sorted(got) == sorted(want.files) and len(got) > 100
    for name in want.files:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name      # no NaN in these arrays: equal values of one dtype are equal bits
    assert all(np.isfinite(want[name]).all() for name in want.files)


@pytest.mark.parametrize('eager', [False, True], ids=['graph', 'eager'])
def test_live_classifier_equals_its_documented_chain(eager):
    """push -> plan -> window -> forward -> softmax -> average, the average window by window, oldest first: three score_ema
    launches against the class's one launch for the step's three windows."""
    model = SM.base_model('ucla_t52').to(DEV).eval()
    rng = np.random.default_rng(11)
    seq = rng.normal(size=(1, 20, 3)) + 0.05 * np.cumsum(rng.normal(size=(40, 20, 3)), axis=0)
    frames = torch.from_numpy(seq).to(DEV)
    B, hop, window, beta, n = 3, 4, 20, 0.5, 4
    live = LiveClassifier(model, FrameRing(32, 'nucla', V=20, device=DEV), window=window, hop_windows=B, hop=hop, beta=beta, frames_per_step=n,
                          eager=eager)
    ring = FrameRing(32, 'nucla', V=20, device=DEV)
    parent = torch.tensor(BONE_PARENT, dtype=torch.int32, device=DEV)
    ema = torch.zeros(live.num_class, dtype=torch.float64, device=DEV)
    seen = torch.zeros(1, dtype=torch.int64, device=DEV)
    moved = []
    for s in range(10):
        chunk = frames[n * s:n * s + n]
        got = live.step(chunk)
        ops.ring_push(chunk.contiguous(), ring.buf, ring.state)
        plan = ops.ring_plan(ring.state, ring.capacity, B, window, hop)
        with torch.no_grad():
            logits = model(ops.window_nucla(ring.buf, plan, parent, 52, 1, 'joint'))
        probs, _, _ = ops.window_vote(logits, plan)
        for j in range(B):                                                      # oldest first
            smoothed, label, conf = ops.score_ema(probs[j], plan[j], beta, ema, seen)
        for name, a, b in zip(('label', 'conf', 'smoothed', 'logits', 'ema', 'seen'), got + (live.ema, live.seen),
                              (label, conf, smoothed, logits, ema, seen)):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (s, name)
        moved.append(int(seen))
    assert moved == [0, 0, 0, 0, 1, 3, 6, 9, 12, 15] and int(label) >= 0          # invalid, partly valid and all-valid steps
