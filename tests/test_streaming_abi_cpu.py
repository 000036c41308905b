"""The entry points of csrc/streaming.hip refuse bad arguments before any HIP call, with a negative status and a message that
begins with their own name; FrameRing, SlidingWindow and LiveClassifier refuse bad constructor arguments before any launch.  No
GPU needed: the host addresses below are never dereferenced."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from tam_gcn_amd import build, _lib
    build.build()
    return _lib.load()


_buf = (C.c_double * 64)()
P = C.addressof(_buf) + (-C.addressof(_buf)) % 16


def _refused(lib, fn, args, text=None):
    rc = getattr(lib, fn)(*args)
    msg = lib.tamgcn_last_error()
    assert rc < 0, (fn, rc)
    assert msg.startswith(fn.encode() + b':'), msg
    if text:
        assert text.encode() in msg, msg


# a call every check accepts, per entry point (never made: each test breaks one argument)
GOOD = {
    'tamgcn_ring_push': [P, 4, 1, 60, 8, P, 16, P, None],
    'tamgcn_ring_plan': [P, 16, 3, 9, 4, P, None],
    'tamgcn_window_nucla': [P, 16, P, 3, P, 20, 52, 1, 0, P, None],
    'tamgcn_window_clip': [P, 16, P, 3, 3, 17, 1, 8, P, None],
    'tamgcn_window_vote': [P, P, 6, 10, 27, P, P, P, None],
    'tamgcn_score_ema': [P, P, 10, 0.8, P, P, P, P, P, None],
}
POINTERS = {'tamgcn_ring_push': (0, 5, 7), 'tamgcn_ring_plan': (0, 5), 'tamgcn_window_nucla': (0, 2, 4, 9),
            'tamgcn_window_clip': (0, 2, 8), 'tamgcn_window_vote': (0, 1, 5), 'tamgcn_score_ema': (0, 1, 4, 5, 6, 7, 8)}


def _with(fn, **changes):
    args = list(GOOD[fn])
    for i, v in changes.items():
        args[int(i[1:])] = v
    return args


@pytest.mark.parametrize('fn', sorted(GOOD))
def test_null_pointers_are_refused(lib, fn):
    for i in POINTERS[fn]:
        _refused(lib, fn, _with(fn, **{f'a{i}': None}), 'null pointer')


def test_ring_push_refuses_what_does_not_fit(lib):
    _refused(lib, 'tamgcn_ring_push', _with('tamgcn_ring_push', a1=17), 'n = 17 frames outside 1..cap = 16')
    _refused(lib, 'tamgcn_ring_push', _with('tamgcn_ring_push', a1=0), 'n = 0')
    for elem in (0, 2, 16, -4):
        _refused(lib, 'tamgcn_ring_push', _with('tamgcn_ring_push', a4=elem), f'elem {elem}')
    _refused(lib, 'tamgcn_ring_push', _with('tamgcn_ring_push', a2=0), 'bad dims P=0 R=60 cap=16')
    _refused(lib, 'tamgcn_ring_push', _with('tamgcn_ring_push', a6=0), 'bad dims')


def test_ring_plan_refuses_an_empty_or_oversized_window(lib):
    _refused(lib, 'tamgcn_ring_plan', _with('tamgcn_ring_plan', a3=0), 'window L = 0 outside 1..cap = 16')
    _refused(lib, 'tamgcn_ring_plan', _with('tamgcn_ring_plan', a3=-3), 'window L = -3')
    _refused(lib, 'tamgcn_ring_plan', _with('tamgcn_ring_plan', a3=17), 'window L = 17')
    _refused(lib, 'tamgcn_ring_plan', _with('tamgcn_ring_plan', a4=0), 'bad dims cap=16 B=3 hop=0')
    _refused(lib, 'tamgcn_ring_plan', _with('tamgcn_ring_plan', a2=0), 'bad dims')


def test_window_nucla_refuses_its_limits(lib):
    _refused(lib, 'tamgcn_window_nucla', _with('tamgcn_window_nucla', a6=65), 'time_steps 65 outside 1..64')
    _refused(lib, 'tamgcn_window_nucla', _with('tamgcn_window_nucla', a6=0), 'time_steps 0')
    _refused(lib, 'tamgcn_window_nucla', _with('tamgcn_window_nucla', a7=20), 'centre joint 20 outside 0..19')
    _refused(lib, 'tamgcn_window_nucla', _with('tamgcn_window_nucla', a8=4), 'mode 4')
    _refused(lib, 'tamgcn_window_nucla', _with('tamgcn_window_nucla', a3=0), 'bad dims cap=16 B=0 V=20')


def test_window_clip_refuses_bad_dims(lib):
    for i in (1, 3, 4, 5, 6, 7):
        _refused(lib, 'tamgcn_window_clip', _with('tamgcn_window_clip', **{f'a{i}': 0}), 'bad dims')
    _refused(lib, 'tamgcn_window_clip', _with('tamgcn_window_clip', a1=2 ** 30, a5=4), 'channel plane above 2^30')


def test_scores_refuse_too_many_classes(lib):
    _refused(lib, 'tamgcn_window_vote', _with('tamgcn_window_vote', a3=4097), 'K=4097')
    _refused(lib, 'tamgcn_window_vote', _with('tamgcn_window_vote', a6=None), 'go together')
    _refused(lib, 'tamgcn_window_vote', _with('tamgcn_window_vote', a4=0), 'n_frames = 0')
    _refused(lib, 'tamgcn_score_ema', _with('tamgcn_score_ema', a2=4097), 'K = 4097 outside 1..4096')
    _refused(lib, 'tamgcn_score_ema', _with('tamgcn_score_ema', a2=0), 'K = 0')
    for beta in (1.0, -0.1, float('nan')):
        _refused(lib, 'tamgcn_score_ema', _with('tamgcn_score_ema', a3=beta), 'beta')


class _Net(torch.nn.Module):
    """Stands in for a model: the constructors look at its mode and its joint count before anything else."""
    num_point = 20

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_frame_ring_refuses_bad_arguments_before_any_allocation():
    from tam_gcn_amd.streaming import FrameRing
    for kw in (dict(capacity=0, V=20), dict(capacity=16), dict(capacity=16, V=0), dict(capacity=True, V=20), dict(capacity=16.0, V=20),
               dict(capacity=16, V=20, prep='ntu'), dict(capacity=16, V=20, prep='nucla', M=2), dict(capacity=16, V=20, prep='nucla', C=2),
               dict(capacity=16, V=20, prep='clip', C=0), dict(capacity=16, V=20, device='cpu')):
        with pytest.raises(ValueError, match='FrameRing'):
            FrameRing(**kw)


def test_sliding_window_refuses_bad_arguments():
    from tam_gcn_amd.streaming import SlidingWindow
    net = _Net().eval()
    for kw in (dict(window=0, hop=8), dict(window=20, hop=0), dict(window=20, hop=8, prep='ntu'), dict(window=20, hop=8, stream='velocity'),
               dict(window=20, hop=8, time_steps=65), dict(window=20, hop=8, time_steps=0), dict(window=20, hop=8, window_size=64),
               dict(window=20, hop=8, prep='clip'), dict(window=20, hop=8, prep='clip', window_size=64, time_steps=52),
               dict(window=20, hop=8, batch_windows=0), dict(window=20.5, hop=8)):
        with pytest.raises(ValueError, match='SlidingWindow'):
            SlidingWindow(net, **kw)
    with pytest.raises(ValueError, match='eval'):
        SlidingWindow(_Net().train(), window=20, hop=8)
    with pytest.raises(ValueError, match='num_point'):
        SlidingWindow(torch.nn.Linear(2, 2).eval(), window=20, hop=8)


def test_live_classifier_refuses_bad_arguments_before_any_launch():
    from tam_gcn_amd.streaming import FrameRing, LiveClassifier
    net = _Net().eval()

    class Ring(FrameRing):                           # the geometry of a ring without its device tensors
        def __init__(self, capacity, prep='nucla', V=20, C=3, M=1):
            self.capacity, self.prep, self.V, self.C, self.M = capacity, prep, V, C, M
    with pytest.raises(ValueError, match='must be a FrameRing'):
        LiveClassifier(net, object(), window=20)
    for kw in (dict(window=0), dict(window=20, hop_windows=0), dict(window=20, hop=0), dict(window=20, beta=1.0), dict(window=20, beta=-0.5),
               dict(window=20, beta='x'), dict(window=20, frames_per_step=0), dict(window=20, frames_per_step=65),
               dict(window=65), dict(window=20, hop_windows=4, hop=15),                      # 20 + 3 * 15 = 65 > 64
               dict(window=20, stream='velocity'), dict(window=20, time_steps=65), dict(window=20, window_size=64)):
        with pytest.raises(ValueError, match='LiveClassifier'):
            LiveClassifier(net, Ring(64), **kw)
    with pytest.raises(ValueError, match='joints'):
        LiveClassifier(net, Ring(64, V=17), window=20)
    with pytest.raises(ValueError, match='eval'):
        LiveClassifier(_Net().train(), Ring(64), window=20)
    with pytest.raises(ValueError, match='window_size'):
        LiveClassifier(net, Ring(64, prep='clip'), window=20)


def test_the_per_step_state_watch_sees_what_the_state_key_sees():
    """streaming._StateWatch reads evaluation._state_key's tensors and counters without walking the module tree: an in-place edit, a
    BatchNorm update and load_state_dict move it at once and once; a replaced sub-module object at the next whole comparison."""
    from tam_gcn_amd import functional as Fn
    from tam_gcn_amd.evaluation import _state_key
    from tam_gcn_amd.models.ctrgcn import Model
    from tam_gcn_amd.streaming import _StateWatch
    m = Model(num_class=10, num_point=20, num_person=1, graph='tam_gcn_amd.graph.ucla.Graph', graph_args=dict(labeling_mode='spatial')).eval()
    w = _StateWatch(m)
    assert not w.moved() and w.full == _state_key(m)
    with torch.no_grad():
        m.fc.bias.add_(1.0)
    assert w.moved() and not w.moved() and w.full == _state_key(m)
    Fn._bn_epoch(m.data_bn)[0] += 1
    assert w.moved() and not w.moved()
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert w.moved() and not w.moved()
    w = _StateWatch(m, recheck=3)
    m.fc = torch.nn.Linear(256, 10)
    assert [w.moved() for _ in range(4)] == [False, False, True, False]
    m.fc = torch.nn.Linear(256, 10)
    w.invalidate()
    assert w.moved() and not w.moved()
