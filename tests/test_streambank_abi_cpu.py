"""The tamgcn_bank_* entry points of csrc/streaming.hip refuse bad arguments before any HIP call, with a negative status and a
message that begins with their own name; RingBank and LiveBank refuse bad constructor arguments before any launch.  No GPU
needed: the host addresses below are never dereferenced."""
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
    'tamgcn_bank_push': [P, 3, 2, 1, 60, 8, P, 16, P, P, P, None],
    'tamgcn_bank_plan': [P, P, 3, 16, 2, 9, 4, P, None],
    'tamgcn_bank_window_nucla': [P, 3, 16, P, 2, P, 20, 52, 1, 0, P, None],
    'tamgcn_bank_window_clip': [P, 3, 16, P, 2, 3, 17, 1, 8, P, None],
    'tamgcn_bank_ema': [P, P, P, 3, 2, 10, 0.8, P, P, P, P, P, P, None],
    'tamgcn_bank_decide': [P, P, P, P, P, 3, 0.6, 3, P, P, P, P, 16, None],
}
# the pointers that must not be null (counts and restart may be)
POINTERS = {'tamgcn_bank_push': (0, 6, 8), 'tamgcn_bank_plan': (0, 7), 'tamgcn_bank_window_nucla': (0, 3, 5, 10),
            'tamgcn_bank_window_clip': (0, 3, 9), 'tamgcn_bank_ema': (0, 1, 7, 8, 9, 10, 11, 12), 'tamgcn_bank_decide': (0, 1, 2, 4, 8, 9, 10, 11)}
FEEDS_AT = {'tamgcn_bank_push': 1, 'tamgcn_bank_plan': 2, 'tamgcn_bank_window_nucla': 1, 'tamgcn_bank_window_clip': 1, 'tamgcn_bank_ema': 3,
            'tamgcn_bank_decide': 5}


def _with(fn, **changes):
    args = list(GOOD[fn])
    for i, v in changes.items():
        args[int(i[1:])] = v
    return args


def test_every_bank_entry_point_is_exported(lib):
    for fn in GOOD:
        assert hasattr(lib, fn), fn


@pytest.mark.parametrize('fn', sorted(GOOD))
def test_null_pointers_are_refused(lib, fn):
    for i in POINTERS[fn]:
        _refused(lib, fn, _with(fn, **{f'a{i}': None}), 'null pointer')


@pytest.mark.parametrize('fn', sorted(GOOD))
def test_the_feed_count_is_bounded(lib, fn):
    for S in (0, -1, 1025):
        _refused(lib, fn, _with(fn, **{f'a{FEEDS_AT[fn]}': S}), f'S = {S} feeds outside 1..1024')


def test_bank_push_refuses_what_does_not_fit(lib):
    fn = 'tamgcn_bank_push'
    _refused(lib, fn, _with(fn, a2=17), 'n = 17 frames outside 1..cap = 16')
    _refused(lib, fn, _with(fn, a2=0), 'n = 0')
    for elem in (0, 2, 16, -4):
        _refused(lib, fn, _with(fn, a5=elem), f'elem {elem}')
    _refused(lib, fn, _with(fn, a3=0), 'bad dims P=0 R=60 cap=16')
    _refused(lib, fn, _with(fn, a4=0), 'bad dims')
    _refused(lib, fn, _with(fn, a7=0), 'bad dims')
    _refused(lib, fn, _with(fn, a4=2 ** 30), 'too large')


def test_bank_plan_refuses_an_empty_or_oversized_window(lib):
    fn = 'tamgcn_bank_plan'
    _refused(lib, fn, _with(fn, a5=0), 'window L = 0 outside 1..cap = 16')
    _refused(lib, fn, _with(fn, a5=17), 'window L = 17')
    _refused(lib, fn, _with(fn, a6=0), 'bad dims cap=16 B=2 hop=0')
    _refused(lib, fn, _with(fn, a4=0), 'bad dims')
    _refused(lib, fn, _with(fn, a3=0), 'bad dims')
    _refused(lib, fn, _with(fn, a4=2 ** 30), 'windows')


def test_bank_windows_refuse_their_limits(lib):
    fn = 'tamgcn_bank_window_nucla'
    _refused(lib, fn, _with(fn, a7=65), 'time_steps 65 outside 1..64')
    _refused(lib, fn, _with(fn, a7=0), 'time_steps 0')
    _refused(lib, fn, _with(fn, a8=20), 'centre joint 20 outside 0..19')
    _refused(lib, fn, _with(fn, a9=4), 'mode 4')
    _refused(lib, fn, _with(fn, a4=0), 'bad dims cap=16 B=0 V=20')
    _refused(lib, fn, _with(fn, a2=0), 'bad dims')
    fn = 'tamgcn_bank_window_clip'
    for i in (2, 4, 5, 6, 7, 8):
        _refused(lib, fn, _with(fn, **{f'a{i}': 0}), 'bad dims')
    _refused(lib, fn, _with(fn, a2=2 ** 30, a6=4), 'channel plane above 2^30')


def test_bank_scores_refuse_their_limits(lib):
    fn = 'tamgcn_bank_ema'
    _refused(lib, fn, _with(fn, a5=4097), 'K = 4097 outside 1..4096')
    _refused(lib, fn, _with(fn, a5=0), 'K = 0')
    _refused(lib, fn, _with(fn, a4=0), 'B = 0')
    for beta in (1.0, -0.1, float('nan')):
        _refused(lib, fn, _with(fn, a6=beta), 'beta')
    fn = 'tamgcn_bank_decide'
    _refused(lib, fn, _with(fn, a6=float('nan')), 'threshold is NaN')
    _refused(lib, fn, _with(fn, a7=0), 'hold = 0')
    _refused(lib, fn, _with(fn, a12=0), 'log_capacity = 0')


class _Net(torch.nn.Module):
    """Stands in for a model: the constructors look at its mode and its joint count before anything else."""
    num_point = 20

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_ring_bank_refuses_bad_arguments_before_any_allocation():
    from tam_gcn_amd.streaming import RingBank
    for kw in (dict(feeds=0, capacity=16, V=20), dict(feeds=1025, capacity=16, V=20), dict(feeds=True, capacity=16, V=20),
               dict(feeds=2.0, capacity=16, V=20), dict(feeds=3, capacity=0, V=20), dict(feeds=3, capacity=16), dict(feeds=3, capacity=16, V=0),
               dict(feeds=3, capacity=16, V=20, prep='ntu'), dict(feeds=3, capacity=16, V=20, prep='nucla', M=2),
               dict(feeds=3, capacity=16, V=20, prep='nucla', C=2), dict(feeds=3, capacity=16, V=20, prep='clip', C=0),
               dict(feeds=3, capacity=16, V=20, device='cpu')):
        with pytest.raises(ValueError, match='RingBank'):
            RingBank(**kw)


def test_live_bank_refuses_bad_arguments_before_any_launch():
    from tam_gcn_amd.streaming import FrameRing, LiveBank, RingBank
    net = _Net().eval()

    class Bank(RingBank):                            # the geometry of a bank without its device tensors
        def __init__(self, capacity, feeds=3, prep='nucla', V=20, C=3, M=1):
            self.feeds, self.capacity, self.prep, self.V, self.C, self.M = feeds, capacity, prep, V, C, M

    class Ring(FrameRing):
        def __init__(self):
            pass
    with pytest.raises(ValueError, match='must be a RingBank'):
        LiveBank(net, Ring(), window=20)
    for kw in (dict(window=0), dict(window=20, hop_windows=0), dict(window=20, hop=0), dict(window=20, beta=1.0), dict(window=20, beta=-0.5),
               dict(window=20, beta='x'), dict(window=20, frames_per_step=0), dict(window=20, frames_per_step=65),
               dict(window=65), dict(window=20, hop_windows=4, hop=15),                      # 20 + 3 * 15 = 65 > 64
               dict(window=20, stream='velocity'), dict(window=20, time_steps=65), dict(window=20, window_size=64),
               dict(window=20, chunk_windows=0), dict(window=20, threshold='x'), dict(window=20, threshold=float('nan')),
               dict(window=20, threshold=0.6, hold=0), dict(window=20, hold=1.5), dict(window=20, log_capacity=0)):
        with pytest.raises(ValueError, match='LiveBank'):
            LiveBank(net, Bank(64), **kw)
    with pytest.raises(ValueError, match='joints'):
        LiveBank(net, Bank(64, V=17), window=20)
    with pytest.raises(ValueError, match='eval'):
        LiveBank(_Net().train(), Bank(64), window=20)
    with pytest.raises(ValueError, match='window_size'):
        LiveBank(net, Bank(64, prep='clip'), window=20)
