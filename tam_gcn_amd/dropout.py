"""Device dropout for training: a counter-based mask drawn, applied and remembered inside the kernels (include/tamgcn.h,
tamgcn_drop_add_act_fwd has the draw; DESIGN.md "Device dropout").

    stream = dropout.enable(model, seed=1234)       # opt-in: a model nobody enabled keeps torch's nn.Dropout path
    ...train: eager steps or a CapturedStep...
    ckpt['dropout'] = stream.state_dict()           # (seed, call): resuming replays the same masks

The state is an int64 [2] tensor (seed, call) on the device, read there by every kernel that draws, so a captured graph sees
its current value; ``call`` advances once per training forward, in a one-thread launch after the last site.  It is NOT a
registered buffer: the state-dict keys of the models stay those of the reference.  Nothing here installs a forward hook (the
small-batch eval families step aside for hooked models): the modules look their stream and site up as plain attributes."""
import torch

from . import ops

_STREAM, _SITE = '_tamgcn_drop_stream', '_tamgcn_drop_site'


class DropoutStream:
    """The (seed, call) state of the masks of one model, on ``device``."""

    def __init__(self, seed, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('tam_gcn_amd: the dropout stream lives on a HIP (cuda) device; there is no CPU path')
        self._state = torch.tensor([_i64(seed), 0], dtype=torch.int64, device=device)

    @property
    def tensor(self):
        """The int64 [2] device tensor the kernels read."""
        return self._state

    def advance(self):
        """call += 1 on the device, in stream order (capturable)."""
        ops.dropout_advance(self._state)

    def state(self):
        """(seed, call) as Python ints; synchronises."""
        s, c = self._state.tolist()
        return s & (2 ** 64 - 1), c & (2 ** 64 - 1)

    def set_state(self, seed, call):
        self._state.copy_(torch.tensor([_i64(seed), _i64(call)], dtype=torch.int64), non_blocking=False)

    def state_dict(self):
        seed, call = self.state()
        return {'seed': seed, 'call': call}

    def load_state_dict(self, sd):
        self.set_state(sd['seed'], sd['call'])


def _i64(v):
    """An unsigned 64-bit value as the int64 with the same bits."""
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _sites(module):
    """The modules that draw, in module order: every st_gcn with dropout > 0, then every model head with a Dropout."""
    from .models import ctrgcn, stgcn
    blocks = [m for m in module.modules() if isinstance(m, stgcn.st_gcn) and m._dropout and 0 < m._dropout < 1]
    heads = [m for m in module.modules() if isinstance(m, (ctrgcn.Model, stgcn.Model)) and isinstance(m.drop_out, torch.nn.Dropout)
             and 0 < m.drop_out.p < 1]
    return blocks + heads


def _models(module):
    from .models import ctrgcn, stgcn
    return [m for m in module.modules() if isinstance(m, (ctrgcn.Model, stgcn.Model))]


def enable(module, seed=None):
    """Route the dropout of every st_gcn block (dropout > 0) and model head under ``module`` to the device path and return
    their common DropoutStream.  seed None: torch.initial_seed()."""
    sites = _sites(module)
    if not sites:
        raise ValueError('tam_gcn_amd.dropout.enable: no st_gcn block or model head with 0 < dropout < 1 under this module')
    if len(sites) > ops.DROP_MAX_SITES:
        raise ValueError(f'tam_gcn_amd.dropout.enable: {len(sites)} sites, at most {ops.DROP_MAX_SITES} share a stream')
    dev = next((p.device for p in module.parameters()), None)
    if dev is None:
        raise ValueError('tam_gcn_amd.dropout.enable: the module has no parameters to take the device from')
    stream = DropoutStream(torch.initial_seed() if seed is None else seed, dev)
    disable(module)
    for i, m in enumerate(sites):
        m.__dict__[_STREAM], m.__dict__[_SITE] = stream, i
    for m in _models(module):               # a model advances the stream after its last site, whether or not its head draws
        m.__dict__[_STREAM] = stream
    module.__dict__[_STREAM] = stream
    return stream


def disable(module):
    """Back to torch's nn.Dropout everywhere under ``module``."""
    for m in module.modules():
        m.__dict__.pop(_STREAM, None)
        m.__dict__.pop(_SITE, None)


def stream_of(module):
    """The DropoutStream attached to this very module by enable(), or None."""
    return module.__dict__.get(_STREAM)


def site_of(module):
    return module.__dict__.get(_SITE)


def streams_under(module):
    """Every distinct DropoutStream attached to ``module`` or a sub-module."""
    out = []
    for m in module.modules():
        s = m.__dict__.get(_STREAM)
        if s is not None and all(s is not o for o in out):
            out.append(s)
    return out
