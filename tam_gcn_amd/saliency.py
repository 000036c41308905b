"""Input-gradient saliency of a trained model in eval() mode (reference tools/train_stgcn_group.py:264-356: back-propagate the
true-class score to the input, sum the gradient's magnitude per joint, average over body parts per class).

    g = input_gradient(model, x, labels)          # d sum_n logits[n, labels[n]] / d x, x's shape; labels=None: the arg-max class
    g = input_gradient(model, x, dlogits=w)       # any linear functional sum(w * logits) of the logits, w (N, K)
    s = joint_saliency(model, x, labels)          # (N, V) = |g| summed over channels, frames and persons

    imp = PartImportance(model, num_class)        # body parts: the reference's five N-UCLA groups, or parts={name: [joints]}
    for x, y in loader:
        imp.update(x, y)                          # no host synchronisation
    weights = imp.compute()                       # {class: {part: weight}}, the largest part of a class at 1;  imp.to_json(path)

Routing.  An ST-GCN model (models.stgcn.Model) the f2s kernel family supports, fp32 on the device, without forward hooks, with
the family enabled (TAMGCN_F2) and at most f2s.F2S_BWD_MAX_FRAMES clip-persons x frames (N * M * T) takes the family: the
forward's two launches per block, then two launches per block backwards (csrc/f2s_bwd.hip) that compute the DATA gradient
only, and one reduction launch -- no autograd graph, no weight gradients.  Everything else (larger inputs, CTR-GCN models,
geometry outside the family) takes the general path: torch.autograd.grad of the seeded logits with respect to a detached copy
of x.  Neither route touches a parameter's .grad.  There is no CPU path."""
import json

import torch

from . import _lib
from . import f2s

__all__ = ['input_gradient', 'joint_saliency', 'PartImportance', 'UCLA_PARTS']

# the 20 N-UCLA joints by limb, the grouping of the reference's analysis: neck and head, shoulder to hand, hip to foot
UCLA_PARTS = {'head': (2, 3), 'l_hand': (4, 5, 6, 7), 'r_hand': (8, 9, 10, 11), 'l_leg': (12, 13, 14, 15), 'r_leg': (16, 17, 18, 19)}


def _check(model, x, labels, dlogits):
    if model.training:
        raise ValueError('saliency: put the model in eval() mode first')
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError('tam_gcn_amd: expected a HIP (cuda) tensor; there is no CPU path')
    if x.dim() not in (3, 5):
        raise ValueError(f'saliency: expected x (N, C, T, V, M) or (N, T, V*C), got {tuple(x.shape)}')
    if labels is not None and dlogits is not None:
        raise ValueError('saliency: give labels or dlogits, not both')


def _as5(model, x):
    if x.dim() == 5:
        return x
    N, T, VC = x.shape
    return x.view(N, T, model.num_point, -1).permute(0, 3, 1, 2).contiguous().unsqueeze(-1)


def _engine(model, x):
    """The f2s engine if this call is one for the family, else None."""
    if not hasattr(model, 'st_gcn_networks') or not hasattr(model, '_small_batch_engine') or x.dtype != torch.float32:
        return None
    frames = x.shape[0] * x.shape[4] * x.shape[2] if x.dim() == 5 else x.shape[0] * x.shape[1]
    if not f2s.enabled() or frames > f2s.F2S_BWD_MAX_FRAMES:
        return None
    return model._small_batch_engine(x, '_tamgcn_f2s', f2s.FusedEvalST)


def _general(model, x, labels, dlogits):
    """autograd through Model.forward: the gradient of sum(seed * logits) with respect to x alone"""
    xd = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        logits = model(xd)
        if dlogits is None:
            lab = logits.detach().argmax(1) if labels is None else labels.to(device=x.device, dtype=torch.int64).view(-1)
            dlogits = torch.zeros_like(logits).scatter_(1, lab.view(-1, 1), 1.0)
        elif tuple(dlogits.shape) != tuple(logits.shape):
            raise ValueError(f'dlogits must be {tuple(logits.shape)}, got {tuple(dlogits.shape)}')
        (g,) = torch.autograd.grad(logits, xd, dlogits.to(device=x.device, dtype=logits.dtype))
    return g


def input_gradient(model, x, labels=None, dlogits=None, trace=None):
    """The gradient of sum(seed * model(x)) with respect to x, in x's shape.  seed: dlogits (N, K), else one-hot of labels (N),
    else one-hot of the arg-max class (taken on the device).  trace: a list that receives, per block, dict(gout, out, h, dx) when
    the family serves the call (it stays empty on the general path)."""
    _check(model, x, labels, dlogits)
    eng = _engine(model, x)
    if eng is None:
        return _general(model, x, labels, dlogits)
    _, g, _ = eng.saliency_pass(_as5(model, x), labels, dlogits, trace)
    if x.dim() == 3:
        g = g[..., 0].permute(0, 2, 3, 1).reshape(x.shape)
    return g


def joint_saliency(model, x, labels=None):
    """(N, V): |input_gradient| summed over channels, frames and persons (reference :309)."""
    _check(model, x, labels, None)
    eng = _engine(model, x)
    if eng is not None:
        return eng.saliency_pass(_as5(model, x), labels, None, None, want_dxin=False)[0]
    g = _as5(model, _general(model, x, labels, None))
    return g.abs().sum((1, 2, 4))


class PartImportance:
    """Per-class body-part importance from joint saliency, accumulated on the device (reference :280-346).  Samples count in
    batch order until their class holds `per_class` of them; a sample's part value is the mean of its joints' saliency; a
    class's value is the mean over its counted samples, divided by the class's largest part value (by 1 when that is 0); a class
    without a sample gives 0.  `update` never synchronises with the host; `compute` does, once."""

    def __init__(self, model, num_class, parts=None, per_class=200):
        V = int(getattr(model, 'num_point', 0))
        if parts is None:
            if V != 20:
                raise ValueError(f'PartImportance: the default body parts are those of the 20-joint N-UCLA skeleton; a model of {V} joints needs parts=')
            parts = UCLA_PARTS
        self.names = list(parts)
        self.parts = [[int(j) for j in parts[k]] for k in self.names]
        if not self.parts or len(self.parts) > 256:
            raise ValueError('PartImportance: 1 .. 256 parts')
        for k, js in zip(self.names, self.parts):
            if not js or any(not 0 <= j < V for j in js):
                raise ValueError(f'PartImportance: part {k!r} needs joints inside [0, {V})')
        self.model, self.num_class, self.per_class, self.V = model, int(num_class), int(per_class), V
        self._dev = None

    def _state(self, dev):
        if self._dev is None:
            off = [0]
            for js in self.parts:
                off.append(off[-1] + len(js))
            self._off = torch.tensor(off, dtype=torch.int32, device=dev)
            self._joints = torch.tensor([j for js in self.parts for j in js], dtype=torch.int32, device=dev)
            self.count = torch.zeros(self.num_class, dtype=torch.int32, device=dev)
            self.sum = torch.zeros(self.num_class, len(self.parts), dtype=torch.float64, device=dev)
            self._dev = dev
        elif dev != self._dev:
            raise RuntimeError(f'PartImportance: state lives on {self._dev}, batch on {dev}')

    def reset(self):
        if self._dev is not None:
            self.count.zero_()
            self.sum.zero_()

    def update(self, x, labels):
        sal = joint_saliency(self.model, x, labels)
        return self.update_saliency(sal, labels)

    def update_saliency(self, sal, labels):
        """Add a batch whose (N, V) joint saliency is already known."""
        import ctypes as C
        if not sal.is_cuda:
            raise RuntimeError('tam_gcn_amd: expected a HIP (cuda) tensor; there is no CPU path')
        self._state(sal.device)
        sal = sal.detach().to(torch.float32).contiguous()
        N, V = sal.shape
        if V != self.V:
            raise ValueError(f'PartImportance: saliency of {V} joints, the model has {self.V}')
        lab = labels.to(device=sal.device, dtype=torch.int64).contiguous().view(N)
        lib = _lib.load()
        st = C.c_void_p(torch.cuda.current_stream(sal.device).cuda_stream)
        for i in range(0, N, 4096):                                           # the entry point takes 4096 samples a call
            n = min(4096, N - i)
            _lib.check(lib.tamgcn_saliency_accumulate(sal[i:i + n].data_ptr(), lab[i:i + n].data_ptr(), n, V, self._off.data_ptr(),
                                                      self._joints.data_ptr(), len(self.parts), self.num_class, self.per_class,
                                                      self.count.data_ptr(), self.sum.data_ptr(), st), 'tamgcn_saliency_accumulate')
        return self

    def compute(self):
        """{class index: {part name: weight}}; the only synchronisation"""
        if self._dev is None:
            return {k: {p: 0.0 for p in self.names} for k in range(self.num_class)}
        count, total = self.count.cpu().tolist(), self.sum.cpu().tolist()
        res = {}
        for k in range(self.num_class):
            mean = [v / count[k] if count[k] else 0.0 for v in total[k]]
            top = max(mean)
            if top == 0:
                top = 1.0
            res[k] = {p: v / top for p, v in zip(self.names, mean)}
        return res

    def to_json(self, path):
        res = self.compute()
        with open(path, 'w') as f:
            json.dump({str(k): v for k, v in res.items()}, f, indent=2)
        return res
