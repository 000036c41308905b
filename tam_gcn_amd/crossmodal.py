"""The cross-modal attention model of the reference (models/resnet_gcn_attention.py) with its own layers on the device.

    head  = CrossModalHead(num_class=10, gcn_dim=256, rgb_dim=2048)
    logits = head(f_gcn, f_rgb)                   # f_gcn (N, gcn_dim), f_rgb (N, rgb_dim, H, W) -> (N, num_class)

    model = ResNet_GCN_Attention(gcn, resnet, num_class=10)      # gcn: models.ctrgcn.Model, resnet: x_rgb -> (N, rgb_dim, H, W)
    logits = model(x_gcn, x_rgb)

The head is reference lines 89-120: attention_transform (Linear -> BatchNorm1d -> ReLU -> Linear -> Sigmoid) turns the pooled
skeleton feature into rgb_dim channel gates, the gates scale the image map, the map is average-pooled and classified.  Here that
is three HIP launches and the classifier GEMM forward, four (five when d f_gcn is wanted) and the classifier's backward
(csrc/xmodal/, include/tamgcn_xmodal.h): since pool(f_rgb * att) = att * pool(f_rgb) and d f_rgb = d pooled * att / (H W)
broadcast, the gated copy of the map the reference writes and reads in both directions never exists.  Train and eval mode of the
BatchNorm1d are both on the device, running statistics and num_batches_tracked included; nothing synchronises with the host and
a forward + backward can be captured by torch.cuda.graph.  Parameter names, shapes and default initialisation are the
reference's, so its checkpoints load with load_state_dict.  There is no CPU path and no fallback to torch.

The ResNet trunk stays the user's torch module (INTEGRATION.md shows the reference's conv1 inflation); the skeleton feature comes
from guidance.pooled_feature when the CTR-GCN is frozen (the reference's configuration) and through autograd otherwise."""
import torch
import torch.nn as nn

from . import guidance
from . import torch_ops
from .models.ctrgcn import _require_hip

__all__ = ['CrossModalHead', 'ResNet_GCN_Attention']


def _build_layers(num_class, gcn_dim, rgb_dim):
    if gcn_dim % 4 or rgb_dim % 8 or gcn_dim < 4 or rgb_dim < 8:
        raise ValueError(f'cross-modal head: gcn_dim = {gcn_dim} must be a positive multiple of 4 and rgb_dim = {rgb_dim} of 8 '
                         '(the hidden width rgb_dim // 2 must be a multiple of 4)')
    if num_class < 1:
        raise ValueError(f'cross-modal head: num_class = {num_class} must be at least 1')
    attention_transform = nn.Sequential(                    # reference :60-66
        nn.Linear(gcn_dim, rgb_dim // 2),
        nn.BatchNorm1d(rgb_dim // 2),
        nn.ReLU(inplace=True),
        nn.Linear(rgb_dim // 2, rgb_dim),
        nn.Sigmoid())
    return attention_transform, nn.Linear(rgb_dim, num_class)


def _run_head(attention_transform, classifier, training, f_gcn, f_rgb):
    if not isinstance(f_gcn, torch.Tensor) or not isinstance(f_rgb, torch.Tensor):
        raise TypeError('cross-modal head: f_gcn and f_rgb must be tensors')
    f_gcn, f_rgb = _require_hip(f_gcn), _require_hip(f_rgb)
    fc1, bn, _, fc2, _ = attention_transform
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise ValueError('cross-modal head: the BatchNorm1d must be affine and track running statistics with a numeric momentum '
                         '(the reference\'s nn.BatchNorm1d defaults)')
    if not fc1.weight.is_cuda:
        raise RuntimeError('cross-modal head: the module is on the CPU; move it to the HIP device (there is no CPU path)')
    return torch_ops.XModalHeadFn.apply(f_gcn, f_rgb, fc1.weight, fc1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                        bn.num_batches_tracked, fc2.weight, fc2.bias, classifier.weight, classifier.bias,
                                        bool(training and bn.training), float(bn.momentum), float(bn.eps))


class CrossModalHead(nn.Module):
    """attention_transform and classifier of the reference model; forward(f_gcn (N, gcn_dim), f_rgb (N, rgb_dim, H, W)) -> logits.
    1 <= N <= 1024 in eval mode, 2 <= N in train mode (N = 1 raises torch's own BatchNorm error)."""

    def __init__(self, num_class=10, gcn_dim=256, rgb_dim=2048):
        super().__init__()
        self.attention_transform, self.classifier = _build_layers(num_class, gcn_dim, rgb_dim)

    def forward(self, f_gcn, f_rgb):
        return _run_head(self.attention_transform, self.classifier, self.training, f_gcn, f_rgb)


class ResNet_GCN_Attention(nn.Module):
    """The reference's model around a tam_gcn_amd CTR-GCN and the caller's image trunk.  `resnet` is any module that maps x_rgb to
    the (N, rgb_dim, H, W) fp32 map (ResNet-50 up to layer4 in the reference).  Attributes gcn, resnet, attention_transform and
    classifier are the reference's, so are the state-dict keys."""

    def __init__(self, gcn, resnet, num_class=10, gcn_dim=256, rgb_dim=2048, freeze_gcn=True):
        super().__init__()
        if not hasattr(gcn, '_block_stack') or not hasattr(gcn, 'extract_feature'):
            raise TypeError(f'ResNet_GCN_Attention: {type(gcn).__name__} is no tam_gcn_amd.models.ctrgcn.Model')
        self.gcn = gcn
        if freeze_gcn:                                          # reference :24-26
            for param in self.gcn.parameters():
                param.requires_grad = False
        self.resnet = resnet
        self.attention_transform, self.classifier = _build_layers(num_class, gcn_dim, rgb_dim)

    def forward(self, x_gcn, x_rgb):
        if any(p.requires_grad for p in self.gcn.parameters()):
            f_gcn = self.gcn.extract_feature(x_gcn)[0].mean((2, 3, 4))          # reference :82-85, through autograd
        else:
            f_gcn = guidance.pooled_feature(self.gcn, x_gcn)                     # the same numbers, host-free, no autograd
        f_rgb = self.resnet(x_rgb)
        return _run_head(self.attention_transform, self.classifier, self.training, f_gcn, f_rgb)
