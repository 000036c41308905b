"""-m gpu: tam_gcn_amd.crossmodal end to end.  CrossModalHead against the fp64 restatement (tests/crossmodal_ref.py) in train and
eval mode: logits, every gradient, the BatchNorm1d buffers.  ResNet_GCN_Attention with a frozen and an unfrozen CTR-GCN against
the same composition with torch's own head on the device.  Capture by torch.cuda.graph, opcheck of the two operators, the
reference's state-dict keys, the refusals.

End-to-end bar.  Nothing is teacher-forced here, so a result carries the rounding of every stage before it.  Each stage is a sum of
L terms with relative error <= (L + 4) 2^-24 of its magnitude (fp64_bars); to first order the relative errors of the stages on the
path add, forward D, N (statistics), Hd, P, R and backward R, N, R, N, Hd:
    max |got - ref| <= (sum of (L + 4) over those ten stages) * 2^-24 * scale
with scale = max |ref| of the tensor -- except db1, whose reference is rounding noise around 0 in train mode (the batch formula
centres dz1) and whose scale is the largest column sum of |dz1|.  ReLUs: a hidden unit whose fp64 pre-activation lies within its own
rounding bar of 0 may take either side on the device.  The seeds of crossmodal_ref.E2E_CASES keep those units under 1 % of the
hidden activations (asserted on the reference before a device result is looked at, and in tests/test_crossmodal_ref_cpu.py without
a GPU).  The fused operator offers no way to mask a unit on the device, so instead of leaving those units out of both sides the
reference's backward takes the device's side on exactly them: their contributions stay in the comparison, and a device ReLU that
differs from the reference anywhere else fails it."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import crossmodal_ref as R                                              # noqa: E402
from tam_gcn_amd import torch_ops                                       # noqa: E402,F401
from tam_gcn_amd.crossmodal import CrossModalHead, ResNet_GCN_Attention   # noqa: E402
from tam_gcn_amd.models.ctrgcn import Model                             # noqa: E402

DEV = 'cuda:0'
UCLA = dict(num_class=10, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))


def make_head(shape, p):
    N, D, Hd, Rr, P, K = shape
    assert Rr == 2 * Hd
    head = CrossModalHead(num_class=K, gcn_dim=D, rgb_dim=Rr)
    at, cl = head.attention_transform, head.classifier
    with torch.no_grad():
        for dst, k in ((at[0].weight, 'W1'), (at[0].bias, 'b1'), (at[1].weight, 'gamma'), (at[1].bias, 'beta'), (at[1].running_mean, 'rmean'),
                       (at[1].running_var, 'rvar'), (at[1].num_batches_tracked, 'nbt'), (at[3].weight, 'W2'), (at[3].bias, 'b2'),
                       (cl.weight, 'Wc'), (cl.bias, 'bc')):
            dst.copy_(p[k])
    return head.to(DEV)


def head_results(head, f, f_rgb, dlogits):
    f, f_rgb = f.to(DEV).requires_grad_(True), f_rgb.to(DEV).requires_grad_(True)
    head.zero_grad(set_to_none=True)
    out = head(f, f_rgb)
    out.backward(dlogits.to(DEV))
    at, cl = head.attention_transform, head.classifier
    return dict(logits=out.detach(), df=f.grad, df_rgb=f_rgb.grad, dW1=at[0].weight.grad, db1=at[0].bias.grad, dgamma=at[1].weight.grad,
                dbeta=at[1].bias.grad, dW2=at[3].weight.grad, db2=at[3].bias.grad, dWc=cl.weight.grad, dbc=cl.bias.grad,
                running_mean=at[1].running_mean, running_var=at[1].running_var, num_batches_tracked=at[1].num_batches_tracked)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('shape,seed', R.E2E_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f's{v}')
def test_head_against_the_fp64_restatement(shape, seed, training):
    N, D, Hd, Rr, P, K = shape
    p, f, f_rgb, dl = R.make_problem(shape, seed)
    f_rgb = f_rgb.reshape(N, Rr, 7, 7)
    ref = R.head(p, f, f_rgb, dl, training)
    near = R.relu_margin_mask(ref['pre'], ref['pre_bar'])
    assert float(near.double().mean()) <= R.RELU_CAP
    head = make_head(shape, p).train(training)
    probe = copy.deepcopy(head)                                 # the device's own ReLU sides: a1 of the operator, on buffers of its own
    at, cl = probe.attention_transform, probe.classifier
    a1 = torch.ops.tamgcn.xmodal_head(f.to(DEV), f_rgb.to(DEV), at[0].weight, at[0].bias, at[1].weight, at[1].bias, at[1].running_mean,
                                      at[1].running_var, at[1].num_batches_tracked, at[3].weight, at[3].bias, cl.weight, cl.bias, training,
                                      0.1, 1e-5)[4]
    side = (a1 > 0).cpu()
    assert torch.equal(side | near, (ref['pre'] > 0) | near), 'a device ReLU differs from the reference outside the rounding bar'
    ref = R.head(p, f, f_rgb, dl, training, relu_side=side)
    got = head_results(head, f, f_rgb, dl)
    bar = sum(L + 4 for L in (D, N, Hd, P, Rr, Rr, N, Rr, N, Hd)) * R.U
    assert int(got['num_batches_tracked']) == ref['num_batches_tracked'] == 3 + int(training)
    line = []
    for k, g in got.items():
        if k == 'num_batches_tracked':
            continue
        r = ref[k]
        scale = float(ref['db1_mag'].max()) if k == 'db1' else float(r.abs().max())
        err = float((g.double().cpu() - r).abs().max())
        line.append(f'{k} {err / scale:.2e}')
        assert tuple(g.shape) == tuple(r.shape) and err <= bar * scale, (k, err, bar * scale)
    print(f'\nxmodal_e2e {"x".join(map(str, shape))} {"train" if training else "eval"} (bar {bar:.2e}): ' + ' '.join(line))


class TorchComposition(nn.Module):
    """the reference's forward (models/resnet_gcn_attention.py:82-120) over the same sub-modules with torch's own layers"""

    def __init__(self, model):
        super().__init__()
        self.m = model

    def forward(self, x_gcn, x_rgb):
        m = self.m
        f_gcn = m.gcn.extract_feature(x_gcn)[0].mean(dim=(2, 3, 4))
        att = m.attention_transform(f_gcn).unsqueeze(-1).unsqueeze(-1)
        out = nn.functional.adaptive_avg_pool2d(m.resnet(x_rgb) * att, (1, 1))
        return m.classifier(torch.flatten(out, 1))


def small_trunk(rgb_dim):
    return nn.Sequential(nn.Conv2d(15, 32, 3, stride=2, padding=1), nn.ReLU(), nn.Conv2d(32, rgb_dim, 3, stride=2, padding=1))


@pytest.mark.parametrize('freeze', [True, False], ids=['frozen', 'unfrozen'])
def test_model_against_the_torch_composition(freeze):
    """fp32 against fp32 on the device: the two differ by the rounding of the head alone (its sums are at most rgb_dim = 64 terms
    here), so logits, head and trunk gradients agree to 1e-4 of their largest entry; the CTR-GCN's gradients pass d f through ten
    blocks whose ReLUs may flip on a last-bit difference and are held in relative L2 to 1e-3, as tests/test_gpu_model.py holds
    deep gradients."""
    torch.manual_seed(7)
    model = ResNet_GCN_Attention(Model(**UCLA), small_trunk(64), num_class=10, gcn_dim=256, rgb_dim=64, freeze_gcn=freeze).to(DEV).train()
    assert all(p.requires_grad != freeze for p in model.gcn.parameters())
    twin = TorchComposition(copy.deepcopy(model)).train()
    gen = torch.Generator().manual_seed(8)
    x_gcn = torch.randn(4, 3, 16, 20, 1, generator=gen).to(DEV)
    x_rgb = torch.randn(4, 15, 28, 28, generator=gen).to(DEV)
    lab = torch.tensor([1, 4, 7, 2], device=DEV)
    outs = []
    for net in (model, twin):
        out = net(x_gcn, x_rgb)
        nn.functional.cross_entropy(out, lab).backward()
        outs.append(out.detach())
    assert outs[0].shape == (4, 10)

    def rel(a, b):
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    assert rel(outs[0], outs[1]) <= 1e-4
    mine, theirs = dict(model.named_parameters()), dict(twin.m.named_parameters())
    noise_floor = 1e-6 * max(float(q.grad.norm()) for q in theirs.values() if q.grad is not None)   # fp32: 2^-24 of the sums behind it
    for k, q in theirs.items():
        if k.startswith('gcn.'):
            if freeze:
                assert mine[k].grad is None and q.grad is None, k
            elif q.grad is not None and float(q.grad.norm()) <= noise_floor:      # a bias in front of a train-mode BatchNorm: its
                assert float(mine[k].grad.norm()) <= noise_floor, k               # gradient is rounding noise around 0 in both
            elif q.grad is not None:
                assert float((mine[k].grad - q.grad).norm() / q.grad.norm()) <= 1e-3, k
        else:
            assert mine[k].grad is not None and float(mine[k].grad.abs().max()) > 0, k          # gradients reach the trunk and the head
            if k == 'attention_transform.0.bias':            # train-mode BatchNorm centres dz1: both are rounding noise around 0,
                noise = 1e-4 * float(theirs['attention_transform.0.weight'].grad.abs().max())      # held to the scale of dW1
                assert float(mine[k].grad.abs().max()) <= noise and float(q.grad.abs().max()) <= noise, k
                continue
            assert rel(mine[k].grad, q.grad) <= 1e-4, (k, rel(mine[k].grad, q.grad))
    if not freeze:
        assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.gcn.parameters())
    for k, b in twin.m.named_buffers():
        if k.startswith('attention_transform'):
            a = dict(model.named_buffers())[k]
            assert torch.equal(a, b) if a.dtype == torch.int64 else rel(a, b) <= 1e-5, k
    model.eval()
    twin.eval()
    with torch.no_grad():
        assert rel(model(x_gcn[:1], x_rgb[:1]), twin(x_gcn[:1], x_rgb[:1])) <= 1e-4           # one clip, eval


def test_forward_and_backward_are_captured_and_replayed():
    shape = (17, 64, 36, 72, 49, 10)
    p, f, f_rgb, dl = R.make_problem(shape, 41)
    head = make_head(shape, p).train()
    sf, srgb, sdl = (torch.zeros_like(t, device=DEV) for t in (f, f_rgb.reshape(17, 72, 7, 7), dl))
    srgb.requires_grad_(True)
    sf.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            head.zero_grad(set_to_none=True)
            sf.grad = srgb.grad = None
            head(sf, srgb).backward(sdl)
    torch.cuda.current_stream().wait_stream(side)
    head.zero_grad(set_to_none=True)
    sf.grad = srgb.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # a host synchronisation or a host copy inside would end the capture
        out = head(sf, srgb)
        out.backward(sdl)
    for step in range(2):
        pp, ff, rr, dd = R.make_problem(shape, 50 + step)
        eager = copy.deepcopy(head)                             # the buffers as they are before this replay
        with torch.no_grad():
            sf.copy_(ff)
            srgb.copy_(rr.reshape(17, 72, 7, 7))
            sdl.copy_(dd)
        before = int(head.attention_transform[1].num_batches_tracked)
        graph.replay()
        torch.cuda.synchronize()
        assert int(head.attention_transform[1].num_batches_tracked) == before + 1
        torch.cuda.set_sync_debug_mode('error')                 # the eager call itself must not synchronise either
        try:
            want = head_results(eager, sf.detach().clone(), srgb.detach().clone(), sdl)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        at, cl = head.attention_transform, head.classifier
        got = dict(logits=out, df=sf.grad, df_rgb=srgb.grad, dW1=at[0].weight.grad, db1=at[0].bias.grad, dgamma=at[1].weight.grad,
                   dbeta=at[1].bias.grad, dW2=at[3].weight.grad, db2=at[3].bias.grad, dWc=cl.weight.grad, dbc=cl.bias.grad,
                   running_mean=at[1].running_mean, running_var=at[1].running_var, num_batches_tracked=at[1].num_batches_tracked)
        for k in want:
            assert torch.equal(got[k], want[k]), f'replay {step}: {k} differs from the eager call'


def test_opcheck_of_the_two_operators():
    shape = (2, 4, 4, 8, 1, 2)
    p, f, f_rgb, dl = R.make_problem(shape, 61)
    d = {k: v.to(DEV) for k, v in p.items()}
    f, f_rgb, dl = f.to(DEV), f_rgb.to(DEV), dl.to(DEV)
    args = (f, f_rgb, d['W1'], d['b1'], d['gamma'], d['beta'], d['rmean'], d['rvar'], d['nbt'], d['W2'], d['b2'], d['Wc'], d['bc'], True, 0.1, 1e-5)
    torch.library.opcheck(torch.ops.tamgcn.xmodal_head, args)
    logits, g, att, m, a1, xhat, invstd = torch.ops.tamgcn.xmodal_head(*args)
    assert int(d['nbt']) >= 4 and logits.shape == (2, 2)
    bargs = (dl, f, d['W1'], d['gamma'], d['W2'], d['Wc'], g, att, m, a1, xhat, invstd, 1, 1, True, True, True)
    torch.library.opcheck(torch.ops.tamgcn.xmodal_head_backward, bargs)
    grads = torch.ops.tamgcn.xmodal_head_backward(*bargs[:-2], False, False)
    assert grads[0].numel() == 0 and grads[1].numel() == 0 and grads[2].shape == d['W1'].shape


def test_state_dict_with_the_reference_key_names():
    model = ResNet_GCN_Attention(Model(**UCLA), small_trunk(64), num_class=10, gcn_dim=256, rgb_dim=64)
    head_keys = {'attention_transform.0.weight', 'attention_transform.0.bias', 'attention_transform.1.weight', 'attention_transform.1.bias',
                 'attention_transform.1.running_mean', 'attention_transform.1.running_var', 'attention_transform.1.num_batches_tracked',
                 'attention_transform.3.weight', 'attention_transform.3.bias', 'classifier.weight', 'classifier.bias'}
    sd = model.state_dict()
    assert {k for k in sd if not k.startswith(('gcn.', 'resnet.'))} == head_keys
    assert any(k.startswith('gcn.') for k in sd) and any(k.startswith('resnet.') for k in sd)
    assert sd['attention_transform.0.weight'].shape == (32, 256) and sd['attention_transform.3.weight'].shape == (64, 32)
    gen = torch.Generator().manual_seed(3)
    ckpt = {k: (torch.randn(v.shape, generator=gen) if v.is_floating_point() else torch.full_like(v, 9)) for k, v in sd.items()}
    other = ResNet_GCN_Attention(Model(**UCLA), small_trunk(64), num_class=10, gcn_dim=256, rgb_dim=64)
    assert other.load_state_dict(ckpt, strict=True).missing_keys == []
    for k, v in other.state_dict().items():
        assert torch.equal(v, ckpt[k]), k
    full = CrossModalHead()                                       # the reference's sizes and torch's default initialisation
    assert full.attention_transform[0].weight.shape == (1024, 256) and full.classifier.weight.shape == (10, 2048)


def test_refusals():
    shape = (2, 4, 4, 8, 1, 2)
    p, f, f_rgb, dl = R.make_problem(shape, 71)
    head = make_head(shape, p).train()
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        head(f[:1].to(DEV), f_rgb[:1].to(DEV))
    head.eval()
    assert head(f[:1].to(DEV), f_rgb[:1].to(DEV)).shape == (1, 2)
    with pytest.raises(RuntimeError, match='CPU'):
        head(f, f_rgb.to(DEV))
    with pytest.raises(RuntimeError, match='fp32'):
        head(f.to(DEV).double(), f_rgb.to(DEV))
    with pytest.raises(ValueError, match='1..1024'):
        head(torch.zeros(1025, 4, device=DEV), torch.zeros(1025, 8, 1, 1, device=DEV))
    with pytest.raises(ValueError, match='do not chain'):
        head(f.to(DEV), torch.zeros(2, 12, 1, 1, device=DEV))
    with pytest.raises(ValueError, match='multiple of'):
        CrossModalHead(num_class=3, gcn_dim=6, rgb_dim=16)
    with pytest.raises(ValueError, match='multiple of'):
        CrossModalHead(num_class=3, gcn_dim=8, rgb_dim=12)
