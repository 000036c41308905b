"""-m gpu: the device dropout (tam_gcn_amd/dropout.py; include/tamgcn.h, tamgcn_drop_add_act_fwd) against tests/dropout_ref.py.

  1. the forward kernel alone: keep nibble == mask() exactly, sign nibble == (out > 0) exactly, values within the derived
     rounding bar of the fp64 restatement, dropped elements exactly +0;
  2. the backward kernel alone: dza / dzr bit-equal to the fp32 products, part within tests/ew_ref.py's bars for add_act_bwd's sums;
  3. st_gcn with dropout.enable() against the fp64 teacher fed the same mask, bars of stgcn_block_ref.bars();
  4. the stream: same (seed, call) -> same bits, advance() -> the reference's call + 1, set_state() goes back, a captured
     forward + advance replays call, call + 1, call + 2;
  5. a small ST-GCN model under CapturedStep: graph == eager bit for bit, construction consumes no draw, every micro-batch its own call;
  6. the heads of both models; 7. eval mode, disable() and a never-enabled model behave as before.

Shapes are the smallest that reach every path of the two kernels (tests/dropout_ref.py KERNEL_CASES)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dropout_ref as D                                                         # noqa: E402
import fp64_bars as B                                                           # noqa: E402
import stgcn_block_ref as R                                                     # noqa: E402
from cases import tag_seed                                                      # noqa: E402
from params import fill_state_, make_input, make_labels                         # noqa: E402
from tam_gcn_amd import dropout, functional as Fn, ops                          # noqa: E402
from tam_gcn_amd.models import ctrgcn as CM, stgcn as M                         # noqa: E402
from tam_gcn_amd.ops import S                                                   # noqa: E402

DEV = torch.device('cuda:0')
KCASES = pytest.mark.parametrize('tag', list(D.KERNEL_CASES), ids=lambda t: t.replace(' ', '_'))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _state(seed, call):
    return torch.tensor([dropout._i64(seed), dropout._i64(call)], dtype=torch.int64, device=DEV)


def _src(x, coef):
    x = ops.with_slack(_dev(x))
    return S(x, coef=_dev(coef)) if coef is not None else S(x)


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
@KCASES
def test_forward_kernel(tag):
    q = D.kernel_problem(tag)
    N, C, T, V = q['shape']
    res = _src(q['r'], q['rcoef']) if q['r'] is not None else None
    out, bits = ops.drop_add_act_fwd(_src(q['z'], q['acoef']), res, q['relu'], C, _state(q['seed'], q['call']), q['site'], q['p'])
    torch.cuda.synchronize()
    out, bits = out.cpu(), bits.cpu().numpy()
    assert bits.shape == (N, C, (T * V + 3) // 4)
    sign, keep = D.nibbles(bits, T * V)
    assert np.array_equal(keep.reshape(q['shape']), q['keep'].numpy()), 'keep nibble != mask()'
    want_sign = (out > 0).numpy() if q['relu'] else np.zeros(q['shape'], dtype=bool)
    assert np.array_equal(sign.reshape(q['shape']), want_sign), 'sign nibble != (out > 0)'
    if T * V % 4:                                           # the unused bits of a row's last byte stay clear
        used = (1 << (T * V % 4)) - 1
        assert not (bits[..., -1] & ~np.uint8(used | (used << 4))).any()
    ref, bar, pre = D.fwd_ref(q)
    # a pre-ReLU value within its bar of zero; a dropped element without residual is +0 exactly (bar 0): no decision there
    near = ((pre.abs() <= bar) & (bar > 0)) if q['relu'] else torch.zeros(q['shape'], dtype=torch.bool)
    assert int(near.sum()) == 0 <= D.EXCLUDE_CAP * out.numel()          # seeded O(1) inputs: the reference leaves out none
    err = (out.double() - ref).abs()
    print(f'{tag}: max err / bar {float((err / bar.clamp_min(1e-300))[bar > 0].max()):.3g}, kept {float(q["keep"].float().mean()):.4f}')
    assert bool((err <= bar).all()), f'{int((err > bar).sum())} elements outside the three-rounding bar'
    if q['r'] is None:                                      # a dropped element is +0, not -0
        dropped = out[~q['keep']]
        assert bool((dropped == 0).all()) and not bool(torch.signbit(dropped).any())


@KCASES
def test_backward_kernel(tag):
    q = D.kernel_problem(tag)
    N, C, T, V = q['shape']
    has_r = q['r'] is not None
    bits = D.pack_bits(q['sign'], q['keep'])
    d32, za32, bars = D.bwd_ref(q)
    dza, dzr, part = ops.drop_add_act_bwd(_dev(q['dout']), _dev(bits), q['relu'], q['p'], _dev(q['z']), _dev(q['a_save']),
                                          _dev(q['r']) if has_r else None, _dev(q['r_save']) if has_r else None, want_dzr=True)
    torch.cuda.synchronize()
    assert torch.equal(dza.cpu(), za32), 'dza is not fl32(d * scale) under the keep bits'
    assert torch.equal(dzr.cpu(), d32), 'dzr is not dout under the sign bits'
    assert part.shape == (4 if has_r else 2, C, N)
    for i, k in enumerate(sorted(bars)):
        b = bars[k]
        worst = B.check(f'{tag} part[{i}]', part[i], b.val, b.mag, b.L, allow=b.allow)
        print(f'{tag} {k}: max err {worst:.3g}')
    # two runs are bit-equal (fixed-order sums), and the form without sums (functional.dropout) writes the same dza
    dza2, _, part2 = ops.drop_add_act_bwd(_dev(q['dout']), _dev(bits), q['relu'], q['p'], _dev(q['z']), _dev(q['a_save']),
                                          _dev(q['r']) if has_r else None, _dev(q['r_save']) if has_r else None, want_dzr=True)
    dza3, dzr3, part3 = ops.drop_add_act_bwd(_dev(q['dout']), _dev(bits), q['relu'], q['p'], None, None, None, None, want_dzr=False)
    assert torch.equal(dza2, dza) and torch.equal(part2, part)
    assert torch.equal(dza3, dza) and dzr3 is None and part3 is None


def test_forward_then_backward_use_the_same_bits():
    """The bits the forward writes are the bits the backward wants: dz of the pair equals the restatement built from the
    forward's own output signs."""
    q = D.kernel_problem('tail3 L175')
    N, C, T, V = q['shape']
    out, bits = ops.drop_add_act_fwd(_src(q['z'], q['acoef']), _src(q['r'], q['rcoef']), True, C, _state(q['seed'], q['call']), q['site'], q['p'])
    dza, dzr, _ = ops.drop_add_act_bwd(_dev(q['dout']), bits, True, q['p'], _dev(q['z']), _dev(q['a_save']), None, None, want_dzr=True)
    q = dict(q, sign=(out > 0).cpu())
    d32, za32, _ = D.bwd_ref(q)
    assert torch.equal(dza.cpu(), za32) and torch.equal(dzr.cpu(), d32)


# ---------------------------------------------------------------------------------------------------------------------
# 3: the block
# ---------------------------------------------------------------------------------------------------------------------
def _drop_block(tag):
    """The module of D.BLOCK_CASES[tag] with dropout = DROP_P, enabled as site DROP_SITE of a stream at (DROP_SEED, DROP_CALL)."""
    kt, cin, cout, stride, residual, T, V = D.BLOCK_CASES[tag]
    blk = M.st_gcn(cin, cout, (kt, 3), stride, dropout=D.DROP_P, residual=residual)
    fill_state_(blk.state_dict(), seed=tag_seed(tag))
    fillers = [M.st_gcn(3, 4, (1, 3), dropout=D.DROP_P) for _ in range(D.DROP_SITE)]
    holder = torch.nn.ModuleList(fillers + [blk]).to(DEV).train()
    stream = dropout.enable(holder, seed=D.DROP_SEED)
    stream.set_state(D.DROP_SEED, D.DROP_CALL)
    assert dropout.site_of(blk) == D.DROP_SITE and dropout.stream_of(blk) is stream
    return blk, stream


def _run_block(blk, b, t):
    for p in blk.parameters():
        p.grad = None
    with torch.no_grad():
        for k, buf in blk.named_buffers():
            buf.copy_(b.sd[k].to(buf.dtype))
    x = t.x.float().to(DEV).requires_grad_(True)
    Ae = b.Ae.float().to(DEV).requires_grad_(True)
    y = blk(x, Ae)[0]
    y.backward(b.cot.float().to(DEV))
    torch.cuda.synchronize()
    return y.detach(), x.grad, Ae.grad, {k: p.grad for k, p in blk.named_parameters()}, {k: v.detach().clone() for k, v in blk.named_buffers()}


@pytest.mark.parametrize('mode', [1, 0], ids=['split_bf16_bwd', 'exact_f32'])
@pytest.mark.parametrize('tag', list(D.BLOCK_CASES), ids=R.iso_id)
def test_block_against_the_teacher_with_the_same_mask(tag, mode):
    from tam_gcn_amd import _lib
    b, t = D.block_teacher(tag)
    blk, stream = _drop_block(tag)
    lib = _lib.load()
    prev = lib.tamgcn_get_split_mode()
    lib.tamgcn_set_split_mode(mode)
    try:
        got = _run_block(blk, b, t)
    finally:
        lib.tamgcn_set_split_mode(prev)
    assert stream.state() == (D.DROP_SEED, D.DROP_CALL)                 # a bare block leaves advance() to its caller
    ratios = R.verify(got, t, mode)
    print(R.line(f'dropout {R.iso_id(tag)} mode {mode} nudges {t.tries} worst {max(ratios.values()):.2g}', ratios))


def test_block_without_saved_state_keeps_no_bits_and_matches():
    """no_grad in train mode: the same output bit for bit, through the bit-less launch."""
    tag = 'k9 64->64 s1'
    b, t = D.block_teacher(tag)
    blk, stream = _drop_block(tag)
    x, Ae = t.x.float().to(DEV), b.Ae.float().to(DEV)
    y1 = blk(x.clone().requires_grad_(True), Ae)[0].detach()
    with torch.no_grad():
        y2 = blk(x, Ae)[0]
    assert torch.equal(y1, y2)


# ---------------------------------------------------------------------------------------------------------------------
# 4: the stream
# ---------------------------------------------------------------------------------------------------------------------
SHAPE4 = (2, 8, 7, 25)


def _kept(out):
    return (out != 0).cpu()


def test_stream_semantics():
    stream = dropout.DropoutStream(991, DEV)
    assert stream.state() == (991, 0)
    x = (make_input(SHAPE4, 4) + 2.0).to(DEV)                            # positive: out != 0 exactly where an element was kept
    a = Fn.dropout(x, 0.5, stream, 7)
    assert torch.equal(a, Fn.dropout(x, 0.5, stream, 7))                 # same (seed, call): the same bits
    assert torch.equal(_kept(a), D.mask_nctv(991, 0, 7, SHAPE4, 0.5))
    assert torch.equal(a.cpu(), torch.where(D.mask_nctv(991, 0, 7, SHAPE4, 0.5), x.cpu() * 2.0, torch.zeros(())))
    stream.advance()
    b = Fn.dropout(x, 0.5, stream, 7)
    assert stream.state() == (991, 1) and torch.equal(_kept(b), D.mask_nctv(991, 1, 7, SHAPE4, 0.5))
    assert not torch.equal(a, b)
    stream.set_state(991, 0)
    assert torch.equal(Fn.dropout(x, 0.5, stream, 7), a)                 # back to an earlier state: that forward again
    big = (2 ** 40 + 7, 2 ** 33)
    stream.load_state_dict({'seed': big[0], 'call': big[1]})
    assert stream.state_dict() == {'seed': big[0], 'call': big[1]}
    assert torch.equal(_kept(Fn.dropout(x, 0.25, stream, 9)), D.mask_nctv(big[0], big[1], 9, SHAPE4, 0.25))
    # the gradient is the same mask and scale
    xg = x.clone().requires_grad_(True)
    g = make_input(SHAPE4, 5).to(DEV)
    Fn.dropout(xg, 0.25, stream, 9).backward(g)
    sc = float(D.consts(0.25)[1])
    assert torch.equal(xg.grad.cpu(), torch.where(D.mask_nctv(big[0], big[1], 9, SHAPE4, 0.25), g.cpu() * sc, torch.zeros(())))


def test_captured_forward_draws_a_new_mask_every_replay():
    stream = dropout.DropoutStream(17, DEV)
    x = (make_input(SHAPE4, 6) + 2.0).to(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            Fn.dropout(x, 0.5, stream, 3)
            stream.advance()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    call = 2 ** 32 - 2                                                   # the replays cross the low word of the counter
    stream.set_state(17, call)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = Fn.dropout(x, 0.5, stream, 3)
        stream.advance()
    assert stream.state() == (17, call)                                  # capturing executes nothing
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_kept(out), D.mask_nctv(17, call + k, 3, SHAPE4, 0.5)), k
    assert stream.state() == (17, call + 3)


# ---------------------------------------------------------------------------------------------------------------------
# 5: model and CapturedStep
# ---------------------------------------------------------------------------------------------------------------------
XSHAPE = (4, 3, 13, 20, 1)
MARGS = dict(in_channels=3, num_class=4, num_point=20, num_person=1, graph='graph.ucla.Graph', graph_args=dict(labeling_mode='spatial'))
DROP_BLOCKS = (0, 2, 4)                                                  # no residual, identity, conv residual


def _model(enable_seed=None):
    """The reference's Model hands `dropout` to its head only (models/stgcn.py:121, :141-150); the blocks of DROP_BLOCKS get theirs
    here, the way a user of the published dropout = 0.5 network sets them."""
    m = M.Model(**MARGS, dropout=0.5)
    fill_state_(m.state_dict(), seed=R.PARAM_SEED)
    for i in DROP_BLOCKS:
        m.st_gcn_networks[i]._dropout = m.st_gcn_networks[i].tcn[4].p = 0.5
    m = m.to(DEV).train()
    return m, (dropout.enable(m, seed=enable_seed) if enable_seed is not None else None)


def _bn_state(m):
    return [t.clone() for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)
            for t in (mod.running_mean, mod.running_var, mod.num_batches_tracked)]


def _train(eager, accum, batches):
    from tam_gcn_amd.distributed import ParamArena
    from tam_gcn_amd.optim import FusedSGD
    from tam_gcn_amd.training import CapturedStep
    m, stream = _model(enable_seed=77)
    assert [dropout.site_of(m.st_gcn_networks[i]) for i in DROP_BLOCKS] == [0, 1, 2] and dropout.site_of(m) == 3
    arena = ParamArena(m)
    bucket = arena.grad_bucket()
    opt = FusedSGD(arena, bucket, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
    stream.set_state(77, 10)
    before = arena.flat.clone()
    step = CapturedStep(m, Fn.CrossEntropyLoss(), opt, arena, bucket, *batches[0], eager=eager, accum_steps=accum)
    assert stream.state() == (77, 10)                                    # construction (its warm-up steps) consumes no draw
    assert torch.equal(arena.flat, before)
    losses = [step.step(x, y).clone() for x, y in batches]
    torch.cuda.synchronize()
    assert stream.state() == (77, 10 + len(batches))                     # one call per forward, micro-batches included
    return torch.stack(losses).cpu(), arena.flat.cpu(), [t.cpu() for t in _bn_state(m)]


@pytest.mark.parametrize('accum', [1, 2])
def test_captured_step_equals_eager_with_device_dropout(accum):
    n = 3 if accum == 1 else 4
    batches = [(make_input(XSHAPE, 30 + i).to(DEV), make_labels(XSHAPE[0], 4, 130 + i).to(DEV)) for i in range(n)]
    if accum == 2:
        batches[1] = batches[0]                                          # the same micro-batch twice: only the mask differs
    ref, got = _train(True, accum, batches), _train(False, accum, batches)
    assert torch.equal(got[0], ref[0]), (got[0], ref[0])
    assert torch.equal(got[1], ref[1]), float((got[1] - ref[1]).abs().max())
    assert len(got[2]) == len(ref[2]) > 0 and all(torch.equal(a, b) for a, b in zip(got[2], ref[2]))
    if accum == 2:
        assert float(ref[0][0]) != float(ref[0][1])                      # every micro-batch drew its own mask


def test_a_wrapped_model_without_head_dropout_still_advances_once_per_forward():
    m = M.Model(**MARGS)                                                 # dropout = 0: no head site
    fill_state_(m.state_dict(), seed=R.PARAM_SEED)
    m.st_gcn_networks[1]._dropout = m.st_gcn_networks[1].tcn[4].p = 0.5
    holder = torch.nn.Sequential(m).to(DEV).train()
    stream = dropout.enable(holder, seed=8)
    assert dropout.site_of(m.st_gcn_networks[1]) == 0 and dropout.site_of(m) is None and dropout.stream_of(m) is stream
    x = make_input(XSHAPE, 43).to(DEV)
    a = holder(x)
    b = holder(x)
    assert stream.state() == (8, 2) and not torch.equal(a, b)
    stream.set_state(8, 0)
    assert torch.equal(holder(x), a)


# ---------------------------------------------------------------------------------------------------------------------
# 6: the heads
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['stgcn', 'ctrgcn'])
def test_head_mask_and_logits(which):
    if which == 'stgcn':
        m = M.Model(**MARGS, dropout=0.5)
        fill_state_(m.state_dict(), seed=R.PARAM_SEED)
        W, bias = m.fcn.weight.detach().view(4, -1), m.fcn.bias.detach()
    else:
        m = CM.Model(**{k: v for k, v in MARGS.items() if k != 'in_channels'}, drop_out=0.5)
        fill_state_(m.state_dict(), seed=R.PARAM_SEED)
        W, bias = m.fc.weight.detach(), m.fc.bias.detach()
    m = m.to(DEV).train()
    stream = dropout.enable(m, seed=4242)
    site = dropout.site_of(m)
    stream.set_state(4242, 6)
    x = make_input(XSHAPE, 40).to(DEV)
    with torch.no_grad():
        h, N, Mp = m._blocks(x)[:3]
        pooled = h.view(N, Mp, h.size(1), -1).mean(3).mean(1)            # train-mode BatchNorm: independent of the running statistics
        logits = m(x)
        dropped = Fn.dropout(pooled, 0.5, stream, site)                  # m(x) advanced the stream: this is call 7
    torch.cuda.synchronize()
    assert stream.state() == (4242, 7)
    Cc = pooled.shape[1]
    pooled, dropped = pooled.cpu(), dropped.cpu()
    assert float(pooled.min()) > 0                                       # means of ReLU outputs: out != 0 iff kept
    keep7 = torch.from_numpy(D.mask(4242, 7, site, N, Cc, 0.5))
    assert torch.equal(dropped != 0, keep7) and torch.equal(dropped, torch.where(keep7, pooled * 2.0, torch.zeros(())))
    keep6 = torch.from_numpy(D.mask(4242, 6, site, N, Cc, 0.5)).double()
    # the fp64 head on the device's pooled vector with the mask of call 6; stemhead_ref.fc_fwd's bar (C products and the bias)
    # with one more rounding for the product with the scale
    ref = (pooled.double() * keep6 * 2.0) @ W.double().cpu().t() + bias.double().cpu()
    mag = (pooled.double().abs() * keep6 * 2.0) @ W.double().cpu().abs().t() + bias.double().cpu().abs()
    B.check(f'{which} head logits', logits, ref, mag, Cc + 2)
    # a wrong mask is far outside that bar
    wrong = (pooled.double() * torch.from_numpy(D.mask(4242, 5, site, N, Cc, 0.5)).double() * 2.0) @ W.double().cpu().t() + bias.double().cpu()
    with pytest.raises(B.BarError):
        B.check('wrong call', logits, wrong, mag, Cc + 2)


# ---------------------------------------------------------------------------------------------------------------------
# 7: nothing else moved
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_mode_is_untouched_and_disable_goes_back(monkeypatch):
    from tam_gcn_amd import f2s
    plain, _ = _model()
    enabled, stream = _model(enable_seed=5)
    x = make_input(XSHAPE, 41).to(DEV)
    plain.eval(), enabled.eval()
    with torch.no_grad():
        a, b = plain(x), enabled(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert isinstance(enabled.__dict__.get('_tamgcn_f2s'), f2s.FusedEvalST)          # still the small-batch eval family
    assert stream.state() == (5, 0)
    assert set(enabled.state_dict()) == set(plain.state_dict())                      # the state is no registered buffer
    # after disable() an active block calls torch's dropout again
    blk = enabled.st_gcn_networks[2].train()
    calls = []
    real = torch.nn.functional.dropout

    def spy(inp, p=0.5, training=True, inplace=False):
        calls.append(p)
        return real(inp, p, training, inplace)

    monkeypatch.setattr(torch.nn.functional, 'dropout', spy)
    h = make_input((2, 64, 13, 20), 42).to(DEV)
    Ae = (enabled.A * enabled.edge_importance[2]).detach()
    blk(h, Ae)
    assert calls == []                                                               # enabled: the device path
    dropout.disable(enabled)
    assert dropout.stream_of(blk) is None and dropout.streams_under(enabled) == []
    blk(h, Ae)
    assert calls == [0.5]
