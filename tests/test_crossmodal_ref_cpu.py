"""tests/crossmodal_ref.py, the fp64 restatement the cross-modal head's kernels are held to, against torch's own modules composed
exactly as the reference composes them (models/resnet_gcn_attention.py:60-70, :89-120) in float64 on the CPU: logits, every
parameter gradient, d f, d f_rgb and the three BatchNorm1d buffers, in train and in eval mode, to fp64 rounding.  Also here,
without a GPU: the extension header goes through the binding generator unmodified and leaves the core binding alone, the built
library exports what the header declares, every entry point refuses bad arguments before it launches anything, and the seeds of
the end-to-end GPU test keep the reference's own near-zero ReLUs under the cap."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import crossmodal_ref as R
from tam_gcn_amd import _abi, _lib, _xm_lib, build

RTOL = 1e-12


def torch_head(p, f, f_rgb, dlogits, training):
    """the reference's composition, float64"""
    N, D = f.shape
    Hd, Rr, K = p['W1'].shape[0], p['W2'].shape[0], p['Wc'].shape[0]
    at = nn.Sequential(nn.Linear(D, Hd), nn.BatchNorm1d(Hd), nn.ReLU(inplace=True), nn.Linear(Hd, Rr), nn.Sigmoid()).double()
    cl = nn.Linear(Rr, K).double()
    with torch.no_grad():
        for dst, k in ((at[0].weight, 'W1'), (at[0].bias, 'b1'), (at[1].weight, 'gamma'), (at[1].bias, 'beta'), (at[1].running_mean, 'rmean'),
                       (at[1].running_var, 'rvar'), (at[3].weight, 'W2'), (at[3].bias, 'b2'), (cl.weight, 'Wc'), (cl.bias, 'bc')):
            dst.copy_(p[k])
        at[1].num_batches_tracked.copy_(p['nbt'])
    at.train(training)
    f = f.double().requires_grad_(True)
    f_rgb = f_rgb.double().requires_grad_(True)
    att = at(f)
    f_attended = f_rgb * att.unsqueeze(-1).unsqueeze(-1)
    out = cl(torch.flatten(nn.AdaptiveAvgPool2d((1, 1))(f_attended), 1))
    out.backward(dlogits.double())
    return dict(logits=out.detach(), df=f.grad, df_rgb=f_rgb.grad, dW1=at[0].weight.grad, db1=at[0].bias.grad, dgamma=at[1].weight.grad,
                dbeta=at[1].bias.grad, dW2=at[3].weight.grad, db2=at[3].bias.grad, dWc=cl.weight.grad, dbc=cl.bias.grad,
                running_mean=at[1].running_mean, running_var=at[1].running_var, num_batches_tracked=int(at[1].num_batches_tracked))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', R.STAGE_SHAPES[:4] + ((1, 8, 8, 16, 4, 3),))
def test_restatement_is_the_torch_composition(shape, training):
    p, f, f_rgb, dl = R.make_problem(shape, seed=5, dtype=torch.float64)
    f_rgb = f_rgb.reshape(shape[0], shape[3], -1, 1)
    if shape[0] == 1 and training:                          # torch's own refusal, which the device head repeats word for word
        with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
            torch_head(p, f, f_rgb, dl, training)
        return
    want = torch_head(p, f, f_rgb, dl, training)
    got = R.head(p, f, f_rgb, dl, training)
    assert set(want) <= set(got)
    for k, w in want.items():
        if k == 'num_batches_tracked':
            assert got[k] == w == 3 + int(training)
            continue
        scale = max(1.0, float(w.abs().max()))
        err = float((got[k] - w).abs().max())
        assert tuple(got[k].shape) == tuple(w.shape) and err <= RTOL * scale, (k, err)


def test_magnitudes_dominate_and_drop_masks_both_directions():
    p, f, f_rgb, dl = R.make_problem((17, 64, 36, 72, 49, 10), seed=2)
    h = R.hidden_fwd(f, p['W1'], p['b1'], p['gamma'], p['beta'], p['rmean'], p['rvar'], p['nbt'], True, 0.1, 1e-5)
    for k in ('mean', 'invstd', 'xhat', 'a1', 'running_mean', 'running_var'):
        assert bool((h[k][1] >= h[k][0].abs() * (1 - 1e-12)).all()), k
    drop = torch.zeros(17, 36, dtype=torch.bool)
    drop[3, 5] = True
    a, b = R.head(p, f, f_rgb, dl, True), R.head(p, f, f_rgb, dl, True, drop=drop)
    assert float(b['a1'][3, 5]) == 0.0 and (float(a['a1'][3, 5]) == 0.0 or not torch.equal(a['dW2'], b['dW2']))


@pytest.mark.parametrize('shape,seed', R.E2E_CASES)
@pytest.mark.parametrize('training', [True, False])
def test_the_end_to_end_seeds_stay_under_the_relu_cap(shape, seed, training):
    p, f, f_rgb, dl = R.make_problem(shape, seed)
    ref = R.head(p, f, f_rgb, dl, training)
    near = R.relu_margin_mask(ref['pre'], ref['pre_bar'])
    assert float(near.double().mean()) <= R.RELU_CAP, (int(near.sum()), near.numel())


def test_the_extension_header_derives_and_the_core_binding_is_untouched():
    structs, funcs, rets, defines = _abi.parse_abi(_xm_lib.XM_HEADER)
    classes, sigs, defs = _lib.derive(_xm_lib.XM_HEADER, ())
    assert structs == {} and classes == {} and defs['TAMGCN_XM_VERSION'] == _xm_lib.XM_VERSION == defines['TAMGCN_XM_VERSION']
    assert set(sigs) == set(_xm_lib.SIGNATURES) == {'tamgcn_xm_version', 'tamgcn_xm_last_error', 'tamgcn_xm_hidden_fwd', 'tamgcn_xm_gate_fwd',
                                                   'tamgcn_xm_pool_fwd', 'tamgcn_xm_pool_bwd', 'tamgcn_xm_gate_bwd', 'tamgcn_xm_hidden_bwd'}
    assert sigs['tamgcn_xm_last_error'] == (C.c_char_p, []) and sigs['tamgcn_xm_version'] == (C.c_int, [])
    res, args = sigs['tamgcn_xm_hidden_fwd']
    assert res is C.c_int and args[:8] == [C.c_void_p] * 8 and args[8:12] == [C.c_int] * 4 and args[12:14] == [C.c_float] * 2
    assert all(fn.startswith('tamgcn_xm_') for fn in sigs) and not set(sigs) & set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES) == 137
    assert 'libtamgcn_xmodal.so' in build.XM_LIB and not set(build.XM_SRC) & set(build.SRC)


@pytest.fixture(scope='module')
def xm():
    build.build(verbose=False)
    return _xm_lib.load()


def test_the_library_exports_every_declared_symbol(xm):
    assert not build.needs_build_xmodal() and not build.needs_build()
    raw = C.CDLL(build.XM_LIB)
    for name in _xm_lib.SIGNATURES:
        assert hasattr(raw, name), name
    assert xm.tamgcn_xm_version() == _xm_lib.XM_VERSION == 1


def test_every_entry_point_refuses_bad_arguments_before_any_launch(xm):
    """no GPU is needed: a refused call returns before it touches the runtime.  q is an address-like integer that is never read."""
    q, odd = 0x10000, 0x10004
    err = lambda: xm.tamgcn_xm_last_error().decode()                     # noqa: E731

    def hidden_fwd(f=q, W1=q, nbt=q, N=2, D=4, Hd=4, training=1, momentum=0.1, eps=1e-5, a1=q):
        return xm.tamgcn_xm_hidden_fwd(f, W1, q, q, q, q, q, nbt, N, D, Hd, training, momentum, eps, a1, q, q, q, None)
    for kw, word in ((dict(f=None), 'f is NULL'), (dict(W1=odd), 'W1'), (dict(N=0), 'N = 0'), (dict(N=1025), '1..1024'),
                     (dict(N=1), 'N >= 2'), (dict(D=6), 'D = 6'), (dict(Hd=0), 'Hd = 0'), (dict(nbt=None), 'num_batches_tracked'),
                     (dict(momentum=1.5), 'momentum'), (dict(eps=-1.0), 'eps'), (dict(a1=None), 'a1')):
        assert hidden_fwd(**kw) == -1 and 'tamgcn_xm_hidden_fwd' in err() and word in err(), (kw, err())

    def gate_fwd(a1=q, N=2, Hd=4, R=8, att=q):
        return xm.tamgcn_xm_gate_fwd(a1, q, q, N, Hd, R, att, None)
    for kw, word in ((dict(a1=None), 'a1'), (dict(att=odd), 'att'), (dict(N=0), 'N = 0'), (dict(Hd=5), 'Hd = 5'), (dict(R=-4), 'R = -4')):
        assert gate_fwd(**kw) == -1 and 'tamgcn_xm_gate_fwd' in err() and word in err(), (kw, err())

    def pool_fwd(f_rgb=odd, att=q, N=2, R=8, P=49, m=q):
        return xm.tamgcn_xm_pool_fwd(f_rgb, att, N, R, P, m, q, None)
    for kw, word in ((dict(f_rgb=None), 'f_rgb'), (dict(f_rgb=q + 2), 'f_rgb'), (dict(att=odd), 'att'), (dict(P=0), 'P = 0'), (dict(R=6), 'R = 6'),
                     (dict(N=1024, R=2048, P=1024), '2^31'), (dict(m=None), 'm is NULL')):
        assert pool_fwd(**kw) == -1 and 'tamgcn_xm_pool_fwd' in err() and word in err(), (kw, err())

    def pool_bwd(dg=q, N=2, R=8, P=49, dz2=q, df_rgb=odd):
        return xm.tamgcn_xm_pool_bwd(dg, q, q, N, R, P, dz2, df_rgb, None)
    for kw, word in ((dict(dg=None), 'dg'), (dict(dz2=odd), 'dz2'), (dict(df_rgb=q + 1), 'df_rgb'), (dict(P=-1), 'P = -1'), (dict(N=2000), 'N = 2000')):
        assert pool_bwd(**kw) == -1 and 'tamgcn_xm_pool_bwd' in err() and word in err(), (kw, err())

    def gate_bwd(dz2=q, N=2, Hd=4, R=8, da1=q):
        return xm.tamgcn_xm_gate_bwd(dz2, q, q, N, Hd, R, q, q, da1, None)
    for kw, word in ((dict(dz2=None), 'dz2'), (dict(da1=odd), 'da1'), (dict(N=0), 'N = 0'), (dict(Hd=2), 'Hd = 2'), (dict(R=9), 'R = 9')):
        assert gate_bwd(**kw) == -1 and 'tamgcn_xm_gate_bwd' in err() and word in err(), (kw, err())

    def hidden_bwd(da1=q, N=2, D=4, Hd=4, training=1, dz1=q, df=None):
        return xm.tamgcn_xm_hidden_bwd(da1, q, q, q, q, q, q, N, D, Hd, training, q, q, q, q, dz1, df, None)
    for kw, word in ((dict(da1=None), 'da1'), (dict(dz1=None), 'dz1'), (dict(df=odd), 'df'), (dict(N=1), 'N >= 2'), (dict(D=0), 'D = 0'),
                     (dict(Hd=7), 'Hd = 7'), (dict(N=1025, training=0), '1..1024')):
        assert hidden_bwd(**kw) == -1 and 'tamgcn_xm_hidden_bwd' in err() and word in err(), (kw, err())
