"""fp64 restatement of the cross-modal attention head (reference models/resnet_gcn_attention.py:60-70, :89-120), stage by stage
as include/tamgcn_xmodal.h cuts it, forward, backward and BatchNorm1d buffer updates, with the magnitudes the rounding bars of
tests/fp64_bars.py need: every stage returns {name: (ref, mag)} with `mag` the same expression over absolute values (see
fp64_bars), plus where a stage is not a plain sum an element-wise allowance `allow` for the error its own intermediate carries.

Bars (U = 2^-24; first order in U, each derived from the arithmetic of the stage, none from a device result):
  hidden_fwd  z = f W1^T + b1 is a D-term sum:            Ez = (D + 4) U (|f| |W1|^T + |b1|)
              mean = sum_n z / N:                          fp64_bars L = N on mean_n |z|, allow Em = mean_n Ez
              d = z - mean:                                Ed = Ez + Em + (N + 4) U mean_n |z| + 2 U |d|
              var = sum_n d^2 / N:                         Ev = mean_n (2 |d| Ed) + (N + 4) U var
              invstd = (var + eps)^-1/2:                   Ei = invstd^3 Ev / 2 + 4 U invstd
              xhat = d invstd:                             Ex = Ed invstd + |d| Ei + 2 U |xhat|
              a1 = relu(gamma xhat + beta) (1-Lipschitz):  Ea = |gamma| Ex + 3 U (|gamma xhat| + |beta|)
              running_mean, running_var:                   momentum Em (momentum N / (N - 1) Ev) + 4 U of the magnitudes
  gate_fwd    att = sigmoid(z2), z2 an Hd-term sum; sigmoid' <= 1/4:   allow = (Hd + 4) U mag(z2) / 4 + SIGMOID_ALLOW, where
              SIGMOID_ALLOW is twice the largest error of the device's 1 / (1 + expf(-z)) against fp64 over a dense grid of
              z in [-30, 30] (measured on an MI355X, profiles/xmodal_stage_bars.txt)
  pool_fwd    m a P-term sum; g = att m
  pool_bwd    dz2 = dg m att (1 - att): four roundings on |dg m att| (1 + att);  df_rgb = dg att / P: two roundings
  gate_bwd    dW2, db2 N-term sums, da1 an R-term sum
  hidden_bwd  dbeta, dgamma N-term sums (Eb, Eg); dz1 = gamma invstd (dy - dbeta / N - xhat dgamma / N): eight roundings on its
              magnitude, allow |gamma invstd| (Eb + |xhat| Eg) / N; dW1, db1 N-term sums and df an Hd-term sum OF THE DEVICE'S dz1
              (teacher-forced inside the stage)."""
import torch

U = 2.0 ** -24
SIGMOID_ALLOW = 2 * 8.93e-8        # 2 x the measured maximum (8.925e-08 at z = 7.2475), profiles/xmodal_stage_bars.txt
DT = torch.float64


def d64(t):
    return t.detach().to('cpu', DT)


def hidden_fwd(f, W1, b1, gamma, beta, rmean, rvar, nbt, training, momentum, eps):
    f, W1, b1, gamma, beta, rmean, rvar = (d64(t) for t in (f, W1, b1, gamma, beta, rmean, rvar))
    N, D = f.shape
    z = f @ W1.T + b1
    Ez = (D + 4) * U * (f.abs() @ W1.abs().T + b1.abs())
    out = {}
    if training:
        mean, Em = z.mean(0), Ez.mean(0)
        d = z - mean
        var = (d * d).mean(0)
        out['running_mean'] = ((1 - momentum) * rmean + momentum * mean, (1 - momentum) * rmean.abs() + momentum * z.abs().mean(0),
                               momentum * Em + momentum * (N + 4) * U * z.abs().mean(0))
        Ed = Ez + Em + (N + 4) * U * z.abs().mean(0) + 2 * U * d.abs()
        Ev = (2 * d.abs() * Ed).mean(0) + (N + 4) * U * var
        out['running_var'] = ((1 - momentum) * rvar + momentum * var * N / (N - 1), (1 - momentum) * rvar.abs() + momentum * var * N / (N - 1),
                              momentum * N / (N - 1) * Ev)
        out['num_batches_tracked'] = int(nbt) + 1
        out['mean'] = (mean, z.abs().mean(0), Em)
    else:
        mean, var = rmean, rvar
        d = z - mean
        Ed = Ez + 2 * U * d.abs()
        Ev = torch.zeros_like(var)
        out['running_mean'], out['running_var'], out['num_batches_tracked'] = (rmean, rmean.abs(), 0.0), (rvar, rvar.abs(), 0.0), int(nbt)
        out['mean'] = (mean, mean.abs(), 0.0)
    invstd = (var + eps) ** -0.5
    Ei = 0.5 * invstd ** 3 * Ev + 4 * U * invstd
    xhat = d * invstd
    Ex = Ed * invstd + d.abs() * Ei + 2 * U * xhat.abs()
    pre = gamma * xhat + beta
    out['invstd'] = (invstd, invstd, Ei)
    out['xhat'] = (xhat, xhat.abs(), Ex)
    out['a1'] = (torch.relu(pre), (gamma * xhat).abs() + beta.abs(), gamma.abs() * Ex)
    out['pre'], out['pre_bar'] = pre, gamma.abs() * Ex + 3 * U * ((gamma * xhat).abs() + beta.abs())
    return out


def gate_fwd(a1, W2, b2):
    a1, W2, b2 = d64(a1), d64(W2), d64(b2)
    z2 = a1 @ W2.T + b2
    mag = a1.abs() @ W2.abs().T + b2.abs()
    att = torch.sigmoid(z2)
    return {'att': (att, att, 0.25 * (a1.shape[1] + 4) * U * mag + SIGMOID_ALLOW)}


def pool_fwd(f_rgb, att):
    f_rgb, att = d64(f_rgb), d64(att)
    N, R = att.shape
    m = f_rgb.reshape(N, R, -1).mean(2)
    mag = f_rgb.abs().reshape(N, R, -1).mean(2)
    return {'m': (m, mag), 'g': (att * m, att.abs() * mag)}


def fc_fwd(g, Wc, bc):
    g, Wc, bc = d64(g), d64(Wc), d64(bc)
    return {'logits': (g @ Wc.T + bc, g.abs() @ Wc.abs().T + bc.abs())}


def fc_bwd(dlogits, g, Wc):
    dl, g, Wc = d64(dlogits), d64(g), d64(Wc)
    return {'dWc': (dl.T @ g, dl.abs().T @ g.abs()), 'dbc': (dl.sum(0), dl.abs().sum(0)), 'dg': (dl @ Wc, dl.abs() @ Wc.abs())}


def pool_bwd(dg, m, att, P, shape=None):
    dg, m, att = d64(dg), d64(m), d64(att)
    dz2 = dg * m * att * (1 - att)
    dfr = (dg * att / P)[:, :, None].expand(-1, -1, P)
    if shape is not None:
        dfr = dfr.reshape(shape)
    return {'dz2': (dz2, (dg * m * att).abs() * (1 + att.abs())), 'df_rgb': (dfr, dfr.abs())}


def gate_bwd(dz2, a1, W2):
    dz2, a1, W2 = d64(dz2), d64(a1), d64(W2)
    return {'dW2': (dz2.T @ a1, dz2.abs().T @ a1.abs()), 'db2': (dz2.sum(0), dz2.abs().sum(0)), 'da1': (dz2 @ W2, dz2.abs() @ W2.abs())}


def hidden_bwd(da1, a1, xhat, invstd, gamma, f, W1, training, dz1_dev=None, drop=None, on=None):
    """dz1_dev: the device's dz1, which the sums dW1, db1 and df are then taken of (teacher-forced); drop: a (N, Hd) bool mask of
    hidden activations whose contribution is left out; on: the ReLU mask to use instead of a1 > 0 (tests/test_gpu_crossmodal.py)."""
    da1, a1, xhat, invstd, gamma, f, W1 = (d64(t) for t in (da1, a1, xhat, invstd, gamma, f, W1))
    N = f.shape[0]
    dy = torch.where(a1 > 0 if on is None else on, da1, torch.zeros((), dtype=DT))
    if drop is not None:
        dy = torch.where(drop, torch.zeros((), dtype=DT), dy)
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    mb, mg = dy.abs().sum(0), (dy * xhat).abs().sum(0)
    sc = gamma * invstd
    if training:
        dz1 = sc * (dy - dbeta / N - xhat * dgamma / N)
        mz = sc.abs() * (dy.abs() + mb / N + xhat.abs() * mg / N)
        az = sc.abs() * ((N + 4) * U * mb + xhat.abs() * (N + 4) * U * mg) / N
    else:
        dz1, mz, az = sc * dy, (sc * dy).abs(), 0.0
    out = {'dbeta': (dbeta, mb), 'dgamma': (dgamma, mg), 'dz1': (dz1, mz, az)}
    z = dz1 if dz1_dev is None else d64(dz1_dev)
    out['dW1'] = (z.T @ f, z.abs().T @ f.abs())
    out['db1'] = (z.sum(0), z.abs().sum(0))
    out['df'] = (z @ W1, z.abs() @ W1.abs())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the whole head, chained in fp64: what tests/test_crossmodal_ref_cpu.py holds to torch's own modules
# ---------------------------------------------------------------------------------------------------------------------
PARAMS = ('W1', 'b1', 'gamma', 'beta', 'W2', 'b2', 'Wc', 'bc')


def head(p, f, f_rgb, dlogits, training, momentum=0.1, eps=1e-5, drop=None, relu_side=None):
    """p: dict of W1 b1 gamma beta rmean rvar nbt W2 b2 Wc bc.  Returns {name: ref} of the logits, every gradient and the buffers;
    'pre' / 'pre_bar' are the hidden pre-activation (input of the ReLU) and its fp32 rounding bar.  drop: see hidden_bwd; the
    forward then also runs with those activations at 0.  relu_side: a (N, Hd) bool tensor, the side (a1 > 0) another evaluation took;
    the backward follows it on the units within their bar of 0 (relu_margin_mask) and nowhere else."""
    h = hidden_fwd(f, p['W1'], p['b1'], p['gamma'], p['beta'], p['rmean'], p['rvar'], p['nbt'], training, momentum, eps)
    a1, xhat, invstd = h['a1'][0], h['xhat'][0], h['invstd'][0]
    on = None
    if relu_side is not None:
        on = torch.where(relu_margin_mask(h['pre'], h['pre_bar']), relu_side.cpu(), h['pre'] > 0)
    if drop is not None:
        a1 = torch.where(drop, torch.zeros((), dtype=DT), a1)
    att = gate_fwd(a1, p['W2'], p['b2'])['att'][0]
    pf = pool_fwd(f_rgb, att)
    m, g = pf['m'][0], pf['g'][0]
    out = {'logits': fc_fwd(g, p['Wc'], p['bc'])['logits'][0], 'pre': h['pre'], 'pre_bar': h['pre_bar'], 'a1': a1, 'att': att,
           'running_mean': h['running_mean'][0], 'running_var': h['running_var'][0], 'num_batches_tracked': h['num_batches_tracked']}
    fb = fc_bwd(dlogits, g, p['Wc'])
    P = f_rgb.shape[2] * f_rgb.shape[3]
    pb = pool_bwd(fb['dg'][0], m, att, P, tuple(f_rgb.shape))
    gb = gate_bwd(pb['dz2'][0], a1, p['W2'])
    hb = hidden_bwd(gb['da1'][0], a1, xhat, invstd, p['gamma'], f, p['W1'], training, drop=drop, on=on)
    out.update(dWc=fb['dWc'][0], dbc=fb['dbc'][0], df_rgb=pb['df_rgb'][0], dW2=gb['dW2'][0], db2=gb['db2'][0], dgamma=hb['dgamma'][0],
               dbeta=hb['dbeta'][0], dW1=hb['dW1'][0], db1=hb['db1'][0], db1_mag=hb['db1'][1], df=hb['df'][0])
    return out


def make_problem(shape, seed, dtype=torch.float32):
    """Seeded inputs and parameters of a head of shape (N, D, Hd, R, P, K); P is laid out as (P, 1)."""
    N, D, Hd, R, P, K = shape
    gen = torch.Generator().manual_seed(seed)

    def r(*s, scale=1.0):
        return (torch.randn(*s, generator=gen, dtype=torch.float64) * scale).to(dtype)
    p = dict(W1=r(Hd, D, scale=D ** -0.5), b1=r(Hd, scale=0.1), gamma=1 + r(Hd, scale=0.2), beta=r(Hd, scale=0.2),
             rmean=r(Hd, scale=0.3), rvar=(0.5 + r(Hd).abs()), nbt=torch.tensor(3, dtype=torch.int64),
             W2=r(R, Hd, scale=Hd ** -0.5), b2=r(R, scale=0.1), Wc=r(K, R, scale=R ** -0.5), bc=r(K, scale=0.1))
    f = r(N, D)
    f_rgb = torch.relu(r(N, R, P, 1)) + r(N, R, P, 1, scale=0.05)            # a post-ReLU map, mostly
    dlogits = r(N, K, scale=1.0 / N)
    return p, f, f_rgb, dlogits


def relu_margin_mask(pre, pre_bar):
    """hidden activations whose fp64 pre-activation lies within its own fp32 rounding bar of 0: their ReLU may flip"""
    return pre.abs() <= pre_bar


# shapes (N, D, Hd, R, P, K) of tests/test_gpu_crossmodal_stages.py, and the end-to-end cases of tests/test_gpu_crossmodal.py with
# the seeds tests/test_crossmodal_ref_cpu.py verifies (the fp64 reference alone keeps the ReLUs within their rounding bar of 0
# under RELU_CAP of the hidden activations)
STAGE_SHAPES = ((2, 4, 4, 8, 1, 2), (3, 8, 20, 40, 3, 3), (17, 64, 36, 72, 49, 10), (33, 256, 128, 256, 50, 10), (16, 256, 1024, 2048, 49, 10))
E2E_CASES = (((17, 64, 36, 72, 49, 10), 11), ((16, 256, 1024, 2048, 49, 10), 12))
RELU_CAP = 0.01
