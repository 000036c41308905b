/*
 * tamgcn.h — C ABI of the MI355X-native CTR-GCN hot path (libtamgcn.so).
 *
 * The reference (Tamnemng/TAM-GCN) has no FFI / operator registry: its hot
 * path is stock ATen ops issued from models/ctrgcn.py.  The
 * entry points below are therefore what a binding for that path binds
 * instead of those ATen calls; each one cites the reference lines whose
 * arithmetic it replaces.  Plain pointers and sizes only: no torch types.
 *
 * Conventions
 *   - every tensor is fp32, dense, NCHW-contiguous (N, C, T, V), V innermost,
 *     and lives in device (HBM) memory owned by the caller;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     allocates nothing, never synchronises the device and is safe inside
 *     hipGraph stream capture; scratch/partial buffers are caller-provided;
 *   - return value 0 = launched; <0 = rejected before any launch
 *     (tamgcn_last_error() gives the reason for the calling thread);
 *   - calls are re-entrant per stream: no global mutable state;
 *   - READ SLACK.  Skeletons whose joint count V is not a multiple of 4 (NTU: 25): the 16-byte kernels read the last piece
 *     of a frame whole, i.e. up to 12 bytes past the last element of a SOURCE activation.  The contract is one statement,
 *     for every entry point: 16 readable bytes behind the last element of each such buffer (one whole piece; what is read
 *     there is discarded).  The buffers it binds are the activations streamed in 16-byte pieces from dword-aligned rows:
 *     tamgcn_conv / _conv_pair d->src, the tamgcn_tconv_* d->src and d->mask, x3 and dy of the tamgcn_ctrgc_tiled_* and
 *     tamgcn_vgen_* aggregation and dE-accumulation entry points, and d->x of the f2v / f2g stages.  Every other operand is
 *     read inside its extent.  The Python layer allocates that slack (ops.empty) and copies caller tensors that lack it
 *     (ops.with_slack); tests/slack_audit.py holds every launch to it.
 *
 * "src" operands.  Most kernels read their activation operand through a fused
 * per-channel affine/mix prologue so that train-mode BatchNorm apply (forward)
 * and BatchNorm-backward apply never cost a separate pass over HBM:
 *      value(n,c,t,v) = act( c1[c]*x1 + c2[c]*x2 + c0[c] )
 * with coef = [3][ctot] = (c1, c2, c0) indexed by absolute channel, x2 and
 * coef optional (NULL: value = x1), act 0 = identity, 1 = ReLU.
 * Out-of-range taps (temporal zero padding) are 0 *after* the prologue, as in
 * the reference where padding follows BN+ReLU (models/ctrgcn.py:95-107).
 */
#ifndef TAMGCN_H
#define TAMGCN_H

#ifdef __cplusplus
extern "C" {
#endif

#define TAMGCN_VERSION 401          /* round 4: bumped on every change of a struct layout, signature or documented semantics */
#define TAMGCN_MAX_SUBSETS 3
#define TAMGCN_MAX_V 32             /* joints supported by the LDS-resident CTRGC tiles (V in {20, 25}); V in {32, 64}: tamgcn_ctrgc_tiled_* */

typedef struct tamgcn_src {
    const float* x1;
    const float* x2;                /* optional */
    const float* coef;              /* optional, [3][ctot] */
    int ctot;                       /* channels of the x1/x2 allocations */
    int coff;                       /* first channel used */
    int act;                        /* 0 none, 1 relu */
} tamgcn_src;

/* ------------------------------------------------------------------------
 * Library
 * --------------------------------------------------------------------- */
int         tamgcn_version(void);
const char* tamgcn_last_error(void);
/* symbol (template arguments included) of the kernel the calling thread's last ABI call launched;
 * lets a profiler attribute HIP-event timings to the rows of a rocprofv3 kernel trace */
const char* tamgcn_last_kernel(void);
/* GEMM arithmetic policy (process-wide; initial value from the environment variable TAMGCN_SPLIT_BF16, default 0 =
 * the reference's own arithmetic; 1 is an opt-in):
 *   0  exact fp32-input MFMA (v_mfma_f32_16x16x4_f32) in every GEMM;
 *   1  as 0 in the forward; weight-gradient GEMMs and the data-gradient GEMMs into >= 128 channels run as a 2-term
 *      bf16 split (three v_mfma_f32_16x16x32_bf16, ~4.5e-6 relative error): their results never feed an activation.
 * Takes effect for launches issued after the call; not a stream operation. */
int         tamgcn_get_split_mode(void);
int         tamgcn_set_split_mode(int mode);

/* bytes of LDS the CTRGC kernels need for (S subsets, V joints, R rel-channels): the fused LDS-resident workgroup for
 * V = 20, the streaming family (tamgcn_ctrgc_tiled_*) for V in {25, 32, 64};
 * <0 if the shape is unsupported.  Lets the host fail early and loudly.  Every other 2 <= V <= 32 runs on the
 * run-time-V family: tamgcn_vgen_supported / tamgcn_vgen_lds_bytes. */
int         tamgcn_ctrgc_lds_bytes(int S, int V, int R);

/* ------------------------------------------------------------------------
 * k x 1 convolution over (N,C,T,V) as an MFMA GEMM (fp32 in / fp32 acc,
 * v_mfma_f32_16x16x4_f32).  Replaces aten::convolution for
 *   - 1x1 channel mixing: CTRGC conv1..4 on pooled joints, unit_gcn.down,
 *     unit_gcn.offset_conv, the 4 MS-TCN branch entry convs, unit_tcn
 *     (reference models/ctrgcn.py:161-164, 211-213, 219-221, 95-99, 114, 122, 183)
 *   - dilated temporal convs (TemporalConv, models/ctrgcn.py:56-62)
 * and, with wmode = 1, for their data gradients (aten::convolution_backward,
 * input part): the weight is then read transposed with taps flipped and the
 * src is zero-upsampled by `up` (the forward stride).
 *
 *   y[n, ycoff+m, (t*ostride), v] = bias[m]
 *        + sum_{k,j} W(m,k,j) * src(n, k, t*stride + j*dil - pad, v)
 *        + bcast[m, n, v]*bcast_scale + add1[...] + add2[...]
 *   then  y *= (mask_src > 0)  if mask is given,
 *   and per-channel partial sums  (sum y, sum y*(aux - aux_center))  -> stats_part
 *   (aux = y itself, uncentred, when aux is NULL: the train-mode BatchNorm moments).
 * ---------------------------------------------------------------------- */
typedef struct tamgcn_conv_desc {
    tamgcn_src src;                 /* (N, src.ctot, T_in, V); uses K channels from src.coff */
    int N, K, T_in, V;
    const float* w;                 /* wmode 0: [M][K][KT]   wmode 1: [K][M][KT] (read transposed+flipped) */
    const float* bias;              /* [M] or NULL */
    int M, KT, dil, stride, pad;
    int wmode;                      /* 0 forward, 1 data-gradient */
    int up;                         /* src zero-upsampling factor (1 = none); wmode 1 with strided fwd */
    float* y;                       /* (N, yctot, T_y, V) */
    int yctot, ycoff;
    int T_out;                      /* number of output t computed */
    int T_y;                        /* T extent of the y allocation */
    int ostride;                    /* output t stride (1; 2 scatters a strided 1x1 data-gradient) */
    const float* add1;              /* optional, same geometry as y (may alias y) */
    const float* add2;              /* optional, same geometry as y */
    const float* bcast;             /* optional [M][N][V], broadcast over t */
    float bcast_scale;
    const tamgcn_src* mask;         /* optional, geometry of y: y *= (value > 0) */
    const float* aux;               /* optional, geometry (N, auxctot, T_y, V) at auxcoff */
    const float* aux_center;        /* [auxctot] per-channel value subtracted from aux (the BN batch mean) */
    int auxctot, auxcoff;
    float* stats_part;              /* optional [2][stats_ctot][nparts] written at channel stats_coff+m */
    int stats_ctot, stats_coff;
    /* eval-mode fusion: with BatchNorm folded to a per-channel affine the convolution can finish
     * its consumer's work:  y = act( c1[ch]*(conv + bias) + c0[ch] + bcast + add1 + add2 ),  ch = ycoff + m,
     * c1 = post_coef[ch], c0 = post_coef[2*post_ctot + ch] (the [3][post_ctot] layout tamgcn_bn_fwd_finalize writes),
     * post_act 1 = ReLU after the adds.  NULL / 0: the plain form above. */
    const float* post_coef;
    int post_ctot, post_act;
} tamgcn_conv_desc;

/* number of stats partials per channel the call writes (= N * t-tiles) */
int tamgcn_conv_nparts(const tamgcn_conv_desc* d);
int tamgcn_conv(const tamgcn_conv_desc* d, void* stream);

/* ReLU sign bits.  The forward kernels that apply a ReLU can leave one bit per element (1 iff the stored value is > 0;
 * -0.0, +0.0 and NaN give 0) beside their output, so that the backward reads 1/16 of a tensor pass instead of the activation.
 * Layout of the bits of an (N, C, T, V) tensor: every (n, c) row of L = T*V floats has ceil(L / 4) bytes; byte i of a row
 * holds elements 4i .. 4i+3 in bits 0 .. 3 (bits 4 .. 7 are 0).  Row (n, c) starts at byte (n*C + c) * ceil(L / 4).
 *
 * tamgcn_conv_signmask: tamgcn_conv with  y *= bit  in place of  y *= (mask_src > 0)  -- after bias, broadcast, add1 and
 * add2, before the moments and the store; `bits` has bctot channels of T_y*V elements and row m of the output uses channel
 * bcoff + m.  Served by the two-source, stride-1 form of the LDS-DMA GEMM only (V % 4 == 0, K % 16 == 0, no fp32 mask, no
 * output affine, ostride 1, split mode 0 or M < 128); anything else is refused: mask with the element-wise kernels instead.
 * Every element equals the one tamgcn_conv writes, or 0. */
int tamgcn_conv_signmask(const tamgcn_conv_desc* d, const unsigned char* bits, int bctot, int bcoff, void* stream);

/* Weight gradient of the same convolution (aten::convolution_backward, weight part):
 *   dW[m][k][j] = sum_{n,t,v} gy(n,m,t,v) * src(n,k,t*stride + j*dil - pad, v)
 * Both operands go through the prologue.  Split over n into `nsplit` partial
 * slabs (deterministic: no float atomics), reduced by tamgcn_reduce_sum. */
typedef struct tamgcn_wgrad_desc {
    tamgcn_src gy;                  /* (N, gy.ctot, T_out, V), M channels from gy.coff */
    tamgcn_src src;                 /* (N, src.ctot, T_in, V), K channels from src.coff */
    int N, M, K, T_in, T_out, V, KT, dil, stride, pad;
    float* part;                    /* [nsplit][M][K][KT] */
    int nsplit;
} tamgcn_wgrad_desc;
/* Largest nsplit tamgcn_wgrad accepts for this descriptor: N, or more when the contraction can also be
 * split inside a sample (1x1 stride-1 form).  Size `part` and nsplit from it. */
int tamgcn_wgrad_max_split(const tamgcn_wgrad_desc* d);
int tamgcn_wgrad(const tamgcn_wgrad_desc* d, void* stream);

/* Two stride-1 1x1 convolutions of the same tensor as one launch (MS-TCN: the stacked entry convolutions W0 and the plain
 * 1x1 branch W1 both read g):   [y0; y1] = [W0; W1] . act(src) + [bias0; bias1]
 * Rows [0, M0) go to (y0, yctot0, ycoff0) and the moment slice (stats_part0, stats_ctot0, stats_coff0), rows [M0, M0 + M1)
 * to their own; w0 [M0][K], w1 [M1][K].  Runs the LDS-DMA GEMM of tamgcn_conv with the tiling of the single descriptor that
 * has M = M0 + M1; a shape that kernel does not serve is refused.  Every output element and every moment partial is
 * bit-identical to the two tamgcn_conv launches; the partial count is tamgcn_conv_nparts of M = M0 + M1. */
typedef struct tamgcn_conv_pair_desc {
    int N, T, V;                    /* every tensor is (N, *, T, V) */
    int stride;                     /* must be 1 (a strided plain branch computes every other frame: two launches) */
    tamgcn_src src;
    int K, M0, M1;
    const float* w0; const float* w1;
    const float* bias0; const float* bias1;   /* optional */
    float* y0; int yctot0, ycoff0;
    float* y1; int yctot1, ycoff1;
    float* stats_part0; int stats_ctot0, stats_coff0;   /* optional; both or neither */
    float* stats_part1; int stats_ctot1, stats_coff1;
} tamgcn_conv_pair_desc;
int tamgcn_conv_pair(const tamgcn_conv_pair_desc* d, void* stream);

/* Two weight gradients against the same src as one launch: rows [0, M0) of the gradient operand come from gy0, rows
 * [M0, M0 + M1) from gy1 (both with the two-source BatchNorm-backward prologue); part [nsplit][M0 + M1][K].
 * nsplit <= tamgcn_wgrad_max_split of the tamgcn_wgrad_desc with M = M0 + M1.  M0 % 8 == 0.  At the nsplit of a
 * single tamgcn_wgrad launch the rows hold that launch's bits (a row's sum does not depend on the rows beside it). */
typedef struct tamgcn_wgrad_pair_desc {
    tamgcn_src gy0, gy1, src;
    int N, M0, M1, K, T, V;
    int stride;                     /* must be 1 */
    float* part;
    int nsplit;
} tamgcn_wgrad_pair_desc;
int tamgcn_wgrad_pair(const tamgcn_wgrad_pair_desc* d, void* stream);

/* Several slab reductions in ONE launch (a layer's backward produces ~25 of them; the sums over (n, t, v) of aten's
 * convolution_backward / native_batch_norm_backward for the modules of reference models/ctrgcn.py:53-284): for each descriptor
 * out[e] (+)= scale * sum_s part[s*stride_s + e], fp64 accumulation in a fixed order. */
typedef struct tamgcn_reduce_desc {
    const float* part; float* out;
    int nsplit, accumulate;
    long long stride_s, count;
    float scale;
} tamgcn_reduce_desc;
int tamgcn_reduce_multi(const tamgcn_reduce_desc* descs, int n, void* stream);

/* out[e] = (accumulate ? out[e] : 0) + scale * sum_{s<nsplit} part[s*stride_s + e]
 * (fp64 accumulation, fixed order).  `part` is scratch: for nsplit > 128 it is reduced in place first. */
int tamgcn_reduce_sum(float* part, int nsplit, long long stride_s, long long count,
                      float scale, int accumulate, float* out, void* stream);

/* ------------------------------------------------------------------------
 * BatchNorm bookkeeping (aten::native_batch_norm / _backward,
 * reference nn.BatchNorm2d at models/ctrgcn.py:64,100,115,118,123,186,213,221,230)
 * ---------------------------------------------------------------------- */
/* training=1: mean/var from partial sums [2][part_ctot][nparts] (channels part_coff..+C),
 *             running stats updated (momentum, unbiased var), *nbt += 1;
 * training=0: running stats used.
 * Writes coef (c1 = gamma*invstd, c2 = 0, c0 = beta - mean*c1) at channels coef_coff..+C of
 * a [3][coef_ctot] array and save = (mean, invstd) at the same channels of a [2][coef_ctot] array. */
int tamgcn_bn_fwd_finalize(const float* part, int part_ctot, int part_coff, int nparts, double count,
                           const float* gamma, const float* beta,
                           float* running_mean, float* running_var, long long* num_batches_tracked,
                           float momentum, float eps, int training,
                           float* coef, float* save, int coef_ctot, int coef_coff, int C, void* stream);

/* Coefficients of unit_gcn's offset_conv input diff = down(x) - bn(y) (reference models/ctrgcn.py:256-258) as a two-source
 * prologue c1*x1 + c2*x2 + c0 from the [3][C] sets tamgcn_bn_fwd_finalize wrote for down's BatchNorm (coef_d) and bn (coef_y):
 *   mode 0 (x1 = down's conv output, x2 = y):  (cd[0], -cy[0], cd[2] - cy[2])
 *   mode 1 (down = identity, x1 = x, x2 = y):  (1, -cy[0], -cy[2])          mode 2 (no residual, x1 = y):  (-cy[0], 0, -cy[2]) */
int tamgcn_coef_diff(const float* coef_d, const float* coef_y, float* out, int C, int mode, void* stream);

/* part = [2][part_ctot][nparts] partial sums of (dz, dz*(x_pre - mean)) per channel; every backward
 * reducer below centres by the saved batch mean (save[0]) so that dgamma has no cancellation.
 * Produces dgamma, dbeta, the bias gradient of the conv that fed the BN (optional) and the
 * backward-apply coefficients  d x_pre = c1*dz + c2*x_pre + c0  (train: full BN backward;
 * eval: c1 = gamma*invstd, c2 = c0 = 0). */
int tamgcn_bn_bwd_finalize(const float* part, int part_ctot, int part_coff, int nparts, double count,
                           const float* gamma, const float* save, int save_ctot, int save_coff,
                           int training, float* dgamma, float* dbeta, float* dbias_conv,
                           float* coef, int coef_ctot, int coef_coff, int C, void* stream);

/* Several BatchNorms in one launch: the same arithmetic as the two entry points above, one descriptor per BatchNorm
 * (fields = their arguments).  A block's forward finalises ~11 BatchNorms and its backward ~9; the ones whose partial sums
 * are ready together share a launch. */
typedef struct tamgcn_bn_fwd_desc {
    const float* part; int part_ctot, part_coff, nparts; double count;
    const float* gamma; const float* beta; float* running_mean; float* running_var; long long* num_batches_tracked;
    float momentum, eps; int training;
    float* coef; float* save; int coef_ctot, coef_coff, C;
} tamgcn_bn_fwd_desc;
typedef struct tamgcn_bn_bwd_desc {
    const float* part; int part_ctot, part_coff, nparts; double count;
    const float* gamma; const float* save; int save_ctot, save_coff, training;
    float* dgamma; float* dbeta; float* dbias_conv; float* coef; int coef_ctot, coef_coff, C;
} tamgcn_bn_bwd_desc;
int tamgcn_bn_fwd_finalize_multi(const tamgcn_bn_fwd_desc* descs, int n, void* stream);
int tamgcn_bn_bwd_finalize_multi(const tamgcn_bn_bwd_desc* descs, int n, void* stream);

/* ------------------------------------------------------------------------
 * CTRGC — channel-wise topology refinement graph convolution
 * (reference models/ctrgcn.py:172-177, and the 3-subset sum :252-254).
 * ---------------------------------------------------------------------- */
/* xbar[c][n][v] = mean_t src(n,c,t,v)   (layout (C, N, V): one "sample" with T = N, so the
 * pooled 1x1 convs conv1/conv2 run through tamgcn_conv with N=1, T=N). */
int tamgcn_tmean(const tamgcn_src* src, int N, int C, int T, int V, float* xbar, void* stream);

typedef struct tamgcn_ctrgc_desc {
    int N, Cin, Cout, S, R, T, V;
    tamgcn_src x;                   /* block input (N, Cin, T, V) */
    const float* pq;                /* [S*2*R][N][V]: row (s*2+0)*R+r = p, (s*2+1)*R+r = q  (conv1/conv2 of xbar) */
    const float* w3;                /* [S*Cout][Cin]  conv3 weights, subsets stacked */
    const float* b3;                /* [S*Cout] */
    const float* w4;                /* [S][Cout][R]   conv4 */
    const float* b4;                /* [S][Cout] */
    const float* A;                 /* [S][V][V]      PA (or the A given to CTRGC.forward) */
    const float* alpha;             /* [1] device scalar */
    const float* E;                 /* (N, S, Cout, V, V) from tamgcn_ctrgc_build_e: fwd / bwd_dx3 load their E tiles from it */
} tamgcn_ctrgc_desc;

/* E[n,s,c,u,v] = alpha*(W4_s tanh(p_s[n,:,u] - q_s[n,:,v]) + b4_s)[c] + A_s[u,v] for every channel, once per
 * layer and sample (R <= 32): reference models/ctrgcn.py:174-176 (tanh of the pairwise difference, conv4, * alpha + A); pass it as d->E to tamgcn_ctrgc_fwd and tamgcn_ctrgc_bwd_dx3. */
int tamgcn_ctrgc_build_e(const tamgcn_ctrgc_desc* d, float* E, void* stream);

/* y[n,c,t,u] = sum_s sum_v E_s[n,c,u,v] * (W3_s x + b3_s)[n,c,t,v],  E_s = d->E (V = 20, S in {1, 3}, Cout % 8 == 0;
 * other joint counts: the tamgcn_ctrgc_tiled_* family below).  d->pq, w4, b4, A, alpha are not read.
 * stats_part (optional): [2][Cout][N] partial (sum y, sum y^2) per sample.
 * x3_out (optional): (N, S*Cout, T, V) receives x3 = W3 x + b3 (the tile is in LDS anyway): the backward's dE
 * accumulation and the conv3 weight gradient read it; NULL (inference) keeps the forward write-minimal. */
int tamgcn_ctrgc_fwd(const tamgcn_ctrgc_desc* d, float* y, float* stats_part, float* x3_out, void* stream);

/* dx3[n, s*Cout+c, t, v] = sum_u E_s[n,c,u,v] * dy(n,c,t,u);  db3_part [N][S*Cout];  E_s = d->E, d->w3 / b3 not read */
int tamgcn_ctrgc_bwd_dx3(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy,
                         float* dx3, float* db3_part, void* stream);

/* dE_s[n,c,u,v] = sum_t dy(n,c,t,u) * x3_s[n,c,t,v] pushed through E's definition (autograd of reference
 * models/ctrgcn.py:172-177 w.r.t. PA, alpha, conv4, conv1/conv2 outputs), from the x3 tamgcn_ctrgc_fwd kept (x3_out), as two launches:
 *   _de_acc   dE (N, S, Cout, V, V) = sum_t dy(n,c,t,u) * x3[n, s*Cout+c, t, v]     (streaming, HBM-bound)
 *   _de_tail  one workgroup per (n, s, channel group g of `groups`): dA_part [N*groups][S][V][V],
 *             dw4_part [N][S][Cout][R], db4_part [N][S][Cout], dalpha_part [N*S*groups],
 *             dpq [groups][S*2*R][N][V] (plain stores: every workgroup owns its slice, nothing to zero;
 *             sum the slabs over `groups`).  R <= 32, Cout % (16*groups) == 0.
 * d->x and d->w3/b3 are not read by either. */
int tamgcn_ctrgc_bwd_de_acc(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* x3,
                            float* dE, void* stream);
int tamgcn_ctrgc_bwd_de_tail(const tamgcn_ctrgc_desc* d, const float* dE,
                             float* dA_part, float* dw4_part, float* db4_part,
                             float* dalpha_part, float* dpq, int groups, void* stream);

/* ---- CTRGC for large skeletons (V in {32, 64}; BASELINE.json configs[4]: V = 64, T = 512, C = 256) ---------------
 * One channel's topology E is 3*V*V floats (48 KB at V = 64): the fused LDS-resident kernels above do not apply
 * (tamgcn_ctrgc_lds_bytes < 0).  The same arithmetic (reference models/ctrgcn.py:172-177, V-generic) then runs as
 *   x3 = W3 x + b3                  tamgcn_conv (M = S*Cout), kept in HBM: (N, S*Cout, T, V)
 *   _tiled_build_e                  E (N, S, Cout, V, V), workgroup = (n, s, 512/V rows u)
 *   _tiled_agg_fwd                  y[n,c,t,u] = sum_s sum_v x3_s[n,c,t,v] E_s[n,c,u,v] on MFMA; stats_part [2][Cout][N] optional
 *   _tiled_agg_bwd                  dx3[n,s*Cout+c,t,v] = sum_u dy(n,c,t,u) E_s[n,c,u,v]; db3_part [N][S*Cout] optional
 *   _tiled_de_acc                   dE (N, S, Cout, V, V) = sum_t dy(n,c,t,u) x3[n,s*Cout+c,t,v]
 *   _tiled_de_tail                  dE -> dA_part [N][S][V][V], dw4_part [N*NUC][S][Cout][R], db4_part [N*NUC][S][Cout],
 *                                   dalpha_part [N*S*NUC], dpq [NUC][S*2*R][N][V] (sum the slabs over NUC);
 *                                   NUC = tamgcn_ctrgc_tiled_chunks(V) row chunks of E per (n, s).  R <= 32.
 * d->x, d->w3, d->b3, d->E are not read by these entry points (E and x3 are explicit arguments). */
int tamgcn_ctrgc_tiled_supported(int V);
int tamgcn_ctrgc_tiled_chunks(int V);
int tamgcn_ctrgc_tiled_build_e(const tamgcn_ctrgc_desc* d, float* E, void* stream);
int tamgcn_ctrgc_tiled_agg_fwd(const tamgcn_ctrgc_desc* d, const float* x3, const float* E, float* y, float* stats_part, void* stream);
int tamgcn_ctrgc_tiled_agg_bwd(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* E, float* dx3, float* db3_part, void* stream);
int tamgcn_ctrgc_tiled_de_acc(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* x3, float* dE, void* stream);
int tamgcn_ctrgc_tiled_de_tail(const tamgcn_ctrgc_desc* d, const float* dE, float* dA_part, float* dw4_part, float* db4_part,
                               float* dalpha_part, float* dpq, void* stream);

/* ---- CTRGC for any skeleton of 2 <= V <= 32 joints (a user's own graph: COCO 17, OpenPose 18, hands 21, ...) --------
 * The kernels of the V = 25 route with V as a run-time argument (csrc/vgen.hip): joints padded to 16 or 32 inside the
 * kernels' LDS images, never in HBM.  Same arithmetic, tensors and partial layouts as the entry points they stand beside:
 *   _vgen_build_e    as tamgcn_ctrgc_build_e          E (N, S, Cout, V, V), workgroup = (n, s)
 *   _vgen_agg_fwd    as tamgcn_ctrgc_tiled_agg_fwd    x3 (N, S*Cout, T, V) from tamgcn_conv
 *   _vgen_agg_bwd    as tamgcn_ctrgc_tiled_agg_bwd
 *   _vgen_de_acc     as tamgcn_ctrgc_tiled_de_acc
 *   _vgen_de_tail    as tamgcn_ctrgc_bwd_de_tail      (channel groups, dpq [groups][S*2*R][N][V])
 * S in {1, 3}, Cout % 16 == 0, R a multiple of 4 up to 32.  V = 20, 25 and 32 are accepted too (the library's own
 * routing keeps their dedicated kernels).  x3 and dy are read in 16-byte pieces from dword-aligned rows: READ SLACK (top of
 * this file) applies to them.  E is loaded element by element and needs none.
 * tamgcn_vgen_supported: 1 for 2 <= V <= 32, else 0.  tamgcn_vgen_lds_bytes: the family's largest dynamic-LDS request
 * for (S, V, R), < 0 outside its range. */
int tamgcn_vgen_supported(int V);
int tamgcn_vgen_lds_bytes(int S, int V, int R);
int tamgcn_vgen_build_e(const tamgcn_ctrgc_desc* d, float* E, void* stream);
int tamgcn_vgen_agg_fwd(const tamgcn_ctrgc_desc* d, const float* x3, const float* E, float* y, float* stats_part, void* stream);
int tamgcn_vgen_agg_bwd(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* E, float* dx3, float* db3_part, void* stream);
int tamgcn_vgen_de_acc(const tamgcn_ctrgc_desc* d, const tamgcn_src* dy, const float* x3, float* dE, void* stream);
int tamgcn_vgen_de_tail(const tamgcn_ctrgc_desc* d, const float* dE, float* dA_part, float* dw4_part, float* db4_part,
                        float* dalpha_part, float* dpq, int groups, void* stream);

/* ------------------------------------------------------------------------
 * Element-wise block epilogues and their backward reductions.
 * All stats partial buffers are [nstat][C][nparts]; nparts is returned by
 * tamgcn_ew_nparts(N, T, V) (one partial per (n, chunk of t)).
 * ---------------------------------------------------------------------- */
int tamgcn_ew_nparts(int N, int C, int T, int V);

/* unit_gcn tail, models/ctrgcn.py:256-261:
 *   g = relu( ybn + tanh(obn) + res ),  ybn = y.coef-applied y_pre, obn likewise,
 *   res = 0 | x | coef-applied d_pre  (res may be NULL). */
int tamgcn_gcn_tail_fwd(const tamgcn_src* y, const tamgcn_src* o, const tamgcn_src* res,
                        int N, int C, int T, int V, float* g, void* stream);
/* dsum = dg*(g>0); doz = dsum*(1-tanh(obn)^2); partials (sum doz, sum doz*(o_pre - o_save[c])) */
int tamgcn_gcn_tail_bwd(const float* dg, const float* g, const tamgcn_src* o, const float* o_save,
                        int N, int C, int T, int V, float* dsum, float* doz, float* part, void* stream);
/* The same two with sign bits (layout: see tamgcn_conv_signmask).  _fwd_bits also writes the bits of g.  _bwd_bits takes
 * them in place of g; with bits == NULL and dsum == NULL, dg IS dsum already (its producer masked it: tamgcn_conv_signmask)
 * and only doz and the partials are written.  Every output holds the bits tamgcn_gcn_tail_fwd / _bwd write. */
int tamgcn_gcn_tail_fwd_bits(const tamgcn_src* y, const tamgcn_src* o, const tamgcn_src* res,
                             int N, int C, int T, int V, float* g, unsigned char* bits, void* stream);
int tamgcn_gcn_tail_bwd_bits(const float* dg, const unsigned char* bits, const tamgcn_src* o, const float* o_save,
                             int N, int C, int T, int V, float* dsum, float* doz, float* part, void* stream);
/* dyb = dsum - ddiff ; dres = dsum + ddiff (dres optional);
 * part[0..1] = (sum dyb, sum dyb*y_pre); part[2..3] = (sum dres, sum dres*r_pre) if r_pre given */
int tamgcn_gcn_mid_bwd(const float* dsum, const float* ddiff, const float* y_pre, const float* y_save,
                       const float* r_pre, const float* r_save,
                       int N, int C, int T, int V, float* dyb, float* dres, float* part, void* stream);

/* ------------------------------------------------------------------------
 * The second stage of MultiScale_TemporalConv in one launch per direction (reference models/ctrgcn.py:52-69, 101-119,
 * 137-147; backward: aten::convolution_backward's input gradient of every branch's k x 1 convolution).
 *   forward   for b < nb:  y[:, ycoff + b*Cb + m, t] = bias_b[m] + sum_{k, tap} W_b[m][k][tap] *
 *                              act(src)[:, src.coff + b*Cb + k, t*stride + tap*dil_b - (KT-1)*dil_b/2]      (zero padded)
 *             pool = 1:    y[:, ycoff + nb*Cb + c, t] = max_{i in -1..1} act(src)[:, src.coff + nb*Cb + c, t*stride + i]
 *             stats_part (optional) [2][stats_ctot][nparts]: (sum y, sum y^2) per workgroup at the channels of y.
 *             The prologue must be BatchNorm + ReLU (src.act = 1, no second source).
 *   backward  src = the gradient w.r.t. y, (N, src.ctot, T_out, V), linear two-source prologue (act = 0);
 *             for b < nb:  y[:, ycoff + b*Cb + k, th] = [mask value > 0] * sum_{m, tap, t: t*stride + tap*dil_b - pad_b = th}
 *                              W_b[m][k][tap] * src value[:, src.coff + b*Cb + m, t],        y has T_in frames;
 *             mask = the forward's source with its prologue (channel mask.coff + b*Cb + k); stats_part: (sum y,
 *             sum y * (mask.x1 - center[channel])), the entry BatchNorm's backward moments.  pool is ignored (the pooled
 *             branch's gradient is tamgcn_maxpool_bwd).
 * Built for Cb = 16, 32 or a multiple of 64, KT in {3, 5}, (KT-1)*dil even, V <= 32 or V % 16 == 0, stride 1 or 2:
 * tamgcn_tconv_supported() says whether a shape is (Cb = 96 is not: the weight gradient alone takes any multiple of 32);
 * w_b = [Cb][Cb][KT] as nn.Conv2d stores it. */
#define TAMGCN_TCONV_MAXB 6
typedef struct tamgcn_tconv_desc {
    tamgcn_src src;
    int N, T_in, T_out, V, Cb, nb, KT, stride, pool;     /* T_in: frames of the forward's input, T_out = (T_in-1)/stride + 1 */
    int dil[TAMGCN_TCONV_MAXB];
    const float* w[TAMGCN_TCONV_MAXB];
    const float* bias[TAMGCN_TCONV_MAXB];                /* forward only; entries may be NULL */
    float* y; int yctot, ycoff;
    float* stats_part; int stats_ctot;
    const tamgcn_src* mask; const float* center;         /* backward only */
} tamgcn_tconv_desc;
int tamgcn_tconv_supported(int V, int Cb, int KT, int nb, const int* dil, int stride, int T_in);
int tamgcn_tconv_nparts(const tamgcn_tconv_desc* d, int backward);
int tamgcn_tconv_fwd(const tamgcn_tconv_desc* d, void* stream);
int tamgcn_tconv_bwd(const tamgcn_tconv_desc* d, void* stream);
/* Weight gradient of every temporal branch in one launch (aten::convolution_backward, weight part):
 *   dW_b[m][k][tap] = sum_{n,t,v} gy(n, src.coff + b*Cb + m, t, v) * act(mask)(n, mask.coff + b*Cb + k, t*stride + tap*dil_b - pad_b, v)
 * d->src = the gradient w.r.t. the branches' outputs (two-source prologue, T_out frames), d->mask = the forward's source with
 * its prologue (T_in frames).  The contraction is split over (sample, frame tile) items into nsplit = d->yctot partial slabs
 * d->y = part [nsplit][nb][Cb][Cb][KT] (deterministic: no float atomics; reduce with tamgcn_reduce_*);
 * 1 <= nsplit <= tamgcn_tconv_wgrad_max_split(d).  Shapes: as tamgcn_tconv_supported(). */
int tamgcn_tconv_wgrad_max_split(const tamgcn_tconv_desc* d);
int tamgcn_tconv_wgrad(const tamgcn_tconv_desc* d, void* stream);

/* MaxPool2d((3,1), stride (s,1), pad (1,0)) over the prologue value (models/ctrgcn.py:117),
 * written at channel ycoff of y (N, yctot, T_out, V) + (sum, sum^2) partials [2][yctot][nparts]. */
int tamgcn_maxpool_fwd(const tamgcn_src* src, int N, int C, int T_in, int V, int stride,
                       float* y, int yctot, int ycoff, int T_out, float* stats_part, void* stream);
/* the same pooled value finished for an eval-mode block (row f2):  y = act( c1[ch]*maxpool + c0[ch] + add ),
 * ch = ycoff + c, coef [3][yctot] as tamgcn_bn_fwd_finalize writes it, add optional with the geometry of y. */
int tamgcn_maxpool_post_fwd(const tamgcn_src* src, int N, int C, int T_in, int V, int stride,
                            float* y, int yctot, int ycoff, int T_out, const float* coef, const float* add, int relu, void* stream);
/* d src_value routed to the first arg-max of each window, times relu mask (value > 0);
 * gy goes through its own prologue (gy->act != 0 is honoured, on the staged kernel); result written at channel dcoff of d (N, dctot, T_in, V),
 * partials (sum d, sum d*src.x1) at the same channel of [2][dctot][nparts]. */
int tamgcn_maxpool_bwd(const tamgcn_src* gy, const tamgcn_src* src, const float* src_save, int N, int C, int T_in, int T_out, int V,
                       int stride, float* d, int dctot, int dcoff, float* part, void* stream);

/* out = act( a + res ), a = prologue value of `a`, res = NULL | src (identity or coef-applied
 * conv residual); models/ctrgcn.py:145-146 and :283.  rowmean: NULL | [N][C], the mean over (t, v) of every
 * output row -- the last block hands the model head its pooling input (models/ctrgcn.py:343-345) this way.
 * xbar: NULL | [C][N][V], the mean over t of `out` -- the NEXT block's pooled joint-embedding input (what tamgcn_tmean
 * computes, models/ctrgcn.py:172-174), taken while the row is in registers; needs V % 4 == 0, V <= 64, 16-byte aligned
 * operands and rowmean == NULL. */
int tamgcn_add_act_fwd(const tamgcn_src* a, const tamgcn_src* res, int relu,
                       int N, int C, int T, int V, float* out, float* rowmean, float* xbar, void* stream);
/* dz = dout * (out>0) (relu=1; dz may be NULL when relu=0 and only sums are wanted);
 * part[0..1] = (sum dz, sum dz*a_pre), part[2..3] = (sum dz, sum dz*r_pre) if r_pre given. */
int tamgcn_add_act_bwd(const float* dout, const float* out, int relu, const float* a_pre, const float* a_save,
                       const float* r_pre, const float* r_save,
                       int N, int C, int T, int V, float* dz, float* part, void* stream);
/* relu = 1 with sign bits (layout: see tamgcn_conv_signmask): _fwd_bits also writes the bits of `out`, _bwd_bits takes them
 * in place of `out`.  Every output holds the bits tamgcn_add_act_fwd / _bwd write. */
int tamgcn_add_act_fwd_bits(const tamgcn_src* a, const tamgcn_src* res,
                            int N, int C, int T, int V, float* out, float* rowmean, float* xbar, unsigned char* bits, void* stream);
int tamgcn_add_act_bwd_bits(const float* dout, const unsigned char* bits, const float* a_pre, const float* a_save,
                            const float* r_pre, const float* r_save,
                            int N, int C, int T, int V, float* dz, float* part, void* stream);

/* Dropout inside the residual tail (st_gcn with an active Dropout, models/stgcn.py:77-99): out = act(keep * a * scale + res) in
 * _add_act_fwd's single pass.  Added in ABI 401 without a version bump: new entry points, no existing layout or semantics changed.
 * The draw.  state int64 [2] = (seed, call) on the device; both words are READ ON THE DEVICE, so a HIP graph holding the call
 *   sees their current values.  For the site tensor (N, C, T, V): row r = n * C + c, L = T * V, group g = i >> 2 of position
 *   i in the row.  Philox4x32-10 with key = (seed low, seed high) and counter = (call low, call high, r, (site << 20) | g);
 *   word e of the result decides element 4g + e, which is KEPT iff word >= thr.  thr = floor(p 2^32), computed by the caller
 *   in fp64; scale = float32(1 / (1 - p)), computed in fp64 and rounded once.  A kept element is fl32(a * scale), a = the
 *   value of the source descriptor `a` (fma(c1, z, c0) for a BatchNorm-applied tensor); a dropped element is +0.  One forward
 *   pass uses one value of `call` for all its sites, which differ in `site`.  Refused before any launch: L > 2^22 (g < 2^20
 *   shares its counter word with the site), site outside 0 .. 4095, a scale that is not a finite value >= 1.
 * _drop_add_act_fwd  res: NULL (a block without residual) | src.  bits: NULL | the array of tamgcn_conv_signmask's layout, one
 *   byte per four floats of a row: LOW nibble = the sign bits of `out` as _add_act_fwd_bits writes them (zero when relu = 0),
 *   HIGH nibble = the keep bits of the same four elements.
 * _drop_add_act_bwd  d = dout under the sign nibble (relu = 1; dout itself otherwise); dza = fl32(d * scale) where the element
 *   was kept, 0 elsewhere; dzr = d (NULL: not written; required with r_pre).  part (NULL iff a_pre and r_pre are NULL) has
 *   _add_act_bwd's layout: part[0..1] = (sum dza, sum dza (a_pre - a_save[c])), and with r_pre part[2..3] = (sum d,
 *   sum d (r_pre - r_save[c])).  Draws nothing: it reads the bits.  Sums in a fixed order, no atomics.
 * _dropout_advance   call += 1 in a one-thread launch on the stream (plain store), to follow the last site of a forward pass. */
int tamgcn_drop_add_act_fwd(const tamgcn_src* a, const tamgcn_src* res, int relu, int N, int C, int T, int V,
                            const long long* state, int site, unsigned thr, float scale, float* out, unsigned char* bits, void* stream);
int tamgcn_drop_add_act_bwd(const float* dout, const unsigned char* bits, int relu, float scale, const float* a_pre, const float* a_save,
                            const float* r_pre, const float* r_save, int N, int C, int T, int V, float* dza, float* dzr, float* part,
                            void* stream);
int tamgcn_dropout_advance(long long* state, void* stream);

/* y = prologue value (materialise a src; used by stand-alone modules and tests) */
int tamgcn_apply(const tamgcn_src* src, int N, int C, int T, int V, float* y, int yctot, int ycoff, void* stream);

/* ---- stem and head of models.ctrgcn.Model (reference models/ctrgcn.py:328-332, 343-348) -------------------------
 * stem: x (N, C, T, V, M) -> data_bn over channel j = (m*V + v)*C + c with statistics over (n, t) -> (N*M, C, T, V).
 *   _stem_stats  part [2][J][N], J = C*V*M: (sum a, sum a*(b - center[j])) over t; forward a = b = x, center NULL (moments
 *                for tamgcn_bn_fwd_finalize); backward a = dout (N*M, C, T, V), b = x, center = saved mean (for _bn_bwd_finalize)
 *   _stem_apply  dout NULL: out (N*M, C, T, V) = c1[j]*x + c0[j];  dout given: out = dx (N, C, T, V, M) = c1*dout + c2*x + c0
 * head: pooled (N, C) = mean over (m, t, v) of x10 (N*M, C, T, V); logits (N, K) = pooled W^T + b and their gradients. */
int tamgcn_stem_stats(const float* x, const float* dout, const float* center, int N, int C, int T, int V, int M,
                      float* part, void* stream);
int tamgcn_stem_apply(const float* x, const float* dout, const float* coef, int N, int C, int T, int V, int M,
                      float* out, void* stream);
int tamgcn_head_pool_fwd(const float* x, int N, int C, int T, int V, int M, float* pooled, void* stream);
int tamgcn_head_pool_bwd(const float* dpooled, int N, int C, int T, int V, int M, float* dx, void* stream);
int tamgcn_head_fc_fwd(const float* pooled, const float* W, const float* b, int N, int C, int K, float* logits, void* stream);
int tamgcn_head_fc_bwd(const float* dlogits, const float* pooled, const float* W, int N, int C, int K,
                       float* dW, float* db, float* dpooled, void* stream);

/* ---- loss of the harness step (nn.CrossEntropyLoss(), reduction 'mean', ignore_index -100: reference
 *      processor/recognition_rgb.py:19, :62) ----
 * _ce_fwd  loss[0] = mean over the KEPT rows of (logsumexp(logits[n]) - logits[n][labels[n]]); g (N, K) = (softmax - onehot) / kept
 *          (kept for the backward).  labels int64 on the device: a row labelled -100 (torch's default ignore_index) is skipped
 *          -- zero gradient, not counted; the loss is NaN when no row is kept, as torch's is.  Any other label outside
 *          [0, K), where torch raises a device assert, makes loss[0] NaN and zeroes that row of g; nothing outside the
 *          row is read.  One launch (aten: log_softmax + nll_loss).
 * _ce_bwd  dlogits = g * dloss[0]   (aten: nll_loss_backward + log_softmax_backward). */
int tamgcn_ce_fwd(const float* logits, const long long* labels, int N, int K, float* loss, float* g, void* stream);
int tamgcn_ce_bwd(const float* g, const float* dloss, int N, int K, float* dlogits, void* stream);

/* ---- the same loss with torch.nn.CrossEntropyLoss's options (added in ABI 401 without a version bump; csrc/celoss.hip) ----
 * Notation per row n: logp = l - lse(l), p = softmax(l), w_k the class weight (1 when weight is NULL), Wsum = sum_k w_k,
 * eps = label_smoothing.  Exactly one of labels / probs is given.
 *   labels (N) int64   a row is KEPT iff labels[n] != ignore_index (any integer, a valid class id included; that class still
 *                      takes part in the other rows' smoothing sums).
 *                        L_n = (1 - eps) w_y (-logp_y) + (eps / K) sum_k w_k (-logp_k);   0 on ignored rows
 *                        dL_n/dl_j = p_j [(1 - eps) w_y + (eps / K) Wsum] - (1 - eps) w_y [j = y] - (eps / K) w_j;   exactly 0 on ignored rows
 *                      eps = 0 does not evaluate the smoothing sum (no 0 * inf).  'mean' divides both by W = sum over the kept
 *                      rows of w_y, with or without weights and smoothing: no kept row, or kept weights that sum to 0, give NaN.
 *                      A label outside [0, K) that is not ignore_index follows tamgcn_ce_fwd: the reduced loss is NaN, with 'none'
 *                      that row's loss is NaN, that row of g is 0, the row counts nothing towards W and nothing outside the
 *                      row is touched.
 *   probs (N, K) fp32  t' = (1 - eps) t + eps / K;  L_n = -sum_k w_k t'_k logp_k;  dL_n/dl_j = p_j sum_k w_k t'_k - w_j t'_j;
 *                      'mean' divides by N; ignore_index plays no part.
 *   reduction          TAMGCN_CE_MEAN: loss[0] = sum_n L_n / W;  TAMGCN_CE_SUM: loss[0] = sum_n L_n;  TAMGCN_CE_NONE: loss[n] = L_n.
 *   g (N, K)           the final gradient for dloss = 1 (the division by W or N included).  The backward is one product per
 *                      element: tamgcn_ce_bwd (g * dloss[0]) for 'mean' / 'sum', tamgcn_ce_opts_bwd_rows (g[n][k] * dloss[n]) for 'none'.
 * One wave per row, lanes striding over k; the max and expf(l_k - max) in fp32, the shifted sum, lse, p, every weighted sum over
 * k, the row loss and g's arithmetic in fp64 (lane partials in ascending k, then the xor butterfly 1, 2, .., 32), one rounding to
 * fp32.  The sums
 * over rows (the loss terms, W) are fp64 in a fixed order (thread t of 256 takes rows t, t + 256, ..; tree): no floating-point
 * atomics, two runs are bit-equal.  W is computed on the device from the labels of the launch at hand, so a graph replay with
 * other labels is normalised by its own W.  Launches: 'none' one; 'mean' / 'sum' two (rows, then one workgroup that reduces).
 * workspace: tamgcn_ce_opts_workspace_bytes(d) bytes of device memory (8 N for 'mean' / 'sum', 0 for 'none': NULL is taken then),
 * 8-byte aligned, overwritten by every call.  _workspace_bytes returns -1 for a descriptor _fwd would reject.
 * Rejected before any launch, with the entry point and the offending value in tamgcn_last_error(): null pointers, both or
 * neither of labels / probs, N or K < 1, label_smoothing outside [0, 1], an unknown reduction, N * K >= 2^31. */
#define TAMGCN_CE_MEAN 0
#define TAMGCN_CE_SUM 1
#define TAMGCN_CE_NONE 2
typedef struct tamgcn_ce_desc {
    const float* logits;            /* (N, K) */
    const long long* labels;        /* (N) class indices, or NULL */
    const float* probs;             /* (N, K) class probabilities, or NULL */
    const float* weight;            /* (K) class weights, or NULL */
    long long ignore_index;
    double label_smoothing;
    int reduction;                  /* TAMGCN_CE_* */
    int N, K;
} tamgcn_ce_desc;
long long tamgcn_ce_opts_workspace_bytes(const tamgcn_ce_desc* d);
int tamgcn_ce_opts_fwd(const tamgcn_ce_desc* d, float* loss, float* g, void* workspace, void* stream);
int tamgcn_ce_opts_bwd_rows(const float* g, const float* dloss, int N, int K, float* dlogits, void* stream);

/* ---- score-level ensemble of the evaluation scripts ----
 * fused (N, K) = sum_s weights[s] * scores[s]  (softmax = 0: reference ensemble/ensemble_resnet_ctrgcn.py:50-54, score_a + alpha * score_b)
 *             or sum_s weights[s] * softmax_k(scores[s])  (softmax = 1: ensemble/ensemble_ctrgcn_resnet_eval.py:99-106);
 * pred (N) int64 = first arg max over k (numpy.argmax); class_stats NULL | int32 [K][2] = (correct, total) per true class
 * (compute_accuracy, ensemble_ctrgcn_resnet_eval.py:217-234), needs labels (N) int64; a label outside [0, K) belongs to no
 * class row and is left out of every (correct, total) pair (the scripts' labels come from the split lists and are always
 * in range; their overall accuracy divides by len(labels) -- the Python layer does the same and raises on such a label).
 * scores is [S][N][K] contiguous. */
int tamgcn_score_fuse(const float* scores, const float* weights, int S, int N, int K, int softmax,
                      const long long* labels, float* fused, long long* pred, int* class_stats, void* stream);

/* ---- the evaluation epoch's bookkeeping on the device (reference processor/recognition_rgb.py:71-101; the per-class accuracy,
 *      confusion matrix and alpha sweep of ensemble/ensemble_ctrgcn_resnet_eval.py:217-234, :267, :421-438) ----
 * _eval_accumulate  adds ONE batch to a state the caller owns in device memory and zeroes before the first batch; one launch of
 *          one workgroup on `stream`, no synchronisation, capturable.  logits (B, K) fp32, labels (B) int64, index (B) int64 | NULL.
 *          Only the first `valid` rows count: valid_dev (int32 on the device, read by the kernel, so a graph replay can change
 *          it) if not NULL, else the host value; clamped to [0, B].  Rows n >= valid are neither read nor stored.
 *            counts int64 [4 + TAMGCN_EVAL_MAX_TOPK]  [0] batches with a kept row, [1] kept rows, [2] bad labels, [3] bad indices,
 *                                   [4 + i] rows that hit top-topk[i]
 *            sums fp64 [2]          [0] sum of the batch-mean losses, [1] sum of the per-row losses
 *            confusion int32 (K, K) row = label, column = prediction
 *            scores fp32 (num_samples, K) | NULL   row index[n] (index NULL: row base + n) = logits[n] for every n < valid; a
 *                                   row outside [0, num_samples) stores nothing and is counted in counts[3]
 *          A row is KEPT when its label is in [0, K).  Label -100 is skipped silently; any other label outside [0, K) is
 *          counted in counts[2] and makes this batch's mean loss NaN -- tamgcn_ce_fwd's conventions, and its arithmetic: the
 *          batch mean is the value tamgcn_ce_fwd returns for rows [0, valid), bit for bit (one device body, one summation
 *          order).  A batch without a kept row adds nothing to counts[0], counts[1] and sums.
 *          Prediction = first arg max (numpy.argmax).  Row n hits top-k iff #{j : s_j > s_l} + #{j > l : s_j == s_l} < k, l its
 *          label: `l in argsort(s, stable)[-k:]`, the feeder's top_k with ties in stable order; k >= K always hits.
 *          topk: nk <= TAMGCN_EVAL_MAX_TOPK host ints.  Integer state is updated with integer atomics, floating-point state
 *          by one thread; nothing outside the state is written for any label or index value.
 * _score_sweep  correct[i] (int32 [A], device) = #{n : first arg max_k (a[n][k] + alphas[i] * b[n][k]) == labels[n]} for A <=
 *          TAMGCN_SWEEP_MAX_ALPHAS host floats in one launch: tamgcn_score_fuse's arithmetic on the score sets (a, b) with
 *          weights (1, alphas[i]), softmax as there.  a, b (N, K) fp32, labels (N) int64; a label outside [0, K) is never correct. */
#define TAMGCN_EVAL_MAX_TOPK 4
#define TAMGCN_SWEEP_MAX_ALPHAS 16
int tamgcn_eval_accumulate(const float* logits, const long long* labels, const long long* index, int B, int K,
                           int valid, const int* valid_dev, const int* topk, int nk, long long base, long long num_samples,
                           long long* counts, double* sums, int* confusion, float* scores, void* stream);
int tamgcn_score_sweep(const float* a, const float* b, const float* alphas, int A, int N, int K, int softmax,
                       const long long* labels, int* correct, void* stream);

/* ---- input side: skeleton streams and the feeder's per-sample transform ----------------------
 * _stream_derive  the other three inputs of the 4-stream recipe from a joint batch x (N, C, T, V, M) resident in HBM:
 *                 mode 1 bone        out[.., v, m] = x[.., v, m] - x[.., parent[v], m]   (reference feeder/feeder_nucla_gcn.py:27-28,
 *                                    119-123: pair (v1, v2) of self.bone = (v + 1, parent[v] + 1); the pair (3, 3) gives 0)
 *                 mode 2 motion      out[:, :, t] = x[:, :, t + 1] - x[:, :, t], last frame 0          (:124-127)
 *                 mode 3 bone-motion motion of bone (upstream CTR-GCN's fourth stream; the reference feeder's `elif`
 *                                    collapses a 'bone_motion' label path to bone -- stated in DESIGN.md)
 * _feeder_transform  reference feeder/feeder_nucla_gcn.py:85-130 for N ragged clips at once, fp64 arithmetic as numpy's:
 *                 raw (sum L_n, V, 3) fp64 with frame offsets [N + 1]; centre on joint `center_joint` of frame 0 (:98-99),
 *                 p' = p . rot[n] (3 x 3 row-major view matrix Ry.Rx.S of :75-83; identity on the val path), per-coordinate
 *                 min-max to [-1, 1] over the whole clip (:102-105), gather frames idx[n][time_steps] (:108-117: the host
 *                 draws / computes the indices exactly as the reference does), stream `mode` (0 joint, 1..3 as above),
 *                 out (N, 3, time_steps, V, 1) fp32 (:129-130, :154). */
int tamgcn_stream_derive(const float* x, int N, int C, int T, int V, int M, const int* parent, int mode, float* out, void* stream);
int tamgcn_feeder_transform(const double* raw, const long long* offsets, const double* rot, const int* idx, const int* parent,
                            int N, int V, int time_steps, int center_joint, int mode, float* out, void* stream);

/* The same batch without the host: the train path's draws on the device and the transform reading the resident split.
 * Added in ABI 401 without a version bump: new entry points, no existing layout or semantics changed.
 * _feeder_draw   for B batch slots, from device memory only: offsets int64 [n_clips + 1] of the whole split, clip_ids int64
 *                 [B] (slot b takes clip clip_ids[b] mod n_clips, Python's sign rule), state int64 [2] = (seed, call counter).
 *                 Both words of state are READ ON THE DEVICE, so a HIP graph holding this call sees their current values.
 *                 train = 1 (reference :88-93, :110-115, same distributions, a counter-based stream of its own):
 *                   Philox4x32-10, key = (seed low, seed high), counter = (call low, call high, b, j);
 *                   block j = 0 -> w0..w3: agx = -60 + mulhi(w0, 121), agy = -60 + mulhi(w1, 121),
 *                   s = 0.5 + ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53;
 *                   blocks j = 1 .. ceil(time_steps / 4) -> u_0 .. u_{time_steps-1}; with n = 100 L (L = the clip's length,
 *                   position p of `list(arange(L)) * 100` holds frame p mod L) Floyd's algorithm: for i = 0 .. time_steps - 1,
 *                   J = n - time_steps + i, t = (u_i (J + 1)) >> 32, take t unless already taken, else J; idx = the
 *                   positions mod L, sorted ascending.  Then the counter advances by one in a one-thread launch that
 *                   follows the draw on the stream (plain store).  cossin: fp64 [121][2] = (cos, sin) of -60 .. 60 degrees
 *                   computed by the caller's libm, so that rot uses the host's own values.
 *                 train = 0 (:116-118): view (0, 0, 1), rot the identity, idx = np.linspace(0, L - 1, time_steps).astype(int)
 *                   in fp64 as numpy computes it (i * ((L - 1) / (time_steps - 1)) truncated, last element L - 1); state is
 *                   read by nobody and does not advance; cossin may be NULL.
 *                 Out: view fp64 [B][3] = (agx, agy, s); rot fp64 [B][9] = Ry.Rx.S row-major (each 3 x 3 product summed left
 *                 to right); idx int32 [B][time_steps]; labels_out int64 [B] = labels[clip] when both are given (both NULL:
 *                 no gather).  time_steps <= 64 (one lane per output frame).  Clip lengths must satisfy 1 <= L and
 *                 100 L < 2^24 -- the lengths live on the device, so it is the caller that checks (Feeder.load_data does).
 * _feeder_transform_indexed  _feeder_transform's arithmetic (one device body) where slot b reads clip clip_ids[b] mod n_clips
 *                 out of the resident split (raw, offsets [n_clips + 1]) instead of clip b of a gathered copy; rot [B][9],
 *                 idx [B][time_steps], out (B, 3, time_steps, V, 1). */
int tamgcn_feeder_draw(const long long* offsets, long long n_clips, const long long* clip_ids, int B, const long long* labels,
                       long long* state, const double* cossin, int time_steps, int train, double* view, double* rot, int* idx,
                       long long* labels_out, void* stream);
int tamgcn_feeder_transform_indexed(const double* raw, const long long* offsets, long long n_clips, const long long* clip_ids,
                                    const double* rot, const int* idx, const int* parent, int B, int V, int time_steps,
                                    int center_joint, int mode, float* out, void* stream);

/* ---- the feeder for fixed-shape skeleton arrays (csrc/clipfeeder.hip; tam_gcn_amd/feeder/clip_feeder.py) -------------------
 * The split is ONE resident fp32 array raw (n_clips, C, T, V, M); a batch is (B, C, W, V, M) fp32.  Reference: the pipeline of
 * feeder/feeder_nucla_fusion.py:95-106 over feeder/tools.py -- random_shift (:118-130), random_choose / auto_pading (:39-62)
 * or the centre crop, random_move (:65-115).  Added in ABI 401 without a version bump: new entry points only.
 *
 * Shift and window compose to a PLAN of three integers per slot.  With (begin, end) the clip's extent, size = end - begin,
 * bias the shift's draw on 0 .. T - size (0, begin = 0 and size = T without the shift) and d the window's offset -- the crop's
 * start on 0 .. T - W when T > W, minus the pad position on 0 .. W - T when T < W, 0 when T = W; without random_choose
 * (T - W) / 2 and 0 -- the plan is
 *     src0 = d - bias + begin,  lo = max(0, bias - d),  hi = min(W, bias + size - d):
 * output frame t is raw frame src0 + t for lo <= t < hi and zero elsewhere.
 *
 * The draw stream: Philox4x32-10, key = (seed low, seed high), counter = (call low, call high, slot b, block j); state int64 [2]
 * = (seed, call) is READ ON THE DEVICE.  flags = 1 shift | 2 choose | 4 move.
 *     block 0:      bias = mulhi(w0, T - size + 1);  d or the pad position = mulhi(w1, T - W + 1 or W - T + 1);  w2, w3 unused
 *     block 1 + i:  node i of the move: angle index mulhi(w0, nA), scale index mulhi(w1, nS), t_x index mulhi(w2, nT), t_y index
 *                   mulhi(w3, nT)
 * The call counter advances by one after the draw, in a one-thread launch that follows it on the stream (plain store), iff
 * flags != 0.
 *
 * _clip_extent    extent int32 [n_clips][2] = (begin, end): first valid frame and last valid frame + 1, a frame being valid iff
 *                 any of its C V M elements != 0 (NaN is valid, -0.0 is not); no valid frame: (0, T).  One workgroup per clip.
 * _clip_draw      clip_ids int64 [B] (slot b takes clip clip_ids[b] mod n_clips, Python's sign rule) -> plan int32 [B][3],
 *                 draws int32 [B][2] = (bias, d), and with the move: move_idx int32 [B][num_node][4] and, when keys is given
 *                 with the candidate tables angle fp64 [nA], scale [nS], trans [nT], keys fp64 [B][num_node][4] = (angle in
 *                 degrees, scale, t_x, t_y); labels_out int64 [B] = labels[clip] when both are given.
 * _clip_transform the gather: out (B, C, W, V, M) from raw, clip_ids and plan; frames the plan would take from outside the clip
 *                 or the window are clamped away, so no plan reads out of bounds.  node int32 [num_node] and keys fp64
 *                 [B][num_node][4] (both or neither) add the move: node = round_half_even(arange(0, W, W / move_time)) with
 *                 W appended; in segment [node[i], node[i+1]) the four quantities follow np.linspace(key[i], key[i+1], n)
 *                 (k (stop - start) / (n - 1) + start, last element stop, n = 1 -> start), the angle times pi, over 180; then
 *                 for EVERY frame of the window, its zero frames included, in fp64 and in this order
 *                     x' = (cos a . s) x + (-sin a . s) y + t_x,   y' = (sin a . s) x + (cos a . s) y + t_y
 *                 of channels 0 and 1 (C >= 2), rounded to fp32 once; channels >= 2 are copied.  No atomics: two calls give
 *                 the same bits. */
int tamgcn_clip_extent(const float* raw, long long n_clips, int C, int T, int V, int M, int* extent, void* stream);
int tamgcn_clip_draw(const int* extent, long long n_clips, const long long* clip_ids, int B, const long long* labels, long long* state,
                     int flags, int T, int W, int num_node, int nA, int nS, int nT, const double* angle, const double* scale,
                     const double* trans, int* plan, int* draws, int* move_idx, double* keys, long long* labels_out, void* stream);
int tamgcn_clip_transform(const float* raw, long long n_clips, const long long* clip_ids, const int* plan, const int* node,
                          const double* keys, int num_node, int B, int C, int T, int W, int V, int M, float* out, void* stream);

/* ---- the same feeder's crop-and-resize mode: the pipeline CTR-GCN was published with (its feeders/tools.py valid_crop_resize
 * and random_rot) -- a share p of the clip's valid frames, resized linearly in time to W frames, then one 3-D rotation per clip.
 * Added in ABI 401 without a version bump: new entry points only.
 *
 * With (begin, end) from _clip_extent and valid = end - begin >= 1, the CROP of a slot is two integers (start, L):
 *   one p (flag 1 clear, p = p0):  bias = trunc((1.0 - p) * valid / 2) in fp64, then bias = min(bias, (valid - 1) / 2);
 *                                  start = begin + bias, L = valid - 2 bias            (the centre crop; L >= 1 for every p)
 *   p drawn (flag 1):              p = p0 + u (p1 - p0) with u = w0 2^-32, fp64, no contraction;
 *                                  L = min(max(floor(valid p), min_crop), valid);  bias = mulhi(w1, valid - L + 1);
 *                                  start = begin + bias
 *   rotation (flag 2):             a_k = theta (2 (w_k 2^-32) - 1) in fp64, no contraction, k = x, y, z;
 *                                  R = (Rz(a_z) . Ry(a_y)) . Rx(a_x),  Rx = [[1,0,0],[0,c,s],[0,-s,c]],
 *                                  Ry = [[c,0,-s],[0,1,0],[s,0,c]],  Rz = [[c,s,0],[-s,c,0],[0,0,1]], all in fp64, every entry
 *                                  of a product summed over k = 0, 1, 2 left to right, rounded to fp32 once
 * The draw stream is the one above (same key, same counter layout): block 0 gives w0 for p and w1 for bias, block 1 gives
 * w0 .. w2 for the x, y and z angles.  The call counter advances by one after the draw iff flags != 0.
 * This is the published pipeline wherever a clip's valid frames are a prefix without all-zero gaps (begin = 0, and valid = the
 * number of non-zero frames, which is what the published code counts) -- how the NTU data tools write their clips.
 *
 * The RESIZE of output frame t in 0 .. W - 1, in fp32 and without contraction -- torch.nn.functional.interpolate(mode='bilinear',
 * align_corners=False) on the time axis alone:
 *     scale = (float)L / (float)W
 *     src   = max(scale * (t + 0.5f) - 0.5f, 0)
 *     i0    = min((int)src, L - 1);   i1 = min(i0 + 1, L - 1)
 *     l1    = src - i0;               l0 = 1 - l1
 *     y[c]  = l0 * x[c][start + i0] + l1 * x[c][start + i1]
 * then with a rotation out[c] = R[c][0] y[0] + R[c][1] y[1] + R[c][2] y[2] (left to right, C = 3), and without one out = y
 * with no further arithmetic.  L = W gives l1 = 0: the source frames themselves; L = 2 W gives l0 = l1 = 1/2: the once-rounded
 * mean of two frames.
 *
 * _clip_crop_draw  flags = 1 random crop | 2 rotation; 0 < p0 <= p1 <= 1, min_crop >= 1, theta finite and >= 0.  -> crop int32
 *                  [B][2] = (start, L), drawn fp64 [B][4] = (p, a_x, a_y, a_z) (angles 0 without flag 2), rot fp32 [B][9]
 *                  row-major (written with flag 2 only; may be NULL without it), labels_out as _clip_draw.  One thread per slot.
 * _clip_resize     out (B, C, W, V, M) from raw, clip_ids and crop; rot fp32 [B][9] or NULL (none).  L is clamped to 1 .. T and
 *                  start to 0 .. T - L, so no value of crop reads out of bounds.  No atomics: two calls give the same bits. */
int tamgcn_clip_crop_draw(const int* extent, long long n_clips, const long long* clip_ids, int B, const long long* labels,
                          long long* state, int flags, double p0, double p1, int min_crop, double theta, int* crop, double* drawn,
                          float* rot, long long* labels_out, void* stream);
int tamgcn_clip_resize(const float* raw, long long n_clips, const long long* clip_ids, const int* crop, const float* rot /* NULL: none */,
                       int B, int C, int T, int W, int V, int M, float* out, void* stream);

/* ---- f2: the eval-mode TCN_GCN_unit for small batches (callers: reference
 * ensemble/ensemble_ctrgcn_resnet_eval.py:147-183, models/resnet_gcn_attention.py:82-85, visual.py:53-55 -- model(data)
 * on 1..16 clips in eval mode).  Five launches per block, each 50..130 workgroups per clip; V = 20, S = 3 (V = 25: the f2v
 * entry points below).  The CALLER folds
 * every eval-mode BatchNorm into the weights it passes (bn(W x + b) = (s W) x + (s b + t), s = gamma / sqrt(var + eps),
 * t = beta - mean s) -- tam_gcn_amd/f2.py does.  Reference arithmetic: models/ctrgcn.py:172-177, :252-261 (unit_gcn with
 * the offset_conv branch), :93-146 (MultiScale_TemporalConv), :281-283 (residual + ReLU of TCN_GCN_unit).
 *   _f2_e     E (N, S, Cout, V, V) = alpha (W4 tanh(p_u - q_v) + b4) + A with p, q = W12 mean_t(x) + b12  (conv1 / conv2 commute
 *             with the mean over T: SURVEY.md §8a);  reads x, w12, b12, w4, b4, A, alpha; writes d->E
 *             R: every 1 <= R <= 32 is served, not only the stock 8 / 16 / 32 (the p/q product rounds its 16-row tiles of the
 *             2R rows UP: R = 12, 20, 28 have a half-empty last tile); outside 1..32 the descriptor is refused
 *   _f2_gcn   z = sum_s E_s (W3_s x + b3_s);  y = sy z + ty;  res = 0 | x | wd x + bd (res_mode 0 | 1 | 2);
 *             writes sum = y + res and diff = res - y, both (N, Cout, T, V); reads d->E
 *   _f2_gemm  out (N, M, T, V) = epilogue(W x + b), W [M][K] row-major, x (N, K, T, V):
 *             mode 0: relu(add + tanh(.))            (offset_conv + the block tail :258-261; add = sum, x = diff)
 *             mode 1: rows < relu_rows: relu(.), others plain  (entry convs of the temporal / pooled branches stacked over the
 *                     plain 1x1 branch: all read g)
 *   _f2_tcn   h = _f2_gemm mode 1's output (N, Cout, T, V) with Cout = (nb + 2) Cb: branches b < nb: k x 1 conv (dilation dil[b],
 *             stride, "same" padding) of rows [b Cb, (b+1) Cb) with wt[b] [Cb][Cb*ks] (tap innermost), + bt[b]; branch nb:
 *             MaxPool2d((3,1), stride, pad 1) of rows [nb Cb, ..) then sp . + tp; branch nb + 1: rows [(nb+1) Cb, ..) at the
 *             strided frames; + residual (res_mode 0 none | 1 the block input x | 2 wr x(strided frames) + br); ReLU;
 *             out (N, Cout, (T - 1) / stride + 1, V). */
typedef struct tamgcn_f2_gcn_desc {
    int N, Cin, Cout, T, V, S, R, res_mode;
    const float* x;                                  /* (N, Cin, T, V) */
    const float* w12; const float* b12;              /* [S*2R][Cin], [S*2R]: rows s*2R + r = conv1, s*2R + R + r = conv2 */
    const float* w4; const float* b4;                /* [S][Cout][R], [S][Cout] */
    const float* A; const float* alpha;              /* [S][V][V], [1] */
    const float* w3; const float* b3;                /* [S*Cout][Cin], [S*Cout] */
    const float* sy; const float* ty;                /* [Cout] folded unit_gcn.bn */
    const float* wd; const float* bd;                /* [Cout][Cin], [Cout] folded down conv + BatchNorm (res_mode 2) or NULL */
    float* E;                                        /* (N, S, Cout, V, V) */
    float* sum; float* diff;                         /* (N, Cout, T, V) each (not touched by _f2_e) */
    const float* xpart;                              /* NULL | (N, ceil(T/4), Cin, V): the sums over each 4-frame tile of x that the
                                                        previous block's _f2_tcn left (xpart there); _f2_e then takes mean_t(x) from
                                                        them instead of reading x again */
} tamgcn_f2_gcn_desc;
int tamgcn_f2_e(const tamgcn_f2_gcn_desc* d, void* stream);
int tamgcn_f2_gcn(const tamgcn_f2_gcn_desc* d, void* stream);

typedef struct tamgcn_f2_gemm_desc {
    int N, K, M, T, V, mode, relu_rows;
    const float* x; const float* w; const float* b; const float* add;
    float* out;
} tamgcn_f2_gemm_desc;
int tamgcn_f2_gemm(const tamgcn_f2_gemm_desc* d, void* stream);

typedef struct tamgcn_f2_tcn_desc {
    int N, Cin, Cout, T, V, stride, Cb, nb, ks, res_mode;
    int dil[4];
    const float* h;
    const float* wt[4]; const float* bt[4];
    const float* sp; const float* tp;
    const float* x; const float* wr; const float* br;
    float* out;
    float* xpart;                                    /* NULL | (N, ceil(T_out/4), Cout, V): per-tile frame sums of out */
} tamgcn_f2_tcn_desc;
int tamgcn_f2_tcn(const tamgcn_f2_tcn_desc* d, void* stream);

/* ---- f2v: the same four stages for skeletons whose joint count V is NOT a multiple of four, S = 3 (tam_gcn_amd/csrc/f2v.hip,
 * tam_gcn_amd/f2v.py): the f2 descriptors and the algebra above, unchanged.  Served joint counts d->V: 17 (COCO / YOLO-pose
 * keypoints), 18 (OpenPose), 25 (NTU-RGB+D) -- the list FV_JOINTS of f2v.hip; every other d->V is refused on the host before
 * any launch.  What differs from f2 is where the frames lie.  Only the BLOCK's input and output are contiguous (N, C, T, V);
 * every buffer that lives between the launches of one block has frames (rows of joints) of VP = (V + 3) & ~3 floats (20 at V =
 * 17 and 18, 28 at V = 25), so that each is 16-byte aligned whatever T is:
 *   _f2v_e     reads d->x (N, Cin, T, V) contiguous, or d->xpart (N, ceil(T/4), Cin, VP);  writes d->E (N, S, Cout, V, VP):
 *              E[c][u][v] at u*VP + v, columns V..VP-1 zero
 *   _f2v_gcn   reads d->x contiguous and d->E;  writes d->sum, d->diff (N, Cout, T, VP), columns V..VP-1 zero
 *   _f2v_gemm  x, add, out: (N, K | M, T, VP).  Columns V..VP-1 of out get the epilogue of whatever x and add hold there
 *              (finite when those are); no kernel lets them reach a joint
 *   _f2v_tcn   d->h (N, Cout, T, VP);  d->x contiguous (N, Cin, T, V);  d->out contiguous (N, Cout, T_out, V);
 *              d->xpart (N, ceil(T_out/4), Cout, VP): sums of out over each FOUR-frame tile (as f2), columns V..VP-1 zero
 * Columns V..VP-1 of E, sum, diff and xpart are exactly zero whatever the inputs' pad columns hold (those are never trusted).
 * Alignment: x and out 4 bytes, everything else 16.  The contiguous input is read in 16-byte pieces from dword-aligned
 * addresses; the last piece of a frame reaches VP - V floats (at most 12 bytes) past it, so READ SLACK (top of this file: 16
 * readable bytes) applies to x (tam_gcn_amd.ops.empty / with_slack); what is read there is discarded.  Each entry point computes its LDS request from the
 * geometry of d->V and refuses one above 160 KB (none arises for Cin, K <= 256, R <= 32, Cb <= 64).  Deterministic: two runs
 * are bit-equal.
 * Added in ABI 401 without a version bump: new entry points, no existing layout or semantics changed.  V = 17 and 18 were added
 * the same way: more accepted values of d->V, no symbol, descriptor or layout changed. */
int tamgcn_f2v_e(const tamgcn_f2_gcn_desc* d, void* stream);
int tamgcn_f2v_gcn(const tamgcn_f2_gcn_desc* d, void* stream);
int tamgcn_f2v_gemm(const tamgcn_f2_gemm_desc* d, void* stream);
int tamgcn_f2v_tcn(const tamgcn_f2_tcn_desc* d, void* stream);

/* ---- f2g: the same four stages for EVERY joint count 8 <= d->V <= 28, multiples of four included, with V a kernel argument
 * (tam_gcn_amd/csrc/f2g.hip, tam_gcn_amd/f2g.py).  The f2 descriptors, the algebra above and f2v's buffer layout, all
 * unchanged: the block's input and output contiguous (N, C, T, V); E (N, S, Cout, V, VP), sum, diff, the gemm operands, h
 * (N, C, T, VP) and xpart (N, tiles, C, VP) with frames of VP = (V + 3) & ~3 floats; columns V..VP-1 of E, sum, diff and xpart
 * exactly zero whatever the inputs' pad columns hold; at V % 4 == 0, VP = V and nothing is padded.  Alignment and the read
 * slack behind x: as f2v.  The kernels are instantiated per frame pitch VP (8, 12, 16, 20, 24, 28), not per joint
 * count; 17, 18, 20 and 25 are accepted too (the run-time-V form of the f2 / f2v kernels at the same V).  Any other d->V is
 * refused on the host before any launch, the message naming the entry point and "V=<value>".  No grouped entry points.
 *   tamgcn_f2g_supported(V)  1 for 8 <= V <= 28, else 0
 *   tamgcn_f2g_lds_bytes(stage, V, c, r)  the largest dynamic-LDS request, in bytes, that stage 0 (_e: c = Cin, r = R), 1 (_gcn:
 *       c = Cin), 2 (_gemm: c = K) or 3 (_tcn: c = the residual conv's Cin, r = Cb; the maximum over res_mode) makes at joint
 *       count V; -1 for a geometry the entry points refuse (V outside 8..28, c outside 1..256, R outside 1..32, Cb not 16, 32,
 *       48 or 64).  Never above 160 KB: _gcn stages K in chunks chosen from V (112 rows at V = 28, 128 below), _e sums the
 *       frames in two phases instead of four where four partial tiles do not fit.
 * Deterministic: two runs are bit-equal.  Added in ABI 401 without a version bump: new entry points only. */
int tamgcn_f2g_supported(int V);
int tamgcn_f2g_lds_bytes(int stage, int V, int c, int r);
int tamgcn_f2g_e(const tamgcn_f2_gcn_desc* d, void* stream);
int tamgcn_f2g_gcn(const tamgcn_f2_gcn_desc* d, void* stream);
int tamgcn_f2g_gemm(const tamgcn_f2_gemm_desc* d, void* stream);
int tamgcn_f2g_tcn(const tamgcn_f2_tcn_desc* d, void* stream);

/* ---- grouped: the four stages of both families for `groups` models of ONE geometry in one launch (a multi-stream ensemble:
 * tam_gcn_amd.inference.StreamEnsemble).  The descriptors above, unchanged, plus `int groups`:
 *   samples      d->N is the TOTAL number of clip-persons, N % groups == 0; samples [g N/groups, (g+1) N/groups) belong to group g
 *   activations  x, E, sum, diff, h, out, xpart (and the VP-float frames of f2v): the layouts above, indexed by the total sample
 *   parameters   every parameter pointer of the descriptor is group 0's; group g's array follows densely at g times the array's
 *                own size as the descriptor's dimensions give it:  w12 S*2R*Cin,  b12 S*2R,  w4 S*Cout*R,  b4 S*Cout,  A S*V*V,
 *                alpha 1,  w3 S*Cout*Cin,  b3 S*Cout,  sy, ty Cout,  wd Cout*Cin,  bd Cout;  gemm w M*K, b M;  tcn wt[b] Cb*Cb*ks,
 *                bt[b], sp, tp Cb,  wr Cout*Cin,  br Cout.  An absent optional array (wd / bd, wr / br) is absent for every group.
 *   alignment    where a launch reads a weight array in 16-byte pieces (row length a multiple of 16 and a 16-byte aligned base)
 *                the group stride must be a multiple of four floats; it always is under that condition, and is checked.
 * All groups share one geometry; g = sample / (N / groups) is uniform per workgroup.  Arithmetic, tiling and summation order
 * are those of the plain entry points: group g's outputs are bit-equal to a plain call on group g's slice and parameters.
 * Added in ABI 401 without a version bump: new entry points only. */
int tamgcn_f2_e_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream);
int tamgcn_f2_gcn_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream);
int tamgcn_f2_gemm_grouped(const tamgcn_f2_gemm_desc* d, int groups, void* stream);
int tamgcn_f2_tcn_grouped(const tamgcn_f2_tcn_desc* d, int groups, void* stream);
int tamgcn_f2v_e_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream);
int tamgcn_f2v_gcn_grouped(const tamgcn_f2_gcn_desc* d, int groups, void* stream);
int tamgcn_f2v_gemm_grouped(const tamgcn_f2_gemm_desc* d, int groups, void* stream);
int tamgcn_f2v_tcn_grouped(const tamgcn_f2_tcn_desc* d, int groups, void* stream);

/* ---- f2s: the eval-mode st_gcn block of ST-GCN (reference models/stgcn.py:56-64, :75-99) for small batches: TWO launches per
 * block (tam_gcn_amd/csrc/f2s.hip, tam_gcn_amd/f2s.py).  The topology is static and shared by all samples and both BatchNorms
 * fold into the neighbouring weights -- the CALLER folds (bn(y) = s y + t, s = gamma / sqrt(var + eps), t = beta - mean s):
 *   _f2s_gcn  h[n,c,t,w] = relu( sum_k sum_ci wg[k][c][ci] * ( sum_v x[n,ci,t,v] * Ae[k][v][w] ) + bg[c][w] )
 *             x (N, Cin, T, V) contiguous, N counting clip-persons;  Ae [K][V][V] = A * edge_importance;  wg [K][Cout][Cin] =
 *             s1[c] * gcn.conv.weight[k*Cout + c][ci];  bg [Cout][V] -- a TABLE over the joints, because the conv bias is added
 *             before the joint contraction:  bg[c][w] = s1[c] * sum_k b[k*Cout + c] * sum_v Ae[k][v][w] + t1[c]  (s1, t1 =
 *             tcn.0);  h (N, Cout, T, V) contiguous.  (The kernel contracts the channels first, then the joints.)
 *   _f2s_tcn  out[n,c,tau,v] = relu( sum_tap sum_c' wt[c][c'][tap] * h[n,c', tau*stride - (KT-1)/2 + tap, v] + bt[c] + res )
 *             frames outside [0, T) read as zero;  out (N, Cout, T2, V) contiguous, T2 = (T - 1) / stride + 1;  wt [Cout][Cout][KT]
 *             (tap innermost: tcn.2.weight scaled by s2[c]), bt [Cout] = s2 b + t2 (s2, t2 = tcn.3);
 *             res (res_mode): 0 nothing | 1 x[n,c,tau,v] (stride 1, Cin == Cout) |
 *                             2 sum_ci wr[c][ci] * x[n,ci,tau*stride,v] + br[c]  (residual conv + BatchNorm folded, wr [Cout][Cin])
 * Geometry: 2 <= V <= 32, 1 <= K <= 3, 1 <= Cin <= 256, Cout % 16 == 0 and 16 <= Cout <= 256, KT == 9, stride 1 | 2, N <= 65535;
 * anything else is refused on the host before any HIP call.  tamgcn_f2s_supported answers 1 | 0 for a geometry without touching
 * the device.  v_mfma_f32_16x16x4_f32 (exact fp32), fixed summation order (two runs are bit-equal), no atomics; nothing is read
 * or written outside the arrays as dimensioned above, whatever their alignment (4 bytes suffice; 16-byte aligned weights whose
 * rows are a multiple of 4 floats are read in 16-byte pieces).
 * Added in ABI 401 without a version bump: new entry points, no existing layout or semantics changed. */
typedef struct tamgcn_f2s_gcn_desc {
    int N, Cin, Cout, T, V, K;
    const float* x; const float* Ae; const float* wg; const float* bg;
    float* h;
} tamgcn_f2s_gcn_desc;
typedef struct tamgcn_f2s_tcn_desc {
    int N, Cin, Cout, T, V, KT, stride, res_mode;    /* Cin: channels of x (res_mode 2; otherwise ignored) */
    const float* h; const float* wt; const float* bt;
    const float* x; const float* wr; const float* br;    /* x: res_mode 1 | 2, wr / br: res_mode 2; else NULL */
    float* out;
} tamgcn_f2s_tcn_desc;
int tamgcn_f2s_supported(int V, int K, int Cin, int Cout, int KT, int stride);
int tamgcn_f2s_gcn(const tamgcn_f2s_gcn_desc* d, void* stream);
int tamgcn_f2s_tcn(const tamgcn_f2s_tcn_desc* d, void* stream);

/* ---- f2s grouped: both stages for `groups` ST-GCN models of ONE geometry in one launch (a multi-stream ensemble of ST-GCN
 * models: tam_gcn_amd.f2s.GroupedEvalST under tam_gcn_amd.inference.StreamEnsemble).  The contract of the "grouped" block above,
 * on the f2s descriptors, unchanged, plus `int groups`:
 *   samples      d->N is the TOTAL number of clip-persons, N % groups == 0; samples [g N/groups, (g+1) N/groups) belong to group g
 *   activations  x, h, out: the layouts above, indexed by the total sample
 *   parameters   every parameter pointer of the descriptor is group 0's; group g's array follows densely at g times the array's
 *                own size:  Ae K*V*V,  wg K*Cout*Cin,  bg Cout*V;  wt Cout*Cout*9,  bt Cout,  wr Cout*Cin,  br Cout.  An absent
 *                wr / br is absent for every group.
 *   alignment    whether wg, wt and wr are read in 16-byte pieces is decided from group 0's pointer, so where one is, its group
 *                stride must be a multiple of four floats; with Cin % 4 == 0 (wg, wr) and Cout % 16 == 0 (wt) it always is, and
 *                it is checked.
 * All groups share one geometry (V, K, Cin, Cout, stride, res_mode); g = sample / (N / groups) is uniform per workgroup and the
 * parameter pointers are offset once, at the top of the SAME kernel text (a template flag).  Arithmetic, tiling, wave split and
 * summation order are those of the plain entry points: group g's outputs are bit-equal to a plain call on group g's slice and
 * parameters.  Refused on the host before any launch: groups < 1, N % groups != 0, N > 65535 and 2^31 elements or more (both on
 * the TOTAL: the grid's z is the total sample), and whatever the plain entry points refuse.
 * Added in ABI 401 without a version bump: new entry points only. */
int tamgcn_f2s_gcn_grouped(const tamgcn_f2s_gcn_desc* d, int groups, void* stream);
int tamgcn_f2s_tcn_grouped(const tamgcn_f2s_tcn_desc* d, int groups, void* stream);

/* ---- f2s backward: the DATA gradient of that block (tam_gcn_amd/csrc/f2s_bwd.hip), again two launches, for gradient saliency
 * (tam_gcn_amd/saliency.py; reference tools/train_stgcn_group.py:264-356).  In eval mode the block is piecewise linear in x; the
 * two ReLU masks are read from the forward's own h and out, strictly (> 0, as torch).  No weight gradient; x, the biases and bg
 * do not enter.  With s = stride, T2 = (T - 1) / s + 1 and gout (N, Cout, T2, V) the gradient of the block's output:
 *   gz[n,c,tau,v]  = gout[n,c,tau,v] * [out[n,c,tau,v] > 0]                                    (never materialised)
 *   _f2s_tcn_bwd   dh[n,c',t,v] = [h[n,c',t,v] > 0] * sum_c sum_tap wtb[c'][c][tap] * gz[n,c,tau,v],  tau = (t + (KT-1)/2 - tap) / s;
 *                  terms with a non-integral tau or tau outside [0, T2) are zero.  wtb [Cout][Cout][KT] = wt[c][c'][tap] transposed
 *                  in its two channel indices (tap innermost, NOT mirrored: the mirror is in tau).  dh (N, Cout, T, V).
 *   _f2s_gcn_bwd   dx[n,ci,t,v] = sum_k sum_c wgb[k][ci][c] * ( sum_w Ae[k][v][w] * dh[n,c,t,w] ) + res
 *                  Ae [K][V][V]: the forward's array;  wgb [K][Cin][Cout] = wg[k][c][ci];  dx (N, Cin, T, V);
 *                  res (res_mode): 0 nothing | 1 gz[n,ci,t,v] (stride 1, Cin == Cout) |
 *                                  2 [t % s == 0] * sum_c wrb[ci][c] * gz[n,c,t/s,v],  wrb [Cin][Cout] = wr[c][ci]
 *                  gout / out: res_mode 1 | 2, wrb: res_mode 2; else NULL.  Rows ci >= Cin of a 16-row tile are neither read from
 *                  the weights nor stored.
 * Geometry, alignment, determinism and the refusal on the host: as the forward's.
 * Added in ABI 401 without a version bump: new entry points, no existing layout or semantics changed. */
typedef struct tamgcn_f2s_tcn_bwd_desc {
    int N, Cout, T, V, KT, stride;                   /* T: frames of h and dh (the block's input frames) */
    const float* gout; const float* out; const float* h; const float* wtb;
    float* dh;
} tamgcn_f2s_tcn_bwd_desc;
typedef struct tamgcn_f2s_gcn_bwd_desc {
    int N, Cin, Cout, T, V, K, stride, res_mode;
    const float* dh; const float* Ae; const float* wgb;
    const float* gout; const float* out; const float* wrb;
    float* dx;
} tamgcn_f2s_gcn_bwd_desc;
int tamgcn_f2s_tcn_bwd(const tamgcn_f2s_tcn_bwd_desc* d, void* stream);
int tamgcn_f2s_gcn_bwd(const tamgcn_f2s_gcn_bwd_desc* d, void* stream);

/* ---- saliency (tam_gcn_amd/csrc/saliency.hip): what follows the backward chain of a saliency pass.
 *   _saliency_joints      dx0 (N*M, C, T, V): the first block's dx;  coef: the eval-mode data_bn coefficients in _stem_apply's layout,
 *                         of which only c1 (the first J = C*V*M floats) is read.  dxin[n,c,t,v,m] = c1[(m V + v) C + c] *
 *                         dx0[n M + m, c, t, v] is the gradient with respect to the model's input;  sal[n][v] = sum_{m,c,t} |dxin|,
 *                         (N, V), summed in a fixed order (two launches are bit-equal).  dxin: NULL | (N, C, T, V, M) out.
 *   _saliency_accumulate  adds one batch to an on-device state: for i = 0 .. N-1 in order, with k = labels[i] (int64): a label
 *                         outside [0, num_class) or a class with count[k] >= per_class is skipped; else count[k] += 1 and, for
 *                         every part p, sum[k][p] += mean over the joints j of part p of sal[i][j] (taken in fp64).  Part p's
 *                         joints are part_joints[part_off[p] .. part_off[p+1]) (int32, on the device; part_off is trusted, a
 *                         joint outside [0, V) is skipped).  count int32 [num_class], sum fp64 [num_class][P].  One workgroup,
 *                         N <= 4096, P <= 256.  No host synchronisation.
 * Added in ABI 401 without a version bump: new entry points. */
int tamgcn_saliency_joints(const float* dx0, const float* coef, int N, int C, int T, int V, int M, float* sal, float* dxin, void* stream);
int tamgcn_saliency_accumulate(const float* sal, const long long* labels, int N, int V, const int* part_off, const int* part_joints,
                               int P, int num_class, int per_class, int* count, double* sum, void* stream);

/* ---- guidance (tam_gcn_amd/csrc/guidance.hip; tam_gcn_amd/guidance.py): the arithmetic between extract_feature and the plot of
 * the reference's visual.py:53-87, and the pooled feature of models/resnet_gcn_attention.py:82-85, read from the block stack's
 * output h (N*M, C, T', V) (row n*M + m = person m of clip n) without the permuted 5-D copy.  No host synchronisation, no atomics:
 * two calls give the same bits.  2 <= V <= 32.
 *   _guidance_parts    the workgroups of _guidance_reduce, N*M*ceil(T'V / 64) (-1: bad dims): its scratch sizes.
 *   _guidance_reduce   intensity (N, T', V, M) = sqrt(sum_c h^2);  pooled (N, C) = mean over (T', V, M) of h;  csum: parts*C floats of
 *                      scratch (per-workgroup channel sums, added per clip in (m, chunk) order by a second launch);  minmax
 *                      [parts][2]: each workgroup's smallest and largest intensity.  One read of h.
 *   _guidance_weights  weights (N, J).  min / max over ALL nparts partials (the whole call, visual.py:58-59);  f = 255 (I - min) /
 *                      (max - min) in fp32, or I itself when max == min;  person 1 if M > 1 and the mean of f over (T', V) of person
 *                      0 is strictly less than person 1's, else person 0 (only these two are compared);  per target joint v =
 *                      joints[j] (int32 on the device): the mean of the min(k, T') largest of f[n, :, v, person], divided by 127;
 *                      0 for v outside [0, V).  T' <= 1024.  One workgroup per clip.
 *   _guidance_apply    the (225, 45 frames) map of the reference has weights[n][j] in rows 45j .. 45(j+1) when j < J and j < frames,
 *                      0 elsewhere, every column equal; resized to (H, W) bilinearly with align_corners = False that is one factor per
 *                      row: src = max((y + 0.5) 225 / H - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, 224), l = src - i0, factor =
 *                      (1 - l) row[i0] + l row[i1].  out (N, Crgb, H, W) = rgb * factor (rgb, out: both or neither);  map: NULL |
 *                      (N, 1, H, W) = factor.  Pointers need 4-byte alignment only; 16-byte accesses are used where rgb and out
 *                      agree modulo 16.
 * Added in ABI 401 without a version bump: new entry points. */
int tamgcn_guidance_parts(int N, int M, int Tp, int V);
int tamgcn_guidance_reduce(const float* h, int N, int M, int C, int Tp, int V, float* intensity, float* pooled, float* csum, float* minmax,
                           void* stream);
int tamgcn_guidance_weights(const float* intensity, const float* minmax, int nparts, int N, int Tp, int V, int M, const int* joints, int J,
                            int k, float* weights, void* stream);
int tamgcn_guidance_apply(const float* weights, int N, int J, int frames, const float* rgb, int Crgb, int H, int W, float* out, float* map,
                          void* stream);

/* Stem and head of such an ensemble, one launch each:
 *   _stem_streams_eval  x (N, C, T, V, M) joint clips -> out (G*N*M, C, T, V), row g*N*M + n*M + m = model g's eval-mode data_bn
 *                       (coef [G][3][J], J = C*V*M, each in _stem_apply's layout: c1 at [0][j], c0 at [2][j]) of stream modes[g]
 *                       of x (0 joint, 1 bone, 2 motion, 3 bone-motion: _stream_derive's arithmetic, then _stem_apply's fma --
 *                       bit-equal to that pair).  parent int32 [V], modes int32 [G] on the device.  The frame after the last is
 *                       never read (the motion of the last frame is 0).  modes and parent live on the device and are NOT
 *                       validated (as _stream_derive trusts its parent table): a mode outside 0..3 behaves as 3, a parent
 *                       entry outside [0, V) reads outside the frame -- the caller checks both (inference.StreamEnsemble does).
 *   _head_fc_grouped    pooled (G*N, C) (tamgcn_head_pool_fwd with N := G*N), W [G][K][C], b [G][K] or NULL ->
 *                       scores [G][N][K], tamgcn_score_fuse's layout; per row the arithmetic of _head_fc_fwd. */
int tamgcn_stem_streams_eval(const float* x, const int* parent, const int* modes, const float* coef, int G, int N, int C, int T, int V, int M,
                             float* out, void* stream);
int tamgcn_head_fc_grouped(const float* pooled, const float* W, const float* b, int G, int N, int C, int K, float* scores, void* stream);

/* ------------------------------------------------------------------------
 * Optimiser update in place over flat fp32 buffers of n elements (a ParamArena and its FlatGradBucket):
 *   mode 0  torch.optim.SGD (foreach=False):  d = g + wd p;  with momentum m > 0:  s0 = d on the first step, else
 *           s0 = m s0 + (1 - dampening) d;  d = nesterov ? d + m s0 : s0;  p -= lr d
 *   mode 1  torch.optim.Adam (coupled L2 weight decay, no amsgrad):  g += wd p;  s0 = b1 s0 + (1 - b1) g;
 *           s1 = b2 s1 + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) s0 / (sqrt(s1) / sqrt(1 - b2^t) + eps)
 * The learning rate (*lr) and the step count (*step, int32, 0 before the first call) are read on the device, and *step
 * advances by one per call on the device: a HIP graph holding this call sees a changed *lr and counts its own replays.
 * scal: 2 floats of scratch (this step's scalars, written by a one-thread launch before the update).  p, g, s0 and s1
 * must be 16-byte aligned; s0 may be NULL for SGD without momentum, s1 is NULL for SGD.  Two launches.
 * Added in ABI 401 without a version bump: a new entry point, no existing layout or semantics changed. */
typedef struct tamgcn_optim_desc {
    long long n;
    float* p; const float* g;
    float* s0;                                       /* SGD momentum buffer | Adam exp_avg */
    float* s1;                                       /* Adam exp_avg_sq | NULL */
    const float* lr;                                 /* [1] */
    int* step;                                       /* [1] */
    float* scal;                                     /* [2] scratch */
    int mode;                                        /* 0 SGD, 1 Adam */
    int nesterov;
    float momentum, dampening, weight_decay, eps;
    double beta1, beta2;
} tamgcn_optim_desc;
int tamgcn_optim_step(const tamgcn_optim_desc* d, void* stream);

/* The same update behind a gradient guard (three launches, still no host sync):
 *   norm = sqrt(sum g[i]^2) over the n elements of d->g, every square and the whole sum in fp64, reduced in a fixed shape
 *          (one partial per workgroup, then one workgroup adds the partials in order; no floating-point atomics): two
 *          calls on the same buffer give the same bits.
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1, in fp32 (torch.nn.utils.clip_grad_norm_); the update
 *          uses g * coef, applied before the weight-decay term.  d->g itself is NOT rewritten.  With coef == 1 and a
 *          finite sum, p, s0, s1 and *step end bit-identical to tamgcn_optim_step.
 *   finite = isfinite(sum g^2).  With skip_nonfinite and a non-finite sum the call leaves p, s0, s1, *step and scal
 *          untouched and adds one to *skipped; without skip_nonfinite the non-finite values propagate as in torch
 *          (error_if_nonfinite=False).
 * partial: n_partial doubles of scratch, 8-byte aligned, at least one per workgroup of the reduction (2048 always
 * suffices).  stat: 3 floats out: norm before clipping, coefficient applied, 1 / 0 for finite.  skipped: device counter,
 * may be NULL when skip_nonfinite is 0.  Added in ABI 401 without a version bump: a new entry point. */
typedef struct tamgcn_grad_guard {
    float max_norm;                                  /* > 0: clip to this L2 norm; <= 0: measure only */
    int skip_nonfinite;
    double* partial;                                 /* [n_partial] scratch */
    int n_partial;
    float* stat;                                     /* [3] out */
    int* skipped;                                    /* [1] */
} tamgcn_grad_guard;
int tamgcn_optim_step_guarded(const tamgcn_optim_desc* d, const tamgcn_grad_guard* g, void* stream);

/* ------------------------------------------------------------------------
 * Live and sliding-window inference from device-resident frame rings (csrc/streaming.hip, tam_gcn_amd/streaming.py): a bank of
 * S rings for S live feeds in one graph.  Added in ABI 401 without a version bump: new entry points, no existing layout or
 * semantics changed.
 *
 * Frames are numbered absolutely in int64 from 0, the first frame a feed was ever pushed; frame f lives in slot f % cap.  A ring
 * is logically (P, cap, R) with elements of `elem` bytes: P = 1, R = V 3, elem = 8 is fp64 (cap, V, 3), the raw form
 * tamgcn_feeder_transform reads; P = C, R = V M, elem = 4 is fp32 (C, cap, V, M), the clip feeder's layout with T = cap.
 * A sequence that is resident as a whole is a ring of cap = its length that never wraps.  The bank is S rings in one
 * allocation, feed s at s (P cap R) elements: fp64 (S, cap, V, 3) or fp32 (S, C, cap, V, M).  state int64 (S, 2) = (count,
 * pushes) per feed, on the device.  1 <= S <= 1024.  counts and restart are int32 [S] on the device and may be NULL (every feed
 * takes all n frames; no feed restarts).  take_s = min(max(counts[s], 0), n); fresh_s = restart[s] != 0.  A plan is int64
 * (S B, 2) = (start, L) per window, window w that of feed w / B; L = 0 marks an invalid window, and so does any row with
 * start < 0 or L > cap.  No entry point synchronises, none uses atomics: two calls give the same bits, a graph replay the
 * eager call's.
 *
 *   _bank_push          frames (S, P, n, R), 1 <= n <= cap: feed s stores the first take_s frames of its slice at slots
 *                       (c_s + i) % cap of every plane, c_s = fresh_s ? 0 : count_s; a unit of a frame i >= take_s is neither
 *                       read nor stored (it may hold NaN).  A second launch behind it, one thread per feed: fresh_s ->
 *                       (count, pushes) = (0, 0) first; then count += take_s and pushes += 1 where take_s > 0.  take_s = 0
 *                       without restart: nothing of feed s moves.  16-byte accesses where R elem is a multiple of 16 (the feed
 *                       strides then are too) and both arrays are 16-byte aligned.
 *   _bank_plan          plan (S B, 2): window j of a feed's B has length L and ends (B - 1 - j) hop frames before the feed's
 *                       newest frame: j = B - 1 is the newest.  A window that would start before frame 0 or before
 *                       count_s - cap (overwritten) gets (0, 0), and so does every window of a feed with counts[s] <= 0.
 *                       1 <= L <= cap, hop >= 1.  Run it behind _bank_push: it reads the advanced state.
 *   _bank_window_nucla  out (S B, 3, time_steps, V, 1) fp32, plan row w on the ring of feed w / B: the arithmetic of
 *                       tamgcn_feeder_transform on the window's L frames with the identity view and idx = np.linspace(0,
 *                       L - 1, time_steps).astype(int) -- centre on center_joint of the window's first frame, per-coordinate
 *                       min / max over the window, (p - lo) / (hi - lo + 1e-6) * 2 - 1 in fp64, the stream `mode` 0..3 -- one
 *                       body with that kernel, so bit-equal to it on a copy of the window's frames.  time_steps <= 64.
 *                       Invalid windows: zeros.
 *   _bank_window_clip   out (S B, C, W, V, M) fp32, plan row w on the ring of feed w / B: the linear time-resize of
 *                       tamgcn_clip_resize on the crop (start, L) without rotation -- the same taps, src = ((2 t + 1) L - W) /
 *                       (2 W) clamped at 0 as that kernel computes it in fp32, the same blend l0 x[i0] + l1 x[i1] without
 *                       contraction -- sources fetched at (start + i) % cap.  L = W copies the frames (l1 = 0; a -0.0 comes
 *                       out +0.0, as from tamgcn_clip_resize).  Invalid: zeros.
 *   _window_vote        probs[j] = softmax(logits[j]) over K <= 4096 classes, for the rows of any number of feeds: fp64 from the
 *                       fp32 logits, max shift, the sum class ascending, rounded once to fp32.  frame_scores[f], f < n_frames
 *                       (one ring's plan): the mean over j ascending of probs[j] (the fp32 values, summed in fp64, rounded
 *                       once) of the valid windows with start_j <= f < start_j + L_j; frame_label[f] int64 its first arg max;
 *                       no such window: zeros and -1.  frame_scores and frame_label may both be NULL: only probs is written.
 *                       One launch, two with the frame outputs.
 *   _bank_ema           one workgroup per feed, its B windows (probs and plan rows s B + j) j ascending, on ema (S, K) fp64 and
 *                       seen int64 [S].  A valid window: ema_s = probs when seen_s == 0, else beta ema_s + (1 - beta) probs in
 *                       fp64, then seen_s += 1; an invalid one moves nothing.  fresh_s: the average reads as zeros and seen as
 *                       0 first (both are stored, a valid window or not).  After the last window out[s] = (float)ema_s,
 *                       label[s] = the first arg max of ema_s or -1 while seen_s == 0, conf[s] = out[s][label[s]] (0 with -1),
 *                       advanced int32 [S] = 1 where seen moved.  K <= 4096, 0 <= beta < 1.
 *   _bank_decide        one workgroup; the debounce of every feed, then the events in ascending feed order through a scan.
 *                       deb int64 (S, 3) = (stable, cand, run), (-1, -1, 0) at the start and where fresh_s.  Where advanced[s]:
 *                       conf[s] >= threshold and label[s] == cand: run += 1; else conf[s] >= threshold: cand = label[s],
 *                       run = 1; else cand = -1, run = 0; then, if run >= hold and cand != stable: stable = cand and one event
 *                       (s, count_s - 1, label[s]) with conf[s].  log_rows int64 (log_capacity, 3), log_conf fp32
 *                       [log_capacity], log_count int64 [2] = (written, dropped): an event goes to row `written`; a full log
 *                       drops it and counts it, it never overwrites.  hold >= 1, log_capacity >= 1.
 *
 * One ring: _ring_push, _ring_plan, _window_nucla, _window_clip and _score_ema are _bank_push, _bank_plan, _bank_window_nucla,
 * _bank_window_clip and _bank_ema at S = 1 with NULL counts and restart (the same kernels): ring (P, cap, R), state int64 [2],
 * plan (B, 2).  _score_ema takes one window (B = 1): plan_row is its plan row, ema fp64 [K], seen int64 [1], and there is no
 * `advanced`. */
int tamgcn_ring_push(const void* frames, int n, int P, int R, int elem, void* ring, int cap, long long* state, void* stream);
int tamgcn_ring_plan(const long long* state, int cap, int B, int L, int hop, long long* plan, void* stream);
int tamgcn_window_nucla(const double* ring, int cap, const long long* plan, int B, const int* parent, int V, int time_steps,
                        int center_joint, int mode, float* out, void* stream);
int tamgcn_window_clip(const float* ring, int cap, const long long* plan, int B, int C, int V, int M, int W, float* out, void* stream);
int tamgcn_window_vote(const float* logits, const long long* plan, int B, int K, int n_frames, float* probs, float* frame_scores,
                       long long* frame_label, void* stream);
int tamgcn_score_ema(const float* probs, const long long* plan_row, int K, double beta, double* ema, long long* seen, float* out,
                     long long* label, float* conf, void* stream);
int tamgcn_bank_push(const void* frames, int S, int n, int P, int R, int elem, void* ring, int cap, long long* state, const int* counts,
                     const int* restart, void* stream);
int tamgcn_bank_plan(const long long* state, const int* counts, int S, int cap, int B, int L, int hop, long long* plan, void* stream);
int tamgcn_bank_window_nucla(const double* ring, int S, int cap, const long long* plan, int B, const int* parent, int V, int time_steps,
                             int center_joint, int mode, float* out, void* stream);
int tamgcn_bank_window_clip(const float* ring, int S, int cap, const long long* plan, int B, int C, int V, int M, int W, float* out,
                            void* stream);
int tamgcn_bank_ema(const float* probs, const long long* plan, const int* restart, int S, int B, int K, double beta, double* ema,
                    long long* seen, float* out, long long* label, float* conf, int* advanced, void* stream);
int tamgcn_bank_decide(const long long* label, const float* conf, const int* advanced, const int* restart, const long long* state, int S,
                       float threshold, int hold, long long* deb, long long* log_rows, float* log_conf, long long* log_count,
                       int log_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMGCN_H */
