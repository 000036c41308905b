/* libtamgcn_xmodal.so: the cross-modal attention head (reference models/resnet_gcn_attention.py:60-70, :89-120) on gfx950.
 * An extension library of libtamgcn.so with a C ABI of its own, written to the rules of include/tamgcn.h: tam_gcn_amd/_abi.py
 * parses this file and tam_gcn_amd/_xm_lib.py derives the ctypes binding from it.  The core header, its version and its entry
 * points are untouched; the classifier of the head is the core's tamgcn_head_fc_fwd / _bwd.
 *
 * Dimensions: N clips, D = width of the skeleton feature, Hd = hidden units, R = channels of the image map, P = H*W of the map.
 *   D, Hd, R multiples of 4;  1 <= N <= 1024 (2 <= N in training mode);  P >= 1;  N*R*P < 2^31.
 * Every tensor is fp32, row-major and dense.  Every pointer is a device address and must be 16-byte aligned, EXCEPT f_rgb and
 * df_rgb, whose rows of P floats are only dword aligned anyway: those two may start at any multiple of 4 bytes.  No kernel reads
 * or writes outside the tensors it is given (there is no slack contract here), none uses floating-point atomics: two calls on
 * the same inputs give the same bits.  Every entry point returns 0, or a negative value with tamgcn_xm_last_error() set, before
 * anything was launched when an argument is refused (-1) and after a failed launch (-2).  `stream` is a hipStream_t.
 *
 * Forward (three launches, then tamgcn_head_fc_fwd on g):
 *   _hidden_fwd  z = f W1^T + b1 (N, Hd);  xhat = (z - mean) * invstd;  a1 = relu(gamma * xhat + beta).
 *                training != 0: mean / biased variance of the batch, per hidden unit; running_mean = (1 - momentum) running_mean +
 *                momentum mean, running_var likewise with the unbiased variance (torch.nn.BatchNorm1d), num_batches_tracked[0] += 1.
 *                training == 0: mean = running_mean, invstd = 1 / sqrt(running_var + eps); the three buffers are only read (and
 *                num_batches_tracked may be NULL).  Saves a1, xhat (N, Hd), mean, invstd (Hd) for the backward.
 *   _gate_fwd    att = 1 / (1 + expf(-(a1 W2^T + b2))) (N, R), IEEE division.
 *   _pool_fwd    m[n][c] = mean_p f_rgb[n][c][p];  g = att * m, both (N, R).  Summed in an order that depends on P alone.
 * Backward (after tamgcn_head_fc_bwd gave dg):
 *   _pool_bwd    dz2 = dg * m * att * (1 - att) (N, R);  df_rgb[n][c][p] = dg[n][c] * att[n][c] / P unless df_rgb is NULL.
 *   _gate_bwd    dW2 = dz2^T a1 (R, Hd), db2 = sum_n dz2 (R), da1 = dz2 W2 (N, Hd).                          two launches
 *   _hidden_bwd  dy = da1 where a1 > 0 else 0;  dgamma = sum_n dy * xhat, dbeta = sum_n dy;
 *                training: dz1 = gamma * invstd * (dy - dbeta / N - xhat * dgamma / N);  else dz1 = gamma * invstd * dy;
 *                dW1 = dz1^T f (Hd, D), db1 = sum_n dz1, dz1 (N, Hd) is written too;  df = dz1 W1 (N, D) unless df is NULL
 *                (a second launch). */
#ifndef TAMGCN_XMODAL_H
#define TAMGCN_XMODAL_H

#define TAMGCN_XM_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int tamgcn_xm_version(void);
const char* tamgcn_xm_last_error(void);

int tamgcn_xm_hidden_fwd(const float* f, const float* W1, const float* b1, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, long long* num_batches_tracked,
                         int N, int D, int Hd, int training, float momentum, float eps,
                         float* a1, float* xhat, float* mean, float* invstd, void* stream);
int tamgcn_xm_gate_fwd(const float* a1, const float* W2, const float* b2, int N, int Hd, int R, float* att, void* stream);
int tamgcn_xm_pool_fwd(const float* f_rgb, const float* att, int N, int R, int P, float* m, float* g, void* stream);

int tamgcn_xm_pool_bwd(const float* dg, const float* m, const float* att, int N, int R, int P, float* dz2, float* df_rgb, void* stream);
int tamgcn_xm_gate_bwd(const float* dz2, const float* a1, const float* W2, int N, int Hd, int R,
                       float* dW2, float* db2, float* da1, void* stream);
int tamgcn_xm_hidden_bwd(const float* da1, const float* a1, const float* xhat, const float* invstd, const float* gamma,
                         const float* f, const float* W1, int N, int D, int Hd, int training,
                         float* dgamma, float* dbeta, float* dW1, float* db1, float* dz1, float* df, void* stream);

#ifdef __cplusplus
}
#endif
#endif
