/* libtamgcn_rgb.so: the RGB modality's feeder (reference feeder/tools.py:216-246, feeder/feeder_nucla_resnet.py:24-35, :50-64) on
 * gfx950.  An extension library of libtamgcn.so with a C ABI of its own, written to the rules of include/tamgcn.h:
 * tam_gcn_amd/_abi.py parses this file and tam_gcn_amd/_rgb_lib.py derives the ctypes binding from it.  The core header and
 * include/tamgcn_xmodal.h, their versions and their entry points are untouched.
 *
 * Every tensor is dense and row-major, every pointer a device address.  uint8 images are (n, H, W, 3), channel last, as PIL
 * decodes them.  No kernel reads or writes outside the tensors it is given (there is no slack contract here), none uses atomics:
 * two calls on the same inputs give the same bits.  Every entry point returns 0, or a negative value with tamgcn_rgb_last_error()
 * set: -1 when an argument is refused, before anything was launched, -2 after a failed launch.  `stream` is a hipStream_t.
 *
 * _resize   PIL's 8-bit bilinear resample (Pillow's ImagingResample on 8-bit pixels), which is integer arithmetic: per axis and
 *           output index o a window of `count` source samples from `first` on with fixed-point coefficients,
 *               out = clip((2^21 + sum_j coef[o][j] * in[first + j]) >> 22, 0, 255),      int32 accumulator
 *           (a coefficient is about 2^22 * weight, the weights of a window sum to 1 and samples are <= 255: below 2^31).
 *           The host builds the tables (tam_gcn_amd/feeder/rgb_feeder.py, pil_bilinear_tables) once per (n_in, n_out):
 *               coef   int32 (n_out, K), row o holding its `count` coefficients first;   1 <= K <= 64
 *               bounds int32 (n_out, 2) = (first, count),  0 <= first, first + count <= n_in, count <= K.
 *           A window that breaks those limits is cut to them on the device, so a bad table gives wrong bytes, not a wild read.
 *           The horizontal pass runs first, src (n, H0, W0, 3) -> tmp (n, H0, Wo, 3), rounded to uint8; the vertical pass second,
 *           tmp -> dst (n, Ho, Wo, 3).  A pass whose tables are NULL is skipped, as PIL skips it when the sizes are equal; its
 *           sizes must then be equal, and with one pass skipped the other goes from src to dst directly and tmp may be NULL.
 *           With both skipped dst is a copy of src.  src, tmp and dst must not overlap.  n H0 W0, n H0 Wo, n Ho Wo < 2^31 / 3.
 *           Meant to run once per split, at load: two plain launches.
 *
 * _draw     The flip draws of one batch.  state int64 [2] = (seed, call) is read on the device; slot b flips (flip[b] = 1, else 0)
 *           iff word 0 of Philox4x32-10 (Salmon et al., SC'11) with counter (call & 0xFFFFFFFF, call >> 32, b, 0) and key
 *           (seed & 0xFFFFFFFF, seed >> 32) is below 2^31.  A second launch of one thread then writes call + 1: a graph that holds
 *           both draws anew on every replay.  1 <= B.
 *
 * _batch    out fp32 (B, 3 F, S, S) from store uint8 (n, S, S, 3):
 *               out[b][3 f + c][y][x] = lut[c][store[id][y][x'][c]]  (* row_scale[b][y]),    f = 0 .. F - 1,
 *           id = ids[b] modulo n (Python's %, the sign of n), x' = S - 1 - x where flip[b] != 0, else x.
 *               lut        fp32 (3, 256): ToTensor + Normalize of a byte, per channel
 *               flip       int32 [B], or NULL: nobody flips
 *               missing    uint8 [n], or NULL: nobody is missing.  An image with missing[id] != 0 is not read;
 *                          missing_mode 0: its slot is exact zeros (row_scale or not), 1: it is a black image, lut[c][0]
 *               row_scale  fp32 (B, S), or NULL; one fp32 multiplication
 *               labels     int64 [n] with labels_out int64 [B] = labels[id], or both NULL
 *           Where S is a multiple of 4 and store, out are 4- and 16-byte aligned, a thread makes four consecutive x of the three
 *           channels: 12 bytes read as three dwords, 3 F stores of 16 bytes, the table in LDS.  Any other S >= 1 takes a scalar form
 *           of the same arithmetic; the two give the same bits.  Offsets are 64-bit.  1 <= B, n, F;  B S S < 2^31. */
#ifndef TAMGCN_RGB_H
#define TAMGCN_RGB_H

#define TAMGCN_RGB_VERSION 1
#define TAMGCN_RGB_MAX_TAPS 64

#ifdef __cplusplus
extern "C" {
#endif

int tamgcn_rgb_version(void);
const char* tamgcn_rgb_last_error(void);

int tamgcn_rgb_resize(const unsigned char* src, int n, int H0, int W0, int Ho, int Wo,
                      const int* coef_h, const int* bounds_h, int Kh, const int* coef_v, const int* bounds_v, int Kv,
                      unsigned char* tmp, unsigned char* dst, void* stream);
int tamgcn_rgb_draw(long long* state, int B, int* flip, void* stream);
int tamgcn_rgb_batch(const unsigned char* store, long long n, int S, const long long* ids, int B, const float* lut, const int* flip,
                     const unsigned char* missing, int missing_mode, const float* row_scale, int F,
                     const long long* labels, long long* labels_out, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
