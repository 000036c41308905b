"""The case table of the f2g ledger (tests/test_gpu_f2g_stages.py; tests/test_f2g_cpu.py evaluates it in fp32 on the CPU): rows
built with tests/f2_ref.py's own constructors, every one a plain (G = 1) launch -- the family has no grouped entry points.
What the table reaches at least once per stage: the vectorised and the scalar weight-row path (row length % 16 == 0 or not,
and `off`: a row length of the vector path one float off its boundary), a K tail, R in {1, 12, 32}, alpha == 0 and != 0, xpart
given and absent, T in {1, 3, 4, 5, 9, 33}, res_mode 0 / 1 / 2, stride 1 and 2 with the pooled branch's last frame present,
nb in {1, 2, 4}, Cb in {16, 64}, every (ks, dilation) at the halo limit, and Cin = K = 256 (at V = 28 the LDS edge of every
stage: two frame phases in e, 112-row K chunks in gcn).  Cin = 200 crosses the K chunk with a scalar tail behind it."""
import f2_ref as R

JOINTS = (8, 9, 16, 19, 22, 23, 28)       # all six frame pitches; 1, 2, 3, 4 live lanes in a frame's last piece; 16: whole tiles

E_CASES = {
    'cin3_r1_t1': R._e(3, 1, 16, 1),
    'cin16_r12_t3': R._e(16, 12, 16, 3, off=True),
    'cin40_r32_t4': R._e(40, 32, 16, 4),
    'cin16_r16_t5_alpha0': R._e(16, 16, 16, 5, alpha=0.0, off=True),
    'cin40_r8_xpart_t9': R._e(40, 8, 48, 9, src='xpart'),
    'cin16_r20_t33': R._e(16, 20, 16, 33, N=1),
    'cin16_r8_xpart_t33': R._e(16, 8, 16, 33, src='xpart', N=3),
    'cin256_r32_t4': R._e(256, 32, 16, 4, N=1),
    'cin256_r8_xpart_t5': R._e(256, 8, 16, 5, src='xpart', N=1),
}
GCN_CASES = {
    'cin3_res2_t1': R._g(3, 16, 2, 1),
    'cin16_res1_t3': R._g(16, 16, 1, 3, off=True),
    'cin40_res0_t4': R._g(40, 16, 0, 4),
    'cin48_res1_t5': R._g(48, 48, 1, 5, N=3),
    'cin16_res2_t9': R._g(16, 48, 2, 9, off=True),
    'cin40_res0_t33': R._g(40, 16, 0, 33, N=1),
    'cin200_res0_t3': R._g(200, 16, 0, 3, N=1),
    'cin256_res2_t5': R._g(256, 16, 2, 5, N=1),
}
GEMM_CASES = {
    'k16_m16_mode0_t1': R._m(16, 16, 0, 0, 1),
    'k40_m48_mode0_t3': R._m(40, 48, 0, 0, 3, N=3),
    'k48_m48_mode0_t9': R._m(48, 48, 0, 0, 9, off=True),
    'k40_m48_relu8_t5': R._m(40, 48, 1, 8, 5),
    'k16_m48_relu32_t4': R._m(16, 48, 1, 32, 4),
    'k48_m16_relu16_t33': R._m(48, 16, 1, 16, 33, N=1),
    'k256_m16_relu0_t5': R._m(256, 16, 1, 0, 5, N=1, off=True),
}
TCN_CASES = {
    'nb2_cb16_k5_s2_res2_cin3_t8': R._t(2, 16, 5, (2, 1), 2, 8, 2, Cin=3),
    'nb1_cb16_k9_s2_res0_t3': R._t(1, 16, 9, (1,), 2, 3, 0, xpart=False),
    'nb2_cb16_k3_s1_res1_t5': R._t(2, 16, 3, (1, 5), 1, 5, 1, N=3),
    'nb4_cb16_k1_s1_res2_cin40_t1': R._t(4, 16, 1, (1, 1, 1, 1), 1, 1, 2, Cin=40, off=True),
    'nb1_cb64_k7_s1_res0_t9': R._t(1, 64, 7, (1,), 1, 9, 0, N=1),
    'nb2_cb16_k9_s1_res2_cin48_t4': R._t(2, 16, 9, (1, 1), 1, 4, 2, Cin=48, off=True),
    'nb1_cb16_k5_s1_res1_t33': R._t(1, 16, 5, (2,), 1, 33, 1, N=1),
    'nb1_cb64_k3_s2_res2_cin256_t4': R._t(1, 64, 3, (1,), 2, 4, 2, Cin=256, N=1),
}
STAGES = {'e': E_CASES, 'gcn': GCN_CASES, 'gemm': GEMM_CASES, 'tcn': TCN_CASES}
