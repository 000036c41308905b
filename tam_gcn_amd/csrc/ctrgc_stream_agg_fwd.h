// The aggregation forward (workgroup = (n, c)).
// A body FRAGMENT of ctrgc_stream_body.h (read that first): pasted by #include into the __global__ function that is this kernel.
// In scope there: the template argument ST, the policy type G and `const G g`, and (V a template or a kernel argument)
//     int N, Cout, T, V; const float* x3, * E; float* y, * stats_part
    constexpr int PE = G::PE, BT = STREAM_BT, NPF = (ST * BT * G::VMAX / 4 + 255) / 256;
    constexpr int JW = G::NUT >= 2 ? G::NUT / 2 : 1;  // joint tiles per wave
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[2][4];
    float* Es = smem;                         // [ST][G::VP][PE]
    float* Xs = Es + ST * G::VP * PE;            // [ST][BT][PE]
    const int n = blockIdx.x / Cout, c = blockIdx.x - n * Cout;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const bool active = G::NUT >= 2 || wave < 2;
    const int tt = G::NUT >= 2 ? wave >> 1 : wave & 1, ub = G::NUT >= 2 ? (wave & 1) * JW : 0;
    const int CH4 = BT * V / 4;
    const long long TV = (long long)T * V;
    if constexpr (G::PADS && !G::FILL_WITH_E) for (int e = tid; e < ST * BT * PE; e += 256) Xs[e] = 0.f;     // joint pads stay zero
    g.template stage_E<ST, false>(E, Cout, n, c, Es, ST * BT * PE);

    float4 pre[NPF];
    auto prefetch = [&](int t0) {
        const int valid = min(BT, T - t0) * V;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = tid + i * 256, ec = g.idle0(e, ST * CH4), s = g.subset_of(ec, CH4), r = ec - s * CH4;
            const bool ok = e < ST * CH4 && g.in_clip(r * 4, valid, t0, T);
            pre[i] = ok ? reinterpret_cast<const float4*>(x3 + (((long long)n * ST + s) * Cout + c) * TV + (long long)t0 * V)[r]
                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    prefetch(0);
    float s1 = 0.f, s2 = 0.f;
    float* yrow = y + ((long long)n * Cout + c) * TV;
    for (int t0 = 0; t0 < T; t0 += BT) {
        __syncthreads();                      // previous chunk's MFMAs are done with Xs (first pass: E staged, pads zeroed)
        const int valid = min(BT, T - t0) * V;
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = tid + i * 256, s = g.subset_of(e, CH4), r = e - s * CH4;
            if (e < ST * CH4) {
                float4 t = pre[i];
                g.cut4(t, r * 4, valid);
                g.scatter4(Xs + s * BT * PE, PE, r * 4, t);
            }
        }
        __syncthreads();
        if (t0 + BT < T) prefetch(t0 + BT);   // in flight under the MFMAs
        if (active) {
            f32x4 acc[JW];
#pragma unroll
            for (int u = 0; u < JW; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < ST; ++s) {
                const float* ar = Xs + (s * BT + tt * 16 + j) * PE + kq;
                const float* br = Es + (s * G::VP + ub * 16 + j) * PE + kq;
#pragma unroll
                for (int k4 = 0; k4 < g.k4(); ++k4) {
                    const float av = ar[k4 * 4];
#pragma unroll
                    for (int u = 0; u < JW; ++u) acc[u] = mfma16(av, br[u * 16 * PE + k4 * 4], acc[u]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + tt * 16 + kq * 4 + r;
                if (t < T) {
#pragma unroll
                    for (int u = 0; u < JW; ++u) {
                        const int uu = (ub + u) * 16 + j;
                        if (G::FULL || uu < V) {
                            const float v = acc[u][r];
                            yrow[(long long)t * V + uu] = v;
                            s1 += v;
                            s2 = fmaf(v, v, s2);
                        }
                    }
                }
            }
        }
    }
    if (stats_part) {
        s1 = wave_sum64(s1); s2 = wave_sum64(s2);
        if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
        __syncthreads();
        if (tid < 2) stats_part[((long long)tid * Cout + c) * N + n] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    }
