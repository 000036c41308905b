// Host-side check of csrc/streaming.hip under AddressSanitizer and UBSan, on the CPU: every streaming entry point is called with
// one refused argument and a null stream, as tests/test_streaming_abi_cpu.py and tests/test_streambank_abi_cpu.py do, so no
// launch is reached and no GPU is needed.  Each call must return a negative status with a message that begins with the called
// entry point's own name.  Build and run from the repository root (host code only is instrumented):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/streaming_abi_sanitized.cpp tam_gcn_amd/csrc/streaming.hip tam_gcn_amd/csrc/lib.hip -o build/streaming_abi_sanitized
//   build/streaming_abi_sanitized
#include <cstdio>
#include <cstring>

#include "tamgcn.h"

extern "C" const char* tamgcn_last_error(void);

static int failures = 0;

static void refused(const char* fn, int rc) {
    const char* msg = tamgcn_last_error();
    const size_t n = strlen(fn);
    const bool ok = rc < 0 && strncmp(msg, fn, n) == 0 && msg[n] == ':';
    printf("%-26s rc %2d  %s%s\n", fn, rc, msg, ok ? "" : "   <-- not refused under its own name");
    failures += ok ? 0 : 1;
}

int main() {
    alignas(16) static double buf[64];
    void* p = buf;
    double* d = buf;
    float* f = (float*)p;
    long long* l = (long long*)p;
    int* i = (int*)p;
    // one ring: the bank's host bodies at S = 1
    refused("tamgcn_ring_push", tamgcn_ring_push(p, 17, 1, 60, 8, p, 16, l, nullptr));                       // n > cap
    refused("tamgcn_ring_push", tamgcn_ring_push(p, 4, 1, 60, 8, nullptr, 16, l, nullptr));
    refused("tamgcn_ring_plan", tamgcn_ring_plan(l, 16, 3, 17, 4, l, nullptr));                              // L > cap
    refused("tamgcn_window_nucla", tamgcn_window_nucla(d, 16, l, 3, i, 20, 65, 1, 0, f, nullptr));           // time_steps > 64
    refused("tamgcn_window_clip", tamgcn_window_clip(f, 1 << 30, l, 3, 3, 4, 1, 8, f, nullptr));             // plane above 2^30
    refused("tamgcn_window_vote", tamgcn_window_vote(f, l, 6, 4097, 27, f, f, l, nullptr));                  // K > 4096
    refused("tamgcn_score_ema", tamgcn_score_ema(f, l, 10, 1.0, d, l, f, l, f, nullptr));                    // beta = 1
    refused("tamgcn_score_ema", tamgcn_score_ema(f, l, 10, 0.8, d, nullptr, f, l, f, nullptr));
    // the bank
    refused("tamgcn_bank_push", tamgcn_bank_push(p, 1025, 2, 1, 60, 8, p, 16, l, i, i, nullptr));            // S > 1024
    refused("tamgcn_bank_push", tamgcn_bank_push(p, 3, 2, 1, 1 << 30, 8, p, 16, l, nullptr, nullptr, nullptr));   // row too large
    refused("tamgcn_bank_plan", tamgcn_bank_plan(l, i, 3, 16, 1 << 30, 9, 4, l, nullptr));                   // S B too large
    refused("tamgcn_bank_window_nucla", tamgcn_bank_window_nucla(d, 3, 16, l, 2, i, 20, 52, 20, 0, f, nullptr));   // centre joint = V
    refused("tamgcn_bank_window_clip", tamgcn_bank_window_clip(f, 0, 16, l, 2, 3, 17, 1, 8, f, nullptr));    // S = 0
    refused("tamgcn_bank_ema", tamgcn_bank_ema(f, l, i, 3, 2, 10, 0.8, d, l, f, l, f, nullptr, nullptr));    // no `advanced`
    refused("tamgcn_bank_ema", tamgcn_bank_ema(f, l, nullptr, 3, 0, 10, 0.8, d, l, f, l, f, i, nullptr));    // B = 0
    refused("tamgcn_bank_decide", tamgcn_bank_decide(l, f, i, i, l, 3, 0.6f, 0, l, l, f, l, 16, nullptr));   // hold = 0
    printf("%s\n", failures ? "FAILED" : "all refused");
    return failures ? 1 : 0;
}
