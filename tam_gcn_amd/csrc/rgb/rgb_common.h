// Shared host helpers of libtamgcn_rgb.so (gfx950 / CDNA4 only): error text and check macros of its own.  ../common.h and
// ../feeder_common.h are included for their device helpers only (clip_of, philox4x32_10); nothing here defines or calls a
// symbol of libtamgcn.so.
#pragma once
#include "../common.h"
#include "../feeder_common.h"
#include "../../../include/tamgcn_rgb.h"

void tamgcn_rgb_set_error(const char* fmt, ...);

#define RGB_CHECK(cond, ...)                        \
    do {                                            \
        if (!(cond)) {                              \
            tamgcn_rgb_set_error(__VA_ARGS__);      \
            return -1;                              \
        }                                           \
    } while (0)

#define RGB_LAUNCH_CHECK(name)                                                            \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess) {                                                           \
            tamgcn_rgb_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));   \
            return -2;                                                                    \
        }                                                                                 \
    } while (0)

static inline bool rgb_al(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
