// Library-level entry points of libtamgcn_rgb.so: version and per-thread error text.
#include "rgb_common.h"

static thread_local char g_rgb_err[512] = "";

void tamgcn_rgb_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_rgb_err, sizeof(g_rgb_err), fmt, ap);
    va_end(ap);
}

extern "C" int tamgcn_rgb_version(void) { return TAMGCN_RGB_VERSION; }
extern "C" const char* tamgcn_rgb_last_error(void) { return g_rgb_err; }
