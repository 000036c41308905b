// Library-level entry points of libtamgcn_xmodal.so: version and per-thread error text.
#include "xm_common.h"

static thread_local char g_xm_err[512] = "";

void tamgcn_xm_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_xm_err, sizeof(g_xm_err), fmt, ap);
    va_end(ap);
}

extern "C" int tamgcn_xm_version(void) { return TAMGCN_XM_VERSION; }
extern "C" const char* tamgcn_xm_last_error(void) { return g_xm_err; }
