// Error reporting + version for the C ABI (include/mvs_hip.h).  No exceptions cross the boundary:
// every entry point returns 0 or a negative code and leaves a message in a thread-local buffer.
#include <stdarg.h>
#include <stdio.h>
#include "mvs_rt.h"

static thread_local char g_err[512] = "";

// Launch trace: every launch check notes its label (a string literal) here, so a test can tell WHICH size-selected arm a call took
// (the persistent convolution is bit-identical to the one-tile kernel: its output cannot say).  Same lifetime rules as g_err:
// thread local, fixed size, no allocation, no device work -- one pointer store per launch check.  The first MVS_TRACE_MAX labels
// since the last read are kept, later ones only counted.
static const int MVS_TRACE_MAX = 64;
static thread_local const char* g_trace[MVS_TRACE_MAX];
static thread_local int g_ntrace = 0;

void mvs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int mvs_check_launch(const char* what) {
    if (g_ntrace < MVS_TRACE_MAX) g_trace[g_ntrace] = what;
    if (g_ntrace < 0x7fffffff) ++g_ntrace;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        mvs_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return MVS_ERR_LAUNCH;
    }
    return MVS_OK;
}

extern "C" const char* mvs_last_error(void) { return g_err; }

// Labels of the launch checks this thread has passed since the previous call, comma-joined into buf (cap bytes incl. the
// terminator; whole labels only), then forgotten.  Returns how many checks there were: more than the labels written when the
// record (MVS_TRACE_MAX) or buf was too small.  buf == NULL only clears.
extern "C" int mvs_launch_trace(char* buf, int cap) {
    const int n = g_ntrace, kept = n < MVS_TRACE_MAX ? n : MVS_TRACE_MAX;
    g_ntrace = 0;
    if (!buf || cap <= 0) return n;
    int pos = 0;
    buf[0] = 0;
    for (int i = 0; i < kept; ++i) {
        int len = 0;
        while (g_trace[i][len]) ++len;
        if (pos + len + (i ? 1 : 0) + 1 > cap) break;
        if (i) buf[pos++] = ',';
        for (int c = 0; c < len; ++c) buf[pos++] = g_trace[i][c];
        buf[pos] = 0;
    }
    return n;
}
extern "C" int mvs_version(void) { return 100; }  // 0.1.0
extern "C" int mvs_is_emulation(void) {
#if defined(MVS_CPU_EMUL)
    return 1;
#else
    return 0;
#endif
}
