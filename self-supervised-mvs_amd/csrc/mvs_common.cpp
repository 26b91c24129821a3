// Error reporting, launch trace, tuning knobs + version for the C ABI (include/mvs_hip.h).  No exceptions cross the boundary:
// every entry point returns 0 or a negative code and leaves a message in a thread-local buffer.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
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

// Measurement knobs: the values and the name table, both generated from the list in tuning.h.  Full-string keys: an unknown or
// misspelt key is an error, never a silent hit on another knob.
#define MVS_KNOB_DEFAULT(key, def, lo, hi, doc) def,
MvsTuning g_tune = {MVS_KNOBS(MVS_KNOB_DEFAULT)};
struct MvsKnob { const char* name; int* var; int lo, hi; };
static const MvsKnob* mvs_find_knob(const char* key) {
#define MVS_KNOB_ROW(key, def, lo, hi, doc) {#key, &g_tune.key, lo, hi},
    static const MvsKnob knobs[] = {MVS_KNOBS(MVS_KNOB_ROW)};
    for (const MvsKnob& k : knobs)
        if (strcmp(key, k.name) == 0) return &k;
    return nullptr;
}
extern "C" int mvs_set_tuning(const char* key, int value) {
    MVS_REQUIRE(key, MVS_ERR_NULL, "mvs_set_tuning: null key");
    const MvsKnob* k = mvs_find_knob(key);
    if (!k) {
        mvs_set_error("mvs_set_tuning: unknown key '%s'", key);
        return MVS_ERR_UNSUPPORTED;
    }
    *k->var = value < k->lo ? k->lo : (value > k->hi ? k->hi : value);
    return MVS_OK;
}
// the knob's current value (bench.py --ab restores the LIBRARY's defaults after a toggle: tests/test_capi_symbols.py holds
// _lib.DEFAULT_TUNING against the values a freshly loaded library reports)
extern "C" int mvs_get_tuning(const char* key, int* value) {
    MVS_REQUIRE(key && value, MVS_ERR_NULL, "mvs_get_tuning: null argument");
    const MvsKnob* k = mvs_find_knob(key);
    if (!k) {
        mvs_set_error("mvs_get_tuning: unknown key '%s'", key);
        return MVS_ERR_UNSUPPORTED;
    }
    *value = *k->var;
    return MVS_OK;
}

extern "C" int mvs_version(void) { return 100; }  // 0.1.0
extern "C" int mvs_is_emulation(void) {
#if defined(MVS_CPU_EMUL)
    return 1;
#else
    return 0;
#endif
}
