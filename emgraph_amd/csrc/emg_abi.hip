// emg_abi.hip — ABI plumbing: version, thread-local error string, the run-time switches.
#include <stdlib.h>

#include <string>

#include "emg_common.hpp"

namespace emg {

static thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// the library's run-time switches, in the order of emg_common.hpp's enum Switch (tests/test_switches.py holds this table, the
// Python package's and DESIGN.md's to the same names)
struct SwitchDecl { const char* name; enum { Int, Word } kind; const char* doc; };
static const SwitchDecl kSwitches[] = {
    {"EMG_CACHE_POLICY", SwitchDecl::Int, "0 | 1: the fused SGD kernel's cache-policy form off / forced; anything else: by size"},
    {"EMG_WIDE_GROUPS", SwitchDecl::Int, "0: narrow rows share a wave, non-zero: a wave per group; unset: by batch size"},
    {"EMG_GROUPING", SwitchDecl::Word, "sort | count | bucket: the grouping backend; anything else: by size"},
    {"EMG_BUCKET_CAP", SwitchDecl::Int, "test aid: LDS capacity of a bucket, honoured inside (0, kBucketCap)"},
    {"EMG_APPLY_HALF", SwitchDecl::Int, "0: rows of 17-32 chunks one segment per wave"},
    {"EMG_APPLY_FIX", SwitchDecl::Int, "0: the apply's run-time optimizer switch everywhere"},
    {"EMG_DENSE_FUSED", SwitchDecl::Int, "0: Adam's dense pass a launch of its own, non-zero: inside the apply launch; unset: by table size"},
    {"EMG_BF16_V4", SwitchDecl::Int, "0: the v3 count kernel everywhere, 1 (default): v4 for one counter, 2: v4 in every mode at 400 columns"},
    {"EMG_PRE_BITMAP", SwitchDecl::Int, "0: the emitting prefilter kernel instead of the bitmap form"},
    {"EMG_PRE_V4", SwitchDecl::Int, "0: the bitmap prefilter through the v3 kernel at every width"},
};
static_assert(sizeof(kSwitches) / sizeof(kSwitches[0]) == SW_COUNT, "one row per Switch");

const char* sw_word(Switch s) {
    const char* e = getenv(kSwitches[s].name);
    return e && e[0] ? e : nullptr;
}

int sw_int(Switch s) {
    const char* e = sw_word(s);
    return e ? atoi(e) : kSwUnset;
}

}  // namespace emg

extern "C" int emg_version(void) { return EMG_ABI_VERSION; }
extern "C" const char* emg_last_error(void) { return emg::g_last_error.c_str(); }
extern "C" const char* emg_target(void) { return "gfx950"; }
// sha256 (first 16 hex digits) over the kernel sources this library was built from (csrc/build.sh): the committed rocprofv3
// tables and PMC passes under profiles/ carry the hash of the binary they measured, and bench.py quotes one only for the same hash
#ifndef EMG_SRC_HASH
#define EMG_SRC_HASH "unknown"
#endif
extern "C" const char* emg_source_hash(void) { return EMG_SRC_HASH; }
