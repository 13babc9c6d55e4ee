// gcn_error.hip — the library-wide state of the C-ABI of include/gcn_spmm.h: the last error's text, one per thread,
// the two hooks through which every .hip file of this directory records it (declared in gcn_internal.h), and the
// ABI version.  No kernel.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "gcn_spmm.h"
#include "gcn_internal.h"

namespace {

thread_local char g_err[256] = "";

}   // namespace

int gcn_internal_fail(int code, const char *msg)
{
    std::snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int gcn_internal_fail_hip(int hip_error, const char *where)
{
    std::snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString((hipError_t)hip_error));
    return hip_error;
}

extern "C" {

int gcn_abi_version(void) { return GCN_ABI_VERSION; }

const char *gcn_last_error(void) { return g_err; }

}   // extern "C"
