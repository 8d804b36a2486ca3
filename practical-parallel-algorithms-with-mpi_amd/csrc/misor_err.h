// misor_err.h -- error reporting of the host units, 2D (misor_grid.h) and 3D
// (misor_grid3.h) alike.  Internal: nothing here is part of include/misor.h.
#pragma once

#include "misor_internal.h"

// helpers shared by the units: not exported from libmisor.so
#define MISOR_HIDDEN __attribute__((visibility("hidden")))

// record an error message for misor_last_error and return code (misor_api.hip)
MISOR_HIDDEN int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess)                                                             \
            return fail(MISOR_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                        \
    } while (0)

// return the code of a failed call of the library's own (one that has
// already recorded its message through fail)
#define MISOR_TRY(x)           \
    do {                       \
        const int rc_ = (x);   \
        if (rc_) return rc_;   \
    } while (0)

#define NCCLCHK(x)                                                                       \
    do {                                                                                  \
        ncclResult_t r_ = (x);                                                            \
        if (r_ != ncclSuccess)                                                            \
            return fail(MISOR_ECOMM, "%s: %s (%s:%d)", #x, ncclGetErrorString(r_),        \
                        __FILE__, __LINE__);                                              \
    } while (0)
