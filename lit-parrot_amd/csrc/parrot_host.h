// Host-only part of parrot_common.h: error reporting, the tuning hook and small predicates.  No HIP type appears here, so the
// headers that only do host arithmetic (w4_plan.h's layout, gemm_plan.h) also compile with a plain C++ compiler.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/parrot_hip.h"

namespace parrot {

// ---------------------------------------------------------------- errors
void set_error(const char* fmt, ...);

#define PARROT_REQUIRE(cond, ...)                 \
    do {                                          \
        if (!(cond)) {                            \
            ::parrot::set_error(__VA_ARGS__);     \
            return PARROT_EINVAL;                 \
        }                                         \
    } while (0)

#define PARROT_UNSUPPORTED(cond, ...)             \
    do {                                          \
        if (!(cond)) {                            \
            ::parrot::set_error(__VA_ARGS__);     \
            return PARROT_EUNSUPPORTED;           \
        }                                         \
    } while (0)

// The A/B switches behind the measurements of DESIGN.md exist only in a diagnostic build (hipcc -DPARROT_DIAG, `python
// lit-parrot_amd/_build.py --diag`): the shipped library reads no environment variable and keeps no tuning state.
#ifdef PARROT_DIAG
inline int tune_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
#else
inline int tune_env(const char*, int dflt) { return dflt; }
#endif

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace parrot
