// bsmm_host.h -- host-side pieces the .hip files share: the argument checks every entry point spells the same way, the launch with its
// error return, and the one place where a runtime dtype code (and the choice of the 16-byte path) becomes template arguments.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "bsmm.h"
#include "bsmm_common.h"

namespace bsmm {

inline bool dtype_ok(int dtype) { return dtype == BSMM_F32 || dtype == BSMM_F16 || dtype == BSMM_BF16; }
inline bool bsize_ok(int bsize) { return bsize == 8 || bsize == 16 || bsize == 32 || bsize == 64; }
inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }      // a: a power of two
inline bool aligned16(const void* p) { return aligned_to(p, 16); }
// a * b elements can be indexed by a 32-bit int
inline bool product_ok(int a, int b) { return (long long)a * (long long)b < (1ll << 31); }
// workgroups for `units` of them when the kernel strides what lies beyond max_grid
inline unsigned capped(unsigned long long units, int max_grid) { return (unsigned)(units < (unsigned long long)max_grid ? units : max_grid); }

// launch, and leave the calling function with HIP's error code if the launch failed
#define BSMM_LAUNCH(KERNEL, GRID, BLOCK, STREAM, ...)                  \
    do {                                                               \
        KERNEL<<<(GRID), (BLOCK), 0, (STREAM)>>>(__VA_ARGS__);         \
        if (int rc_ = (int)hipGetLastError()) return rc_;              \
    } while (0)

// f(DTf32{}), f(DTf16{}) or f(DTbf16{}) for a dtype code that dtype_ok accepts; f is a generic lambda that names the type as decltype(dt)
template <class F>
int with_dtype(int dtype, F&& f) {
    switch (dtype) {
        case BSMM_F32: return f(DTf32{});
        case BSMM_F16: return f(DTf16{});
        default: return f(DTbf16{});
    }
}

// the same with a second argument std::true_type{} / std::false_type{}: the 16-byte path or the element path
template <class F>
int with_dtype(int dtype, bool wide, F&& f) {
    return with_dtype(dtype, [&](auto dt) { return wide ? f(dt, std::true_type{}) : f(dt, std::false_type{}); });
}

}  // namespace bsmm
