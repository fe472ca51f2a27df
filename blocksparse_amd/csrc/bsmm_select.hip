// bsmm_select.hip -- C-ABI entry points of include/bsmm_select.h: argument checks, the choice of the team geometry (K only) and of the
// 16-byte or the element form (K and pointer alignment only), then one launch of a kernel of bsmm_select_kernels.h.  No allocation, no host
// sync, no environment, no state.
#include <cstdint>
#include <type_traits>

#include "bsmm_select.h"
#include "bsmm_host.h"
#include "bsmm_select_kernels.h"

using namespace bsmm;

namespace {

// what every entry point checks; row_limit: the call holds a row in registers; null_ptr: a required pointer is NULL
int check(const bsmm_select_args* a, bool row_limit, bool topk, const float* mask, bool null_ptr) {
    if (null_ptr || a == nullptr || a->R < 1 || a->K < 1 || !product_ok(a->R, a->K) || !dtype_ok(a->dtype)) return BSMM_ERR_ARG;
    if (topk && (a->k < 1 || a->k > a->K)) return BSMM_ERR_ARG;
    if (mask != nullptr && (a->mask_rows < 1 || a->R % a->mask_rows != 0)) return BSMM_ERR_ARG;
    if (row_limit && a->K > BSMM_SELECT_MAX_K) return BSMM_ERR_UNSUPPORTED;
    return BSMM_OK;
}

inline bool wide_k(int K, int dtype) { return K % (dtype == BSMM_F32 ? 4 : 8) == 0; }

// f(elements per lane, waves per team) as integral constants, from K alone
template <class F>
int with_geom(int K, F&& f) {
    typedef std::integral_constant<int, 8> E8;
    typedef std::integral_constant<int, 16> E16;
    if (K <= BSMM_SELECT_WAVE8_MAX) return f(E8{}, std::integral_constant<int, 1>{});
    if (K <= BSMM_SELECT_WAVE16_MAX) return f(E16{}, std::integral_constant<int, 1>{});
    if (K <= BSMM_SELECT_GROUP2_MAX) return f(E16{}, std::integral_constant<int, 2>{});
    return f(E16{}, std::integral_constant<int, 4>{});
}

template <int NW>
inline unsigned grid_of(int R) { return ((unsigned)R + SEL_ROWS<NW> - 1u) / SEL_ROWS<NW>; }

}  // namespace

extern "C" {

int bsmm_select_path(int K, int dtype, int aligned) {
    if (K < 1 || !dtype_ok(dtype)) return BSMM_ERR_ARG;
    if (K > BSMM_SELECT_MAX_K) return BSMM_ERR_UNSUPPORTED;
    const int geom = K <= BSMM_SELECT_WAVE8_MAX    ? BSMM_SELECT_PATH_WAVE8
                     : K <= BSMM_SELECT_WAVE16_MAX ? BSMM_SELECT_PATH_WAVE16
                     : K <= BSMM_SELECT_GROUP2_MAX ? BSMM_SELECT_PATH_GROUP2
                                                   : BSMM_SELECT_PATH_GROUP4;
    return geom + ((aligned && wide_k(K, dtype)) ? 1 : 0);
}

int bsmm_rectified_top_k(const void* x, void* y, const bsmm_select_args* args) {
    if (int rc = check(args, true, true, nullptr, x == nullptr || y == nullptr)) return rc;
    const bool wide = wide_k(args->K, args->dtype) && aligned16(x) && aligned16(y);
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) -> int {
        typedef decltype(dt) DT;
        typedef typename DT::T T;
        return with_geom(args->K, [&](auto el, auto nw) -> int {
            BSMM_LAUNCH((select_rect_kernel<DT, el.value, nw.value, w.value>), grid_of<nw.value>(args->R), SEL_LANES<nw.value>, st,
                        static_cast<const T*>(x), static_cast<T*>(y), (uint32_t)args->R, (uint32_t)args->K, (uint32_t)args->k, args->rebase != 0);
            return BSMM_OK;
        });
    });
}

int bsmm_masked_top_k_softmax(const void* x, const float* mask, void* y, const bsmm_select_args* args) {
    if (int rc = check(args, true, true, mask, x == nullptr || y == nullptr)) return rc;
    const bool wide = wide_k(args->K, args->dtype) && aligned16(x) && aligned16(y) && aligned16(mask);
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) -> int {
        typedef decltype(dt) DT;
        typedef typename DT::T T;
        return with_geom(args->K, [&](auto el, auto nw) -> int {
            BSMM_LAUNCH((select_softmax_kernel<DT, el.value, nw.value, w.value>), grid_of<nw.value>(args->R), SEL_LANES<nw.value>, st,
                        static_cast<const T*>(x), mask, static_cast<T*>(y), (uint32_t)args->R, (uint32_t)args->K, (uint32_t)args->k,
                        (uint32_t)(mask != nullptr ? args->mask_rows : 1), args->scale);
            return BSMM_OK;
        });
    });
}

int bsmm_masked_softmax_grad(const void* dy, const void* y, const float* mask, void* dx, const bsmm_select_args* args) {
    if (int rc = check(args, true, false, mask, dy == nullptr || y == nullptr || dx == nullptr)) return rc;
    const bool wide = wide_k(args->K, args->dtype) && aligned16(dy) && aligned16(y) && aligned16(dx) && aligned16(mask);
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) -> int {
        typedef decltype(dt) DT;
        typedef typename DT::T T;
        return with_geom(args->K, [&](auto el, auto nw) -> int {
            BSMM_LAUNCH((select_softmax_grad_kernel<DT, el.value, nw.value, w.value>), grid_of<nw.value>(args->R), SEL_LANES<nw.value>, st,
                        static_cast<const T*>(dy), static_cast<const T*>(y), mask, static_cast<T*>(dx), (uint32_t)args->R, (uint32_t)args->K,
                        (uint32_t)(mask != nullptr ? args->mask_rows : 1), args->scale);
            return BSMM_OK;
        });
    });
}

int bsmm_sparse_relu(const void* x, void* y, const bsmm_select_args* args) {
    if (int rc = check(args, true, false, nullptr, x == nullptr || y == nullptr)) return rc;
    const bool wide = wide_k(args->K, args->dtype) && aligned16(x) && aligned16(y);
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) -> int {
        typedef decltype(dt) DT;
        typedef typename DT::T T;
        return with_geom(args->K, [&](auto el, auto nw) -> int {
            BSMM_LAUNCH((select_sparse_relu_kernel<DT, el.value, nw.value, w.value>), grid_of<nw.value>(args->R), SEL_LANES<nw.value>, st,
                        static_cast<const T*>(x), static_cast<T*>(y), (uint32_t)args->R, (uint32_t)args->K, args->alpha);
            return BSMM_OK;
        });
    });
}

int bsmm_select_relu_grad(const void* dz, const void* y, void* dx, const bsmm_select_args* args) {
    if (int rc = check(args, false, false, nullptr, dz == nullptr || y == nullptr || dx == nullptr)) return rc;
    const uint32_t n = (uint32_t)args->R * (uint32_t)args->K, V = args->dtype == BSMM_F32 ? 4u : 8u;
    const bool wide = n % V == 0 && aligned16(dz) && aligned16(y) && aligned16(dx);
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) -> int {
        typedef decltype(dt) DT;
        typedef typename DT::T T;
        constexpr int W = w.value ? SEL_V<DT> : 1;
        const uint32_t units = n / W;
        BSMM_LAUNCH((select_relu_grad_kernel<DT, W>), capped((units + 255u) / 256u, SEL_EW_MAX_GRID), 256, st, static_cast<const T*>(dz),
                    static_cast<const T*>(y), static_cast<T*>(dx), units);
        return BSMM_OK;
    });
}

}  // extern "C"
