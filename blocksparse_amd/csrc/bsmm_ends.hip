// bsmm_ends.hip -- C-ABI entry points of include/bsmm_ends.h: argument checks, the choice of a path (a function of the sizes and of pointer
// alignment only), then launches of the kernels in bsmm_ends_kernels.h.  No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_ends.h"
#include "bsmm_ends_kernels.h"
#include "bsmm_host.h"

using namespace bsmm;

namespace {

inline size_t elem_bytes(int dtype) { return dtype == BSMM_F32 ? 4 : 2; }

// ---- softmax cross-entropy ----------------------------------------------------------------------------------------------------------
int xent_check(const bsmm_xent_args* a) {
    if (a == nullptr || a->N < 1 || a->K < 1 || !product_ok(a->N, a->K) || !dtype_ok(a->dtype)) return BSMM_ERR_ARG;
    return BSMM_OK;
}

int xent_path(const bsmm_xent_args* a) {
    const int K = a->K;
    const bool vec = aligned16(a->x) && aligned16(a->g) && K % 8 == 0;
    // the element path holds half as many elements per lane (16 accesses in flight instead of 4): its two register limits are halved
    const int reg_max = vec ? BSMM_XENT_REG_MAX : BSMM_XENT_REG_MAX / 2, wide_max = vec ? BSMM_XENT_WIDE_MAX : BSMM_XENT_WIDE_MAX / 2;
    int path, rows_per_group = 1;
    if (K <= BSMM_XENT_SHORT_MAX) {
        path = BSMM_XENT_SHORT;
        rows_per_group = 4;
    } else if (K <= reg_max) {
        path = BSMM_XENT_REG;
    } else if (K <= wide_max) {
        path = BSMM_XENT_REG_WIDE;
    } else {
        path = BSMM_XENT_LONG;
    }
    if (vec) path |= BSMM_XENT_VEC;
    if (((long long)a->N + rows_per_group - 1) / rows_per_group > ENDS_MAX_GRID) path |= BSMM_XENT_STRIDED;
    return path;
}

template <class DT, int V>
int xent_forward(const bsmm_xent_args* a, int path) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const T* x = static_cast<const T*>(a->x);
    T* g = static_cast<T*>(a->g);
    const int N = a->N, K = a->K;
    const float gscale = a->dtype == BSMM_F16 ? BSMM_XENT_F16_SCALE : 1.f;
    const int units = (K + V - 1) / V;
    switch (path & 0xff) {
        case BSMM_XENT_SHORT: {
            const unsigned grid = capped(((unsigned long long)N + 3) / 4, ENDS_MAX_GRID);
            // units a lane holds: 1 or 2 on the 16-byte path (K <= 512, <= 1024), 4 or 16 on the element path (K <= 256, <= 1024)
            if constexpr (V == 8) {
                if (units <= 64) BSMM_LAUNCH((xent_rows_kernel<DT, 8, 1, 64>), grid, 256, st, x, a->labels, a->loss, g, N, K, gscale);
                else BSMM_LAUNCH((xent_rows_kernel<DT, 8, 2, 64>), grid, 256, st, x, a->labels, a->loss, g, N, K, gscale);
            } else {
                if (units <= 256) BSMM_LAUNCH((xent_rows_kernel<DT, 1, 4, 64>), grid, 256, st, x, a->labels, a->loss, g, N, K, gscale);
                else BSMM_LAUNCH((xent_rows_kernel<DT, 1, 16, 64>), grid, 256, st, x, a->labels, a->loss, g, N, K, gscale);
            }
            break;
        }
        case BSMM_XENT_REG:
            BSMM_LAUNCH((xent_rows_kernel<DT, V, (V == 8 ? 4 : 16), 256>), capped(N, ENDS_MAX_GRID), 256, st, x, a->labels, a->loss, g, N, K, gscale);
            break;
        case BSMM_XENT_REG_WIDE:
            BSMM_LAUNCH((xent_rows_kernel<DT, V, (V == 8 ? 4 : 16), 1024>), capped(N, ENDS_MAX_GRID), 1024, st, x, a->labels, a->loss, g, N, K, gscale);
            break;
        default:
            BSMM_LAUNCH((xent_long_kernel<DT, V>), capped(N, ENDS_MAX_GRID), 1024, st, x, a->labels, a->loss, g, N, K, gscale);
            break;
    }
    return BSMM_OK;
}

template <class DT, int V>
int xent_backward(const bsmm_xent_args* a) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const uint32_t upr = (uint32_t)(a->K / V), units = (uint32_t)a->N * upr;
    const float unscale = a->dtype == BSMM_F16 ? 1.f / BSMM_XENT_F16_SCALE : 1.f;
    BSMM_LAUNCH((xent_bwd_kernel<DT, V>), capped(((unsigned long long)units + 255) / 256, ENDS_MAX_GRID), 256, st, static_cast<const T*>(a->g), a->dy,
                static_cast<T*>(a->dx), units, upr, unscale);
    return BSMM_OK;
}

// ---- embedding ----------------------------------------------------------------------------------------------------------------------
int embed_check(const bsmm_embed_args* a) {
    if (a == nullptr || a->C < 1 || a->K < 1 || a->nIdx < 1 || !product_ok(a->C, a->K) || !product_ok(a->nIdx, a->K) || !dtype_ok(a->dtype))
        return BSMM_ERR_ARG;
    return BSMM_OK;
}

inline int embed_chunks(int nIdx) { return (nIdx + EMBED_CHUNK - 1) / EMBED_CHUNK; }
inline size_t embed_grad_floats(const bsmm_embed_args* a) { return (size_t)2 * embed_chunks(a->nIdx) * (size_t)a->K; }

// lanes of a team: the column units of a row rounded up to whole waves, 256 at most
inline int embed_team(int KU) { return KU <= 64 ? 64 : (KU <= 128 ? 128 : 256); }

template <class DT, int V>
int embed_backward(const void* dyv, const int32_t* idx, const int32_t* order, float* dw, const bsmm_embed_args* a) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    float* ws = static_cast<float*>(a->workspace);
    const int K = a->K, KU = (K + V - 1) / V, CT = embed_team(KU), tiles = (KU + CT - 1) / CT, teams = 256 / CT;
    const unsigned long long items1 = (unsigned long long)embed_chunks(a->nIdx) * tiles, items2 = (unsigned long long)a->C * tiles;
    if (items1 >= (1ull << 32) || items2 >= (1ull << 32)) return BSMM_ERR_ARG;
    BSMM_LAUNCH((embed_grad_chunks_kernel<DT, V>), capped((items1 + teams - 1) / teams, ENDS_MAX_GRID), 256, st, static_cast<const T*>(dyv), idx, order, dw, ws,
                a->C, K, a->nIdx, CT, tiles, (uint32_t)items1);
    BSMM_LAUNCH((embed_grad_merge_kernel<V>), capped((items2 + teams - 1) / teams, ENDS_MAX_GRID), 256, st, idx, order, dw, ws, a->C, K, a->nIdx, CT, tiles,
                (uint32_t)items2);
    return BSMM_OK;
}

}  // namespace

extern "C" {

int bsmm_xent_path(const bsmm_xent_args* args) {
    if (int rc = xent_check(args)) return rc;
    return xent_path(args);
}

int bsmm_xent_fwd(const bsmm_xent_args* args) {
    if (int rc = xent_check(args)) return rc;
    if (args->x == nullptr || args->labels == nullptr || args->loss == nullptr || args->g == nullptr) return BSMM_ERR_ARG;
    const size_t es = elem_bytes(args->dtype);
    if (!aligned_to(args->x, es) || !aligned_to(args->g, es) || !aligned_to(args->labels, 4) || !aligned_to(args->loss, 4)) return BSMM_ERR_ARG;
    const int path = xent_path(args);
    const bool vec = (path & BSMM_XENT_VEC) != 0;
    return with_dtype(args->dtype, vec, [&](auto dt, auto wide) { return xent_forward<decltype(dt), (wide ? 8 : 1)>(args, path); });
}

int bsmm_xent_bwd(const bsmm_xent_args* args) {
    if (int rc = xent_check(args)) return rc;
    if (args->g == nullptr || args->dy == nullptr || args->dx == nullptr) return BSMM_ERR_ARG;
    const size_t es = elem_bytes(args->dtype);
    if (!aligned_to(args->g, es) || !aligned_to(args->dx, es) || !aligned_to(args->dy, 4)) return BSMM_ERR_ARG;
    const bool vec = aligned16(args->g) && aligned16(args->dx) && args->K % 8 == 0;
    return with_dtype(args->dtype, vec, [&](auto dt, auto wide) { return xent_backward<decltype(dt), (wide ? 8 : 1)>(args); });
}

size_t bsmm_ends_workspace_bytes(const bsmm_embed_args* args, int32_t which) {
    if (which != BSMM_ENDS_EMBED_GRAD || embed_check(args) != BSMM_OK) return 0;
    return embed_grad_floats(args) * sizeof(float);
}

int bsmm_embed_fwd(const void* w, const int32_t* idx, void* y, const bsmm_embed_args* args) {
    if (int rc = embed_check(args)) return rc;
    if (w == nullptr || idx == nullptr || y == nullptr) return BSMM_ERR_ARG;
    const size_t es = elem_bytes(args->dtype), row_bytes = (size_t)args->K * es;
    if (!aligned_to(w, es) || !aligned_to(y, es) || !aligned_to(idx, 4)) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    if (aligned16(w) && aligned16(y) && row_bytes % 16 == 0) {
        const uint32_t upr = (uint32_t)(row_bytes / 16), units = (uint32_t)args->nIdx * upr;
        BSMM_LAUNCH(embed_fwd_kernel<uint4>, capped(((unsigned long long)units + 255) / 256, ENDS_MAX_GRID), 256, st, static_cast<const uint4*>(w), idx,
                    static_cast<uint4*>(y), args->C, upr, units);
    } else if (es == 4) {
        const uint32_t upr = (uint32_t)args->K, units = (uint32_t)args->nIdx * upr;
        BSMM_LAUNCH(embed_fwd_kernel<uint32_t>, capped(((unsigned long long)units + 255) / 256, ENDS_MAX_GRID), 256, st, static_cast<const uint32_t*>(w), idx,
                    static_cast<uint32_t*>(y), args->C, upr, units);
    } else {
        const uint32_t upr = (uint32_t)args->K, units = (uint32_t)args->nIdx * upr;
        BSMM_LAUNCH(embed_fwd_kernel<uint16_t>, capped(((unsigned long long)units + 255) / 256, ENDS_MAX_GRID), 256, st, static_cast<const uint16_t*>(w), idx,
                    static_cast<uint16_t*>(y), args->C, upr, units);
    }
    return BSMM_OK;
}

int bsmm_embed_grad(const void* dy, const int32_t* idx, const int32_t* order, float* dw, const bsmm_embed_args* args) {
    if (int rc = embed_check(args)) return rc;
    if (dy == nullptr || idx == nullptr || order == nullptr || dw == nullptr) return BSMM_ERR_ARG;
    const size_t es = elem_bytes(args->dtype);
    if (!aligned_to(dy, es) || !aligned_to(idx, 4) || !aligned_to(order, 4) || !aligned_to(dw, 4)) return BSMM_ERR_ARG;
    if (args->workspace == nullptr || !aligned_to(args->workspace, 4) || args->workspace_bytes < embed_grad_floats(args) * sizeof(float))
        return BSMM_ERR_ARG;
    const bool vec = aligned16(dy) && aligned16(dw) && aligned16(args->workspace) && args->K % 8 == 0;
    return with_dtype(args->dtype, vec, [&](auto dt, auto wide) { return embed_backward<decltype(dt), (wide ? 8 : 1)>(dy, idx, order, dw, args); });
}

}  // extern "C"
