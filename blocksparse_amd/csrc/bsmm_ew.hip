// bsmm_ew.hip -- C-ABI entry points of include/bsmm_ew.h: argument checks, the cut of the work over workgroups (a function of the sizes
// only), then launches of the kernels in bsmm_ew_kernels.h.  No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_ew.h"
#include "bsmm_ew_kernels.h"
#include "bsmm_host.h"

using namespace bsmm;

namespace {

// ---- the cuts -------------------------------------------------------------------------------------------------------------------------
// axis 0 backward: a row of N in chunks of EW_SPAN columns
inline int a0_chunks(int N) { return (N + EW_SPAN - 1) / EW_SPAN; }
// axis 1 backward: KU column units of V columns, CT of them per tile of 256 lanes, RL lanes per column unit; the rows in P partitions of at
// least 16 rows per lane (a row of K partials per partition: 1 / 24 of the bf16 traffic of 16 rows of dy, x and dx), 1024 at most
struct A1Cut {
    int KU, CT, RL, tiles, P, rpp;
};
inline A1Cut a1_cut(int K, int N, int V) {
    A1Cut c;
    c.KU = (K + V - 1) / V;
    c.CT = c.KU < 256 ? c.KU : 256;
    c.RL = 256 / c.CT;
    c.tiles = (c.KU + 255) / 256;
    const int per = 16 * c.RL, want = (N + per - 1) / per;
    c.P = want < 1 ? 1 : (want > 1024 ? 1024 : want);
    c.rpp = (N + c.P - 1) / c.P;
    return c;
}

int check(const bsmm_ew_args* a) {
    if (a == nullptr || a->K < 1 || a->N < 1 || !product_ok(a->K, a->N)) return BSMM_ERR_ARG;
    if ((a->axis != 0 && a->axis != 1) || !dtype_ok(a->dtype) || a->act < 0 || a->act > 2) return BSMM_ERR_ARG;
    return BSMM_OK;
}

int check_dropout(const bsmm_ew_args* a) {
    if (a->threshold < 0 || a->threshold > 65536 || (a->generate != 0 && a->generate != 1)) return BSMM_ERR_ARG;
    return BSMM_OK;
}

// floats of the partials.  Axis 1: the partition count of the element path, which the 16-byte path never exceeds (fewer column units, more
// lanes per unit, fewer partitions): a bound that is non-decreasing in K and in N whichever path the pointers select.
size_t grad_floats(const bsmm_ew_args* a) {
    if (a->axis == 0) {
        const int chunks = a0_chunks(a->N);
        return chunks > 1 ? (size_t)a->K * chunks : 0;
    }
    return (size_t)a1_cut(a->K, a->N, 1).P * (size_t)a->K;
}

int check_workspace(const bsmm_ew_args* a) {
    const size_t need = grad_floats(a) * sizeof(float);
    if (need == 0) return BSMM_OK;
    if (a->workspace == nullptr || !aligned_to(a->workspace, 4) || a->workspace_bytes < need) return BSMM_ERR_ARG;
    return BSMM_OK;
}

template <class DT, bool VEC>
int forward(const void* xv, const float* b, const void* rv, const uint64_t* state, uint32_t* mask, void* yv, int K, int N, int axis, int act, int drop,
            int threshold, float scale, void* stream) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t total = (uint32_t)((long long)K * N), groups = 4u * ((total + 31u) / 32u);
    BSMM_LAUNCH((ew_fwd_kernel<DT, VEC>), capped((groups + 255u) / 256u, EW_MAX_GRID), 256, st, static_cast<const T*>(xv), b, static_cast<const T*>(rv), state, mask,
              static_cast<T*>(yv), K, N, axis, act, drop, (uint32_t)threshold, scale, total, groups);
    return BSMM_OK;
}

// every forward form; the 16-byte path: aligned activations and, with a bias, groups that stay inside a row
int forward_any(const void* x, const float* b, const void* res, const uint64_t* state, uint32_t* mask, void* y, int K, int N, int axis, int dtype, int act,
                int drop, int threshold, float scale, void* stream) {
    bool vec = aligned16(x) && aligned16(y) && (res == nullptr || aligned16(res));
    if (b != nullptr) vec = vec && (axis == 0 ? N % 8 == 0 : K % 8 == 0 && aligned16(b));
    return with_dtype(dtype, vec, [&](auto dt, auto wide) {
        return forward<decltype(dt), wide>(x, b, res, state, mask, y, K, N, axis, act, drop, threshold, scale, stream);
    });
}

template <class DT, int V>
int backward(const void* dyv, const void* xyv, const float* b, const uint32_t* mask, void* dxv, float* db, int from_y, const bsmm_ew_args* a) {
    typedef typename DT::T T;
    const T* dy = static_cast<const T*>(dyv);
    const T* xy = static_cast<const T*>(xyv);
    T* dx = static_cast<T*>(dxv);
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    float* ws = static_cast<float*>(a->workspace);
    const int K = a->K, N = a->N;
    const unsigned sum_grid = (unsigned)((K + 15) / 16);
    if (a->axis == 0) {
        const int chunks = a0_chunks(N);
        const unsigned long long units = (unsigned long long)K * chunks;
        BSMM_LAUNCH((ew_bwd_a0_kernel<DT, V>), capped(units, EW_MAX_GRID), 256, st, dy, xy, b, mask, dx, chunks > 1 ? ws : db, N, chunks, a->act, from_y, a->scale, (uint32_t)units);
        if (chunks > 1) BSMM_LAUNCH(ew_sum_partials_kernel, sum_grid, 256, st, ws, db, K, chunks, (size_t)1, (size_t)chunks);
        return BSMM_OK;
    }
    const A1Cut c = a1_cut(K, N, V);
    const unsigned long long units = (unsigned long long)c.P * c.tiles;
    BSMM_LAUNCH((ew_bwd_a1_kernel<DT, V>), capped(units, EW_MAX_GRID), 256, st, dy, xy, b, mask, dx, ws, K, N, c.KU, c.CT, c.RL, c.tiles, c.rpp, a->act, from_y, a->scale,
              (uint32_t)units);
    BSMM_LAUNCH(ew_sum_partials_kernel, sum_grid, 256, st, ws, db, K, c.P, (size_t)K, (size_t)1);
    return BSMM_OK;
}

int backward_any(const void* dy, const void* xy, const float* b, const uint32_t* mask, void* dx, float* db, int from_y, const bsmm_ew_args* a) {
    bool vec = aligned16(dy) && (dx == nullptr || aligned16(dx)) && (a->act == 0 || aligned16(xy));
    vec = vec && (a->axis == 0 ? a->N % 8 == 0 : a->K % 8 == 0 && aligned16(b));
    return with_dtype(a->dtype, vec, [&](auto dt, auto wide) { return backward<decltype(dt), (wide ? 8 : 1)>(dy, xy, b, mask, dx, db, from_y, a); });
}

}  // namespace

extern "C" {

size_t bsmm_ew_workspace_bytes(const bsmm_ew_args* args, int32_t which) {
    if (check(args) != BSMM_OK) return 0;
    if (which != BSMM_EW_BIAS_ACT_GRAD && which != BSMM_EW_BIAS_ACT_DROPOUT_GRAD) return 0;
    return grad_floats(args) * sizeof(float);
}

int bsmm_bias_act(const void* x, const float* b, void* y, const bsmm_ew_args* args) {
    if (int rc = check(args)) return rc;
    if (x == nullptr || b == nullptr || y == nullptr) return BSMM_ERR_ARG;
    return forward_any(x, b, nullptr, nullptr, nullptr, y, args->K, args->N, args->axis, args->dtype, args->act, EW_DROP_NONE, 0, 1.f, args->stream);
}

int bsmm_bias_act_grad(const void* dy, const void* x_or_y, const float* b, void* dx, float* db, const bsmm_ew_args* args) {
    if (int rc = check(args)) return rc;
    if (dy == nullptr || b == nullptr || db == nullptr) return BSMM_ERR_ARG;
    if (args->act != BSMM_ACT_NONE && (x_or_y == nullptr || dx == nullptr)) return BSMM_ERR_ARG;
    if (int rc = check_workspace(args)) return rc;
    return backward_any(dy, x_or_y, b, nullptr, dx, db, args->act == BSMM_ACT_RELU ? 1 : 0, args);
}

int bsmm_dropout_mask(uint32_t* mask, const uint64_t* state, int64_t n, int32_t threshold, void* stream) {
    if (mask == nullptr || state == nullptr || n < 1 || n >= ((int64_t)1 << 31) || threshold < 0 || threshold > 65536) return BSMM_ERR_ARG;
    if (!aligned_to(mask, 4) || !aligned_to(state, 8)) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t total = (uint32_t)n, words = (total + 31u) / 32u;
    BSMM_LAUNCH(ew_mask_kernel, capped((words + 255u) / 256u, EW_MAX_GRID), 256, st, mask, state, (uint32_t)threshold, total, words);
    return BSMM_OK;
}

int bsmm_dropout_apply(const void* x, const uint32_t* mask, void* y, int64_t n, float scale, int32_t dtype, void* stream) {
    if (x == nullptr || mask == nullptr || y == nullptr || n < 1 || n >= ((int64_t)1 << 31) || !dtype_ok(dtype) || !aligned_to(mask, 4)) return BSMM_ERR_ARG;
    return forward_any(x, nullptr, nullptr, nullptr, const_cast<uint32_t*>(mask), y, 1, (int)n, 0, dtype, BSMM_ACT_NONE, EW_DROP_READ, 0, scale, stream);
}

int bsmm_bias_act_dropout(const void* x, const float* b, const void* residual, const uint64_t* state, uint32_t* mask, void* y,
                          const bsmm_ew_args* args) {
    if (int rc = check(args)) return rc;
    if (int rc = check_dropout(args)) return rc;
    if (x == nullptr || mask == nullptr || y == nullptr || (b == nullptr && args->act != BSMM_ACT_NONE)) return BSMM_ERR_ARG;
    if (args->generate && (state == nullptr || !aligned_to(state, 8))) return BSMM_ERR_ARG;
    if (!aligned_to(mask, 4)) return BSMM_ERR_ARG;
    return forward_any(x, b, residual, state, mask, y, args->K, args->N, args->axis, args->dtype, args->act,
                       args->generate ? EW_DROP_GENERATE : EW_DROP_READ, args->threshold, args->scale, args->stream);
}

int bsmm_bias_act_dropout_grad(const void* dy, const void* x, const float* b, const uint32_t* mask, void* dx, float* db, const bsmm_ew_args* args) {
    if (int rc = check(args)) return rc;
    if (dy == nullptr || x == nullptr || b == nullptr || mask == nullptr || dx == nullptr || db == nullptr || !aligned_to(mask, 4)) return BSMM_ERR_ARG;
    if (int rc = check_workspace(args)) return rc;
    return backward_any(dy, x, b, mask, dx, db, 0, args);
}

}  // extern "C"
