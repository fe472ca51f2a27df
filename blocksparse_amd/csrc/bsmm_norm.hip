// bsmm_norm.hip -- C-ABI entry points of include/bsmm_norm.h: argument checks, the cut of the work over workgroups (a function of the
// sizes only), then launches of the kernels in bsmm_norm_kernels.h.  No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_norm.h"
#include "bsmm_host.h"
#include "bsmm_norm_kernels.h"

using namespace bsmm;

namespace {

inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }
inline int vec_of(int dtype) { return dtype == BSMM_F32 ? 4 : 8; }

// ---- the cuts.  Every count depends on N and K / S only, never on S: a call with S segments computes, bit for bit, what S calls on the
// slices compute. -----------------------------------------------------------------------------------------------------------------------
// axis 1 backward: workgroups per segment; a group of lanes then walks at least 16 rows (the dg / db partials are one row of 2 K floats per
// group: 1 / 8 of the traffic of 16 bf16 rows of x, dy and dx)
inline int a1_groups(int N) {
    const int p = N / 16;
    return p < 1 ? 1 : (p > 512 ? 512 : p);
}
struct A0Cut {
    int strips, split, rps, tiles;
};
// axis 0: strips of 64 * V columns; a segment's rows in `split` slices of rps rows (at least 32) so that about 1024 workgroups exist
inline A0Cut a0_cut(int Ks, int N, int dtype) {
    A0Cut c;
    const int sw = 64 * vec_of(dtype);
    c.strips = (N + sw - 1) / sw;
    const int want = (1024 + c.strips - 1) / c.strips, most = (Ks + 31) / 32;
    c.split = want < most ? want : most;
    c.rps = (Ks + c.split - 1) / c.split;
    c.tiles = (Ks + LN_A0_ROWS - 1) / LN_A0_ROWS;
    return c;
}
// floats of the slices' partial sums, as a bound that is non-decreasing in N and in Ks: split * N <= (1024 / strips + 1) * N <= 1024 * 64 V + N
inline size_t a0_slice_floats(int Ks, int N, int S, int dtype) {
    const size_t a = (size_t)1024 * 64 * vec_of(dtype) + (size_t)N, b = (size_t)((Ks + 31) / 32) * (size_t)N;
    return round4(2 * (size_t)S * (a < b ? a : b));
}

int check(const bsmm_ln_args* a) {
    if (a == nullptr || a->K < 1 || a->N < 1 || a->segments < 1 || a->K % a->segments != 0) return BSMM_ERR_ARG;
    if ((a->axis != 0 && a->axis != 1) || !dtype_ok(a->dtype) || (a->relu != 0 && a->relu != 1)) return BSMM_ERR_ARG;
    return BSMM_OK;
}

size_t workspace_floats(const bsmm_ln_args* a, int backward) {
    const int Ks = a->K / a->segments;
    if (a->axis == 1) return backward ? (size_t)4 * a1_groups(a->N) * 2 * (size_t)a->K : 0;      // (four groups per workgroup at most)
    const size_t slices = a0_slice_floats(Ks, a->N, a->segments, a->dtype);
    if (!backward) return slices;
    const A0Cut c = a0_cut(Ks, a->N, a->dtype);
    return slices + round4(2 * (size_t)a->segments * a->N) + (size_t)c.strips * 2 * (size_t)a->K;
}

int check_workspace(const bsmm_ln_args* a, int backward) {
    const size_t need = workspace_floats(a, backward) * sizeof(float);
    if (need == 0) return BSMM_OK;
    if (a->workspace == nullptr || !aligned_to(a->workspace, 4) || a->workspace_bytes < need) return BSMM_ERR_ARG;
    return BSMM_OK;
}

// grid sizes stay inside 2^31 - 1 blocks
inline bool grids_ok(const bsmm_ln_args* a) {
    const long long lim = 0x7fffffffll, S = a->segments, N = a->N, Ks = a->K / a->segments;
    if (a->axis == 1) return N * S <= lim;
    const A0Cut c = a0_cut((int)Ks, a->N, a->dtype);
    return (long long)c.strips * c.tiles * S <= lim && (long long)c.strips * c.split * S <= lim && S * N <= lim;
}

template <class DT, bool VEC>
int forward(const void* xv, const float* g, const float* b, void* yv, float* mean, float* rstd, const bsmm_ln_args* a) {
    typedef typename DT::T T;
    const T* x = static_cast<const T*>(xv);
    T* y = static_cast<T*>(yv);
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const int K = a->K, N = a->N, S = a->segments, Ks = K / S;
    if (a->axis == 1) {
        const long long R = (long long)N * S;
        if (Ks <= LN_WAVE_LIMIT) BSMM_LAUNCH((ln_fwd_a1_kernel<DT, VEC, 64>), (unsigned)((R + 3) / 4), 256, st, x, g, b, y, mean, rstd, N, S, Ks, a->relu, a->epsilon);
        else if (Ks <= LN_ROW_LIMIT) BSMM_LAUNCH((ln_fwd_a1_kernel<DT, VEC, 256>), (unsigned)R, 256, st, x, g, b, y, mean, rstd, N, S, Ks, a->relu, a->epsilon);
        else BSMM_LAUNCH((ln_fwd_a1_long_kernel<DT, VEC>), (unsigned)R, 256, st, x, g, b, y, mean, rstd, N, S, Ks, a->relu, a->epsilon);
        return BSMM_OK;
    }
    const A0Cut c = a0_cut(Ks, N, a->dtype);
    float* ws = static_cast<float*>(a->workspace);
    BSMM_LAUNCH((ln_stats_a0_kernel<DT, VEC>), (unsigned)(c.strips * c.split * S), 256, st, x, ws, N, S, Ks, c.strips, c.split, c.rps);
    BSMM_LAUNCH(ln_stats_merge_a0_kernel, (unsigned)(((long long)S * N + 255) / 256), 256, st, ws, mean, rstd, N, S, Ks, c.split, c.rps, a->epsilon);
    BSMM_LAUNCH((ln_norm_a0_kernel<DT, VEC>), (unsigned)(c.strips * c.tiles * S), 256, st, x, g, b, mean, rstd, y, N, Ks, c.strips, c.tiles, a->relu);
    return BSMM_OK;
}

template <class DT, bool VEC>
int backward(const void* dyv, const void* xv, const float* g, const float* b, const float* mean, const float* rstd, void* dxv, float* dg, float* db,
             const bsmm_ln_args* a) {
    typedef typename DT::T T;
    const T* dy = static_cast<const T*>(dyv);
    const T* x = static_cast<const T*>(xv);
    T* dx = static_cast<T*>(dxv);
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const int K = a->K, N = a->N, S = a->segments, Ks = K / S;
    float* ws = static_cast<float*>(a->workspace);
    const unsigned sum_grid = (unsigned)((2ll * K + 63) / 64);
    if (a->axis == 1) {
        const int P = a1_groups(N);
        int rows = P;                                       // rows of partials
        if (Ks <= LN_WAVE_LIMIT) {
            BSMM_LAUNCH((ln_bwd_a1_kernel<DT, VEC, 64>), (unsigned)(P * S), 256, st, dy, x, g, b, mean, rstd, dx, ws, N, S, Ks, P, a->relu);
            rows = 4 * P;
        } else if (Ks <= LN_ROW_LIMIT) {
            BSMM_LAUNCH((ln_bwd_a1_kernel<DT, VEC, 256>), (unsigned)(P * S), 256, st, dy, x, g, b, mean, rstd, dx, ws, N, S, Ks, P, a->relu);
        } else {
            BSMM_LAUNCH((ln_bwd_a1_long_kernel<DT, VEC>), (unsigned)((long long)N * S), 256, st, dy, x, g, b, mean, rstd, dx, N, S, Ks, a->relu);
            BSMM_LAUNCH((ln_dgdb_a1_kernel<DT>), dim3((unsigned)((K + 255) / 256), (unsigned)P), 256, st, dy, x, g, b, mean, rstd, ws, N, K, Ks, P, a->relu);
        }
        BSMM_LAUNCH(ln_sum_partials_kernel, sum_grid, 256, st, ws, dg, db, K, rows);
        return BSMM_OK;
    }
    const A0Cut c = a0_cut(Ks, N, a->dtype);
    float* merged = ws + a0_slice_floats(Ks, N, S, a->dtype);
    float* part = merged + round4(2 * (size_t)S * N);
    BSMM_LAUNCH((ln_bwd_sums_a0_kernel<DT, VEC>), (unsigned)(c.strips * c.split * S), 256, st, dy, x, g, b, mean, rstd, ws, part, N, S, Ks, c.strips, c.split, c.rps,
              a->relu);
    BSMM_LAUNCH(ln_sums_merge_a0_kernel, (unsigned)(((long long)S * N + 255) / 256), 256, st, ws, merged, N, S, c.split);
    BSMM_LAUNCH((ln_bwd_dx_a0_kernel<DT, VEC>), (unsigned)(c.strips * c.tiles * S), 256, st, dy, x, g, b, mean, rstd, merged, dx, N, S, Ks, c.strips, c.tiles,
              a->relu);
    BSMM_LAUNCH(ln_sum_partials_kernel, sum_grid, 256, st, part, dg, db, K, c.strips);
    return BSMM_OK;
}

// the 16-byte path: the contiguous run is a whole number of 16-byte groups and every pointer a lane loads 16 bytes from is aligned
inline bool run_ok(const bsmm_ln_args* a) {
    const int run = a->axis == 0 ? a->N : a->K / a->segments;
    return run % vec_of(a->dtype) == 0;
}

}  // namespace

extern "C" {

size_t bsmm_layer_norm_workspace_bytes(const bsmm_ln_args* args, int32_t backward) {
    if (check(args) != BSMM_OK) return 0;
    return workspace_floats(args, backward ? 1 : 0) * sizeof(float);
}

int bsmm_layer_norm(const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, const bsmm_ln_args* args) {
    if (int rc = check(args)) return rc;
    if (x == nullptr || g == nullptr || b == nullptr || y == nullptr || mean == nullptr || rstd == nullptr) return BSMM_ERR_ARG;
    if (int rc = check_workspace(args, 0)) return rc;
    if (!grids_ok(args)) return BSMM_ERR_UNSUPPORTED;
    bool vec = run_ok(args) && aligned16(x) && aligned16(y);
    vec = vec && (args->axis == 0 ? aligned16(mean) && aligned16(rstd) : aligned16(g) && aligned16(b));
    return with_dtype(args->dtype, vec, [&](auto dt, auto wide) { return forward<decltype(dt), wide>(x, g, b, y, mean, rstd, args); });
}

int bsmm_layer_norm_grad(const void* dy, const void* x, const float* g, const float* b, const float* mean, const float* rstd, void* dx, float* dg,
                         float* db, const bsmm_ln_args* args) {
    if (int rc = check(args)) return rc;
    if (dy == nullptr || x == nullptr || g == nullptr || b == nullptr || mean == nullptr || rstd == nullptr || dx == nullptr || dg == nullptr ||
        db == nullptr)
        return BSMM_ERR_ARG;
    if (int rc = check_workspace(args, 1)) return rc;
    if (!grids_ok(args)) return BSMM_ERR_UNSUPPORTED;
    bool vec = run_ok(args) && aligned16(dy) && aligned16(x) && aligned16(dx);
    vec = vec && (args->axis == 0 ? aligned16(mean) && aligned16(rstd) && aligned16(args->workspace) : aligned16(g) && aligned16(b));
    return with_dtype(args->dtype, vec, [&](auto dt, auto wide) {
        return backward<decltype(dt), wide>(dy, x, g, b, mean, rstd, dx, dg, db, args);
    });
}

}  // extern "C"
