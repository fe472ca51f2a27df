// bsmm_norm_kernels.h -- kernels behind include/bsmm_norm.h: layer norm (forward and gradients) in both activation layouts.  All of them
// are memory bound; a lane moves 16 bytes per load (V = 8 elements of a 16-bit type, 4 of fp32) on the VEC path and single elements,
// still coalesced, on the element path.  K features in S segments of Ks = K / S; N samples; mean / rstd are fp32 [S][N].
//
//   feature axis 1, x (N, K): row n, segment s is the contiguous run x + (n * S + s) * Ks, so the tensor is N * S rows of Ks elements.
//     ln_fwd_a1_kernel<G>   one group of G lanes per row -- a wave (G = 64) for Ks <= 2048, a workgroup (G = 256) for Ks <= 8192: a lane keeps
//                           LN_LANE_ELEMS = 32 elements in registers, x is read ONCE.  Mean first, then the mean of squared deviations
//                           from the registers (the two-pass form).
//     ln_fwd_a1_long_kernel Ks > 8192 = LN_ROW_LIMIT: a workgroup streams the row three times (the sum for the mean, the squared deviations
//                           from that mean, then the normalise pass; the second and third read come from L2): the two-pass form as well.
//     ln_bwd_a1_kernel<G>   same shapes; a group walks rows n, n + stride, ...: per row the two per-sample sums and dx from registers, and
//                           across its rows the dg / db contributions of the lane's own 32 columns in 64 accumulators, stored once at the
//                           end as one row of partials.  x and dy are read ONCE.
//     ln_bwd_a1_long_kernel + ln_dgdb_a1_kernel   Ks > 8192: rows streamed twice; dg / db partials by a column walk of their own (dg in
//                           fp64 within a partial, see ln_dg_term).
//   feature axis 0, x (K, N): the reduction runs down a stride-N column.  A workgroup owns a strip of 64 * V contiguous columns and a slice
//   of a segment's rows; its four waves take every fourth row, a lane owns V columns and keeps their sums in registers, the waves meet in
//   LDS (sp_reduce_a0_kernel of bsmm_sparsity_kernels.h reads this layout the same way).  A segment's rows are cut into `split` slices so
//   that a few strips still fill the chip; the slices' partial sums go to the workspace and a merge kernel adds them in ascending order.
//     ln_stats_a0_kernel    per slice: sum x, then sum (x - the slice's mean)^2 in a second pass over the slice (two-pass within the slice;
//                           the rows come from L1 / L2 the second time).  ln_stats_merge_a0_kernel adds the slices' sums -> mean, and joins
//                           their squared deviations about that mean: each slice's own plus rows * (slice mean - mean)^2, all terms
//                           >= 0.  No term depends on which row of the segment comes first.
//     ln_norm_a0_kernel     the normalise pass, every CU busy whatever the strip count; it re-reads x from L2 / Infinity Cache.
//     ln_bwd_sums_a0_kernel the per-sample sums (partials per slice) and, per row, the strip's dg / db contribution by a wave reduction
//                           (partials per strip; dg in fp64 within a strip);  ln_sums_merge_a0_kernel;  ln_bwd_dx_a0_kernel writes dx.
//   ln_sum_partials_kernel  dg / db = the partial rows added in ascending order (four slices per output, joined in LDS in a fixed order).
#pragma once
#include "bsmm_vec.h"

namespace bsmm {

constexpr int LN_LANE_ELEMS = 32;                      // elements of a row one lane keeps in registers (axis 1)
constexpr int LN_WAVE_LIMIT = 64 * LN_LANE_ELEMS;      // longest row segment one wave takes
constexpr int LN_ROW_LIMIT = 256 * LN_LANE_ELEMS;      // longest row segment that is read once (8192)
constexpr int LN_A0_ROWS = 64;                         // rows of a segment per workgroup of the axis-0 elementwise passes

template <class DT>
struct LnV {
    static constexpr int V = DT::is16 ? 8 : 4;         // elements per 16 bytes
    static constexpr int CH = LN_LANE_ELEMS / V;       // 16-byte chunks a lane holds
};

// sum over the G lanes that share a row: a wave, or the four waves of the workgroup through `red` (every lane gets the same bits)
template <int G>
__device__ __forceinline__ float ln_group_sum(float v, float* red) {
    v = wave_sum(v);
    if constexpr (G == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return v;
}

// acc + d * (x - mean) * rstd in fp64, for the dg of the kernels in which one thread or one wave sums a feature over the samples
// (ln_dgdb_a1_kernel, ln_bwd_sums_a0_kernel); the partial is rounded to fp32 once, when it is stored.  A feature whose dg is hundreds of
// times the mean |dg| (an outlier feature: xhat = 90 in every sample) otherwise carries three fp32 roundings per term and lands about one fp32
// step of its own value away, which is several 1e-5 of the mean |dg|.  The fp32 xhat that masks dy and feeds dx is unchanged.
__device__ __forceinline__ double ln_dg_term(float d, float x, float mean, float rstd, double acc) {
    return fma((double)d, ((double)x - (double)mean) * (double)rstd, acc);
}

// ---- V consecutive elements <-> V floats; VEC: one 16-byte access (bsmm_vec.h), all V valid; else element accesses, those at or beyond lim skipped ----
template <class DT, bool VEC>
__device__ __forceinline__ void ln_load(const typename DT::T* p, int lim, float* v) {
    constexpr int V = LnV<DT>::V;
    if constexpr (!VEC) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = j < lim ? DT::to_f32(p[j]) : 0.f;
    } else {
        vec_load<DT, V>(p, v);
    }
}

template <class DT, bool VEC>
__device__ __forceinline__ void ln_store(typename DT::T* p, int lim, const float* v) {
    constexpr int V = LnV<DT>::V;
    if constexpr (!VEC) {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < lim) p[j] = DT::from_f32(v[j]);
    } else {
        vec_store<DT, V>(p, v);
    }
}

// NV consecutive floats (gain / bias / statistics); VEC: 16-byte loads
template <int NV, bool VEC>
__device__ __forceinline__ void ln_load_f32(const float* p, int lim, float* v) {
    if constexpr (!VEC) {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = j < lim ? p[j] : 0.f;
    } else {
        vec_load_f32<NV>(p, v);
    }
}

// =====================================================================================================================================
// feature axis 1
// =====================================================================================================================================
// grid: N * S rows / (256 / G) groups.  VEC: x, y, g, b 16-byte aligned and Ks % V == 0.
template <class DT, bool VEC, int G>
__global__ void __launch_bounds__(256) ln_fwd_a1_kernel(const typename DT::T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                        typename DT::T* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int N, int S,
                                                        int Ks, int relu, float eps) {
    constexpr int V = LnV<DT>::V, CH = LnV<DT>::CH;
    __shared__ float red[4];
    const int t = threadIdx.x & (G - 1);
    const long long rs = G == 256 ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rs >= (long long)N * S) return;                  // (G == 64 only: a whole wave leaves, and waves never meet)
    const int n = (int)(rs / S), s = (int)(rs - (long long)n * S);
    const typename DT::T* xr = x + (size_t)rs * Ks;
    float v[CH][V];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = (c * G + t) * V;
        if (e < Ks) {
            ln_load<DT, VEC>(xr + e, Ks - e, v[c]);
#pragma unroll
            for (int j = 0; j < V; ++j) sum += v[c][j];
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) v[c][j] = 0.f;
        }
    }
    const float m = ln_group_sum<G>(sum, red) / (float)Ks;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = (c * G + t) * V;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = e + j < Ks ? v[c][j] - m : 0.f;
            v[c][j] = d;
            sq = fmaf(d, d, sq);
        }
    }
    const float r = 1.f / sqrtf(ln_group_sum<G>(sq, red) / (float)Ks + eps);
    if (t == 0) {
        mean[(size_t)s * N + n] = m;
        rstd[(size_t)s * N + n] = r;
    }
    typename DT::T* yr = y + (size_t)rs * Ks;
    const float* gs = g + (size_t)s * Ks;
    const float* bs = b + (size_t)s * Ks;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = (c * G + t) * V;
        if (e < Ks) {
            float gg[V], bb[V], o[V];
            ln_load_f32<V, VEC>(gs + e, Ks - e, gg);
            ln_load_f32<V, VEC>(bs + e, Ks - e, bb);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float pre = fmaf(v[c][j] * r, gg[j], bb[j]);
                o[j] = relu ? fmaxf(pre, 0.f) : pre;
            }
            ln_store<DT, VEC>(yr + e, Ks - e, o);
        }
    }
}

// grid: N * S workgroups, one per row segment of any length
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ln_fwd_a1_long_kernel(const typename DT::T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                             typename DT::T* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int N,
                                                             int S, int Ks, int relu, float eps) {
    constexpr int V = LnV<DT>::V;
    __shared__ float red[4];
    const long long rs = blockIdx.x;
    const int n = (int)(rs / S), s = (int)(rs - (long long)n * S);
    const typename DT::T* xr = x + (size_t)rs * Ks;
    float s1 = 0.f, s2 = 0.f;
    for (int e = threadIdx.x * V; e < Ks; e += 256 * V) {
        float v[V];
        ln_load<DT, VEC>(xr + e, Ks - e, v);                 // (elements past the row read as zero)
#pragma unroll
        for (int j = 0; j < V; ++j) s1 += v[j];
    }
    const float m = ln_group_sum<256>(s1, red) / (float)Ks;
    for (int e = threadIdx.x * V; e < Ks; e += 256 * V) {
        float v[V];
        ln_load<DT, VEC>(xr + e, Ks - e, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = e + j < Ks ? v[j] - m : 0.f;
            s2 = fmaf(d, d, s2);
        }
    }
    const float r = 1.f / sqrtf(ln_group_sum<256>(s2, red) / (float)Ks + eps);
    if (threadIdx.x == 0) {
        mean[(size_t)s * N + n] = m;
        rstd[(size_t)s * N + n] = r;
    }
    typename DT::T* yr = y + (size_t)rs * Ks;
    const float* gs = g + (size_t)s * Ks;
    const float* bs = b + (size_t)s * Ks;
    for (int e = threadIdx.x * V; e < Ks; e += 256 * V) {
        float v[V], gg[V], bb[V], o[V];
        ln_load<DT, VEC>(xr + e, Ks - e, v);
        ln_load_f32<V, VEC>(gs + e, Ks - e, gg);
        ln_load_f32<V, VEC>(bs + e, Ks - e, bb);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float pre = fmaf((v[j] - m) * r, gg[j], bb[j]);
            o[j] = relu ? fmaxf(pre, 0.f) : pre;
        }
        ln_store<DT, VEC>(yr + e, Ks - e, o);
    }
}

// grid: P * S workgroups; workgroup (p, s) walks rows n = p * WPB + w, + P * WPB, ... of segment s (WPB = 256 / G groups, group w).
// part[(p * WPB + w)][2][K]: the group's dg / db contributions, every column of segment s stored (zeros when it had no row).
template <class DT, bool VEC, int G>
__global__ void __launch_bounds__(256) ln_bwd_a1_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ x,
                                                        const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, typename DT::T* __restrict__ dx, float* __restrict__ part, int N,
                                                        int S, int Ks, int P, int relu) {
    constexpr int V = LnV<DT>::V, CH = LnV<DT>::CH, WPB = 256 / G;
    __shared__ float red[4];
    const int t0 = threadIdx.x & (G - 1), w = G == 256 ? 0 : (int)(threadIdx.x >> 6);
    const int p = blockIdx.x / S, s = blockIdx.x - p * S;
    const float* gs = g + (size_t)s * Ks;
    const float* bs = b + (size_t)s * Ks;
    const float rK = 1.f / (float)Ks;
    float adg[CH][V], adb[CH][V];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) adg[c][j] = adb[c][j] = 0.f;
    for (int n = p * WPB + w; n < N; n += P * WPB) {       // (G == 256: one n for the whole workgroup, the barriers inside are uniform)
        // the lane index is made opaque per row: the 32 loop-invariant `e + j < Ks` masks would otherwise be kept in scalar registers across the
        // loop and spill; recomputing a compare per element costs nothing next to the loads
        int t = t0;
        asm volatile("" : "+v"(t));
        const float m = mean[(size_t)s * N + n], r = rstd[(size_t)s * N + n];
        const size_t row = ((size_t)n * S + s) * Ks;
        float xh[CH][V], dv[CH][V];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * G + t) * V;
            if (e < Ks) {
                float gg[V], bb[V] = {};
                ln_load<DT, VEC>(x + row + e, Ks - e, xh[c]);
                ln_load<DT, VEC>(dy + row + e, Ks - e, dv[c]);
                ln_load_f32<V, VEC>(gs + e, Ks - e, gg);
                if (relu) ln_load_f32<V, VEC>(bs + e, Ks - e, bb);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const bool live = VEC || e + j < Ks;
                    const float xhat = live ? (xh[c][j] - m) * r : 0.f;
                    float d = live ? dv[c][j] : 0.f;
                    if (relu && !(fmaf(xhat, gg[j], bb[j]) > 0.f)) d = 0.f;
                    adg[c][j] = fmaf(d, xhat, adg[c][j]);
                    adb[c][j] += d;
                    const float dg_ = d * gg[j];
                    s1 = fmaf(xhat, dg_, s1);
                    s2 += dg_;
                    xh[c][j] = xhat;
                    dv[c][j] = dg_;
                }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) xh[c][j] = dv[c][j] = 0.f;
            }
        }
        const float sum1 = ln_group_sum<G>(s1, red), sum2 = ln_group_sum<G>(s2, red);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = (c * G + t) * V;
            if (e < Ks) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) o[j] = (dv[c][j] - fmaf(xh[c][j], sum1, sum2) * rK) * r;
                ln_store<DT, VEC>(dx + row + e, Ks - e, o);
            }
        }
    }
    const size_t K = (size_t)S * Ks;
    float* pg = part + ((size_t)(p * WPB + w) * 2) * K + (size_t)s * Ks;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = (c * G + t0) * V;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (e + j < Ks) {
                pg[e + j] = adg[c][j];
                pg[K + e + j] = adb[c][j];
            }
        }
    }
}

// grid: N * S workgroups; dx of a row segment of any length, the row read twice
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ln_bwd_a1_long_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ x,
                                                             const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, typename DT::T* __restrict__ dx, int N, int S, int Ks,
                                                             int relu) {
    constexpr int V = LnV<DT>::V;
    __shared__ float red[4];
    const long long rs = blockIdx.x;
    const int n = (int)(rs / S), s = (int)(rs - (long long)n * S);
    const size_t row = (size_t)rs * Ks;
    const float* gs = g + (size_t)s * Ks;
    const float* bs = b + (size_t)s * Ks;
    const float m = mean[(size_t)s * N + n], r = rstd[(size_t)s * N + n], rK = 1.f / (float)Ks;
    float sum1 = 0.f, sum2 = 0.f;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        float s1 = 0.f, s2 = 0.f;
        for (int e = threadIdx.x * V; e < Ks; e += 256 * V) {
            float xv[V], dv[V], gg[V], bb[V] = {}, o[V];
            ln_load<DT, VEC>(x + row + e, Ks - e, xv);
            ln_load<DT, VEC>(dy + row + e, Ks - e, dv);
            ln_load_f32<V, VEC>(gs + e, Ks - e, gg);
            if (relu) ln_load_f32<V, VEC>(bs + e, Ks - e, bb);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool live = e + j < Ks;
                const float xhat = live ? (xv[j] - m) * r : 0.f;
                float d = live ? dv[j] : 0.f;
                if (relu && !(fmaf(xhat, gg[j], bb[j]) > 0.f)) d = 0.f;
                const float dg_ = d * gg[j];
                s1 = fmaf(xhat, dg_, s1);
                s2 += dg_;
                o[j] = (dg_ - fmaf(xhat, sum1, sum2) * rK) * r;
            }
            if (pass == 1) ln_store<DT, VEC>(dx + row + e, Ks - e, o);
        }
        if (pass == 0) {
            sum1 = ln_group_sum<256>(s1, red);
            sum2 = ln_group_sum<256>(s2, red);
        }
    }
}

// grid (ceil(K / 256), P): thread = one feature k, rows n = p, p + P, ...; part[p][2][K]
template <class DT>
__global__ void __launch_bounds__(256) ln_dgdb_a1_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ x,
                                                         const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ part, int N, int K, int Ks, int P, int relu) {
    const int k = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (k >= K) return;
    const int s = k / Ks;
    const float gk = g[k], bk = relu ? b[k] : 0.f;
    double adg = 0.0;                                      // (fp64, rounded once below: see ln_dg_term)
    float adb = 0.f;
    for (int n = p; n < N; n += P) {
        const float xv = DT::to_f32(x[(size_t)n * K + k]), m = mean[(size_t)s * N + n], r = rstd[(size_t)s * N + n];
        const float xhat = (xv - m) * r;
        float d = DT::to_f32(dy[(size_t)n * K + k]);
        if (relu && !(fmaf(xhat, gk, bk) > 0.f)) d = 0.f;
        adg = ln_dg_term(d, xv, m, r, adg);
        adb += d;
    }
    part[((size_t)p * 2) * K + k] = (float)adg;
    part[((size_t)p * 2 + 1) * K + k] = adb;
}

// dg[k] = sum_p part[p][0][k], db[k] = sum_p part[p][1][k], p ascending.  grid ceil(2 K / 64): 64 outputs x 4 slices of the partial rows.
__global__ void __launch_bounds__(256) ln_sum_partials_kernel(const float* __restrict__ part, float* __restrict__ dg, float* __restrict__ db, int K, int PR) {
    __shared__ float red[4][64];
    const int kl = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long long o = (long long)blockIdx.x * 64 + kl;
    const bool live = o < 2ll * K;
    const int which = live && o >= K ? 1 : 0, k = live ? (int)(o - (long long)which * K) : 0;
    const int q = (PR + 3) / 4, p0 = sl * q, p1 = min(PR, p0 + q);
    float sum = 0.f;
    if (live)
        for (int p = p0; p < p1; ++p) sum += part[((size_t)p * 2 + which) * K + k];
    red[sl][kl] = sum;
    __syncthreads();
    if (sl == 0 && live) {
        const float total = ((red[0][kl] + red[1][kl]) + red[2][kl]) + red[3][kl];
        (which ? db : dg)[k] = total;
    }
}

// =====================================================================================================================================
// feature axis 0
// =====================================================================================================================================
// column of slot j of this lane in the strip that starts at n0: 16 bytes per lane, or single elements 64 apart
template <int V, bool VEC>
__device__ __forceinline__ int ln_col(int n0, int lane, int j) {
    return VEC ? n0 + lane * V + j : n0 + j * 64 + lane;
}

template <class DT, bool VEC>
__device__ __forceinline__ void ln_load_row(const typename DT::T* row, int n0, int lane, int N, float* v) {
    constexpr int V = LnV<DT>::V;
    if constexpr (VEC) {
        const int nb = n0 + lane * V;
        if (nb < N) {
            ln_load<DT, true>(row + nb, V, v);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = 0.f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int n = n0 + j * 64 + lane;
            v[j] = n < N ? DT::to_f32(row[n]) : 0.f;
        }
    }
}

template <class DT, bool VEC>
__device__ __forceinline__ void ln_store_row(typename DT::T* row, int n0, int lane, int N, const float* v) {
    constexpr int V = LnV<DT>::V;
    if constexpr (VEC) {
        const int nb = n0 + lane * V;
        if (nb < N) ln_store<DT, true>(row + nb, V, v);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int n = n0 + j * 64 + lane;
            if (n < N) row[n] = DT::from_f32(v[j]);
        }
    }
}

// fp32 per-column values (statistics, per-sample sums) of this lane's V columns; columns outside read as zero
template <int V, bool VEC>
__device__ __forceinline__ void ln_load_cols(const float* base, int n0, int lane, int N, float* v) {
    if constexpr (VEC) {
        const int nb = n0 + lane * V;
        if (nb < N) {
            ln_load_f32<V, true>(base + nb, V, v);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = 0.f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int n = n0 + j * 64 + lane;
            v[j] = n < N ? base[n] : 0.f;
        }
    }
}

// the four waves' per-column sums a[V], c[V] -> wave 0 stores their totals (wave order 0, 1, 2, 3) at out0 / out1 [column]
template <int V, bool VEC>
__device__ __forceinline__ void ln_join_waves(float (*lds)[2][V][64], const float* a, const float* c, float* out0, float* out1, int n0, int N) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        lds[w][0][j][lane] = a[j];
        lds[w][1][j][lane] = c[j];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int n = ln_col<V, VEC>(n0, lane, j);
            if (n < N) {
                out0[n] = ((lds[0][0][j][lane] + lds[1][0][j][lane]) + lds[2][0][j][lane]) + lds[3][0][j][lane];
                out1[n] = ((lds[0][1][j][lane] + lds[1][1][j][lane]) + lds[2][1][j][lane]) + lds[3][1][j][lane];
            }
        }
    }
}

// rows of slice sp of a segment of Ks rows cut into slices of rps rows (the last slices of a long segment may be empty)
__device__ __forceinline__ int ln_slice_rows(int Ks, int rps, int sp) {
    return max(min(Ks, (sp + 1) * rps) - sp * rps, 0);
}

// grid: strips * S * split workgroups (strip fastest).  ws[(sp * S + s)][2][N] over the rows [sp * rps, (sp + 1) * rps) of segment s:
// [0] sum x, [1] sum (x - the SLICE's mean)^2 -- two passes over the slice, the second from L1 / L2, which it has just been read into.
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ln_stats_a0_kernel(const typename DT::T* __restrict__ x, float* __restrict__ ws, int N, int S, int Ks, int strips,
                                                          int split, int rps) {
    constexpr int V = LnV<DT>::V;
    __shared__ float lds[4][2][V][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int strip = blockIdx.x % strips, rest = blockIdx.x / strips, s = rest % S, sp = rest / S;
    const int n0 = strip * 64 * V;
    const typename DT::T* xs = x + (size_t)s * Ks * N;
    const int k0 = sp * rps, rows = ln_slice_rows(Ks, rps, sp), k1 = k0 + rows;
    float s1[V], s2[V], m[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll 4
    for (int k = k0 + w; k < k1; k += 4) {
        float v[V];
        ln_load_row<DT, VEC>(xs + (size_t)k * N, n0, lane, N, v);
#pragma unroll
        for (int j = 0; j < V; ++j) s1[j] += v[j];
    }
    // every wave gets the four waves' sums (wave order 0, 1, 2, 3) and so the slice's mean of its columns
#pragma unroll
    for (int j = 0; j < V; ++j) lds[w][0][j][lane] = s1[j];
    __syncthreads();
    const float rrows = 1.f / (float)max(rows, 1);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        s1[j] = ((lds[0][0][j][lane] + lds[1][0][j][lane]) + lds[2][0][j][lane]) + lds[3][0][j][lane];
        m[j] = s1[j] * rrows;
    }
#pragma unroll 4
    for (int k = k0 + w; k < k1; k += 4) {
        float v[V];
        ln_load_row<DT, VEC>(xs + (size_t)k * N, n0, lane, N, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = v[j] - m[j];
            s2[j] = fmaf(d, d, s2[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) lds[w][1][j][lane] = s2[j];
    __syncthreads();
    if (w == 0) {
        float* out = ws + ((size_t)sp * S + s) * 2 * N;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int n = ln_col<V, VEC>(n0, lane, j);
            if (n < N) {
                out[n] = s1[j];
                out[N + n] = ((lds[0][1][j][lane] + lds[1][1][j][lane]) + lds[2][1][j][lane]) + lds[3][1][j][lane];
            }
        }
    }
}

// one thread per (s, n), the slices in ascending order: mean = sum of the slices' sums / Ks, and the squared deviations from THAT mean
// are, exactly, each slice's own (about its own mean) plus rows * (slice mean - mean)^2: every term is >= 0, nothing cancels
__global__ void __launch_bounds__(256) ln_stats_merge_a0_kernel(const float* __restrict__ ws, float* __restrict__ mean, float* __restrict__ rstd, int N, int S,
                                                                int Ks, int split, int rps, float eps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)S * N) return;
    const int s = (int)(i / N), n = (int)(i - (long long)s * N);
    // (unrolled: the loads of eight slices are in flight together; the adds keep their ascending order)
    float s1 = 0.f;
#pragma unroll 8
    for (int sp = 0; sp < split; ++sp) s1 += ws[((size_t)sp * S + s) * 2 * N + n];
    const float m = s1 / (float)Ks;
    float s2 = 0.f;
#pragma unroll 8
    for (int sp = 0; sp < split; ++sp) {
        const float* p = ws + ((size_t)sp * S + s) * 2 * N + n;
        const int rows = ln_slice_rows(Ks, rps, sp);
        const float d = p[0] * (1.f / (float)max(rows, 1)) - m;
        s2 += fmaf((float)rows * d, d, p[N]);
    }
    mean[i] = m;
    rstd[i] = 1.f / sqrtf(s2 / (float)Ks + eps);
}

// grid: strips * ceil(Ks / LN_A0_ROWS) * S workgroups (strip fastest); wave w takes rows w, w + 4, ... of the workgroup's LN_A0_ROWS
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ln_norm_a0_kernel(const typename DT::T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd, typename DT::T* __restrict__ y,
                                                         int N, int Ks, int strips, int tiles, int relu) {
    constexpr int V = LnV<DT>::V;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int strip = blockIdx.x % strips, rest = blockIdx.x / strips, tile = rest % tiles, s = rest / tiles;
    const int n0 = strip * 64 * V;
    float m[V], r[V];
    ln_load_cols<V, VEC>(mean + (size_t)s * N, n0, lane, N, m);
    ln_load_cols<V, VEC>(rstd + (size_t)s * N, n0, lane, N, r);
    const int k1 = min(Ks, (tile + 1) * LN_A0_ROWS);
#pragma unroll 4
    for (int k = tile * LN_A0_ROWS + w; k < k1; k += 4) {
        const size_t f = (size_t)s * Ks + k;
        const float gk = g[f], bk = b[f];
        float v[V], o[V];
        ln_load_row<DT, VEC>(x + f * N, n0, lane, N, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float pre = fmaf((v[j] - m[j]) * r[j], gk, bk);
            o[j] = relu ? fmaxf(pre, 0.f) : pre;
        }
        ln_store_row<DT, VEC>(y + f * N, n0, lane, N, o);
    }
}

// grid as ln_stats_a0_kernel.  ws[(sp * S + s)][2][N]: the slice's sum_k xhat dy g and sum_k dy g;  part[strip][2][K]: row k's dy xhat and dy
// summed over the strip's columns (each row belongs to one slice and one wave: stored once).
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ln_bwd_sums_a0_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ x,
                                                             const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ ws, float* __restrict__ part, int N, int S,
                                                             int Ks, int strips, int split, int rps, int relu) {
    constexpr int V = LnV<DT>::V;
    __shared__ float lds[4][2][V][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int strip = blockIdx.x % strips, rest = blockIdx.x / strips, s = rest % S, sp = rest / S;
    const int n0 = strip * 64 * V;
    const size_t K = (size_t)S * Ks;
    float m[V], r[V], s1[V], s2[V];
    ln_load_cols<V, VEC>(mean + (size_t)s * N, n0, lane, N, m);
    ln_load_cols<V, VEC>(rstd + (size_t)s * N, n0, lane, N, r);
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.f;
    const int k1 = min(Ks, (sp + 1) * rps);
    for (int k = sp * rps + w; k < k1; k += 4) {
        const size_t f = (size_t)s * Ks + k;
        const float gk = g[f], bk = relu ? b[f] : 0.f;
        float xv[V], dv[V];
        ln_load_row<DT, VEC>(x + f * N, n0, lane, N, xv);
        ln_load_row<DT, VEC>(dy + f * N, n0, lane, N, dv);
        double rdg = 0.0;                                  // (fp64, rounded once below: see ln_dg_term)
        float rdb = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {                      // (columns outside: x = dy = mean = rstd = 0, so xhat = d = 0)
            const float xhat = (xv[j] - m[j]) * r[j];
            float d = dv[j];
            if (relu && !(fmaf(xhat, gk, bk) > 0.f)) d = 0.f;
            rdg = ln_dg_term(d, xv[j], m[j], r[j], rdg);
            rdb += d;
            const float dg_ = d * gk;
            s1[j] = fmaf(xhat, dg_, s1[j]);
            s2[j] += dg_;
        }
        rdg = wave_sum(rdg);
        rdb = wave_sum(rdb);
        if (lane == 0) {
            part[((size_t)strip * 2) * K + f] = (float)rdg;
            part[((size_t)strip * 2 + 1) * K + f] = rdb;
        }
    }
    float* out = ws + ((size_t)sp * S + s) * 2 * N;
    ln_join_waves<V, VEC>(lds, s1, s2, out, out + N, n0, N);
}

// one thread per (s, n): merged[0][s][n] = sum1, merged[1][s][n] = sum2, slices in ascending order
__global__ void __launch_bounds__(256) ln_sums_merge_a0_kernel(const float* __restrict__ ws, float* __restrict__ merged, int N, int S, int split) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, SN = (long long)S * N;
    if (i >= SN) return;
    const int s = (int)(i / N), n = (int)(i - (long long)s * N);
    float s1 = 0.f, s2 = 0.f;
    for (int sp = 0; sp < split; ++sp) {
        const float* p = ws + ((size_t)sp * S + s) * 2 * N + n;
        s1 += p[0];
        s2 += p[N];
    }
    merged[i] = s1;
    merged[SN + i] = s2;
}

// grid as ln_norm_a0_kernel
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ln_bwd_dx_a0_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ x,
                                                           const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ merged, typename DT::T* __restrict__ dx,
                                                           int N, int S, int Ks, int strips, int tiles, int relu) {
    constexpr int V = LnV<DT>::V;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int strip = blockIdx.x % strips, rest = blockIdx.x / strips, tile = rest % tiles, s = rest / tiles;
    const int n0 = strip * 64 * V;
    const float rK = 1.f / (float)Ks;
    float m[V], r[V], sum1[V], sum2[V];
    ln_load_cols<V, VEC>(mean + (size_t)s * N, n0, lane, N, m);
    ln_load_cols<V, VEC>(rstd + (size_t)s * N, n0, lane, N, r);
    ln_load_cols<V, VEC>(merged + (size_t)s * N, n0, lane, N, sum1);
    ln_load_cols<V, VEC>(merged + ((size_t)S + s) * N, n0, lane, N, sum2);
    const int k1 = min(Ks, (tile + 1) * LN_A0_ROWS);
#pragma unroll 2
    for (int k = tile * LN_A0_ROWS + w; k < k1; k += 4) {
        const size_t f = (size_t)s * Ks + k;
        const float gk = g[f], bk = relu ? b[f] : 0.f;
        float xv[V], dv[V], o[V];
        ln_load_row<DT, VEC>(x + f * N, n0, lane, N, xv);
        ln_load_row<DT, VEC>(dy + f * N, n0, lane, N, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xhat = (xv[j] - m[j]) * r[j];
            float d = dv[j];
            if (relu && !(fmaf(xhat, gk, bk) > 0.f)) d = 0.f;
            o[j] = (d * gk - fmaf(xhat, sum1[j], sum2[j]) * rK) * r[j];
        }
        ln_store_row<DT, VEC>(dx + f * N, n0, lane, N, o);
    }
}

}  // namespace bsmm
