// bsmm_ends_kernels.h -- kernels behind include/bsmm_ends.h: softmax cross-entropy and the embedding lookup with its sorted gradient.  All of
// them are memory bound.  A UNIT is V consecutive elements of a row that one lane moves with one access: V = 8 on the 16-byte path (16 bytes
// of a 16-bit type, two 16-byte accesses of fp32), V = 1 on the element path (vec_load / vec_store of bsmm_vec.h, the wave reductions too).
//
//   xent_rows_kernel<V, R, NT>   rows that stay in registers: a team of NT lanes (64: a wave, four rows per workgroup, shuffles only; 256 or
//                                1024: the workgroup, sums of the waves meet in LDS) holds R units per lane.  One read of x, one write of g.
//   xent_long_kernel<V>          rows beyond that: 1024 lanes keep a running (max, sum) over their strips, meet once, and a second sweep
//                                re-reads x and writes g.  A -inf logit adds 0 to the sum, also while the lane's maximum is still -inf.
//   xent_bwd_kernel<V>           dx = unscale(g) * dy[row] over the flat tensor.
//   embed_fwd_kernel<VEC>        y rows as copies of 16 bytes (or of one element).
//   embed_grad_chunks_kernel<V>  stage 1 of the gradient: a team of lanes sums one chunk of EMBED_CHUNK sorted positions of one column tile.
//   embed_grad_merge_kernel<V>   stage 2: per table row, zeros if no index names it, or the partials of a run that crossed chunk borders.
// x and g (and g and dx) may be the SAME pointer: none of them is declared __restrict__, a lane stores a unit only after it has read it, and a
// row is stored only after the whole row has been read (registers) or re-read unit by unit (long rows).
#pragma once
#include "bsmm_ends.h"
#include "bsmm_vec.h"

// every sum below is a chain of separate fp32 additions in a fixed order
#pragma clang fp contract(off)

namespace bsmm {

constexpr float ENDS_LOG2E = 1.44269504088896340736f;
constexpr int ENDS_MAX_GRID = BSMM_XENT_MAX_GRID;
constexpr int EMBED_CHUNK = BSMM_EMBED_CHUNK;
constexpr int EMBED_BATCH = 4;         // rows of dy a lane has in flight

// ---- reductions over a team of NT lanes; every lane gets the result.  NT = 64: shuffles only.  NT > 64: the waves' values meet in LDS and
// every lane adds them in ascending wave order.  `lds` holds NT / 64 floats and is free again when the call returns. ----
template <int NT>
__device__ __forceinline__ float ends_team_max(float v, float* lds) {
    v = wave_max(v);
    if constexpr (NT > 64) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) lds[wave] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v = fmaxf(v, lds[w]);
        __syncthreads();
    }
    return v;
}

template <int NT>
__device__ __forceinline__ float ends_team_sum(float v, float* lds) {
    v = wave_sum(v);
    if constexpr (NT > 64) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) lds[wave] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v += lds[w];
        __syncthreads();
    }
    return v;
}

// =====================================================================================================================================
// softmax cross-entropy
// =====================================================================================================================================
// (sum of the other terms) / s for the label's element.  A label on a -inf logit has probability 0: the others ARE s, and the share is 1
// exactly, which others * (1 / s) misses by an ulp for some s (a NaN s fails the comparison and stays NaN).
__device__ __forceinline__ float xent_others_share(float others, float inv, float s, float xl) {
    return (xl == -INFINITY && others == s) ? 1.f : others * inv;
}

// One row held in the registers of a team of NT lanes: lane t owns units t, t + NT, ... (R of them at most; K <= V * R * NT).
template <class DT, int V, int R, int NT>
__device__ __forceinline__ void xent_row_in_registers(const typename DT::T* xr, typename DT::T* gr, int K, int label, float* loss_row, int t,
                                                      float gscale, float* lds) {
    const int units = (K + V - 1) / V;
    if ((unsigned)label >= (unsigned)K) {                // an ignored row: the same for every lane of the team
        float z[V];
#pragma unroll
        for (int e = 0; e < V; ++e) z[e] = 0.f;
        for (int u = t; u < units; u += NT) vec_store<DT, V>(gr + (size_t)u * V, z);
        if (t == 0) *loss_row = 0.f;
        return;
    }
    // x[label] by a load of its own, issued before any store of the row (g may be x)
    const float xl = DT::to_f32(xr[label]);
    // the units this lane owns, as a count: the loops below test it by arithmetic (the sum) or by a branch (the store) instead of keeping the
    // R lane masks of `u < units` alive in scalar registers from the loads to the stores
    const int mine = (units - t + NT - 1) / NT;
    float v[R * V];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        // a unit past the row reads the row's last unit again: a valid address, the maximum is unchanged, and the sum below leaves it out
        vec_load<DT, V>(xr + (size_t)min(t + j * NT, units - 1) * V, &v[j * V]);
#pragma unroll
        for (int e = 0; e < V; ++e) m = fmaxf(m, v[j * V + e]);
    }
    m = ends_team_max<NT>(m, lds);
    // the sum WITHOUT the label's term: g[label] = p - 1 = -(sum of the others) / s, which keeps its bits when p is close to 1
    float others = 0.f;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const float own = (float)min(max(mine - j, 0), 1);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            v[j * V + e] = exp2f((v[j * V + e] - m) * ENDS_LOG2E) * own;
            others += ((t + j * NT) * V + e == label) ? 0.f : v[j * V + e];
        }
    }
    others = ends_team_sum<NT>(others, lds);
    const float s = others + exp2f((xl - m) * ENDS_LOG2E);
    if (t == 0) *loss_row = logf(s) + (m - xl);
    const float inv = 1.f / s;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (j < mine) {
            const int u = t + j * NT;
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (v[j * V + e] * inv) * gscale;
            vec_store<DT, V>(gr + (size_t)u * V, o);
        }
    }
    // the label's element, by the lane that has just stored its unit (stores of one lane to one address keep their order)
    if (t == (label / V) % NT) gr[label] = DT::from_f32(-xent_others_share(others, inv, s, xl) * gscale);
}

// grid: min(ceil(N / rows per workgroup), ENDS_MAX_GRID); block: NT = 64 -> 256 lanes (four rows at a time), else NT lanes (one row)
template <class DT, int V, int R, int NT>
__global__ void __launch_bounds__(NT == 64 ? 256 : NT) xent_rows_kernel(const typename DT::T* x, const int32_t* __restrict__ labels,
                                                                         float* __restrict__ loss, typename DT::T* g, int N, int K, float gscale) {
    __shared__ float lds[NT > 64 ? NT / 64 : 1];
    if constexpr (NT == 64) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int row = blockIdx.x * 4 + wave; row < N; row += gridDim.x * 4)
            xent_row_in_registers<DT, V, R, 64>(x + (size_t)row * K, g + (size_t)row * K, K, labels[row], loss + row, lane, gscale, lds);
    } else {
        for (int row = blockIdx.x; row < N; row += gridDim.x)
            xent_row_in_registers<DT, V, R, NT>(x + (size_t)row * K, g + (size_t)row * K, K, labels[row], loss + row, (int)threadIdx.x, gscale, lds);
    }
}

// grid: min(N, ENDS_MAX_GRID); block: 1024
template <class DT, int V>
__global__ void __launch_bounds__(1024) xent_long_kernel(const typename DT::T* x, const int32_t* __restrict__ labels, float* __restrict__ loss,
                                                         typename DT::T* g, int N, int K, float gscale) {
    constexpr int NT = 1024;
    __shared__ float lds[NT / 64];
    const int t = threadIdx.x, units = (K + V - 1) / V;
    for (int row = blockIdx.x; row < N; row += gridDim.x) {
        const typename DT::T* xr = x + (size_t)row * K;
        typename DT::T* gr = g + (size_t)row * K;
        const int label = labels[row];
        if ((unsigned)label >= (unsigned)K) {
            float z[V];
#pragma unroll
            for (int e = 0; e < V; ++e) z[e] = 0.f;
            for (int u = t; u < units; u += NT) vec_store<DT, V>(gr + (size_t)u * V, z);
            if (t == 0) loss[row] = 0.f;
            continue;
        }
        // the lane's running maximum and the sum of exp(x - that maximum) over its strips
        // x[label] by a load of its own, before the barriers that precede every store of the row (g may be x)
        const float xl = DT::to_f32(xr[label]);
        float m = -INFINITY, others = 0.f;               // others: the sum without the label's term (see xent_row_in_registers)
        for (int u = t; u < units; u += NT) {
            float v[V];
            vec_load<DT, V>(xr + (size_t)u * V, v);
            float mu = v[0];
#pragma unroll
            for (int e = 0; e < V; ++e) mu = fmaxf(mu, v[e]);
            if (mu > m) {
                others *= exp2f((m - mu) * ENDS_LOG2E);  // (the first strip: m = -inf, the factor is 0 and the sum is 0)
                m = mu;
            }
            if (m > -INFINITY) {
#pragma unroll
                for (int e = 0; e < V; ++e) others += (u * V + e == label) ? 0.f : exp2f((v[e] - m) * ENDS_LOG2E);
            } else {
                // the lane has met no finite logit yet: this unit holds -inf (a class of probability 0: it adds 0, where the difference
                // above would be -inf - -inf = NaN) or NaN, which still makes the sum NaN
#pragma unroll
                for (int e = 0; e < V; ++e) others += (u * V + e == label || v[e] == -INFINITY) ? 0.f : exp2f((v[e] - m) * ENDS_LOG2E);
            }
        }
        const float M = ends_team_max<NT>(m, lds);
        others = (m == -INFINITY) ? 0.f : others * exp2f((m - M) * ENDS_LOG2E);
        others = ends_team_sum<NT>(others, lds);
        const float s = others + exp2f((xl - M) * ENDS_LOG2E);
        if (t == 0) loss[row] = logf(s) + (M - xl);
        const float inv = 1.f / s;
        for (int u = t; u < units; u += NT) {
            float v[V];
            vec_load<DT, V>(xr + (size_t)u * V, v);
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = (exp2f((v[e] - M) * ENDS_LOG2E) * inv) * gscale;
            vec_store<DT, V>(gr + (size_t)u * V, v);
        }
        if (t == (label / V) % NT) gr[label] = DT::from_f32(-xent_others_share(others, inv, s, xl) * gscale);
    }
}

// grid: min(ceil(units / 256), ENDS_MAX_GRID); units = N * upr, upr = units of a row (K / 8 resp. K)
template <class DT, int V>
__global__ void __launch_bounds__(256) xent_bwd_kernel(const typename DT::T* g, const float* __restrict__ dy, typename DT::T* dx, uint32_t units,
                                                       uint32_t upr, float unscale) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const float d = dy[u / upr];
        float v[V];
        vec_load<DT, V>(g + (size_t)u * V, v);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = (v[e] * unscale) * d;
        vec_store<DT, V>(dx + (size_t)u * V, v);
    }
}

// =====================================================================================================================================
// embedding lookup
// =====================================================================================================================================
// U: the type a lane copies (uint4: 16 bytes; uint16_t / uint32_t: one element).  upr: U per row.  grid: min(ceil(nIdx * upr / 256), MAX)
template <class U>
__global__ void __launch_bounds__(256) embed_fwd_kernel(const U* __restrict__ w, const int32_t* __restrict__ idx, U* __restrict__ y, int C,
                                                        uint32_t upr, uint32_t units) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const uint32_t i = u / upr, c = u - i * upr;
        const int32_t k = idx[i];
        U val = U();
        if ((unsigned)k < (unsigned)C) val = w[(size_t)k * upr + c];
        y[u] = val;
    }
}

// the index at sorted position p; an `order` entry outside [0, nIdx) reads as an index that names no row
__device__ __forceinline__ int32_t embed_key(const int32_t* __restrict__ idx, const int32_t* __restrict__ order, int nIdx, int p, int* row) {
    const int32_t i = order[p];
    const bool ok = (unsigned)i < (unsigned)nIdx;
    *row = ok ? i : 0;
    return ok ? idx[i] : -1;
}

// Stage 1.  Work item = (chunk j of EMBED_CHUNK sorted positions, column tile of CT units); a team of CT lanes (64, 128 or 256: whole waves,
// so every branch below is wave-uniform) takes it, 256 / CT teams per workgroup, items beyond the grid by a stride.  ws: 2 rows of K floats
// per chunk: row 2 j for the run that began before the chunk, row 2 j + 1 for the run that goes on behind it.
template <class DT, int V>
__global__ void __launch_bounds__(256) embed_grad_chunks_kernel(const typename DT::T* __restrict__ dy, const int32_t* __restrict__ idx,
                                                                const int32_t* __restrict__ order, float* __restrict__ dw,
                                                                float* __restrict__ ws, int C, int K, int nIdx, int CT, int tiles,
                                                                uint32_t items) {
    const int teams = 256 / CT, team = threadIdx.x / CT, lane = threadIdx.x % CT;
    const int KU = (K + V - 1) / V;
    for (uint32_t item = blockIdx.x * (uint32_t)teams + team; item < items; item += gridDim.x * (uint32_t)teams) {
        const int j = (int)(item / (uint32_t)tiles), tile = (int)(item % (uint32_t)tiles);
        const int cu = tile * CT + lane;
        if (cu >= KU) continue;
        const size_t col = (size_t)cu * V;
        const int p0 = j * EMBED_CHUNK, p1 = min(p0 + EMBED_CHUNK, nIdx);
        int r;
        int32_t cur = embed_key(idx, order, nIdx, p0, &r);
        bool before = p0 > 0 && embed_key(idx, order, nIdx, p0 - 1, &r) == cur;     // the chunk's first run began in an earlier chunk
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        for (int p = p0; p < p1; p += EMBED_BATCH) {
            int32_t kk[EMBED_BATCH];
            float vv[EMBED_BATCH][V];
#pragma unroll
            for (int b = 0; b < EMBED_BATCH; ++b) {
                if (p + b < p1) {
                    kk[b] = embed_key(idx, order, nIdx, p + b, &r);
                    vec_load<DT, V>(dy + (size_t)r * K + col, vv[b]);
                }
            }
#pragma unroll
            for (int b = 0; b < EMBED_BATCH; ++b) {
                if (p + b < p1) {
                    if (kk[b] != cur) {                  // a run ends inside the chunk
                        if ((unsigned)cur < (unsigned)C) vec_store_f32<V>(before ? ws + (size_t)(2 * j) * K + col : dw + (size_t)cur * K + col, acc);
                        before = false;
                        cur = kk[b];
#pragma unroll
                        for (int e = 0; e < V; ++e) acc[e] = 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] += vv[b][e];
                }
            }
        }
        if ((unsigned)cur < (unsigned)C) {
            const bool behind = p1 < nIdx && embed_key(idx, order, nIdx, p1, &r) == cur;
            float* out = before ? ws + (size_t)(2 * j) * K + col : (behind ? ws + (size_t)(2 * j + 1) * K + col : dw + (size_t)cur * K + col);
            vec_store_f32<V>(out, acc);
        }
    }
}

// first sorted position whose index is >= key (nIdx if none)
__device__ __forceinline__ int embed_lower_bound(const int32_t* __restrict__ idx, const int32_t* __restrict__ order, int nIdx, int key) {
    int lo = 0, hi = nIdx, r;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (embed_key(idx, order, nIdx, mid, &r) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Stage 2.  Work item = (table row c, column tile); the same teams.  Positions [lo, hi) hold c: none -> zeros; inside one chunk -> stage 1
// stored the row; else the partials in chunk order: row 2 j + 1 of the chunk the run begins in, then row 2 j of every chunk it goes on in.
template <int V>
__global__ void __launch_bounds__(256) embed_grad_merge_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ order,
                                                               float* __restrict__ dw, const float* __restrict__ ws, int C, int K, int nIdx,
                                                               int CT, int tiles, uint32_t items) {
    const int teams = 256 / CT, team = threadIdx.x / CT, lane = threadIdx.x % CT;
    const int KU = (K + V - 1) / V;
    for (uint32_t item = blockIdx.x * (uint32_t)teams + team; item < items; item += gridDim.x * (uint32_t)teams) {
        const int c = (int)(item / (uint32_t)tiles), tile = (int)(item % (uint32_t)tiles);
        const int cu = tile * CT + lane;
        if (cu >= KU) continue;
        const size_t col = (size_t)cu * V;
        const int lo = embed_lower_bound(idx, order, nIdx, c);
        int hi = lo, r;
        if (lo < nIdx && embed_key(idx, order, nIdx, lo, &r) == c) hi = (c == INT32_MAX) ? nIdx : embed_lower_bound(idx, order, nIdx, c + 1);
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        if (hi > lo) {
            const int jl = lo / EMBED_CHUNK, jh = (hi - 1) / EMBED_CHUNK;
            if (jl == jh) continue;
            vec_load_f32<V>(ws + (size_t)(2 * jl + 1) * K + col, acc);
            for (int j = jl + 1; j <= jh; ++j) {
                float v[V];
                vec_load_f32<V>(ws + (size_t)(2 * j) * K + col, v);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += v[e];
            }
        }
        vec_store_f32<V>(dw + (size_t)c * K + col, acc);
    }
}

}  // namespace bsmm
