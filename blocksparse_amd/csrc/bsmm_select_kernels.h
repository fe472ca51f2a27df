// bsmm_select_kernels.h -- kernels behind include/bsmm_select.h: rectified top-k, top-k softmax and its gradient, sparse ReLU and the
// ReLU-rule gradient.  A row lives in the registers of ONE team of NW waves (NW = 1: a wave per row, four rows per workgroup, no LDS and no
// barrier; NW = 2, 4: the workgroup is the team) and is read from memory once.
//
// Geometry.  A lane holds EL elements as EL / V chunks of V consecutive ones (V = 8, 4 in fp32: one 16-byte access); wave w of the team
// holds the indices [w * 64 * EL, (w + 1) * 64 * EL):
//     index(w, lane, c, j) = w * 64 * EL + (c * 64 + lane) * V + j          register e = c * V + j
// so the index order is wave, chunk, lane, j.  The element form gives a lane the SAME elements by V single accesses: every reduction adds the
// same values in the same order on both forms, and they store the same bits.  Indices >= K are padding: key 0, value 0, never stored.
//
// Selection without a sort (a network over 4096 elements of wave64 lanes would be mostly shuffles):
//   1. sel_key     the score as an unsigned key whose order is the pinned one: -0 -> +0, NaN on top, masked elements and padding 0.
//   2. sel_kth     the k-th largest key by a search over its 32 bits from the top: T |= bit while count(key >= T | bit) >= k.  A count is
//                  EL ballots + popcounts per wave (scalar unit), summed across the team through a double-buffered LDS slot: one barrier
//                  per bit.  A step that counts exactly k ends the search: those k keys are the set.  At most 32 count steps whatever k
//                  and K; all 32 only when equal keys lie across the k-th position.
//   3. sel_pick    every key > T is selected, and of the keys == T the first k - count(key > T) in index order: the number of equal keys in
//                  front of an element is (earlier waves, through LDS) + (earlier chunks, popcounts) + (lower lanes of the chunk, mbcnt over
//                  the chunk's V ballots) + (lower j of the lane).
// Every register array is indexed by compile-time constants only (EL, V, NW are template parameters, the loops unroll): no scratch.
#pragma once
#include "bsmm_select.h"
#include "bsmm_vec.h"

// no contraction the source does not spell out
#pragma clang fp contract(off)

namespace bsmm {

constexpr float SEL_LOG2E = 1.4426950408889634f;
constexpr int SEL_EW_MAX_GRID = 2048;

template <class DT>
constexpr int SEL_V = DT::is16 ? 8 : 4;

// rows per workgroup and lanes per workgroup of a team size
template <int NW>
constexpr int SEL_ROWS = NW == 1 ? 4 : 1;
template <int NW>
constexpr int SEL_LANES = NW == 1 ? 256 : 64 * NW;

__device__ __forceinline__ uint32_t sel_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// bits of `m` below this lane
__device__ __forceinline__ uint32_t sel_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// value descending == key descending; integer tests only, so a NumPy model gives the same keys
__device__ __forceinline__ uint32_t sel_key(float v) {
    const uint32_t b = __float_as_uint(v), mag = b & 0x7fffffffu;
    if (mag > 0x7f800000u) return 0xffffffffu;           // NaN: above +inf (0xff800000)
    if (mag == 0u) return 0x80000000u;                   // -0 == +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // the smallest: -inf -> 0x007fffff, above the 0 of masked elements
}

// the score of a key (0: a masked element, never asked for)
__device__ __forceinline__ float sel_unkey(uint32_t t) {
    if (t == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((t & 0x80000000u) ? (t & 0x7fffffffu) : ~t);
}

// ---- this team's row: which row, which wave of the team; false: no row for this wave (NW == 1 only, where nothing waits on a barrier) ----
template <int NW>
__device__ __forceinline__ bool sel_row(uint32_t R, uint32_t& row, int& wave) {
    if constexpr (NW == 1) {
        wave = 0;
        row = blockIdx.x * 4u + (uint32_t)wave_id();
        return row < R;
    } else {
        wave = wave_id();
        row = blockIdx.x;
        return true;
    }
}

// A copy of a lane's bit mask that the compiler takes for a new value.  A test of one bit becomes a comparison into a pair of scalar
// registers; the compiler shares such a result between every place that asks for the same bit and keeps it live in between -- sixteen
// of them from the loads to the stores are more scalar registers than there are.  Each phase tests a copy of its own.
__device__ __forceinline__ uint32_t sel_fresh(uint32_t m) {
    asm volatile("" : "+v"(m));
    return m;
}

// bit e: element e of this lane lies inside the row.  
template <int EL, int V>
__device__ __forceinline__ uint32_t sel_real(uint32_t K, uint32_t first) {
    uint32_t real = 0;
#pragma unroll
    for (int e = 0; e < EL; ++e) real |= (first + (uint32_t)(e / V) * 64u * V + (uint32_t)(e % V) < K ? 1u : 0u) << e;
    return sel_fresh(real);
}

// ---- EL elements of a row at p (its first element) <-> v; elements outside the row (`real`) read as 0 and are not stored.  The element
// form reads without a branch: an index past the row is clamped to the row's last element (`last` = K - 1) and the value dropped ----
template <class DT, int EL, bool WIDE>
__device__ __forceinline__ void sel_load(const typename DT::T* p, uint32_t real, uint32_t first, uint32_t last, float (&v)[EL]) {
    constexpr int V = SEL_V<DT>;
    real = sel_fresh(real);
#pragma unroll
    for (int c = 0; c < EL / V; ++c) {
        const uint32_t i0 = first + (uint32_t)c * 64u * V;
        if constexpr (WIDE) {
            if (real >> (c * V) & 1u) {
                vec_load<DT, V>(p + i0, &v[c * V]);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) v[c * V + j] = 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float t = DT::to_f32(p[min(i0 + j, last)]);
                v[c * V + j] = (real >> (c * V + j) & 1u) ? t : 0.f;
            }
        }
    }
}

// the fp32 mask likewise; padding reads as 0 (masked)
template <int V, int EL, bool WIDE>
__device__ __forceinline__ void sel_load_f32(const float* p, uint32_t real, uint32_t first, uint32_t last, float (&v)[EL]) {
    real = sel_fresh(real);
#pragma unroll
    for (int c = 0; c < EL / V; ++c) {
        const uint32_t i0 = first + (uint32_t)c * 64u * V;
        if constexpr (WIDE) {
            if (real >> (c * V) & 1u) {
                vec_load_f32<V>(p + i0, &v[c * V]);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) v[c * V + j] = 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float t = p[min(i0 + j, last)];
                v[c * V + j] = (real >> (c * V + j) & 1u) ? t : 0.f;
            }
        }
    }
}

// The fp32 result as it stands, before the one rounding to the storage type: without it the compiler folds the last multiply in front of an
// fp16 element store into the conversion (one rounding instead of two) while the 16-byte form multiplies, then converts, and the two forms
// differ in the last bit of a few values (the same pin as lstm_pin of bsmm_lstm_kernels.h).
__device__ __forceinline__ float sel_pin(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

template <class DT, int EL, bool WIDE>
__device__ __forceinline__ void sel_store(typename DT::T* p, uint32_t real, uint32_t first, const float (&v)[EL]) {
    constexpr int V = SEL_V<DT>;
    real = sel_fresh(real);
#pragma unroll
    for (int c = 0; c < EL / V; ++c) {
        const uint32_t i0 = first + (uint32_t)c * 64u * V;
        float t[V];
#pragma unroll
        for (int j = 0; j < V; ++j) t[j] = sel_pin(v[c * V + j]);
        if constexpr (WIDE) {
            if (real >> (c * V) & 1u) vec_store<DT, V, true>(p + i0, t);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (real >> (c * V + j) & 1u) p[i0 + j] = DT::from_f32(t[j]);
        }
    }
}

// ---- over the team: the wave's butterfly, then the waves in ascending order through `lds` (NW floats, free again on return) ----
template <int NW>
__device__ __forceinline__ float team_sum(float v, float* lds, int wave) {
    v = wave_sum(v);
    if constexpr (NW > 1) {
        lds[wave] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += lds[w];
        __syncthreads();
    }
    return v;
}

// the smallest key over the team; lds: NW words, free again on return
template <int NW>
__device__ __forceinline__ uint32_t team_min_key(uint32_t v, uint32_t* lds, int wave) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, 64));
    if constexpr (NW > 1) {
        __syncthreads();
        lds[wave] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v = min(v, lds[w]);
        __syncthreads();
    }
    return v;
}

template <int NW>
__device__ __forceinline__ float team_max(float v, float* lds, int wave) {
    v = wave_max(v);
    if constexpr (NW > 1) {
        lds[wave] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) v = fmaxf(v, lds[w]);
        __syncthreads();
    }
    return v;
}

// ---- the threshold key T of the row: the k-th largest key, or -- when a step counts exactly k keys and the search stops there -- a lower
// bound of it with exactly k keys at or above.  Either way sel_pick(T) finds the set.  The search stops at the first bit in which the k-th
// and the (k + 1)-th key differ: it runs all 32 steps only on a tie across the k-th position.  cnt: 2 * NW words of LDS (NW > 1); every
// wave of the team sees the same count, so they leave the loop together ----
template <int EL, int NW>
__device__ __forceinline__ uint32_t sel_kth(const uint32_t (&key)[EL], uint32_t k, uint32_t* cnt, int wave) {
    uint32_t T = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        uint32_t n = 0;
#pragma unroll
        for (int e = 0; e < EL; ++e) n += (uint32_t)__popcll(__ballot(key[e] >= cand));
        if constexpr (NW > 1) {
            // the slot of the step before is still being read by a slower wave: two slots, one barrier per step
            uint32_t* slot = cnt + (bit & 1) * NW;
            slot[wave] = n;
            __syncthreads();
            n = slot[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) n += slot[w];
        }
        if (n >= k) T = cand;
        if (n == k) break;               // exactly k keys >= T: they are the set, whatever the bits below say (T is then a lower bound of the k-th key)
    }
    return T;
}

// ---- bit e of the result: element e of this lane is among the first k of the pinned order, T = sel_kth(...).  tot: 2 * NW words of LDS ----
template <int EL, int V, int NW>
__device__ __forceinline__ uint32_t sel_pick(const uint32_t (&key)[EL], uint32_t T, uint32_t k, uint32_t* tot, int wave) {
    uint32_t above = 0, front = 0;       // keys > T in the row; keys == T in the waves before this one
    if constexpr (NW > 1) __syncthreads();    // (the last read of sel_kth's slots: `tot` may be the same words)
#pragma unroll
    for (int e = 0; e < EL; ++e) above += (uint32_t)__popcll(__ballot(key[e] > T));
    if constexpr (NW > 1) {
        uint32_t equal = 0;
#pragma unroll
        for (int e = 0; e < EL; ++e) equal += (uint32_t)__popcll(__ballot(key[e] == T));
        tot[wave] = above;
        tot[NW + wave] = equal;
        __syncthreads();
        above = tot[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) above += tot[w];
#pragma unroll
        for (int w = 0; w < NW - 1; ++w) front += (w < wave) ? tot[NW + w] : 0u;
    }
    const uint32_t need = k - above;     // >= 1: T is the k-th key
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < EL / V; ++c) {
        uint32_t pos = front, chunk = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint64_t b = __ballot(key[c * V + j] == T);
            pos += sel_below(b);
            chunk += (uint32_t)__popcll(b);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool eq = key[c * V + j] == T;
            if (key[c * V + j] > T || (eq && pos < need)) bits |= 1u << (c * V + j);
            pos += eq ? 1u : 0u;
        }
        front += chunk;
    }
    return bits;
}

// ---- rectified top-k.  grid: ceil(R / SEL_ROWS<NW>), block: SEL_LANES<NW> ----
template <class DT, int EL, int NW, bool WIDE>
__global__ void __launch_bounds__(SEL_LANES<NW>) select_rect_kernel(const typename DT::T* __restrict__ x, typename DT::T* __restrict__ y, uint32_t R,
                                                                     uint32_t K, uint32_t k, int rebase) {
    constexpr int V = SEL_V<DT>;
    __shared__ uint32_t cnt[NW > 1 ? 2 * NW : 1];
    uint32_t row;
    int wave;
    if (!sel_row<NW>(R, row, wave)) return;
    const uint32_t first = (uint32_t)wave * 64u * EL + sel_lane() * V;
    const size_t at = (size_t)row * K;
    const uint32_t real = sel_real<EL, V>(K, first);
    float v[EL];
    uint32_t key[EL];
    sel_load<DT, EL, WIDE>(x + at, real, first, K - 1u, v);
#pragma unroll
    for (int e = 0; e < EL; ++e) key[e] = (sel_fresh(real) >> e & 1u) ? sel_key(v[e]) : 0u;
    const uint32_t T = sel_kth<EL, NW>(key, k, cnt, wave);
    const uint32_t bits = sel_pick<EL, V, NW>(key, T, k, cnt, wave);
    float base = 0.f;
    if (rebase) {                        // the k-th key: the smallest selected one (T itself unless the search stopped early)
        uint32_t lo = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < EL; ++e) lo = (sel_fresh(bits) >> e & 1u) ? min(lo, key[e]) : lo;
        base = fmaxf(sel_unkey(team_min_key<NW>(lo, cnt, wave)), 0.f);
    }
#pragma unroll
    for (int e = 0; e < EL; ++e) {
        const float t = (v[e] < base) ? base : v[e];
        v[e] = (sel_fresh(bits) >> e & 1u) ? __fsub_rn(t, base) : 0.f;
    }
    sel_store<DT, EL, WIDE>(y + at, real, first, v);
}

// ---- top-k softmax; k == K: the plain softmax.  mask: nullptr or mask_rows rows of K ----
template <class DT, int EL, int NW, bool WIDE>
__global__ void __launch_bounds__(SEL_LANES<NW>) select_softmax_kernel(const typename DT::T* __restrict__ x, const float* __restrict__ mask,
                                                                        typename DT::T* __restrict__ y, uint32_t R, uint32_t K, uint32_t k,
                                                                        uint32_t mask_rows, float scale) {
    constexpr int V = SEL_V<DT>;
    __shared__ uint32_t cnt[NW > 1 ? 2 * NW : 1];
    __shared__ float red[NW > 1 ? NW : 1];
    uint32_t row;
    int wave;
    if (!sel_row<NW>(R, row, wave)) return;
    const uint32_t first = (uint32_t)wave * 64u * EL + sel_lane() * V;
    const size_t at = (size_t)row * K;
    const uint32_t real = sel_real<EL, V>(K, first);
    float v[EL];
    uint32_t live = real;                // bit e: a real, unmasked element
    sel_load<DT, EL, WIDE>(x + at, real, first, K - 1u, v);
    if (mask != nullptr) {
        float m[EL];
        sel_load_f32<V, EL, WIDE>(mask + (size_t)(row % mask_rows) * K, real, first, K - 1u, m);
#pragma unroll
        for (int e = 0; e < EL; ++e) {
            v[e] = __fmul_rn(__fmul_rn(v[e], m[e]), scale);
            live &= ~((m[e] == 0.f ? 1u : 0u) << e);
        }
    } else {
#pragma unroll
        for (int e = 0; e < EL; ++e) {
            v[e] = __fmul_rn(v[e], scale);
        }
    }
    uint32_t bits = live;
    if (k < K) {
        uint32_t key[EL];
#pragma unroll
        for (int e = 0; e < EL; ++e) key[e] = (sel_fresh(live) >> e & 1u) ? sel_key(v[e]) : 0u;
        const uint32_t T = sel_kth<EL, NW>(key, k, cnt, wave);
        bits = live & sel_pick<EL, V, NW>(key, T, k, cnt, wave);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < EL; ++e) mx = (sel_fresh(live) >> e & 1u) ? fmaxf(mx, v[e]) : mx;
    mx = team_max<NW>(mx, red, wave);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EL; ++e) {
        v[e] = (sel_fresh(bits) >> e & 1u) ? exp2f(__fmul_rn(__fsub_rn(v[e], mx), SEL_LOG2E)) : 0.f;
        s += v[e];
    }
    s = team_sum<NW>(s, red, wave);
    const float inv = 1.f / s;
#pragma unroll
    for (int e = 0; e < EL; ++e) v[e] = (sel_fresh(bits) >> e & 1u) ? __fmul_rn(v[e], inv) : 0.f;
    sel_store<DT, EL, WIDE>(y + at, real, first, v);
}

// ---- dx = (dy - sum(dy * y)) * y * m * scale ----
template <class DT, int EL, int NW, bool WIDE>
__global__ void __launch_bounds__(SEL_LANES<NW>) select_softmax_grad_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ y,
                                                                             const float* __restrict__ mask, typename DT::T* __restrict__ dx,
                                                                             uint32_t R, uint32_t K, uint32_t mask_rows, float scale) {
    constexpr int V = SEL_V<DT>;
    __shared__ float red[NW > 1 ? NW : 1];
    uint32_t row;
    int wave;
    if (!sel_row<NW>(R, row, wave)) return;
    const uint32_t first = (uint32_t)wave * 64u * EL + sel_lane() * V;
    const size_t at = (size_t)row * K;
    const uint32_t real = sel_real<EL, V>(K, first);
    float g[EL], p[EL];
    sel_load<DT, EL, WIDE>(dy + at, real, first, K - 1u, g);
    sel_load<DT, EL, WIDE>(y + at, real, first, K - 1u, p);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EL; ++e) s = __fmaf_rn(g[e], p[e], s);
    s = team_sum<NW>(s, red, wave);
    if (mask != nullptr) {
        float m[EL];
        sel_load_f32<V, EL, WIDE>(mask + (size_t)(row % mask_rows) * K, real, first, K - 1u, m);
#pragma unroll
        for (int e = 0; e < EL; ++e) g[e] = __fmul_rn(__fmul_rn(__fmul_rn(__fsub_rn(g[e], s), p[e]), m[e]), scale);
    } else {
#pragma unroll
        for (int e = 0; e < EL; ++e) g[e] = __fmul_rn(__fmul_rn(__fsub_rn(g[e], s), p[e]), scale);
    }
    sel_store<DT, EL, WIDE>(dx + at, real, first, g);
}

// ---- y = max(x - (mean + alpha * sigma), 0), the population variance around the mean ----
template <class DT, int EL, int NW, bool WIDE>
__global__ void __launch_bounds__(SEL_LANES<NW>) select_sparse_relu_kernel(const typename DT::T* __restrict__ x, typename DT::T* __restrict__ y, uint32_t R,
                                                                            uint32_t K, float alpha) {
    constexpr int V = SEL_V<DT>;
    __shared__ float red[NW > 1 ? NW : 1];
    uint32_t row;
    int wave;
    if (!sel_row<NW>(R, row, wave)) return;
    const uint32_t first = (uint32_t)wave * 64u * EL + sel_lane() * V;
    const size_t at = (size_t)row * K;
    const uint32_t real = sel_real<EL, V>(K, first);
    float v[EL];
    sel_load<DT, EL, WIDE>(x + at, real, first, K - 1u, v);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EL; ++e) s += v[e];                  // (padding is 0)
    const float mean = __fdiv_rn(team_sum<NW>(s, red, wave), (float)K);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < EL; ++e) {
        const float d = (sel_fresh(real) >> e & 1u) ? __fsub_rn(v[e], mean) : 0.f;
        q = __fmaf_rn(d, d, q);
    }
    const float var = __fdiv_rn(team_sum<NW>(q, red, wave), (float)K);
    const float cut = __fadd_rn(mean, __fmul_rn(alpha, __fsqrt_rn(var)));
#pragma unroll
    for (int e = 0; e < EL; ++e) v[e] = fmaxf(__fsub_rn(v[e], cut), 0.f);
    sel_store<DT, EL, WIDE>(y + at, real, first, v);
}

// ---- dx = y > 0 ? dz : 0, element-wise.  grid: min(ceil(units / 256), SEL_EW_MAX_GRID); units of V elements, V > 1: 16-byte accesses ----
template <class DT, int V>
__global__ void __launch_bounds__(256) select_relu_grad_kernel(const typename DT::T* __restrict__ dz, const typename DT::T* __restrict__ y,
                                                                typename DT::T* __restrict__ dx, uint32_t units) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const size_t at = (size_t)u * V;
        float g[V], p[V];
        vec_load<DT, V>(dz + at, g);
        vec_load<DT, V>(y + at, p);
#pragma unroll
        for (int j = 0; j < V; ++j) g[j] = p[j] > 0.f ? g[j] : 0.f;
        vec_store<DT, V, true>(dx + at, g);
    }
}

}  // namespace bsmm
