// bsmm_ew_kernels.h -- kernels behind include/bsmm_ew.h: bias + activation, the dropout mask and its application, the fused epilogue and
// the gradients.  All of them are memory bound.  The unit of work is a GROUP of 8 consecutive elements of the contiguous tensor: 16 bytes of
// a 16-bit type (32 of fp32, two 16-byte accesses), one Philox call, one byte of the mask.
//
//   ew_fwd_kernel<VEC>      every forward form (bias_act, dropout_apply, the fused forward) as runtime switches of one body, so that the fused
//                           call and the composed sequence run the same fp32 operations.  A lane owns group c = i / 8 whatever K and N are:
//                           the mask byte of the group is made (or read) by the lane that owns the elements.  VEC: 16-byte accesses on whole
//                           groups and one row of b per group; else element accesses and a feature index that is carried along the group.
//                           Groups past the last element exist up to the end of the last mask word: they store the zero pad bytes.
//   ew_mask_kernel          the mask alone: a lane makes one 32-bit word (four generator calls) and stores it.
//   ew_bwd_a0_kernel<V>     x (K, N): work unit = (row k, chunk of EW_SPAN columns); the workgroup's lanes walk the chunk V elements at a time
//                           (V = 8: 16-byte accesses, V = 1: elements), sum dx in a register, meet in a wave reduction and LDS, and store one
//                           value: db[k] itself when a row is one chunk, else a partial.
//   ew_bwd_a1_kernel<V>     x (N, K): work unit = (partition p of the rows, tile of 256 column units of V columns).  A lane owns one column
//                           unit and every RL-th row of the partition (RL = 256 / column units when K is narrow), keeps V sums in registers,
//                           lanes with the same columns meet in LDS in ascending order, one row of partials per partition.
//   ew_sum_partials_kernel  db[k] = the partials in ascending order (sixteen slices per output, joined in LDS in a fixed order).
// Units beyond the grid (at most EW_MAX_GRID workgroups) are taken by a grid stride.  The 16-byte accesses and the wave sum are those of
// bsmm_vec.h.
#pragma once
#include "bsmm_vec.h"

// the multiply by the dropout scale and the add of the residual (and every sum) stay separate fp32 operations in this translation unit
#pragma clang fp contract(off)

namespace bsmm {

constexpr int EW_DROP_NONE = 0, EW_DROP_GENERATE = 1, EW_DROP_READ = 2;
constexpr int EW_SPAN = 8192;          // columns of a row one workgroup sweeps (axis 0 backward)
constexpr int EW_MAX_GRID = 2048;

// the keep bits of the 8 elements of generator call c (bit j = element 8 c + j)
__device__ __forceinline__ uint32_t ew_keep8(uint32_t c, uint64_t seed, uint64_t offset, uint32_t threshold) {
    uint32_t w[4];
    ew_philox(c, 0u, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m |= ((w[j] & 0xffffu) < threshold ? 1u : 0u) << (2 * j);
        m |= ((w[j] >> 16) < threshold ? 1u : 0u) << (2 * j + 1);
    }
    return m;
}

// the library's functions, not the hardware approximations: the fp32 results are held to the fp32 bars
__device__ __forceinline__ float ew_sigmoid(float z) { return 1.f / (1.f + expf(-1.702f * z)); }

__device__ __forceinline__ float ew_act(float z, int act) {
    if (act == 1) return fmaxf(z, 0.f);
    if (act == 2) return z * ew_sigmoid(z);
    return z;
}

// act 1: z is the pre-activation or the stored y (the same sign test).  act 2: s (1 - s) by subtraction -- exp(-1.702 z) squared overflows
// for z <= -27 and a product with it is 0 * inf; here z = -100 gives s = 0 and z = 100 gives 1 - s = 0.
__device__ __forceinline__ float ew_act_grad(float g, float z, int act) {
    if (act == 1) return z > 0.f ? g : 0.f;
    if (act == 2) {
        const float s = ew_sigmoid(z);
        return g * (s + 1.702f * z * s * (1.f - s));
    }
    return g;
}

// =====================================================================================================================================
// forward
// =====================================================================================================================================
// grid: min(ceil(groups / 256), EW_MAX_GRID).  groups = 4 * ceil(total / 32): the bytes of the mask.  b == nullptr: no bias.  res == nullptr:
// no residual.  drop: EW_DROP_*.  VEC: x, y, res 16-byte aligned, and with a bias a group never leaves its row (axis 0: N % 8 == 0; axis 1:
// K % 8 == 0 and b 16-byte aligned).
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) ew_fwd_kernel(const typename DT::T* __restrict__ x, const float* __restrict__ b,
                                                     const typename DT::T* __restrict__ res, const uint64_t* __restrict__ state, uint32_t* mask,
                                                     typename DT::T* __restrict__ y, int K, int N, int axis, int act, int drop, uint32_t threshold,
                                                     float scale, uint32_t total, uint32_t groups) {
    uint64_t seed = 0, offset = 0;
    if (drop == EW_DROP_GENERATE) {
        seed = state[0];
        offset = state[1];
    }
    uint8_t* mbytes = reinterpret_cast<uint8_t*>(mask);
    for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < groups; c += gridDim.x * 256u) {
        const uint32_t i0 = c * 8u;
        const int live = i0 >= total ? 0 : (total - i0 < 8u ? (int)(total - i0) : 8);
        uint32_t keep = 0xffu;
        if (drop == EW_DROP_GENERATE) {
            keep = ew_keep8(c, seed, offset, threshold) & ((1u << live) - 1u);
            mbytes[c] = (uint8_t)keep;
        }
        if (live == 0) continue;
        if (drop == EW_DROP_READ) keep = mbytes[c];
        const bool whole = VEC && live == 8;
        float v[8], bb[8], r[8], o[8];
        if (whole) {
            vec_load<DT, 8>(x + i0, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < live ? DT::to_f32(x[i0 + j]) : 0.f;
        }
        if (b != nullptr) {
            if constexpr (VEC) {                         // (a bias on the 16-byte path: every group is whole and lies in one row)
                if (axis == 0) {
                    const float bk = b[i0 / (uint32_t)N];
#pragma unroll
                    for (int j = 0; j < 8; ++j) bb[j] = bk;
                } else {
                    vec_load_f32<8>(b + i0 % (uint32_t)K, bb);
                }
            } else if (axis == 0) {
                uint32_t k = i0 / (uint32_t)N, pos = i0 - k * (uint32_t)N;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    bb[j] = j < live ? b[k] : 0.f;
                    if (++pos == (uint32_t)N) { pos = 0; ++k; }
                }
            } else {
                uint32_t k = i0 % (uint32_t)K;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    bb[j] = j < live ? b[k] : 0.f;
                    if (++k == (uint32_t)K) k = 0;
                }
            }
        }
        if (res != nullptr) {
            if (whole) {
                vec_load<DT, 8>(res + i0, r);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] = j < live ? DT::to_f32(res[i0 + j]) : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = ew_act(b != nullptr ? v[j] + bb[j] : v[j], act);
            if (drop != EW_DROP_NONE) t = ((keep >> j) & 1u) ? t * scale : 0.f;
            if (res != nullptr) t = t + r[j];
            o[j] = t;
        }
        if (whole) {
            vec_store<DT, 8>(y + i0, o);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < live) y[i0 + j] = DT::from_f32(o[j]);
        }
    }
}

// grid: min(ceil(words / 256), EW_MAX_GRID); a lane makes word wd = elements 32 wd .. 32 wd + 31, bits at or beyond total are 0
__global__ void __launch_bounds__(256) ew_mask_kernel(uint32_t* __restrict__ mask, const uint64_t* __restrict__ state, uint32_t threshold, uint32_t total,
                                                      uint32_t words) {
    const uint64_t seed = state[0], offset = state[1];
    for (uint32_t wd = blockIdx.x * 256u + threadIdx.x; wd < words; wd += gridDim.x * 256u) {
        uint32_t out = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) out |= ew_keep8(wd * 4u + q, seed, offset, threshold) << (8 * q);
        const uint32_t i0 = wd * 32u;
        if (total - i0 < 32u) out &= (1u << (total - i0)) - 1u;
        mask[wd] = out;
    }
}

// =====================================================================================================================================
// backward
// =====================================================================================================================================
// dx of V elements that share the bias values bb (V == 8) or bb[0] (V == 1); returns nothing, adds the fp32 values to acc[V]
template <class DT, int V>
__device__ __forceinline__ void ew_bwd_unit(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ xy, const uint32_t* __restrict__ mask,
                                            typename DT::T* __restrict__ dx, size_t i, const float* bb, int act, int from_y, float scale, float* acc) {
    float d[V], a[V], o[V];
    vec_load<DT, V>(dy + i, d);
    if (act != 0) vec_load<DT, V>(xy + i, a);
    uint32_t keep = 0xffu;
    if (mask != nullptr) keep = V == 8 ? (uint32_t)reinterpret_cast<const uint8_t*>(mask)[i >> 3] : (mask[i >> 5] >> (i & 31)) & 1u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float g = d[j];
        if (mask != nullptr) g = ((keep >> j) & 1u) ? g * scale : 0.f;
        const float z = act == 0 ? 0.f : (from_y ? a[j] : a[j] + bb[j]);
        o[j] = ew_act_grad(g, z, act);
        acc[j] += o[j];
    }
    if (dx != nullptr) vec_store<DT, V>(dx + i, o);
}

// grid: min(units, EW_MAX_GRID), units = K * chunks; unit u = (row k = u / chunks, chunk u % chunks) -> out[u]: db (chunks == 1) or the
// partials [K][chunks].  V == 8: N % 8 == 0 and dy, xy, dx 16-byte aligned.
template <class DT, int V>
__global__ void __launch_bounds__(256) ew_bwd_a0_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ xy,
                                                        const float* __restrict__ b, const uint32_t* __restrict__ mask, typename DT::T* __restrict__ dx,
                                                        float* __restrict__ out, int N, int chunks, int act, int from_y, float scale, uint32_t units) {
    __shared__ float red[4];
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t k = u / (uint32_t)chunks, ch = u - k * (uint32_t)chunks;
        const int n0 = (int)ch * EW_SPAN, n1 = N - n0 < EW_SPAN ? N : n0 + EW_SPAN;
        float bb[V];
        const float bk = b[k];
#pragma unroll
        for (int j = 0; j < V; ++j) bb[j] = bk;
        const size_t row = (size_t)k * (size_t)N;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        for (int n = n0 + (int)threadIdx.x * V; n < n1; n += 256 * V) ew_bwd_unit<DT, V>(dy, xy, mask, dx, row + n, bb, act, from_y, scale, acc);
        float s = acc[0];
#pragma unroll
        for (int j = 1; j < V; ++j) s += acc[j];
        s = wave_sum(s);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) out[u] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// grid: min(units, EW_MAX_GRID), units = P * tiles; unit u = (partition p = u / tiles of the rows, rows [p rpp, (p + 1) rpp); tile u % tiles of
// 256 column units).  KU = ceil(K / V) column units, CT = min(KU, 256) of them per tile, RL = 256 / CT lanes share a column unit and take
// every RL-th row.  part[p][K].  V == 8: K % 8 == 0 and dy, xy, dx, b 16-byte aligned.
template <class DT, int V>
__global__ void __launch_bounds__(256) ew_bwd_a1_kernel(const typename DT::T* __restrict__ dy, const typename DT::T* __restrict__ xy,
                                                        const float* __restrict__ b, const uint32_t* __restrict__ mask, typename DT::T* __restrict__ dx,
                                                        float* __restrict__ part, int K, int N, int KU, int CT, int RL, int tiles, int rpp, int act,
                                                        int from_y, float scale, uint32_t units) {
    __shared__ float lds[V][256];
    const int t = threadIdx.x, cl = t % CT, rl = t / CT;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int p = (int)(u / (uint32_t)tiles), tile = (int)(u - (uint32_t)p * (uint32_t)tiles);
        const int cu = tile * 256 + cl;
        const bool mine = rl < RL && cu < KU;
        const int k0 = cu * V;
        const long long r0 = (long long)p * rpp, r1 = r0 + rpp < N ? r0 + rpp : N;
        float bb[V], acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) bb[j] = acc[j] = 0.f;
        if (mine) {
            if constexpr (V == 8) vec_load_f32<8>(b + k0, bb);
            else bb[0] = b[k0];
#pragma unroll 2
            for (long long r = r0 + rl; r < r1; r += RL) ew_bwd_unit<DT, V>(dy, xy, mask, dx, (size_t)r * (size_t)K + k0, bb, act, from_y, scale, acc);
        }
        if (RL > 1) {                                    // (uniform over the workgroup)
            __syncthreads();
#pragma unroll
            for (int j = 0; j < V; ++j) lds[j][t] = acc[j];
            __syncthreads();
            if (rl == 0 && mine) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float s = 0.f;
                    for (int q = 0; q < RL; ++q) s += lds[j][q * CT + cl];
                    acc[j] = s;
                }
            }
        }
        if (rl == 0 && mine) {
#pragma unroll
            for (int j = 0; j < V; ++j) part[(size_t)p * K + k0 + j] = acc[j];
        }
    }
}

// db[k] = sum_p part[p * ps + k * ks], p ascending.  grid ceil(K / 16): 16 outputs x 16 slices of the partials (at K = 4096 and 512 partitions
// that is 256 workgroups of 32 loads per lane).
__global__ void __launch_bounds__(256) ew_sum_partials_kernel(const float* __restrict__ part, float* __restrict__ db, int K, int P, size_t ps, size_t ks) {
    __shared__ float red[16][16];
    const int kl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const long long k = (long long)blockIdx.x * 16 + kl;
    const bool live = k < K;
    const int q = (P + 15) / 16, p0 = sl * q, p1 = min(P, p0 + q);
    float sum = 0.f;
    if (live)
        for (int p = p0; p < p1; ++p) sum += part[(size_t)p * ps + (size_t)k * ks];
    red[sl][kl] = sum;
    __syncthreads();
    if (sl == 0 && live) {
        float total = red[0][kl];
#pragma unroll
        for (int s = 1; s < 16; ++s) total += red[s][kl];
        db[k] = total;
    }
}

}  // namespace bsmm
