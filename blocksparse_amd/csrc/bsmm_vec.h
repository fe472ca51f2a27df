// bsmm_vec.h -- device-side pieces the streaming kernel families share (sparsity, optim, norm, ew, ends, lstm): V consecutive elements of a
// tensor <-> V floats by the widest access the caller has checked the alignment for, and the reductions over the 64 lanes of a wave.
// A helper that adds something of its own (elements skipped at a row's end, an unaligned form) stays with its family and calls these for its
// 16-byte branch; sums across the waves of a workgroup stay with their kernels too: their order of additions is part of the pinned bits.
#pragma once
#include <type_traits>

#include "bsmm_common.h"

namespace bsmm {

// one dword of two 16-bit elements (the first in bits 0..15) <-> two floats
template <class DT>
__device__ __forceinline__ void vec_unpack2(uint32_t w, float* v) {
    v[0] = DT::to_f32((uint16_t)(w & 0xffffu));
    v[1] = DT::to_f32((uint16_t)(w >> 16));
}

// PACK2: bf16 by one conversion of the pair (bf16_pack2: the same rounding, other instructions); else two conversions, a shift and an or
template <class DT, bool PACK2>
__device__ __forceinline__ uint32_t vec_pack2(const float* v) {
    if constexpr (PACK2 && std::is_same<DT, DTbf16>::value) return bf16_pack2(v[0], v[1]);
    else return (uint32_t)DT::from_f32(v[0]) | ((uint32_t)DT::from_f32(v[1]) << 16);
}

// ---- the fp32 side streams (gain, bias, statistics, partials): V floats at p <-> V floats; V = 1, or a multiple of 4 by 16-byte accesses
// (p 16-byte aligned) ----
template <int V>
__device__ __forceinline__ void vec_load_f32(const float* p, float* v) {
    if constexpr (V == 1) {
        v[0] = p[0];
    } else {
        static_assert(V % 4 == 0, "fp32: 4 elements are 16 bytes");
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const float4 a = reinterpret_cast<const float4*>(p)[q];
            v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
        }
    }
}

template <int V>
__device__ __forceinline__ void vec_store_f32(float* p, const float* v) {
    if constexpr (V == 1) {
        p[0] = v[0];
    } else {
        static_assert(V % 4 == 0, "fp32: 4 elements are 16 bytes");
#pragma unroll
        for (int q = 0; q < V / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

// ---- V consecutive elements of a tensor at p <-> V floats.  V == 1: one element.  Otherwise p is aligned to the V elements: 16-byte
// accesses (fp32: V a multiple of 4; a 16-bit type: V == 8), or V == 4 of a 16-bit type by one 8-byte access.  The single accesses are
// written without a loop: a loop that runs once is unrolled late, and in some callers the registers then come out numbered otherwise. ----
template <class DT, int V>
__device__ __forceinline__ void vec_load(const typename DT::T* p, float* v) {
    if constexpr (V == 1) {
        v[0] = DT::to_f32(p[0]);
    } else if constexpr (!DT::is16 && V == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (!DT::is16) {
        vec_load_f32<V>(p, v);
    } else if constexpr (V == 4) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        vec_unpack2<DT>(q.x, v);
        vec_unpack2<DT>(q.y, v + 2);
    } else {
        static_assert(V == 8, "16-bit types: 8 elements are 16 bytes");
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) vec_unpack2<DT>(wd[j], v + 2 * j);
    }
}

// PACK2: see vec_pack2
template <class DT, int V, bool PACK2 = false>
__device__ __forceinline__ void vec_store(typename DT::T* p, const float* v) {
    if constexpr (V == 1) {
        p[0] = DT::from_f32(v[0]);
    } else if constexpr (!DT::is16 && V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (!DT::is16) {
        vec_store_f32<V>(p, v);
    } else if constexpr (V == 4) {
        *reinterpret_cast<uint2*>(p) = make_uint2(vec_pack2<DT, PACK2>(v), vec_pack2<DT, PACK2>(v + 2));
    } else {
        static_assert(V == 8, "16-bit types: 8 elements are 16 bytes");
        uint32_t wd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wd[j] = vec_pack2<DT, PACK2>(v + 2 * j);
        *reinterpret_cast<uint4*>(p) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
}

// ---- over the 64 lanes of a wave, shuffles only; every lane gets the same bits ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// ---- the library's one generator (the dropout masks of bsmm_ew_kernels.h, the stochastic rounding of bsmm_quant_kernels.h) ----
// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> w[0..3]
__device__ __forceinline__ void ew_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* w) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

}  // namespace bsmm
