// bsmm_optim_kernels.h -- kernels behind include/bsmm_optim.h: the gated Adam step, the gated moving average and the two stages of the
// global-norm clip.  All of them stream: the Adam pass moves 26 - 28 bytes per element (28 - 30 with the 16-bit working copy), the only roof
// is the device copy rate.
//
//   vector path   every pointer 16-byte aligned: a lane owns 4 consecutive elements (16-byte loads and stores of the fp32 tensors, 8 bytes
//                 of a 16-bit one); a wave covers 256 consecutive elements, which lie inside one block for bsize >= 16 -- gate and lr
//                 select are then read once per wave (readfirstlane) and a skipped block is a uniform branch around every memory
//                 instruction.  For bsize 8 the gate varies per 16 lanes and the lanes of skipped blocks are masked off.  A flat tensor's
//                 size % 4 trailing elements go through the element form in the first lanes of the grid.
//   element path  anything else: one element per lane.
// Both paths call ONE arithmetic function per element, so the bits of a result do not depend on the path.  The grid is capped at
// OPT_MAX_GRID workgroups and strides the rest; stores are plain (the lines stay in L2 for the forward pass that follows).
//
//   sum of squares  per-lane serial sum over the lane's strided elements, a wave reduce, a fixed-order sum across the four waves through
//                   LDS, one plain vector store per workgroup into the slot of that workgroup; slots no workgroup owns are stored as 0.
#pragma once
#include "bsmm_common.h"

namespace bsmm {

constexpr int OPT_THREADS = 256;
constexpr int OPT_MAX_GRID = 2048;       // 8 workgroups per CU on 256 CUs
constexpr int OPT_SS_SLOTS = 1024;       // partial sums (= workgroups at most) per tensor of bsmm_sum_squared

struct NoP16 {};                         // "no 16-bit working copy"

struct AdamParams {
    float lr, lr_new, beta1, beta2, epsilon, grad_scale, clip_sigma, saturate;
    int zero_infs, zero_nans;
};

// zero_infs / zero_nans / saturate of the reference (ew_zero_inf, ew_zero_nan, clamp)
__device__ __forceinline__ float opt_pre(float g, int zero_infs, int zero_nans, float saturate) {
    if (zero_infs && fabsf(g) == __builtin_inff()) g = 0.f;
    if (zero_nans && g != g) g = 0.f;
    if (saturate != 0.f) g = fmaxf(fminf(g, saturate), -saturate);
    return g;
}

// one element of the Adam step; gs = grad_scale * norm_scale
__device__ __forceinline__ void adam_elem(float g, float& m, float& v, float& p, const AdamParams& a, float gs, float lr) {
    g = opt_pre(g, a.zero_infs, a.zero_nans, a.saturate);
    g *= gs;
    v = a.beta2 * v + (1.f - a.beta2) * g * g;
    const float sigma = sqrtf(v);
    if (a.clip_sigma != 0.f) {
        const float clip = a.clip_sigma * sigma;
        g = fminf(fmaxf(g, -clip), clip);
    }
    m = a.beta1 * m + (1.f - a.beta1) * g;
    p -= lr * m / (sigma + a.epsilon);
}

// 4 consecutive elements of a tensor <-> 4 floats (16 bytes of fp32, 8 bytes of a 16-bit type)
template <class DT>
__device__ __forceinline__ void opt_load4(const typename DT::T* p, float v[4]) {
    if constexpr (!DT::is16) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = DT::to_f32((uint16_t)(q.x & 0xffffu)); v[1] = DT::to_f32((uint16_t)(q.x >> 16));
        v[2] = DT::to_f32((uint16_t)(q.y & 0xffffu)); v[3] = DT::to_f32((uint16_t)(q.y >> 16));
    }
}
template <class DT>
__device__ __forceinline__ void opt_store4(typename DT::T* p, const float v[4]) {
    if constexpr (!DT::is16) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)DT::from_f32(v[0]) | ((uint32_t)DT::from_f32(v[1]) << 16),
                                                  (uint32_t)DT::from_f32(v[2]) | ((uint32_t)DT::from_f32(v[3]) << 16));
    }
}

// block of element i (bb = bsize^2, 0 for a flat tensor); uniform: the wave's elements lie inside one block
__device__ __forceinline__ int opt_block_of(size_t i, int bb, bool uniform) {
    const int b = (int)(i / (size_t)bb);
    return uniform ? __builtin_amdgcn_readfirstlane(b) : b;
}

// ---- Adam -------------------------------------------------------------------------------------------------------------------------
// GT: gradient type; PT: type of the 16-bit working copy or NoP16; VEC: the vector path
// (opt_adam_row in bsmm_optim_list_kernels.h is this loop for workgroup w of G of one row of a list: an edit here is an edit there)
template <class GT, class PT, bool VEC>
__global__ void __launch_bounds__(OPT_THREADS) opt_adam_kernel(float* __restrict__ param, float* __restrict__ mean, float* __restrict__ var,
                                                               const typename GT::T* __restrict__ grad, void* __restrict__ param16,
                                                               const float* __restrict__ gate, const float* __restrict__ lr_select,
                                                               const float* __restrict__ norm_scale, size_t size, int bb, AdamParams a) {
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;                                   // the clip's "skip this step": nothing is stored
    const float gs = a.grad_scale * ns;
    const bool per_block = gate != nullptr || lr_select != nullptr;
    const size_t tid = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x, nthreads = (size_t)gridDim.x * OPT_THREADS;
    size_t done = 0;                                         // elements the vector loop covers
    if constexpr (VEC) {
        const size_t units = size >> 2;
        done = units << 2;
        const bool uniform = bb >= 256;
        for (size_t u = tid; u < units; u += nthreads) {
            const size_t i = u << 2;
            float lr = a.lr;
            if (per_block) {
                const int b = opt_block_of(i, bb, uniform);
                if (gate != nullptr && gate[b] == 0.f) continue;
                if (lr_select != nullptr && lr_select[b] != 0.f) lr = a.lr_new;
            }
            float g[4], m[4], v[4], p[4];
            opt_load4<GT>(grad + i, g);
            opt_load4<DTf32>(mean + i, m);
            opt_load4<DTf32>(var + i, v);
            opt_load4<DTf32>(param + i, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_elem(g[j], m[j], v[j], p[j], a, gs, lr);
            opt_store4<DTf32>(mean + i, m);
            opt_store4<DTf32>(var + i, v);
            opt_store4<DTf32>(param + i, p);
            if constexpr (!std::is_same<PT, NoP16>::value) opt_store4<PT>(static_cast<typename PT::T*>(param16) + i, p);
        }
    }
    // the element form: everything on the element path, the size % 4 trailing elements of a flat tensor on the vector path
    for (size_t i = done + tid; i < size; i += nthreads) {
        float lr = a.lr;
        if (per_block) {
            const int b = opt_block_of(i, bb, false);
            if (gate != nullptr && gate[b] == 0.f) continue;
            if (lr_select != nullptr && lr_select[b] != 0.f) lr = a.lr_new;
        }
        float m = mean[i], v = var[i], p = param[i];
        adam_elem(GT::to_f32(grad[i]), m, v, p, a, gs, lr);
        mean[i] = m;
        var[i] = v;
        param[i] = p;
        if constexpr (!std::is_same<PT, NoP16>::value) static_cast<typename PT::T*>(param16)[i] = PT::from_f32(p);
    }
}

// ---- moving average: e -= (1 - decay) (e - p) ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ema_elem(float e, float p, float rate) { return e - rate * (e - p); }

// (opt_ema_row in bsmm_optim_list_kernels.h is this loop for one row of a list: an edit here is an edit there)

template <class ET, bool VEC>
__global__ void __launch_bounds__(OPT_THREADS) opt_ema_kernel(typename ET::T* __restrict__ ema, const float* __restrict__ param,
                                                              const float* __restrict__ gate, size_t size, int bb, float rate) {
    const size_t tid = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x, nthreads = (size_t)gridDim.x * OPT_THREADS;
    size_t done = 0;
    if constexpr (VEC) {
        const size_t units = size >> 2;
        done = units << 2;
        const bool uniform = bb >= 256;
        for (size_t u = tid; u < units; u += nthreads) {
            const size_t i = u << 2;
            if (gate != nullptr && gate[opt_block_of(i, bb, uniform)] == 0.f) continue;
            float e[4], p[4];
            opt_load4<ET>(ema + i, e);
            opt_load4<DTf32>(param + i, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ema_elem(e[j], p[j], rate);
            opt_store4<ET>(ema + i, e);
        }
    }
    for (size_t i = done + tid; i < size; i += nthreads) {
        if (gate != nullptr && gate[opt_block_of(i, bb, false)] == 0.f) continue;
        ema[i] = ET::from_f32(ema_elem(ET::to_f32(ema[i]), param[i], rate));
    }
}

// ---- global norm, stage 1 ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float opt_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// this workgroup's sum of `acc` over its 256 lanes, in a fixed order; valid in thread 0
__device__ __forceinline__ float opt_group_sum(float acc, float* share) {
    acc = opt_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) share[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((share[0] + share[1]) + share[2]) + share[3];
}

// VEC: a lane loads 16 bytes (4 fp32 or 8 16-bit elements) per step.  The grid is min(OPT_SS_SLOTS, ceil(steps / 256)) workgroups -- a
// function of size and path -- and workgroup w stores slot w; the slots from gridDim.x on are stored as 0.
// (opt_sum_squared_row in bsmm_optim_list_kernels.h is this body for one row of a list and must add in this order: an edit here is an edit there)
template <class DT, bool VEC>
__global__ void __launch_bounds__(OPT_THREADS) opt_sum_squared_kernel(const typename DT::T* __restrict__ x, float* __restrict__ slots, size_t size,
                                                                      float grad_scale, float saturate, int zero_infs, int zero_nans) {
    __shared__ float share[4];
    constexpr int W = VEC ? (DT::is16 ? 8 : 4) : 1;
    const size_t tid = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x, nthreads = (size_t)gridDim.x * OPT_THREADS;
    const size_t units = size / W;
    float acc = 0.f;
    for (size_t u = tid; u < units; u += nthreads) {
        float v[W];
        if constexpr (!VEC) {
            v[0] = DT::to_f32(x[u]);
        } else if constexpr (!DT::is16) {
            opt_load4<DT>(x + u * 4, v);
        } else {
            const uint4 q = *reinterpret_cast<const uint4*>(x + u * 8);
            const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[2 * j] = DT::to_f32((uint16_t)(wd[j] & 0xffffu));
                v[2 * j + 1] = DT::to_f32((uint16_t)(wd[j] >> 16));
            }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float s = opt_pre(v[j], zero_infs, zero_nans, saturate) * grad_scale;
            acc = fmaf(s, s, acc);
        }
    }
    if (W > 1 && tid < size - units * W) {                   // the size % W trailing elements, one each in the first lanes of the grid
        const float s = opt_pre(DT::to_f32(x[units * W + tid]), zero_infs, zero_nans, saturate) * grad_scale;
        acc = fmaf(s, s, acc);
    }
    const float total = opt_group_sum(acc, share);
    if (threadIdx.x == 0) slots[blockIdx.x] = total;
    for (size_t s = (size_t)gridDim.x + tid; s < (size_t)OPT_SS_SLOTS; s += nthreads) slots[s] = 0.f;
}

// ---- global norm, stage 2: one workgroup (a template only so that two translation units may include this header) --------------------------
template <int UNUSED = 0>
__global__ void __launch_bounds__(OPT_THREADS) opt_clip_norm_kernel(const float* __restrict__ slots, int count, float clip_norm,
                                                                    float* __restrict__ norm_out, float* __restrict__ scale_out) {
    __shared__ float share[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < count; i += OPT_THREADS) acc += slots[i];
    const float total = opt_group_sum(acc, share);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(total);
        const bool finite = fabsf(norm) < __builtin_inff();  // false for Inf and NaN
        *scale_out = finite ? clip_norm / fmaxf(norm, clip_norm) : 0.f;
        *norm_out = norm;
    }
}

}  // namespace bsmm
