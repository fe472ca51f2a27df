// bsmm_optim_kernels.h -- kernels behind include/bsmm_optim.h: the gated Adam step, the gated moving average and the two stages of the
// global-norm clip.  All of them stream: the Adam pass moves 26 - 28 bytes per element (28 - 30 with the 16-bit working copy), the only roof
// is the device copy rate.
//
//   vector path   every pointer 16-byte aligned: a lane owns 4 consecutive elements (16-byte loads and stores of the fp32 tensors, 8 bytes
//                 of a 16-bit one: vec_load / vec_store of bsmm_vec.h); a wave covers 256 consecutive elements, which lie inside one block
//                 for bsize >= 16 -- gate and lr select are then read once per wave (readfirstlane) and a skipped block is a uniform
//                 branch around every memory instruction.  For bsize 8 the gate varies per 16 lanes and the lanes of skipped blocks are masked off.  A flat tensor's
//                 size % 4 trailing elements go through the element form in the first lanes of the grid.
//   element path  anything else: one element per lane.
// Both paths call ONE arithmetic function per element, so the bits of a result do not depend on the path.  The grid is capped at
// OPT_MAX_GRID workgroups and strides the rest; stores are plain (the lines stay in L2 for the forward pass that follows).
//
//   sum of squares  per-lane serial sum over the lane's strided elements, a wave reduce, a fixed-order sum across the four waves through
//                   LDS, one plain vector store per workgroup into the slot of that workgroup; slots no workgroup owns are stored as 0.
#pragma once
#include "bsmm_vec.h"

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

// block of element i (bb = bsize^2, 0 for a flat tensor); uniform: the wave's elements lie inside one block
__device__ __forceinline__ int opt_block_of(size_t i, int bb, bool uniform) {
    const int b = (int)(i / (size_t)bb);
    return uniform ? __builtin_amdgcn_readfirstlane(b) : b;
}

// ---- Adam -------------------------------------------------------------------------------------------------------------------------
// GT: gradient type; PT: type of the 16-bit working copy or NoP16; VEC: the vector path.  The loop of workgroup w of the G that share one
// tensor: a row of a list (bsmm_optim_list_kernels.h); gs = grad_scale * norm_scale.
template <class GT, class PT, bool VEC>
__device__ __forceinline__ void opt_adam_row(float* __restrict__ param, float* __restrict__ mean, float* __restrict__ var,
                                             const typename GT::T* __restrict__ grad, void* __restrict__ param16, const float* __restrict__ gate,
                                             const float* __restrict__ lr_select, size_t size, int bb, const AdamParams& a, float gs, size_t w, size_t G) {
    const bool per_block = gate != nullptr || lr_select != nullptr;
    const size_t tid = w * OPT_THREADS + threadIdx.x, nthreads = G * OPT_THREADS;
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
            vec_load<GT, 4>(grad + i, g);
            vec_load<DTf32, 4>(mean + i, m);
            vec_load<DTf32, 4>(var + i, v);
            vec_load<DTf32, 4>(param + i, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_elem(g[j], m[j], v[j], p[j], a, gs, lr);
            vec_store<DTf32, 4>(mean + i, m);
            vec_store<DTf32, 4>(var + i, v);
            vec_store<DTf32, 4>(param + i, p);
            if constexpr (!std::is_same<PT, NoP16>::value) vec_store<PT, 4>(reinterpret_cast<typename PT::T*>(param16) + i, p);
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
        if constexpr (!std::is_same<PT, NoP16>::value) reinterpret_cast<typename PT::T*>(param16)[i] = PT::from_f32(p);
    }
}

// The per-tensor kernel keeps its own copy of the loop above (w = blockIdx.x, G = gridDim.x): with one call of opt_adam_row in its place
// the vector loop came out the same, the prologue and the element loop did not, and the headline step measured 0.56 us (3 %) slower, beyond
// the 0.47 us between the repeats of the copy (profiles/shared_helpers_ab.md).  An edit there is an edit here: tests/test_optimize_list_gpu.py
// holds the two to the same bits.
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
            vec_load<GT, 4>(grad + i, g);
            vec_load<DTf32, 4>(mean + i, m);
            vec_load<DTf32, 4>(var + i, v);
            vec_load<DTf32, 4>(param + i, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_elem(g[j], m[j], v[j], p[j], a, gs, lr);
            vec_store<DTf32, 4>(mean + i, m);
            vec_store<DTf32, 4>(var + i, v);
            vec_store<DTf32, 4>(param + i, p);
            if constexpr (!std::is_same<PT, NoP16>::value) vec_store<PT, 4>(static_cast<typename PT::T*>(param16) + i, p);
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

// workgroup w of the G that share the tensor: a launch of its own (blockIdx.x of gridDim.x) or a row of a list
template <class ET, bool VEC>
__device__ __forceinline__ void opt_ema_row(typename ET::T* __restrict__ ema, const float* __restrict__ param, const float* __restrict__ gate,
                                            size_t size, int bb, float rate, size_t w, size_t G) {
    const size_t tid = w * OPT_THREADS + threadIdx.x, nthreads = G * OPT_THREADS;
    size_t done = 0;
    if constexpr (VEC) {
        const size_t units = size >> 2;
        done = units << 2;
        const bool uniform = bb >= 256;
        for (size_t u = tid; u < units; u += nthreads) {
            const size_t i = u << 2;
            if (gate != nullptr && gate[opt_block_of(i, bb, uniform)] == 0.f) continue;
            float e[4], p[4];
            vec_load<ET, 4>(ema + i, e);
            vec_load<DTf32, 4>(param + i, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ema_elem(e[j], p[j], rate);
            vec_store<ET, 4>(ema + i, e);
        }
    }
    for (size_t i = done + tid; i < size; i += nthreads) {
        if (gate != nullptr && gate[opt_block_of(i, bb, false)] == 0.f) continue;
        ema[i] = ET::from_f32(ema_elem(ET::to_f32(ema[i]), param[i], rate));
    }
}

template <class ET, bool VEC>
__global__ void __launch_bounds__(OPT_THREADS) opt_ema_kernel(typename ET::T* __restrict__ ema, const float* __restrict__ param,
                                                              const float* __restrict__ gate, size_t size, int bb, float rate) {
    opt_ema_row<ET, VEC>(ema, param, gate, size, bb, rate, blockIdx.x, gridDim.x);
}

// ---- global norm, stage 1 ----------------------------------------------------------------------------------------------------------------
// this workgroup's sum of `acc` over its 256 lanes, in a fixed order; valid in thread 0
__device__ __forceinline__ float opt_group_sum(float acc, float* share) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) share[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((share[0] + share[1]) + share[2]) + share[3];
}

// VEC: a lane loads 16 bytes (4 fp32 or 8 16-bit elements) per step.  Workgroup w of G stores slot w -- G is min(OPT_SS_SLOTS, ceil(steps /
// 256)), a function of size and path -- and the slots from G on are stored as 0.  The order of the additions is pinned.
template <class DT, bool VEC>
__device__ __forceinline__ void opt_sum_squared_row(const typename DT::T* __restrict__ x, float* __restrict__ slots, size_t size, float grad_scale,
                                                    float saturate, int zero_infs, int zero_nans, size_t w, size_t G, float* share) {
    constexpr int W = VEC ? (DT::is16 ? 8 : 4) : 1;
    const size_t tid = w * OPT_THREADS + threadIdx.x, nthreads = G * OPT_THREADS;
    const size_t units = size / W;
    float acc = 0.f;
    for (size_t u = tid; u < units; u += nthreads) {
        float v[W];
        vec_load<DT, W>(x + u * W, v);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float s = opt_pre(v[j], zero_infs, zero_nans, saturate) * grad_scale;
            acc = fmaf(s, s, acc);
        }
    }
    if (W > 1 && tid < size - units * W) {                   // the size % W trailing elements, one each in the first lanes of the row's grid
        const float s = opt_pre(DT::to_f32(x[units * W + tid]), zero_infs, zero_nans, saturate) * grad_scale;
        acc = fmaf(s, s, acc);
    }
    const float total = opt_group_sum(acc, share);
    if (threadIdx.x == 0) slots[w] = total;
    for (size_t s = G + tid; s < (size_t)OPT_SS_SLOTS; s += nthreads) slots[s] = 0.f;
}

template <class DT, bool VEC>
__global__ void __launch_bounds__(OPT_THREADS) opt_sum_squared_kernel(const typename DT::T* __restrict__ x, float* __restrict__ slots, size_t size,
                                                                      float grad_scale, float saturate, int zero_infs, int zero_nans) {
    __shared__ float share[4];
    opt_sum_squared_row<DT, VEC>(x, slots, size, grad_scale, saturate, zero_infs, zero_nans, blockIdx.x, gridDim.x, share);
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
