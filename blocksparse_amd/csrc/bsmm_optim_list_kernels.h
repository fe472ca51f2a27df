// bsmm_optim_list_kernels.h -- kernels behind include/bsmm_optim_list.h: the Adam step, the moving average and stage 1 of the global norm
// over a table of tensors in one launch each, and the one-lane kernel that advances the device step state.
//
// The table (built on the host, bsmm_opt_list_build): OptRow[count], then three prefix arrays of count + 1 ints -- Adam, moving
// average, sum of squares -- where prefix[r + 1] - prefix[r] = G_r is the number of workgroups of row r in that stage.  G_r is what the
// per-tensor launch of bsmm_optim.hip would use as its grid (a row without an average has none in the moving-average stage; the Adam
// stage caps a row at OPT_LIST_ADAM_GRID, below).  A
// workgroup finds its row by a binary search over the stage's prefix array (uniform: scalar loads of a read-only array that stays in
// L2), takes w = blockIdx.x - prefix[r] and runs the per-tensor loop with (w, G_r) in place of (blockIdx.x, gridDim.x).  So
//   * the decomposition of every row -- which lane touches which element, in which order the sum of squares adds -- is that of the
//     per-tensor kernels in bsmm_optim_kernels.h: a lane-step of the vector path is 4 consecutive elements at u * 4 with
//     u = w * 256 + lane + k * G_r * 256, a wave's 256 elements start on a multiple of 256 and lie inside one block for bsize >= 16 (gate
//     and lr select once per wave), bsize 8 masks per lane; no row is cut into contiguous pieces, so there is no piece boundary to align;
//   * one large weight gets up to OPT_LIST_ADAM_GRID (Adam) / OPT_MAX_GRID (average) / OPT_SS_SLOTS (sum of squares) workgroups that
//     stride it, forty tiny tensors one workgroup each, in the same grid;
//   * gradient type, working-copy type and access path are properties of the row: one switch per workgroup, none per element.
// The arithmetic is adam_elem / ema_elem / opt_pre / opt_group_sum of bsmm_optim_kernels.h, not restated here.  Stores are plain.
#pragma once
#include "bsmm_optim_kernels.h"

namespace bsmm {

// access-path bits of OptRow::paths: the 16-byte path of a stage (every pointer the stage touches is 16-byte aligned)
constexpr int OPT_PATH_ADAM = 1, OPT_PATH_EMA = 2, OPT_PATH_SS = 4;
// dtype codes of include/bsmm.h (BSMM_F32 / BSMM_F16 / BSMM_BF16)
constexpr int OPT_DT_F32 = 0, OPT_DT_F16 = 1, OPT_DT_BF16 = 2;
// Workgroups per CU that one row may have in the Adam stage (the per-tensor launches cap at OPT_MAX_GRID = 8 per CU), so that a large
// row's workgroups are resident together and none runs as a tail behind the others.  A CU admits min(8, 512 / vgprs, 800 / (ceil16(sgprs)
// + 16)) workgroups of 256 threads; opt_adam_list_kernel, which holds all 18 type / path bodies, is built with 66 and 105: 6
// (tests/test_optimize_list_host.py checks the cap against the registers of the built code object).  Each element is independent, so
// this partition changes no result.  A build-time switch so that other values can be timed against the default.
#ifndef OPT_LIST_ADAM_WG_PER_CU
#define OPT_LIST_ADAM_WG_PER_CU 6
#endif
constexpr int OPT_LIST_ADAM_GRID = OPT_LIST_ADAM_WG_PER_CU * 256;

struct OptRow {                          // 96 bytes: bsmm_opt_tensor, then what the builder decided
    float* param;
    float* mean;
    float* var;
    const void* grad;
    void* param16;
    const float* gate;
    const float* lr_select;
    void* ema;
    unsigned long long size;
    int bsize, grad_dtype, param16_dtype, ema_dtype;
    int paths;                           // OPT_PATH_*
    int reserved;
};

struct OptState {                        // bsmm_opt_state
    int step;
    float lr_t, lr_new_t;
    int reserved;
};

// row of workgroup `wg`: the r with prefix[r] <= wg < prefix[r + 1] (rows without workgroups are passed over); uniform
__device__ __forceinline__ int opt_find_row(const int* __restrict__ prefix, int count, int wg) {
    int lo = 0, hi = count;              // invariant: prefix[lo] <= wg < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- Adam: opt_adam_row for workgroup w of the G of its row -------------------------------------------------------------------------------
template <class GT, class PT>
__device__ __forceinline__ void opt_adam_path(const OptRow& r, const AdamParams& a, float gs, size_t w, size_t G) {
    const typename GT::T* grad = reinterpret_cast<const typename GT::T*>(r.grad);
    const int bb = r.bsize * r.bsize;
    if (r.paths & OPT_PATH_ADAM)
        opt_adam_row<GT, PT, true>(r.param, r.mean, r.var, grad, r.param16, r.gate, r.lr_select, (size_t)r.size, bb, a, gs, w, G);
    else
        opt_adam_row<GT, PT, false>(r.param, r.mean, r.var, grad, r.param16, r.gate, r.lr_select, (size_t)r.size, bb, a, gs, w, G);
}

template <class GT>
__device__ __forceinline__ void opt_adam_p16(const OptRow& r, const AdamParams& a, float gs, size_t w, size_t G) {
    if (r.param16 == nullptr) opt_adam_path<GT, NoP16>(r, a, gs, w, G);
    else if (r.param16_dtype == OPT_DT_F16) opt_adam_path<GT, DTf16>(r, a, gs, w, G);
    else opt_adam_path<GT, DTbf16>(r, a, gs, w, G);
}

// a.lr / a.lr_new arrive unset: they are the state's, read here
__global__ void __launch_bounds__(OPT_THREADS) opt_adam_list_kernel(const OptRow* __restrict__ rows, const int* __restrict__ prefix, int count,
                                                                    const OptState* __restrict__ state, const float* __restrict__ norm_scale,
                                                                    AdamParams a) {
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;                                   // the clip's "skip this step": nothing is stored
    const float gs = a.grad_scale * ns;
    a.lr = state->lr_t;
    a.lr_new = state->lr_new_t;
    const int ri = opt_find_row(prefix, count, (int)blockIdx.x);
    const OptRow r = rows[ri];
    const size_t w = (size_t)((int)blockIdx.x - prefix[ri]), G = (size_t)(prefix[ri + 1] - prefix[ri]);
    switch (r.grad_dtype) {
        case OPT_DT_F32: opt_adam_p16<DTf32>(r, a, gs, w, G); break;
        case OPT_DT_F16: opt_adam_p16<DTf16>(r, a, gs, w, G); break;
        default: opt_adam_p16<DTbf16>(r, a, gs, w, G); break;
    }
}

// ---- moving average ------------------------------------------------------------------------------------------------------------------------
template <class ET>
__device__ __forceinline__ void opt_ema_path(const OptRow& r, float rate, size_t w, size_t G) {
    typename ET::T* ema = reinterpret_cast<typename ET::T*>(r.ema);
    const int bb = r.bsize * r.bsize;
    if (r.paths & OPT_PATH_EMA) opt_ema_row<ET, true>(ema, r.param, r.gate, (size_t)r.size, bb, rate, w, G);
    else opt_ema_row<ET, false>(ema, r.param, r.gate, (size_t)r.size, bb, rate, w, G);
}

__global__ void __launch_bounds__(OPT_THREADS) opt_ema_list_kernel(const OptRow* __restrict__ rows, const int* __restrict__ prefix, int count, float rate) {
    const int ri = opt_find_row(prefix, count, (int)blockIdx.x);
    const OptRow r = rows[ri];
    const size_t w = (size_t)((int)blockIdx.x - prefix[ri]), G = (size_t)(prefix[ri + 1] - prefix[ri]);
    switch (r.ema_dtype) {
        case OPT_DT_F32: opt_ema_path<DTf32>(r, rate, w, G); break;
        case OPT_DT_F16: opt_ema_path<DTf16>(r, rate, w, G); break;
        default: opt_ema_path<DTbf16>(r, rate, w, G); break;
    }
}

// ---- global norm, stage 1 ------------------------------------------------------------------------------------------------------------------
template <class DT>
__device__ __forceinline__ void opt_sum_squared_path(const OptRow& r, float* slots, float grad_scale, float saturate, int zero_infs, int zero_nans,
                                                     size_t w, size_t G, float* share) {
    const typename DT::T* x = reinterpret_cast<const typename DT::T*>(r.grad);
    if (r.paths & OPT_PATH_SS) opt_sum_squared_row<DT, true>(x, slots, (size_t)r.size, grad_scale, saturate, zero_infs, zero_nans, w, G, share);
    else opt_sum_squared_row<DT, false>(x, slots, (size_t)r.size, grad_scale, saturate, zero_infs, zero_nans, w, G, share);
}

__global__ void __launch_bounds__(OPT_THREADS) opt_sum_squared_list_kernel(const OptRow* __restrict__ rows, const int* __restrict__ prefix, int count,
                                                                           float* __restrict__ workspace, float grad_scale, float saturate,
                                                                           int zero_infs, int zero_nans) {
    __shared__ float share[4];
    const int ri = opt_find_row(prefix, count, (int)blockIdx.x);
    const OptRow r = rows[ri];
    const size_t w = (size_t)((int)blockIdx.x - prefix[ri]), G = (size_t)(prefix[ri + 1] - prefix[ri]);
    float* slots = workspace + (size_t)ri * OPT_SS_SLOTS;
    switch (r.grad_dtype) {
        case OPT_DT_F32: opt_sum_squared_path<DTf32>(r, slots, grad_scale, saturate, zero_infs, zero_nans, w, G, share); break;
        case OPT_DT_F16: opt_sum_squared_path<DTf16>(r, slots, grad_scale, saturate, zero_infs, zero_nans, w, G, share); break;
        default: opt_sum_squared_path<DTbf16>(r, slots, grad_scale, saturate, zero_infs, zero_nans, w, G, share); break;
    }
}

// ---- the step state: one active lane -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) opt_advance_kernel(OptState* __restrict__ state, const float* __restrict__ lr, const float* __restrict__ lr_new,
                                                         double beta1, double beta2, int zero_init) {
    if (threadIdx.x != 0) return;
    const int step = state->step + 1;
    double c = 1.0;
    if (!zero_init) c = sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step));
    const float lr_t = (float)((double)*lr * c);
    OptState s;
    s.step = step;
    s.lr_t = lr_t;
    s.lr_new_t = lr_new != nullptr ? (float)((double)*lr_new * c) : lr_t;
    s.reserved = 0;
    *state = s;
}

}  // namespace bsmm
