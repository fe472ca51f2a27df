// bsmm_optim.hip -- C-ABI entry points of include/bsmm_optim.h: argument checks, then launches of the kernels in bsmm_optim_kernels.h.
// No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_host.h"
#include "bsmm_optim.h"
#include "bsmm_optim_kernels.h"

using namespace bsmm;

namespace {

// workgroups for `work` lane-steps: one step per lane up to the cap, strided beyond it
inline unsigned grid_for(size_t work, int cap) {
    const size_t g = (work + OPT_THREADS - 1) / OPT_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

// size / bsize of a flat (bsize 0) or block-sparse tensor, and its optional per-block arrays
int check_shape(size_t size, int bsize, const void* gate, const void* lr_select) {
    if (size == 0) return BSMM_ERR_ARG;
    if (bsize == 0) return (gate != nullptr || lr_select != nullptr) ? BSMM_ERR_ARG : BSMM_OK;
    if (!bsize_ok(bsize)) return BSMM_ERR_UNSUPPORTED;
    if (size % ((size_t)bsize * bsize) != 0) return BSMM_ERR_ARG;
    if (size / ((size_t)bsize * bsize) > 0x7fffffffu) return BSMM_ERR_UNSUPPORTED;
    return BSMM_OK;
}

template <class GT, class PT>
int launch_adam(const bsmm_adam_args* a, const AdamParams& p) {
    const int bb = a->bsize * a->bsize;
    const bool vec = aligned16(a->param) && aligned16(a->mean) && aligned16(a->var) && aligned16(a->grad) && aligned16(a->param16);
    const typename GT::T* grad = static_cast<const typename GT::T*>(a->grad);
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    if (vec)
        opt_adam_kernel<GT, PT, true><<<grid_for((a->size + 3) / 4, OPT_MAX_GRID), OPT_THREADS, 0, st>>>(a->param, a->mean, a->var, grad, a->param16, a->gate,
                                                                                                           a->lr_select, a->norm_scale, a->size, bb, p);
    else
        opt_adam_kernel<GT, PT, false><<<grid_for(a->size, OPT_MAX_GRID), OPT_THREADS, 0, st>>>(a->param, a->mean, a->var, grad, a->param16, a->gate,
                                                                                                  a->lr_select, a->norm_scale, a->size, bb, p);
    return (int)hipGetLastError();
}

template <class GT>
int adam_p16(const bsmm_adam_args* a, const AdamParams& p) {
    if (a->param16 == nullptr) return launch_adam<GT, NoP16>(a, p);
    if (a->param16_dtype == BSMM_F16) return launch_adam<GT, DTf16>(a, p);
    return launch_adam<GT, DTbf16>(a, p);
}

template <class ET>
int launch_ema(void* ema, const float* param, const float* gate, float decay, size_t size, int bsize, hipStream_t st) {
    typename ET::T* e = static_cast<typename ET::T*>(ema);
    const float rate = 1.f - decay;
    if (aligned16(ema) && aligned16(param))
        opt_ema_kernel<ET, true><<<grid_for((size + 3) / 4, OPT_MAX_GRID), OPT_THREADS, 0, st>>>(e, param, gate, size, bsize * bsize, rate);
    else
        opt_ema_kernel<ET, false><<<grid_for(size, OPT_MAX_GRID), OPT_THREADS, 0, st>>>(e, param, gate, size, bsize * bsize, rate);
    return (int)hipGetLastError();
}

template <class DT>
int launch_sum_squared(const void* x, float* slots, size_t size, float grad_scale, float saturate, int zero_infs, int zero_nans, hipStream_t st) {
    const typename DT::T* p = static_cast<const typename DT::T*>(x);
    constexpr int W = DT::is16 ? 8 : 4;
    if (aligned16(x))
        opt_sum_squared_kernel<DT, true><<<grid_for((size + W - 1) / W, OPT_SS_SLOTS), OPT_THREADS, 0, st>>>(p, slots, size, grad_scale, saturate, zero_infs, zero_nans);
    else
        opt_sum_squared_kernel<DT, false><<<grid_for(size, OPT_SS_SLOTS), OPT_THREADS, 0, st>>>(p, slots, size, grad_scale, saturate, zero_infs, zero_nans);
    return (int)hipGetLastError();
}

inline bool workspace_ok(const void* workspace, size_t bytes, int tensor_cnt) {
    return workspace != nullptr && aligned_to(workspace, 4) && bytes >= bsmm_sum_squared_workspace_bytes(tensor_cnt);
}

}  // namespace

extern "C" {

int bsmm_adam(const bsmm_adam_args* a) {
    if (a == nullptr || a->param == nullptr || a->mean == nullptr || a->var == nullptr || a->grad == nullptr) return BSMM_ERR_ARG;
    if (int rc = check_shape(a->size, a->bsize, a->gate, a->lr_select)) return rc;
    if (!dtype_ok(a->grad_dtype)) return BSMM_ERR_UNSUPPORTED;
    if (a->param16 != nullptr && a->param16_dtype != BSMM_F16 && a->param16_dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    AdamParams p;
    p.lr = a->lr;
    p.lr_new = a->lr_new;
    p.beta1 = a->beta1;
    p.beta2 = a->beta2;
    p.epsilon = a->epsilon;
    p.grad_scale = a->grad_scale;
    p.clip_sigma = a->clip_sigma;
    p.saturate = a->saturate;
    p.zero_infs = a->zero_infs != 0;
    p.zero_nans = a->zero_nans != 0;
    return with_dtype(a->grad_dtype, [&](auto dt) { return adam_p16<decltype(dt)>(a, p); });
}

int bsmm_ema(void* ema, const float* param, const float* gate, float decay, size_t size, int32_t bsize, int32_t ema_dtype, void* stream) {
    if (ema == nullptr || param == nullptr) return BSMM_ERR_ARG;
    if (int rc = check_shape(size, bsize, gate, nullptr)) return rc;
    if (!dtype_ok(ema_dtype)) return BSMM_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(ema_dtype, [&](auto dt) { return launch_ema<decltype(dt)>(ema, param, gate, decay, size, bsize, st); });
}

size_t bsmm_sum_squared_workspace_bytes(int32_t tensor_cnt) {
    return tensor_cnt <= 0 ? 0 : (size_t)tensor_cnt * OPT_SS_SLOTS * sizeof(float);
}

int bsmm_sum_squared(const void* x, size_t size, int32_t dtype, float grad_scale, float saturate, int32_t zero_infs, int32_t zero_nans,
                     int32_t tensor_idx, int32_t tensor_cnt, void* workspace, size_t workspace_bytes, void* stream) {
    if (x == nullptr || size == 0 || tensor_cnt <= 0 || tensor_idx < 0 || tensor_idx >= tensor_cnt) return BSMM_ERR_ARG;
    if (!dtype_ok(dtype)) return BSMM_ERR_UNSUPPORTED;
    if (!workspace_ok(workspace, workspace_bytes, tensor_cnt)) return BSMM_ERR_WORKSPACE;
    float* slots = static_cast<float*>(workspace) + (size_t)tensor_idx * OPT_SS_SLOTS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto dt) {
        return launch_sum_squared<decltype(dt)>(x, slots, size, grad_scale, saturate, zero_infs != 0, zero_nans != 0, st);
    });
}

int bsmm_clip_norm(const void* workspace, size_t workspace_bytes, int32_t tensor_cnt, float clip_norm, float* norm_out, float* scale_out,
                   void* stream) {
    if (norm_out == nullptr || scale_out == nullptr || tensor_cnt <= 0) return BSMM_ERR_ARG;
    if (tensor_cnt > (1 << 20)) return BSMM_ERR_UNSUPPORTED;
    if (!workspace_ok(workspace, workspace_bytes, tensor_cnt)) return BSMM_ERR_WORKSPACE;
    opt_clip_norm_kernel<0><<<1, OPT_THREADS, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const float*>(workspace), tensor_cnt * OPT_SS_SLOTS, clip_norm,
                                                                                  norm_out, scale_out);
    return (int)hipGetLastError();
}

}  // extern "C"
