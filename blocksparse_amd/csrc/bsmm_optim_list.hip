// bsmm_optim_list.hip -- C-ABI entry points of include/bsmm_optim_list.h: the host-side table builder, argument checks, then launches of
// the kernels in bsmm_optim_list_kernels.h.  No allocation, no copies, no host sync, no environment, no state.
#include <cstdint>
#include <cstring>

#include "bsmm_host.h"
#include "bsmm_optim_list.h"
#include "bsmm_optim_list_kernels.h"

using namespace bsmm;

namespace {

constexpr int32_t LIST_MAX_ROWS = 1 << 20;               // the limit of bsmm_clip_norm

// the checks and the grid rule of bsmm_optim.hip (file-local there), restated so that a row is accepted here exactly when the per-tensor
// calls accept it and gets the workgroups their launches would use (the Adam stage: up to OPT_LIST_ADAM_GRID, see there)
inline unsigned grid_for(size_t work, int cap) {
    const size_t g = (work + OPT_THREADS - 1) / OPT_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

int check_shape(size_t size, int bsize, const void* gate, const void* lr_select) {
    if (size == 0) return BSMM_ERR_ARG;
    if (bsize == 0) return (gate != nullptr || lr_select != nullptr) ? BSMM_ERR_ARG : BSMM_OK;
    if (!bsize_ok(bsize)) return BSMM_ERR_UNSUPPORTED;
    if (size % ((size_t)bsize * bsize) != 0) return BSMM_ERR_ARG;
    if (size / ((size_t)bsize * bsize) > 0x7fffffffu) return BSMM_ERR_UNSUPPORTED;
    return BSMM_OK;
}

int check_row(const bsmm_opt_tensor& t) {
    if (t.param == nullptr || t.mean == nullptr || t.var == nullptr || t.grad == nullptr) return BSMM_ERR_ARG;
    if (int rc = check_shape(t.size, t.bsize, t.gate, t.lr_select)) return rc;
    if (!dtype_ok(t.grad_dtype)) return BSMM_ERR_UNSUPPORTED;
    if (t.param16 != nullptr && t.param16_dtype != BSMM_F16 && t.param16_dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    if (t.ema != nullptr && !dtype_ok(t.ema_dtype)) return BSMM_ERR_UNSUPPORTED;
    return BSMM_OK;
}

inline size_t rows_bytes(int32_t count) { return (size_t)count * sizeof(OptRow); }
inline size_t prefix_bytes(int32_t count) { return ((size_t)3 * ((size_t)count + 1) * sizeof(int) + 15) & ~(size_t)15; }

// a descriptor bsmm_opt_list_build could have written, and the table it belongs to
inline bool list_ok(const bsmm_opt_list* info, const void* table_dev) {
    return info != nullptr && table_dev != nullptr && aligned16(table_dev) && info->count > 0 && info->count <= LIST_MAX_ROWS &&
           info->table_bytes == bsmm_opt_list_bytes(info->count) && info->adam_grid >= info->count && info->sum_squared_grid >= info->count &&
           info->ema_grid >= 0;
}

inline const OptRow* table_rows(const void* table_dev) { return reinterpret_cast<const OptRow*>(table_dev); }
inline const int* table_prefix(const void* table_dev, int32_t count, int stage) {
    return reinterpret_cast<const int*>(reinterpret_cast<const char*>(table_dev) + rows_bytes(count)) + (size_t)stage * ((size_t)count + 1);
}

}  // namespace

extern "C" {

size_t bsmm_opt_list_bytes(int32_t count) {
    return (count <= 0 || count > LIST_MAX_ROWS) ? 0 : rows_bytes(count) + prefix_bytes(count);
}

int bsmm_opt_list_build(const bsmm_opt_tensor* rows, int32_t count, void* table_host, size_t table_bytes, bsmm_opt_list* info) {
    if (rows == nullptr || count <= 0 || info == nullptr) return BSMM_ERR_ARG;
    if (count > LIST_MAX_ROWS) return BSMM_ERR_UNSUPPORTED;
    for (int32_t i = 0; i < count; ++i)
        if (int rc = check_row(rows[i])) return rc;
    const size_t need = bsmm_opt_list_bytes(count);
    if (table_host == nullptr || table_bytes < need) return BSMM_ERR_WORKSPACE;
    std::memset(table_host, 0, need);
    char* base = reinterpret_cast<char*>(table_host);
    int* prefix = reinterpret_cast<int*>(base + rows_bytes(count));
    int* pre[3] = {prefix, prefix + ((size_t)count + 1), prefix + 2 * ((size_t)count + 1)};
    uint64_t total[3] = {0, 0, 0};
    for (int32_t i = 0; i < count; ++i) {
        const bsmm_opt_tensor& t = rows[i];
        OptRow r;
        std::memset(&r, 0, sizeof(r));
        r.param = t.param;
        r.mean = t.mean;
        r.var = t.var;
        r.grad = t.grad;
        r.param16 = t.param16;
        r.gate = t.gate;
        r.lr_select = t.lr_select;
        r.ema = t.ema;
        r.size = t.size;
        r.bsize = t.bsize;
        r.grad_dtype = t.grad_dtype;
        r.param16_dtype = t.param16_dtype;
        r.ema_dtype = t.ema_dtype;
        // the rules of launch_adam / launch_ema / launch_sum_squared (a null param16 counts as aligned there too)
        const bool adam_vec = aligned16(t.param) && aligned16(t.mean) && aligned16(t.var) && aligned16(t.grad) && aligned16(t.param16);
        const bool ema_vec = t.ema != nullptr && aligned16(t.ema) && aligned16(t.param);
        const bool ss_vec = aligned16(t.grad);
        r.paths = (adam_vec ? OPT_PATH_ADAM : 0) | (ema_vec ? OPT_PATH_EMA : 0) | (ss_vec ? OPT_PATH_SS : 0);
        const size_t ss_w = t.grad_dtype == BSMM_F32 ? 4 : 8;
        const unsigned g[3] = {grid_for(adam_vec ? (t.size + 3) / 4 : t.size, OPT_LIST_ADAM_GRID),
                               t.ema == nullptr ? 0u : grid_for(ema_vec ? (t.size + 3) / 4 : t.size, OPT_MAX_GRID),
                               grid_for(ss_vec ? (t.size + ss_w - 1) / ss_w : t.size, OPT_SS_SLOTS)};
        std::memcpy(base + (size_t)i * sizeof(OptRow), &r, sizeof(r));
        for (int s = 0; s < 3; ++s) {
            pre[s][i] = (int)total[s];
            total[s] += g[s];
        }
    }
    for (int s = 0; s < 3; ++s) {
        if (total[s] > 0x7fffffffu) return BSMM_ERR_UNSUPPORTED;
        pre[s][count] = (int)total[s];
    }
    info->table_bytes = need;
    info->count = count;
    info->adam_grid = (int32_t)total[0];
    info->ema_grid = (int32_t)total[1];
    info->sum_squared_grid = (int32_t)total[2];
    return BSMM_OK;
}

int bsmm_opt_advance(bsmm_opt_state* state, const float* lr, const float* lr_new, double beta1, double beta2, int32_t zero_init_variables,
                     void* stream) {
    if (state == nullptr || lr == nullptr || !aligned_to(state, 4)) return BSMM_ERR_ARG;
    opt_advance_kernel<<<1, 64, 0, reinterpret_cast<hipStream_t>(stream)>>>(reinterpret_cast<OptState*>(state), lr, lr_new, beta1, beta2,
                                                                             zero_init_variables != 0);
    return (int)hipGetLastError();
}

int bsmm_adam_list(const bsmm_opt_list* info, const void* table_dev, const bsmm_opt_state* state, const float* norm_scale,
                   const bsmm_adam_settings* s, void* stream) {
    if (!list_ok(info, table_dev) || state == nullptr || s == nullptr) return BSMM_ERR_ARG;
    AdamParams p;
    p.lr = 0.f;                                          // the kernel reads both rates from *state
    p.lr_new = 0.f;
    p.beta1 = s->beta1;
    p.beta2 = s->beta2;
    p.epsilon = s->epsilon;
    p.grad_scale = s->grad_scale;
    p.clip_sigma = s->clip_sigma;
    p.saturate = s->saturate;
    p.zero_infs = s->zero_infs != 0;
    p.zero_nans = s->zero_nans != 0;
    opt_adam_list_kernel<<<(unsigned)info->adam_grid, OPT_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        table_rows(table_dev), table_prefix(table_dev, info->count, 0), info->count, reinterpret_cast<const OptState*>(state), norm_scale, p);
    return (int)hipGetLastError();
}

int bsmm_ema_list(const bsmm_opt_list* info, const void* table_dev, float decay, void* stream) {
    if (!list_ok(info, table_dev)) return BSMM_ERR_ARG;
    if (info->ema_grid == 0) return BSMM_OK;             // no row has an average
    opt_ema_list_kernel<<<(unsigned)info->ema_grid, OPT_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        table_rows(table_dev), table_prefix(table_dev, info->count, 1), info->count, 1.f - decay);
    return (int)hipGetLastError();
}

int bsmm_sum_squared_list(const bsmm_opt_list* info, const void* table_dev, float grad_scale, float saturate, int32_t zero_infs,
                          int32_t zero_nans, void* workspace, size_t workspace_bytes, void* stream) {
    if (!list_ok(info, table_dev)) return BSMM_ERR_ARG;
    if (workspace == nullptr || !aligned_to(workspace, 4) || workspace_bytes < bsmm_sum_squared_workspace_bytes(info->count))
        return BSMM_ERR_WORKSPACE;
    opt_sum_squared_list_kernel<<<(unsigned)info->sum_squared_grid, OPT_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        table_rows(table_dev), table_prefix(table_dev, info->count, 2), info->count, reinterpret_cast<float*>(workspace), grad_scale, saturate,
        zero_infs != 0, zero_nans != 0);
    return (int)hipGetLastError();
}

}  // extern "C"
