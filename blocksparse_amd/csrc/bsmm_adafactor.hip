// bsmm_adafactor.hip -- C-ABI entry points of include/bsmm_adafactor.h: argument checks, the workspace layout, then the launches of the
// kernels in bsmm_adafactor_kernels.h.  No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_adafactor.h"
#include "bsmm_adafactor_kernels.h"
#include "bsmm_host.h"

using namespace bsmm;

namespace {

typedef unsigned __int128 u128;

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// Workspace, in floats.  Dense: [0, 2048) x^2 slots, [2048, 2304) rv slots, then (2-d form) colpart[nslabs][Kpad] and rowpart[rows][nchunks]
// -- sized for the element path's chunks of 256 columns, the 16-byte path uses fewer.  Block form: [0, 1024) x^2 slots, [1024, 2048) live
// counts (int32), [2304, 2304 + blocks) the blocks' m.  Every section starts on a multiple of 16 bytes from the base.
inline size_t kpad_of(size_t cols) { return ceil_div(cols, 4) * 4; }

u128 workspace_floats(size_t rows, size_t cols, int bsize) {
    if (rows == 0 || cols == 0) return 0;
    if (bsize != 0) {
        if (!bsize_ok(bsize) || cols != (size_t)bsize * bsize || rows > 0x7fffffffu) return 0;
        return (u128)ADF_HEAD + rows;
    }
    if (rows == 1) return ADF_HEAD;
    if (cols > SIZE_MAX - 4) return 0;
    return (u128)ADF_HEAD + (u128)ceil_div(rows, ADF_SLAB) * kpad_of(cols) + (u128)rows * ceil_div(cols, ADF_THREADS);
}

struct Call {
    const bsmm_adafactor_args* a;
    AdfParams p;
    float* ws;
    hipStream_t st;
    bool vec;
    int p16;
};

template <class GT, bool VEC>
int launch_2d(const Call& c) {
    const bsmm_adafactor_args* a = c.a;
    const typename GT::T* grad = static_cast<const typename GT::T*>(a->grad);
    const size_t C = a->rows, K = a->cols, Kpad = kpad_of(K);
    const size_t nslabs = ceil_div(C, ADF_SLAB), nchunks = ceil_div(K, (size_t)ADF_THREADS * (VEC ? 4 : 1)), ntiles = nslabs * nchunks;
    const unsigned gtile = capped(ntiles, ADF_X2_SLOTS);
    const int ncolwg = (int)capped(ceil_div(K, 64), ADF_COL_GRID), nrvwg = (int)capped(ceil_div(C, 4), ADF_RV_SLOTS);
    float *x2slots = c.ws, *rvslots = c.ws + ADF_X2_SLOTS, *colpart = c.ws + ADF_HEAD, *rowpart = colpart + nslabs * Kpad;
    const float inv_c = (float)(1.0 / (double)C), inv_k = (float)(1.0 / (double)K), inv_n = (float)(1.0 / ((double)C * (double)K));
    BSMM_LAUNCH((adf2_partial_kernel<GT, VEC>), gtile, ADF_THREADS, c.st, grad, a->norm_scale, colpart, rowpart, C, K, Kpad, nchunks, ntiles, c.p);
    BSMM_LAUNCH((adf2_finalize_kernel<0>), ncolwg + nrvwg, ADF_THREADS, c.st, a->cv, a->rv, a->norm_scale, colpart, rowpart, rvslots, C, K, Kpad,
                nslabs, nchunks, ncolwg, nrvwg, inv_c, inv_k, c.p);
    BSMM_LAUNCH((adf2_x2_kernel<GT, VEC>), gtile, ADF_THREADS, c.st, grad, a->norm_scale, a->cv, a->rv, rvslots, x2slots, C, K, nchunks, ntiles,
                nrvwg, inv_c, c.p);
    BSMM_LAUNCH((adf2_apply_kernel<GT, VEC>), gtile, ADF_THREADS, c.st, a->param, a->param16, c.p16, grad, a->norm_scale, a->cv, a->rv, rvslots,
                x2slots, C, K, nchunks, ntiles, nrvwg, (int)gtile, inv_c, inv_n, c.p);
    return BSMM_OK;
}

template <class GT, bool VEC>
int launch_1d(const Call& c) {
    const bsmm_adafactor_args* a = c.a;
    const typename GT::T* grad = static_cast<const typename GT::T*>(a->grad);
    const size_t K = a->cols;
    const unsigned grid = capped(ceil_div(K / (VEC ? 4 : 1), ADF_THREADS), ADF_X2_SLOTS);
    const float inv_n = (float)(1.0 / (double)K);
    BSMM_LAUNCH((adf1_moment_kernel<GT, VEC>), grid, ADF_THREADS, c.st, grad, a->norm_scale, a->cv, c.ws, K, c.p);
    BSMM_LAUNCH((adf1_apply_kernel<GT, VEC>), grid, ADF_THREADS, c.st, a->param, a->param16, c.p16, grad, a->norm_scale, a->cv, c.ws, K, (int)grid,
                inv_n, c.p);
    return BSMM_OK;
}

template <class GT, bool VEC>
int launch_block(const Call& c) {
    const bsmm_adafactor_args* a = c.a;
    const typename GT::T* grad = static_cast<const typename GT::T*>(a->grad);
    const size_t blocks = a->rows;
    const unsigned grid = capped(ceil_div(blocks, 4), ADF_BLK_SLOTS);
    float *x2slots = c.ws, *mblk = c.ws + ADF_HEAD;
    int* liveslots = reinterpret_cast<int*>(c.ws + ADF_BLK_SLOTS);
#define ADF_MOMENT(BS)                                                                                                                      \
    BSMM_LAUNCH((adfb_moment_kernel<GT, BS, VEC>), grid, ADF_THREADS, c.st, grad, a->norm_scale, a->gate, a->cv, a->rv, mblk, x2slots, liveslots, \
                blocks, c.p)
    switch (a->bsize) {
        case 8: ADF_MOMENT(8); break;
        case 16: ADF_MOMENT(16); break;
        case 32: ADF_MOMENT(32); break;
        default: ADF_MOMENT(64); break;
    }
#undef ADF_MOMENT
    BSMM_LAUNCH((adfb_apply_kernel<GT, VEC>), grid, ADF_THREADS, c.st, a->param, a->param16, c.p16, grad, a->norm_scale, a->gate, a->cv, a->rv, mblk,
                x2slots, liveslots, (int)grid, blocks, a->bsize, c.p);
    return BSMM_OK;
}

}  // namespace

extern "C" {

size_t bsmm_adafactor_workspace_bytes(size_t rows, size_t cols, int32_t bsize) {
    const u128 bytes = workspace_floats(rows, cols, bsize) * sizeof(float);
    return bytes > (u128)(SIZE_MAX / 2) ? 0 : (size_t)bytes;
}

int bsmm_adafactor(const bsmm_adafactor_args* a) {
    if (a == nullptr || a->param == nullptr || a->cv == nullptr || a->grad == nullptr) return BSMM_ERR_ARG;
    if (a->rows == 0 || a->cols == 0) return BSMM_ERR_ARG;
    if (a->bsize == 0) {
        if (a->gate != nullptr) return BSMM_ERR_ARG;
        if (a->rows > 1 && a->rv == nullptr) return BSMM_ERR_ARG;
    } else {
        if (!bsize_ok(a->bsize)) return BSMM_ERR_UNSUPPORTED;
        if (a->cols != (size_t)a->bsize * a->bsize || a->rv == nullptr) return BSMM_ERR_ARG;
        if (a->rows > 0x7fffffffu) return BSMM_ERR_UNSUPPORTED;
    }
    if (!dtype_ok(a->grad_dtype)) return BSMM_ERR_UNSUPPORTED;
    if (a->param16 != nullptr && a->param16_dtype != BSMM_F16 && a->param16_dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    if (!(a->clip_thresh > 0.f)) return BSMM_ERR_ARG;
    const size_t need = bsmm_adafactor_workspace_bytes(a->rows, a->cols, a->bsize);
    if (need == 0) return BSMM_ERR_UNSUPPORTED;
    if (a->workspace == nullptr || !aligned_to(a->workspace, 4) || a->workspace_bytes < need) return BSMM_ERR_WORKSPACE;
    Call c;
    c.a = a;
    c.p.lr = a->lr;
    c.p.decay = a->decay;
    c.p.omd = 1.f - a->decay;
    c.p.epsilon = a->epsilon;
    c.p.clip_thresh = a->clip_thresh;
    c.p.grad_scale = a->grad_scale;
    c.p.saturate = a->saturate;
    c.p.zero_infs = a->zero_infs != 0;
    c.p.zero_nans = a->zero_nans != 0;
    c.ws = static_cast<float*>(a->workspace);
    c.st = static_cast<hipStream_t>(a->stream);
    c.p16 = a->param16 != nullptr ? a->param16_dtype : 0;
    c.vec = a->cols % 4 == 0 && aligned16(a->param) && aligned16(a->cv) && aligned16(a->grad) && aligned16(a->param16) && aligned16(a->workspace);
    return with_dtype(a->grad_dtype, c.vec, [&](auto dt, auto wide) {
        using GT = decltype(dt);
        constexpr bool VEC = decltype(wide)::value;
        if (a->bsize != 0) return launch_block<GT, VEC>(c);
        return a->rows == 1 ? launch_1d<GT, VEC>(c) : launch_2d<GT, VEC>(c);
    });
}

}  // extern "C"
