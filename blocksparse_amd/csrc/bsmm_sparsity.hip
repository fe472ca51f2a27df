// bsmm_sparsity.hip -- C-ABI entry points of include/bsmm_sparsity.h: argument checks, then launches of the kernels in
// bsmm_sparsity_kernels.h.  No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_host.h"
#include "bsmm_sparsity.h"
#include "bsmm_sparsity_kernels.h"

using namespace bsmm;

namespace {

// how bsmm_reduced_dw cuts the contraction: slices of at least 128 (a multiple of 64) terms, at most ~2048 waves in all.  `S_bound` (what
// the workspace is sized for) is non-decreasing in Kc; the launch uses S <= S_bound slices, none of them empty.
struct RdwCut {
    int tiles, S_bound, S, kchunk;
};
inline RdwCut rdw_cut(int CB, int KB, int Kc) {
    RdwCut c;
    c.tiles = ((CB + 31) / 32) * ((KB + 31) / 32);
    const int smax = c.tiles >= 2048 ? 1 : 2048 / c.tiles;
    const int want = (Kc + 127) / 128;
    c.S_bound = want < smax ? want : smax;
    c.kchunk = ((Kc + c.S_bound - 1) / c.S_bound + 63) / 64 * 64;
    c.S = (Kc + c.kchunk - 1) / c.kchunk;
    return c;
}

int check_blocks(const void* w, int blocks, int bsize, int dtype) {
    if (w == nullptr || blocks <= 0) return BSMM_ERR_ARG;
    if (!bsize_ok(bsize) || !dtype_ok(dtype)) return BSMM_ERR_UNSUPPORTED;
    return BSMM_OK;
}

template <class DT>
int launch_norm(const void* w, float* out, int blocks, int bsize, int norm_type, int as_gate, float threshold, hipStream_t st) {
    sp_block_norm_kernel<DT><<<(blocks + 3) / 4, 256, 0, st>>>(static_cast<const typename DT::T*>(w), out, blocks, bsize * bsize, norm_type, as_gate, threshold);
    return (int)hipGetLastError();
}

int norm_dispatch(const void* w, float* out, int blocks, int bsize, int dtype, int norm_type, int as_gate, float threshold, void* stream) {
    if (int rc = check_blocks(w, blocks, bsize, dtype)) return rc;
    if (out == nullptr) return BSMM_ERR_ARG;
    if (norm_type != BSMM_NORM_MAX && norm_type != BSMM_NORM_L2) return BSMM_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto dt) { return launch_norm<decltype(dt)>(w, out, blocks, bsize, norm_type, as_gate, threshold, st); });
}

template <class DT>
int launch_decay(void* w, const float* gate, float rate, float epsilon, int blocks, int bsize, hipStream_t st) {
    sp_block_l2_decay_kernel<DT><<<(blocks + 3) / 4, 256, 0, st>>>(static_cast<typename DT::T*>(w), gate, blocks, bsize * bsize, rate, epsilon);
    return (int)hipGetLastError();
}

template <class DT, class OT>
int launch_reduce(const PtrList8& xs, void* out, int pcount, int F, int N, int bsize, int axis, int norm_type, bool in_aligned, hipStream_t st) {
    uint16_t* o = static_cast<uint16_t*>(out);
    if (axis == 0) {
        const dim3 grid((N / 8 + 255) / 256, F / bsize, pcount);
        if (in_aligned && aligned16(out)) sp_reduce_a0_kernel<DT, OT, true><<<grid, 256, 0, st>>>(xs, o, N, bsize, pcount, norm_type);
        else sp_reduce_a0_kernel<DT, OT, false><<<grid, 256, 0, st>>>(xs, o, N, bsize, pcount, norm_type);
    } else {
        const dim3 grid((F + 511) / 512, (N + SP_A1_ROWS - 1) / SP_A1_ROWS, pcount);
        const int vec_out = (N % 8 == 0 && aligned16(out)) ? 1 : 0;
        if (in_aligned) sp_reduce_a1_kernel<DT, OT, true><<<grid, 256, 0, st>>>(xs, o, N, F, bsize, pcount, norm_type, vec_out);
        else sp_reduce_a1_kernel<DT, OT, false><<<grid, 256, 0, st>>>(xs, o, N, F, bsize, pcount, norm_type, vec_out);
    }
    return (int)hipGetLastError();
}

template <class DT>
int launch_rdw(const void* x_red, const void* y_red, float* dw, int CB, int KB, int Kc, float scale, int accumulate, void* workspace, hipStream_t st) {
    const RdwCut c = rdw_cut(CB, KB, Kc);
    const uint16_t* xr = static_cast<const uint16_t*>(x_red);
    const uint16_t* yr = static_cast<const uint16_t*>(y_red);
    float* ws = static_cast<float*>(workspace);
    if (Kc % 8 == 0 && aligned16(x_red) && aligned16(y_red)) sp_rdw_kernel<DT, true><<<c.tiles * c.S, 64, 0, st>>>(xr, yr, ws, CB, KB, Kc, c.S, c.kchunk);
    else sp_rdw_kernel<DT, false><<<c.tiles * c.S, 64, 0, st>>>(xr, yr, ws, CB, KB, Kc, c.S, c.kchunk);
    if (int rc = (int)hipGetLastError()) return rc;
    sp_rdw_sum_kernel<<<c.tiles * 4, 256, 0, st>>>(ws, dw, CB, KB, c.tiles, c.S, scale, accumulate);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int bsmm_block_norm(const void* w, float* norm_out, int32_t blocks, int32_t bsize, int32_t dtype, int32_t norm_type, void* stream) {
    return norm_dispatch(w, norm_out, blocks, bsize, dtype, norm_type, 0, 0.f, stream);
}

int bsmm_block_threshold_prune(const void* w, float* gate, float threshold, int32_t norm_type, int32_t blocks, int32_t bsize, int32_t dtype,
                               void* stream) {
    return norm_dispatch(w, gate, blocks, bsize, dtype, norm_type, 1, threshold, stream);
}

int bsmm_block_l2_decay(void* w, const float* gate, float rate, float epsilon, int32_t blocks, int32_t bsize, int32_t dtype, void* stream) {
    if (int rc = check_blocks(w, blocks, bsize, dtype)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto dt) { return launch_decay<decltype(dt)>(w, gate, rate, epsilon, blocks, bsize, st); });
}

int bsmm_block_prune(float* gate, const int32_t* idx, int32_t blocks, int32_t keep, void* stream) {
    if (gate == nullptr || idx == nullptr || blocks <= 0 || keep < 0 || keep > blocks) return BSMM_ERR_ARG;
    sp_block_prune_kernel<<<(blocks + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(gate, idx, blocks, keep);
    return (int)hipGetLastError();
}

int bsmm_feature_reduce(const void* const* xs, int32_t pcount, void* out, int32_t F, int32_t N, int32_t bsize, int32_t axis, int32_t dtype,
                        int32_t norm_type, void* stream) {
    if (xs == nullptr || out == nullptr || pcount < 1 || pcount > 8 || F <= 0 || N <= 0) return BSMM_ERR_ARG;
    if (!bsize_ok(bsize) || !dtype_ok(dtype) || (axis != 0 && axis != 1) || (axis == 0 && bsize == 64)) return BSMM_ERR_UNSUPPORTED;
    if (norm_type != BSMM_NORM_MAX && norm_type != BSMM_NORM_L2) return BSMM_ERR_UNSUPPORTED;
    if (F % bsize != 0 || (axis == 0 && N % 8 != 0)) return BSMM_ERR_ARG;
    if (F / bsize > 65535 || (N + SP_A1_ROWS - 1) / SP_A1_ROWS > 65535) return BSMM_ERR_UNSUPPORTED;      // (grid limits: F / bsize and N / 64 up to 65535)
    PtrList8 list;
    bool in_aligned = true;
    for (int p = 0; p < 8; ++p) {
        list.p[p] = p < pcount ? xs[p] : nullptr;
        if (p < pcount && xs[p] == nullptr) return BSMM_ERR_ARG;
        if (p < pcount && !aligned16(xs[p])) in_aligned = false;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_dtype(dtype, [&](auto dt) {                  // (fp32 activations reduce to bf16)
        typedef decltype(dt) DT;
        return launch_reduce<DT, std::conditional_t<DT::is16, DT, DTbf16>>(list, out, pcount, F, N, bsize, axis, norm_type, in_aligned, st);
    });
}

size_t bsmm_reduced_dw_workspace_bytes(int32_t CB, int32_t KB, int32_t contraction) {
    if (CB <= 0 || KB <= 0 || contraction <= 0) return 0;
    const RdwCut c = rdw_cut(CB, KB, contraction);
    return (size_t)c.tiles * c.S_bound * 1024 * sizeof(float);
}

int bsmm_reduced_dw(const void* x_red, const void* y_red, float* dw, int32_t CB, int32_t KB, int32_t contraction, float scale,
                    int32_t accumulate, int32_t red_dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (x_red == nullptr || y_red == nullptr || dw == nullptr || CB <= 0 || KB <= 0 || contraction <= 0) return BSMM_ERR_ARG;
    if (red_dtype != BSMM_F16 && red_dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    if ((long long)((CB + 31) / 32) * ((KB + 31) / 32) > (1 << 20)) return BSMM_ERR_UNSUPPORTED;
    if (workspace == nullptr || !aligned_to(workspace, 4) || workspace_bytes < bsmm_reduced_dw_workspace_bytes(CB, KB, contraction))
        return BSMM_ERR_WORKSPACE;
    if (scale == 0.f) return BSMM_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (red_dtype == BSMM_F16) return launch_rdw<DTf16>(x_red, y_red, dw, CB, KB, contraction, scale, accumulate, workspace, st);
    return launch_rdw<DTbf16>(x_red, y_red, dw, CB, KB, contraction, scale, accumulate, workspace, st);
}

}  // extern "C"
