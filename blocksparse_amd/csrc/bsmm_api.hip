// bsmm_api.hip -- the C-ABI surface (include/bsmm.h) for gfx950.  The kernel dispatch behind the three matmul entry points:
// bsmm_xprop_dispatch.h (fprop / bprop), bsmm_updat_dispatch.h (weight gradient), bsmm_dispatch.h (what they share).
#include "bsmm_l2norm.h"
#include "bsmm_sparse_proj.h"
#include "bsmm_xprop_dispatch.h"
#include "bsmm_updat_dispatch.h"

namespace {
template <class F>
int l2_by_types(int xd, int yd, int bsize, F&& f) {
    auto with_bs = [&](auto tx, auto ty) {
        switch (bsize) {
            case 8: return f(tx, ty, std::integral_constant<int, 8>{});
            case 16: return f(tx, ty, std::integral_constant<int, 16>{});
            case 32: return f(tx, ty, std::integral_constant<int, 32>{});
            default: return (int)BSMM_ERR_UNSUPPORTED;
        }
    };
    auto with_y = [&](auto tx) {
        if (yd == BSMM_F32) return with_bs(tx, DTf32{});
        if (yd == BSMM_F16) return with_bs(tx, DTf16{});
        if (yd == BSMM_BF16) return with_bs(tx, DTbf16{});
        return (int)BSMM_ERR_UNSUPPORTED;
    };
    if (xd == BSMM_F32) return with_y(DTf32{});
    if (xd == BSMM_F16) return with_y(DTf16{});
    if (xd == BSMM_BF16) return with_y(DTbf16{});
    return (int)BSMM_ERR_UNSUPPORTED;
}
}  // namespace

extern "C" {

int bsmm_fprop(const void* X, const void* W, void* Y, const bsmm_args* args) { return xprop(true, X, W, Y, args); }

int bsmm_bprop(const void* DY, const void* W, void* DX, const bsmm_args* args) { return xprop(false, DY, W, DX, args); }

int bsmm_updat(const void* const* X, const void* const* DY, void* DW, const bsmm_args* a) {
    int rc = check_common(a);
    if (rc) return rc;
    if (!X || !DY || (!DW && !(a->flags & BSMM_FLAG_DW_SUMS))) return BSMM_ERR_ARG;      // (DW is not written in sums mode)
    if (a->flags & FLAG_INTERNAL_Q64) return BSMM_ERR_ARG;                               // (the library's own bit)
    if (a->pcount < 1 || a->pcount > 8) return BSMM_ERR_ARG;
    if (a->bsize == 64 && !a->plan) return BSMM_ERR_UNSUPPORTED;
    if ((rc = check_plan(true, a))) return rc;
    if (a->bsize == 64) return DW ? updat64(X, DY, DW, a) : (int)BSMM_ERR_ARG;
    return updat(X, DY, DW, a);
}

size_t bsmm_prepared_bytes(int op, const bsmm_args* a) {
    if (!a || (op != BSMM_OP_FPROP && op != BSMM_OP_BPROP)) return 0;
    if (a->bsize == 64) return (a->axis == 1 && a->blocks > 0 && a->plan && a->plan_magic == B64PLAN_MAGIC) ? b64_w_bytes(a) : 0;   // the quadrant copy of W
    if (a->dtype == BSMM_F32 && a->bsize == 32 && a->plan && a->plan_magic == XCPLAN_MAGIC && a->plan_width == XS_G && a->blocks > 0) return xcols_w_bytes(a);
    return 0;
}

int bsmm_prepare_weights(int op, const void* W, void* prepared, const bsmm_args* a) {
    if (!a || !W || !prepared || (op != BSMM_OP_FPROP && op != BSMM_OP_BPROP)) return BSMM_ERR_ARG;
    if (bsmm_prepared_bytes(op, a) == 0) return BSMM_ERR_UNSUPPORTED;
    if (!aligned16(W) || !aligned16(prepared)) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    if (a->bsize == 64) {      // (one image per op: bprop numbers the quadrants the other way round, see bsmm_b64.h)
        const int swap = op == BSMM_OP_BPROP;
        if (elem_size(a->dtype) == 4) b64_split_kernel<4><<<a->blocks, 256, 0, st>>>(static_cast<const unsigned char*>(W), static_cast<unsigned char*>(prepared), a->blocks, swap);
        else                          b64_split_kernel<2><<<a->blocks, 256, 0, st>>>(static_cast<const unsigned char*>(W), static_cast<unsigned char*>(prepared), a->blocks, swap);
        return (int)hipGetLastError();
    }
    by_bool(op == BSMM_OP_FPROP, [&](auto fp) { split3_w_kernel<decltype(fp)::value><<<a->blocks, 256, 0, st>>>(static_cast<const float*>(W), static_cast<uint16_t*>(prepared), a->blocks); });
    return (int)hipGetLastError();
}

int bsmm_updat_finalize(const float* sums, void* DW, const float* gate, int32_t blocks, int32_t bsize, int32_t dtype, float alpha, float beta,
                        void* stream) {
    if (!sums || !DW || blocks <= 0) return BSMM_ERR_ARG;
    if (bsize != 8 && bsize != 16 && bsize != 32) return BSMM_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(sums) & 15) || (reinterpret_cast<uintptr_t>(DW) & 7)) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nel = (size_t)blocks * bsize * bsize;
    const unsigned grid = (unsigned)((nel / 4 + 255) / 256);
    switch (dtype) {
        case BSMM_F16:  updat_finalize_gated_kernel<DTf16><<<grid, 256, 0, st>>>(sums, static_cast<uint16_t*>(DW), nel, bsize * bsize, alpha, beta, gate); break;
        case BSMM_BF16: updat_finalize_gated_kernel<DTbf16><<<grid, 256, 0, st>>>(sums, static_cast<uint16_t*>(DW), nel, bsize * bsize, alpha, beta, gate); break;
        case BSMM_F32:  updat_finalize_gated_kernel<DTf32><<<grid, 256, 0, st>>>(sums, static_cast<float*>(DW), nel, bsize * bsize, alpha, beta, gate); break;
        default: return BSMM_ERR_UNSUPPORTED;
    }
    return (int)hipGetLastError();
}

int bsmm_l2_normalize(void* y, float* sum_sqr, const void* x, const float* gain, const int32_t* l2_lut, int32_t cols, int32_t bsize,
                      int32_t x_dtype, int32_t y_dtype, float epsilon, void* stream) {
    if (!y || !sum_sqr || !x || !l2_lut || cols <= 0) return BSMM_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(l2_lut) & 15) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return l2_by_types(x_dtype, y_dtype, bsize, [&](auto tx, auto ty, auto bs) {
        typedef decltype(tx) TX;
        typedef decltype(ty) TY;
        l2_normalize_kernel<TX, TY, decltype(bs)::value><<<cols, 256, 0, st>>>(static_cast<typename TY::T*>(y), sum_sqr, static_cast<const typename TX::T*>(x),
                                                                               gain, l2_lut, epsilon);
        return (int)hipGetLastError();
    });
}

int bsmm_l2_normalize_grad(void* dx, float* dgain, const void* dy, const void* x, const float* gain, const float* sum_sqr, const int32_t* l2_lut,
                           int32_t cols, int32_t bsize, int32_t x_dtype, int32_t y_dtype, float epsilon, void* stream) {
    if (!dx || !dy || !x || !sum_sqr || !l2_lut || cols <= 0) return BSMM_ERR_ARG;
    if (gain && !dgain) return BSMM_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(l2_lut) & 15) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return l2_by_types(x_dtype, y_dtype, bsize, [&](auto tx, auto ty, auto bs) {
        typedef decltype(tx) TX;
        typedef decltype(ty) TY;
        l2_normalize_grad_kernel<TX, TY, decltype(bs)::value><<<cols, 256, 0, st>>>(static_cast<typename TX::T*>(dx), dgain, static_cast<const typename TY::T*>(dy),
                                                                                    static_cast<const typename TX::T*>(x), gain, sum_sqr, l2_lut, epsilon);
        return (int)hipGetLastError();
    });
}

int bsmm_sparse_op(void* z, const void* x, const void* y, const int32_t* lut, int32_t op, int32_t K, int32_t rows_z, int32_t N, int32_t dtype,
                   void* stream) {
    if (!z || !x || !lut || K <= 0 || N <= 0 || rows_z <= 0) return BSMM_ERR_ARG;
    if ((op == SP_ADD || op == SP_MUL) && !y) return BSMM_ERR_ARG;
    if (op < SP_GAT || op > SP_MUL) return BSMM_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype != BSMM_F32 && dtype != BSMM_F16 && dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    const size_t esz = elem_size(dtype);
    if (op == SP_ADD && z != x) {                        // the unmapped rows pass through
        hipError_t e = hipMemcpyAsync(z, x, (size_t)rows_z * N * esz, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid(K, std::min((N + 255) / 256, 64));
    auto go = [&](auto t) {
        typedef decltype(t) DT;
        typedef typename DT::T T;
        switch (op) {
            case SP_GAT: sparse_proj_kernel<DT, SP_GAT><<<grid, 256, 0, st>>>(static_cast<T*>(z), static_cast<const T*>(x), nullptr, lut, K, N); break;
            case SP_SCT: sparse_proj_kernel<DT, SP_SCT><<<grid, 256, 0, st>>>(static_cast<T*>(z), static_cast<const T*>(x), nullptr, lut, K, N); break;
            case SP_ADD: sparse_proj_kernel<DT, SP_ADD><<<grid, 256, 0, st>>>(static_cast<T*>(z), static_cast<const T*>(z), static_cast<const T*>(y), lut, K, N); break;
            default:     sparse_proj_kernel<DT, SP_MUL><<<grid, 256, 0, st>>>(static_cast<T*>(z), static_cast<const T*>(x), static_cast<const T*>(y), lut, K, N); break;
        }
        return (int)hipGetLastError();
    };
    if (dtype == BSMM_F32) return go(DTf32{});
    if (dtype == BSMM_F16) return go(DTf16{});
    return go(DTbf16{});
}

int bsmm_sparse_mul_grad(void* dx, void* dy, const void* dz, const void* x, const void* y, const int32_t* lut, int32_t K, int32_t rows_x, int32_t N,
                         int32_t dtype, void* stream) {
    if (!dx || !dy || !dz || !x || !y || !lut || K <= 0 || N <= 0 || rows_x <= 0) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype != BSMM_F32 && dtype != BSMM_F16 && dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    const size_t esz = elem_size(dtype);
    if (dx != dz) {
        hipError_t e = hipMemcpyAsync(dx, dz, (size_t)rows_x * N * esz, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid(K, std::min((N + 255) / 256, 64));
    auto go = [&](auto t) {
        typedef decltype(t) DT;
        typedef typename DT::T T;
        // reads dz through dx (identical after the copy / when aliased): every mapped element is read before it is overwritten by the same thread
        sparse_mul_grad_kernel<DT><<<grid, 256, 0, st>>>(static_cast<T*>(dx), static_cast<T*>(dy), static_cast<const T*>(dx), static_cast<const T*>(x),
                                                         static_cast<const T*>(y), lut, K, N);
        return (int)hipGetLastError();
    };
    if (dtype == BSMM_F32) return go(DTf32{});
    if (dtype == BSMM_F16) return go(DTf16{});
    return go(DTbf16{});
}

int bsmm_gate_grad(void* dw_out, float* dg, const void* dw, const void* W, const float* gate, int32_t blocks, int32_t bsize,
                   int32_t dtype, void* stream) {
    if (!dw_out || !dg || !dw || !W || !gate || blocks <= 0) return BSMM_ERR_ARG;
    if (bsize != 8 && bsize != 16 && bsize != 32) return BSMM_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case BSMM_F32: gate_grad_kernel<DTf32><<<blocks, 256, 0, st>>>(static_cast<float*>(dw_out), dg, static_cast<const float*>(dw), static_cast<const float*>(W), gate, bsize); break;
        case BSMM_F16: gate_grad_kernel<DTf16><<<blocks, 256, 0, st>>>(static_cast<uint16_t*>(dw_out), dg, static_cast<const uint16_t*>(dw), static_cast<const uint16_t*>(W), gate, bsize); break;
        case BSMM_BF16: gate_grad_kernel<DTbf16><<<blocks, 256, 0, st>>>(static_cast<uint16_t*>(dw_out), dg, static_cast<const uint16_t*>(dw), static_cast<const uint16_t*>(W), gate, bsize); break;
        default: return BSMM_ERR_UNSUPPORTED;
    }
    return (int)hipGetLastError();
}

int bsmm_gate_weights(const void* W, const float* gate, void* out, int32_t blocks, int32_t bsize, int32_t dtype, int32_t pieces, void* stream) {
    if (!W || !gate || !out || blocks <= 0) return BSMM_ERR_ARG;
    if ((bsize != 8 && bsize != 16 && bsize != 32 && bsize != 64) || (dtype != BSMM_F16 && dtype != BSMM_BF16) || (pieces != 1 && pieces != 2)) return BSMM_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int per8 = bsize * bsize / 8;
    const size_t total8 = (size_t)blocks * per8;
    const unsigned grid = (unsigned)((total8 + 255) / 256);
    const uint4* w = static_cast<const uint4*>(W);
    uint4* o = static_cast<uint4*>(out);
    if (dtype == BSMM_BF16) {
        if (pieces == 1) gate_weights_kernel<DTbf16, 1><<<grid, 256, 0, st>>>(w, gate, o, per8, total8);
        else             gate_weights_kernel<DTbf16, 2><<<grid, 256, 0, st>>>(w, gate, o, per8, total8);
    } else {
        if (pieces == 1) gate_weights_kernel<DTf16, 1><<<grid, 256, 0, st>>>(w, gate, o, per8, total8);
        else             gate_weights_kernel<DTf16, 2><<<grid, 256, 0, st>>>(w, gate, o, per8, total8);
    }
    return (int)hipGetLastError();
}

int bsmm_gated_repair(int op, const void* X, const void* W, void* Y, const bsmm_args* args) {
    if (op != BSMM_OP_FPROP && op != BSMM_OP_BPROP) return BSMM_ERR_ARG;
    return gated_repair(op == BSMM_OP_FPROP, X, W, Y, args);
}

#ifdef X4_TIMELINE
extern "C" int bsmm_debug_x4_timeline_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_x4_tl), sizeof(bsmm::g_x4_tl)); }
#endif
#ifdef X4_ENDSTAMPS
extern "C" int bsmm_debug_x4_ends_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_x4_ends), sizeof(bsmm::g_x4_ends)); }
#endif
#ifdef U2_STAMPS
extern "C" int bsmm_debug_u2_trace_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_u2_trace), sizeof(bsmm::g_u2_trace)); }
#endif
#ifdef U6_STAMPS
extern "C" int bsmm_debug_u6_trace_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_u6_trace), sizeof(bsmm::g_u6_trace)); }
#endif
#ifdef X4_STAMPS
extern "C" int bsmm_debug_x4_trace_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_x4_trace), sizeof(bsmm::g_x4_trace)); }
#endif
#ifdef BSMM_XC_TRACE
int bsmm_debug_trace_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_xc_trace), sizeof(bsmm::g_xc_trace)); }
#endif
#ifdef X7L_TRACE
int bsmm_debug_x7_trace_copy(void* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(bsmm::g_x7_trace), sizeof(bsmm::g_x7_trace)); }
#endif

int bsmm_identity_init(void* W, const int32_t* updat_lut, int32_t CB, int32_t KB, int32_t blocks, int32_t bsize,
                       float scale, int32_t dtype, void* stream) {
    if (!W || !updat_lut || CB <= 0 || KB <= 0 || blocks <= 0 || bsize <= 0) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case BSMM_F32:
            identity_init_kernel<DTf32><<<blocks, 256, 0, st>>>(static_cast<float*>(W), updat_lut, CB, KB, bsize, scale);
            break;
        case BSMM_F16:
            identity_init_kernel<DTf16><<<blocks, 256, 0, st>>>(static_cast<uint16_t*>(W), updat_lut, CB, KB, bsize, scale);
            break;
        case BSMM_BF16:
            identity_init_kernel<DTbf16><<<blocks, 256, 0, st>>>(static_cast<uint16_t*>(W), updat_lut, CB, KB, bsize, scale);
            break;
        default:
            return BSMM_ERR_UNSUPPORTED;
    }
    return (int)hipGetLastError();
}

// widths the plan options select (defaults: the wide shapes)
static inline int opt_xc_group(int32_t options) { return (options & BSMM_PLAN_XCOL_NARROW) ? XC_G : 16; }

static long xprop_plan(const int32_t* lut, int32_t segments, int32_t blocks, int32_t n_out, int32_t bsize, int32_t dtype, int32_t axis,
                       int32_t options, int32_t* out) {
    if (axis != 0 && axis != 1) return 0;
    if (bsize == 64) {      // 'BS64': the quadrant view's lut + the bsize-32 plan built from it (feature axis 1 only)
        if (axis != 1 || !lut || segments <= 0 || blocks <= 0 || blocks >= (1 << 28)) return axis != 1 ? 0 : -1;
        std::vector<int32_t> lut32, nested;
        if (!b64_expand_xprop_lut(lut, segments, blocks, lut32)) return -1;
        const int32_t nopt = options;
        const long nw = xprop_plan(lut32.data(), 2 * segments, 4 * blocks, 2 * n_out, 32, dtype, axis, nopt, nullptr);
        if (nw < 0) return -1;
        nested.resize((size_t)nw);
        if (nw > 0 && out) xprop_plan(lut32.data(), 2 * segments, 4 * blocks, 2 * n_out, 32, dtype, axis, nopt, nested.data());
        return b64_emit(0, blocks, segments, lut32, nested, out);
    }
    if (bsize == 8) return dtype == BSMM_F32 ? 0 : build_super8_xprop_plan(lut, segments, blocks, n_out, out, opt_xc_group(options));   // 'BSS8'
    if (bsize != 32 && bsize != 16) return 0;   // plan kernels: bsize 32 (any dtype) / 16 and 8 (16-bit)
    if (dtype == BSMM_F32) {
        if (bsize != 32) return 0;
        return build_xcol_plan(lut, segments, blocks, n_out, out, XS_G);      // (BSMM_PLAN_F32_MFMA named the retired fp32 matrix-core kernel: ignored)
    }
    if (bsize == 16)         // 'BSX7' (staged / list kernels); BSMM_PLAN_XCOL_UNSTAGED / _NARROW named the round-1 kernel, retired in round 4: ignored
        return build_xcol16s_plan(lut, segments, blocks, n_out, out, !(options & BSMM_PLAN_FLOW_CONSECUTIVE));      // (0: the layout does not fit the table fields -> no plan, per-segment kernels)
    if ((options & BSMM_PLAN_XCOL_FLOW) && axis == 1 && !(options & (BSMM_PLAN_XCOL_UNSTAGED | BSMM_PLAN_XCOL_NARROW))) {   // barrier-free persistent kernel
        const long n = build_xflow_plan(lut, segments, blocks, n_out, out, (options & BSMM_PLAN_FLOW_SCHEDULED) != 0, (options & BSMM_PLAN_FLOW_CONSECUTIVE) != 0);
        if (n != 0) return n;
    }
    if (!(options & (BSMM_PLAN_XCOL_UNSTAGED | BSMM_PLAN_XCOL_NARROW))) {   // default: the staged kernel (either feature axis)
        const long n = build_xcol2_plan(lut, segments, blocks, n_out, out, (options >> BSMM_PLAN_XPROP_PH_SHIFT) & 7, axis == 0 && !(options & BSMM_PLAN_FLOW_CONSECUTIVE));
        if (n != 0) return n;                                            // 0: the layout does not fit the table fields
    }
    return build_xcol_plan(lut, segments, blocks, n_out, out, opt_xc_group(options));
}

long bsmm_xprop_plan_words(const int32_t* host_lut, int32_t segments, int32_t blocks, int32_t n_out_blocks, int32_t bsize,
                           int32_t dtype, int32_t axis, int32_t options) {
    return xprop_plan(host_lut, segments, blocks, n_out_blocks, bsize, dtype, axis, options, nullptr);
}

int bsmm_xprop_plan_build(const int32_t* host_lut, int32_t segments, int32_t blocks, int32_t n_out_blocks, int32_t bsize,
                          int32_t dtype, int32_t axis, int32_t options, int32_t* host_plan_out) {
    if (!host_plan_out) return BSMM_ERR_ARG;
    const long n = xprop_plan(host_lut, segments, blocks, n_out_blocks, bsize, dtype, axis, options, host_plan_out);
    return n > 0 ? BSMM_OK : (n == 0 ? BSMM_ERR_UNSUPPORTED : BSMM_ERR_ARG);
}

static long updat_plan(const int32_t* lut, int32_t blocks, int32_t CB, int32_t KB, int32_t bsize, int32_t dtype, int32_t axis, int32_t options,
                       int32_t* out) {
    if (dtype == BSMM_F32 || (axis != 0 && axis != 1)) return 0;   // windowed kernels: 16-bit types
    if (bsize == 64) {      // 'BS64': the quadrant view's updat lut + the bsize-32 (streaming) plan built from it
        if (axis != 1 || !lut || blocks <= 0 || blocks >= (1 << 28)) return axis != 1 ? 0 : -1;
        std::vector<int32_t> lut32((size_t)8 * blocks), nested;
        for (int w = 0; w < blocks; ++w)
            for (int q = 0; q < 4; ++q) {
                lut32[(size_t)2 * (4 * w + q)] = 2 * lut[2 * w] + (q >> 1);
                lut32[(size_t)2 * (4 * w + q) + 1] = 2 * lut[2 * w + 1] + (q & 1);
            }
        const int32_t nopt = options | BSMM_PLAN_UPDAT_NO_DIRECT;      // (the composite call derives the nested plan's descriptor itself: no direct blocks there)
        const long nw = updat_plan(lut32.data(), 4 * blocks, 2 * CB, 2 * KB, 32, dtype, axis, nopt, nullptr);
        if (nw < 0) return -1;
        nested.resize((size_t)nw);
        if (nw > 0 && out) updat_plan(lut32.data(), 4 * blocks, 2 * CB, 2 * KB, 32, dtype, axis, nopt, nested.data());
        return b64_emit(1, blocks, 0, lut32, nested, out);
    }
    if (bsize == 8) return build_super8_updat_plan(lut, blocks, CB, KB, out);   // 'BSS8'
    if (bsize == 16) {
        // 'BSUP' items of the windowed kernel; on feature axis 0 the 'BSU6' section of the row-owner kernel behind them (header word [8]):
        // the call picks per minibatch size (updat_typed)
        const long base = build_updat_plan(lut, blocks, CB, KB, UW16, UP16_MAXB, out);
        if (base <= 0 || axis != 0 || (options & BSMM_PLAN_UPDAT16_WINDOWED)) return base;
        const long off = (base + 3) & ~3L;
        const long sec = build_updat16_rows_section(lut, blocks, CB, KB, out ? out + off : nullptr);
        if (sec <= 0) return base;
        if (out) { std::fill(out + base, out + off, 0); out[8] = (int32_t)off; }
        return off + sec;
    }
    if (bsize != 32) return 0;
    int force = options & BSMM_PLAN_WINDOW_MASK;
    // BSMM_PLAN_WINDOW_8 / _16 / _16W named the windowed bsize-32 kernels of round 1 (retired in round 4): the same window side on the streaming kernel
    if (force == BSMM_PLAN_WINDOW_8) force = BSMM_PLAN_STREAM_8;
    if (force == BSMM_PLAN_WINDOW_16 || force == BSMM_PLAN_WINDOW_16W) force = BSMM_PLAN_STREAM_16;
    {     // either feature axis
        // streaming kernel: 16x16 windows while a window's blocks fit the 64 accumulator slots of a workgroup (with some
        // slack for the rows that do not pack: <= 56 on average), 8x8 windows for denser layouts
        const double windows = (double)((CB + 15) / 16) * ((KB + 15) / 16);
        int ws = force == BSMM_PLAN_STREAM_16 ? 16 : (force == BSMM_PLAN_STREAM_8 ? 8 : (blocks <= 56.0 * windows ? 16 : 8));
        // very sparse layouts on feature axis 1: 32 x 32 windows (a 16 x 16 window then holds < 10 blocks for its 32 KiB per chunk).  Measured at
        // 8192^2, N = 4096 (profiles/r03_updat_ws32.txt): 3 % 71 against 95 us; 5 % (BASELINE configs[3]) 102 against 96 -- so only below ~3.7 %
        // (Round 6: with DIRECT blocks the bigger window also wins at 4 - 5 % on a grid of >= 64 such windows -- 8192^2 N = 4096, BASELINE configs[3]:
        //  81 / 85 / 91 us at 4 / 4.5 / 5 % against 99 / 98 / 100 -- but only for LONG minibatches: at N = 1024 / 2048 it loses, 42 / 57 against 29 / 50 us,
        //  because 64 items need the partial sums and their summing pass where 256 items store directly.  A plan does not know the minibatch, so the
        //  rule stays; the host class builds the BSMM_PLAN_STREAM_32 plan as well and picks per call: profiles/r06_updat_ws32.txt)
        const double windows32 = (double)((CB + 31) / 32) * ((KB + 31) / 32);
        if (force == BSMM_PLAN_STREAM_32 || (force == 0 && axis == 1 && windows32 >= 16 && blocks <= 38.0 * windows32)) ws = 32;
        // direct blocks (round 6): what a window's 16 waves cannot hold gets its own workgroups instead of a sliced last round (feature axis 1)
        const int direct_max = (axis == 1 && !(options & BSMM_PLAN_UPDAT_NO_DIRECT)) ? U2_DIRECT_MAX : 0;
        return build_updat2_plan(lut, blocks, CB, KB, ws, out, (options >> BSMM_PLAN_UPDAT_SETS_SHIFT) & 15, direct_max);
    }
}

long bsmm_updat_plan_words(const int32_t* host_updat_lut, int32_t blocks, int32_t CB, int32_t KB, int32_t bsize, int32_t dtype,
                           int32_t axis, int32_t options) {
    return updat_plan(host_updat_lut, blocks, CB, KB, bsize, dtype, axis, options, nullptr);
}

int bsmm_updat_plan_build(const int32_t* host_updat_lut, int32_t blocks, int32_t CB, int32_t KB, int32_t bsize, int32_t dtype,
                          int32_t axis, int32_t options, int32_t* host_plan_out) {
    if (!host_plan_out) return BSMM_ERR_ARG;
    const long n = updat_plan(host_updat_lut, blocks, CB, KB, bsize, dtype, axis, options, host_plan_out);
    return n > 0 ? BSMM_OK : (n == 0 ? BSMM_ERR_UNSUPPORTED : BSMM_ERR_ARG);
}

// descriptor of a flat (non-composite) plan: (magic, width, waves, items)
static bool describe_flat(const int32_t* p, long words, int32_t d[5]) {
    if (words < 8) return false;
    d[4] = 0;
    switch (p[0]) {
        case XCPLAN_MAGIC:   if (p[1] != XCPLAN_VERSION || words < XC_HDR) return false;   d[1] = p[2]; d[2] = p[2]; d[3] = 0; break;
        case X2PLAN_MAGIC:   if (p[1] != X2PLAN_VERSION || words < X2_HDR || p[11] < 2 || p[11] > 4 || p[12] < X2_HDR || words < (long)p[12] + (long)p[3] * X2_G) return false;   d[1] = p[2]; d[2] = p[2]; d[3] = 0; d[4] = p[11]; break;
        case X4PLAN_MAGIC:   if (p[1] != X4PLAN_VERSION || words < X4_HDR || p[2] != X4_G) return false;   d[1] = p[2]; d[2] = p[2]; d[3] = 0; break;
        case X7PLAN_MAGIC:   if (p[1] != X7PLAN_VERSION || words < X7_HDR || p[12] < X7_HDR || words < (long)p[12] + (long)p[3] * X7_G) return false;   d[1] = p[2]; d[2] = 16; d[3] = 0; d[4] = p[14] ? 1 : 0; break;
        case UPLAN_MAGIC:    if (p[1] != UPLAN_VERSION || words < UP_HDR || p[8] < 0 || (p[8] > 0 && (p[8] + U6_HDR > words || p[p[8]] != U6PLAN_MAGIC ||
                                 p[8] + U6_HDR + (long)p[p[8] + 4] * U6_ITEM > words))) return false;
                             d[1] = p[2]; d[2] = p[7]; d[3] = p[4]; d[4] = p[8];               // (plan_inner: word offset of the 'BSU6' section, 0 = none;
                             if (p[8] > 0) {                                                   //  its window width / item count beside the plan's: up_pack)
                                 if (p[2] > 255 || p[7] > 255 || p[p[8] + 4] <= 0 || p[p[8] + 4] >= (1 << 23)) return false;
                                 d[1] = up_pack(p[2], p[p[8] + 3]); d[2] = up_pack(p[7], p[p[8] + 4]);
                             }
                             break;
        case U2PLAN_MAGIC:   if (p[1] != U2PLAN_VERSION || words < U2_HDR || p[26] != U2_HDR + p[4] * U2_ITEM || words < (long)p[26] + p[5]) return false;   // (the launcher addresses the block map behind the items)
                               if (p[27] < 0 || p[27] > 0x1fff || p[28] < 0 || p[28] > U2_DIRECT_MAX) return false;
                               if (p[28] > 0 && (p[30] != U2_DIRECT_PARTS || p[29] < p[26] + p[5] || words < (long)p[29] + 4L * p[28])) return false;      // direct blocks
                               d[1] = p[2]; d[2] = p[7]; d[3] = p[4]; d[4] = u2_pack_inner(p[8], p[25] > 0, p[27], p[28]); break;
        default: return false;
    }
    d[0] = p[0];
    return true;
}

int bsmm_plan_attach(bsmm_args* a, const int32_t* host_plan, long words, const int32_t* device_plan) {
    if (!a) return BSMM_ERR_ARG;
    a->plan = nullptr;
    a->plan_magic = a->plan_width = a->plan_waves = a->plan_items = a->plan_inner = 0;
    if (!device_plan) return BSMM_OK;
    if (!host_plan || words < 8 || (reinterpret_cast<uintptr_t>(device_plan) & 15)) return BSMM_ERR_ARG;
    int32_t d[5];
    if (host_plan[0] == S8PLAN_MAGIC) {
        if (host_plan[1] != S8PLAN_VERSION || host_plan[2] <= 0 || host_plan[6] != words) return BSMM_ERR_ARG;
        const int32_t off = host_plan[5];
        if (off < S8_HDR || off >= words || !describe_flat(host_plan + off, words - off, d)) return BSMM_ERR_ARG;
        int code = -1;                                                                    // word [7]: 0 = xprop, 1 = updat
        if (!host_plan[7] && d[0] == XCPLAN_MAGIC) code = 0;
        if (!host_plan[7] && d[0] == X2PLAN_MAGIC) code = 1;
        if (host_plan[7] && d[0] == UPLAN_MAGIC) code = 0;
        if (host_plan[7] && d[0] == U2PLAN_MAGIC) code = 2;
        if (code < 0 || d[1] > 255 || (uint32_t)d[4] >= (1u << 21)) return BSMM_ERR_ARG;
        a->plan_magic = S8PLAN_MAGIC; a->plan_width = host_plan[2]; a->plan_waves = d[2]; a->plan_items = d[3];
        a->plan_inner = s8_pack_inner(d[1], code, code ? d[4] : 0);
    } else if (host_plan[0] == B64PLAN_MAGIC) {
        if (host_plan[1] != B64PLAN_VERSION || host_plan[2] <= 0 || host_plan[6] != words || (host_plan[3] != 0 && host_plan[3] != 1)) return BSMM_ERR_ARG;
        const int32_t off = host_plan[5];
        if (off != b64_off_nested(host_plan[3], host_plan[7], host_plan[2]) || off > words) return BSMM_ERR_ARG;
        a->plan_magic = B64PLAN_MAGIC; a->plan_inner = host_plan[3];
        if (off < words) {      // a nested bsize-32 plan (none: the nested call runs the kernels without a plan)
            if (!describe_flat(host_plan + off, words - off, d) || nested_code(d[0]) == 0 || d[2] > 31 || (uint32_t)d[4] > 0xffffffu) return BSMM_ERR_ARG;
            a->plan_width = d[1]; a->plan_items = d[3];
            a->plan_waves = b64_pack_waves(d[2], nested_code(d[0]), d[4]);
        }
    } else {
        if (!describe_flat(host_plan, words, d)) return BSMM_ERR_ARG;
        a->plan_magic = d[0]; a->plan_width = d[1]; a->plan_waves = d[2]; a->plan_items = d[3]; a->plan_inner = d[4];
    }
    a->plan = device_plan;
    return BSMM_OK;
}

size_t bsmm_workspace_bytes(int op, const bsmm_args* a) {
    if (!a) return 0;
    const bool xprop_op = op == BSMM_OP_FPROP || op == BSMM_OP_BPROP;
    if (a->bsize == 64) {   // 'BS64' plans: [the quadrant copy of W, unless prepared][the quadrants' gates][what the nested bsize-32 call needs]
        if (a->axis != 1 || !a->plan || a->plan_magic != B64PLAN_MAGIC || a->plan_inner != (xprop_op ? 0 : 1)) return 0;
        bsmm_args b = b64_inner(a, !xprop_op);
        if (!xprop_op) { b.flags |= BSMM_FLAG_DW_SUMS; return bsmm_workspace_bytes(op, &b); }
        return (a->prepared_w ? 0 : b64_w_bytes(a)) + b64_gate_bytes(a) + bsmm_workspace_bytes(op, &b);
    }
    if (xprop_op) {
        // The maximum over the routes the call COULD take (no operand pointers here: the answer must not depend on their alignment).  Always among them
        // (no plan, a gate, the cost model): the per-segment kernels -- a transposed copy of W for fprop, an fp32 image of the output of locked tables behind it.
        size_t need = xprop_route_bytes(XRoute{XP_SEGMENT, op == BSMM_OP_FPROP && a->bsize != 8, false, a->locks > 0}, a);
        if (a->bsize == 8 && a->dtype != BSMM_F32 && a->plan && a->plan_magic == S8PLAN_MAGIC && a->plan_width > 0)      // 'BSS8' plans: the expanded W
            need = std::max(need, xprop_route_bytes(XRoute{XP_SUPER8, false, false, false}, a));
        if (a->bsize == 32 && a->dtype == BSMM_F32 && a->plan && a->plan_magic == XCPLAN_MAGIC)      // bf16 pieces of the activations and (unless prepared) the weights
            need = std::max(need, xprop_route_bytes(XRoute{XP_F32SPLIT, false, false, false}, a));
        return need;
    }
    if (op != BSMM_OP_UPDAT) return 0;
    if (a->dtype == BSMM_F32) {                                 // fp32 through bf16 pieces: the route's head + the pieces of X and DY; the three routes
        const URoute r = f32_split_route(a, true);              // that start at 256 minibatch rows are reserved for at ANY minibatch (as ever); the
        return r == UR_NONE ? 0 : f32_split_layout(a, r).bytes();   // per-block fp32 kernel of every other call needs no workspace
    }
    if (a->bsize == 8) {   // 'BSS8' plans: the fp32 sums of the super-blocks
        if (!a->plan || a->plan_magic != S8PLAN_MAGIC || a->plan_width <= 0) return 0;
        if (s8_nested_code(a) == 2) {      // nested streaming plan: its sums + partial-sum regions
            const bsmm_args b = s8_updat_inner(a);
            return u2_query_bytes(&b);
        }
        return (size_t)a->plan_width * 1024 * sizeof(float);
    }
    if (a->plan && (a->bsize == 32 || a->bsize == 16)) {
        if (a->plan_magic == U2PLAN_MAGIC) return u2_query_bytes(a);      // streaming kernel: sized as if gated, whatever the launch will store directly
        if (a->plan_magic != UPLAN_MAGIC || a->bsize != 16) return 0;     // (a plan check_plan refuses: nothing to size)
        // bsize 16 windowed kernel: one fp32 image of the sums (split-minibatch path); with the 'BSU6' section (feature axis 0) one image per part
        // of the row-owner kernel's largest minibatch split
        return updat16_images_bytes(a, a->plan_inner > 0 && a->axis == 0 ? U6_MAX_SPLIT : 1);
    }
    return 0;
}

const char* bsmm_error_string(int code) {
    switch (code) {
        case BSMM_OK: return "ok";
        case BSMM_ERR_ARG: return "bsmm: invalid argument (null pointer, non-positive size, misaligned lut, pcount outside 1..8)";
        case BSMM_ERR_UNSUPPORTED: return "bsmm: unsupported configuration (bsize must be 8/16/32, axis 0/1, dtype f32/f16/bf16, gate NULL)";
        case BSMM_ERR_WORKSPACE: return "bsmm: workspace missing, misaligned or smaller than bsmm_workspace_bytes()";
        default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "bsmm: unknown error";
    }
}

int bsmm_version(void) { return BSMM_VERSION; }

}  // extern "C"
