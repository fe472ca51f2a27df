// bsmm_xprop_dispatch.h -- fprop / bprop: the launchers of every kernel family, the ONE decision of a call (xprop_route), the workspace of
// each route (xprop_route_bytes) and the call itself (xprop_typed: decide, one workspace check, pre-passes, launch, finalize).
#pragma once
#include "bsmm_dispatch.h"
#include "bsmm_xcol.h"
#include "bsmm_xcol_v2.h"
#include "bsmm_xflow.h"
#include "bsmm_xsmall.h"
#include "bsmm_xsmall0.h"
#include "bsmm_xmid.h"
#include "bsmm_xcol16_v2.h"
#include "bsmm_xprop.h"

namespace {
// workgroup map of the grouped kernels: `ntiles` row tiles x `segments` groups; fewer than 8 row tiles: the groups of a tile over P XCDs
// (p_tiled: P for 8 tiles or more -- 1 but for measurement builds)
inline XMap xmap(int ntiles, int segments, int p_tiled = 1) {
    XMap m;
    m.ntiles = ntiles;
    m.segments = segments;
    m.P = ntiles >= 8 ? p_tiled : (8 + ntiles - 1) / ntiles;
    if (m.P > segments) m.P = segments;
    m.SP = (segments + m.P - 1) / m.P;
    return m;
}
template <class DT, int BS, int AXIS, bool FPROP>
int launch_xprop_valu(const void* X, const void* W, void* Y, const bsmm_args* a, hipStream_t st, float* yacc) {
    typedef typename DT::T T;
    dim3 grid(a->segments, (a->N + 255) / 256);    // segments on x: no 65535 limit
    trace(a, BSMM_K_XPROP_VALU);
    xprop_valu_kernel<DT, BS, AXIS, FPROP><<<grid, 256, 0, st>>>(static_cast<const T*>(X), static_cast<const T*>(W),
                                                                 static_cast<T*>(Y), a->lut, a->N, a->C, a->K, a->gate, yacc);
    return (int)hipGetLastError();
}

template <class DT, int BS, int AXIS>
int launch_xprop_mfma(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st, float* yacc) {
    typedef typename DT::T T;
    const int N = a->N;
    trace(a, BSMM_K_XPROP_SEGMENT);
    auto go = [&](auto nsub_tag) {
        constexpr int NSUB = decltype(nsub_tag)::value;
        constexpr int NT = 4 * BS * NSUB;
        const XMap m = xmap((N + NT - 1) / NT, a->segments);
        by_bool(a->gate != nullptr, [&](auto gated_tag) {
            constexpr bool GATED = decltype(gated_tag)::value;
            if constexpr (BS == 32)
                xprop32_kernel<DT, AXIS, NSUB, GATED><<<m.grid(), 256, 0, st>>>(static_cast<const T*>(X), static_cast<const T*>(Wsel),
                                                                                static_cast<T*>(Y), a->lut, m, N, a->C, a->K, a->gate, yacc);
            else
                xprop16_kernel<DT, AXIS, NSUB, GATED><<<m.grid(), 256, 0, st>>>(static_cast<const T*>(X), static_cast<const T*>(Wsel),
                                                                                static_cast<T*>(Y), a->lut, m, N, a->C, a->K, a->gate, yacc);
        });
    };
    // per-wave minibatch extent: BS*NSUB columns; use the wide tile only when it still fills the chip
    if constexpr (BS == 32) {
        if (N >= 2048) go(std::integral_constant<int, 2>{});
        else           go(std::integral_constant<int, 1>{});
    } else {
        if (N >= 2048) go(std::integral_constant<int, 4>{});
        else if (N >= 512) go(std::integral_constant<int, 2>{});
        else           go(std::integral_constant<int, 1>{});
    }
    return (int)hipGetLastError();
}

// grouped (xcol) kernels need args->plan built by bsmm_xprop_plan_build for args->lut
#ifndef BSMM_XC_WIDE_PH
#define BSMM_XC_WIDE_PH 4
#endif

// bsize 16, 'BSX7' plan: which inner loop.  The list-driven kernel multiplies every block on its own with the K = 16 instruction; where most
// blocks have their pair partner (dense layouts) the round-2 kernel's K = 32 instruction per PAIR wins on feature axis 1 -- measured at 4096^2,
// N = 8192 (profiles/r03_x7_density.txt): 20 % 152 / 145 against 166 / 149 us, 30 % 201 / 193 against 210 / 184, 50 % 315 / 319 against 284 / 263;
// on feature axis 0 the list kernel wins at every density (50 %: 251 / 237 against 321 / 301).
inline bool x7_use_list(const bsmm_args* a) {
#ifdef X7_POSITIONAL
    return a->axis == 0 && !a->gate;      // (measurement build: the pair kernel wherever it exists)
#else
    if (a->gate) return false;
    if (a->plan_inner & 1) return true;      // (doubled tables, header word [14] of the plan: the pair kernel's positional table cannot hold them)
    const double dens = (double)a->blocks / std::max(1.0, (a->C / 16.0) * (a->K / 16.0));
    return a->axis == 0 || dens < 0.4;
#endif
}

// 'BSX7' plans (check_plan; the round-1 kernel and its 'BSX6' plans were retired in round 4), never gated (xprop_route).  list: the
// list kernel (XRoute::own_transpose), which reads W as stored (transw) or its transposed copy; else the pair kernel
template <class DT, int AXIS>
int launch_xcol16_v2(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st, bool list, bool transw) {
    typedef typename DT::T T;
    const int n_out = a->K / 16;
    const XMap m = xmap((a->N + XC_R - 1) / XC_R, (n_out + X7_G - 1) / X7_G);
    trace(a, BSMM_K_XCOL16_STAGED);
    if (!list) {
        // (feature axis 1, dense layouts only -- x7_use_list: on feature axis 0 the list kernel wins at every density, and that instantiation
        //  of the pair kernel spilled 4 registers: not built)
        if constexpr (AXIS == 1) {
            if (int rc = ensure_lds<&xcol16_v2_kernel<DT, 1, false>>(X7_LDS)) return rc;
            xcol16_v2_kernel<DT, 1, false><<<m.grid(), 1024, X7_LDS, st>>>(static_cast<const T*>(X), static_cast<const T*>(Wsel), static_cast<T*>(Y), a->plan, m,
                                                                           a->N, a->C, a->K, nullptr);
            return (int)hipGetLastError();
        }
        return BSMM_ERR_ARG;
    }
    return by_bool(transw, [&](auto tw) -> int {
        constexpr bool TW = decltype(tw)::value;
        if (int rc = ensure_lds<&xcol16_list_kernel<DT, AXIS, TW>>(X7_LDS)) return rc;
        xcol16_list_kernel<DT, AXIS, TW><<<m.grid(), 1024, X7_LDS, st>>>(static_cast<const T*>(X), static_cast<const T*>(Wsel), static_cast<T*>(Y), a->plan, m,
                                                                        a->N, a->C, a->K);
        return (int)hipGetLastError();
    });
}

// fp32 on the bf16 matrix cores: split pre-passes into the workspace ([3][N*C] activation pieces, then [3][blocks*1024]
// weight pieces), then the wide xcol kernel with three slabs per step.
inline size_t xcols_w_bytes(const bsmm_args* a) { return 6 * (size_t)a->blocks * 1024; }
#ifndef XS_NO_FUSE      // (experiment switch: -DXS_NO_FUSE=1 keeps the activation-split pre-pass on feature axis 1 too, for A/B)
#define XS_NO_FUSE 0
#endif
// feature axis 1 (round 4): the activations are split inside the kernel (xcol32sf_kernel) -- no pieces of X in the workspace
inline bool xcols_fused(const bsmm_args* a) { return a->axis == 1 && !XS_NO_FUSE; }
inline size_t xcols_workspace_bytes(const bsmm_args* a) {
    return (xcols_fused(a) ? 0 : 6 * (size_t)a->N * a->C) + (a->prepared_w ? 0 : xcols_w_bytes(a));
}
// (the 16-wide 'BSXC' plan: check_plan; X 16-byte aligned and C % 32 == 0: xprop_route; the workspace: checked by xprop_typed)
template <int AXIS>
int launch_xcol32s(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a, hipStream_t st) {
    const size_t nx = (size_t)a->N * a->C;
    const bool fused = AXIS == 1 && xcols_fused(a);
    if (a->prepared_w && !aligned16(a->prepared_w)) return BSMM_ERR_ARG;
    uint16_t* xp = static_cast<uint16_t*>(a->workspace);
    const uint16_t* wp = static_cast<const uint16_t*>(a->prepared_w);
    if (!fused) split3_x_kernel<<<(unsigned)((nx / 8 + 255) / 256), 256, 0, st>>>(static_cast<const float*>(X), xp, nx);
    if (!wp) {      // W's pieces are a constant of the pass: a caller that holds them (bsmm_prepare_weights) skips this launch
        uint16_t* wq = fused ? xp : xp + 3 * nx;
        by_bool(fprop, [&](auto fp) { split3_w_kernel<decltype(fp)::value><<<a->blocks, 256, 0, st>>>(static_cast<const float*>(W), wq, a->blocks); });
        wp = wq;
    }
    const int n_out = a->K / 32;
    XMap m = xmap((a->N + XC_R - 1) / XC_R, (n_out + XS_G - 1) / XS_G);
    trace(a, BSMM_K_XCOL32_F32SPLIT);
    if constexpr (AXIS == 1) {
        if (fused) {
            if (int rc = ensure_lds<&xcol32sf_kernel>(XSF_LDS)) return rc;
#ifndef XSF_GMAP
#define XSF_GMAP 1      // (experiment switch: 0 = the row-tile-per-XCD mapping of the other grouped kernels)
#endif
            unsigned grid = (unsigned)m.grid();
            if (XSF_GMAP && m.segments % 8 == 0 && m.ntiles >= 4) { m.P = 0; grid = (unsigned)(m.segments * m.ntiles); }   // one group per XCD at a time
            xcol32sf_kernel<<<grid, 64 * XS_G, XSF_LDS, st>>>(static_cast<const float*>(X), wp, static_cast<float*>(Y), a->plan, m, a->N, a->C, a->K, a->blocks);
            return (int)hipGetLastError();
        }
    }
    if (int rc = ensure_lds<&xcol32s_kernel<AXIS>>(XS_LDS)) return rc;
    xcol32s_kernel<AXIS><<<m.grid(), 64 * XS_G, XS_LDS, st>>>(xp, wp, static_cast<float*>(Y), a->plan, m, a->N, a->C, a->K, a->blocks);
    return (int)hipGetLastError();
}

// round-1 grouped kernels ('BSXC' plans), W as stored (their TRANSW = true forms are not built: launch_xgroup32)
template <class DT, int AXIS, int G, int PH>
int launch_xcol_g(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st) {
    typedef typename DT::T T;
    const XMap m = xmap((a->N + XC_R - 1) / XC_R, (a->K / 32 + G - 1) / G);
    const T* x = static_cast<const T*>(X);
    const T* w = static_cast<const T*>(Wsel);
    if constexpr (AXIS == 1) {
        constexpr int LDS = xc_lds_bytes(G, PH);
        if (int rc = ensure_lds<&xcol32_a1_kernel<DT, false, G, PH>>(LDS)) return rc;
        trace(a, BSMM_K_XCOL32);
        xcol32_a1_kernel<DT, false, G, PH><<<m.grid(), 64 * G, LDS, st>>>(x, w, static_cast<T*>(Y), a->plan, m, a->N, a->C, a->K);
    } else {
        constexpr int LDS = 2 * PH * XC0_SLAB;
        if (int rc = ensure_lds<&xcol32_a0_kernel<DT, false, G, PH>>(LDS)) return rc;
        trace(a, BSMM_K_XCOL32);
        xcol32_a0_kernel<DT, false, G, PH><<<m.grid(), 64 * G, LDS, st>>>(x, w, static_cast<T*>(Y), a->plan, m, a->N, a->C, a->K);
    }
    return (int)hipGetLastError();
}

template <class DT, int AXIS>
int launch_xcol(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st) {
    if (a->plan_width == 16)   return launch_xcol_g<DT, AXIS, 16, BSMM_XC_WIDE_PH>(X, Wsel, Y, a, st);
    if (a->plan_width == XC_G) return launch_xcol_g<DT, AXIS, XC_G, XC_PH>(X, Wsel, Y, a, st);
    return BSMM_ERR_ARG;
}

template <class DT, bool TRANSW, int AXIS, bool GATED, int PH>
int launch_xcol_v2_ph(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st) {
    typedef typename DT::T T;
    const int n_out = a->K / 32;
    const XMap m = xmap((a->N + X2_R - 1) / X2_R, (n_out + X2_G - 1) / X2_G);
    if (int rc = ensure_lds<&xcol32_v2_kernel<DT, TRANSW, AXIS, GATED, PH>>(X2_LDS)) return rc;
    trace(a, BSMM_K_XCOL32_STAGED);
    xcol32_v2_kernel<DT, TRANSW, AXIS, GATED, PH><<<m.grid(), 64 * X2_G, X2_LDS, st>>>(static_cast<const T*>(X), static_cast<const T*>(Wsel), static_cast<T*>(Y), a->plan, m,
                                                                                 a->N, a->C, a->K, GATED ? a->gate : nullptr);
    return (int)hipGetLastError();
}

template <class DT, bool TRANSW, int AXIS, bool GATED = false>
int launch_xcol_v2(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st) {
    switch (a->plan_inner) {     // steps per phase the plan was cut for
        case 2: return launch_xcol_v2_ph<DT, TRANSW, AXIS, GATED, 2>(X, Wsel, Y, a, st);
        case 3: return launch_xcol_v2_ph<DT, TRANSW, AXIS, GATED, 3>(X, Wsel, Y, a, st);
        case 4: return launch_xcol_v2_ph<DT, TRANSW, AXIS, GATED, 4>(X, Wsel, Y, a, st);
    }
    return BSMM_ERR_ARG;
}

#ifndef BSMM_FLOW_P
#define BSMM_FLOW_P 0             // measurement builds: groups of a row tile spread over P XCDs (measured at the bench shape, profiles/r05_flow_xcd_map.txt: no effect)
#endif
// barrier-free persistent kernel ('BSX4' plans, bsmm_xflow.h): one workgroup per CU walks its (row tile, group) units
template <class DT, bool TRANSW, int RT>
int launch_xflow_rt(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st) {
    typedef typename DT::T T;
    const int n_out = a->K / 32;
    constexpr int R = 32 * RT;
    // (measurement builds, BSMM_FLOW_P: groups of a row tile spread over P XCDs -- an XCD then runs segments / P groups at a time)
    const XMap m = xmap((a->N + R - 1) / R, (n_out + X4_G - 1) / X4_G, BSMM_FLOW_P ? BSMM_FLOW_P : 1);
    if (int rc = ensure_lds<&xflow32_kernel<DT, TRANSW, RT>>(X4_LDS)) return rc;
    trace(a, BSMM_K_XCOL32_FLOW | (RT == 2 ? (BSMM_KV_FLOW_HALF_UNITS << 8) : 0));
    const int cus = device_cus();
    const int grid = std::min(m.grid(), std::max(8, cus / 8 * 8));
    xflow32_kernel<DT, TRANSW, RT><<<grid, 64 * X4_G, X4_LDS, st>>>(static_cast<const T*>(X), static_cast<const T*>(Wsel), static_cast<T*>(Y), a->plan,
                                                                    m, a->N, a->C, a->K);
    return (int)hipGetLastError();
}

// Units of 128 rows unless they leave CUs idle: 64-row units (twice as many, each with half the multiplies per weight block) from there down.
#ifndef BSMM_FLOW_RT
#define BSMM_FLOW_RT 0            // 0: by the unit count; 2 / 4: forced (measurement builds)
#endif
template <class DT, bool TRANSW>
int launch_xflow(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st) {
    const long units128 = (long)((a->N + X4_R - 1) / X4_R) * ((a->K / 32 + X4_G - 1) / X4_G);
    const bool half = BSMM_FLOW_RT == 2 || (BSMM_FLOW_RT == 0 && units128 < device_cus());
    return half ? launch_xflow_rt<DT, TRANSW, 2>(X, Wsel, Y, a, st) : launch_xflow_rt<DT, TRANSW, 4>(X, Wsel, Y, a, st);
}

template <class DT, int AXIS>
int launch_xgroup32(const void* X, const void* Wsel, void* Y, const bsmm_args* a, hipStream_t st, bool transw) {
    if (a->plan_magic == X4PLAN_MAGIC) {      // (X4_G wide, feature axis 1: check_plan; never gated: xprop_route; never nested in a 'BSS8' plan: s8_inner)
        if constexpr (AXIS == 1) return by_bool(transw, [&](auto tw) { return launch_xflow<DT, decltype(tw)::value>(X, Wsel, Y, a, st); });
        else return BSMM_ERR_ARG;
    }
    if (a->plan_magic == X2PLAN_MAGIC) {
        if (a->plan_width != X2_G) return BSMM_ERR_ARG;
        return by_bool(transw, [&](auto tw) {
            constexpr bool TW = decltype(tw)::value;
            return a->gate ? launch_xcol_v2<DT, TW, AXIS, true>(X, Wsel, Y, a, st) : launch_xcol_v2<DT, TW, AXIS>(X, Wsel, Y, a, st);
        });
    }
    // round-1 grouped kernels ('BSXC' plans: the bsize-8 super-block path): fprop always comes with the transposed copy of W (`transw` is
    // only ever set for the staged / flow plans above), so the TRANSW = true instantiations -- the axis-0 one spilled 3 registers -- are not built
    if (a->plan_magic != XCPLAN_MAGIC || transw) return BSMM_ERR_ARG;
    return launch_xcol<DT, AXIS>(X, Wsel, Y, a, st);
}

template <class DT, int BS>
int launch_transpose(const void* W, void* Wt, int blocks, hipStream_t st) {
    typedef typename DT::T T;
    transpose_blocks_kernel<DT, BS><<<blocks, 256, 0, st>>>(static_cast<const T*>(W), static_cast<T*>(Wt), blocks);
    return (int)hipGetLastError();
}

// Workspace layout of an xprop call (both parts 16-byte aligned): [0, wt) the transposed / expanded / split weights of
// the kernel that runs, then [wt, wt + N*K*4) the fp32 accumulators of LOCKED output blocks when the reference-policy
// table is walked by the per-segment kernels with a 16-bit storage type (lut segments that share an output block are
// summed in fp32 and rounded ONCE by lock_finalize_kernel -- the reference rounds every partial sum to 16 bit with
// red.add.f16x2, src/blocksparse_hgemm_cn_64_op_gpu.cu:211-240).
inline size_t wt_bytes(const bsmm_args* a) { return round16((size_t)a->blocks * a->bsize * a->bsize * elem_size(a->dtype)); }
inline size_t lock_acc_bytes(const bsmm_args* a) {
    return (a->locks > 0 && a->dtype != BSMM_F32) ? (size_t)a->N * a->K * sizeof(float) : 0;
}
// workspace of the super-block xprop path: the expanded W, then the non-finite flag of the call
inline size_t s8_w_bytes(const bsmm_args* a) { return round16((size_t)a->plan_width * 1024 * elem_size(a->dtype)); }
inline size_t s8_xprop_bytes(const bsmm_args* a) { return s8_w_bytes(a) + 16; }

// bsize 8 on the matrix cores: W expanded into the 32x32 super-blocks of the 'BSS8' plan, then the bsize-32 kernel of the nested plan.
// Exactness with non-finite activations: a super-block multiplies its zero-filled (absent) 8x8 parts with live
// activations, and 0 * Inf = NaN would reach outputs the reference leaves finite (it walks only the lookup-table entries,
// blocksparse/matmul.py:353-392).  One scan of X leaves a flag behind the expanded weights; when it is set -- never, for a
// healthy network -- the per-entry V_FMA kernel recomputes Y after the matrix-core pass (same stream, Y fully rewritten).
template <class DT, int AXIS>
int launch_xsuper8(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a, hipStream_t st) {
    typedef typename DT::T T;
    const int ns = a->plan_width;
    int32_t* flag = reinterpret_cast<int32_t*>(static_cast<char*>(a->workspace) + s8_w_bytes(a));
    by_bool(fprop, [&](auto fp) { expand8_kernel<DT, decltype(fp)::value><<<ns, 256, 0, st>>>(static_cast<const T*>(W), a->plan, static_cast<T*>(a->workspace), flag); });
    const size_t n8 = (size_t)a->N * a->C / 8;                 // (C % 32 == 0 and X 16-byte aligned on this path)
    const int sgrid = (int)std::min<size_t>((n8 + 255) / 256, (size_t)device_cus() * 8);
    if (a->dtype == BSMM_BF16) nonfinite16_kernel<0x7f80u><<<sgrid, 256, 0, st>>>(static_cast<const uint4*>(X), n8, flag);
    else                       nonfinite16_kernel<0x7c00u><<<sgrid, 256, 0, st>>>(static_cast<const uint4*>(X), n8, flag);
    bsmm_args b = s8_inner(a, false);
    int rc = launch_xgroup32<DT, AXIS>(X, a->workspace, Y, &b, st, false);
    if (rc) return rc;
    dim3 grid(a->segments, (a->N + 255) / 256);
    by_bool(fprop, [&](auto fp) {
        xprop_valu_kernel<DT, 8, AXIS, decltype(fp)::value><<<grid, 256, 0, st>>>(static_cast<const T*>(X), static_cast<const T*>(W), static_cast<T*>(Y), a->lut,
                                                                                 a->N, a->C, a->K, nullptr, nullptr, flag);
    });
    rc = (int)hipGetLastError();
    trace(a, BSMM_K_XPROP_SUPER8);
    return rc;
}

// the small-minibatch kernels, one launch per kernel family: its LDS latch, the trace, the launch (feature axis 1: rows of XSM_R; feature axis 0: columns of XS0_C)
template <class DT, int BS, int AXIS>
int launch_xsmall(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a, hipStream_t st) {
    typedef typename DT::T T;
    return by_bool(fprop, [&](auto fp) -> int {
        constexpr bool FP = decltype(fp)::value;
        const T* x = static_cast<const T*>(X);
        const T* w = static_cast<const T*>(W);
        T* y = static_cast<T*>(Y);
        const dim3 grid(a->segments, AXIS == 1 ? (a->N + XSM_R - 1) / XSM_R : (a->N + XS0_C - 1) / XS0_C);
        if constexpr (BS != 32 && AXIS == 1) {
            constexpr int LDSN = XSM_NW * XSM_PART;
            if (int rc = ensure_lds<&xsmall_narrow_kernel<DT, BS, FP>>(LDSN)) return rc;
            trace(a, BSMM_K_XPROP_SMALL);
            xsmall_narrow_kernel<DT, BS, FP><<<grid, 64 * XSM_NW, LDSN, st>>>(x, w, y, a->lut, a->N, a->C, a->K);
        } else if constexpr (BS == 32 && AXIS == 1) {
            if (int rc = ensure_lds<&xsmall32_kernel<DT, FP>>(XSM_LDS)) return rc;
            trace(a, BSMM_K_XPROP_SMALL);
            xsmall32_kernel<DT, FP><<<grid, 64 * XSM_NW, XSM_LDS, st>>>(x, w, y, a->lut, a->N, a->C, a->K);
        } else if constexpr (BS == 8) {
            if (int rc = ensure_lds<&xsmall8_a0_kernel<DT, FP>>(XS16_LDS)) return rc;
            trace(a, BSMM_K_XPROP_SMALL);
            xsmall8_a0_kernel<DT, FP><<<grid, 64 * XS0_NW, XS16_LDS, st>>>(x, w, y, a->lut, a->N);
        } else if constexpr (BS == 16) {
            if (int rc = ensure_lds<&xsmall16_a0_kernel<DT, FP>>(XS16_LDS)) return rc;
            trace(a, BSMM_K_XPROP_SMALL);
            xsmall16_a0_kernel<DT, FP><<<grid, 64 * XS0_NW, XS16_LDS, st>>>(x, w, y, a->lut, a->N);
        } else {
            if (int rc = ensure_lds<&xsmall32_a0_kernel<DT, FP>>(XS0_LDS)) return rc;
            trace(a, BSMM_K_XPROP_SMALL);
            xsmall32_a0_kernel<DT, FP><<<grid, 64 * XS0_NW, XS0_LDS, st>>>(x, w, y, a->lut, a->N);
        }
        return (int)hipGetLastError();
    });
}

#ifndef BSMM_MID_MAP
#define BSMM_MID_MAP 0            // the medium-minibatch kernel's workgroup shape: 0 = by the size of the activations, 1 = one block x 4 row chunks, 2 = 4 blocks x one row chunk
#endif
#ifndef BSMM_MID_RT
#define BSMM_MID_RT 0             // its rows per wave: 0 = by the wave count, 2 = 64, 4 = 128 (measurement builds)
#endif
// medium minibatches (bsize 32, 16-bit, feature axis 1): one wave per (output block, 64 rows), bsmm_xmid.h
template <class DT>
int launch_xmid(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a, hipStream_t st) {
    typedef typename DT::T T;
    trace(a, BSMM_K_XPROP_MID);
    // (128-row waves -- <4, 6>, half the weight traffic per output -- measured no faster anywhere the flow kernel is not faster
    //  still: BSMM_MID_RT=4 builds them for measurements)
    const bool big = BSMM_MID_RT == 4;
    auto go = [&](auto rt_tag, auto dws_tag) -> int {
        constexpr int RT = decltype(rt_tag)::value, DWS = decltype(dws_tag)::value;
        // which four tasks make a workgroup: see the kernel
        const int by_column = BSMM_MID_MAP == 1 || (BSMM_MID_MAP == 0 && (long)a->N * a->C * 2 <= (5L << 20)) ? 1 : 0;
        const int nchunks = (a->N + xmd_rows(RT) - 1) / xmd_rows(RT);
        const XMap m = by_column ? xmap((nchunks + XMD_NW - 1) / XMD_NW, a->segments) : xmap(nchunks, (a->segments + XMD_NW - 1) / XMD_NW);
        constexpr int LDS = xmd_lds(RT, DWS);
        return by_bool(fprop, [&](auto fp) -> int {
            constexpr bool FP = decltype(fp)::value;
            if (int rc = ensure_lds<&xmid32_kernel<DT, FP, RT, DWS>>(LDS)) return rc;
            xmid32_kernel<DT, FP, RT, DWS><<<m.grid(), 64 * XMD_NW, LDS, st>>>(static_cast<const T*>(X), static_cast<const T*>(W), static_cast<T*>(Y), a->lut, m,
                                                                              a->segments, a->N, a->C, a->K, by_column);
            return (int)hipGetLastError();
        });
    };
    return big ? go(std::integral_constant<int, 4>{}, std::integral_constant<int, 6>{}) : go(std::integral_constant<int, 2>{}, std::integral_constant<int, 4>{});
}

enum XPath { XP_VALU, XP_SEGMENT, XP_XCOL32, XP_XCOL16, XP_F32SPLIT, XP_SUPER8, XP_SMALL, XP_MID };
#ifndef BSMM_SMALL_N_MAX
#define BSMM_SMALL_N_MAX 4096     // the small-minibatch kernel (bsmm_xsmall.h) is considered up to this many minibatch rows (the cost model decides)
#endif
#ifndef XS0_NMAX
#define XS0_NMAX 512              // feature axis 0: the small-minibatch kernel (bsmm_xsmall0.h) up to this many minibatch columns
#endif
#ifndef XSN_NMAX
#define XSN_NMAX 512              // bsize 16 / 8, feature axis 1: the narrow small-minibatch kernel (bsmm_xsmall.h) up to this many minibatch rows
#endif
#ifndef BSMM_MID_MODE
#define BSMM_MID_MODE 0           // medium-minibatch kernel (bsmm_xmid.h): 0 = by the cost model, 1 = whenever it can run, -1 = never (measurement builds)
#endif

// ONE decision per call, as updat_path / UPath on the other half: the kernel family and what follows from it for the workspace layout,
// the pre-passes and the launch (they used to be derived separately and could disagree).
struct XRoute {
    XPath path;
    bool wt_copy;           // the call needs the transposed copy of W at the start of the workspace: fprop, not XP_VALU, not bsize 8, not a kernel that transposes for itself
    bool own_transpose;     // the kernel reads W transposed itself: the staged / flow 'BSX2' / 'BSX4' plans, the 'BSX7' list kernel (x7_use_list is asked here and nowhere else)
    bool locked;            // locked outputs on the per-segment kernels: fp32 accumulators behind the copy (16-bit types) or a zero-fill of Y (fp32)
};

template <class DT, int BS, int AXIS>
XRoute xprop_route(const void* X, const void* W, const void* Y, const bsmm_args* a, bool fprop) {
    auto take = [&](XPath p) {
        XRoute r = {p, false, false, false};
        r.own_transpose = (p == XP_XCOL32 && (a->plan_magic == X2PLAN_MAGIC || a->plan_magic == X4PLAN_MAGIC)) || (p == XP_XCOL16 && a->plan_magic == X7PLAN_MAGIC && x7_use_list(a));
        r.wt_copy = fprop && BS != 8 && (p == XP_SEGMENT || ((p == XP_XCOL32 || p == XP_XCOL16) && !r.own_transpose));
        r.locked = (p == XP_VALU || p == XP_SEGMENT) && a->locks > 0;   // several segments accumulate into the same output block
        return r;
    };
    const int variant = call_variant(a);
    const bool vec_ok = aligned16(X) && aligned16(W) && aligned16(Y);
    // gated calls: the staged bsize-32 kernel applies gates (exactly: bsmm_xcol_v2.h); everything else runs the per-segment kernels.
    // (Round 6: the GATED instantiation of the bsize-16 pair kernel is no longer built -- 22 spilled registers, 280-308 us at BASELINE
    //  configs[2]'s shape against 85 us ungated; a gated call on the fast kernels is bsmm_gate_weights + the UNGATED call, include/bsmm.h.)
    const bool gate_ok = a->gate == nullptr || (DT::is16 && BS == 32 && a->plan_magic == X2PLAN_MAGIC);
    const bool plan_ok = a->plan != nullptr && gate_ok && vec_ok && (variant == 0 || variant == 3);
    const bool force = variant == 3;
    // what the kernels without a gate and without fp32 accumulators ask of a call, and the "plain call" of the production dispatch among them
    const bool free_out = vec_ok && !a->gate && a->locks == 0 && a->segments > 0;
    const bool plain = variant == 0 && free_out;
    if constexpr (BS == 8) {
        if constexpr (DT::is16 && AXIS == 0) {      // short minibatches on feature axis 0 (bsmm_xsmall0.h, round 6: the reference benchmark's (8, 0) shapes)
            // (BS=8 in scripts/gpu_a0_xprop_sweep.py: at N = 1024 114 against 365, 51 against 108, 162 against 226, 249 against 451 us)
            if (plain && a->N % 8 == 0 && a->N <= 2 * XS0_NMAX) return take(XP_SMALL);
        }
        if constexpr (DT::is16 && AXIS == 1) {      // short minibatches on feature axis 1 (bsmm_xsmall.h::xsmall_narrow_kernel, round 6)
            // (the same sweep: against the V_FMA kernel 11.6 against 32 us at 4096^2 10 % N = 64, 43 against 216 at 20480 / 1.5 %; up to 512 rows it also
            //  beats the super-block path where that applies: 291 against 426 us at 20480 / 1.5 % N = 512)
            if (plain && a->N <= XSN_NMAX && a->C % 8 == 0 && a->K % 8 == 0) return take(XP_SMALL);
        }
        if constexpr (DT::is16) {
            // bsize 8 on the matrix cores: expand W into the 32x32 super-blocks of the 'BSS8' plan and run the bsize-32 kernel
            const bool shape_ok = a->C % 32 == 0 && a->K % 32 == 0 && !(AXIS == 0 && (a->N % 8 != 0));
            const bool fill = (long)((a->N + XC_R - 1) / XC_R) * ((a->K / 32 + XC_G - 1) / XC_G) >= device_cus() * 7 / 8;
            // (locked reference-policy tables stay on the exact kernel: the repair pass of the super-block path writes Y directly)
            if (plan_ok && a->plan_magic == S8PLAN_MAGIC && a->plan_width > 0 && shape_ok && a->locks == 0 && (fill || force)) return take(XP_SUPER8);
        }
        if constexpr (DT::is16 && AXIS == 0) {
            // no super-block path for this call (no plan, or too few units for the chip -- hidden 2560 at N = 2048: 643 us on the V_FMA kernel): the
            // pair kernel at any minibatch (its time grows with blocks x N like the V_FMA kernel's, at a third of it)
            if (plain && a->N % 8 == 0) return take(XP_SMALL);
        }
        return take(XP_VALU);
    }
    if (variant == 1 || !vec_ok) return take(XP_VALU);
    // the per-segment kernel without a plan, us per call (round 4: refit on graph replays -- the 14.4 us floor of round 2 was the host's)
    const double t_segment_noplan = 6.0 + 1.2e-5 * (double)a->blocks * a->N;
    // small minibatches on feature axis 1: every output block's entry list cut over the 8 waves of a workgroup (bsmm_xsmall.h); needs no plan.
    // Measured as hipGraph replays (scripts/gpu_smalln_sweep.py, profiles/r04_smalln.txt): 3 + 1.35e-5 us per (block, minibatch row)
    bool small_ok = false;
    double t_small = 0.0;
    if constexpr (BS == 32 && DT::is16 && AXIS == 1) {
        small_ok = plain && a->N <= BSMM_SMALL_N_MAX && a->C % 32 == 0 && a->K % 32 == 0;
        t_small = 3.0 + 1.35e-5 * (double)a->blocks * a->N;
    }
    // medium minibatches: one wave per (output block, 64 rows) walks the block's whole entry list from a private LDS ring (bsmm_xmid.h)
    bool mid_ok = false;
    double t_mid = 0.0;
    if constexpr (BS == 32 && DT::is16 && AXIS == 1) {
        mid_ok = BSMM_MID_MODE >= 0 && (variant == 0 || (a->flags & BSMM_FLAG_FORCE_MID)) && free_out && a->C % 32 == 0 && a->K % 32 == 0 &&
                 (long)a->N * a->C * 2 < (1L << 32) && a->blocks < (1 << 21);
        // measured as hipGraph replays (profiles/r04_smalln.txt): ~0.9 us per entry of a column and round of 8 waves per CU; a half-empty
        // machine is not proportionally faster (occupancy o: o >= 1 -> o, below -> 0.25 + 0.5 o)
        const double o = (double)a->segments * ((a->N + 63) / 64) / (8.0 * device_cus());
        t_mid = 4.5 + 0.9 * ((double)a->blocks / a->segments) * std::max(1.12 * o, 0.25 + 0.5 * o);   // (full rounds: 12 % more per round, measured)
        if ((BSMM_MID_MODE > 0 || (a->flags & BSMM_FLAG_FORCE_MID)) && mid_ok) return take(XP_MID);
    }
    // small minibatches on feature axis 0 (round 6, bsmm_xsmall0.h): the regime of the reference's own benchmark (N = 64).  Measured against the
    // per-segment and the plan kernels in scripts/gpu_a0_xprop_sweep.py
    if constexpr ((BS == 32 || BS == 16) && DT::is16 && AXIS == 0) {
        // (hipGraph replays, fprop / bprop us, this kernel against what ran before: hidden 2560 dense N = 64 8.3 / 8.1 against 45.8 / 27.1, N = 512 22.7
        //  against 64.6 / 54.3, N = 1024 38.5 against 95; 20480 at 1.7 % N = 64 10.5 against 63.8 / 44.3, N = 512 60 against 82 / 73, N = 1024 116
        //  against 91 / 81: up to 512 columns always, up to 1024 where the columns are long -- >= 16 blocks on average)
        // (bsize 16, the same sweep with BS=16: at N = 1024 the kernel still wins at every shape -- 51 against 118, 25 against 41, 72 against 83, 109 against 210 us)
        const bool n_ok = a->N <= XS0_NMAX || (a->N <= 2 * XS0_NMAX && (BS == 16 || (long)a->blocks >= 16L * a->segments));
        if (plain && a->N % 8 == 0 && n_ok && a->C % BS == 0 && a->K % BS == 0) return take(XP_SMALL);
    }
    if constexpr (BS == 16 && DT::is16 && AXIS == 1) {
        // (scripts/gpu_a1_narrow_sweep.py, hipGraph replays: against the per-segment kernel the narrow kernel wins fprop up to 256 rows -- 7.2 against
        //  14.8 us at 4096^2 10 % N = 64, 58 against 73 at hidden 2560 dense N = 256: that kernel transposes W in a pre-pass -- and bprop up to 64)
        if (plain && a->N <= (fprop ? XSN_NMAX / 2 : XSN_NMAX / 8) && a->C % 16 == 0 && a->K % 16 == 0) return take(XP_SMALL);
    }
    if (!plan_ok) {
        if (mid_ok && t_mid < (small_ok ? t_small : 1e30) && t_mid < t_segment_noplan + 8.0) return take(XP_MID);
        if (small_ok && t_small < t_segment_noplan + 8.0) return take(XP_SMALL);     // (the per-segment fprop also pays a transpose pre-pass)
        return take(XP_SEGMENT);
    }
    // grouped kernels need enough (row tile x group) workgroups to fill 256 CUs; below that the per-segment kernel,
    // which has segments x tiles workgroups, is faster
    if constexpr (BS == 16) {
        if constexpr (!DT::is16) return take(XP_SEGMENT);
        if (AXIS == 0 && (a->N % 8 != 0)) return take(XP_SEGMENT);            // 16-byte aligned row pieces
        if (a->plan_magic == X7PLAN_MAGIC && (AXIS == 1 ? (long)a->C : (long)a->N) * 256 >= (1L << 32)) return take(XP_SEGMENT);   // 32-bit lane offsets
        const bool enough = (long)((a->N + XC_R - 1) / XC_R) * ((a->K / 16 + 15) / 16) >= device_cus() * 7 / 8;
        return take((enough || force) ? XP_XCOL16 : XP_SEGMENT);
    }
    if constexpr (BS == 32 && !DT::is16) {
        if (a->plan_magic != XCPLAN_MAGIC) return take(XP_SEGMENT);           // 'BSXC' (G = 16): the exact bf16 split
        if (AXIS == 0 && (a->N % 8 != 0)) return take(XP_SEGMENT);
        if (a->C % 32 != 0) return take(XP_SEGMENT);
        const bool enough = (long)((a->N + 127) / 128) * ((a->K / 32 + XC_G - 1) / XC_G) >= device_cus() * 7 / 8;
        return take((enough || force) ? XP_F32SPLIT : XP_SEGMENT);
    }
    if constexpr (BS == 32 && DT::is16) {
        if (AXIS == 0 && (a->N % 8 != 0)) return take(XP_SEGMENT);            // axis-0 xcol needs 16-byte aligned row pieces
        // staged kernel: 32-bit per-lane byte offsets inside a slab's source (128 rows of C elements / 64 rows of N elements)
        if ((a->plan_magic == X2PLAN_MAGIC || a->plan_magic == X4PLAN_MAGIC) && (AXIS == 1 ? (long)a->C : (long)a->N) * 256 >= (1L << 32)) return take(XP_SEGMENT);
        if (a->plan_magic == X4PLAN_MAGIC && AXIS != 1) return take(XP_SEGMENT);
        if (force) return take(XP_XCOL32);
        // Cost model fitted to the measurements in profiles/r01_sweeps.md (4096^2 / 20 % and 8192^2 / 5 %, N = 512 .. 8192):
        // the grouped kernel pays ~0.48 us per pair step of a group plus ~0.045 us per block, once per round of 256
        // workgroups, whatever the density; the per-segment kernel pays ~1.04e-5 us per (block, minibatch row).
        const int G = a->plan_width > 0 ? a->plan_width : 16;
        const double CB = a->C / 32.0, KB = a->K / 32.0;
        const double ngroups = (double)((a->K / 32 + G - 1) / G), ntiles = (double)((a->N + XC_R - 1) / XC_R);
        const double cus = (double)device_cus();
        const double rounds = std::max(1.0, std::ceil(ntiles * ngroups / cus));
        const double dens = std::min(1.0, a->blocks / std::max(1.0, CB * KB));
        const double steps = std::ceil(CB / 2.0) * (1.0 - std::pow(1.0 - dens, 2.0 * G));
        double t_group = rounds * (0.48 * steps + 0.045 * a->blocks / ngroups) + 8.0;
        double t_segment = 17.0 + 1.04e-5 * (double)a->blocks * a->N;
        if (a->plan_magic == X2PLAN_MAGIC || a->plan_magic == X4PLAN_MAGIC) {
            // staged kernel, refit (scripts/gpu_xprop_sweep.py, 4096^2 20 % / 5 %, 8192^2 5 %, 2048^2 20 %, N = 128 .. 8192): a round
            // costs 0.28 us per pair step + 0.040 us per block of the group, up to 20 % more when the round fills all CUs
            const double fill = std::min(1.0, ntiles * ngroups / rounds / cus);
            t_group = rounds * (0.28 * steps + 0.040 * a->blocks / ngroups) * (1.0 + 0.2 * fill) + 4.0;
            t_segment = t_segment_noplan;
        }
        if (mid_ok && t_mid <= t_group && t_mid <= t_segment && (!small_ok || t_mid < t_small)) return take(XP_MID);
        if (small_ok && t_small <= t_group && t_small <= t_segment) return take(XP_SMALL);
        return take(t_group < t_segment ? XP_XCOL32 : XP_SEGMENT);
    }
    return take(XP_SEGMENT);
}

// the fp32 accumulators of locked outputs lie behind the transposed copy of W when the call has one
inline size_t lock_acc_offset(const XRoute& r, const bsmm_args* a) { return r.wt_copy ? wt_bytes(a) : 0; }
// workspace of the route a call takes (0: none), checked once before anything is enqueued; bsmm_workspace_bytes: the maximum over the routes a call could take
inline size_t xprop_route_bytes(const XRoute& r, const bsmm_args* a) {
    switch (r.path) {
        case XP_SMALL: case XP_MID: return 0;
        case XP_SUPER8: return s8_xprop_bytes(a);
        case XP_F32SPLIT: return xcols_workspace_bytes(a);
        default: return lock_acc_offset(r, a) + (r.locked ? lock_acc_bytes(a) : 0);
    }
}

// decide, ONE workspace check, the pre-passes (transposed copy of W, zero-fill of locked outputs), the route's launcher, the lock finalize
template <class DT, int BS, int AXIS>
int xprop_typed(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const XRoute r = xprop_route<DT, BS, AXIS>(X, W, Y, a, fprop);
    if (!workspace_ok(a, xprop_route_bytes(r, a))) return BSMM_ERR_WORKSPACE;
    const void* Wsel = W;
    if (r.wt_copy) {      // these kernels read the weights with the contraction index contiguous
        if constexpr (BS != 8) {
            if (int rc = launch_transpose<DT, BS>(W, a->workspace, a->blocks, st)) return rc;
            Wsel = a->workspace;
        }
    }
    float* yacc = (r.locked && DT::is16) ? reinterpret_cast<float*>(static_cast<char*>(a->workspace) + lock_acc_offset(r, a)) : nullptr;
    if (r.locked) {      // start from zero: the fp32 accumulators (rounded once by the finalize pass below), or the fp32 Y itself
        const hipError_t e = yacc ? hipMemsetAsync(yacc, 0, lock_acc_bytes(a), st) : hipMemsetAsync(Y, 0, (size_t)a->N * a->K * elem_size(a->dtype), st);
        if (e != hipSuccess) return (int)e;
    }
    int rc = BSMM_ERR_UNSUPPORTED;
    switch (r.path) {      // (a route is only ever decided for the types and shapes its kernels are built for: the `if constexpr` of each case)
        case XP_VALU:     rc = by_bool(fprop, [&](auto fp) { return launch_xprop_valu<DT, BS, AXIS, decltype(fp)::value>(X, W, Y, a, st, yacc); }); break;
        case XP_SEGMENT:  if constexpr (BS != 8) rc = launch_xprop_mfma<DT, BS, AXIS>(X, Wsel, Y, a, st, yacc); break;
        case XP_XCOL32:   if constexpr (BS == 32 && DT::is16) rc = launch_xgroup32<DT, AXIS>(X, Wsel, Y, a, st, r.own_transpose && fprop); break;
        case XP_XCOL16:   if constexpr (BS == 16 && DT::is16) rc = launch_xcol16_v2<DT, AXIS>(X, Wsel, Y, a, st, r.own_transpose, fprop); break;
        case XP_F32SPLIT: if constexpr (BS == 32 && !DT::is16) rc = launch_xcol32s<AXIS>(fprop, X, W, Y, a, st); break;
        case XP_SUPER8:   if constexpr (BS == 8 && DT::is16) rc = launch_xsuper8<DT, AXIS>(fprop, X, W, Y, a, st); break;
        case XP_SMALL:    if constexpr (DT::is16) rc = launch_xsmall<DT, BS, AXIS>(fprop, X, W, Y, a, st); break;
        case XP_MID:      if constexpr (BS == 32 && DT::is16 && AXIS == 1) rc = launch_xmid<DT>(fprop, X, W, Y, a, st); break;
    }
    if (rc == 0 && yacc) {
        dim3 grid(a->segments, (a->N + 255) / 256);
        lock_finalize_kernel<DT, BS, AXIS><<<grid, 256, 0, st>>>(yacc, static_cast<T*>(Y), a->lut, a->N, a->K);
        rc = (int)hipGetLastError();
    }
    return rc;
}

// Exactness of a gated call that ran as [bsmm_gate_weights -> the UNGATED kernels] with non-finite activations: a gate-0 block is a zero image
// there, and the matrix cores multiply it with the live activations -- 0 * Inf = NaN would reach outputs that the in-kernel GATED path
// (`if (g == 0.f) continue`) and the reference (`if (gate != 0)`, src/blocksparse_hgemm_cn_64_op_gpu.cu:96-100) leave finite.  As on the
// super-block path (launch_xsuper8): one scan of X leaves a flag in the workspace; when it is set -- never, for a healthy network -- the per-entry
// V_FMA kernel recomputes Y from W and the gate over the PLAIN table after the matrix-core pass (same stream, Y fully rewritten; no host sync,
// capturable).  Activations that are not 16-byte aligned are not scanned: the flag is set and Y always recomputed.
template <class DT, int BS, int AXIS>
int gated_repair_typed(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a) {
    if constexpr (!DT::is16 || BS == 8) return BSMM_ERR_UNSUPPORTED;      // (what bsmm_gate_weights + the ungated call is taken for)
    else {
        typedef typename DT::T T;
        hipStream_t st = static_cast<hipStream_t>(a->stream);
        int32_t* flag = static_cast<int32_t*>(a->workspace);
        const bool scan = aligned16(X);
        if (hipMemsetAsync(flag, scan ? 0 : 1, 16, st) != hipSuccess) return (int)hipGetLastError();
        if (scan) {
            const size_t n8 = (size_t)a->N * a->C / 8;                 // (C % 16 == 0: check_common)
            const int sgrid = (int)std::min<size_t>((n8 + 255) / 256, (size_t)device_cus() * 8);
            if (a->dtype == BSMM_BF16) nonfinite16_kernel<0x7f80u><<<sgrid, 256, 0, st>>>(static_cast<const uint4*>(X), n8, flag);
            else                       nonfinite16_kernel<0x7c00u><<<sgrid, 256, 0, st>>>(static_cast<const uint4*>(X), n8, flag);
        }
        dim3 grid(a->segments, (a->N + 255) / 256);
        by_bool(fprop, [&](auto fp) {
            xprop_valu_kernel<DT, BS, AXIS, decltype(fp)::value><<<grid, 256, 0, st>>>(static_cast<const T*>(X), static_cast<const T*>(W), static_cast<T*>(Y), a->lut,
                                                                                      a->N, a->C, a->K, a->gate, nullptr, flag);
        });
        return (int)hipGetLastError();
    }
}

int gated_repair(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a) {
    int rc = check_common(a);
    if (rc) return rc;
    if (!X || !W || !Y || !a->gate || a->segments <= 0) return BSMM_ERR_ARG;
    if (a->bsize == 64 || a->locks != 0) return BSMM_ERR_UNSUPPORTED;      // (the repair pass writes Y directly: unlocked tables only)
    if (!workspace_ok(a, 16)) return BSMM_ERR_WORKSPACE;
    return with_dtype(a->dtype, [&](auto dt) {
        return by_shape(a, [&](auto bs, auto ax) { return gated_repair_typed<decltype(dt), decltype(bs)::value, decltype(ax)::value>(fprop, X, W, Y, a); });
    });
}

int xprop(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a);

// bsize 64: the bsize-32 call on the quadrants (b64_inner)
int xprop64(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a) {
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    if (!a->plan || !aligned16(W)) return BSMM_ERR_ARG;       // (check_plan: a 'BS64' xprop plan)
    bsmm_args b = b64_inner(a, false);
    // workspace: [quadrant copy of W, unless the caller prepared one][gates of the quadrants][the inner call's]
    const size_t wq = a->prepared_w ? 0 : b64_w_bytes(a), gq = b64_gate_bytes(a);
    const size_t inner = bsmm_workspace_bytes(fprop ? BSMM_OP_FPROP : BSMM_OP_BPROP, &b);
    if (!workspace_ok(a, wq + gq + inner)) return BSMM_ERR_WORKSPACE;
    char* ws = static_cast<char*>(a->workspace);
    const void* Wq = a->prepared_w;
    if (!Wq) {
        if (elem_size(a->dtype) == 4) b64_split_kernel<4><<<a->blocks, 256, 0, st>>>(static_cast<const unsigned char*>(W), reinterpret_cast<unsigned char*>(ws), a->blocks, fprop ? 0 : 1);
        else                          b64_split_kernel<2><<<a->blocks, 256, 0, st>>>(static_cast<const unsigned char*>(W), reinterpret_cast<unsigned char*>(ws), a->blocks, fprop ? 0 : 1);
        Wq = ws;
    } else if (!aligned16(Wq)) return BSMM_ERR_ARG;
    if (a->gate) {
        b64_gate_kernel<<<(4 * a->blocks + 255) / 256, 256, 0, st>>>(a->gate, reinterpret_cast<float*>(ws + wq), a->blocks);
        b.gate = reinterpret_cast<const float*>(ws + wq);
    }
    b.workspace = inner ? ws + wq + gq : nullptr;
    b.workspace_bytes = inner ? a->workspace_bytes - wq - gq : 0;
    return xprop(fprop, X, Wq, Y, &b);
}

int xprop(bool fprop, const void* X, const void* W, void* Y, const bsmm_args* a) {
    int rc = check_common(a);
    if (rc) return rc;
    if (!X || !W || !Y || a->segments <= 0) return BSMM_ERR_ARG;
    if (a->bsize == 64 && !a->plan) return BSMM_ERR_UNSUPPORTED;      // bsize 64 runs through its plan only
    if ((rc = check_plan(false, a))) return rc;
    if (a->bsize == 64) return xprop64(fprop, X, W, Y, a);
    return with_dtype(a->dtype, [&](auto dt) {
        return by_shape(a, [&](auto bs, auto ax) { return xprop_typed<decltype(dt), decltype(bs)::value, decltype(ax)::value>(fprop, X, W, Y, a); });
    });
}
}  // namespace
