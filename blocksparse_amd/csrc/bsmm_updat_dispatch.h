// bsmm_updat_dispatch.h -- the weight gradient: the ONE decision of a call (updat_path), the workspace of each route (updat_route_bytes),
// the launchers and the call itself (updat_typed), the fp32 routes through bf16 pieces, bsize 64 on the quadrants (updat64).
#pragma once
#include "bsmm_dispatch.h"
#include "bsmm_updat.h"
#include "bsmm_updat_tr.h"
#include "bsmm_updat_win.h"
#include "bsmm_updat_v2.h"
#include "bsmm_updat16_rows.h"

namespace {
#ifndef UTS_NMAX
#define UTS_NMAX 768      // minibatch rows (x pairs) up to which the one-wave-per-block updat kernel takes the per-block calls (experiment switch: 0 = never)
#endif
#ifndef UAW_NMAX
#define UAW_NMAX 128              // bsize 32 / 16, feature axis 0, weight gradient: the one-wave-per-block kernel up to this many minibatch columns x pairs
#endif
#ifndef U8P_ON
#define U8P_ON 1                  // bsize 8, feature axis 0, weight gradient: the pair kernel (bsmm_updat.h) where the cost model picks it (0: never; measurement builds)
#endif
// internal to the library (never set by callers: bsmm_updat refuses a public call that carries it): the blocks of this bsize-32 call are the
// quadrants of 64 x 64 blocks and DW is the 64-layout (updat64)
constexpr int32_t FLAG_INTERNAL_Q64 = 1 << 30;

inline bool operands_aligned16(const PtrList8& xs, const PtrList8& es, int pcount) {
    bool ok = true;
    for (int p = 0; p < pcount; ++p) ok = ok && aligned16(xs.p[p]) && aligned16(es.p[p]);
    return ok;
}
inline const float* updat_gate(const bsmm_args* a) { return (a->flags & BSMM_FLAG_GATED_DW) ? a->gate : nullptr; }   // gated dw: per-block kernels, the streaming and the row-owner kernel

// workgroups per work item of the windowed kernels (each takes a slice of the minibatch): the caller's choice
// (bsmm_args.split), else enough to give every CU a workgroup while each keeps >= 8 chunks
inline int updat_split(const bsmm_args* a, int nitems, int nchunks) {
    if (a->split > 0) return std::min(a->split, std::max(1, nchunks));
    int split = 1;
    const int cus = device_cus();
    while (nitems * split < cus && split * 2 <= nchunks / 8 && split < 8) split *= 2;
    return split;
}

// Streaming kernel (bsmm_updat_v2.h, 'BSU2' plans).  Default grid: 8 x U workgroups (U = CUs / 8) in the XCD-aware schedule of
// the plan (plan_inner = NSETS | common set size << 8).  Every item is ONE workgroup's -- and is stored directly -- when the plan
// has 8 sets of equal size that fill whole rounds of U; otherwise partial sums meet in the fp32 workspace.  The caller can ask
// for `split` workgroups per item instead (1: one per item, direct).
// partial-sum path of the streaming kernel: the workspace holds the fp32 sums [blocks][1024] (only written for
// BSMM_FLAG_DW_SUMS) and behind them one region of 64 accumulator slots x 4 KiB per (round, workgroup)
struct U2Launch { int grid; bool scratch; int flat; int rounds; int direct; };      // grid: the schedule's workgroups; direct: workgroups of the direct blocks behind them
// (+ 2 KiB: the fused data-parallel reduction reads / writes the sums in `world` 32-byte aligned shards, include/bsmm_dist.h)
inline size_t u2_sums_bytes(const bsmm_args* a) { return round16((size_t)a->blocks * 1024 * sizeof(float)) + 2048; }
inline size_t u2_region_bytes() { return (size_t)U2_WAVES * U2_SLOTS * 4096; }
// (a direct block's workgroup leaves ONE 4 KiB partial sum: packed behind the regions of the schedule's workgroups, 64 to a region's worth)
inline size_t u2_direct_bytes(int direct_wgs) { return (size_t)((direct_wgs + 63) / 64) * u2_region_bytes(); }
inline int u2_chunk(const bsmm_args* a) { return a->axis == 1 ? U2_CH : U2_CH0; }   // minibatch entries per chunk of the streaming kernel
inline U2Launch updat2_shape(const bsmm_args* a, bool gated) {
    const int cus = device_cus();
    const int nsets = u2_sets(a), longest = u2_longest_set(a), common = u2_sets_equal(a) ? longest : 0;
    U2Launch L;
    L.direct = u2_direct_blocks(a) * U2_DIRECT_PARTS;           // (their partial sums meet in the summing pass: such a plan always takes the scratch path)
    if (a->split >= 1) {
        const long nchunks = (long)a->pcount * ((a->N + u2_chunk(a) - 1) / u2_chunk(a));
        const long sp = std::max<long>(1, std::min<long>(a->split, nchunks));
        L.grid = (int)(a->plan_items * sp); L.scratch = sp > 1 || gated || L.direct > 0; L.flat = 1;
        L.rounds = (a->plan_items + L.grid - 1) / L.grid;
        return L;
    }
    const int U = std::max(1, cus / 8);
    L.grid = 8 * U; L.flat = 0;
    L.scratch = gated || L.direct > 0 || !(nsets == 8 && common > 0 && common % U == 0);
    L.rounds = (longest + U - 1) / U;
    return L;
}
// the streaming kernel's workspace for a launch shape: the sums, the partial-sum regions, the direct blocks' (needed when L.scratch)
inline size_t u2_workspace_bytes(const bsmm_args* a, const U2Launch& L) {
    return u2_sums_bytes(a) + (size_t)L.rounds * L.grid * u2_region_bytes() + u2_direct_bytes(L.direct);
}
// what bsmm_workspace_bytes answers for a streaming plan: it does not know the operands, so it sizes the launch as if it were gated and took
// the partial-sum path
inline size_t u2_query_bytes(const bsmm_args* a) { return u2_workspace_bytes(a, updat2_shape(a, true)); }

// the streaming launch of a call: the descriptor must be one of this kernel's, then the shape (0, or BSMM_ERR_ARG)
template <int AXIS>
int updat2_decide(const bsmm_args* a, bool gated, U2Launch* L) {
    if (a->plan_magic != U2PLAN_MAGIC || a->plan_waves != U2_WAVES || a->plan_items <= 0 || (a->plan_width != 16 && a->plan_width != 8 && !(a->plan_width == 32 && AXIS == 1))) return BSMM_ERR_ARG;
    *L = updat2_shape(a, gated);
    if (L->direct > 0 && AXIS != 1) return BSMM_ERR_ARG;         // (the builder makes direct blocks for feature axis 1 only)
    // (raw sums: left by the summing pass; updat64: that pass writes the quadrants into their 64 x 64 blocks)
    if (a->flags & (BSMM_FLAG_DW_SUMS | FLAG_INTERNAL_Q64)) L->scratch = true;
    return 0;
}

// (the caller has decided L -- updat2_decide -- and checked the workspace against u2_workspace_bytes when L.scratch)
template <class DT, int AXIS>
int launch_updat2(const PtrList8& xs, const PtrList8& es, void* DW, const bsmm_args* a, const float* gate, const U2Launch& L) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const bool sums_only = (a->flags & BSMM_FLAG_DW_SUMS) != 0;
    const bool q64 = (a->flags & FLAG_INTERNAL_Q64) != 0;
    float* scratch = nullptr;      // the partial-sum regions
    float* sums = nullptr;
    if (L.scratch) {
        sums = static_cast<float*>(a->workspace);
        scratch = reinterpret_cast<float*>(static_cast<char*>(a->workspace) + u2_sums_bytes(a));
    }
    auto go = [&](auto ws_tag) -> int {      // window side of the plan's items
        constexpr int WS = decltype(ws_tag)::value;
        constexpr int LDS = AXIS == 1 ? u2_lds_bytes(WS) : u2_lds_bytes0(WS);
        if (int rc = ensure_lds<&updat32_a1_v2_kernel<DT, WS, AXIS>>(LDS)) return rc;
        updat32_a1_v2_kernel<DT, WS, AXIS><<<L.grid + L.direct, 64 * U2_WAVES, LDS, st>>>(xs, es, static_cast<T*>(DW), scratch, a->plan, a->N, a->C, a->K,
                                                                                  a->pcount, a->alpha, a->beta, L.flat, L.grid, L.rounds);
        return 0;
    };
    int rc = BSMM_ERR_ARG;
    if (a->plan_width == 32) { if constexpr (AXIS == 1) rc = go(std::integral_constant<int, 32>{}); }
    else if (a->plan_width == 16) rc = go(std::integral_constant<int, 16>{});
    else rc = go(std::integral_constant<int, 8>{});
    if (rc) return rc;
    if (scratch) {
        const int CPI = a->pcount * ((a->N + u2_chunk(a) - 1) / u2_chunk(a));
        const int32_t* bmap = a->plan + U2_HDR + (size_t)a->plan_items * U2_ITEM;     // behind the items (bsmm_plan.h)
        if (sums_only) updat2_reduce_kernel<DT, true><<<a->blocks, 128, 0, st>>>(scratch, nullptr, sums, a->plan, bmap, nullptr, L.rounds * L.grid, L.grid, L.flat, CPI, 1.f, 0.f);
        else           updat2_reduce_kernel<DT, false><<<a->blocks, 128, 0, st>>>(scratch, static_cast<T*>(DW), nullptr, a->plan, bmap, gate, L.rounds * L.grid, L.grid, L.flat, CPI, a->alpha, a->beta, q64 ? 1 : 0);
    }
    return (int)hipGetLastError();
}

// the bsize-32 streaming call over the super-blocks of a 'BSS8' updat plan: raw fp32 sums of the super-blocks at the start of the workspace
inline bsmm_args s8_updat_inner(const bsmm_args* a) {
    bsmm_args b = s8_inner(a, true);
    b.flags = BSMM_FLAG_DW_SUMS; b.split = 0; b.gate = nullptr; b.trace = nullptr;
    b.lut = a->plan ? a->plan + s8_off_lut32(a->plan_width) : nullptr;
    return b;
}

// Row-owner kernel for bsize 16 on feature axis 0 (bsmm_updat16_rows.h).  grid = items x split, part of the minibatch = linear id % split.
// split: the caller's (bsmm_args.split, at most U6_MAX_SPLIT), else the smallest power of two that gives every CU a workgroup.  Measured
// against the windowed kernel (scripts/gpu_updat16_rows_sweep.py, profiles/r05_updat16_rows_sweep.txt): the row-owner kernel wins once
// three quarters of the CUs get a workgroup and a workgroup keeps 8 chunks of 64 minibatch entries (16 when four or more parts leave
// their sums for the finalize pass) -- 17 to 43 % at 4096^2 / 8192^2, N >= 4096; otherwise 0: the call takes the windowed kernel
// (2048^2 has 16 windows of 512 x 512: never).  ONE rule for the dispatch and for bsmm_workspace_bytes (the sizing used to
// reserve the images and the pieces of the fp32 route -- several hundred MB -- for shapes the dispatch then sent to the per-block kernel,
// which needs no workspace).
constexpr int U6_MAX_SPLIT = 8;
inline int u6_split(const bsmm_args* a, int pcount) {
    const int nchunks = (a->N + 63) / 64, nitems = up_section(a->plan_waves);
    if (a->split > 0) return std::min(std::min(a->split, nchunks), U6_MAX_SPLIT);
    const int cus = device_cus();
    int split = 1;
    while (split < U6_MAX_SPLIT && nitems * split < cus) split *= 2;
    const bool pays = 4L * nitems * split >= 3L * cus && (long)pcount * nchunks / split >= (split >= 4 ? 16 : 8);
    if (!pays && call_variant(a) != 3) return 0;
    return std::max(1, std::min(split, nchunks));
}
inline bool u6_section_ok(const bsmm_args* a) { return up_section(a->plan_waves) > 0 && (up_section(a->plan_width) == 32 || up_section(a->plan_width) == 16); }
// bsize 16: `parts` fp32 images of the sums (the windowed kernel's split-minibatch path: one; the row-owner kernel: one per part of the minibatch)
inline size_t updat16_images_bytes(const bsmm_args* a, int parts) { return (size_t)parts * a->blocks * 256 * sizeof(float); }

// `split` from u6_split.  images: the fp32 call through six bf16 piece pairs (updat16_f32_rows below): `pcount` pairs in xs / es, the images there
// (always, also for one part), DW in fp32 with alpha / beta / gate by the finalize pass unless *skip_if (the non-finite flag of the split).
// Otherwise one fp32 image of the sums per part in the workspace (a gated call: always -- the finalize pass applies the gate).
template <class DT>
int launch_updat16_rows(const PtrList8& xs, const PtrList8& es, void* DW, const bsmm_args* a, int split, int pcount, float* images = nullptr,
                        const float* gate = nullptr, const int32_t* skip_if = nullptr) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const bool f32 = images != nullptr;
    const int32_t* sec = a->plan + a->plan_inner;
    const int nitems = up_section(a->plan_waves), wk = up_section(a->plan_width);
    const size_t nel = (size_t)a->blocks * 256;
    float* scratch = f32 ? images : ((split > 1 || gate) ? static_cast<float*>(a->workspace) : nullptr);
    trace(a, BSMM_K_UPDAT16_ROWS);
    // (split 1 / 2 / 4 / 8: rounds of 8 workgroups = 8 / split items x split parts, see the kernel's workgroup map)
    const bool pow2 = split == 1 || split == 2 || split == 4 || split == 8;
    const unsigned grid = pow2 ? 8u * (unsigned)((nitems + 8 / split - 1) / (8 / split)) : (unsigned)nitems * split;
    T* dw16 = f32 ? nullptr : static_cast<T*>(DW);
    if (wk == 32) {
        if (int rc = ensure_lds<&updat16_rows_kernel<DT, 32>>(U6Geom<32>::LDS)) return rc;
        updat16_rows_kernel<DT, 32><<<grid, 64 * U6_WAVES, U6Geom<32>::LDS, st>>>(xs, es, dw16, scratch, sec, a->N, a->C, a->K, pcount, a->alpha, a->beta, split, nel);
    } else {
        if (int rc = ensure_lds<&updat16_rows_kernel<DT, 16>>(U6Geom<16>::LDS)) return rc;
        updat16_rows_kernel<DT, 16><<<grid, 64 * U6_WAVES, U6Geom<16>::LDS, st>>>(xs, es, dw16, scratch, sec, a->N, a->C, a->K, pcount, a->alpha, a->beta, split, nel);
    }
    const unsigned fgrid = (unsigned)((nel / 4 + 255) / 256);
    if (f32)          updat16_rows_finalize_kernel<DTf32><<<fgrid, 256, 0, st>>>(scratch, static_cast<float*>(DW), nel, split, a->alpha, a->beta, gate, skip_if);
    else if (scratch) updat16_rows_finalize_kernel<DT><<<fgrid, 256, 0, st>>>(scratch, dw16, nel, split, a->alpha, a->beta, gate);
    return (int)hipGetLastError();
}

// ONE decision per call, as on the xprop half (xprop_route): which kernel, with the few numbers its launch needs.  Used for the workspace
// check (updat_route_bytes) and the launch (updat_typed); the fp32 part (f32_split_route) also answers bsmm_workspace_bytes.
enum URoute {
    UR_NONE,            // (f32_split_route: no fp32 split route applies)
    UR_VALU,            // V_FMA kernel, any shape
    UR_BLOCK,           // per block, four waves (updat32_kernel / updat16_kernel)
    UR_WAVE_A0,         // one wave per block, feature axis 0 (updat_a0_wave_kernel)
    UR_PAIRS8,          // bsize 8, feature axis 0: one wave per pair of blocks
    UR_ONE_WAVE_TR,     // bsize 32, feature axis 1: one wave per block, transposing reads
    UR_BLOCK_TR,        // LDS-DMA + transposing-read kernel, bsize 32 / 16 on feature axis 1
    UR_WIN16,           // bsize 16 windowed ('BSUP' items)
    UR_ROWS16,          // bsize 16 row owner ('BSU6' section)
    UR_STREAM,          // bsize 32 streaming ('BSU2')
    UR_SUPER8,          // bsize 8 through the streaming kernel over super-blocks ('BSS8')
    UR_F32_STREAM, UR_F32_SUPER8, UR_F32_WIN16, UR_F32_ROWS16,      // fp32 through six bf16 piece pairs on the kernel named
    UR_ERR_UNSUPPORTED, UR_ERR_ARG
};
struct UPath {
    URoute route;
    int split;          // UR_WIN16, UR_ROWS16, UR_F32_ROWS16: workgroups per item
    U2Launch u2;        // UR_STREAM, UR_SUPER8, UR_F32_STREAM, UR_F32_SUPER8: the streaming launch
};

// one-wave-per-block kernel (updat32_a1_small_kernel), us: hipGraph replays at 4096^2 20 %: 5.3 / 6.6 / 9.3 / 12.1 / 18.1 / 26.8 us at
// N = 64 / 128 / 256 / 384 / 512 / 768
inline double t_one_wave(const bsmm_args* a, long rows) {
    const double rounds_s = std::max(1.0, std::ceil(a->blocks / (20.0 * device_cus())));
    return 4.0 + rounds_s * (double)rows * (rows <= 384 ? 0.021 : 0.033);
}

// Non-finite activations in the fp32 split routes.  A finite x beyond the bf16 range still splits exactly
// (bsmm_xcols.h::split3), an Inf or NaN cannot: its products with the partner's three pieces come out as Inf or NaN as their signs fall,
// where the fp32 kernels -- and the reference's fp32 kernels -- give what IEEE gives for the unsplit product.  So the split kernels raise a
// flag (4 bytes behind the pieces in the workspace), the finalize pass leaves DW alone when it is set, and the per-block fp32 kernel of
// the shape -- always launched, the flag is its condition: ~2 us of empty workgroups on finite inputs -- then computes the call the way
// fp32 ran before round 4.  (A call that asks for the raw sums, BSMM_FLAG_DW_SUMS, gets the split path's sums as they are.)
constexpr size_t F32_SPLIT_FLAG_BYTES = 16;

// fp32 weight gradient on feature axis 1, bsize 32, with a streaming plan (round 4).  The per-block fp32 kernel gathers its fragments at a
// stride of C elements there (25 TF: 2.2 ms at the bench shape).  Instead: X and DY are split into three bf16 pieces each (exact:
// bsmm_xcols.h) and the SIX significant piece products  x3 y1, x2 y2, x1 y3, x2 y1, x1 y2, x1 y1  (smallest first; the other three are below
// 2^-26 of the product) go through the bf16 streaming kernel as six (x, dy) PAIRS of ONE launch -- its pair list is what the reference's
// Plist<T, 8> is (src/gpu_types.h:167-170) -- with fp32 sums, and the finalize pass writes the fp32 DW with alpha / beta / gate.  bf16 x bf16
// products are exact in fp32 and the accumulation is fp32: the result has the accuracy of an fp32 matrix-core product.
inline bool updat_f32_split_applies(const bsmm_args* a) {
    return a->dtype == BSMM_F32 && a->bsize == 32 && a->axis == 1 && a->plan && a->plan_magic == U2PLAN_MAGIC && a->pcount == 1 && a->split == 0 &&
           a->C % 32 == 0 && a->K % 32 == 0 && (long)a->N * std::max(a->C, a->K) < (1L << 30) && call_variant(a) != 1 && call_variant(a) != 2;
}
// The same for bsize 8 (either feature axis): the six piece products run as six pairs of the streaming launch over the 32x32 SUPER-blocks of
// the 'BSS8' plan (bsmm_super8.h), gather8_f32_kernel writes the present 8x8 parts in fp32.  (The V_FMA kernel it replaces: 5.9 / 2.0 ms on
// feature axis 1 / 0 at 4096^2, 10 %, N = 8192.)
inline bool updat8_f32_split_applies(const bsmm_args* a) {
    if (!(a->dtype == BSMM_F32 && a->bsize == 8 && a->plan && a->plan_magic == S8PLAN_MAGIC && a->plan_width > 0 && a->plan_items > 0)) return false;
    if (s8_nested_code(a) != 2) return false;                                           // the nested plan must be the streaming kernel's
    return a->pcount == 1 && a->split == 0 && !(a->flags & (BSMM_FLAG_GATED_DW | BSMM_FLAG_DW_SUMS)) && a->C % 32 == 0 && a->K % 32 == 0 &&
           !(a->axis == 0 && a->N % 8 != 0) && (long)a->N * std::max(a->C, a->K) < (1L << 30) && call_variant(a) != 1 && call_variant(a) != 2;
}
// ... and for bsize 16 on feature axis 1 on the windowed kernel: six pairs of one launch, raw fp32 sums by its scratch path, fp32 finalize:
// 1.44 -> 1.12 ms at 4096^2, 10 %, N = 8192.  (Feature axis 0 measured too: 1.05 ms against 1.01 for the per-block fp32 kernel, whose
// fragments are contiguous there -- not taken.)
inline bool updat16_f32_split_applies(const bsmm_args* a) {
    return a->dtype == BSMM_F32 && a->bsize == 16 && a->axis == 1 && a->plan && a->plan_magic == UPLAN_MAGIC && up_base(a->plan_width) == UW16 && up_base(a->plan_waves) == UP_WAVES &&
           a->plan_items > 0 && a->pcount == 1 && a->split == 0 && !(a->flags & BSMM_FLAG_DW_SUMS) && a->C % 16 == 0 && a->K % 16 == 0 &&
           !(a->axis == 0 && a->N % 8 != 0) && call_variant(a) != 1 && call_variant(a) != 2;
}
// ... and on feature axis 0 (round 5) the six pairs go through the row-owner kernel (bsmm_updat16_rows.h) where it pays (u6_split) -- its
// images take the place of the sums.  Short minibatches, few windows: the per-block fp32 kernel, as before.
inline bool updat16_f32_rows_applies(const bsmm_args* a) {
    return a->dtype == BSMM_F32 && a->bsize == 16 && a->axis == 0 && a->plan && a->plan_magic == UPLAN_MAGIC && up_base(a->plan_width) == UW16 && up_base(a->plan_waves) == UP_WAVES &&
           a->plan_inner > 0 && a->pcount == 1 && !(a->flags & BSMM_FLAG_DW_SUMS) && a->N % 8 == 0 && (long)a->N * std::max(a->C, a->K) < (1L << 31) &&
           call_variant(a) != 1 && call_variant(a) != 2;
}
inline bool updat16_f32_rows_taken(const bsmm_args* a) {
    return updat16_f32_rows_applies(a) && (call_variant(a) == 3 || (a->N >= 256 && u6_split(a, 6) > 0));
}
// Which fp32 split route a call with a plan takes; UR_NONE: the kernels without a plan.  Needs no operand pointer, so bsmm_workspace_bytes asks
// it too -- with `any_n`, because it has always reserved for the three routes of the first rule whatever the minibatch.
inline URoute f32_split_route(const bsmm_args* a, bool any_n = false) {
    // (minibatches of a few rows: two split launches + a six-pair stream cost more than the per-block kernel)
    const bool long_n = any_n || a->N >= 256 || call_variant(a) == 3;
    if (updat_f32_split_applies(a) && (long_n || (a->flags & BSMM_FLAG_DW_SUMS))) return UR_F32_STREAM;
    if (updat8_f32_split_applies(a) && long_n) return UR_F32_SUPER8;
    if (updat16_f32_split_applies(a) && long_n) return UR_F32_WIN16;
    if (updat16_f32_rows_taken(a)) return UR_F32_ROWS16;
    return UR_NONE;
}
// the 16-bit streaming call behind UR_F32_STREAM / UR_F32_SUPER8: six pairs, raw sums at the start of the workspace
inline bsmm_args f32_stream_inner(const bsmm_args* a, URoute r) {
    bsmm_args b = *a;
    if (r == UR_F32_SUPER8) b = s8_updat_inner(a);
    b.dtype = BSMM_BF16; b.pcount = 6; b.flags = BSMM_FLAG_DW_SUMS; b.split = 0; b.gate = nullptr; b.trace = nullptr;
    return b;
}
// Workspace of an fp32 split route: [head: what the 16-bit launch behind the route needs][pieces of X: 3 N C bf16][pieces of DY: 3 N K bf16]
// [the non-finite flag].  head: the streaming call's workspace as bsmm_workspace_bytes sizes it / the windowed kernel's fp32 sums / the
// row-owner kernel's U6_MAX_SPLIT images.
struct F32Split {
    size_t head, nx, ne;
    size_t bytes() const { return head + 6 * (nx + ne) + F32_SPLIT_FLAG_BYTES; }
    uint16_t* xp(void* ws) const { return reinterpret_cast<uint16_t*>(static_cast<char*>(ws) + head); }
    uint16_t* ep(void* ws) const { return xp(ws) + 3 * nx; }
    int32_t* flag(void* ws) const { return reinterpret_cast<int32_t*>(ep(ws) + 3 * ne); }
};
inline F32Split f32_split_layout(const bsmm_args* a, URoute r) {
    F32Split s = {0, (size_t)a->N * a->C, (size_t)a->N * a->K};
    if (r == UR_F32_STREAM || r == UR_F32_SUPER8) { const bsmm_args b = f32_stream_inner(a, r); s.head = round16(u2_query_bytes(&b)); }
    else s.head = round16(updat16_images_bytes(a, r == UR_F32_ROWS16 ? U6_MAX_SPLIT : 1));
    return s;
}
// shared start of the four routes: flag cleared, X and DY split into the workspace, the six piece pairs listed
struct F32Pieces { PtrList8 xs, es; const int32_t* flag; };
inline int f32_split_prologue(const F32Split& s, const PtrList8& x, const PtrList8& e, const void* DW, const bsmm_args* a, F32Pieces& pc) {
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    if (!aligned16(x.p[0]) || !aligned16(e.p[0]) || !aligned16(DW)) return BSMM_ERR_ARG;
    uint16_t* xp = s.xp(a->workspace);
    uint16_t* ep = s.ep(a->workspace);
    int32_t* flag = s.flag(a->workspace);
    if (hipError_t err = hipMemsetAsync(flag, 0, F32_SPLIT_FLAG_BYTES, st); err != hipSuccess) return (int)err;
    split3_x_kernel<<<(unsigned)((s.nx / 8 + 255) / 256), 256, 0, st>>>(static_cast<const float*>(x.p[0]), xp, s.nx, flag);
    split3_x_kernel<<<(unsigned)((s.ne / 8 + 255) / 256), 256, 0, st>>>(static_cast<const float*>(e.p[0]), ep, s.ne, flag);
    static const int xi[6] = {2, 1, 0, 1, 0, 0}, ei[6] = {0, 1, 2, 0, 1, 0};      // piece indices of the six products, smallest first
    for (int p = 0; p < 8; ++p) {
        pc.xs.p[p] = p < 6 ? xp + xi[p] * s.nx : nullptr;
        pc.es.p[p] = p < 6 ? ep + ei[p] * s.ne : nullptr;
    }
    pc.flag = flag;
    return 0;
}
template <int BS, int AXIS>
int f32_split_repair(const PtrList8& xs, const PtrList8& es, void* DW, const bsmm_args* a, const int32_t* flag) {
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const float* ug = updat_gate(a);
    const int grid = 8 * ((a->blocks + 7) / 8);
    if constexpr (BS == 32)
        updat32_kernel<DTf32, AXIS><<<grid, 256, 0, st>>>(xs, es, static_cast<float*>(DW), a->lut, a->blocks, a->N, a->C, a->K, 1, a->alpha, a->beta, ug, flag);
    else if constexpr (BS == 16)
        updat16_kernel<DTf32, AXIS><<<grid, 256, 0, st>>>(xs, es, static_cast<float*>(DW), a->lut, a->blocks, a->N, a->C, a->K, 1, a->alpha, a->beta, ug, flag);
    else
        updat_valu_kernel<DTf32, BS, AXIS><<<a->blocks, 256, 0, st>>>(xs, es, static_cast<float*>(DW), a->lut, a->blocks, a->N, a->C, a->K, 1, a->alpha, a->beta, ug, flag);
    return (int)hipGetLastError();
}

// The four routes behind their prologue (pc: the piece pairs and the flag; x, e: the caller's fp32 pair for the repair pass).
int updat32_f32_split(const UPath& u, const F32Pieces& pc, const PtrList8& x, const PtrList8& e, void* DW, const bsmm_args* a) {
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const bsmm_args b = f32_stream_inner(a, u.route);
    if (int rc = launch_updat2<DTbf16, 1>(pc.xs, pc.es, nullptr, &b, nullptr, u.u2)) return rc;
    trace(a, BSMM_K_UPDAT_STREAM);
    if (a->flags & BSMM_FLAG_DW_SUMS) return (int)hipGetLastError();      // the raw fp32 sums stay at the start of the workspace, as for the 16-bit types
    const size_t nel = (size_t)a->blocks * 1024;
    updat_finalize_gated_kernel<DTf32><<<(unsigned)((nel / 4 + 255) / 256), 256, 0, st>>>(static_cast<const float*>(a->workspace), static_cast<float*>(DW), nel, 1024,
                                                                                         a->alpha, a->beta, updat_gate(a), pc.flag);
    return f32_split_repair<32, 1>(x, e, DW, a, pc.flag);
}
template <int AXIS>
int updat8_f32_split(const UPath& u, const F32Pieces& pc, const PtrList8& x, const PtrList8& e, void* DW, const bsmm_args* a) {
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const bsmm_args b = f32_stream_inner(a, u.route);
    if (int rc = launch_updat2<DTbf16, AXIS>(pc.xs, pc.es, nullptr, &b, nullptr, u.u2)) return rc;
    trace(a, BSMM_K_UPDAT_SUPER8);
    gather8_f32_kernel<<<a->plan_width, 256, 0, st>>>(static_cast<const float*>(a->workspace), a->plan, static_cast<float*>(DW), a->alpha, a->beta, pc.flag);
    return f32_split_repair<8, AXIS>(x, e, DW, a, pc.flag);
}
template <int AXIS>
int updat16_f32_split(const UPath& u, const F32Pieces& pc, const PtrList8& x, const PtrList8& e, void* DW, const bsmm_args* a) {
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    float* sums = static_cast<float*>(a->workspace);
    const size_t nel = (size_t)a->blocks * 256;
    if (hipError_t err = hipMemsetAsync(sums, 0, nel * sizeof(float), st); err != hipSuccess) return (int)err;
    if (int rc = ensure_lds<&updat16_win_kernel<DTbf16, AXIS>>(2 * UWN_SLOT)) return rc;
    trace(a, BSMM_K_UPDAT16_WIN);
    updat16_win_kernel<DTbf16, AXIS><<<dim3(a->plan_items, u.split), 512, 2 * UWN_SLOT, st>>>(pc.xs, pc.es, nullptr, sums, a->plan, a->N, a->C, a->K, 6, 1.f, 0.f);
    updat_finalize_gated_kernel<DTf32><<<(unsigned)((nel / 4 + 255) / 256), 256, 0, st>>>(sums, static_cast<float*>(DW), nel, 256, a->alpha, a->beta, updat_gate(a), pc.flag);
    return f32_split_repair<16, AXIS>(x, e, DW, a, pc.flag);
}
int updat16_f32_rows(const UPath& u, const F32Pieces& pc, const PtrList8& x, const PtrList8& e, void* DW, const bsmm_args* a) {
    if (int rc = launch_updat16_rows<DTbf16>(pc.xs, pc.es, DW, a, u.split, 6, static_cast<float*>(a->workspace), updat_gate(a), pc.flag)) return rc;
    return f32_split_repair<16, 0>(x, e, DW, a, pc.flag);
}
template <int BS, int AXIS>
int updat_f32_split(const UPath& u, const PtrList8& x, const PtrList8& e, void* DW, const bsmm_args* a) {
    F32Pieces pc;
    if (int rc = f32_split_prologue(f32_split_layout(a, u.route), x, e, DW, a, pc)) return rc;
    if constexpr (BS == 32 && AXIS == 1) return updat32_f32_split(u, pc, x, e, DW, a);
    if constexpr (BS == 8) return updat8_f32_split<AXIS>(u, pc, x, e, DW, a);
    if constexpr (BS == 16 && AXIS == 1) return updat16_f32_split<1>(u, pc, x, e, DW, a);
    if constexpr (BS == 16 && AXIS == 0) return updat16_f32_rows(u, pc, x, e, DW, a);
    return BSMM_ERR_UNSUPPORTED;
}

template <class DT, int BS, int AXIS>
UPath updat_path(const PtrList8& xs, const PtrList8& es, const void* DW, const bsmm_args* a) {
    UPath u = {UR_VALU, 0, {0, false, 0, 0, 0}};
    auto take = [&u](URoute r) { u.route = r; return u; };
    const int N = a->N;
    const long rows = (long)N * a->pcount;
    const int variant = call_variant(a);
    const bool sums_only = (a->flags & BSMM_FLAG_DW_SUMS) != 0;     // only the streaming kernel can leave raw sums
    const bool q64 = (a->flags & FLAG_INTERNAL_Q64) != 0;
    const bool gated = updat_gate(a) != nullptr;
    if constexpr (!DT::is16) {
        // fp32 with a plan: the bf16-split route where one applies, else the kernels without a plan (none of them reads the plan)
        const URoute r = a->plan ? f32_split_route(a) : UR_NONE;
        if (r == UR_F32_STREAM || r == UR_F32_SUPER8) {
            const bsmm_args b = f32_stream_inner(a, r);
            if (updat2_decide<AXIS>(&b, false, &u.u2)) return take(UR_ERR_ARG);
        }
        if (r == UR_F32_WIN16) u.split = updat_split(a, a->plan_items, (N + 63) / 64);
        if (r == UR_F32_ROWS16) {
            if (!u6_section_ok(a)) return take(UR_ERR_ARG);
            u.split = u6_split(a, 6);
        }
        if (r != UR_NONE) return take(r);
    }
    if (sums_only && !(BS == 32 && DT::is16 && a->plan && a->plan_magic == U2PLAN_MAGIC)) return take(UR_ERR_UNSUPPORTED);
    for (int p = 0; p < a->pcount; ++p)
        if (!xs.p[p] || !es.p[p]) return take(UR_ERR_ARG);
    // every operand pointer 16-byte aligned; on feature axis 0 16-byte row loads also need every row start aligned
    const bool ptr_ok = aligned16(DW) && operands_aligned16(xs, es, a->pcount);
    const bool vec_ok = AXIS == 0 ? ptr_ok && N % (DT::is16 ? 8 : 4) == 0 : aligned16(DW);
    const bool al = ptr_ok && (AXIS == 1 || N % 8 == 0);            // (the 16-bit kernels below: operand base pointers, on feature axis 0 16-byte row pieces)
    const bool use_valu = (BS == 8) || variant == 1 || !vec_ok;
    const bool planned = variant == 0 || variant == 3;
    if constexpr (BS == 8 && DT::is16 && AXIS == 0) {
        // short minibatches (round 6, scripts/gpu_a0_updat8_sweep.py): one wave per pair of blocks, operand fragments straight from global memory
        // (hipGraph replays, us: the pair kernel costs 6 + 3.4e-6 per (block, minibatch column); the super-block path about 30 + (0.0022 + 2e-6 N) per
        //  super-block -- hidden 2560 dense N = 64: 29 against 41; 20480 at 1.4 %: 26.5 against 228 at N = 64, 333 against 724 at N = 1024; 4096 at 10 %:
        //  9.4 against 45.5 at N = 64, 94 against 66 at N = 1024.  Without a plan the alternative is the V_FMA kernel: always the pair kernel)
        const bool s8 = a->plan != nullptr && a->plan_magic == S8PLAN_MAGIC && a->plan_width > 0;
        const double t_pair = 6.0 + 3.4e-6 * (double)a->blocks * N * a->pcount;
        const double t_s8 = 30.0 + (double)a->plan_width * (0.0022 + 2e-6 * (double)N * a->pcount);
        if (al && variant == 0 && a->split == 0 && !sums_only && (!s8 || t_pair < t_s8) && U8P_ON) return take(UR_PAIRS8);
    }
    if constexpr (BS == 8 && DT::is16) {
        // bsize 8 on the matrix cores: fp32 sums of whole 32x32 super-blocks ('BSS8' plan) into the workspace, then the
        // present 8x8 parts get alpha / beta and are rounded once
        // (operands the streaming kernel's 32-bit byte offsets cannot address fall through to the generic kernels below: ADVICE r3)
        const bool s8_big = (long)N * std::max(a->C, a->K) >= (1L << 30);
        if (a->plan != nullptr && a->plan_magic == S8PLAN_MAGIC && a->plan_width > 0 && a->plan_items > 0 && !gated && al && a->C % 32 == 0 && a->K % 32 == 0 && planned &&
            !(s8_inner(a, true).plan_magic == U2PLAN_MAGIC && s8_big)) {
            const bsmm_args b = s8_updat_inner(a);
            if (b.plan_magic != U2PLAN_MAGIC) return take(UR_ERR_ARG);      // (the nested plan is the streaming kernel's since round 3)
            if (updat2_decide<AXIS>(&b, false, &u.u2)) return take(UR_ERR_ARG);
            return take(UR_SUPER8);
        }
    }
    if constexpr (BS == 32 && DT::is16) {
        // streaming kernel ('BSU2' plan): 32-bit byte offsets inside an operand
        if (!use_valu && al && planned && a->plan != nullptr && a->plan_magic == U2PLAN_MAGIC && (long)N * std::max(a->C, a->K) < (1L << 30)) {
            bool stream = true;
            if (variant == 0 && AXIS == 0 && a->split == 0 && !sums_only && !q64) {
                // feature axis 0 (round 6; scripts/gpu_a0_updat_sweep.py, hipGraph replays): the per-block kernel costs 7 + 1.37e-5 us per (block,
                // minibatch column) -- 12.8 against the streaming kernel's 33.9 us at the reference benchmark's hidden 2560 / N = 64, 12.8 against 46
                // at 20480 / 1.7 %.  It is taken while that stays under 45 us, and whenever the windows are nearly empty (< 8 blocks per item: the
                // streaming kernel then moves a 32 KiB window per chunk for a handful of blocks, 537 against 227 us at 20480 / 1.7 % / N = 2048)
                const double t_blk0 = 7.0 + 1.37e-5 * (double)a->blocks * N * a->pcount;
                if (a->blocks < 8L * a->plan_items || t_blk0 < 45.0) stream = false;
            }
            if (variant == 0 && AXIS == 1) {
                // Fitted to scripts/gpu_updat_sweep.py (4096^2 20 % / 5 %, 8192^2 5 %, 2048^2 20 %, N = 128 .. 8192, us):
                // streaming kernel: 6 + 0.40 per 16-row chunk of a workgroup's share + 0.45 per MiB of partial sums (written by the
                // kernel, read back by the reduce pass; a block has nparts partial sums, times the slices of the last round);
                // per-block transposing-read kernel: 8 + rounds of 512 blocks * N * r, r = 0.004 while X and DY are small
                // (16 MiB), rising to 0.0105 at 128 MiB.
                const U2Launch L = updat2_shape(a, gated);
                const double chunks = (double)a->plan_items * a->pcount * ((N + 15) / 16);      // (the fit is per 16 minibatch entries)
                double t_stream = 6.0 + chunks / L.grid * 0.40;
                if (L.scratch && !L.flat) {
                    const int nsets = u2_sets(a), longest = u2_longest_set(a), U = std::max(1, L.grid / 8);
                    const int m_last = longest % U;
                    const double sliced = longest > 0 ? (double)m_last / longest : 0.0;
                    const double mult = (8.0 / std::max(1, nsets)) * ((1.0 - sliced) + sliced * (m_last > 0 ? std::min(U / m_last, U2_MAX_SLICES) : 1));
                    t_stream += 0.45 * mult * a->blocks * 4096.0 / 1048576.0;
                } else if (L.scratch) {
                    t_stream += 8.0;
                }
                const double rounds_b = std::max(1.0, std::ceil(a->blocks / (2.0 * device_cus())));
                const double foot = (double)N * a->pcount * (a->C + a->K) * 2.0 / 1048576.0;                 // MiB of X and DY
                const double rate = std::min(0.0105, std::max(0.004, 0.004 + 0.0065 * (foot - 16.0) / 112.0));
                double t_blk = 8.0 + rounds_b * (double)N * a->pcount * rate;
                // small minibatches: the one-wave-per-block kernel (t_one_wave) against 15.9 / 17.1 / 18.2 / 19.7 / 22.9 / 28.5 us for the kernel above
                if (rows <= UTS_NMAX) t_blk = std::min(t_blk, t_one_wave(a, rows));
                stream = t_stream <= t_blk || sums_only;
                // quadrants of 64 x 64 blocks: the streaming kernel, or (round 6) the one-wave-per-block kernel
                if (q64) stream = t_stream <= (rows <= UTS_NMAX ? t_one_wave(a, rows) : 1e30);
            }
            if (stream) return take(updat2_decide<AXIS>(a, gated, &u.u2) ? UR_ERR_ARG : UR_STREAM);
        }
        // (only the streaming kernel's summing pass leaves raw sums; the quadrant layout: that pass or the small-minibatch kernel below)
        if (sums_only || (q64 && !(AXIS == 1 && variant == 0 && rows <= UTS_NMAX))) return take(UR_ERR_UNSUPPORTED);
    }
    if constexpr (BS == 32 && AXIS == 1 && DT::is16) {
        // small minibatches: one wave per block, no reduction (gate in its epilogue)
        if (!use_valu && ptr_ok && variant != 1 && rows <= UTS_NMAX) return take(UR_ONE_WAVE_TR);
        if (q64) return take(UR_ERR_UNSUPPORTED);
        if (!use_valu && !gated && ptr_ok && variant != 1) return take(UR_BLOCK_TR);   // LDS-DMA + transposing-read kernel
    }
    if constexpr (BS == 16 && DT::is16) {
        // row-owner kernel ('BSU6' section, bsmm_updat16_rows.h): half the bytes per block of the windowed kernel, 64 (or fewer) work items --
        // taken when every workgroup gets enough chunks of 64 minibatch entries (u6_split)
        const bool rows_ok = AXIS == 0 && a->plan_inner > 0 && (long)N * std::max(a->C, a->K) < (1L << 31);
        const bool plan16 = !use_valu && al && planned && a->plan != nullptr;
        // a GATED call can take the row-owner kernel too (round 5: its finalize pass applies the gate); the windowed kernel has no gate
        if (plan16 && gated && rows_ok && a->plan_magic == UPLAN_MAGIC) {
            if (!u6_section_ok(a)) return take(UR_ERR_ARG);
            if ((u.split = u6_split(a, a->pcount)) > 0) return take(UR_ROWS16);
        }
        bool blk16 = false;
        if constexpr (AXIS == 0) {
            // (round 6, the same sweep: the per-block kernel costs 7 + 6.6e-6 us per (block, minibatch column); the windowed kernel about 5 + 0.03 per
            //  window + 1.1e-4 per (window, column).  Nearly empty windows -- the reference benchmark's sparse shapes: 73 against 18.6 us at 20480 /
            //  1.5 % / N = 64 -- always take the per-block kernel)
            if (variant == 0 && a->split == 0 && a->plan != nullptr && a->plan_items > 0) {      // (a caller who names a split wants the plan kernels)
                const double t_blk0 = 7.0 + 6.6e-6 * (double)a->blocks * N * a->pcount;
                const double t_win0 = 5.0 + 0.03 * a->plan_items + 1.1e-4 * (double)a->plan_items * N * a->pcount;
                blk16 = a->blocks < 8L * a->plan_items || t_blk0 < 0.6 * t_win0;
            }
        }
        if (plan16 && !gated && !blk16 && a->plan_items > 0) {   // windowed, 16x16 blocks
            if (a->plan_magic != UPLAN_MAGIC || up_base(a->plan_width) != UW16 || up_base(a->plan_waves) != UP_WAVES) return take(UR_ERR_ARG);
            if (rows_ok) {
                if (!u6_section_ok(a)) return take(UR_ERR_ARG);
                if ((u.split = u6_split(a, a->pcount)) > 0) return take(UR_ROWS16);
            }
            u.split = updat_split(a, a->plan_items, (N + 63) / 64);
            return take(UR_WIN16);
        }
    }
    if constexpr (BS == 16 && AXIS == 1 && DT::is16) {
        if (!use_valu && !gated && ptr_ok && variant != 1) return take(UR_BLOCK_TR);   // LDS-DMA + transposing-read kernel, 16x16 blocks
    }
    if constexpr ((BS == 32 || BS == 16) && AXIS == 0 && DT::is16) {
        // a few dozen minibatch columns (round 6): one wave per block, fragments straight from global memory (bsmm_updat.h::updat_a0_wave_kernel)
        // (hipGraph replays at the reference benchmark's shapes, N = 64: bsize 32 10.6 against 12.6 us, bsize 16 15 - 16 against 17 - 19; from 128 columns
        //  on the four-wave kernels below are as fast or faster at bsize 32)
        if (!use_valu && al && variant == 0 && a->split == 0 && rows <= (BS == 32 ? UAW_NMAX / 2 : UAW_NMAX)) return take(UR_WAVE_A0);
    }
    return take(use_valu ? UR_VALU : UR_BLOCK);
}

// workspace of the route a call takes (0: none), checked once before its launch
inline size_t updat_route_bytes(const UPath& u, const bsmm_args* a) {
    switch (u.route) {
        case UR_STREAM: return u.u2.scratch ? u2_workspace_bytes(a, u.u2) : 0;
        case UR_SUPER8: { const bsmm_args b = s8_updat_inner(a); return u2_workspace_bytes(&b, u.u2); }
        case UR_ROWS16: return (u.split > 1 || updat_gate(a)) ? updat16_images_bytes(a, u.split) : 0;
        case UR_WIN16:  return u.split > 1 ? updat16_images_bytes(a, 1) : 0;
        case UR_F32_STREAM: case UR_F32_SUPER8: case UR_F32_WIN16: case UR_F32_ROWS16: return f32_split_layout(a, u.route).bytes();
        default: return 0;
    }
}

template <class DT, int BS, int AXIS>
int updat_typed(const PtrList8& xs, const PtrList8& es, void* DW, const bsmm_args* a) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const UPath u = updat_path<DT, BS, AXIS>(xs, es, DW, a);
    if (u.route == UR_ERR_ARG) return BSMM_ERR_ARG;
    if (u.route == UR_ERR_UNSUPPORTED) return BSMM_ERR_UNSUPPORTED;
    if (!workspace_ok(a, updat_route_bytes(u, a))) {
        if (u.route == UR_WIN16) trace(a, BSMM_K_UPDAT16_WIN);      // (this route has always named itself before it looked at the workspace)
        return BSMM_ERR_WORKSPACE;
    }
    const int N = a->N;
    const float* ug = updat_gate(a);
    T* dw = static_cast<T*>(DW);
    const int q64 = (a->flags & FLAG_INTERNAL_Q64) ? 1 : 0;
    const int grid8 = 8 * ((a->blocks + 7) / 8);
    switch (u.route) {
        case UR_F32_STREAM: case UR_F32_SUPER8: case UR_F32_WIN16: case UR_F32_ROWS16:
            if constexpr (!DT::is16) return updat_f32_split<BS, AXIS>(u, xs, es, DW, a);
            break;
        case UR_PAIRS8:
            if constexpr (BS == 8 && DT::is16 && AXIS == 0) {
                trace(a, BSMM_K_UPDAT_BLOCK);
                const int pairs = (a->blocks + 1) / 2;
                updat8_a0_pairs_kernel<DT><<<(pairs + 3) / 4, 256, 0, st>>>(xs, es, dw, a->lut, a->blocks, N, a->pcount, a->alpha, a->beta, ug);
                return (int)hipGetLastError();
            }
            break;
        case UR_SUPER8:
            if constexpr (BS == 8 && DT::is16) {
                const bsmm_args b = s8_updat_inner(a);
                if (int rc = launch_updat2<DT, AXIS>(xs, es, nullptr, &b, nullptr, u.u2)) return rc;
                trace(a, BSMM_K_UPDAT_SUPER8);
                gather8_kernel<DT><<<a->plan_width, 256, 0, st>>>(static_cast<const float*>(a->workspace), a->plan, dw, a->alpha, a->beta);
                return (int)hipGetLastError();
            }
            break;
        case UR_STREAM:
            if constexpr (BS == 32 && DT::is16) {
                trace(a, BSMM_K_UPDAT_STREAM);
                return launch_updat2<DT, AXIS>(xs, es, DW, a, ug, u.u2);
            }
            break;
        case UR_ONE_WAVE_TR:
            if constexpr (BS == 32 && AXIS == 1 && DT::is16) {
                if (int rc = ensure_lds<&updat32_a1_small_kernel<DT>>(UTS_LDS)) return rc;
                trace(a, BSMM_K_UPDAT_BLOCK_TR | (BSMM_KV_ONE_WAVE << 8));
                const int grid = 8 * (((a->blocks + 3) / 4 + 7) / 8);
                updat32_a1_small_kernel<DT><<<grid, 256, UTS_LDS, st>>>(xs, es, dw, a->lut, a->blocks, N, a->C, a->K, a->pcount, a->alpha, a->beta, ug, q64);
                return (int)hipGetLastError();
            }
            break;
        case UR_BLOCK_TR:
            if constexpr (BS == 32 && AXIS == 1 && DT::is16) {
                if (int rc = ensure_lds<&updat32_a1_tr_kernel<DT>>(UT_LDS)) return rc;
                trace(a, BSMM_K_UPDAT_BLOCK_TR);
                updat32_a1_tr_kernel<DT><<<grid8, 256, UT_LDS, st>>>(xs, es, dw, a->lut, a->blocks, N, a->C, a->K, a->pcount, a->alpha, a->beta);
                return (int)hipGetLastError();
            }
            if constexpr (BS == 16 && AXIS == 1 && DT::is16) {
                if (int rc = ensure_lds<&updat16_a1_tr_kernel<DT>>(UT16_LDS)) return rc;
                trace(a, BSMM_K_UPDAT_BLOCK_TR);
                updat16_a1_tr_kernel<DT><<<grid8, 256, UT16_LDS, st>>>(xs, es, dw, a->lut, a->blocks, N, a->C, a->K, a->pcount, a->alpha, a->beta);
                return (int)hipGetLastError();
            }
            break;
        case UR_ROWS16:
            if constexpr (BS == 16 && AXIS == 0 && DT::is16) return launch_updat16_rows<DT>(xs, es, DW, a, u.split, a->pcount, nullptr, ug);
            break;
        case UR_WIN16:
            if constexpr (BS == 16 && DT::is16) {
                if (int rc = ensure_lds<&updat16_win_kernel<DT, AXIS>>(2 * UWN_SLOT)) return rc;
                trace(a, BSMM_K_UPDAT16_WIN);
                float* scratch = nullptr;
                const size_t nel = (size_t)a->blocks * 256;
                if (u.split > 1) {
                    scratch = static_cast<float*>(a->workspace);
                    hipError_t e = hipMemsetAsync(scratch, 0, nel * sizeof(float), st);
                    if (e != hipSuccess) return (int)e;
                }
                updat16_win_kernel<DT, AXIS><<<dim3(a->plan_items, u.split), 512, 2 * UWN_SLOT, st>>>(xs, es, dw, scratch, a->plan, N, a->C, a->K, a->pcount, a->alpha, a->beta);
                if (u.split > 1)
                    updat_finalize_kernel<DT><<<(unsigned)((nel / 4 + 255) / 256), 256, 0, st>>>(scratch, dw, nel, a->alpha, a->beta);
                return (int)hipGetLastError();
            }
            break;
        case UR_WAVE_A0:
            if constexpr ((BS == 32 || BS == 16) && AXIS == 0 && DT::is16) {
                trace(a, BSMM_K_UPDAT_BLOCK);
                updat_a0_wave_kernel<DT, BS><<<(a->blocks + 3) / 4, 256, 0, st>>>(xs, es, dw, a->lut, a->blocks, N, a->pcount, a->alpha, a->beta, ug);
                return (int)hipGetLastError();
            }
            break;
        case UR_BLOCK:
            trace(a, BSMM_K_UPDAT_BLOCK);
            if constexpr (BS == 32)      updat32_kernel<DT, AXIS><<<grid8, 256, 0, st>>>(xs, es, dw, a->lut, a->blocks, N, a->C, a->K, a->pcount, a->alpha, a->beta, ug);
            else if constexpr (BS == 16) updat16_kernel<DT, AXIS><<<grid8, 256, 0, st>>>(xs, es, dw, a->lut, a->blocks, N, a->C, a->K, a->pcount, a->alpha, a->beta, ug);
            return (int)hipGetLastError();
        case UR_VALU:
            trace(a, BSMM_K_UPDAT_VALU);
            updat_valu_kernel<DT, BS, AXIS><<<a->blocks, 256, 0, st>>>(xs, es, dw, a->lut, a->blocks, N, a->C, a->K, a->pcount, a->alpha, a->beta, ug);
            return (int)hipGetLastError();
        default: break;
    }
    return BSMM_ERR_UNSUPPORTED;
}

// the internal entry: validated arguments in (bsmm_updat; updat64 for its quadrant call), return code out
int updat(const void* const* X, const void* const* DY, void* DW, const bsmm_args* a) {
    PtrList8 xs, es;
    for (int p = 0; p < 8; ++p) {
        xs.p[p] = p < a->pcount ? X[p] : nullptr;
        es.p[p] = p < a->pcount ? DY[p] : nullptr;
    }
    return with_dtype(a->dtype, [&](auto dt) {
        return by_shape(a, [&](auto bs, auto ax) { return updat_typed<decltype(dt), decltype(bs)::value, decltype(ax)::value>(xs, es, DW, a); });
    });
}

int updat64(const void* const* X, const void* const* DY, void* DW, const bsmm_args* a) {
    // the streaming bsize-32 kernel on the quadrants.  16-bit types with the streaming plan only (what the reference runs bsize 64 in: fp16
    // tensor cores).
    if (!a->plan) return BSMM_ERR_UNSUPPORTED;
    bsmm_args b = b64_inner(a, true);
    if (a->dtype == BSMM_F32 || b.plan_magic != U2PLAN_MAGIC) return BSMM_ERR_UNSUPPORTED;
    const bool sums_only = (a->flags & BSMM_FLAG_DW_SUMS) != 0;
    if (sums_only) return BSMM_ERR_UNSUPPORTED;                  // (the raw sums of a bsize-64 call would be in quadrant order)
    // (round 5: the streaming kernel's summing pass writes every quadrant into its place in the 64 x 64 block with alpha / beta / the block's
    //  gate and ONE rounding -- the separate pass over the quadrant sums, b64_finalize_kernel: 20 us at the bench shape, is gone)
    b.flags = a->flags | FLAG_INTERNAL_Q64;
    b.gate = a->gate; b.alpha = a->alpha; b.beta = a->beta;
    b.workspace = a->workspace; b.workspace_bytes = a->workspace_bytes;
    if (!a->workspace || a->workspace_bytes < bsmm_workspace_bytes(BSMM_OP_UPDAT, &b)) return BSMM_ERR_WORKSPACE;
    if (int rc = check_plan(true, &b)) return rc;               // (the nested descriptor, as a public bsize-32 call's would be)
    return updat(X, DY, DW, &b);
}
}  // namespace
