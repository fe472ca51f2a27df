// bsmm_xcol_v2.h -- xprop kernel "wave owns an output column" with the WEIGHTS staged through LDS too ('BSX2' plans),
// feature_axis = 1, bsize 32, 16-bit storage types.
//
// What bounded bsmm_xcol.h (99 us per pass at the bench shape against ~22 us of matrix work): a wave fetched its weight
// fragments into registers with ordinary loads one step ahead, and the vector-memory counter is in order -- so the
// `s_waitcnt vmcnt(0)` in front of every step also waited for the activation slabs of the NEXT phase that had just been
// requested (16 drains per phase; a phase was one memory round trip long whatever the matrix work), and four register sets
// of fragments kept the kernel on the 128-register edge.  Here everything a phase needs comes by LDS-DMA, requested one
// whole phase ahead by whichever wave the plan names, and there is ONE wait per phase:
//   workgroup = 16 output blocks x 128 minibatch rows, 16 waves, wave v owns output block v (4 row tiles x 16 accumulators);
//   phase = up to 2 pair steps and up to X2_WCAP weight blocks (bsmm_plan.h); LDS = 2 halves x (2 activation slabs of
//   16 KiB + X2_WCAP weight blocks of 2 KiB) = 160 KiB;
//   per phase and wave: vmcnt(0) + barrier; 2 slab DMAs + <= 3 weight DMAs for the next phase; then for each of its <= 4
//   blocks 2 + 8 ds_read_b128 and 8 MFMAs.
//   activation slab: rows of 128 B, the eight 16-byte pieces of row r XOR-swizzled with (r >> 1) & 7;
//   weight block:   rows of 64 B, the four pieces of row r XOR-swizzled with (r >> 2) & 3 (both conflict-free for b128).
#pragma once
#include "bsmm_common.h"
#include "bsmm_plan.h"
#include "bsmm_xprop.h"      // XMap

namespace bsmm {

// measurement switches (ablation builds, scripts/build_variants.py): wrong results by construction
#ifndef X2_NO_XDMA
#define X2_NO_XDMA 0
#endif
#ifndef X2_NO_WDMA
#define X2_NO_WDMA 0
#endif
#ifndef X2_NO_READS
#define X2_NO_READS 0
#endif
#ifndef X2_NO_MFMA
#define X2_NO_MFMA 0
#endif
#ifndef X2_NO_EPILOGUE
#define X2_NO_EPILOGUE 0
#endif
constexpr int X2_R = 128;                          // minibatch rows per workgroup
constexpr int X2_SLAB = X2_R * 128;                // 16 KiB
constexpr int X2_LDS = 163840;                     // 160 KiB: two ring halves of 80 KiB = PH slabs + (WCAP + 1) weight slots (bsmm_plan.h)
static_assert(X2_R * X2_G * 64 <= X2_LDS && x2_wcap(2) == 23 && x2_wcap(3) == 15 && x2_wcap(4) == 7, "ring and epilogue tile must fit the LDS");

// TRANSW = true (fprop): Wsel is W in its natural [c-in-block][k-in-block] layout; the blocks are staged unswizzled and the
// fragment (8 consecutive c for one k per lane) is built with four transposing 8-byte reads -- no transposed copy of W, no
// pre-pass, no workspace.
// AXIS = 0: activations (C, N), minibatch contiguous: a slab is [64 feature rows] x [128 minibatch columns] (256 B per row,
// 16-byte pieces XOR-swizzled with 4 * (row & 3)), the B operand (8 consecutive FEATURES of one minibatch column per lane) is
// built with transposing reads as in xcol32_a0_kernel, output rows are features.  Requires N % 8 == 0.  Same plans.
// GATED: per-block fp32 gates (hgemm_blocksparse_*_sdd's `Gate`, src/blocksparse_hgemm_cn_64_op_gpu.cu:54-66,96-124).  The wave that
// requests a weight block also fetches its gate into the ring half's gate table; a block with gate 0 is skipped, otherwise
// g * w is formed in fp32 per fragment element and split into TWO 16-bit pieces (hi = round(g w), lo = round(g w - hi)) that are
// both multiplied: the product is exact to ~2^-17 instead of the 2^-9 of a single bf16 rounding of g * w (which measured
// 2.2e-3 against the oracle, above the 1e-3 bar) -- the reference applies the gate to the fp32 block product
// (blocksparse/matmul.py:367-373); twice the MFMAs and ~80 vector instructions per block, for gated calls only.
// PH = steps per phase (2, 3 or 4; the plan's choice): LDS half = PH slabs of 16 KiB + x2_wcap(PH) weight slots + the gate table.
template <class DT, bool TRANSW, int AXIS = 1, bool GATED = false, int PH = 2>
__global__ void __launch_bounds__(64 * X2_G, 4)
xcol32_v2_kernel(const typename DT::T* __restrict__ X, const typename DT::T* __restrict__ Wsel,
                    typename DT::T* __restrict__ Y, const int32_t* __restrict__ plan, XMap map, int N, int Cin, int Kout,
                    const float* __restrict__ gate = nullptr) {
    typedef typename DT::T T;
    static_assert(DT::is16 && PH >= 2 && PH <= 4, "xcol v2 kernel: 16-bit storage types, 2..4 steps per phase");
    constexpr int X2_XHALF = PH * X2_SLAB;                 // activation bytes per ring half
    constexpr int X2_WHALF = 81920 - X2_XHALF;             // weight bytes per ring half: the plan's slots + one for the gate table
    constexpr int X2_GTAB = x2_wcap(PH) * 2048;            // the gate table of a ring half: fp32 per slot (gated calls)
    constexpr int X2_WBASE = 2 * X2_XHALF;                 // weight ring behind the activation ring
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int tile, grp;
    if (!xmap_decode(map, blockIdx.x, tile, grp)) return;
    const int4 gh = *reinterpret_cast<const int4*>(plan + plan[5] + 4 * grp);
    const int ph_off = __builtin_amdgcn_readfirstlane(gh.x), nph = __builtin_amdgcn_readfirstlane(gh.y);
    const int ob0 = __builtin_amdgcn_readfirstlane(gh.z), nob = __builtin_amdgcn_readfirstlane(gh.w);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (spelled out: wave_id() changes this kernel's instruction order, profiles/device_prims_isa.md)
    const int32_t* pxt = plan + plan[6] + 2 * ph_off;                                                   // two words per phase
    const int4* tab = reinterpret_cast<const int4*>(plan + plan[7]) + ((size_t)ph_off * X2_G + wave) * 2;   // X2_ROW = 8 words
    const int r = lane & 31, h = lane >> 5;
    const int n_tile = tile * X2_R;
    const uint32_t base_addr = lds_addr_of(smem);
    const int npairs_full = Cin / 64;

    // activation DMA: a slab is 16 instructions of 1 KiB (8 rows of 128 B); wave v issues instruction v of each slab
    const unsigned char* xt = reinterpret_cast<const unsigned char*>(X);
    uint32_t xvoff, xvoff_tail;
    if constexpr (AXIS == 1) {
        const int row = 8 * wave + (lane >> 3);
        const int xr = min(n_tile + row, N - 1) - n_tile;            // rows past N are clamped (never stored)
        const int piece = (lane & 7) ^ ((row >> 1) & 7);
        xvoff = (uint32_t)xr * (uint32_t)Cin * 2u + piece * 16;
        xvoff_tail = xvoff - ((piece & 4) ? 64 : 0);                  // last pair of an odd block count: re-read its even half
    } else {
        // instruction v = slab rows 4v .. 4v+3 (256 B each): lane -> (row, stored piece lane & 15); columns past N are clamped
        const int row = 4 * wave + (lane >> 4);
        const int piece = (lane & 15) ^ (4 * (row & 3));
        const int col = min(n_tile + piece * 8, N - 8) - n_tile;
        xvoff = (uint32_t)row * (uint32_t)N * 2u + (uint32_t)col * 2u;
        xvoff_tail = (uint32_t)min(row, 31) * (uint32_t)N * 2u + (uint32_t)col * 2u;   // missing odd block: re-read row 31 of the even one
    }
    // per pair step the source moves by 128 B (axis 1: 64 features of a row) / by 64 rows of N elements (axis 0)
    const size_t xstep = AXIS == 1 ? (size_t)128 : (size_t)N * 128;
    const unsigned char* xtile = static_cast<const unsigned char*>(uniform_ptr(xt + (AXIS == 1 ? (size_t)n_tile * Cin * 2 : (size_t)n_tile * 2)));
    const unsigned char* wsel = static_cast<const unsigned char*>(uniform_ptr(Wsel));
    // weight DMA: lane i of an instruction writes piece i of a 1 KiB half block (rows 16*hb + (i >> 2)); it fetches the
    // piece that the swizzle puts there: (i & 3) ^ ((row >> 2) & 3) = (i & 3) ^ ((i >> 4) & 3)
    const uint32_t wvoff = TRANSW ? (uint32_t)lane * 16u : (uint32_t)((lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4));

    // fragment read offsets
    const int xsw = (r >> 1) & 7;
    uint32_t xrd[2][2];      // axis 1: [half][kk], inside a 32-row band of slab 0 of ring half 0
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) xrd[half][kk] = r * 128 + (((4 * half + 2 * kk + h) ^ xsw) << 4);
    // axis 0 (xcol32_a0_kernel): 16-lane group g16 -> minibatch columns 16 * (g16 & 1) .. of a 32-column tile, K half g16 >> 1;
    // lane t16 points at row (t16 >> 2) of a 4-row band, 8 bytes at column 4 * (t16 & 3)
    const int g16x = lane >> 4, t16x = lane & 15, trowx = t16x >> 2;
    const int tcolbx = (16 * (g16x & 1) + 4 * (t16x & 3)) * 2;
    uint32_t wrd[2];         // [kk], inside slot 0 of ring half 0
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        if constexpr (TRANSW) {   // rows 16kk + 8h + (t16 >> 2) (+4), 8 bytes at column 16 * (g16 & 1) + 4 * (t16 & 3)  (bsmm_updat_tr.h)
            const int g16 = lane >> 4, t16 = lane & 15;
            wrd[kk] = X2_WBASE + (16 * kk + 8 * h + (t16 >> 2)) * 64 + (16 * (g16 & 1) + 4 * (t16 & 3)) * 2;
        } else {
            wrd[kk] = X2_WBASE + r * 64 + (((2 * kk + h) ^ ((r >> 2) & 3)) << 4);
        }
    }

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) zero_tile(acc[t]);

    // gated calls: lanes 0..2 fetch the gates of my three duties (first half block of a block only) for ring half hb_; the
    // values are written into that half's gate table at the top of the next phase, behind the same wait as the DMAs
    float gpend = 0.f;
    uint32_t gaddr = X2_WBASE + X2_GTAB + 31 * 4;      // LDS address my pending gate goes to (slot 31: nobody's)
    auto fetch_gates = [&](int d0, int d1, int d2, int hbn) {
        if constexpr (GATED) {
            const int dsel = lane == 0 ? d0 : (lane == 1 ? d1 : d2);
            const bool valid = lane < 3 && dsel != -1 && !(dsel & 1);
            gpend = valid ? gate[(dsel & 0x3ffffff) >> 1] : 0.f;
            gaddr = X2_WBASE + hbn * X2_WHALF + X2_GTAB + (valid ? (((uint32_t)dsel >> 26) >> 1) : 31u) * 4;
        }
    };

    // DMAs of one phase into ring half `hb`: px = pair of step 0 | pair of step 1 << 16, d0..d2 = weight duties
#define X2_ISSUE(px_, pxb_, d0_, d1_, d2_, hb_)                                                                                   \
    do {                                                                                                                    \
        const uint32_t xdst = base_addr + (hb_) * X2_XHALF + wave * 1024;                                                   \
        const uint32_t wdst = base_addr + X2_WBASE + (hb_) * X2_WHALF;                                                      \
        _Pragma("unroll") for (int u_ = 0; u_ < PH; ++u_) {                                                                 \
            const int pu = (int)(((u_ < 2 ? (uint32_t)(px_) : (uint32_t)(pxb_)) >> (16 * (u_ & 1))) & 0xffffu);             \
            if (!X2_NO_XDMA && (u_ == 0 || pu != 0xffff))                                                                   \
                glds16_saddr(xtile + (size_t)pu * xstep, pu < npairs_full ? xvoff : xvoff_tail, xdst + u_ * X2_SLAB);       \
        }                                                                                                                   \
        if (X2_NO_WDMA) break;                                                                                              \
        if ((d0_) != -1) glds16_saddr(wsel + ((size_t)((d0_) & 0x3ffffff) << 10), wvoff, wdst + (((uint32_t)(d0_) >> 26) << 10)); \
        if ((d1_) != -1) glds16_saddr(wsel + ((size_t)((d1_) & 0x3ffffff) << 10), wvoff, wdst + (((uint32_t)(d1_) >> 26) << 10)); \
        if ((d2_) != -1) glds16_saddr(wsel + ((size_t)((d2_) & 0x3ffffff) << 10), wvoff, wdst + (((uint32_t)(d2_) >> 26) << 10)); \
    } while (0)

    // one block: weight fragment from its slot, the four row tiles' activation fragments, 8 MFMAs
    auto block = [&](uint32_t xoff, uint32_t wbase_half, uint32_t slot, int half) {
        if (X2_NO_READS) return;
        const uint32_t woff = wbase_half + (slot << 11);
        float g = 1.f;
        if constexpr (GATED) {
            g = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(*reinterpret_cast<const uint32_t*>(smem + X2_WBASE + wbase_half + X2_GTAB + slot * 4)));
            if (g == 0.f) return;
        }
        auto xread = [&](int t, int kk) -> uint4 {
            if constexpr (AXIS == 1) {
                return *reinterpret_cast<const uint4*>(smem + xrd[half][kk] + xoff + t * 4096);
            } else {
                // rows (features) 32 * half + 16 * kk + 8 * (g16 >> 1) + {0..3 | 4..7}; row & 3 == trow for both bands
                const int row0 = 32 * half + 16 * kk + 8 * (g16x >> 1) + trowx;
                const int byte = 64 * t + tcolbx;                             // byte inside the 256-byte row (before swizzle)
                const int sw = (((byte >> 4) ^ (4 * trowx)) << 4) | (byte & 15);
                const uint2 lo = ds_tr16(smem + xoff + row0 * 256 + sw), hi = ds_tr16(smem + xoff + (row0 + 4) * 256 + sw);
                return make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
        };
        uint4 wq[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if constexpr (TRANSW) wq[kk] = ds_tr16_frag(smem + wrd[kk] + woff, 64);
            else                  wq[kk] = *reinterpret_cast<const uint4*>(smem + wrd[kk] + woff);
        }
        if constexpr (GATED) {
            // one K half at a time (4 activation fragments live instead of 8: the split pieces need the registers)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                uint4 xg[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) xg[t] = xread(t, kk);
                uint4 whi = wq[kk], wlo = zero_u4();
                if (g != 1.f) {              // (gate 1 -- the usual value of a pruning mask -- needs no arithmetic: hi = w, lo = 0)
                    uint32_t hi[4], lo[4];
                    const uint32_t src[4] = {wq[kk].x, wq[kk].y, wq[kk].z, wq[kk].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float p0 = g * DT::to_f32((uint16_t)(src[e] & 0xffffu)), p1 = g * DT::to_f32((uint16_t)(src[e] >> 16));
                        const uint16_t h0 = DT::from_f32(p0), h1 = DT::from_f32(p1);
                        const uint16_t l0 = DT::from_f32(p0 - DT::to_f32(h0)), l1 = DT::from_f32(p1 - DT::to_f32(h1));
                        hi[e] = (uint32_t)h0 | ((uint32_t)h1 << 16);
                        lo[e] = (uint32_t)l0 | ((uint32_t)l1 << 16);
                    }
                    whi = make_uint4(hi[0], hi[1], hi[2], hi[3]); wlo = make_uint4(lo[0], lo[1], lo[2], lo[3]);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = DT::mfma32(whi, xg[t], acc[t]);
                if (g != 1.f) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = DT::mfma32(wlo, xg[t], acc[t]);
                }
            }
            return;
        }
        uint4 xf[4][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int t = 0; t < 4; ++t) xf[t][kk] = xread(t, kk);
        // (all ten fragment reads of a block forced in front of its first MFMA by a sched_barrier: 61.5 / 84.0 / 158.2 us, neutral --
        //  profiles/r02_xcol_v2_ablation.md)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (X2_NO_MFMA) asm volatile("" ::"v"(wq[kk].x), "v"(wq[kk].w), "v"(xf[t][kk].x), "v"(xf[t][kk].w));
                else acc[t] = DT::mfma32(wq[kk], xf[t][kk], acc[t]);
            }
    };

    if (nph > 0) {
        {   // prologue: phase 0 into ring half 0
            const int4 d = tab[0], e = tab[1];
            const int px0 = __builtin_amdgcn_readfirstlane(pxt[0]), px0b = __builtin_amdgcn_readfirstlane(pxt[1]);
            const int d0 = __builtin_amdgcn_readfirstlane(d.z), d1 = __builtin_amdgcn_readfirstlane(d.w), d2 = __builtin_amdgcn_readfirstlane(e.x);
            X2_ISSUE(px0, px0b, d0, d1, d2, 0);
            fetch_gates(d0, d1, d2, 0);
        }
        int hb = 0;
        for (int tb = 0; tb < nph; tb += 64) {       // lane-indexed tables for phases [tb, tb + 64)
            const int idx = min(tb + lane, nph - 1), idn = min(tb + lane + 1, nph - 1);
            const int4 cn = tab[(size_t)idx * X2_G * 2];
            int cwv = cn.x, cwv2 = cn.y;
            const int4 dn = tab[(size_t)idn * X2_G * 2], en = tab[(size_t)idn * X2_G * 2 + 1];
            int d0v = dn.z, d1v = dn.w, d2v = en.x, pxv = pxt[2 * idn], pxv2 = pxt[2 * idn + 1];
            // the table loads must have landed before the loop: a wait the compiler places INSIDE it would drain the DMA queue
            asm volatile("" : "+v"(cwv), "+v"(cwv2), "+v"(d0v), "+v"(d1v), "+v"(d2v), "+v"(pxv), "+v"(pxv2));
            const int tend = min(64, nph - tb);
            for (int qi = 0; qi < tend; ++qi) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // my DMA shares of this phase have landed
                if constexpr (GATED) {                               // ... and the gates I fetched with them: into this half's table
                    *reinterpret_cast<float*>(smem + gaddr) = gpend;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_s_barrier();                        // everyone's have; everyone left the previous phase
                // (odd waves requesting the next phase AFTER their blocks: 69.5 / 86.6 / 163.3 us, worse -- with a drain per phase the late
                //  requests lose half their time to land; profiles/r02_xcol_v2_ablation.md)
                if (tb + qi + 1 < nph) {
                    const int px1 = __builtin_amdgcn_readlane(pxv, qi), px1b = PH > 2 ? __builtin_amdgcn_readlane(pxv2, qi) : -1;
                    const int d0 = __builtin_amdgcn_readlane(d0v, qi), d1 = __builtin_amdgcn_readlane(d1v, qi), d2 = __builtin_amdgcn_readlane(d2v, qi);
                    X2_ISSUE(px1, px1b, d0, d1, d2, hb ^ 1);
                    fetch_gates(d0, d1, d2, hb ^ 1);
                }
                const uint32_t cw = (uint32_t)__builtin_amdgcn_readlane(cwv, qi);
                const uint32_t xo = hb * X2_XHALF, wo = hb * X2_WHALF;
                if ((cw & 0xff) != 0xff)         block(xo, wo, cw & 0xff, 0);
                if (((cw >> 8) & 0xff) != 0xff)  block(xo, wo, (cw >> 8) & 0xff, 1);
                if (((cw >> 16) & 0xff) != 0xff) block(xo + X2_SLAB, wo, (cw >> 16) & 0xff, 0);
                if ((cw >> 24) != 0xff)          block(xo + X2_SLAB, wo, cw >> 24, 1);
                if constexpr (PH > 2) {
                    const uint32_t cw2 = (uint32_t)__builtin_amdgcn_readlane(cwv2, qi);
                    if ((cw2 & 0xff) != 0xff)        block(xo + 2 * X2_SLAB, wo, cw2 & 0xff, 0);
                    if (((cw2 >> 8) & 0xff) != 0xff) block(xo + 2 * X2_SLAB, wo, (cw2 >> 8) & 0xff, 1);
                    if constexpr (PH > 3) {
                        if (((cw2 >> 16) & 0xff) != 0xff) block(xo + 3 * X2_SLAB, wo, (cw2 >> 16) & 0xff, 0);
                        if ((cw2 >> 24) != 0xff)          block(xo + 3 * X2_SLAB, wo, cw2 >> 24, 1);
                    }
                }
                hb ^= 1;
            }
        }
    }
#undef X2_ISSUE

    if constexpr (AXIS == 0) {
        // D[o][n]: col = n = r, rows o = (reg & 3) + 8 * (reg >> 2) + 4h  ->  Y[(ob * 32 + o) * N + n]: 64-byte row segments
        if (X2_NO_EPILOGUE) { if (acc[0][0] + acc[1][1] + acc[2][2] + acc[3][3] == 12345.f) Y[0] = DT::from_f32(1.f); return; }
        // (round 6, 'BSX2' version 3: the wave's output block comes from the plan's table -- an unbalanced layout is regrouped on this axis)
        const int my_ob = __builtin_amdgcn_readfirstlane(plan[plan[12] + X2_G * grp + wave]);
        if (my_ob < 0) return;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = n_tile + t * 32 + r;
            if (n >= N) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int o = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                Y[(size_t)(my_ob * 32 + o) * N + n] = DT::from_f32(acc[t][reg]);
            }
        }
        return;
    }
    // Epilogue (as bsmm_xcol.h): D[o][n]: col = n = r (lane), rows o = (reg & 3) + 8 * (reg >> 2) + 4h.  The 16 waves own 16
    // ADJACENT output blocks = 1024 contiguous bytes per minibatch row: staged through the idle ring as [128 rows][1024 B]
    // (16-byte pieces of row n XOR-swizzled with n & 31) and stored as full rows.
    constexpr int ROWB = X2_G * 64;
    if (X2_NO_EPILOGUE) { if (acc[0][0] + acc[1][1] + acc[2][2] + acc[3][3] == 12345.f) Y[0] = DT::from_f32(1.f); return; }
    __syncthreads();
    if (wave < nob) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = t * 32 + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t lo = pack_pair<DT>(acc[t][4 * q + 0], acc[t][4 * q + 1]);
                const uint32_t hi = pack_pair<DT>(acc[t][4 * q + 2], acc[t][4 * q + 3]);
                const int piece = wave * 4 + q;
                *reinterpret_cast<uint2*>(smem + n * ROWB + ((piece ^ (n & 31)) << 4) + 8 * h) = make_uint2(lo, hi);
            }
        }
    }
    __syncthreads();
    {
        const int rowbytes = nob * 64;
        T* ybase = Y + (size_t)ob0 * 32;
        constexpr int PPR = ROWB / 16;
        for (int i = threadIdx.x; i < X2_R * PPR; i += 64 * X2_G) {
            const int n = i / PPR, piece = i % PPR;
            if (n_tile + n < N && piece * 16 < rowbytes) {
                const uint4 v = *reinterpret_cast<const uint4*>(smem + n * ROWB + ((piece ^ (n & 31)) << 4));
                *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(ybase + (size_t)(n_tile + n) * Kout) + piece * 16) = v;
            }
        }
    }
}

}  // namespace bsmm
