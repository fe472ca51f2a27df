// bsmm_dispatch.h -- what the two halves of the kernel dispatch (bsmm_xprop_dispatch.h, bsmm_updat_dispatch.h) and the entry points
// (bsmm_api.hip, the one translation unit that includes all three) share: the argument and plan checks, the packed descriptor words, the
// workspace predicate, run-time values as template arguments, the calls nested in 'BS64' / 'BSS8' plans.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>

#include "bsmm.h"
#include "bsmm_host.h"
#include "bsmm_plan.h"
#include "bsmm_super8.h"
#include "bsmm_xcols.h"
#include "bsmm_b64.h"

using namespace bsmm;

namespace {
// kernel-choice overrides come with the call (bsmm_args.flags), never from process state:
//   0 production dispatch, 1 = BSMM_FLAG_FORCE_VALU, 2 = BSMM_FLAG_NO_PLAN, 3 = BSMM_FLAG_FORCE_PLAN
inline int call_variant(const bsmm_args* a) {
    if (a->flags & BSMM_FLAG_FORCE_VALU) return 1;
    if (a->flags & BSMM_FLAG_NO_PLAN) return 2;
    if (a->flags & BSMM_FLAG_FORCE_PLAN) return 3;
    return 0;
}
inline void trace(const bsmm_args* a, int k) { if (a->trace) *a->trace = k; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device); the result is checked.  The kernel is a template
// ARGUMENT, so every kernel instantiation has its own latch (a latch per function TYPE would be shared by all kernels of one
// signature, e.g. every xcol32_v3_kernel<...>: only the first of them would get the attribute).  The latch is a cache of an
// idempotent driver call, not a switch: it never changes what a later call computes.
template <auto Kernel>
inline int ensure_lds(int bytes) {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipGetLastError();
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

inline size_t elem_size(int dtype) { return dtype == BSMM_F32 ? 4 : 2; }

// compute units of the current device (the kernel-choice cost models and the streaming updat grid scale with it); the driver is
// asked once per device -- a cache of a constant, not a switch
inline int device_cus() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    const int slot = dev & 63;
    int cus = cached[slot].load(std::memory_order_relaxed);
    if (cus > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cached[slot].store(cus, std::memory_order_relaxed);
    return cus;
}

int check_common(const bsmm_args* a) {
    if (!a || !a->lut) return BSMM_ERR_ARG;
    if (a->blocks <= 0 || a->N <= 0 || a->C <= 0 || a->K <= 0) return BSMM_ERR_ARG;
    if (a->bsize != 8 && a->bsize != 16 && a->bsize != 32 && !(a->bsize == 64 && a->axis == 1)) return BSMM_ERR_UNSUPPORTED;   // 64: axis 1 only, as the reference
    if (a->axis != 0 && a->axis != 1) return BSMM_ERR_UNSUPPORTED;
    if (a->dtype != BSMM_F32 && a->dtype != BSMM_F16 && a->dtype != BSMM_BF16) return BSMM_ERR_UNSUPPORTED;
    if (a->C % a->bsize || a->K % a->bsize) return BSMM_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(a->lut) & 15) return BSMM_ERR_ARG;
    return BSMM_OK;
}

// A plan must be one this library built for THIS kind of call (the descriptor comes from bsmm_plan_attach): anything else
// is refused here, on the host, instead of reaching a kernel that would not recognise it.
int check_plan(bool updat, const bsmm_args* a) {
    if (!a->plan) return BSMM_OK;
    if (reinterpret_cast<uintptr_t>(a->plan) & 15) return BSMM_ERR_ARG;
    const int32_t m = a->plan_magic;
    if (a->bsize == 64) return (m == B64PLAN_MAGIC && a->plan_inner == (updat ? 1 : 0)) ? BSMM_OK : BSMM_ERR_ARG;
    if (a->bsize == 8) return (m == S8PLAN_MAGIC && a->plan_width > 0 && (a->plan_items > 0) == updat && (a->dtype != BSMM_F32 || updat)) ? BSMM_OK : BSMM_ERR_ARG;   // (fp32: updat only, UR_F32_SUPER8)
    // (fp32 too: the bf16-split routes run on the 16-bit plans of bsize 32 / 16; bsize-32 'BSUP' plans: retired in round 4, refused as bsmm.h says)
    if (updat) return (((m == UPLAN_MAGIC && a->bsize == 16) || (m == U2PLAN_MAGIC && a->bsize == 32)) && a->plan_items > 0) ? BSMM_OK : BSMM_ERR_ARG;
    if (a->bsize == 16) return (m == X7PLAN_MAGIC && a->plan_width == X7_G && a->dtype != BSMM_F32) ? BSMM_OK : BSMM_ERR_ARG;
    if (a->dtype == BSMM_F32) return (m == XCPLAN_MAGIC && a->plan_width == XS_G) ? BSMM_OK : BSMM_ERR_ARG;
    return (m == XCPLAN_MAGIC || (m == X2PLAN_MAGIC && a->plan_width == X2_G) || (m == X4PLAN_MAGIC && a->plan_width == X4_G && a->axis == 1)) ? BSMM_OK : BSMM_ERR_ARG;
}

// ---- the packed words of the call descriptor (bsmm_plan_attach packs, everything else reads through the accessor beside the packer; the
// bit layout is ABI: include/bsmm.h, tests/test_abi.py) ----
// 'BSU2', plan_inner: item sets (4 bits) | all sets equally long (bit 4) | longest set << 8 (13 bits) | direct blocks << 21 (10 bits)
inline int32_t u2_pack_inner(int sets, bool equal, int longest, int direct) { return sets | (equal ? 16 : 0) | (longest << 8) | (direct << 21); }
inline int u2_sets(const bsmm_args* a) { return a->plan_inner & 15; }
inline bool u2_sets_equal(const bsmm_args* a) { return (a->plan_inner & 16) != 0; }
inline int u2_longest_set(const bsmm_args* a) { return (a->plan_inner >> 8) & 0x1fff; }
inline int u2_direct_blocks(const bsmm_args* a) { return (a->plan_inner >> 21) & 0x3ff; }
static_assert(U2_DIRECT_MAX <= 0x3ff, "direct blocks: 10 bits");
// 'BSUP' with a 'BSU6' section, plan_width / plan_waves: the plan's own window width / waves (8 bits) | the section's window width / item count << 8
inline int32_t up_pack(int base, int section) { return base | (section << 8); }
inline int up_base(int32_t word) { return word & 255; }
inline int up_section(int32_t word) { return word >> 8; }
static_assert(UW16 <= 255 && UP_WAVES <= 255 && U6_WC <= 255, "window width / waves: 8 bits");
// 'BSS8', plan_inner: the nested bsize-32 plan's width (8 bits) | its format << 8 (3 bits; 0: round-1 'BSXC' / 'BSUP', 1: staged 'BSX2', 2: streaming
// 'BSU2') | the nested plan's own plan_inner << 11
inline int32_t s8_pack_inner(int width, int code, int32_t inner) { return width | (code << 8) | (int32_t)((uint32_t)inner << 11); }
inline int s8_nested_width(const bsmm_args* a) { return a->plan_inner & 0xff; }
inline int s8_nested_code(const bsmm_args* a) { return (a->plan_inner >> 8) & 7; }
inline int32_t s8_nested_inner(const bsmm_args* a) { return (int32_t)((uint32_t)a->plan_inner >> 11); }
// 'BS64', plan_waves: the nested bsize-32 plan's waves (5 bits) | code of its format << 5 (3 bits, kNestedMagic) | its plan_inner << 8
inline int32_t b64_pack_waves(int waves, int code, int32_t inner) { return waves | (code << 5) | (int32_t)((uint32_t)inner << 8); }
inline int b64_nested_waves(const bsmm_args* a) { return a->plan_waves & 31; }
inline int b64_nested_code(const bsmm_args* a) { return (a->plan_waves >> 5) & 7; }
inline int32_t b64_nested_inner(const bsmm_args* a) { return (int32_t)((uint32_t)a->plan_waves >> 8); }
static_assert(U2_WAVES <= 31 && UP_WAVES <= 31 && X2_G <= 31 && X4_G <= 31, "nested waves: 5 bits");

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
// THE workspace check of a call: `need` bytes (0: none) at a 16-byte aligned address
inline bool workspace_ok(const bsmm_args* a, size_t need) { return need == 0 || (a->workspace && a->workspace_bytes >= need && aligned16(a->workspace)); }
// a run-time bool (fprop / bprop, transposed weights) as a template argument: f(std::true_type{}) or f(std::false_type{})
template <class F>
inline auto by_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// the (bsize, axis) of a call as template arguments: f(std::integral_constant<int, BS>{}, std::integral_constant<int, AXIS>{}); bsize 32 / 16 / 8
template <class F>
inline int by_shape(const bsmm_args* a, F&& f) {
    if (a->axis != 0 && a->axis != 1) return BSMM_ERR_UNSUPPORTED;
    auto with_bs = [&](auto bs) -> int { return a->axis == 0 ? f(bs, std::integral_constant<int, 0>{}) : f(bs, std::integral_constant<int, 1>{}); };
    switch (a->bsize) {
        case 32: return with_bs(std::integral_constant<int, 32>{});
        case 16: return with_bs(std::integral_constant<int, 16>{});
        case 8:  return with_bs(std::integral_constant<int, 8>{});
    }
    return BSMM_ERR_UNSUPPORTED;
}

// the bsize-32 call nested in a 'BSS8' plan
inline bsmm_args s8_inner(const bsmm_args* a, bool updat) {
    const int ns = a->plan_width, code = s8_nested_code(a);
    bsmm_args b = *a;
    b.bsize = 32; b.blocks = ns; b.plan = a->plan + s8_off_nested(ns);
    b.plan_width = s8_nested_width(a);
    b.plan_inner = s8_nested_inner(a);
    b.plan_magic = updat ? (code == 2 ? U2PLAN_MAGIC : UPLAN_MAGIC) : (code == 1 ? X2PLAN_MAGIC : XCPLAN_MAGIC);
    return b;
}

// ---- bsize 64 (feature axis 1): the quadrant view on the bsize-32 path ('BS64' plans, bsmm_plan.h / bsmm_b64.h) ----
// descriptor of a 'BS64' plan in bsmm_args (bsmm_plan_attach): plan_width / plan_items = the nested plan's, plan_waves: b64_pack_waves,
// plan_inner = 0 (xprop) / 1 (updat)
const int32_t kNestedMagic[8] = {0, XCPLAN_MAGIC, X2PLAN_MAGIC, 0 /* (3: 'BSXF', retired) */, UPLAN_MAGIC, U2PLAN_MAGIC, X4PLAN_MAGIC, 0};
inline int nested_code(int32_t magic) { for (int i = 1; i < 8; ++i) if (kNestedMagic[i] == magic) return i; return 0; }
inline size_t b64_w_bytes(const bsmm_args* a) { return round16((size_t)a->blocks * 4096 * elem_size(a->dtype)); }
inline size_t b64_gate_bytes(const bsmm_args* a) { return a->gate ? round16((size_t)a->blocks * 4 * sizeof(float)) : 0; }
// the bsize-32 call behind a bsize-64 one (workspace fields left to the caller)
inline bsmm_args b64_inner(const bsmm_args* a, bool updat) {
    bsmm_args b = *a;
    b.bsize = 32; b.blocks = 4 * a->blocks; b.prepared_w = nullptr;
    b.lut = a->plan + B64_HDR;
    if (!updat) { b.segments = 2 * a->segments; b.locks = 2 * a->locks; }
    b.plan = a->plan + b64_off_nested(updat ? 1 : 0, updat ? 0 : a->segments, a->blocks);
    b.plan_magic = kNestedMagic[b64_nested_code(a)];
    b.plan_waves = b64_nested_waves(a);
    b.plan_inner = b64_nested_inner(a);
    if (b.plan_magic == 0) { b.plan = nullptr; b.plan_width = b.plan_waves = b.plan_items = b.plan_inner = 0; }
    return b;
}
}  // namespace
