"""Memory-contract tier of the block-sparse matmul: no kernel family stores outside its outputs and workspaces, leaves an output element
unstored, relies on scratch it did not clear, or lets a read outside an input reach a result.

Every case runs fprop / bprop / updat through the product API on a FRESH operator (its grow-on-demand workspace cannot have been sized by an
earlier, larger call) with the layout's inputs placed in a guard arena (tests/_guard.py) and every allocation the package makes -- outputs,
workspaces, gate images, prepared weight pieces -- routed into the same arena: 0xFF everywhere (NaN in every float type) before the call,
guards of at least 128 rows / 64 KiB on both sides of every tensor, the tensor's end flush against its back guard.  Per case:

  (a) the kernel family (and variant) the case is there for ran (bsmm_args.trace);
  (b) no guard byte changed, around any buffer (the failure names the buffer by the line that allocated it);
  (c) no output element is NaN: every element was stored, and none was computed from poisoned memory;
  (d) tests/_parity.py::assert_blocks against the float64 oracle, at that file's bars.

Shapes are the edges, not the sizes: minibatches of 1 and 33, one below / at / above the row tiles (63 / 64 / 65, 127 / 128 / 129) and the dispatch
thresholds (XSN_NMAX / 8, / 2 and XSN_NMAX itself, BSMM_SMALL_N_MAX, UTS_NMAX, UAW_NMAX, XS0_NMAX and twice that, GATE_IMAGES_MIN_N), N % 8 != 0 on
feature axis 0, grids of 37 x 53, 1 x 70, 70 x 1, 5 x 5 dense, one block, an empty row and column of blocks, operands offset by one element.
(BlocksparseMatMul.LONG_MINIBATCH needs a grid of 64 windows of 32 x 32 blocks -- 256 blocks a side -- and is not reachable at these sizes.)
Production dispatch where it reaches a family at such a shape, the suite's usual switches (set_kernel_variant, plan_options) elsewhere; the
expected code of a production case is what the dispatch rules of csrc/bsmm_xprop_dispatch.h and csrc/bsmm_updat_dispatch.h give for it on 256 compute units.  A retuned dispatch
constant therefore turns (a) red for the cases it moves: read the rule, and where the new choice is the intended one put its code into the row --
or move the case's shape so that the family it is there for is still reached (test_memory_bounds_table.py says which must be).

The table is explicit -- nothing is random, the ids are stable -- and tests/test_memory_bounds_table.py (CPU tier) holds it against the
trace codes of blocksparse_amd/_lib.py, so a kernel family added later cannot stay out of this tier unnoticed."""
import collections

import numpy as np
import pytest

import _guard as GD
import _parity as P
from oracle import bsmm_oracle as orc

# what the shapes below straddle (the dispatch thresholds of csrc/bsmm_xprop_dispatch.h and csrc/bsmm_updat_dispatch.h; test_memory_bounds_table.py checks them against the source)
XS0_NMAX, XSN_NMAX, UAW_NMAX, UTS_NMAX, SMALL_N_MAX = 512, 512, 128, 768, 4096

Case = collections.namedtuple("Case", "id bs axis dt lay N variant opts flow seg exp pairs alpha beta mis gate split mode")


def C(id, bs, axis, dt, lay, N, exp, variant=0, opts=(), flow=True, seg=False, pairs=1, alpha=1.0, beta=0.0, mis=0, gate=None, split=0, mode="all"):
    """exp: (fprop, bprop, updat) trace codes by name, "NAME/VARIANT" where the variant byte is part of the statement; None = the pass is not run.
    variant: _lib.set_kernel_variant; opts: names of _lib.PLAN_* bits; gate: None / "general" / "binary" (fprop, bprop and updat gated);
    mode: "all" | "sums" (updat(sums_only=True) + updat_finalize)."""
    return Case(id, bs, axis, dt, lay, N, variant, tuple(opts), flow, seg, exp, pairs, alpha, beta, mis, gate, split, mode)


def layouts(name):
    if name == "r37x53":                # sides that are no multiple of any group width (8 / 16 / 32)
        return P.random_layout(37, 53, 0.15, seed=11)
    if name == "r40x24":
        return P.random_layout(40, 24, 0.3, seed=2)
    if name == "1x70":
        return np.ones((1, 70), dtype=np.int32)
    if name == "70x1":
        return np.ones((70, 1), dtype=np.int32)
    if name == "d5":
        return np.ones((5, 5), dtype=np.int32)
    if name == "one":
        return np.ones((1, 1), dtype=np.int32)
    if name == "holes":                 # an empty row and an empty column of blocks
        lay = P.random_layout(21, 19, 0.3, seed=5)
        lay[3, :] = 0
        lay[:, 5] = 0
        return lay
    if name == "hubs":                  # hub rows / columns: the reference-policy tables cut them into segments that share output blocks
        return P.ba_layout(40, 3, seed=1)
    if name == "r36x52":                # bsize 8: C and K multiples of 32 (the super-block path's condition)
        return P.random_layout(36, 52, 0.12, seed=7)
    if name == "r66x70":                # bsize 16 / 8: partial windows on both edges
        return P.random_layout(66, 70, 0.12, seed=9)
    if name == "s60":                   # 16 x 16-block windows with a handful of blocks each
        return P.random_layout(60, 60, 0.02, seed=3)
    if name == "8x128":                 # enough 128-row units of the flow kernel for its full-unit variant (needs >= one per compute unit)
        return P.random_layout(8, 128, 0.3, seed=13)
    if name == "direct":                # window (0, 0) crowded beyond what its 16 waves hold: the streaming plan gets direct blocks
        lay = P.random_layout(33, 17, 0.22, seed=9)
        rng = np.random.default_rng(10)
        free = np.argwhere(lay[:16, :16] == 0)
        for i in rng.permutation(len(free))[:25]:
            lay[free[i][0], free[i][1]] = 1
        return lay
    raise KeyError(name)


S, M, F, ST, ST16, X32 = "K_XPROP_SMALL", "K_XPROP_MID", "K_XCOL32_FLOW", "K_XCOL32_STAGED", "K_XCOL16_STAGED", "K_XCOL32"
FH = "K_XCOL32_FLOW/KV_FLOW_HALF_UNITS"
FF = "K_XCOL32_FLOW/0"
SEG, VAL, S8, F32S = "K_XPROP_SEGMENT", "K_XPROP_VALU", "K_XPROP_SUPER8", "K_XCOL32_F32SPLIT"
UV, UB, UTR, U1W, USTR, UW16, UR16, US8 = ("K_UPDAT_VALU", "K_UPDAT_BLOCK", "K_UPDAT_BLOCK_TR/0", "K_UPDAT_BLOCK_TR/KV_ONE_WAVE", "K_UPDAT_STREAM",
                                           "K_UPDAT16_WIN", "K_UPDAT16_ROWS", "K_UPDAT_SUPER8")

CASES = []
_add = CASES.append

# ---- bsize 32, feature axis 1, 16-bit, production dispatch: the small-minibatch kernel (64-row workgroups) and the one-wave weight gradient ----
for n in (1, 33, 63, 64, 65):
    _add(C("a1-b32-bf16-prod-N%d" % n, 32, 1, "bf16", "r37x53", n, (S, S, U1W)))
_add(C("a1-b32-f16-prod-N65", 32, 1, "f16", "r37x53", 65, (S, S, U1W)))
_add(C("a1-b32-bf16-prod-1x70-N33", 32, 1, "bf16", "1x70", 33, (S, S, U1W)))
_add(C("a1-b32-bf16-prod-70x1-N33", 32, 1, "bf16", "70x1", 33, (S, S, U1W)))
_add(C("a1-b32-bf16-prod-one-N1", 32, 1, "bf16", "one", 1, (S, S, U1W)))
_add(C("a1-b32-bf16-prod-holes-N65", 32, 1, "bf16", "holes", 65, (S, S, U1W)))
_add(C("a1-b32-bf16-prod-3pairs-N65", 32, 1, "bf16", "r37x53", 65, (None, None, U1W), pairs=3, alpha=0.5, beta=2.0))
# UTS_NMAX: the last minibatch of the one-wave kernel and the first one past it (no plan: the transposing-read kernel)
_add(C("a1-b32-bf16-noplan-N768", 32, 1, "bf16", "r37x53", UTS_NMAX, (SEG, SEG, U1W), variant=2))
_add(C("a1-b32-bf16-noplan-N769", 32, 1, "bf16", "r37x53", UTS_NMAX + 1, (SEG, SEG, UTR), variant=2))
_add(C("a1-b32-f16-noplan-8pairs-N129", 32, 1, "f16", "r40x24", 129, (None, None, UTR), variant=2, pairs=8, alpha=0.25, beta=0.5))
# BSMM_SMALL_N_MAX: at and just above
_add(C("a1-b32-bf16-prod-one-N4096", 32, 1, "bf16", "one", SMALL_N_MAX, (S, S, USTR)))
_add(C("a1-b32-bf16-prod-one-N4097", 32, 1, "bf16", "one", SMALL_N_MAX + 1, (FH, FH, USTR)))
# the medium-minibatch kernel: one wave per (output block, 64 rows)
for n in (63, 64, 65, 200):
    _add(C("a1-b32-bf16-mid-N%d" % n, 32, 1, "bf16", "r37x53", n, (M, M, None), variant=4))
_add(C("a1-b32-bf16-mid-4blocks-N2241", 32, 1, "bf16", "r37x53", 2241, (M, M, None), variant=4))   # activations above 5 MiB: workgroups of 4 output blocks x one row chunk
_add(C("a1-b32-f16-mid-holes-N129", 32, 1, "f16", "holes", 129, (M, M, None), variant=4))
# ---- the plan kernels, forced: flow (both unit sizes), staged, the round-1 grouped kernel; streaming weight gradient ----
for n in (1, 33, 127, 128, 129):
    _add(C("a1-b32-bf16-flow-N%d" % n, 32, 1, "bf16", "r37x53", n, (FH, FH, USTR), variant=3))
_add(C("a1-b32-f16-flow-holes-N129", 32, 1, "f16", "holes", 129, (FH, FH, USTR), variant=3))
_add(C("a1-b32-bf16-flow-1x70-N65", 32, 1, "bf16", "1x70", 65, (FH, FH, USTR), variant=3))
_add(C("a1-b32-bf16-flow-70x1-N65", 32, 1, "bf16", "70x1", 65, (FH, FH, USTR), variant=3))
_add(C("a1-b32-bf16-flow-d5-N200", 32, 1, "bf16", "d5", 200, (FH, FH, USTR), variant=3))
_add(C("a1-b32-bf16-flow-full-units-N4097", 32, 1, "bf16", "8x128", 4097, (FF, FH, USTR), variant=3))
for n in (127, 128, 129):
    _add(C("a1-b32-bf16-staged-N%d" % n, 32, 1, "bf16", "r37x53", n, (ST, ST, None), variant=3, flow=False))
_add(C("a1-b32-f16-staged-holes-N33", 32, 1, "f16", "holes", 33, (ST, ST, None), variant=3, flow=False))
_add(C("a1-b32-bf16-xcol32-wide-N129", 32, 1, "bf16", "r37x53", 129, (X32, X32, None), variant=3, opts=("PLAN_XCOL_UNSTAGED",)))
_add(C("a1-b32-bf16-xcol32-narrow-N65", 32, 1, "bf16", "r37x53", 65, (X32, X32, None), variant=3, opts=("PLAN_XCOL_NARROW",)))
_add(C("a1-b32-bf16-stream-direct-N392", 32, 1, "bf16", "direct", 392, (None, None, USTR), variant=3))
_add(C("a1-b32-bf16-stream-nodirect-N392", 32, 1, "bf16", "direct", 392, (None, None, USTR), variant=3, opts=("PLAN_UPDAT_NO_DIRECT",)))
_add(C("a1-b32-bf16-stream32-N200", 32, 1, "bf16", "direct", 200, (None, None, USTR), variant=3, opts=("PLAN_STREAM_32",)))
_add(C("a1-b32-bf16-stream8-N72", 32, 1, "bf16", "r37x53", 72, (None, None, USTR), variant=3, opts=("PLAN_STREAM_8",)))
_add(C("a1-b32-bf16-stream-3pairs-N65", 32, 1, "bf16", "r37x53", 65, (None, None, USTR), variant=3, pairs=3, alpha=0.5, beta=2.0))
_add(C("a1-b32-f16-stream-8pairs-N33", 32, 1, "f16", "holes", 33, (None, None, USTR), variant=3, pairs=8, alpha=2.0, beta=-1.0))
_add(C("a1-b32-bf16-stream-split3-N200", 32, 1, "bf16", "r37x53", 200, (None, None, USTR), variant=3, split=3))
_add(C("a1-b32-bf16-stream-sums-N129", 32, 1, "bf16", "r37x53", 129, (None, None, USTR), variant=3, mode="sums", alpha=0.5))
_add(C("a1-b32-bf16-stream-one-N1", 32, 1, "bf16", "one", 1, (None, None, USTR), variant=3))
# ---- reference-policy (segmented, locked) tables on the per-segment kernels: the fp32 image of the output in the workspace ----
_add(C("a1-b32-bf16-locked-N65", 32, 1, "bf16", "hubs", 65, (SEG, SEG, None), variant=2, seg=True))
_add(C("a0-b32-f16-locked-N40", 32, 0, "f16", "hubs", 40, (SEG, SEG, None), variant=2, seg=True))
_add(C("a1-b16-bf16-locked-N33", 16, 1, "bf16", "hubs", 33, (SEG, SEG, None), variant=2, seg=True))
# ---- V_FMA kernels: forced, and through operands that are element-aligned but not 16-byte aligned ----
_add(C("a1-b32-bf16-valu-N33", 32, 1, "bf16", "r37x53", 33, (VAL, VAL, UV), variant=1))
_add(C("a1-b32-bf16-unaligned-N65", 32, 1, "bf16", "r37x53", 65, (VAL, VAL, UB), mis=1))
_add(C("a1-b32-f32-unaligned-N33", 32, 1, "f32", "holes", 33, (VAL, VAL, UB), mis=1))
_add(C("a0-b32-bf16-unaligned-N40", 32, 0, "bf16", "r37x53", 40, (VAL, VAL, UV), mis=1))
_add(C("a1-b32-f32-unaligned-dw-N33", 32, 1, "f32", "r37x53", 33, (VAL, VAL, UV), mis=1, alpha=0.5, beta=2.0))   # a misaligned dw: the V_FMA weight gradient
_add(C("a0-b32-f32-prod-N33", 32, 0, "f32", "holes", 33, (SEG, SEG, UV)))                     # fp32 rows of N % 4 != 0 elements
_add(C("a0-b16-f32-prod-N66", 16, 0, "f32", "r66x70", 66, (SEG, SEG, UV)))
_add(C("a1-b8-f32-prod-r37x53-N65", 8, 1, "f32", "r37x53", 65, (VAL, VAL, UV), pairs=3, alpha=0.5, beta=2.0))   # bsize 8 without super-blocks
_add(C("a1-b16-f16-unaligned-N129", 16, 1, "f16", "r66x70", 129, (VAL, VAL, UV), mis=1, beta=0.5, alpha=2.0))
# ---- fp32, bsize 32 ----
_add(C("a1-b32-f32-prod-N33", 32, 1, "f32", "r37x53", 33, (SEG, SEG, UB)))
for n in (127, 129):
    _add(C("a1-b32-f32-split-N%d" % n, 32, 1, "f32", "r37x53", n, (F32S, F32S, USTR), variant=3))
_add(C("a1-b32-f32-split-holes-N1", 32, 1, "f32", "holes", 1, (F32S, F32S, USTR), variant=3))
_add(C("a0-b32-f32-split-N136", 32, 0, "f32", "r37x53", 136, (F32S, F32S, UB), variant=3))
_add(C("a1-b32-f32-updat-split-N264", 32, 1, "f32", "r37x53", 264, (None, None, USTR), alpha=0.5, beta=0.25))
_add(C("a1-b32-f32-updat-split-sums-N257", 32, 1, "f32", "holes", 257, (None, None, USTR), mode="sums"))
# ---- bsize 32, feature axis 0 ----
for n in (8, 40, XS0_NMAX, XS0_NMAX + 8):
    _add(C("a0-b32-bf16-prod-N%d" % n, 32, 0, "bf16", "r37x53", n, (S if n <= XS0_NMAX else SEG,) * 2 + (UB,)))
_add(C("a0-b32-f16-prod-70x1-N1024", 32, 0, "f16", "70x1", 2 * XS0_NMAX, (S, ST, UB)))         # long columns: the small kernel up to 2 x XS0_NMAX
_add(C("a0-b32-f16-prod-70x1-N1032", 32, 0, "f16", "70x1", 2 * XS0_NMAX + 8, (SEG, ST, UB)))
_add(C("a0-b32-bf16-prod-N33", 32, 0, "bf16", "r37x53", 33, (SEG, SEG, UV)))                     # N % 8 != 0: per-segment / V_FMA
_add(C("a0-b32-bf16-prod-holes-N64", 32, 0, "bf16", "holes", UAW_NMAX // 2, (S, S, UB)))
_add(C("a0-b32-bf16-prod-holes-N72", 32, 0, "bf16", "holes", UAW_NMAX // 2 + 8, (S, S, UB)))
for n in (200, 264):
    _add(C("a0-b32-bf16-staged-N%d" % n, 32, 0, "bf16", "r37x53", n, (ST, ST, USTR), variant=3))
_add(C("a0-b32-f16-staged-holes-N8", 32, 0, "f16", "holes", 8, (ST, ST, USTR), variant=3, pairs=3, alpha=0.5, beta=2.0))
_add(C("a0-b32-bf16-xcol32-N40", 32, 0, "bf16", "r37x53", 40, (X32, X32, None), variant=3, opts=("PLAN_XCOL_UNSTAGED",)))
# ---- bsize 16, feature axis 1: XSN_NMAX / 8 (bprop) and XSN_NMAX / 2 (fprop) ----
for n in (1, 33, XSN_NMAX // 8, XSN_NMAX // 8 + 1, XSN_NMAX // 2, XSN_NMAX // 2 + 1):
    _add(C("a1-b16-bf16-prod-N%d" % n, 16, 1, "bf16", "r66x70", n, (S if n <= XSN_NMAX // 2 else SEG, S if n <= XSN_NMAX // 8 else SEG, UW16)))
_add(C("a1-b16-f16-prod-holes-N63", 16, 1, "f16", "holes", 63, (S, S, UW16)))
for n in (127, 129):
    _add(C("a1-b16-bf16-list-N%d" % n, 16, 1, "bf16", "r66x70", n, (ST16, ST16, UW16), variant=3))
_add(C("a1-b16-f16-pairs-d5-N65", 16, 1, "f16", "d5", 65, (ST16, ST16, UW16), variant=3))        # dense: the pair kernel
_add(C("a1-b16-bf16-noplan-N65", 16, 1, "bf16", "r66x70", 65, (SEG, SEG, UTR), variant=2, pairs=3, alpha=0.5, beta=2.0))
_add(C("a1-b16-bf16-win-8pairs-N40", 16, 1, "bf16", "holes", 40, (None, None, UW16), variant=3, pairs=8))
_add(C("a1-b16-bf16-win-split-N1032", 16, 1, "bf16", "r66x70", 1032, (None, None, UW16), variant=3, split=2))
_add(C("a1-b16-f32-updat-split-N264", 16, 1, "f32", "r66x70", 264, (SEG, SEG, UW16), alpha=0.5, beta=0.25))
# ---- bsize 16, feature axis 0 ----
for n in (8, 40, XS0_NMAX, 2 * XS0_NMAX, 2 * XS0_NMAX + 8):
    _add(C("a0-b16-bf16-prod-N%d" % n, 16, 0, "bf16", "r66x70", n, (S if n <= 2 * XS0_NMAX else SEG,) * 2 + (UW16,)))
# (nearly empty windows: the per-block kernels -- one wave per block up to UAW_NMAX columns, four from there)
_add(C("a0-b16-bf16-prod-sparse-N128", 16, 0, "bf16", "s60", UAW_NMAX, (S, S, UB)))
_add(C("a0-b16-bf16-prod-sparse-N136", 16, 0, "bf16", "s60", UAW_NMAX + 8, (S, S, UB)))
_add(C("a0-b16-f16-prod-sparse-3pairs-N40", 16, 0, "f16", "s60", 40, (None, None, UB), pairs=3, alpha=0.5, beta=2.0))
_add(C("a0-b16-f16-prod-N33", 16, 0, "f16", "r66x70", 33, (SEG, SEG, UV)))
for n in (200, 264):
    _add(C("a0-b16-bf16-list-rows-N%d" % n, 16, 0, "bf16", "r66x70", n, (ST16, ST16, UR16), variant=3))
_add(C("a0-b16-f16-rows-3pairs-N72", 16, 0, "f16", "holes", 72, (None, None, UR16), variant=3, pairs=3, alpha=0.5, beta=2.0))
_add(C("a0-b16-bf16-rows-split3-N520", 16, 0, "bf16", "r66x70", 520, (None, None, UR16), variant=3, split=3))
_add(C("a0-b16-bf16-win-N200", 16, 0, "bf16", "r66x70", 200, (None, None, UW16), variant=3, opts=("PLAN_UPDAT16_WINDOWED",)))
_add(C("a0-b16-f32-rows-N264", 16, 0, "f32", "r66x70", 264, (SEG, SEG, UR16), variant=3))
# ---- bsize 8 ----
for n in (1, 33, XSN_NMAX, XSN_NMAX + 1):
    _add(C("a1-b8-bf16-prod-N%d" % n, 8, 1, "bf16", "r36x52", n, (S if n <= XSN_NMAX else VAL,) * 2 + (US8,)))
_add(C("a1-b8-f16-prod-r37x53-N65", 8, 1, "f16", "r37x53", 65, (S, S, UV)))                       # C, K no multiples of 32: no super-blocks
for n in (127, 129):
    _add(C("a1-b8-bf16-super8-N%d" % n, 8, 1, "bf16", "r36x52", n, (S8, S8, US8), variant=3))
_add(C("a1-b8-f16-super8-3pairs-N33", 8, 1, "f16", "r36x52", 33, (S8, S8, US8), variant=3, pairs=3, alpha=0.5, beta=2.0))
for n in (8, 40, 2 * XS0_NMAX, 2 * XS0_NMAX + 8):
    _add(C("a0-b8-bf16-prod-N%d" % n, 8, 0, "bf16", "r36x52", n, (S, S, UB)))
_add(C("a0-b8-bf16-prod-N33", 8, 0, "bf16", "r36x52", 33, (VAL, VAL, UV)))
_add(C("a0-b8-f16-super8-N200", 8, 0, "f16", "r36x52", 200, (S8, S8, US8), variant=3))
_add(C("a1-b8-f32-updat-split-N264", 8, 1, "f32", "r36x52", 264, (VAL, VAL, US8), alpha=0.5, beta=0.25))
_add(C("a0-b8-f32-updat-split-N256", 8, 0, "f32", "r36x52", 256, (VAL, VAL, US8)))
# ---- bsize 64 on feature axis 1: the composite plan (quadrant copy + gates + the nested bsize-32 call) ----
for n in (33, 129):
    _add(C("a1-b64-bf16-prod-N%d" % n, 64, 1, "bf16", "holes", n, (S, S, U1W)))
_add(C("a1-b64-f16-forced-N129", 64, 1, "f16", "holes", 129, (FH, FH, USTR), variant=3, pairs=3, alpha=0.5, beta=2.0))
_add(C("a1-b64-bf16-gated-N65", 64, 1, "bf16", "holes", 65, (ST, ST, USTR), variant=3, gate="general"))
# ---- gated calls: the GATED staged kernel below GATE_IMAGES_MIN_N, weight images (over doubled tables for general gates) from there on ----
_add(C("a1-b32-bf16-gated-staged-N129", 32, 1, "bf16", "r40x24", 129, (ST, ST, USTR), variant=3, gate="general"))
_add(C("a0-b32-f16-gated-staged-N72", 32, 0, "f16", "holes", 72, (ST, ST, USTR), variant=3, gate="general"))
_add(C("a1-b32-bf16-gated-segment-N65", 32, 1, "bf16", "r40x24", 65, (SEG, SEG, U1W), gate="general"))
_add(C("a1-b32-bf16-gated-images2-N1025", 32, 1, "bf16", "r40x24", 1025, (FH, FH, USTR), variant=3, gate="general"))
_add(C("a1-b32-bf16-gated-image1-N1024", 32, 1, "bf16", "r40x24", 1024, (FH, FH, USTR), variant=3, gate="binary"))
_add(C("a1-b16-bf16-gated-segment-N2047", 16, 1, "bf16", "holes", 2047, (SEG, SEG, None), variant=3, gate="general"))
_add(C("a1-b16-bf16-gated-images2-N2048", 16, 1, "bf16", "holes", 2048, (ST16, ST16, None), variant=3, gate="general"))
_add(C("a1-b16-bf16-gated-images2-N2049", 16, 1, "bf16", "holes", 2049, (ST16, ST16, None), variant=3, gate="general"))
# (doubled tables name every (output block, input block) twice: entry lists in the flow and bsize-16 list plans, a second step over the same
#  pair of input blocks in the positional plans of the staged and the round-1 kernels)
_add(C("a1-b32-bf16-gated-images2-noflow-N1025", 32, 1, "bf16", "r40x24", 1025, (ST, ST, None), variant=3, gate="general", flow=False))
_add(C("a0-b32-bf16-gated-images2-N1032", 32, 0, "bf16", "r40x24", 1032, (ST, ST, None), variant=3, gate="general"))
_add(C("a0-b32-bf16-gated-images2-d5-N1160", 32, 0, "bf16", "d5", 1160, (ST, ST, None), variant=3, gate="general"))
_add(C("a1-b32-bf16-gated-images2-xcol32-N1025", 32, 1, "bf16", "r40x24", 1025, (X32, X32, None), variant=3, gate="general", opts=("PLAN_XCOL_UNSTAGED",)))
_add(C("a0-b32-bf16-gated-images2-xcol32-N1032", 32, 0, "bf16", "holes", 1032, (X32, X32, None), variant=3, gate="general", opts=("PLAN_XCOL_NARROW",)))
_add(C("a0-b32-f16-gated-image1-N1032", 32, 0, "f16", "r40x24", 1032, (ST, ST, None), variant=3, gate="general"))
_add(C("a1-b16-bf16-gated-images2-dense-N2049", 16, 1, "bf16", "d5", 2049, (ST16, ST16, None), variant=3, gate="general"))
_add(C("a0-b16-bf16-gated-images2-N2056", 16, 0, "bf16", "r66x70", 2056, (ST16, ST16, None), variant=3, gate="general"))
_add(C("a0-b16-f16-gated-image1-N2056", 16, 0, "f16", "holes", 2056, (ST16, ST16, None), variant=3, gate="general"))
_add(C("a0-b16-f16-gated-rows-N264", 16, 0, "f16", "r66x70", 264, (None, None, UR16), variant=3, gate="general"))
_add(C("a1-b8-bf16-gated-N33", 8, 1, "bf16", "r36x52", 33, (VAL, VAL, UV), gate="general"))

# ---- the degenerate grids (one row / one column of blocks, 5 x 5 dense, a single block, empty rows and columns) on the other (bsize, axis) ----
for _bs, _ax, _lay, _v, _exp in (
        (32, 0, "1x70", 0, (S, S, UB)),
        (32, 0, "1x70", 3, (ST, ST, USTR)),
        (32, 0, "70x1", 0, (S, S, UB)),
        (32, 0, "70x1", 3, (ST, ST, USTR)),
        (32, 0, "d5", 0, (S, S, UB)),
        (32, 0, "d5", 3, (ST, ST, USTR)),
        (32, 0, "one", 0, (S, S, UB)),
        (32, 0, "one", 3, (ST, ST, USTR)),
        (32, 0, "holes", 0, (S, S, UB)),
        (32, 0, "holes", 3, (ST, ST, USTR)),
        (16, 1, "1x70", 0, (S, S, UW16)),
        (16, 1, "1x70", 3, (ST16, ST16, UW16)),
        (16, 1, "70x1", 0, (S, S, UW16)),
        (16, 1, "70x1", 3, (ST16, ST16, UW16)),
        (16, 1, "d5", 0, (S, S, UW16)),
        (16, 1, "d5", 3, (ST16, ST16, UW16)),
        (16, 1, "one", 0, (S, S, UW16)),
        (16, 1, "one", 3, (ST16, ST16, UW16)),
        (16, 1, "holes", 0, (S, S, UW16)),
        (16, 1, "holes", 3, (ST16, ST16, UW16)),
        (16, 0, "1x70", 0, (S, S, UW16)),
        (16, 0, "1x70", 3, (ST16, ST16, UW16)),
        (16, 0, "70x1", 0, (S, S, UW16)),
        (16, 0, "70x1", 3, (ST16, ST16, UR16)),
        (16, 0, "d5", 0, (S, S, UB)),
        (16, 0, "d5", 3, (ST16, ST16, UR16)),
        (16, 0, "one", 0, (S, S, UB)),
        (16, 0, "one", 3, (ST16, ST16, UR16)),
        (16, 0, "holes", 0, (S, S, UW16)),
        (16, 0, "holes", 3, (ST16, ST16, UR16)),
        (8, 1, "1x70", 0, (S, S, UV)),
        (8, 1, "1x70", 3, (VAL, VAL, UV)),
        (8, 1, "70x1", 0, (S, S, UV)),
        (8, 1, "70x1", 3, (VAL, VAL, UV)),
        (8, 1, "d5", 0, (S, S, UV)),
        (8, 1, "d5", 3, (VAL, VAL, UV)),
        (8, 1, "one", 0, (S, S, UV)),
        (8, 1, "one", 3, (VAL, VAL, UV)),
        (8, 1, "holes", 0, (S, S, UV)),
        (8, 1, "holes", 3, (VAL, VAL, UV)),
        (8, 0, "1x70", 0, (S, S, UB)),
        (8, 0, "1x70", 3, (VAL, VAL, UV)),
        (8, 0, "70x1", 0, (S, S, UB)),
        (8, 0, "70x1", 3, (VAL, VAL, UV)),
        (8, 0, "d5", 0, (S, S, UB)),
        (8, 0, "d5", 3, (VAL, VAL, UV)),
        (8, 0, "one", 0, (S, S, UB)),
        (8, 0, "one", 3, (VAL, VAL, UV)),
        (8, 0, "holes", 0, (S, S, UB)),
        (8, 0, "holes", 3, (VAL, VAL, UV)),
):
    _dt = "f16" if _lay in ("70x1", "one") else "bf16"
    _n = 33 if _ax else 40
    _add(C("a%d-b%d-%s-%s-%s-N%d" % (_ax, _bs, _dt, "forced" if _v else "prod", _lay, _n), _bs, _ax, _dt, _lay, _n, _exp, variant=_v))

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def expected_codes():
    """{trace-code name} and {(code name, variant name)} the table expects somewhere (for the CPU-tier coverage test)."""
    fams, variants = set(), set()
    for c in CASES:
        for e in c.exp:
            if e is None:
                continue
            name, _, var = e.partition("/")
            fams.add(name)
            if var and var != "0":
                variants.add((name, var))
    return fams, variants


# ---------------------------------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import BlocksparseMatMul, _lib, matmul
    _lib.load()
    return torch, BlocksparseMatMul, _lib, matmul


def _gate_values(blocks, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "binary":
        g = (rs.rand(blocks) < 0.8).astype(np.float32)
    else:                                  # zeros, negatives, values above one
        g = rs.uniform(-0.5, 2.0, size=blocks).astype(np.float32)
        g[rs.rand(blocks) < 0.2] = 0.0
    return g


def _trace(lib):
    return lib.last_kernel(), lib.last_kernel_variant()


def _want(lib, e):
    name, _, var = e.partition("/")
    return getattr(lib, name), (None if not var else (0 if var == "0" else getattr(lib, var)))


def run_case(torch, BSMM, lib, mm, c):
    """Runs one case; returns (observations, failures): the trace of every pass and one line per violated statement."""
    obs, fails = {}, []
    td = getattr(torch, P.TORCH_DT[c.dt])
    lay = layouts(c.lay)
    opts = 0
    for o in c.opts:
        opts |= getattr(lib, o)
    lib.set_kernel_variant(c.variant)
    arena = GD.GuardArena(torch, "cuda")
    try:
        b = BSMM(lay, block_size=c.bs, feature_axis=c.axis, plan_options=opts, segmented=c.seg, updat_split=c.split)
        b.flow = c.flow
        t = orc.build_layout_luts(np.asarray(lay), c.bs)
        N = c.N
        W, X, E = P.make_inputs(b.w_shape, b.i_shape(N), b.o_shape(N), c.dt, seed=len(c.id) * 131 + N)
        Xs, Es = [X], [E]
        for p in range(1, c.pairs):
            _, Xp, Ep = P.make_inputs(b.w_shape, b.i_shape(N), b.o_shape(N), c.dt, seed=len(c.id) * 131 + N + 1000 * p)
            Xs.append(Xp); Es.append(Ep)
        w = arena.place(W, "w", c.mis, td)
        xs = [arena.place(a, "x%d" % p, c.mis, td) for p, a in enumerate(Xs)]
        es = [arena.place(a, "dy%d" % p, c.mis, td) for p, a in enumerate(Es)]
        G = gate = None
        if c.gate:
            G = _gate_values(b.blocks, c.gate, 7 + N)
            gate = arena.place(G, "gate")
        DW0 = dw0 = None
        if c.beta != 0.0:
            DW0 = orc.round_to(np.random.RandomState(5).normal(size=b.w_shape).astype(np.float32) * 0.05, c.dt)
            dw0 = arena.place(DW0, "dw", c.mis, td)
        W64 = np.asarray(W, dtype=np.float64) * (G.astype(np.float64)[:, None, None] if G is not None else 1.0)
        if G is not None and c.dt == "f16" and c.bs in b.GATE_IMAGES_MIN_N and N >= b.GATE_IMAGES_MIN_N[c.bs]:
            # fp16 over ONE weight image, whatever the gate: the operation is x . round_fp16(g w) -- the reference's own arithmetic (mul.rn.f16x2 on
            # the weight fragments, src/blocksparse_hgemm_cn_64_op_gpu.cu:104-110; blocksparse_amd/matmul.py::_gated_xprop) -- so that is what
            # the oracle multiplies, in float64
            W64 = orc.round_to((G[:, None, None] * np.asarray(W, dtype=np.float32)).astype(np.float32), "f16").astype(np.float64)
        outs = {}
        with GD.routed(arena, mm):
            if c.exp[0] is not None:
                outs["Y"] = b.fprop(xs[0], w, gate=gate); obs["fprop"] = _trace(lib)
            if c.exp[1] is not None:
                outs["DX"] = b.bprop(es[0], w, gate=gate); obs["bprop"] = _trace(lib)
            if c.exp[2] is not None:
                if c.mode == "sums":
                    sums = b.updat(xs, es, sums_only=True); obs["updat"] = _trace(lib)
                    outs["SUMS"] = sums
                    outs["DW"] = b.updat_finalize(sums, alpha=c.alpha, dtype=td)
                else:
                    outs["DW"] = b.updat(xs, es, alpha=c.alpha, beta=c.beta, dw=dw0, gate=gate); obs["updat"] = _trace(lib)
        torch.cuda.synchronize()
        obs["buffers"] = len(arena.entries)
        # (a) the family the case is there for
        for op, e in zip(("fprop", "bprop", "updat"), c.exp):
            if e is None:
                continue
            fam, var = _want(lib, e)
            if obs[op][0] != fam or (var is not None and obs[op][1] != var):
                fails.append("(a) %s ran trace %s, the case expects %s" % (op, obs[op], e))
        if F32S in c.exp and not any(n.startswith("_prepared:") for n in arena.names()):
            fails.append("(a) no prepared weight pieces (bsmm_prepare_weights) among the buffers: %s" % arena.names())
        # (b) guards
        for name, side, first, count in arena.report():
            fails.append("(b) %s %s guard: %d byte(s) changed, nearest at %d" % (name, side, count, first))
        # (c) every element stored, none from poison
        for name, out in outs.items():
            try:
                GD.assert_stored(torch, out, name)
            except GD.GuardError as err:
                fails.append("(c) " + str(err))
        # (d) the float64 oracle, tests/_parity.py's bars
        refs = {}
        if "Y" in outs:
            refs["Y"] = (orc.fprop_fast(t, X, W64, c.axis, dtype=np.float64), b.KB)
        if "DX" in outs:
            refs["DX"] = (orc.bprop_fast(t, E, W64, c.axis, dtype=np.float64), b.CB)
        if "DW" in outs:
            U = sum(orc.updat_fast(t, xp, ep, c.axis, dtype=np.float64) for xp, ep in zip(Xs, Es))
            if "SUMS" in outs:
                try:
                    P.assert_blocks(P.to_host(outs["SUMS"]), U, "f32", b.blocks, (c.id, "SUMS"))
                except AssertionError as err:
                    fails.append("(d) " + str(err))
            if G is not None:
                U = U * G.astype(np.float64)[:, None, None]
            refs["DW"] = (c.alpha * U + (c.beta * DW0.astype(np.float64) if DW0 is not None else 0.0), b.blocks)
        for name, (ref, nb) in refs.items():
            got = P.to_host(outs[name])
            if name != "DW":
                got, ref = P.act_blocks(got, c.axis, N, nb, c.bs), P.act_blocks(ref, c.axis, N, nb, c.bs)
            try:
                P.assert_blocks(got, ref, c.dt, nb, (c.id, name))
            except AssertionError as err:
                fails.append("(d) " + str(err)[:600])
    finally:
        lib.set_kernel_variant(0)
        arena.release()
    return obs, fails


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matmul_memory_contract(env, case):
    torch, BSMM, lib, mm = env
    obs, fails = run_case(torch, BSMM, lib, mm, case)
    assert obs["buffers"] > 0
    assert not fails, "%s: %s\n  " % (case.id, obs) + "\n  ".join(fails)


# ---- the other allocating operators of BlocksparseMatMul: gate_grad, l2_normalize and its gradient, identity_init ----------------
AUX = [(32, "bf16", "r37x53"), (32, "f32", "holes"), (16, "f16", "holes"), (16, "f32", "r66x70"), (8, "bf16", "holes"), (8, "f32", "r36x52"),
       (32, "f16", "one"), (64, "bf16", "holes")]


def _collect(fails, fn, *a):
    try:
        fn(*a)
    except AssertionError as err:
        fails.append(str(err)[:600])


@pytest.mark.parametrize("bs,dt,lay", AUX, ids=["b%d-%s-%s" % a for a in AUX])
def test_aux_ops_memory_contract(env, bs, dt, lay):
    """gate_grad, l2_normalize (with a gain) and its gradient, identity_init: guards, every element stored, and the values against the float64
    oracle at the bars tests/test_l2norm.py and tests/test_gating.py hold them to."""
    torch, BSMM, lib, mm = env
    td = getattr(torch, P.TORCH_DT[dt])
    layout = layouts(lay)
    b = BSMM(layout, block_size=bs, feature_axis=1 if bs == 64 else 0)
    t = orc.build_layout_luts(np.asarray(layout), bs)
    rs = np.random.RandomState(bs + len(lay))
    W = orc.round_to(rs.normal(size=b.w_shape).astype(np.float32), dt)
    U = orc.round_to(rs.normal(size=b.w_shape).astype(np.float32), dt)
    G = _gate_values(b.blocks, "general", 3)
    gain = rs.uniform(0.5, 1.5, b.K).astype(np.float32)
    arena = GD.GuardArena(torch, "cuda")
    fails = []
    w, u = arena.place(W, "w", 0, td), arena.place(U, "u", 0, td)
    gate, tgain = arena.place(G, "gate"), arena.place(gain, "gain")
    bar = max(P.L2_BAR[dt], 2e-6)
    with GD.routed(arena, mm):
        dwg, dg = b.gate_grad(u, w, gate)
        if bs != 64:
            y, ss = b._l2_fwd(w, tgain, 1e-12, td)
            dx, dgain = b._l2_bwd(u, w, tgain, ss, 1e-12)
        ident = b.identity_init(0.5)(dtype=td, device="cuda")
    torch.cuda.synchronize()
    assert len(arena.entries) >= 4 + (3 if bs == 64 else 7)
    _collect(fails, arena.check)
    outs = [("gate_grad dw", dwg), ("gate_grad dg", dg), ("identity", ident)] + ([("l2 y", y), ("l2 sums", ss), ("l2 dx", dx), ("l2 dgain", dgain)] if bs != 64 else [])
    for name, out in outs:
        _collect(fails, GD.assert_stored, torch, out, name)
    rdw, rdg = orc.gate_grad(U, W, G)
    checks = [("gate_grad dw", P.to_host(dwg), orc.round_to(rdw, dt), bar), ("gate_grad dg", P.to_host(dg), rdg, bar),
              ("identity", P.to_host(ident), orc.identity_init(t, 0.5), 0.0)]
    if bs != 64:
        Y, S = orc.l2_normalize(t, W, gain=gain)
        D, DG = orc.l2_normalize_grad(t, W, U, gain=gain)
        checks += [("l2 y", P.to_host(y), orc.round_to(Y, dt), bar), ("l2 sums", P.to_host(ss), S, 2e-6), ("l2 dx", P.to_host(dx), orc.round_to(D, dt), bar),
                   ("l2 dgain", P.to_host(dgain), DG, 2e-6 if dt == "f32" else bar)]
    for name, got, ref, tol in checks:
        l2, _ = P.errors(got, ref)
        if not l2 <= tol:                      # (NaN or Inf in `got`: l2 is nan / inf and this fails too)
            fails.append("%s: L2 %.3e > %.1e" % (name, l2, tol))
    arena.release()
    assert not fails, "\n  ".join(fails)
