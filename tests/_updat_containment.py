"""Containment of non-finite activations in the WEIGHT GRADIENT, and its gate rule: the case table, the poison, the expected classes, a
float64 walk with the reference's skip, and models of two defects (mutants).  Shared by tests/test_updat_containment_host.py (no GPU: the
conditions of every case, the class arithmetic against the walk, both mutants caught) and tests/test_updat_containment_gpu.py (the
kernels).  NumPy only.  The fprop / bprop half of the contract is tests/_containment.py; its layouts and gate values are reused here.

The property.  Block w = (c, k) of the layout, bs the block size, p the (x, dy) pair:
    DW[w][i][j] is non-finite  iff  block w is not gated off and some pair p and minibatch index n exist with X_p[n, c bs + i] or
    DY_p[n, k bs + j] non-finite -- and then it has the class (+Inf, -Inf, NaN) that a float64 walk of the unsplit products gives.
    A block with gate[w] == 0 contributes NOTHING, whatever X and DY hold: DW[w] = beta DW0[w] rounded once; with beta == 0 that is +0
    everywhere and DW0 is not read.  (Reference: blocksparse/matmul.py:416-418 `if gate[w] != 0.0`; src/blocksparse_hgemm_cn_64_op_gpu.cu:
    737-739,874-875 `if (gate != 0.0f) {...} else if (!accumulate) zero`.  gate_grad -- dw g, dg = sum dw w -- multiplies in the reference
    too and is not part of this contract.)
    Every other element is finite and has the clean call's bits -- except on a route that sums through atomics or answers a poisoned call
    with a repair pass (`bitwise` False): there it meets statement (1) of _parity.block_report against the float64 walk.

The poison.  Every case makes two poisoned calls, one with the poison in X, one with it in DY:
    +Inf at minibatch index N - 1 (the LAST: the streaming and windowed kernels re-read row N - 1 for the rows past N and zero them in LDS)
         in feature I1 of block c1 (DY: k1), in pair 0 -- the pair boundary of a multi-pair call;
    NaN  at minibatch index 0 in feature I2 of block c2 (k2), in the last pair of three (pair min(2, pairs - 1)).
c1's block row (k1's block column) has at least two blocks; in gated cases one of them has gate 0 and one a gate != 0, and one more gate-0
block lies outside the poisoned rows and columns.  For bsize 8 another 8-block of c1's 32-feature group has blocks too (the super-block
sums of the bsize-8 path hold their products with c1).  The PARTNER operand's values at the two poisoned minibatch indices have magnitude
>= 2^-10 (redrawn until they do): +-Inf times a normal number, so the class cannot depend on how a matrix core treats fp16 subnormals.

beta is a power of two wherever it is not 0: beta DW0 is exact in fp32, so "rounded once" has one meaning."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _containment as CT
import _parity as P
from blocksparse_amd import _lib as L
from oracle import bsmm_oracle as O

MUTANTS = ("gate as a multiplier", "one-sided tail")
GENERAL_GATES = CT.GENERAL_GATES
FIN, PINF, NINF, NAN = 0, 1, 2, 3
I1, I2 = CT.I1, CT.I2             # feature (inside its block) of the Inf and of the NaN
PARTNER_MIN = 2.0 ** -10
CUS = 256                         # the compute units the dispatch conditions below are evaluated for
UTS_NMAX, UAW_NMAX = 768, 128     # csrc/bsmm_updat_dispatch.h (tests/test_memory_bounds_table.py holds these numbers against the source)
N_AXIS = {0: (72, 264, 776), 1: (40, 75, 264, 776)}     # all ragged against chunks of 16 / 32 / 64


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def _direct():
    """window (0, 0) crowded beyond what its 16 waves hold: the streaming plan gets direct blocks (tests/test_memory_bounds_gpu.py::layouts)"""
    lay = P.random_layout(33, 17, 0.22, seed=9)
    rng = np.random.default_rng(10)
    free = np.argwhere(lay[:16, :16] == 0)
    for i in rng.permutation(len(free))[:25]:
        lay[free[i][0], free[i][1]] = 1
    return lay


def _odd(lay):
    """the same layout with an odd number of blocks (the bsize-8 pair kernel's last pair then has no partner)"""
    lay = np.array(lay)
    if int((lay != 0).sum()) % 2 == 0:
        r, c = np.argwhere(lay == 0)[0]
        lay[r, c] = 1
    return lay


LAYOUTS = dict(CT.LAYOUTS)
LAYOUTS["direct"] = _direct()
LAYOUTS["odd12x10"] = _odd(CT.LAYOUTS["r12x10"])
for _l in LAYOUTS.values():
    _l.flags.writeable = False


@functools.lru_cache(maxsize=None)
def luts(lkey, bs):
    return O.build_layout_luts(LAYOUTS[lkey], bs)


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
def _case(route, lay, bs, axis, dtype, N, variant, code, chunk, **o):
    """route: the URoute of csrc/bsmm_updat_dispatch.h the case is there for; variant: _lib.set_kernel_variant (0 production, 1 V_FMA, 2 no
    plan, 3 plan forced); code / kv: the BSMM_K_* trace code and the BSMM_KV_* variant every call of the case must report; chunk: the
    minibatch entries per step of the route's kernel (N is ragged against it).  Options:
      pairs, alpha, beta   the call (beta != 0: DW0 holds ordinary finite values)
      gate                 None / "binary" / "general"
      opts                 names of _lib.PLAN_* bits;  split: BlocksparseMatMul(updat_split=)
      mode                 "dw", or "sums": updat(sums_only=True) followed by updat_finalize(gate=...)
      unaligned_dw         dw one element into a fresh allocation
      bitwise = False      finite elements of a poisoned call are NOT the clean call's bits: fp32 atomics (a split minibatch of the windowed
                           kernel) or a repair pass (the fp32 split routes: the per-block fp32 kernel rewrites DW when their flag is set)
      k_first              block columns to try first for k1 (the "direct" layout: columns that hold direct blocks of the streaming plan --
                           block row 0, the first choice for c1, holds some already; the host tier checks both against the plan)
      cond                 K_UPDAT_BLOCK is reported by three routes: which one the dispatch rules select (dispatch_kind below)"""
    c = dict(route=route, lay=lay, bs=bs, axis=axis, dtype=dtype, N=N, variant=variant, code=code, kv=None, chunk=chunk, pairs=1, alpha=1.0,
             beta=0.0, gate=None, opts=(), split=0, mode="dw", unaligned_dw=False, bitwise=True, cond=None, k_first=())
    tag = o.pop("tag", None)
    c.update(o)
    c["id"] = "-".join(str(x) for x in (route, lay, "b%d" % bs, "a%d" % axis, dtype, "N%d" % N, "p%d" % c["pairs"], c["gate"], tag) if x is not None)
    return c


def _cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    K = L
    # V_FMA kernel (chunks of 64): every bsize, both axes, bf16 and fp32; one production call with an unaligned dw
    for i, (bs, axis, dtype) in enumerate((b, a, d) for b in (32, 16, 8) for a in (0, 1) for d in ("bf16", "f32")):
        gate = (None, "general", "binary")[i % 3]
        add("valu", "r12x10", bs, axis, dtype, (40, 75)[i % 2] if axis else 72, 1, K.K_UPDAT_VALU, 64, gate=gate,
            **({"alpha": 0.5, "beta": 2.0} if i % 4 == 1 else {}))
    add("valu", "r12x10", 32, 1, "bf16", 40, 0, K.K_UPDAT_VALU, 64, gate="general", alpha=0.5, beta=2.0, unaligned_dw=True, tag="unaligned-dw")
    # per-block four-wave kernels, without a plan (a wave's step: 32 minibatch entries, 16 for bsize 16 in fp32)
    add("block4", "r12x10", 32, 0, "bf16", 72, 2, K.K_UPDAT_BLOCK, 32, gate="general", cond="block4")
    add("block4", "r12x10", 32, 0, "f16", 264, 2, K.K_UPDAT_BLOCK, 32, cond="block4", pairs=3, alpha=0.5, beta=2.0)
    add("block4", "r12x10", 16, 0, "bf16", 776, 2, K.K_UPDAT_BLOCK, 32, gate="binary", cond="block4")
    add("block4", "r12x10", 16, 0, "f16", 72, 2, K.K_UPDAT_BLOCK, 32, cond="block4")
    add("block4", "r12x10", 32, 1, "f32", 40, 2, K.K_UPDAT_BLOCK, 32, gate="general", cond="block4")
    add("block4", "r12x10", 32, 0, "f32", 72, 2, K.K_UPDAT_BLOCK, 32, cond="block4")
    add("block4", "r12x10", 16, 1, "f32", 75, 2, K.K_UPDAT_BLOCK, 16, gate="binary", cond="block4", alpha=2.0, beta=0.5)
    add("block4", "r12x10", 16, 0, "f32", 264, 2, K.K_UPDAT_BLOCK, 16, gate="general", cond="block4")
    # (the only way a 16-bit call on feature axis 1 gets there: gated -- the transposing-read kernel has no gate -- and past UTS_NMAX)
    add("block4", "r12x10", 32, 1, "bf16", 776, 2, K.K_UPDAT_BLOCK, 32, gate="general", cond="block4")
    # one wave per block on feature axis 0 (production; steps of 16 / 32 columns): N pairs on both sides of UAW_NMAX / 2 (bsize 32), UAW_NMAX (bsize 16)
    # (bsize 32 below its limit of 64: N = 40 -- every N of N_AXIS[0] is above it.  bsize 16: gated, so that the windowed kernel is out.)
    add("wave_a0", "r12x10", 32, 0, "bf16", 40, 0, K.K_UPDAT_BLOCK, 16, gate="general", cond="wave_a0")
    add("wave_a0", "r12x10", 32, 0, "f16", 40, 0, K.K_UPDAT_BLOCK, 16, cond="wave_a0", alpha=0.5, beta=2.0)
    add("wave_a0", "r12x10", 32, 0, "bf16", 72, 0, K.K_UPDAT_BLOCK, 32, gate="general", cond="block4", tag="past")
    add("wave_a0", "r12x10", 16, 0, "bf16", 72, 0, K.K_UPDAT_BLOCK, 32, gate="binary", cond="wave_a0")
    add("wave_a0", "r12x10", 16, 0, "f16", 72, 0, K.K_UPDAT_BLOCK, 32, gate="general", cond="block4", pairs=2, tag="past")
    # bsize-8 pair kernel (production, feature axis 0; 32 columns per step): an odd block count
    add("pairs8", "odd12x10", 8, 0, "bf16", 72, 0, K.K_UPDAT_BLOCK, 32, gate="general", cond="pairs8")
    add("pairs8", "odd12x10", 8, 0, "f16", 264, 0, K.K_UPDAT_BLOCK, 32, cond="pairs8", alpha=0.5, beta=2.0)
    # one-wave transposing kernel (bsize 32, feature axis 1, N pairs <= UTS_NMAX, no plan)
    add("one_wave_tr", "r12x10", 32, 1, "f16", 40, 2, K.K_UPDAT_BLOCK_TR, 32, kv=K.KV_ONE_WAVE)
    add("one_wave_tr", "r12x10", 32, 1, "bf16", 75, 2, K.K_UPDAT_BLOCK_TR, 32, kv=K.KV_ONE_WAVE, gate="binary")
    add("one_wave_tr", "r12x10", 32, 1, "bf16", 264, 2, K.K_UPDAT_BLOCK_TR, 32, kv=K.KV_ONE_WAVE, gate="general", alpha=0.5, beta=2.0)
    # transposing-read kernel: bsize 32 past UTS_NMAX, bsize 16
    add("block_tr", "r12x10", 32, 1, "bf16", 776, 2, K.K_UPDAT_BLOCK_TR, 32, kv=0)
    add("block_tr", "r12x10", 16, 1, "bf16", 75, 2, K.K_UPDAT_BLOCK_TR, 32, kv=0)
    add("block_tr", "r12x10", 16, 1, "f16", 264, 2, K.K_UPDAT_BLOCK_TR, 32, kv=0, pairs=3, alpha=0.5, beta=2.0)
    # windowed bsize 16 (chunks of 64): both axes, one part and a forced split of 2 (fp32 atomics into the workspace: not bitwise)
    add("win16", "r48", 16, 1, "bf16", 75, 3, K.K_UPDAT16_WIN, 64, split=1)
    add("win16", "r48", 16, 1, "f16", 264, 3, K.K_UPDAT16_WIN, 64, split=2, bitwise=False, tag="split2")
    add("win16", "r48", 16, 0, "bf16", 72, 3, K.K_UPDAT16_WIN, 64, split=1, opts=("PLAN_UPDAT16_WINDOWED",), pairs=3, alpha=0.5, beta=2.0)
    add("win16", "r48", 16, 0, "bf16", 264, 3, K.K_UPDAT16_WIN, 64, split=2, opts=("PLAN_UPDAT16_WINDOWED",), bitwise=False, tag="split2")
    # row owner bsize 16 (feature axis 0, chunks of 64): one part, two parts, gated (its finalize pass applies the gate)
    add("rows16", "r48", 16, 0, "bf16", 72, 3, K.K_UPDAT16_ROWS, 64, split=1)
    add("rows16", "r48", 16, 0, "f16", 264, 3, K.K_UPDAT16_ROWS, 64, split=2, tag="split2")
    add("rows16", "r48", 16, 0, "bf16", 264, 3, K.K_UPDAT16_ROWS, 64, gate="general")
    add("rows16", "r48", 16, 0, "f16", 776, 3, K.K_UPDAT16_ROWS, 64, gate="binary", alpha=0.5, beta=2.0)
    # streaming kernel (chunks of 16 rows on feature axis 1, 32 columns on feature axis 0)
    for axis, N in ((1, 264), (0, 264)):
        ch = 16 if axis else 32
        add("stream", "r48", 32, axis, "bf16", N, 3, K.K_UPDAT_STREAM, ch, split=1, tag="stored")          # every item one workgroup's: stored directly
        add("stream", "r48", 32, axis, "bf16", N, 3, K.K_UPDAT_STREAM, ch, tag="sums")                     # the default here: partial sums + the summing pass
        add("stream", "r48", 32, axis, "f16" if axis else "bf16", N, 3, K.K_UPDAT_STREAM, ch, gate="general" if axis else "binary", alpha=0.5, beta=2.0)
    add("stream", "r48", 32, 1, "bf16", 75, 3, K.K_UPDAT_STREAM, 16, split=2, tag="split2")
    add("stream", "r48", 32, 1, "bf16", 40, 3, K.K_UPDAT_STREAM, 16, gate="binary")
    add("stream", "r48", 32, 0, "f16", 72, 3, K.K_UPDAT_STREAM, 32, gate="general")
    add("stream", "r48", 32, 1, "bf16", 75, 3, K.K_UPDAT_STREAM, 16, pairs=3, alpha=0.5, beta=-1.0)
    add("stream", "direct", 32, 1, "bf16", 264, 3, K.K_UPDAT_STREAM, 16, k_first=(13,), tag="direct-blocks")
    add("stream", "direct", 32, 1, "bf16", 264, 3, K.K_UPDAT_STREAM, 16, gate="general", k_first=(13,), tag="direct-blocks")
    add("stream", "r48", 32, 1, "bf16", 264, 3, K.K_UPDAT_STREAM, 16, mode="sums", gate="general", alpha=0.5, beta=2.0, tag="finalize")
    add("stream", "r48", 32, 0, "bf16", 72, 3, K.K_UPDAT_STREAM, 32, mode="sums", gate="binary", tag="finalize")
    # bsize 8 through the streaming kernel over 32 x 32 super-blocks; a gated bsize-8 call leaves that path
    add("super8", "s64", 8, 1, "bf16", 264, 3, K.K_UPDAT_SUPER8, 16)
    add("super8", "s64", 8, 0, "f16", 264, 3, K.K_UPDAT_SUPER8, 32, alpha=0.5, beta=2.0)
    add("gated-b8", "s64", 8, 1, "bf16", 75, 3, K.K_UPDAT_VALU, 64, gate="general")
    add("gated-b8", "s64", 8, 0, "f16", 72, 3, K.K_UPDAT_VALU, 64, gate="binary")
    # bsize 64 on feature axis 1, gated: the quadrants go through the streaming kernel or the one-wave kernel, the gate is the 64-block's
    add("b64", "r10x12", 64, 1, "bf16", 264, 3, K.K_UPDAT_STREAM, 16, gate="general")
    add("b64", "r10x12", 64, 1, "bf16", 75, 3, K.K_UPDAT_STREAM, 16, gate="binary", alpha=0.5, beta=2.0)
    add("b64", "r10x12", 64, 1, "bf16", 40, 0, K.K_UPDAT_BLOCK_TR, 32, kv=K.KV_ONE_WAVE, gate="general")
    add("b64", "r10x12", 64, 1, "f16", 40, 0, K.K_UPDAT_BLOCK_TR, 32, kv=K.KV_ONE_WAVE, gate="binary", alpha=0.5, beta=2.0)
    # the three fp32 routes through six bf16 piece pairs, gated: a poisoned call raises their flag and the per-block fp32 kernel writes DW
    add("f32split", "r48", 32, 1, "f32", 264, 0, K.K_UPDAT_STREAM, 16, gate="general", bitwise=False, alpha=0.5, beta=0.25)
    add("f32split", "r48", 16, 1, "f32", 264, 0, K.K_UPDAT16_WIN, 64, gate="general", bitwise=False)
    add("f32split", "r48", 16, 0, "f32", 264, 3, K.K_UPDAT16_ROWS, 64, gate="binary", bitwise=False, alpha=2.0, beta=0.5)
    for i, c in enumerate(out):
        c["seed"] = 9000 + i
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
ROUTES = ("valu", "block4", "wave_a0", "pairs8", "one_wave_tr", "block_tr", "win16", "rows16", "stream", "super8", "gated-b8", "b64", "f32split")
# the cases the mutants are NAMED on (tests/test_updat_containment_host.py checks every case a mutant applies to; these must be among them)
NAMED = {
    MUTANTS[0]: ("stream-r48-b32-a1-f16-N264-p1-general", "rows16-r48-b16-a0-bf16-N264-p1-general", "b64-r10x12-b64-a1-bf16-N264-p1-general",
                 "pairs8-odd12x10-b8-a0-bf16-N72-p1-general", "f32split-r48-b32-a1-f32-N264-p1-general"),
    MUTANTS[1]: ("stream-r48-b32-a1-bf16-N264-p1-sums", "win16-r48-b16-a1-bf16-N75-p1", "super8-s64-b8-a0-f16-N264-p1", "stream-r48-b32-a0-bf16-N264-p1-stored"),
}


def dispatch_kind(c):
    """Which of the three routes that report K_UPDAT_BLOCK the rules of csrc/bsmm_updat_dispatch.h::updat_path select for the case's numbers
    ("block4": updat32_kernel / updat16_kernel; "wave_a0": updat_a0_wave_kernel; "pairs8": updat8_a0_pairs_kernel), or None where they select
    another kernel.  Operands are 16-byte aligned, no split is named, CUS compute units."""
    bs, axis, N, rows, v = c["bs"], c["axis"], c["N"], c["N"] * c["pairs"], c["variant"]
    is16, gated = c["dtype"] != "f32", c["gate"] is not None
    blocks = luts(c["lay"], bs)["blocks"]
    if v == 1 or c["split"] or c["mode"] != "dw" or c["unaligned_dw"]:
        return None
    if axis == 0 and N % (8 if is16 else 4):
        return None
    if bs == 8:
        # the pair kernel: 6 + 3.4e-6 us per (block, column) against at least 30 us for the super-block path
        return "pairs8" if is16 and axis == 0 and v == 0 and 6.0 + 3.4e-6 * blocks * rows < 30.0 else None
    if not is16:
        return "block4" if v == 2 else None          # (fp32 with a plan: the split routes where they apply)
    if v == 2:                                       # no plan: the windowed, row-owner and streaming kernels are out
        if axis == 0:
            return "block4"
        if bs == 32:
            return "block4" if gated and rows > UTS_NMAX else None      # (else the one-wave or the transposing-read kernel)
        return "block4" if gated else None
    if v == 0 and axis == 0:
        if bs == 32 and not 7.0 + 1.37e-5 * blocks * rows < 45.0:       # the streaming kernel, unless the per-block estimate stays under 45 us
            return None
        if bs == 16:
            # ungated: the windowed kernel.  Gated: the row-owner kernel where it pays -- never with fewer than 8 chunks of 64 columns
            if not gated or c["pairs"] * -(-N // 64) >= 8:
                return None
        return "wave_a0" if rows <= (UAW_NMAX // 2 if bs == 32 else UAW_NMAX) else "block4"
    return None


# ---- the poisoned blocks and the gate -----------------------------------------------------------------------------------------------------
def _pick_line(lay, bs, avoid=(), first=()):
    """(line of the Inf, line of the NaN) among the rows of `lay` ([line][other side]): the first line (of `first`, then of all) with at least
    two blocks (bsize 8: and another line of its group of four with blocks), a line from the middle of the others"""
    n = lay.shape[0]
    for a in list(first) + list(range(n)):
        if a in avoid or lay[a].sum() < 2:
            continue
        if bs == 8 and not any(lay[q].any() for q in CT.partners(a, 8, n)):
            continue
        others = [q for q in range(n) if q != a and lay[q].any() and (bs != 8 or q // 4 != a // 4)]
        if others:
            return a, others[len(others) // 2]
    raise AssertionError("no line with two blocks in this layout")


@functools.lru_cache(maxsize=None)
def setup(cid):
    """{c1, c2, k1, k2, pn (pair of the NaN), gate (float32 [blocks] or None), off_x / on_x / off_dy / on_dy / off_out (the blocks whose gate
    is forced: in c1's row, in k1's column, outside every poisoned line)}"""
    c = BY_ID[cid]
    t, bs = luts(c["lay"], c["bs"]), c["bs"]
    lay = LAYOUTS[c["lay"]] != 0
    wid = {ck: w for w, ck in enumerate(t["updat_list"])}
    c1, c2 = _pick_line(lay, bs)
    s = None
    avoid = []
    while s is None:
        k1, k2 = _pick_line(lay.T, bs, tuple(avoid), c["k_first"])
        ks, cs = np.nonzero(lay[c1])[0], np.nonzero(lay[:, k1])[0]
        off, on = {(c1, int(ks[0])), (int(cs[0]), k1)}, {(c1, int(ks[-1])), (int(cs[-1]), k1)}
        if off & on:
            avoid.append(k1)
            continue
        s = dict(c1=c1, c2=c2, k1=k1, k2=k2, pn=min(2, c["pairs"] - 1), off_x=wid[(c1, int(ks[0]))], on_x=wid[(c1, int(ks[-1]))],
                 off_dy=wid[(int(cs[0]), k1)], on_dy=wid[(int(cs[-1]), k1)])
    outside = [w for w, (ci, ki) in enumerate(t["updat_list"]) if ci not in (c1, c2) and ki not in (k1, k2)]
    s["off_out"] = outside[len(outside) // 2]
    gate = None
    if c["gate"] is not None:
        rs = np.random.RandomState(c["seed"])
        if c["gate"] == "binary":
            gate = (rs.rand(t["blocks"]) < 0.75).astype(np.float32)
        else:
            gate = np.asarray(GENERAL_GATES[c["dtype"]], dtype=np.float32)[rs.randint(0, 5, t["blocks"])]
        gate[[s["off_x"], s["off_dy"], s["off_out"]]] = 0.0
        gate[[s["on_x"], s["on_dy"]]] = 1.0 if c["gate"] == "binary" else GENERAL_GATES[c["dtype"]][2]
        gate.flags.writeable = False
    s["gate"] = gate
    return s


def act_shape(c, n_blocks):
    return (c["N"], n_blocks * c["bs"]) if c["axis"] else (n_blocks * c["bs"], c["N"])


def at(c, a, n):
    """the feature vector of an activation at minibatch index n"""
    return a[n] if c["axis"] else a[:, n]


def poison(c, side, acts):
    """a copy of the list of X (side "x") or of DY ("dy") with the two poisoned elements"""
    s, bs, N = setup(c["id"]), c["bs"], c["N"]
    b1, b2 = (s["c1"], s["c2"]) if side == "x" else (s["k1"], s["k2"])
    acts = [np.array(a, dtype=np.float32, copy=True) for a in acts]
    f1, f2 = b1 * bs + I1, b2 * bs + bs + I2
    if c["axis"]:
        acts[0][N - 1, f1], acts[s["pn"]][0, f2] = np.inf, np.nan
    else:
        acts[0][f1, N - 1], acts[s["pn"]][f2, 0] = np.inf, np.nan
    for a in acts:
        a.flags.writeable = False
    return acts


def classes(a):
    """FIN / PINF / NINF / NAN per element"""
    a = np.asarray(a)
    return np.where(np.isnan(a), NAN, np.where(np.isposinf(a), PINF, np.where(np.isneginf(a), NINF, FIN))).astype(np.int8)


def expected_classes(c, side, Xs, Es, mutant=None):
    """The class of every element of DW under the poison on `side`: boolean and sign arithmetic on the layout, the gate and the partner's
    signs (Xs, Es: the CLEAN operands).  `mutant`: what a kernel with that defect would leave instead --
      gate as a multiplier: alpha gate[w] sum with gate[w] == 0 -- 0 Inf and 0 NaN are NaN in the gated-off blocks of the poisoned lines;
      one-sided tail: the rows past N zeroed in one operand only while the other keeps its clamped copy of row N - 1: Inf 0 = NaN joins the
      sum of every element the Inf reaches, wherever N is no multiple of the route's chunk."""
    s, bs, N = setup(c["id"]), c["bs"], c["N"]
    t = luts(c["lay"], bs)
    gate = s["gate"]
    out = np.zeros((t["blocks"], bs, bs), dtype=np.int8)
    b1, b2 = (s["c1"], s["c2"]) if side == "x" else (s["k1"], s["k2"])
    partner = at(c, (Es if side == "x" else Xs)[0], N - 1)          # the Inf sits in pair 0, at index N - 1
    for w, (ci, ki) in enumerate(t["updat_list"]):
        mine, other = (ci, ki) if side == "x" else (ki, ci)
        g = 1.0 if gate is None else float(gate[w])
        off = g == 0.0
        if off and mutant != MUTANTS[0]:
            continue
        blk = out[w] if side == "x" else out[w].T                   # [feature of the poisoned side][feature of the partner]
        if mine == b1:
            sign = np.sign(partner[other * bs:(other + 1) * bs]) * np.sign(c["alpha"] * g)
            assert off or (sign != 0).all()
            blk[I1, :] = NAN if off else np.where(sign > 0, PINF, NINF)
            if mutant == MUTANTS[1] and N % c["chunk"]:
                blk[I1, :] = NAN
        if mine == b2:
            blk[bs + I2, :] = NAN
    return out


# ---- inputs and the float64 walk ------------------------------------------------------------------------------------------------------------
def walk(c, Xs, Es, gate, DW0):
    """float64, block by block with the reference's skip (blocksparse/matmul.py:416-418 `if gate[w] != 0.0`): the operands of a skipped block
    are never touched.  alpha gate[w] is the fp32 product the kernels form."""
    t, bs, axis = luts(c["lay"], c["bs"]), c["bs"], c["axis"]
    U = np.zeros((t["blocks"], bs, bs))
    Xs = [np.asarray(a, dtype=np.float64) for a in Xs]
    Es = [np.asarray(a, dtype=np.float64) for a in Es]
    with np.errstate(invalid="ignore", over="ignore"):
        for w, (ci, ki) in enumerate(t["updat_list"]):
            g = 1.0 if gate is None else float(gate[w])
            if g == 0.0:
                continue
            for X, E in zip(Xs, Es):
                if axis:
                    U[w] += X[:, ci * bs:(ci + 1) * bs].T @ E[:, ki * bs:(ki + 1) * bs]
                else:
                    U[w] += X[ci * bs:(ci + 1) * bs] @ E[ki * bs:(ki + 1) * bs].T
            U[w] *= float(np.float32(c["alpha"]) * np.float32(g))
        if c["beta"] != 0.0:
            U += c["beta"] * np.asarray(DW0, dtype=np.float64)
    return U


def _partners_away_from_zero(rs, a, c):
    """redraw the values at minibatch indices 0 and N - 1 until every magnitude is >= PARTNER_MIN"""
    for n in (0, c["N"] - 1):
        v = at(c, a, n)
        while (np.abs(v) < PARTNER_MIN).any():
            bad = np.abs(v) < PARTNER_MIN
            v[bad] = O.round_to(rs.normal(0.0, 0.1, int(bad.sum())).astype(np.float16).astype(np.float32), c["dtype"])


@functools.lru_cache(maxsize=3)
def reference(cid):
    """Everything a test needs of a case, computed once: the operands (float32 arrays holding storage-type values), DW0 (None with
    beta == 0), the gate, the poisoned operand lists, the float64 walk of the CLEAN call, the expected classes and what the gate-0 blocks
    must hold.  Read-only."""
    c = BY_ID[cid]
    t, bs = luts(c["lay"], c["bs"]), c["bs"]
    s = setup(cid)
    rs = np.random.RandomState(c["seed"] + 17)
    Xs, Es = [], []
    for p in range(c["pairs"]):
        _, X, E = P.make_inputs((1, 1, 1), act_shape(c, t["CB"]), act_shape(c, t["KB"]), c["dtype"], c["seed"] + 1000 * p)
        _partners_away_from_zero(rs, X, c)
        _partners_away_from_zero(rs, E, c)
        Xs.append(X)
        Es.append(E)
    DW0 = None
    if c["beta"] != 0.0:
        DW0 = O.round_to(rs.normal(size=(t["blocks"], bs, bs)).astype(np.float32) * 0.05, c["dtype"])
    r = dict(Xs=Xs, Es=Es, DW0=DW0, gate=s["gate"], want64=walk(c, Xs, Es, s["gate"], DW0),
             x=dict(Xs=poison(c, "x", Xs), Es=Es, cls=expected_classes(c, "x", Xs, Es)),
             dy=dict(Xs=Xs, Es=poison(c, "dy", Es), cls=expected_classes(c, "dy", Xs, Es)))
    # a gate-0 block: +0 (beta == 0), else beta DW0 -- exact in fp32 for the powers of two used here -- rounded to the storage type
    r["off_values"] = (np.zeros((t["blocks"], bs, bs), dtype=np.float32) if DW0 is None else
                       O.round_to((np.float32(c["beta"]) * DW0).astype(np.float32), c["dtype"]))
    for v in Xs + Es + [r["want64"], r["x"]["cls"], r["dy"]["cls"], r["off_values"]] + ([DW0] if DW0 is not None else []):
        v.flags.writeable = False
    return r
