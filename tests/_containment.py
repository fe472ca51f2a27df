"""Containment of non-finite activations in fprop / bprop: the case table, the poison, the expected masks, a float64 walk with the
reference's skip, and mask models of kernels that would break the property (mutants).  Shared by tests/test_containment_host.py (no GPU:
the conditions of every case, the masks against the walk, every mutant caught) and tests/test_containment_gpu.py (the kernels).  NumPy only.

The property.  fprop and bprop read an activation block only through the entries of the layout, and an entry whose gate is 0 is skipped
(reference: blocksparse/matmul.py:353-399 `if gate[w] != 0.0`; src/blocksparse_hgemm_cn_64_op_gpu.cu:96-100 `if (gate != 0)`).  An Inf or
NaN in one element of X therefore reaches exactly the output blocks its feature block is connected to through a live entry, in its own
minibatch row (feature axis 1) or column (feature axis 0), and nothing else.  A whole-tensor L2 on Gaussian data cannot see a violation.

The poison (fprop: in X; bprop: the same in DY, on the transposed layout): two single elements,
  +Inf at minibatch index N - 1 in feature block c1 (the LAST index: a kernel that clamps the rows past N onto row N - 1 re-reads it),
  NaN  at minibatch index 0     in feature block c2.
c1 is chosen so that some output block has c1's PARTNER connected and c1 itself not -- the partner is c1 ^ 1 (the other half of a K = 32
matrix-core step for bsize 16, of a pair step for bsize 32), for bsize 8 another block of c1's 32-feature group (the same super-block row) --
and, in gated cases, so that another output block is connected to c1 only through an entry whose gate is 0.  Every gate-0 weight block holds NaN.

Where the layout allows it c1 is block 0 (every layout here but one pass of one): the block a kernel would read if the unused half of an odd
list's last K-concatenated step kept the default entry (0, 0) with zero weights instead of zero activations.

The expected mask is boolean arithmetic on the layout: output element (n, block k, any o) is non-finite iff n is a poisoned index and its
poisoned block has an entry to k whose gate is absent or != 0.

General gates.  fp16 cases draw them from {0, 1, -0.5, 2, 0.25}: an fp16 call over weight images multiplies with round_fp16(g w) (ONE image:
the reference's own arithmetic, mul.rn.f16x2), which is exact for these gates, so that _parity's criterion -- the float64 sum rounded once --
applies to it unchanged.  bf16 / fp32 cases draw from {0, 1, -0.5, 1.75, 0.3} (bf16 over images: two pieces, g w to 2^-17)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _parity as P
from blocksparse_amd import _lib as L
from oracle import bsmm_oracle as O

MUTANTS = ("zero fragment against an absent partner", "gate as a multiplier", "poisoned row leaks into its clamped re-read neighbour",
           "odd tail's zero fragment against block 0")
GENERAL_GATES = {"f16": (0.0, 1.0, -0.5, 2.0, 0.25), "bf16": (0.0, 1.0, -0.5, 1.75, 0.3), "f32": (0.0, 1.0, -0.5, 1.75, 0.3)}
I1, I2 = 3, -1                    # feature (inside its block) of the Inf and of the NaN
FLOW_RT4_CUS = 256                # the compute units the RT = 4 flow case is sized for (units of 128 rows >= CUs: csrc launch_xflow)
IMAGES_MIN_N = {32: 1024, 16: 1024}     # BlocksparseMatMul.GATE_IMAGES_MIN_N of the image cases (bsize 16: lowered, as tests/test_gating.py does)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def _heavy(CB, KB, dens, seed, col, row, holes):
    """random + one nearly full column and one nearly full row (`holes` of their cells stay empty)"""
    lay = P.random_layout(CB, KB, dens, seed)
    rs = np.random.RandomState(seed)
    lay[:, col] = 1
    lay[rs.permutation(CB)[:holes[0]], col] = 0
    lay[row, :] = 1
    lay[row, rs.permutation(KB)[:holes[1]]] = 0
    lay[row, col] = 1
    return lay


LAYOUTS = {
    "r12x10": P.random_layout(12, 10, 0.35, 71),            # V_FMA, per-segment, in-kernel gates, fp32 split without the XCD map
    "r10x12": P.random_layout(10, 12, 0.35, 72),            # bsize 64
    "small24": _heavy(24, 24, 0.15, 73, 3, 5, (3, 4)),      # small-minibatch kernels: lists with odd and even counts, one longer than 16
    "locks24x12": _heavy(24, 12, 0.12, 74, 2, 4, (2, 1)),   # segmented = True: output blocks shared by several segments
    "r48": P.random_layout(48, 48, 0.12, 75),               # mid, staged, flow (64-row units), bsize-16 list kernel, weight images
    "flow12x48": P.random_layout(12, 48, 0.15, 76),         # flow with 128-row units (fprop: 3 groups x 87 row tiles)
    "d20x16": P.random_layout(20, 16, 0.5, 77),             # bsize-16 pair kernel: density >= 0.4
    "w12x128": P.random_layout(12, 128, 0.15, 78),          # fp32 split, fprop: 8 groups of 16 output blocks (one group per XCD at a time)
    "s64": P.random_layout(64, 64, 0.12, 79),               # bsize 8 in 32 x 32 super-blocks
}
for _l in LAYOUTS.values():
    _l.flags.writeable = False


@functools.lru_cache(maxsize=None)
def luts(lkey, bs):
    return O.build_layout_luts(LAYOUTS[lkey], bs)


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
def _case(route, lay, bs, axis, dtype, N, variant, code, gate=None, **opts):
    """variant: _lib.set_kernel_variant (0 production, 1 V_FMA, 2 no plan, 3 plan forced, 4 mid forced); code: the BSMM_K_* trace code both
    passes must report (None with code_from_ungated: whatever the ungated call of the same operator reports).  opts:
      passes          ("fprop", "bprop") unless the route exists for one only
      kv              {pass: BSMM_KV_* variant inside the family}
      bitwise = False finite elements of the poisoned call are NOT the clean call's bits: fp32 lock accumulators (atomic order) or a repair pass
                      (another kernel rewrites the output) -- they meet statement (1) of _parity.block_report instead
      segmented, flow, unaligned, images: how the operator / the call is set up (tests/test_containment_gpu.py::_operator)"""
    c = dict(route=route, lay=lay, bs=bs, axis=axis, dtype=dtype, N=N, variant=variant, code=code, gate=gate,
             passes=("fprop", "bprop"), kv=None, bitwise=True, segmented=False, flow=True, unaligned=False, images=False, code_from_ungated=False)
    c.update(opts)
    c["id"] = "%s-%s-b%d-a%d-%s-N%d%s%s" % (route, lay, bs, axis, dtype, N, "-" + gate if gate else "", "-" + opts["tag"] if "tag" in opts else "")
    return c


def _cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))
    # V_FMA kernels
    for bs in (32, 16, 8):
        for axis in (0, 1):
            for dtype in ("bf16", "f32"):
                add("valu", "r12x10", bs, axis, dtype, 40, 1, L.K_XPROP_VALU)
    add("valu", "r12x10", 32, 1, "bf16", 40, 0, L.K_XPROP_VALU, unaligned=True, tag="unaligned")      # production dispatch, X two bytes off
    # per-segment kernels: NSUB 1 / 2 (bsize 32: N < / >= 2048), 1 / 2 / 4 (bsize 16: N < 512 / < 2048 / >= 2048)
    for bs, Ns in ((32, (40, 2056)), (16, (40, 520, 2056))):
        for N in Ns:
            for axis in (0, 1):
                for dtype in ("bf16", "f16", "f32"):
                    add("segment", "r12x10", bs, axis, dtype, N, 2, L.K_XPROP_SEGMENT)
    for dtype in ("bf16", "f32"):
        add("segment", "locks24x12", 32, 1, dtype, 40, 2, L.K_XPROP_SEGMENT, segmented=True, bitwise=False, tag="locks")
    # the five small-minibatch kernels (production dispatch)
    for dtype in ("bf16", "f16"):
        for bs in (32, 16, 8):
            add("small", "small24", bs, 1, dtype, 40, 0, L.K_XPROP_SMALL)
            # (bsize 16 on feature axis 1: bprop leaves the narrow kernel above 64 rows, fprop above 256 -- xprop_route)
            add("small", "small24", bs, 1, dtype, 70, 0, L.K_XPROP_SMALL, **({"passes": ("fprop",)} if bs == 16 else {}))
            add("small", "small24", bs, 0, dtype, 72, 0, L.K_XPROP_SMALL)
    # the mid kernel: one block x 4 row chunks per workgroup (N C 2 <= 5 MiB), 4 blocks x one chunk above
    for dtype in ("bf16", "f16"):
        for N in (130, 1736):
            add("mid", "r48", 32, 1, dtype, N, 4, L.K_XPROP_MID)
    # forced plan kernels
    add("staged", "r48", 32, 0, "bf16", 264, 3, L.K_XCOL32_STAGED)
    add("staged", "r48", 32, 1, "bf16", 264, 3, L.K_XCOL32_STAGED, flow=False)
    add("flow", "r48", 32, 1, "bf16", 264, 3, L.K_XCOL32_FLOW, kv={"fprop": L.KV_FLOW_HALF_UNITS, "bprop": L.KV_FLOW_HALF_UNITS})
    add("flow", "flow12x48", 32, 1, "bf16", 128 * ((FLOW_RT4_CUS + 2) // 3) + 8, 3, L.K_XCOL32_FLOW, kv={"fprop": 0, "bprop": L.KV_FLOW_HALF_UNITS})
    add("list16", "r48", 16, 0, "bf16", 264, 3, L.K_XCOL16_STAGED)
    add("list16", "r48", 16, 1, "bf16", 264, 3, L.K_XCOL16_STAGED)
    for dtype in ("bf16", "f16"):
        add("pair16", "d20x16", 16, 1, dtype, 264, 3, L.K_XCOL16_STAGED)
    add("f32split", "w12x128", 32, 1, "f32", 520, 3, L.K_XCOL32_F32SPLIT)        # fprop: 8 groups, 5 row tiles -> one group per XCD; bprop: one group
    add("f32split", "r12x10", 32, 1, "f32", 264, 3, L.K_XCOL32_F32SPLIT)
    add("f32split", "r12x10", 32, 0, "f32", 264, 3, L.K_XCOL32_F32SPLIT)
    for axis in (0, 1):
        add("super8", "s64", 8, axis, "f16", 264, 3, L.K_XPROP_SUPER8, bitwise=False)
    add("b64", "r10x12", 64, 1, "bf16", 264, 3, L.K_XCOL32_FLOW, kv={"fprop": L.KV_FLOW_HALF_UNITS, "bprop": L.KV_FLOW_HALF_UNITS})
    # gated calls
    for kind in ("binary", "general"):
        for dtype in ("bf16", "f16"):
            for axis in (0, 1):
                add("gated-segment", "r12x10", 32, axis, dtype, 264, 2, L.K_XPROP_SEGMENT, gate=kind)
                add("gated-segment", "r12x10", 16, axis, dtype, 264, 0, L.K_XPROP_SEGMENT, gate=kind)
    for axis in (0, 1):
        add("gated-staged", "r48", 32, axis, "bf16", 264, 3, L.K_XCOL32_STAGED, gate="general")
        add("gated-staged", "r48", 32, axis, "f16", 264, 3, L.K_XCOL32_STAGED, gate="binary")
    for bs, codes in ((32, (L.K_XCOL32_STAGED, L.K_XCOL32_FLOW)), (16, (L.K_XCOL16_STAGED, L.K_XCOL16_STAGED))):
        for axis in (0, 1):
            # one exact image over the plain tables; two bf16 images over the doubled tables; one fp16 image for any gate
            for kind, dtype in (("binary", "bf16"), ("general", "bf16"), ("general", "f16")):
                add("gated-images", "r48", bs, axis, dtype, 1160, 3, codes[axis], gate=kind, images=True, bitwise=False)
    add("gated-images", "r48", 32, 1, "bf16", 1160, 0, None, gate="binary", images=True, bitwise=False, code_from_ungated=True, tag="production")
    add("gated-images", "r48", 16, 0, "f16", 1160, 0, None, gate="binary", images=True, bitwise=False, code_from_ungated=True, tag="production")
    # (activations two bytes off: the ungated call over the image is the V_FMA kernel's, and the repair pass runs without its scan)
    add("gated-images", "r48", 32, 1, "bf16", 1160, 0, L.K_XPROP_VALU, gate="binary", images=True, bitwise=False, unaligned=True, tag="unaligned")
    for axis in (0, 1):
        add("gated-f32", "r12x10", 32, axis, "f32", 264, 0, L.K_XPROP_SEGMENT, gate="general")
        add("gated-b8", "r12x10", 8, axis, "bf16", 264, 0, L.K_XPROP_VALU, gate="binary" if axis else "general")
    for i, c in enumerate(out):
        c["seed"] = 7000 + i
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
# the cases the mutants are NAMED on (tests/test_containment_host.py checks every case a mutant applies to; these must be among them)
NAMED = {
    MUTANTS[0]: ("pair16-d20x16-b16-a1-bf16-N264", "super8-s64-b8-a1-f16-N264", "staged-r48-b32-a0-bf16-N264"),
    MUTANTS[1]: ("gated-images-r48-b32-a1-bf16-N1160-binary", "gated-images-r48-b16-a0-bf16-N1160-general", "gated-segment-r12x10-b16-a1-f16-N264-general"),
    MUTANTS[2]: ("small-small24-b32-a1-bf16-N70", "segment-r12x10-b16-a0-f32-N520", "mid-r48-b32-a1-bf16-N130"),
    MUTANTS[3]: ("small-small24-b16-a1-bf16-N40", "small-small24-b8-a0-f16-N72", "segment-r12x10-b16-a1-bf16-N40"),
}


# ---- the layout a pass walks, the poison, the gate ------------------------------------------------------------------------------------------
def pass_layout(c, which):
    """[input block][output block] of the pass: the layout for fprop, its transpose for bprop"""
    lay = LAYOUTS[c["lay"]] != 0
    return lay if which == "fprop" else lay.T


def partners(cb, bs, n_in):
    """the input blocks whose matrix-core step, pair step or super-block row `cb` shares"""
    if bs == 8:
        return [p for p in range(cb & ~3, min((cb & ~3) + 4, n_in)) if p != cb]
    return [cb ^ 1] if (cb ^ 1) < n_in else []


def _pick(lay, bs, gated):
    """(c1, c2, k_absent, k_g0, k_live) on an [in][out] layout: see the module docstring; k_g0 / k_live: the output blocks whose entry from c1 gets
    gate 0 / a gate != 0 (None / any connected block in ungated cases)"""
    n_in, n_out = lay.shape
    for c1 in range(n_in):
        ks = np.nonzero(lay[c1])[0]
        if len(ks) < (2 if gated else 1):
            continue
        absent = [k for k in range(n_out) if not lay[c1, k] and any(lay[p, k] for p in partners(c1, bs, n_in))]
        if not absent:
            continue
        near = set([c1] + partners(c1, bs, n_in))
        c2s = [c for c in range(n_in) if c not in near and 0 < lay[c].sum() < n_out]
        if not c2s:
            continue
        return dict(c1=c1, c2=c2s[len(c2s) // 2], k_absent=absent[0], k_g0=int(ks[0]) if gated else None, k_live=int(ks[-1]))
    raise AssertionError("no block with an absent partner in this layout")


@functools.lru_cache(maxsize=None)
def setup(cid):
    """The poisoned blocks of both passes and the gate of a case: {"fprop": pick, "bprop": pick, "gate": float32 [blocks] or None, "G": the
    gate as an [input block c][output block k] matrix of the LAYOUT (1 where there is no gate)}"""
    c = BY_ID[cid]
    t = luts(c["lay"], c["bs"])
    lay = LAYOUTS[c["lay"]] != 0
    s = {w: _pick(pass_layout(c, w), c["bs"], c["gate"] is not None) for w in ("fprop", "bprop")}
    wid = {ck: w for w, ck in enumerate(t["updat_list"])}
    gate = None
    if c["gate"] is not None:
        rs = np.random.RandomState(c["seed"])
        if c["gate"] == "binary":
            gate = (rs.rand(t["blocks"]) < 0.75).astype(np.float32)
        else:
            gate = np.asarray(GENERAL_GATES[c["dtype"]], dtype=np.float32)[rs.randint(0, 5, t["blocks"])]
        f, b = s["fprop"], s["bprop"]
        off = (wid[(f["c1"], f["k_g0"])], wid[(b["k_g0"], b["c1"])])          # (bprop picks live on the transposed layout: (in, out) = (k, c))
        on = (wid[(f["c1"], f["k_live"])], wid[(b["k_live"], b["c1"])])
        assert not set(off) & set(on), "the two passes ask opposite gates of one block"
        gate[list(off)] = 0.0
        gate[list(on)] = 1.0 if c["gate"] == "binary" else GENERAL_GATES[c["dtype"]][2]
    G = np.ones(lay.shape, dtype=np.float32)
    if gate is not None:
        for (ci, ki), w in wid.items():
            G[ci, ki] = gate[w]
    s.update(gate=gate, G=G)
    return s


def live(c, which):
    """[in][out] boolean: the entries of the pass that a call does not skip"""
    G = setup(c["id"])["G"]
    return pass_layout(c, which) & ((G if which == "fprop" else G.T) != 0)


def feat_blocks(c, which):
    """(input, output) feature blocks of the pass"""
    return pass_layout(c, which).shape


def act_shape(c, n_blocks):
    return (c["N"], n_blocks * c["bs"]) if c["axis"] else (n_blocks * c["bs"], c["N"])


def poison(c, which, a):
    """a copy of the pass' input with the two poisoned elements"""
    s, bs, N = setup(c["id"])[which], c["bs"], c["N"]
    a = np.array(a, dtype=np.float32, copy=True)
    f1, f2 = s["c1"] * bs + I1, s["c2"] * bs + bs + I2
    if c["axis"]:
        a[N - 1, f1], a[0, f2] = np.inf, np.nan
    else:
        a[f1, N - 1], a[f2, 0] = np.inf, np.nan
    return a


def _mask_of(c, which, reach1, reach2, leak=False):
    """the output-shaped mask of: minibatch index N - 1 non-finite in the output blocks reach1, index 0 in reach2 (`leak`: N - 2 as N - 1)"""
    bs, N = c["bs"], c["N"]
    rows = np.zeros((N, len(reach1)), dtype=bool)
    rows[N - 1] = reach1
    rows[0] |= reach2
    if leak:
        rows[N - 2] |= reach1
    m = np.repeat(rows, bs, axis=1)
    return m if c["axis"] else np.ascontiguousarray(m.T)


def expected_mask(c, which, mutant=None):
    """~isfinite of the pass' output under the poison: boolean arithmetic on the layout and the gate.  `mutant`: the mask a kernel with that
    defect would leave instead."""
    s = setup(c["id"])[which]
    lay, ok = pass_layout(c, which), live(c, which)
    n_in, n_out = lay.shape
    reach = {}
    for cb in (s["c1"], s["c2"]):
        r = ok[cb].copy()
        if mutant == MUTANTS[1]:                 # the gate multiplies the block product: 0 * Inf
            r = lay[cb].copy()
        if mutant == MUTANTS[0]:                 # the zero fragment standing in for the absent (cb, k) meets cb's live activations
            for k in range(n_out):
                if lay[cb, k]:
                    continue
                if c["bs"] == 8:                 # any block of the 32 x 32 super-block
                    r[k] |= bool(lay[cb & ~3:(cb & ~3) + 4, k & ~3:(k & ~3) + 4].any())
                else:
                    r[k] |= any(lay[p, k] for p in partners(cb, c["bs"], n_in))
        if mutant == MUTANTS[3] and cb == 0:     # an odd list's last K-concatenated step: zero weights, but the activations of the default entry (0, 0)
            r |= lay.sum(axis=0) % 2 == 1
        reach[cb] = r
    return _mask_of(c, which, reach[s["c1"]], reach[s["c2"]], leak=mutant == MUTANTS[2])


# ---- inputs and the float64 walk ------------------------------------------------------------------------------------------------------------
def walk(c, which, a, W, gate):
    """float64, entry by entry with the reference's skip (blocksparse/matmul.py:353-399: `if gate[w] != 0.0`); a skipped block's weights are
    never touched.  (oracle.bsmm_oracle scales the weights by the gate instead: the same for finite data, NaN for the NaN weights here.)"""
    t, bs, axis, N = luts(c["lay"], c["bs"]), c["bs"], c["axis"], c["N"]
    n_in, n_out = feat_blocks(c, which)
    a = np.asarray(a, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    A = a.reshape(N, n_in, bs) if axis else a.reshape(n_in, bs, N)
    out = np.zeros((N, n_out, bs) if axis else (n_out, bs, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for ob, entries in t[which + "_list"]:
            for ib, w in entries:
                g = 1.0 if gate is None else float(gate[w])
                if g == 0.0:
                    continue
                Wb = W[w] if which == "fprop" else W[w].T          # [in feature][out feature] of this pass
                if axis:
                    out[:, ob, :] += g * (A[:, ib, :] @ Wb)
                else:
                    out[ob] += g * (Wb.T @ A[ib])
    return out.reshape(act_shape(c, n_out))


@functools.lru_cache(maxsize=3)
def reference(cid):
    """Everything a test needs of a case, computed once: inputs (float32 arrays holding storage-type values; gate-0 weight blocks are NaN),
    the poisoned inputs, the float64 walk of the CLEAN inputs and the expected masks, per pass.  Read-only."""
    c = BY_ID[cid]
    t, bs = luts(c["lay"], c["bs"]), c["bs"]
    s = setup(cid)
    W, X, E = P.make_inputs((t["blocks"], bs, bs), act_shape(c, t["CB"]), act_shape(c, t["KB"]), c["dtype"], c["seed"])
    if s["gate"] is not None:
        W[s["gate"] == 0] = np.nan
    r = dict(W=W, gate=s["gate"])
    for which, a in (("fprop", X), ("bprop", E)):
        r[which] = dict(clean=a, poisoned=poison(c, which, a), want64=walk(c, which, a, W, s["gate"]), mask=expected_mask(c, which))
    for v in [W] + [x for w in ("fprop", "bprop") for x in r[w].values()]:
        v.flags.writeable = False
    return r
