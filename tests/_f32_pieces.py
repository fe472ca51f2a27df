"""Host helpers (NumPy only) for the tests of the fp32 routes that multiply bf16 PIECES: every fp32 x is split into x1 + x2 + x3
(csrc/bsmm_xcols.h::split3) and x * y is the sum of the six piece products PAIRS below (bsmm_updat_dispatch.h::f32_split_prologue, the MFMA sequence
of xcol32s_kernel / xcol32sf_kernel).  Here: the split restated bit for bit, inputs that HAVE a third piece, selector partners that isolate
single pairs, the product with any pair list (the true one and its mutants), an fp32 noise model, and the bar between the two.

Everything below speaks of GROUPS: a list of (A, B) float32 matrices with A @ B the group's output and the shared dimension the whole
reduction of that output -- one weight block of DW (A = X_c^T, B = DY_k, length N) or one feature block of Y / DX (A and B concatenated over
the blocks of the column).  `groups_of` makes them from a case's operands, `group_outputs` cuts a device result the same way.

CASES is the one table shared by tests/test_f32_pieces_host.py (which checks on the CPU that the inputs of every case can tell a wrong pair
from fp32 noise) and tests/test_f32_pieces_gpu.py (which runs them)."""
import itertools

import numpy as np

import _parity as P
from oracle import bsmm_oracle as orc

# (piece of the first operand, piece of the second), smallest products first: xi / ei of f32_split_prologue
PAIRS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
THIRD_ORDER = ((2, 0), (1, 1), (0, 2))
REDRAW_CAP = 0.01
MIN_PIECE = 2.0 ** -60          # every non-zero piece >= this, every value <= 1 / this: piece products stay normal fp32 numbers


# ---- the split ---------------------------------------------------------------------------------------------------------------------------
def _bf16_bits(x):
    """float32 -> bf16 bit pattern (uint16), round to nearest even (v_cvt_pk_bf16_f32); finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """The three bf16 pieces of a float32 array as float32 arrays (p1, p2, p3), csrc/bsmm_xcols.h::split3 bit for bit: round to nearest
    even, a first piece that rounded up to Inf steps back to 0x7f7f, the two subtractions in fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b1 = _bf16_bits(x)
    b1 = (b1 - ((b1 & 0x7FFF) == 0x7F80).astype(np.uint16)).astype(np.uint16)
    p1 = _bf16_value(b1)
    with np.errstate(over="ignore", invalid="ignore"):
        r1 = (x - p1).astype(np.float32)
        p2 = _bf16_value(_bf16_bits(r1))
        r2 = (r1 - p2).astype(np.float32)
        p3 = _bf16_value(_bf16_bits(r2))
    return p1, p2, p3


def _sums_back_in_every_order(x):
    """Elementwise: p_a + p_b + p_c == x in fp32 for all six orders of the pieces."""
    p = split3(x)
    ok = np.ones(x.shape, dtype=bool)
    for a, b, c in itertools.permutations(range(3)):
        ok &= ((p[a] + p[b]).astype(np.float32) + p[c]).astype(np.float32) == x
    return ok


def _in_range(x):
    ok = np.abs(x) <= np.float32(1.0 / MIN_PIECE)
    for p in split3(x):
        ok &= (p == 0) | (np.abs(p) >= np.float32(MIN_PIECE))
    return ok & (x != 0)


def _draw(shape, scale, rng, spread, accept, post=None):
    """normal * scale * 2^randint(-spread, spread) as float32 (never through a 16-bit type), elements that `accept` rejects redrawn.
    Returns (array, share of elements redrawn at least once)."""
    def raw(n):
        v = (rng.standard_normal(n) * scale * np.exp2(rng.integers(-spread, spread + 1, size=n))).astype(np.float32)
        return post(v) if post is not None else v
    n = int(np.prod(shape))
    x = raw(n)
    bad = ~accept(x)
    first = int(bad.sum())
    for _ in range(64):
        if not bad.any():
            break
        x[bad] = raw(int(bad.sum()))
        bad[bad] = ~accept(x[bad])
    assert not bad.any(), "redraw did not converge"
    return x.reshape(shape), first / max(n, 1)


def full_significand(shape, scale, rng, spread, with_share=False):
    """fp32 values with all 24 significand bits in play: 96 % of them have a non-zero third piece.  An element whose pieces do not sum
    back to it exactly in fp32 in all six orders is redrawn (the orders that start p1 + p3: 0.07 % of values), and so is one whose pieces
    or piece products could leave the normal fp32 range (the matrix cores may flush denormals)."""
    x, share = _draw(shape, scale, rng, spread, lambda v: _sums_back_in_every_order(v) & _in_range(v))
    return (x, share) if with_share else x


# ---- selector partners -------------------------------------------------------------------------------------------------------------------
SECOND_ORDER_UNIT = np.float32(1.0 + 2.0 ** -9)     # pieces 1 and 2^-9, no third


def _mask14(v):
    return (v.view(np.uint32) & np.uint32(0xFFFFFC00)).view(np.float32)


def _exact_against_second_order_unit(x):
    """x (14 significant bits: pieces 1 and 2 only) times 1 + 2^-9: the four live piece products summed in fp32 give the product in all 24
    orders.  (Scaling the partner by +-2^s scales every term: the verdict does not depend on s.)"""
    p = split3(x)
    u = split3(np.full(1, SECOND_ORDER_UNIT, dtype=np.float32))
    terms = [(p[i] * u[j][0]).astype(np.float32) for i in (0, 1) for j in (0, 1)]       # bf16 x bf16: exact in fp32
    want = (x.astype(np.float64) * float(SECOND_ORDER_UNIT))
    ok = (p[2] == 0) & (want.astype(np.float32).astype(np.float64) == want)
    for order in itertools.permutations(range(4)):
        s = terms[order[0]]
        for q in order[1:]:
            s = (s + terms[q]).astype(np.float32)
        ok &= s.astype(np.float64) == want
    return ok


def two_piece(shape, scale, rng, spread, with_share=False):
    """The full operand of the second-order selectors: full_significand masked to 14 significant bits (& 0xFFFFFC00)."""
    x, share = _draw(shape, scale, rng, spread, lambda v: _exact_against_second_order_unit(v) & _in_range(v), post=_mask14)
    return (x, share) if with_share else x


def selector_values(n, order, rng, smax=3):
    """n partner entries +-2^s (order 1) or +-2^s (1 + 2^-9) (order 2), s in -smax .. smax."""
    v = np.exp2(rng.integers(-smax, smax + 1, size=n)) * rng.choice([-1.0, 1.0], size=n)
    return (v * (float(SECOND_ORDER_UNIT) if order == 2 else 1.0)).astype(np.float32)


# ---- products from pieces ----------------------------------------------------------------------------------------------------------------
def mutants():
    """{name: pair list}: each of the six pairs dropped, each third-order pair replaced by a copy of another third-order pair."""
    out = {}
    for p in PAIRS:
        out["drop x%dy%d" % (p[0] + 1, p[1] + 1)] = tuple(q for q in PAIRS if q != p)
    for a in THIRD_ORDER:
        for b in THIRD_ORDER:
            if a != b:
                out["x%dy%d twice for x%dy%d" % (b[0] + 1, b[1] + 1, a[0] + 1, a[1] + 1)] = tuple(b if q == a else q for q in PAIRS)
    return out


def six_pair_product(xs, es, pairs=PAIRS, op=np.multiply):
    """sum over (i, j) in `pairs` of op(xs[i], es[j]) in float64; xs, es: the piece triples of split3; op: any bilinear map (elementwise
    product, np.matmul, ...)."""
    total = None
    for i, j in pairs:
        t = op(np.asarray(xs[i], dtype=np.float64), np.asarray(es[j], dtype=np.float64))
        total = t if total is None else total + t
    return total


def _rel(d, ref):
    return float(np.sqrt((d ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-300))


def _identity(g, prod):
    return prod


def fp32_products(A, B):
    """(A @ B by sequential fp32 accumulation with rounded products, A @ B by NumPy's fp32 matmul) for one group, as float32."""
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for l in range(A.shape[1]):
        acc = (acc + (A[:, l, None] * B[None, l, :]).astype(np.float32)).astype(np.float32)
    return acc, A @ B


def fp32_noise(A, B):
    """The larger L2-relative error of the two fp32 accumulations of one group against float64."""
    want = A.astype(np.float64) @ B.astype(np.float64)
    return max(_rel(emu.astype(np.float64) - want, want) for emu in fp32_products(A, B))


def tight_bar(groups, epilogue=_identity, live=None):
    """noise: the worst group of the fp32 noise model (the larger of the two accumulations); mutant: the best-hidden group of the best-hidden
    mutant; bar = sqrt(noise * mutant), valid only where mutant / noise >= 9 (3x margin on either side).  All errors are L2-relative per
    group against the float64 product.  `epilogue(g, product)` maps a group's raw product to what the call stores (alpha / beta / gate),
    applied alike to the oracle, the noise model (then rounded to fp32) and the mutants; `live[g]` False leaves a group out (its output does
    not depend on the product)."""
    muts = mutants()
    noise, mutant, hidden = 0.0, np.inf, None
    for g, (A, B) in enumerate(groups):
        if live is not None and not live[g]:
            continue
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        want = epilogue(g, A64 @ B64)
        for emu in fp32_products(A, B):
            out = np.asarray(epilogue(g, emu.astype(np.float64))).astype(np.float32).astype(np.float64)
            noise = max(noise, _rel(out - want, want))
        xs, es = split3(A), split3(B)
        terms = {p: np.matmul(xs[p[0]].astype(np.float64), es[p[1]].astype(np.float64)) for p in PAIRS}
        for name, pairs in muts.items():
            err = _rel(epilogue(g, sum(terms[p] for p in pairs)) - want, want)
            if err < mutant:
                mutant, hidden = err, (name, g)
    return {"noise": noise, "mutant": mutant, "hidden": hidden, "ratio": mutant / max(noise, 1e-300),
            "bar": float(np.sqrt(noise * mutant)), "valid": mutant >= 9.0 * noise}


# ---- layouts and cases -------------------------------------------------------------------------------------------------------------------
def _capped(CB, KB, density, seed, cap):
    """P.random_layout, the first seed from `seed` on whose rows and columns hold at most `cap` blocks (reduction length <= cap * bsize)."""
    for s in range(seed, seed + 200):
        lay = P.random_layout(CB, KB, density, seed=s)
        if lay.sum(axis=0).max() <= cap and lay.sum(axis=1).max() <= cap:
            return lay
    raise AssertionError("no layout")


def _holes(lay):
    lay = lay.copy()
    lay[2, :] = 0
    lay[:, 3] = 0
    return lay


def _one_per_column(n, seed):
    """A permutation layout without a fixed point pattern of its own: one block per block row and per block column, so with a selector in W
    every element of Y and of DX is a single product."""
    perm = np.random.default_rng(seed).permutation(n)
    lay = np.zeros((n, n), dtype=np.int32)
    lay[perm, np.arange(n)] = 1
    return lay


LAYOUTS = {
    "rand6x5": _capped(6, 5, 0.5, 21, 4),                 # at most 4 blocks per row / column
    "holes6x5": _holes(_capped(6, 5, 0.5, 21, 4)),        # ... with an empty block row and an empty block column
    "perm5": _one_per_column(5, 7),                       # odd: the last pair step has no odd half
    "perm18": _one_per_column(18, 8),                     # more output blocks than the 16 of a workgroup of the xcol kernels: two groups
    "rand12x10": P.random_layout(12, 10, 0.5, seed=22),   # ~6 blocks per column: the longer xprop reduction
    "rand8x12": P.random_layout(8, 12, 0.5, seed=23),     # bsize 8: the super-block plan needs multiples of 4 blocks a side
    "holes8x12": _holes(P.random_layout(8, 12, 0.5, seed=23)),
}

# xprop routes: (name, feature axis, how the call is made).  "abi": bsmm_fprop / bsmm_bprop with prepared_w = NULL (the library splits W
# into the workspace); "prepared": the product API, which hands the call the pieces bsmm_prepare_weights made.
XPROP_ROUTES = (("a1-fused-split", 1, "abi"), ("a0-pre-split", 0, "abi"), ("a1-prepared-weights", 1, "prepared"))
# updat routes: (name, trace code name, bsize, feature axis, layouts (random, holes), takes a gate)
UPDAT_ROUTES = (("stream32-a1", "K_UPDAT_STREAM", 32, 1, ("rand6x5", "holes6x5"), True),
                ("super8-a0", "K_UPDAT_SUPER8", 8, 0, ("rand8x12", "holes8x12"), False),      # (the route declines gated calls)
                ("super8-a1", "K_UPDAT_SUPER8", 8, 1, ("rand8x12", "holes8x12"), False),
                ("win16-a1", "K_UPDAT16_WIN", 16, 1, ("rand6x5", "holes6x5"), True),
                ("rows16-a0", "K_UPDAT16_ROWS", 16, 0, ("rand6x5", "holes6x5"), True))


# Where the bar between noise and mutants does not exist.  A group of DW is one weight block: 1024 elements at bsize 32, 256 at 16, 64 at 8,
# and the fewer the elements, the further the best-hidden block of a mutant and the noisiest block of the fp32 model move towards each other.
# mutant / noise on the CPU: bsize 32 9.7 .. 15, bsize 16 9.5 .. 10.6 at N = 40 (and N = 72 on feature axis 0) but 7.4 .. 8.3 at the
# (route, N) below, bsize 8 2.8 .. 5.9 at every N.  Those cases take the rule of the longer ones (the per-block fp32 kernels on the same
# inputs as the yardstick) and say so in their ids; the host tier asserts that every case NOT listed here has its ratio >= 9.
NO_TIGHT_BAR = {("win16-a1", 72), ("win16-a1", 128), ("rows16-a0", 128)} | {(r, n) for r in ("super8-a0", "super8-a1") for n in (40, 72, 128)}


def _cases():
    out = []
    seed = 1000
    for name, axis, how in XPROP_ROUTES:
        for op in ("fprop", "bprop"):
            base = dict(route=name, op=op, bs=32, axis=axis, how=how, kernel="K_XCOL32_F32SPLIT")
            for order in (1, 2):
                for role in ("partner-in-W", "partner-in-acts"):
                    for N in (72, 136) if axis == 1 else (72,):
                        seed += 1
                        out.append(dict(base, kind="selector", order=order, role=role, N=N, seed=seed,
                                        layout="perm5" if role == "partner-in-W" else "rand6x5"))
                out.append(dict(base, kind="selector", order=order, role="partner-in-W", N=72, seed=5000 + len(out), layout="perm18"))
            for lay, N in (("rand6x5", 72), ("holes6x5", 136)):
                seed += 1
                out.append(dict(base, kind="tight", layout=lay, N=N, seed=seed))
            seed += 1
            out.append(dict(base, kind="yardstick", layout="rand12x10", N=264, seed=seed))
    for name, kernel, bs, axis, lays, gated in UPDAT_ROUTES:
        base = dict(route=name, op="updat", bs=bs, axis=axis, how="api", kernel=kernel)
        for order in (1, 2):
            for role in ("partner-in-DY", "partner-in-X"):
                for N in (72, 136) if axis == 1 else (72,):
                    seed += 1
                    out.append(dict(base, kind="selector", order=order, role=role, N=N, seed=seed, layout=lays[0]))
        for lay, N in ((lays[0], 40), (lays[1], 72), (lays[0], 128)):
            seed += 1
            out.append(dict(base, kind="yardstick(ratio<9)" if (name, N) in NO_TIGHT_BAR else "tight", layout=lay, N=N, seed=seed))
        seed += 1
        out.append(dict(base, kind="yardstick", layout=lays[0], N=392 if name == "stream32-a1" else 264, seed=seed))
        seed += 1
        out.append(dict(base, kind="alpha-beta-gate" if gated else "alpha-beta(no gate taken)-yardstick(ratio<9)", layout=lays[0], N=72, seed=seed,
                        gated=gated))
    for c in out:
        c["id"] = "-".join(str(c[k]) for k in ("route", "op", "kind", "order", "role", "layout", "N") if k in c).replace(" ", "_")
    return out


CASES = _cases()
ALPHA, BETA = 0.5, 0.25
SPREAD = 6


def shapes(case):
    lay = LAYOUTS[case["layout"]]
    CB, KB = lay.shape
    bs, N, axis = case["bs"], case["N"], case["axis"]
    C, K = CB * bs, KB * bs
    return dict(layout=lay, blocks=int(lay.sum()), C=C, K=K, w=(int(lay.sum()), bs, bs), i=(N, C) if axis else (C, N), o=(N, K) if axis else (K, N))


def _acts(a, axis):
    """An activation array as (minibatch, features) whatever the feature axis (a view)."""
    return a if axis else a.T


def _one_hot_rows(N, F, vals, rng):
    """(N, F): row n holds vals[n] at one random feature, nothing else."""
    a = np.zeros((N, F), dtype=np.float32)
    a[np.arange(N), rng.integers(0, F, size=N)] = vals
    return a


def _injection(N, F, vals, rng):
    """(N, F): min(N, F) distinct features each hold one value, each in a row of its own; the other features (F > N) are zero."""
    a = np.zeros((N, F), dtype=np.float32)
    m = min(N, F)
    feats, rows = rng.permutation(F)[:m], rng.permutation(N)[:m]
    a[rows, feats] = vals[:m]
    return a


def make_inputs(case):
    """{W, X, E (float32, the shapes of the operator), redraw (worst share over the drawn operands), dw0, gate (alpha / beta cases)}.  Only
    the operands the case's op reads are non-trivial."""
    rng = np.random.default_rng(case["seed"])
    s = shapes(case)
    axis, N, bs, op = case["axis"], case["N"], case["bs"], case["op"]
    shares = []

    def full(shape, scale):
        gen = two_piece if case.get("order") == 2 else full_significand
        a, share = gen(shape, scale, rng, SPREAD, with_share=True)
        shares.append(share)
        return a

    def lay_out(a):      # (N, F) -> the operator's activation layout
        return np.ascontiguousarray(a if axis else a.T)

    W = np.zeros(s["w"], dtype=np.float32)
    X = np.zeros(s["i"], dtype=np.float32)
    E = np.zeros(s["o"], dtype=np.float32)
    out = {}
    if case["kind"] == "selector":
        order = case["order"]
        if op == "updat":
            part_feats, full_shape, full_scale = (s["K"], (N, s["C"]), 0.1) if case["role"] == "partner-in-DY" else (s["C"], (N, s["K"]), 0.1)
            partner = lay_out(_injection(N, part_feats, selector_values(max(N, part_feats), order, rng), rng))
            other = lay_out(full(full_shape, full_scale))
            X, E = (other, partner) if case["role"] == "partner-in-DY" else (partner, other)
        else:
            feats = s["C"] if op == "fprop" else s["K"]
            if case["role"] == "partner-in-W":
                for w in range(s["blocks"]):         # a scaled permutation inside each block
                    W[w][rng.permutation(bs), np.arange(bs)] = selector_values(bs, order, rng)
                acts = lay_out(full((N, feats), 0.1))
            else:
                W = full(s["w"], 0.01)
                acts = lay_out(_one_hot_rows(N, feats, selector_values(N, order, rng), rng))
            if op == "fprop":
                X = acts
            else:
                E = acts
    else:
        if op in ("fprop", "bprop"):
            W = full(s["w"], 0.01)
        if op in ("fprop", "updat"):
            X = full(s["i"], 0.1)
        if op in ("bprop", "updat"):
            E = full(s["o"], 0.1)
    out.update(W=W, X=X, E=E, redraw=max(shares))
    if case["kind"].startswith("alpha-beta"):
        prod = raw_product(case, out)
        rms = np.sqrt((prod ** 2).mean(axis=(1, 2)))
        gate = rng.uniform(0.0, 2.0, size=s["blocks"]).astype(np.float32)
        gate[1], gate[s["blocks"] // 2] = 0.0, 1.0
        if not case["gated"]:
            gate = None
        # beta * dw0 at the rms of alpha * gate * product, block by block (the product's where the gate is 0): the product carries
        # 1 / sqrt(2) of every live block's norm
        g = np.ones(s["blocks"]) if gate is None else np.where(gate == 0, 1.0, gate.astype(np.float64))
        dw0 = (rng.standard_normal(s["w"]) * (ALPHA * g * rms / BETA)[:, None, None]).astype(np.float32)
        out.update(gate=gate, dw0=dw0)
    return out


def tables(case):
    return orc.build_layout_luts(LAYOUTS[case["layout"]], case["bs"])


def raw_product(case, inp):
    """The float64 oracle of the bare product (no alpha / beta / gate), in the operator's output shape."""
    t, axis = tables(case), case["axis"]
    if case["op"] == "fprop":
        return orc.fprop(t, inp["X"], inp["W"], axis)
    if case["op"] == "bprop":
        return orc.bprop(t, inp["E"], inp["W"], axis)
    return orc.updat(t, inp["X"], inp["E"], axis)


def groups_of(case, inp):
    """[(A, B)] with A @ B the output group in the orientation of `group_outputs`; groups with no block have zero-width A.  (For Y / DX the
    first operand of a group is the activations: a mutant name that `tight_bar` reports reads x = activations, y = weights there.)"""
    t, axis, bs, op = tables(case), case["axis"], case["bs"], case["op"]
    if op == "updat":
        X, E = _acts(inp["X"], axis), _acts(inp["E"], axis)
        return [(np.ascontiguousarray(X[:, c * bs:(c + 1) * bs].T), np.ascontiguousarray(E[:, k * bs:(k + 1) * bs])) for c, k in t["updat_list"]]
    W = inp["W"]
    acts = _acts(inp["X"] if op == "fprop" else inp["E"], axis)
    lists = dict(t["fprop_list" if op == "fprop" else "bprop_list"])
    out = []
    for f in range(t["KB"] if op == "fprop" else t["CB"]):
        ent = lists.get(f, [])
        A = np.concatenate([acts[:, i * bs:(i + 1) * bs] for i, _ in ent] or [np.zeros((acts.shape[0], 0), np.float32)], axis=1)
        B = np.concatenate([(W[w] if op == "fprop" else W[w].T) for _, w in ent] or [np.zeros((0, bs), np.float32)], axis=0)
        out.append((np.ascontiguousarray(A), np.ascontiguousarray(B)))      # (N, L) @ (L, bs)
    return out


def group_outputs(case, out):
    """A result in the operator's output shape as one matrix per group, oriented like A @ B of `groups_of`."""
    out = np.asarray(out)
    bs = case["bs"]
    if case["op"] == "updat":
        return list(out)
    a = _acts(out, case["axis"])
    return [a[:, f * bs:(f + 1) * bs] for f in range(a.shape[1] // bs)]


def epilogue_of(case, inp):
    """(epilogue for tight_bar, live mask) of an alpha / beta / gate case."""
    gate, dw0 = inp.get("gate"), inp["dw0"].astype(np.float64)
    gv = np.ones(len(dw0)) if gate is None else gate.astype(np.float64)
    return (lambda g, prod: ALPHA * gv[g] * prod + BETA * dw0[g]), list(gv != 0)


def group_errors(case, got, want):
    """Per-group L2-relative errors (groups whose oracle is all zero: the absolute norm of what was stored there)."""
    errs = []
    for g, w in zip(group_outputs(case, np.asarray(got, dtype=np.float64)), group_outputs(case, want)):
        den = np.sqrt((w ** 2).sum())
        errs.append(float(np.sqrt(((g - w) ** 2).sum()) / (den if den > 0 else 1.0)))
    return np.array(errs)


# ---- selectors: which pairs are live, which mutants must show ---------------------------------------------------------------------------
def live_pairs(case):
    """The pairs whose product is non-zero in a selector case.  The first index of a pair is the piece of X (updat) / of the weights
    (xprop: the kernels' wq[i]), the second the piece of DY / of the activations."""
    partner_first = case["role"] in ("partner-in-X", "partner-in-W")
    n_full = 3 if case["order"] == 1 else 2
    n_part = case["order"]
    return tuple((i, j) for i, j in PAIRS if (i < (n_part if partner_first else n_full)) and (j < (n_full if partner_first else n_part)))


def selector_elements(case, inp):
    """(partner value, full-operand value) per output element of a selector case, in the operator's output shape, and the mask of live
    elements: an output element is a single product partner * full, or nothing (partner 0)."""
    keep = dict(inp)
    if case["op"] == "updat":
        pk, fk = ("E", "X") if case["role"] == "partner-in-DY" else ("X", "E")
    else:
        ak = "X" if case["op"] == "fprop" else "E"
        pk, fk = ("W", ak) if case["role"] == "partner-in-W" else (ak, "W")
    ones = dict(keep)
    ones[pk] = (keep[pk] != 0).astype(np.float32)
    full_vals = raw_product(case, ones)                       # the gathered element of the full operand (times 1)
    ones = dict(keep)
    ones[fk] = np.ones_like(keep[fk])
    part_vals = raw_product(case, ones)                       # the partner entry that meets it
    return part_vals.astype(np.float32), full_vals.astype(np.float32), part_vals != 0


def selector_mutant_report(case, inp):
    """{mutant name: share of live output elements it changes} for the mutants that touch a live pair, and `exact`: whether the true
    pair list reproduces the float64 product exactly in fp32."""
    part, full, live = selector_elements(case, inp)
    partner_first = case["role"] in ("partner-in-X", "partner-in-W")
    first, second = (part, full) if partner_first else (full, part)
    xs, es = split3(first[live]), split3(second[live])
    want = first[live].astype(np.float64) * second[live].astype(np.float64)
    lp = live_pairs(case)
    rep = {"exact": bool((six_pair_product(xs, es) == want).all() and (want.astype(np.float32).astype(np.float64) == want).all()), "mutants": {}}
    for name, pairs in mutants().items():
        if all(pairs.count(p) == 1 for p in lp):
            continue
        rep["mutants"][name] = float((six_pair_product(xs, es, pairs).astype(np.float32) != want.astype(np.float32)).mean())
    return rep
