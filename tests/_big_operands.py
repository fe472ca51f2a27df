"""Matmul operands at and past the 32-bit offset limits of the kernels: the case table, the data builders and the expected values shared by
tests/test_big_operands_host.py (CPU tier) and tests/test_big_operands_gpu.py.

The contract under test: a bsmm_fprop / bsmm_bprop / bsmm_updat call either computes the right result or returns an error code before it
launches anything.  Ten predicates of the dispatch exist only because a kernel keeps 32-bit byte offsets inside an operand
(bsmm_xprop_dispatch.h: the mid kernel, the bsize-16 and bsize-32 staged / flow plans; bsmm_updat_dispatch.h: the fp32 streaming split, the
bsize-8 fp32 split, the fp32 row-owner kernel, `s8_big`, the streaming kernel, `rows_ok`; matmul.py: `native64`); every other route claims
by its silence to address any operand.  CASES holds a pair for each predicate -- the largest size that still takes the limited kernel and
the first size that must not -- and operands past 2^31 elements / 2^32 bytes for the routes without one.

Data.  Nobody computes a float64 oracle over 2^31 elements in seconds, so the inputs are made such that it is not needed:
  values   W in {-2..2}/16, X and DY in {-2..2}/4: exact in bf16 / fp16 / fp32 and in the first bf16 piece of the fp32 split, every product
           exact in fp32, every partial sum an integer multiple of the unit below 2^24 units (`exactness`): the expected value is the
           float64 oracle (oracle/bsmm_oracle.py) rounded once to the storage type and the device result must be BIT-EQUAL to it;
  period   along the minibatch an operand repeats a random base of P rows (P odd: 509, 127 for the wide family), filled on the device by a
           broadcast copy plus a ragged tail; the oracle runs on one period, expected Y / DX repeat with it, expected DW is
           R * DW_period + DW_tail + marker terms;
  markers  single minibatch rows of +-3/4 (no base row holds a 3): the first and the last row and the row on each side of every 2^31-byte
           (hence every 2^32-byte) boundary of the operand; the expected values hold one row of Y / DX and one rank-1 term of DW for each.
`count_mismatches` compares a whole result, chunked, on whatever device it lies, with the period broadcast and the marker rows; only
coordinates and a few values go to the host.

All arrays here are MINIBATCH-MAJOR, (rows, features); `fill` writes the operator's layout ((features, N) on feature axis 0).

Left out: the feature-axis-1 forms of the staged-plan predicates (bsmm_xprop_dispatch.h, "32-bit lane offsets") need C >= 2^24 features,
and no dense layout matrix reaches that.  Attention (bst_*) and the fused element-wise families refuse >= 2^31 elements and are covered
by test_ewops_host.py / test_lstm_host.py."""
import functools

import numpy as np

import _parity as PAR
from oracle import bsmm_oracle as orc

GIB = 1 << 30
BOUNDARY = 1 << 31            # markers sit on each side of every multiple of this many bytes
LIMIT_UNITS = 1 << 24         # integers up to here are exact in fp32
ESZ = {"bf16": 2, "f32": 4}
MAX_LIVE = 24 * GIB
W_UNIT, A_UNIT = 1.0 / 16, 1.0 / 4
MARKER = 3                    # |marker values| in units of A_UNIT: no base row holds one


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
def _wide_layout(n=4096):
    """n x n blocks, one to three per block row and per block column: three permutations, the second on every second row, the third on
    every third."""
    rng = np.random.default_rng(41)
    lay = np.zeros((n, n), dtype=np.int32)
    rows = np.arange(n)
    lay[rows, rng.permutation(n)] = 1
    p2, p3 = rng.permutation(n), rng.permutation(n)
    lay[rows[::2], p2[::2]] = 1
    lay[rows[::3], p3[::3]] = 1
    return lay


def _locks_layout():
    """32 x 32 at 15 % with one full block column and one full block row: the reference-policy tables cut those into segments that share an
    output block (locks > 0 in fprop and in bprop)."""
    lay = PAR.random_layout(32, 32, 0.15, seed=31).copy()
    lay[:, 5] = 1
    lay[9, :] = 1
    return lay


_LAYOUTS = {
    "r32": lambda: PAR.random_layout(32, 32, 0.15, seed=31),       # bsize 32, C = K = 1024
    "r64": lambda: PAR.random_layout(64, 64, 0.15, seed=32),       # bsize 16
    "r128": lambda: PAR.random_layout(128, 128, 0.15, seed=33),    # bsize 8
    "r16": lambda: PAR.random_layout(16, 16, 0.15, seed=34),       # bsize 64
    "r64x4": lambda: PAR.random_layout(64, 4, 0.5, seed=35),       # bsize 16, C = 1024, K = 64
    "locks32": _locks_layout,
    "d2": lambda: np.ones((2, 2), dtype=np.int32),                 # bsize 32, C = K = 64
    "d4": lambda: np.ones((4, 4), dtype=np.int32),                 # bsize 16, C = K = 64
    "wide": _wide_layout,                                          # bsize 32, C = K = 131072
}


@functools.lru_cache(maxsize=None)
def layout(name):
    return _LAYOUTS[name]()


@functools.lru_cache(maxsize=None)
def tables(name, bs):
    return orc.build_layout_luts(layout(name), bs)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def _case(family, tag, lay, bs, axis, dtype, N, variant=3, expect=None, segmented=False, refusal_ok=False, P=509, native64=None):
    CB, KB = layout(lay).shape
    c = dict(family=family, layout=lay, bs=bs, axis=axis, dtype=dtype, N=N, C=CB * bs, K=KB * bs, variant=variant, segmented=segmented,
             refusal_ok=refusal_ok, P=P, expect=dict(expect or {}), native64=native64, seed=7)
    c["id"] = "%s-%s-bs%d-a%d-%s-N%d-v%d" % (family, tag, bs, axis, dtype, N, variant)
    c["bytes"] = device_bytes(c)
    return c


def device_bytes(c):
    """Device bytes live at the worst moment of a case.  The three passes run one after the other and each holds only its own tensors:
    fprop X + Y, bprop DY + DX, updat X + DY (the test drops the operator's cached workspaces between the passes); on top the large
    workspace of the pass, then 3/4 GiB for W / DW, the tables and the kernels' own scratch (5/4 GiB on the 4096 x 4096 layout, where the
    partial-sum regions of the streaming weight-gradient kernel alone take 1/2 GiB) and 3/4 GiB for the comparison's temporaries (chunk-sized
    masks and their reduction).  The GPU tier asserts that the peak it measures stays below this figure."""
    e = ESZ[c["dtype"]]
    N, C, K = c["N"], c["C"], c["K"]
    f32 = c["dtype"] == "f32"
    E = N * max(C, K)
    ws_x = 0
    if f32 and c["bs"] == 32 and c["axis"] == 0:
        ws_x = 6 * N * max(C, K)                      # the pre-split pieces of the activations (feature axis 1 splits inside the kernel)
    if c["segmented"] and not f32:
        ws_x = 4 * N * max(C, K)                      # fp32 image of the locked outputs
    ws_u = 0
    if f32 and c["variant"] in (0, 3):                # the six-pair routes: three bf16 pieces of X and of DY
        takes = {(32, 1): E < (1 << 30), (8, 0): E < (1 << 30), (8, 1): E < (1 << 30), (16, 1): True, (16, 0): E < (1 << 31)}
        if takes.get((c["bs"], c["axis"]), False):
            ws_u = 6 * N * (C + K)
    xprop = e * N * (C + K) + ws_x
    updat = e * N * (C + K) + ws_u
    scratch = 3 * GIB // 4 if int(layout(c["layout"]).sum()) <= 4096 else 5 * GIB // 4
    return max(xprop, updat) + scratch + 3 * GIB // 4


def _cases():
    out = []
    M20, M21, M24 = 1 << 20, 1 << 21, 1 << 24
    # -- long, C = K = 1024, plans forced: E = N * 1024 on each side of 2^30
    for N, below in ((M20 - 8, True), (M20, False)):
        for axis in (0, 1):
            out.append(_case("long", "e30", "r32", 32, axis, "bf16", N, expect={"updat": ("is" if below else "not", "K_UPDAT_STREAM")}))
            out.append(_case("long", "e30", "r64", 16, axis, "bf16", N))
            out.append(_case("long", "e30", "r128", 8, axis, "bf16", N, expect={"updat": ("is" if below else "not", "K_UPDAT_SUPER8")}))
            out.append(_case("long", "e30", "r128", 8, axis, "f32", N, expect={"updat": ("is" if below else "not", "K_UPDAT_SUPER8")}))
        out.append(_case("long", "e30", "r16", 64, 1, "bf16", N, native64=below))
        out.append(_case("long", "e30", "r32", 32, 1, "f32", N, expect={"updat": ("is" if below else "not", "K_UPDAT_STREAM")}))
    # (feature axis 0: the split pre-pass over N * C elements leaves 6 GiB of pieces in the workspace; no predicate)
    split = {"fprop": ("is", "K_XCOL32_F32SPLIT"), "bprop": ("is", "K_XCOL32_F32SPLIT")}
    out.append(_case("long", "e30", "r32", 32, 0, "f32", M20, expect=split))
    # (the windowed six-pair route has no size limit: 4 GiB of fp32 per operand)
    out.append(_case("long", "e30", "r64", 16, 1, "f32", M20, expect={"updat": ("is", "K_UPDAT16_WIN")}))
    # -- bsize 16 on feature axis 0: the row-owner kernel on each side of E = 2^31 (fp32: K = 64, so that the three bf16 pieces of both
    #    operands -- 6 bytes per element -- fit under MAX_LIVE next to the operands; the predicate looks at N * max(C, K) alone)
    for N, below in ((M21 - 8, True), (M21, False)):
        out.append(_case("long", "e31", "r64", 16, 0, "bf16", N, expect={"updat": ("is" if below else "not", "K_UPDAT16_ROWS")}))
        out.append(_case("long", "e31", "r64x4", 16, 0, "f32", N, expect={"updat": ("is" if below else "not", "K_UPDAT16_ROWS")}))
    # -- the mid kernel on each side of N * C * 2 = 2^32 (FLAG_FORCE_MID: variant 4)
    mid = {"fprop": ("is", "K_XPROP_MID"), "bprop": ("is", "K_XPROP_MID")}
    out.append(_case("long", "mid", "r32", 32, 1, "bf16", M21 - 8, variant=4, expect=mid))
    out.append(_case("long", "mid", "r32", 32, 1, "bf16", M21 + 8, variant=4, expect={k: ("not", v[1]) for k, v in mid.items()}))
    # -- E > 2^31, 4 GiB of bf16 per operand: the plan kernels, the generic kernels, the V_FMA kernels, the locked finalize over N * K
    for axis in (0, 1):
        out.append(_case("long", "e31+", "r32", 32, axis, "bf16", M21 + 8))
        out.append(_case("long", "e31+", "r32", 32, axis, "bf16", M21 + 8, variant=2))
    out.append(_case("long", "e31+", "r32", 32, 1, "bf16", M21 + 8, variant=1,
                     expect={"fprop": ("is", "K_XPROP_VALU"), "bprop": ("is", "K_XPROP_VALU"), "updat": ("is", "K_UPDAT_VALU")}))
    # (the reference-policy table with the plans left out: the per-segment kernels are the ones that take locked outputs)
    out.append(_case("long", "e31+locks", "locks32", 32, 1, "bf16", M21 + 8, variant=2, segmented=True,
                     expect={"fprop": ("is", "K_XPROP_SEGMENT"), "bprop": ("is", "K_XPROP_SEGMENT")}))
    # -- row stride, feature axis 0, C = K = 64: a feature row of N elements on each side of N * 256 = 2^32 bytes of lane offset
    for N, below in ((M24 - 8, True), (M24, False)):
        for lay, bs, name in (("d2", 32, "K_XCOL32_STAGED"), ("d4", 16, "K_XCOL16_STAGED")):
            how = "is" if below else "not"
            out.append(_case("rowstride", "n24", lay, bs, 0, "bf16", N, expect={"fprop": (how, name), "bprop": (how, name)}, refusal_ok=True))
    # (the V_FMA kernel puts (N + 255) / 256 = 65536 row tiles on grid.y there -- HIP may refuse that launch)
    valu = {"fprop": ("is", "K_XPROP_VALU"), "bprop": ("is", "K_XPROP_VALU"), "updat": ("is", "K_UPDAT_VALU")}
    out.append(_case("rowstride", "n24", "d2", 32, 0, "bf16", M24, variant=1, expect=valu, refusal_ok=True))
    # -- wide, feature axis 1, C = K = 131072: the row stride, not the row count, is large
    for N in (8192 - 8, 16384 + 8):
        for variant in (0, 3):
            out.append(_case("wide", "c17", "wide", 32, 1, "bf16", N, variant=variant, P=127))
    out.sort(key=lambda c: (c["bytes"], c["id"]))
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def marker_rows(N, F, esz, axis, boundary=BOUNDARY):
    """Minibatch indices of the marker rows of an operand of N rows and F features: first, last, and the row that holds the byte on each
    side of every multiple of `boundary` inside the operand ((N, F) on feature axis 1, (F, N) on feature axis 0)."""
    rows = {0, N - 1}
    total = N * F * esz
    for b in range(boundary, total, boundary):
        for byte in (b - 1, b):
            el = byte // esz
            rows.add(el // F if axis == 1 else el % N)
    return sorted(rows)


def case_markers(c, boundary=BOUNDARY):
    """One marker set for X and DY (their union): a marker row of DW's sum then has both factors planted."""
    e = ESZ[c["dtype"]]
    return sorted(set(marker_rows(c["N"], c["C"], e, c["axis"], boundary)) | set(marker_rows(c["N"], c["K"], e, c["axis"], boundary)))


def base_data(c, nmark):
    """{W (blocks, bs, bs), X (P, C), E (P, K), Xm (nmark, C), Em (nmark, K)} as float64, minibatch-major."""
    rng = np.random.default_rng(c["seed"])
    t = tables(c["layout"], c["bs"])
    P = c["P"]
    W = rng.integers(-2, 3, size=(t["blocks"], c["bs"], c["bs"])) * W_UNIT
    X = rng.integers(-2, 3, size=(P, c["C"])) * A_UNIT
    E = rng.integers(-2, 3, size=(P, c["K"])) * A_UNIT
    mrng = np.random.default_rng(c["seed"] + 1000)
    Xm = mrng.choice([-MARKER, MARKER], size=(nmark, c["C"])) * A_UNIT
    Em = mrng.choice([-MARKER, MARKER], size=(nmark, c["K"])) * A_UNIT
    return dict(W=W, X=X, E=E, Xm=Xm, Em=Em)


def _acts(a, axis):
    """minibatch-major <-> the oracle's layout of the feature axis."""
    return a if axis else np.ascontiguousarray(a.T)


def _fprop(c, X, W):
    return _acts(orc.fprop(tables(c["layout"], c["bs"]), _acts(X, c["axis"]), W, c["axis"]), c["axis"])


def _bprop(c, E, W):
    return _acts(orc.bprop(tables(c["layout"], c["bs"]), _acts(E, c["axis"]), W, c["axis"]), c["axis"])


def _updat(c, X, E):
    return orc.updat(tables(c["layout"], c["bs"]), _acts(X, c["axis"]), _acts(E, c["axis"]), c["axis"])


def expected(c, boundary=BOUNDARY):
    """Everything a case's checks need, float64 and minibatch-major: the data (`base_data`), markers, Y / DX of one period (Yp, DXp) and of
    the marker rows (Ym, DXm), DW of the whole operand."""
    marks = case_markers(c, boundary)
    d = base_data(c, len(marks))
    P, N = c["P"], c["N"]
    R, tail = divmod(N, P)
    out = dict(d, markers=marks, R=R, tail=tail)
    out["Yp"], out["Ym"] = _fprop(c, d["X"], d["W"]), _fprop(c, d["Xm"], d["W"])
    out["DXp"], out["DXm"] = _bprop(c, d["E"], d["W"]), _bprop(c, d["Em"], d["W"])
    dw = R * _updat(c, d["X"], d["E"])
    if tail:
        dw = dw + _updat(c, d["X"][:tail], d["E"][:tail])
    at = [m % P for m in marks]
    out["DW"] = dw + _updat(c, d["Xm"], d["Em"]) - _updat(c, d["X"][at], d["E"][at])
    return out


def exactness(c, ex):
    """The largest magnitude, in units of the product of the operand units, that a partial sum of any output element can reach.  DW: a sum
    over an interval of the minibatch is at most R |period sum| + (max prefix - min prefix of a period) + the marker terms, for every element
    of every block; Y / DX: the sum of the magnitudes of a column's terms."""
    t, bs = tables(c["layout"], c["bs"]), c["bs"]
    Xt = np.ascontiguousarray(np.rint(ex["X"] / A_UNIT).astype(np.int32).T).reshape(-1, bs, c["P"])      # (feature blocks, bs, P)
    Et = np.ascontiguousarray(np.rint(ex["E"] / A_UNIT).astype(np.int32).T).reshape(-1, bs, c["P"])
    ul = np.asarray(t["updat_list"], dtype=np.int64).reshape(-1, 2)
    batch = max(1, (1 << 24) // (bs * bs * c["P"]))
    # (where even the sum of the magnitudes of all N terms, each at most 2 * 2, stays below the limit there is nothing to scan)
    coarse = float(c["N"] * 4)
    scan = coarse + len(ex["markers"]) * (MARKER * MARKER + 4) >= LIMIT_UNITS
    worst = 0.0 if scan else coarse
    for b0 in range(0, len(ul) if scan else 0, batch):
        cb, kb = ul[b0:b0 + batch, 0], ul[b0:b0 + batch, 1]
        pre = np.cumsum(Xt[cb][:, :, None, :] * Et[kb][:, None, :, :], axis=-1)                           # (blocks, bs, bs, P) prefix sums
        span = np.maximum(pre.max(axis=-1), 0) - np.minimum(pre.min(axis=-1), 0)
        worst = max(worst, float((ex["R"] * np.abs(pre[..., -1]).astype(np.int64) + span).max()))
    dw = worst + len(ex["markers"]) * (MARKER * MARKER + 4)            # a marker term replaces a base term of at most 2 * 2
    lay = layout(c["layout"])
    longest = int(max(lay.sum(axis=0).max(), lay.sum(axis=1).max())) * bs
    return {"DW": dw, "Y": longest * MARKER * 2, "DX": longest * MARKER * 2}


def wrap_partners_distinct(c, ex, boundary=BOUNDARY):
    """No two minibatch rows whose byte offsets differ by a multiple of `boundary` hold equal contents (feature axis 0: no two runs of a
    feature row boundary / 2 elements apart, whichever feature rows they fall into).  Checked on the base: its rows are pairwise distinct, no
    distance is a multiple of P, and a marker row holds values no base row does."""
    e, N, P, axis = ESZ[c["dtype"]], c["N"], c["P"], c["axis"]
    for name, F in (("X", c["C"]), ("E", c["K"])):
        base = ex[name]
        probe = np.random.default_rng(5).random(max(F, P))      # distinct projections: distinct rows
        if len(np.unique(base @ probe[:F])) != P:
            return False
        if axis == 1:
            stride = F * e
            j = 1
            while j * boundary < N * stride:
                if (j * boundary) % stride == 0 and ((j * boundary) // stride) % P == 0:
                    return False
                j += 1
        else:
            if len(np.unique(probe[:P] @ base)) != F:               # feature rows differ as sequences of the period
                return False
            j = 1
            while j * boundary < N * F * e:
                df, dn = divmod(j * boundary // e, N)
                # the partner of element (f, n) is (f + df, n + dn) or, past the row's end, (f + df + 1, n + dn - N): compare one period's worth
                n = np.arange(2 * P)
                for f in (0, F // 2):
                    for f2, shift in ((f + df, dn), (f + df + 1, dn - N)):
                        if 0 <= f2 < F and np.array_equal(base[n % P, f], base[(n + shift) % P, f2]):
                            return False
                j += 1
    return True


# ---- torch side: fill and compare (any device) -------------------------------------------------------------------------------------------
def torch_dtype(torch, dtype):
    return getattr(torch, PAR.TORCH_DT[dtype])


def to_storage(torch, a, dtype, device="cpu"):
    """float64 -> storage type, rounded once (every value here is exact in fp32, so the step through fp32 rounds nothing)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    assert np.array_equal(t.numpy().astype(np.float64), a), "a value is not exact in fp32"
    return t.to(device).to(torch_dtype(torch, dtype))


FILL_CHUNK = 1 << 28


def fill(torch, base, N, axis, markers, rows):
    """The operand of N minibatch rows in the operator's layout -- (N, F) on feature axis 1, (F, N) on feature axis 0 -- from one period
    `base` (P, F) by broadcast copies, a ragged tail, then the marker rows; base / rows: storage type, on the device the result is wanted."""
    P, F = base.shape
    R, tail = divmod(N, P)
    step = max(1, FILL_CHUNK // (P * F))
    idx = torch.as_tensor(list(markers), dtype=torch.long, device=base.device)
    if axis == 1:
        out = torch.empty((N, F), dtype=base.dtype, device=base.device)
        for r0 in range(0, R, step):
            r1 = min(R, r0 + step)
            out[r0 * P:r1 * P].view(r1 - r0, P, F).copy_(base.unsqueeze(0).expand(r1 - r0, P, F))
        if tail:
            out[R * P:].copy_(base[:tail])
        out[idx] = rows
        return out
    bt = base.t().contiguous()
    out = torch.empty((F, N), dtype=base.dtype, device=base.device)
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        out[:, r0 * P:r1 * P].unflatten(1, (r1 - r0, P)).copy_(bt.unsqueeze(1).expand(F, r1 - r0, P))
    if tail:
        out[:, R * P:].copy_(bt[:, :tail])
    out[:, idx] = rows.t()
    return out


def _bits(torch, t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


COMPARE_CHUNK = 1 << 26


def count_mismatches(torch, got, period, axis, markers, rows, report=8):
    """Bit comparison of a whole result -- (N, F) on feature axis 1, (F, N) on feature axis 0 -- with the period (P, F) broadcast along the
    minibatch and the marker `rows` at `markers`.  Returns (number of mismatching elements, [(minibatch row, feature, got bits, want bits)] of
    the first few)."""
    P, F = period.shape
    N = got.shape[0] if axis == 1 else got.shape[1]
    gi, pi, mi = _bits(torch, got), _bits(torch, period), _bits(torch, rows)
    pti = pi.t().contiguous()
    step = max(1, COMPARE_CHUNK // (P * F)) * P
    total, found = 0, []
    for a in range(0, N, step):
        b = min(N, a + step)
        full = (b - a) // P * P
        parts = []                                             # (first row, mismatch mask shaped (rows, F))
        if full:
            if axis == 1:
                ne = gi[a:a + full].view(full // P, P, F) != pi
                parts.append((a, ne.view(full, F)))
            else:
                ne = gi[:, a:a + full].unflatten(1, (full // P, P)) != pti.unsqueeze(1)
                parts.append((a, ne.reshape(F, full).t()))
        if a + full < b:                                       # the ragged tail of the operand
            n = b - a - full
            ne = (gi[a + full:b] != pi[:n]) if axis == 1 else (gi[:, a + full:b] != pti[:, :n]).t()
            parts.append((a + full, ne))
        for first, ne in parts:
            last = first + ne.shape[0]
            for j, m in enumerate(markers):
                if first <= m < last:
                    ne[m - first] = (gi[m] if axis == 1 else gi[:, m]) != mi[j]
            n_bad = int(torch.count_nonzero(ne).item())
            total += n_bad
            if n_bad and len(found) < report:
                for r, f in ne.nonzero()[:report - len(found)].tolist():
                    n = first + r
                    g = int((gi[n, f] if axis == 1 else gi[f, n]).item())
                    want = mi[markers.index(n), f] if n in markers else pi[n % P, f]
                    found.append((n, f, g, int(want.item())))
    return total, found


# ---- mutants: three addressing faults, at a scaled-down wrap distance ---------------------------------------------------------------------
def mutate(torch, correct, kind, wrap_bytes, sentinel_bits=0x7FC1):
    """A result as a faulty kernel would leave it, from the `correct` one (storage order).  wrap: the byte offset of every access taken mod
    `wrap_bytes`; clamp: the element index held in a signed register of log2(wrap_bytes) bits and clamped at its largest value; grid: the rows
    (of the stored matrix) past a grid limit never written -- the buffer keeps its sentinel."""
    flat = correct.reshape(-1)
    n = flat.numel()
    i = torch.arange(n, dtype=torch.long, device=flat.device)
    if kind == "wrap":
        out = flat[i % (wrap_bytes // flat.element_size())]
    elif kind == "clamp":
        out = flat[torch.clamp(i, max=wrap_bytes // 2 - 1)]
    elif kind == "grid":
        out = flat.clone()
        rows = correct.shape[0]
        limit = (rows * 3 // 4) * correct.shape[1]
        _bits(torch, out)[limit:] = sentinel_bits
    else:
        raise ValueError(kind)
    return out.reshape(correct.shape)


MUTANTS = ("wrap", "clamp", "grid")


def small_case(axis, dtype="bf16", N=4099 + 8, bs=32, lay="d2"):
    """A case of the table's shape at a size the CPU multiplies in full; with `SMALL_BOUNDARY` in place of 2^31 it has several boundaries
    and the markers beside them."""
    return _case("small", "host", lay, bs, axis, dtype, N, P=509)


SMALL_BOUNDARY = 1 << 17
