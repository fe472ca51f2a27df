"""Layouts, inputs, expected values, float32 models (and their mutants) and the per-unit criterion for the block-sparse attention products
bst_nt / bst_nn / bst_tn (csrc/bst_kernels.h, dispatched in csrc/bst_api.hip).  Shared by tests/test_bst_mm_host.py (no GPU: the helpers agree
with the float64 oracle, the models pass every assertion on these very inputs, every mutant is caught by a named case) and
tests/test_bst_mm_gpu.py (the kernels must pass them).  NumPy only.

Two kinds of statement:
  * SELECTOR operands (section A): one operand holds +-2^s entries that pick exactly one element of the other for every output element, so
    the output is a single product, exact in fp32 on every path (native 16-bit MFMA, widening fp32 MFMA, three-piece bf16 split, V_FMA):
    the expected value is that product rounded once to the output type and the assertion is equality of bits (zeros by value).  What an
    output type can show of the bf16 pieces of an fp32 operand: fp32 outputs (nn / tn) all three; fp16 scores (nt) the second piece in
    full and the third through the rounding; bf16 scores the lower pieces only where they flip the rounding -- a selected product
    rounded to bf16 is its first piece -- which is why (f32, f16) is among the pairs the SPLIT form of the nt kernel is run with.
  * RANDOM data (section B) against the float64 oracle, _parity.assert_blocks on every unit -- nt: one block (n, h, b); nn / tn: one
    (n, h, output row-block) of BS x hs values -- plus, for fp32 outputs, a unit L2 bar that sits between the float32 model of the kernel and
    the same model without the third bf16 piece (f32_unit_bar).

Which kernel a configuration reaches is a function of (bsize, head state, types, flag): nt_kernel / xn_kernel restate the conditions of
csrc/bst_api.hip (the attention ABI has no trace word)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_bst as G
import _parity as P
import _f32_pieces as FP
from oracle import bst_oracle as O
from oracle import bsmm_oracle as R

FLAG_FP32_MFMA = 1                      # include/bst.h BST_FLAG_FP32_MFMA
TYPE_PAIRS = (("f32", "bf16"), ("f32", "f16"), ("f16", "f16"), ("f16", "bf16"), ("bf16", "bf16"), ("bf16", "f16"))      # (activations, scores): by_types
VARIANTS = tuple((a, s, 0) for a, s in TYPE_PAIRS) + (("f32", "bf16", FLAG_FP32_MFMA),)
F32_SUITE_BAR = P.L2_BAR["f32"]         # 2e-6: the fp32 unit bar never exceeds it
SEL_OPS = ("nt_q", "nt_k", "nn", "tn")  # nt with Q one-hot, nt with K one-hot, nn, tn
PIECE_MUTANTS = ("third piece dropped", "second piece dropped", "third piece for the second")
MUTANTS = PIECE_MUTANTS + ("score tile transposed", "key rows j and j^8 exchanged", "head h+1 read for head h", "pair hp-8 in the slot of hp",
                           "fifth step skipped", "Q tile not reloaded")


# ---- which kernel (csrc/bst_api.hip) ----------------------------------------------------------------------------------------------------
def nt_kernel(bsize, hs, act, flag=0):
    if bsize < 32:
        return "bst_nt_valu_kernel"
    if hs in (32, 64, 128):
        return "bst_nt_mfma_kernel<SPLIT>" if act == "f32" and not flag else "bst_nt_mfma_kernel"
    return "bst_nt_mfma_direct_kernel"


def xn_kernel(bsize, hs, act, score, flag=0):
    if bsize < 32:
        return "bst_xn_valu_kernel"
    if act != "f32" and act == score and hs % 32 == 0:
        return "bst_xn_mfma16_kernel"
    if act == "f32" and score == "bf16" and not flag:
        return "bst_xn_split_kernel"
    return "bst_xn_mfma_kernel"


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def holes(heads_l, Qb, Kb, nblocks, seed):
    """[heads_l][Qb][Kb] (2-D for heads_l == 1) with `nblocks` blocks per head, query row (h + 1) % Qb and key column (h + 2) % Kb empty."""
    rs = np.random.RandomState(seed)
    lay = np.zeros((heads_l, Qb, Kb), dtype=np.int32)
    for h in range(heads_l):
        qe, ke = (h + 1) % Qb, (h + 2) % Kb
        cells = [(q, k) for q in range(Qb) if q != qe for k in range(Kb) if k != ke]
        for c in rs.permutation(len(cells))[:nblocks]:
            lay[h][cells[c]] = 1
    return lay if heads_l > 1 else lay[0]


def prefix(nb):
    """3 x 6, the first nb cells (row-major) present: the query row changes inside a walk of NT_NB = 8 tiles."""
    lay = np.zeros(18, dtype=np.int32)
    lay[:nb] = 1
    return lay.reshape(3, 6)


STEP_ROWS = (0, 1, 2, 3, 4, 5, 8, 9, 13)


def steps_layout():
    """9 x 13: query rows of 0, 1, 2, 3, 4, 5, 8, 9 and 13 blocks (seeded random subsets of the key blocks)."""
    rs = np.random.RandomState(913)
    lay = np.zeros((9, 13), dtype=np.int32)
    for q, n in enumerate(STEP_ROWS):
        lay[q, np.sort(rs.permutation(13)[:n])] = 1
    return lay


LAYOUTS = {"per_head": holes(2, 4, 5, 8, 31), "shared": holes(1, 4, 5, 8, 32),
           "c_per_head3": holes(3, 3, 6, 6, 33), "c_per_head2": holes(2, 3, 6, 6, 34), "c_shared": holes(1, 3, 6, 6, 35),
           "steps": steps_layout(), "steps_t": np.ascontiguousarray(steps_layout().T), "rect": G.layouts()["rect_3heads"]}
for _nb in range(1, 18):
    LAYOUTS["prefix%d" % _nb] = prefix(_nb)
for _l in LAYOUTS.values():
    _l.flags.writeable = False


@functools.lru_cache(maxsize=None)
def luts(lkey):
    return O.build_luts(LAYOUTS[lkey])


def row_lengths(L, trans=False):
    """sorted set of non-zero list lengths over all heads"""
    return sorted({len(e) for per in L["tn_list" if trans else "nn_list"] for e in per if e})


# ---- the case tables ----------------------------------------------------------------------------------------------------------------------
def _cfg(sec, lkey, heads, batch, bs, hs, act, score, flag, **kw):
    c = dict(sec=sec, lay=lkey, heads=heads, batch=batch, bs=bs, hs=hs, act=act, score=score, flag=flag)
    c.update(kw)
    c["id"] = "%s-%s-h%dn%d-b%d-hs%d-%s-%s%s%s" % (sec, lkey, heads, batch, bs, hs, act, score, "-f32mfma" if flag else "", "-" + kw["data"] if "data" in kw else "")
    return c


A_SHAPES = tuple((bs, hs) for bs in (32, 64) for hs in (32, 64, 128, 96, 40, 8)) + tuple((bs, hs) for bs in (8, 16) for hs in (8, 24, 72))
A_KINDS = (("per_head", 2, 2), ("shared", 3, 1))                      # layout, heads, batch
C_PAIRS = ((3, 3, "c_per_head3"), (5, 2, "c_shared"), (1, 9, "c_shared"), (2, 8, "c_per_head2"), (17, 1, "c_shared"))      # heads, batch, layout
C_TYPES = (("bf16", "bf16", 32, 64), ("f32", "bf16", 32, 64), ("f16", "f16", 64, 32))
B_SHAPES = ((32, 64), (32, 40), (64, 32), (16, 24))
D_NB = {32: (1, 2, 7, 8, 9, 10, 15, 16, 17), 64: (1, 2, 3, 4, 5)}
D_HS = (32, 64, 128, 40, 96)
D_VARIANTS = (("f32", "bf16", 0), ("f32", "bf16", 1), ("bf16", "bf16", 0), ("f16", "bf16", 0))
E_SHAPES = ((32, 64), (64, 32), (32, 40))
E_VARIANTS = (("f32", "bf16", 0), ("f32", "bf16", 1), ("bf16", "bf16", 0), ("f16", "f16", 0), ("f16", "bf16", 0))


def _cases():
    out = []
    for bs, hs in A_SHAPES:
        for lkey, heads, batch in A_KINDS:
            for act, score, flag in VARIANTS:
                out.append(_cfg("A", lkey, heads, batch, bs, hs, act, score, flag))
    for heads, batch, lkey in C_PAIRS:
        for act, score, bs, hs in C_TYPES:
            out.append(_cfg("C", lkey, heads, batch, bs, hs, act, score, 0))
    for bs, hs in B_SHAPES:
        for act, score in TYPE_PAIRS:
            for data in ("gen", "full") if act == "f32" else ("gen",):
                out.append(_cfg("B", "rect", 3, 1 if bs == 64 else 2, bs, hs, act, score, 0, data=data))
    for bs, nbs in D_NB.items():
        for nb in nbs:
            for hs in D_HS:
                for act, score, flag in D_VARIANTS:
                    out.append(_cfg("D", "prefix%d" % nb, 2, 1, bs, hs, act, score, flag, data="full" if act == "f32" else "gen", nb=nb))
    for lkey in ("steps", "steps_t"):
        for bs, hs in E_SHAPES:
            for act, score, flag in E_VARIANTS:
                out.append(_cfg("E", lkey, 2, 1, bs, hs, act, score, flag, data="full" if act == "f32" else "gen"))
    for i, c in enumerate(out):
        c["seed"] = 40000 + i
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}


def section(sec, **match):
    return [c for c in CASES if c["sec"] == sec and all(c[k] == v for k, v in match.items())]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def data(shape, dtype, rng):
    """Magnitude in [2^-6, 1), random sign, full random significand of the type (24 / 11 / 8 bits), as float32: every input, piece, product with
    a +-2^s selector (|s| <= 3) and output is a normal number in fp32, fp16 and bf16.  fp32 values whose three bf16 pieces do not sum back
    exactly in every order are redrawn (tests/_f32_pieces.py)."""
    n = int(np.prod(shape))
    if dtype == "f32":
        def raw(m):
            bits = (rng.integers(0, 2, m).astype(np.uint32) << 31) | (rng.integers(121, 127, m).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, m).astype(np.uint32)
            return bits.view(np.float32)
        x = raw(n)
        bad = ~FP._sums_back_in_every_order(x)
        for _ in range(64):
            if not bad.any():
                break
            x[bad] = raw(int(bad.sum()))
            bad[bad] = ~FP._sums_back_in_every_order(x[bad])
        assert not bad.any()
    else:
        mb = 10 if dtype == "f16" else 7
        x = (rng.choice([-1.0, 1.0], n) * (1.0 + rng.integers(0, 1 << mb, n) / float(1 << mb)) * np.exp2(rng.integers(-6, 0, n))).astype(np.float32)
    return x.reshape(shape)


def selectors(n, rng):
    """n values +-2^s, s in -3 .. 3"""
    return (np.exp2(rng.integers(-3, 4, size=n)) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


def third_piece_share(x):
    return float((FP.split3(np.asarray(x, dtype=np.float32).ravel())[2] != 0).mean())


def _dims(c):
    L = luts(c["lay"])
    return L, c["batch"], c["heads"], c["bs"], c["hs"], L["ctx_blks_q"], L["ctx_blks_k"]


def _hl(L, h):
    return h if L["lut_heads"] > 1 else 0


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


@functools.lru_cache(maxsize=256)
def _selector_case(cid, op, fill):
    c = BY_ID[cid]
    L, N, H, bs, hs, Qb, Kb = _dims(c)
    rng = np.random.default_rng(c["seed"] * 8 + SEL_OPS.index(op))
    act, score = c["act"], c["score"]

    def full(shape):
        if fill == "gen":        # the old inputs: uniform(-1, 1) through fp16 (11 significand bits: no third piece), then the storage type
            return R.round_to(rng.uniform(-1.0, 1.0, shape).astype(np.float16).astype(np.float32), act)
        return data(shape, act, rng)

    if op in ("nn", "tn"):
        trans = op == "tn"
        ctx_c, ctx_b = (Kb, Qb) if trans else (Qb, Kb)
        W = np.zeros((N, H, L["blocks"], bs, bs), dtype=np.float32)
        B = full((N, ctx_b * bs, H * hs))
        B5 = B.reshape(N, ctx_b, bs, H, hs)
        want = np.zeros((N, ctx_c, bs, H, hs), dtype=np.float32)
        ar = np.arange(bs)
        for h in range(H):
            for oc, ent in enumerate(L["tn_list" if trans else "nn_list"][_hl(L, h)]):
                if not ent:
                    continue
                ids, others = np.array([b for b, _ in ent]), np.array([x for _, x in ent])
                for n in range(N):
                    e, x, v = rng.integers(0, len(ent), bs), rng.integers(0, bs, bs), selectors(bs, rng)
                    if trans:
                        W[n, h, ids[e], x, ar] = v                 # column j = ar of the output's key block, row i = x of one block of its list
                    else:
                        W[n, h, ids[e], ar, x] = v                 # row i = ar, column j = x
                    want[n, oc, :, h, :] = v[:, None] * B5[n, others[e], x, h, :]
        return _frozen(dict(W=W, B=B, want=R.round_to(want.reshape(N, ctx_c * bs, H * hs), act)))
    # nt: the one-hot operand has one feature per (batch entry, row, head)
    rows_q, rows_k = Qb * bs, Kb * bs
    rows_sel = rows_q if op == "nt_q" else rows_k
    f = rng.integers(0, hs, (N, rows_sel, H))
    v = selectors(N * rows_sel * H, rng).reshape(N, rows_sel, H)
    sel = np.zeros((N, rows_sel, H, hs), dtype=np.float32)
    n_i, r_i, h_i = np.meshgrid(np.arange(N), np.arange(rows_sel), np.arange(H), indexing="ij")
    sel[n_i, r_i, h_i, f] = v
    other = full((N, rows_k if op == "nt_q" else rows_q, H * hs))
    o4 = other.reshape(N, -1, H, hs)
    want = np.zeros((N, H, L["blocks"], bs, bs), dtype=np.float32)
    for h in range(H):
        for b, (q, k) in enumerate(L["nt_list"][_hl(L, h)]):
            for n in range(N):
                if op == "nt_q":         # S[i, j] = v_i * K[j, f_i]
                    fi, vi = f[n, q * bs:(q + 1) * bs, h], v[n, q * bs:(q + 1) * bs, h]
                    want[n, h, b] = (o4[n, k * bs:(k + 1) * bs, h][:, fi] * vi[None, :]).T
                else:                    # S[i, j] = Q[i, f_j] * v_j
                    fj, vj = f[n, k * bs:(k + 1) * bs, h], v[n, k * bs:(k + 1) * bs, h]
                    want[n, h, b] = o4[n, q * bs:(q + 1) * bs, h][:, fj] * vj[None, :]
    sel = sel.reshape(N, rows_sel, H * hs)
    Q, K = (sel, other) if op == "nt_q" else (other, sel)
    return _frozen(dict(Q=Q, K=K, want=R.round_to(want, score)))


def selector_case(c, op, fill="full"):
    """Inputs and the expected result (float32 arrays holding storage-type values) of one selector operation of a configuration.
    nn / tn: W (scores: selectors), B (activations: data), want [N, rows, heads * hs];  nt_q / nt_k: Q, K, want [N, heads, blocks, bs, bs]."""
    return _selector_case(c["id"], op, fill)


@functools.lru_cache(maxsize=64)
def _random_case(cid):
    c = BY_ID[cid]
    L, N, H, bs, hs, Qb, Kb = _dims(c)
    act, score = c["act"], c["score"]
    inp = G.gen_inputs(np.asarray(LAYOUTS[c["lay"]]), H, bs, hs, N, L["blocks"], c["seed"])
    if c.get("data") == "full":
        rng = np.random.default_rng(c["seed"])
        for name in ("Q", "K", "V", "E"):
            inp[name] = FP.full_significand(inp[name].shape, 0.5, rng, 2)
    Q, K, V, E = (R.round_to(inp[n], act) for n in ("Q", "K", "V", "E"))
    W = R.round_to(inp["W"], score)
    return _frozen(dict(Q=Q, K=K, V=V, E=E, W=W, NT=O.nt(L, Q, K, bs, H), NN=O.nn(L, W, V, bs, H), TN=O.tn(L, W, E, bs, H)))


def random_case(c):
    """G.gen_inputs data (fp32 activations of a data == "full" configuration: _f32_pieces.full_significand) in the storage types, and the
    unrounded float64 oracle of nt(Q, K), nn(W, V), tn(W, E)."""
    return _random_case(c["id"])


# ---- float32 models of the kernels -----------------------------------------------------------------------------------------------------
def _source_pair(n, h, heads, mutant):
    """(batch entry, head) whose activations the model reads for the output slot (n, h)"""
    if mutant == "head h+1 read for head h":
        return n, (h + 1) % heads
    if mutant == "pair hp-8 in the slot of hp":
        hp = n * heads + h
        if hp >= 8:
            return (hp - 8) // heads, (hp - 8) % heads
    return n, h


def _pieces(x, mutant):
    p = list(FP.split3(x))
    if mutant == "third piece dropped":
        p[2] = np.zeros_like(p[2])
    elif mutant == "second piece dropped":
        p[1] = np.zeros_like(p[1])
    elif mutant == "third piece for the second":
        p[1] = p[2]
    return p


def _mm(a, b, seq):
    """a [.., m, k] @ b [.., k, n] in float32: NumPy's matmul, or (seq) one rounded product and one rounded addition per k"""
    if not seq:
        return np.matmul(a, b)
    acc = np.zeros(a.shape[:-1] + b.shape[-1:], dtype=np.float32)
    for k in range(a.shape[-1]):
        acc = acc + a[..., :, k, None] * b[..., k, None, :]
    return acc


def model_nt(c, Q, K, mutant=None, seq=False):
    """bst_nt in NumPy float32, tile by tile as the kernel of the configuration walks them: fp32 accumulation over the features in chunks of 32,
    two chains (even and odd chunks) in the staged kernel, one in the direct and V_FMA kernels; the SPLIT form multiplies bf16 pieces, the
    three small products into one chain, the three large ones into the other; one rounding to the score type."""
    L, N, H, bs, hs, Qb, Kb = _dims(c)
    kern = nt_kernel(bs, hs, c["act"], c["flag"])
    staged, split = kern.startswith("bst_nt_mfma_kernel"), kern.endswith("<SPLIT>")
    T = min(bs, 32)
    SUB = bs // T
    Q4 = np.asarray(Q, dtype=np.float32).reshape(N, Qb * bs, H, hs)
    K4 = np.asarray(K, dtype=np.float32).reshape(N, Kb * bs, H, hs)
    out = np.zeros((N, H, L["blocks"], bs, bs), dtype=np.float32)
    ar = np.arange(T)
    for n in range(N):
        for h in range(H):
            ns, hsrc = _source_pair(n, h, H, mutant)
            nt_list = L["nt_list"][_hl(L, h)]
            qrow = np.array([q * bs + T * ti for q, k in nt_list for ti in range(SUB) for tj in range(SUB)])
            krow = np.array([k * bs + T * tj for q, k in nt_list for ti in range(SUB) for tj in range(SUB)])
            if mutant == "Q tile not reloaded" and staged:
                qrow = qrow[8 * (np.arange(len(qrow)) // 8)]          # the Q tile of the walk's first tile (NT_NB = 8)
            A = Q4[ns][qrow[:, None] + ar, hsrc]                      # [tiles, T (i), hs]
            B = K4[ns][krow[:, None] + ar, hsrc]                      # [tiles, T (j), hs]
            if mutant == "key rows j and j^8 exchanged" and T >= 16:
                B = B[:, ar ^ 8]
            acc = [np.zeros((len(qrow), T, T), dtype=np.float32) for _ in range(2)]
            for ci, f0 in enumerate(range(0, hs, 32)):
                a, b = A[..., f0:f0 + 32], np.swapaxes(B[..., f0:f0 + 32], 1, 2)
                if split:
                    qp, kp = _pieces(a, mutant), _pieces(b, mutant)
                    for i, j in ((0, 2), (2, 0), (1, 1)):             # (Q piece, K piece): kp2 qp0, kp0 qp2, kp1 qp1
                        acc[1] = acc[1] + _mm(qp[i], kp[j], seq)
                    for i, j in ((0, 1), (1, 0), (0, 0)):
                        acc[0] = acc[0] + _mm(qp[i], kp[j], seq)
                else:
                    w = ci % 2 if staged else 0
                    acc[w] = acc[w] + _mm(a, b, seq)
            tile = acc[0] + acc[1]
            if mutant == "score tile transposed":
                tile = np.swapaxes(tile, 1, 2)
            out[n, h] = tile.reshape(L["blocks"], SUB, SUB, T, T).transpose(0, 1, 3, 2, 4).reshape(L["blocks"], bs, bs)
    return R.round_to(out, c["score"])


def model_xn(c, W, B, trans, mutant=None, seq=False, split=None):
    """bst_nn / bst_tn in NumPy float32: the steps (entry, 32-wide slice of the contraction index) of an output block dealt to four partial
    sums, then ((p0 + p1) + p2) + p3 (xn_reduce_store); the split form adds the products of the third, second and first bf16 piece of the
    activations in that order; the V_FMA kernel (bsize 8 / 16) is one chain over the entries; one rounding to the activation type."""
    L, N, H, bs, hs, Qb, Kb = _dims(c)
    kern = xn_kernel(bs, hs, c["act"], c["score"], c["flag"])
    valu = kern == "bst_xn_valu_kernel"
    if split is None:
        split = kern == "bst_xn_split_kernel"
    ctx_c, ctx_b = (Kb, Qb) if trans else (Qb, Kb)
    width = bs if valu else 32
    W = np.asarray(W, dtype=np.float32)
    B5 = np.asarray(B, dtype=np.float32).reshape(N, ctx_b, bs, H, hs)
    out = np.zeros((N, ctx_c, bs, H, hs), dtype=np.float32)
    ar = np.arange(bs)
    for n in range(N):
        for h in range(H):
            ns, hsrc = _source_pair(n, h, H, mutant)
            for oc, ent in enumerate(L["tn_list" if trans else "nn_list"][_hl(L, h)]):
                parts = [np.zeros((bs, hs), dtype=np.float32) for _ in range(4)]
                step = 0
                for b, x in ent:
                    Wb = W[n, h, b].T if trans else W[n, h, b]                    # [output row, contraction index]
                    if mutant == "score tile transposed" and bs >= 32:
                        S = bs // 32
                        Wb = Wb.reshape(S, 32, S, 32).transpose(0, 3, 2, 1).reshape(bs, bs)
                    Bb = B5[ns, x, :, hsrc, :]
                    if mutant == "key rows j and j^8 exchanged" and bs >= 16:
                        Bb = Bb[ar ^ 8]
                    for k0 in range(0, bs, width):
                        step += 1
                        if mutant == "fifth step skipped" and step == 5:
                            continue
                        w = 0 if valu else (step - 1) % 4
                        a, bb = Wb[:, k0:k0 + width], Bb[k0:k0 + width]
                        if split:
                            p = _pieces(bb, mutant)
                            for i in (2, 1, 0):
                                parts[w] = parts[w] + _mm(a, p[i], seq)
                        else:
                            parts[w] = parts[w] + _mm(a, bb, seq)
                out[n, oc, :, h, :] = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    return R.round_to(out.reshape(N, ctx_c * bs, H * hs), c["act"])


def model_selector(c, op, inp, mutant=None):
    if op in ("nn", "tn"):
        return model_xn(c, inp["W"], inp["B"], op == "tn", mutant)
    return model_nt(c, inp["Q"], inp["K"], mutant)


# ---- the assertions ---------------------------------------------------------------------------------------------------------------------
def mismatches(got, want):
    """coordinates where the two differ (zeros compare by value: +0 == -0; a NaN differs from everything)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.argwhere(~(got == want))


def assert_bits(got, want, ctx=""):
    """Section A: every element equal to the expected storage value."""
    bad = mismatches(got, want)
    if len(bad):
        got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
        first = ["%s got %r want %r" % (tuple(int(i) for i in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in bad[:8]]
        raise AssertionError("%s: %d of %d elements differ; first at [%s]" % (ctx, len(bad), got.size, "; ".join(first)))
    return got.size


def nt_units(c):
    L = luts(c["lay"])
    return [("batch %d head %d block %d" % (n, h, b), (n, h, b)) for n in range(c["batch"]) for h in range(c["heads"]) for b in range(L["blocks"])]


def xn_units(c, trans):
    """(label, index into [N, ctx_c, bs, heads, hs], list length) per (n, h, output block); length 0: the block must be zero"""
    L = luts(c["lay"])
    out = []
    for h in range(c["heads"]):
        for oc, ent in enumerate(L["tn_list" if trans else "nn_list"][_hl(L, h)]):
            for n in range(c["batch"]):
                out.append(("batch %d head %d %s block %d (%d blocks)" % (n, h, "key" if trans else "query", oc, len(ent)), (n, oc, slice(None), h), len(ent)))
    return out


def check_units(got, want64, c, op, ctx="", f32_bar=None):
    """_parity.assert_blocks (groups = 1) on every unit of an nt / nn / tn result, every unit examined before anything is raised; fp32 outputs
    also meet `f32_bar` per unit.  Returns the worst figures and, for nn / tn, the list lengths examined."""
    L, N, H, bs, hs, Qb, Kb = _dims(c)
    got, want64 = np.asarray(got), np.asarray(want64)
    if op == "nt":
        dtype, units = c["score"], [(lab, ix, 1) for lab, ix in nt_units(c)]
    else:
        dtype = c["act"]
        ctx_c = Kb if op == "tn" else Qb
        got, want64 = got.reshape(N, ctx_c, bs, H, hs), want64.reshape(N, ctx_c, bs, H, hs)
        units = xn_units(c, op == "tn")
    worst = dict(unit_l2=0.0, elem_flips=0, elem_bad=0, units=0)
    fails, lengths = [], set()
    for lab, ix, length in units:
        g, w = got[ix], want64[ix]
        if length == 0:
            if np.any(g != 0):
                fails.append("%s: an empty list gives non-zero output" % lab)
            continue
        lengths.add(length)
        rep = P.block_report(g, w, dtype, 1)
        worst["unit_l2"] = max(worst["unit_l2"], rep["tensor_l2"])
        worst["elem_flips"] += rep["elem_flips"]
        worst["elem_bad"] += rep["elem_bad"]
        worst["units"] += 1
        try:
            P.assert_blocks(g, w, dtype, 1, ctx="%s %s" % (ctx, lab))
            if dtype == "f32" and f32_bar is not None:
                assert rep["tensor_l2"] <= f32_bar, ("%s %s" % (ctx, lab), "fp32 unit L2 %.3e above %.3e" % (rep["tensor_l2"], f32_bar))
        except AssertionError as err:
            fails.append(str(err))
    worst["lengths"] = sorted(lengths)
    print("FIGURES %s %s: unit_l2 %.3e elem_flips %d elem_bad %d over %d units%s%s" %
          (ctx, op, worst["unit_l2"], worst["elem_flips"], worst["elem_bad"], worst["units"],
           "" if op == "nt" else ", lists of %s blocks" % worst["lengths"], "" if f32_bar is None or dtype != "f32" else ", fp32 bar %.3e" % f32_bar))
    assert not fails, "%s %s: %d of %d units fail\n  " % (ctx, op, len(fails), len(units)) + "\n  ".join(fails[:6])
    return worst


def _unit_l2s(got, want64, c, trans):
    L, N, H, bs, hs, Qb, Kb = _dims(c)
    ctx_c = Kb if trans else Qb
    g = np.asarray(got, dtype=np.float64).reshape(N, ctx_c, bs, H, hs)
    w = np.asarray(want64).reshape(N, ctx_c, bs, H, hs).astype(np.float32).astype(np.float64)
    return [float(np.linalg.norm(g[ix] - w[ix]) / np.linalg.norm(w[ix])) for _, ix, length in xn_units(c, trans) if length]


@functools.lru_cache(maxsize=None)
def _f32_unit_bar(cid):
    c = BY_ID[cid]
    full = BY_ID[cid[:-len("gen")] + "full"] if c.get("data") == "gen" else c         # a section B pair: the bar of the full-significand sibling
    r = random_case(full)
    noise, mutant = 0.0, np.inf
    for trans, b, want in ((False, r["V"], r["NN"]), (True, r["E"], r["TN"])):
        for seq in (False, True):
            noise = max(noise, max(_unit_l2s(model_xn(full, r["W"], b, trans, seq=seq), want, full, trans)))
        mutant = min(mutant, min(_unit_l2s(model_xn(full, r["W"], b, trans, mutant="third piece dropped", split=True), want, full, trans)))
    bar = min(float(np.sqrt(noise * mutant)), F32_SUITE_BAR)
    tight = bar >= 3.0 * noise and mutant >= 3.0 * bar
    return dict(noise=noise, mutant=mutant, bar=bar if tight else F32_SUITE_BAR, tight=tight)


def f32_unit_bar(c):
    """For a random-data configuration with fp32 activations: `noise`, the worst unit L2 (against the float64 oracle rounded to fp32) of the
    float32 model in the kernel's order, with NumPy's matmul and with one rounding per product and addition; `mutant`, the best-hidden unit of
    the three-piece model without its third piece; bar = their geometric mean, never above 2e-6; `tight` where a factor of 3 lies on either
    side -- elsewhere the bar stays 2e-6.  A configuration on G.gen_inputs data (no third piece: the mutant is the model) takes the figures
    of its full-significand sibling."""
    assert c["act"] == "f32"
    return _f32_unit_bar(c["id"])
