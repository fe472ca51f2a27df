"""CPU tier of the attention matmul tests (tests/test_bst_mm_gpu.py), on the case table of tests/_bst_mm.py:
  * the helpers: every selector case's expected values are the float64 oracle (O.nt / O.nn / O.tn) rounded once; the data are normal numbers with a
    third bf16 piece; the layouts have the row lengths, tile counts, head-batch counts and table kinds they are there for;
  * the float32 models of the kernels pass every assertion the GPU tier makes on the same inputs: bit equality on the selector cases, the
    per-unit criterion on random data, and they fix the fp32 unit bar between themselves and the model without its third piece;
  * every mutant of the models (a piece dropped or misplaced, a transposed tile, exchanged lane groups, a wrong head, a wrong batch-head slot,
    a skipped step, a stale Q tile) fails the bit equality on a case named here.
Every report is printed (`FIGURES ...`)."""
import os

import numpy as np
import pytest

import _bst_mm as M
import _f32_pieces as FP
from oracle import bst_oracle as O
from oracle import bsmm_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(c, op, inp):
    L = M.luts(c["lay"])
    if op == "nn":
        return R.round_to(O.nn(L, inp["W"], inp["B"], c["bs"], c["heads"]), c["act"])
    if op == "tn":
        return R.round_to(O.tn(L, inp["W"], inp["B"], c["bs"], c["heads"]), c["act"])
    return R.round_to(O.nt(L, inp["Q"], inp["K"], c["bs"], c["heads"]), c["score"])


def _selector_group(cases, ops=M.SEL_OPS):
    n = 0
    for c in cases:
        for op in ops:
            inp = M.selector_case(c, op)
            want = inp["want"]
            assert np.array_equal(_oracle(c, op, inp), want), (c["id"], op, "the helper's expected values are not the oracle rounded once")
            assert np.count_nonzero(want) >= 0.5 * want.size * (0.5 if op in ("nn", "tn") else 1.0), (c["id"], op, "mostly zeros: nothing selected")
            n += M.assert_bits(M.model_selector(c, op, inp), want, "model %s %s" % (c["id"], op))
    return n


# ---- layouts and data ------------------------------------------------------------------------------------------------------------------------
def test_layout_facts():
    for lkey, heads, batch in M.A_KINDS:
        lay = np.asarray(M.LAYOUTS[lkey])
        L = M.luts(lkey)
        assert L["lut_heads"] == (heads if lkey == "per_head" else 1) and lay.ndim == (3 if lkey == "per_head" else 2)
        for l2 in (lay if lay.ndim == 3 else lay[None]):
            assert (l2.sum(axis=1) == 0).any() and (l2.sum(axis=0) == 0).any(), "an empty query row and an empty key column"
            assert l2.sum(axis=1).max() > 1 and l2.sum(axis=0).max() > 1
    pairs = []
    for heads, batch, lkey in M.C_PAIRS:
        lay = np.asarray(M.LAYOUTS[lkey])
        assert lay.shape[-2:] == (3, 6) and heads * batch > 8
        assert M.luts(lkey)["lut_heads"] in (1, heads)
        pairs.append(heads * batch)
    assert pairs == [9, 10, 9, 16, 17]
    assert M.luts("c_per_head3")["lut_heads"] == 3 and M.luts("c_shared")["lut_heads"] == 1
    assert all(c["heads"] * c["batch"] <= 8 for c in M.CASES if c["sec"] != "C"), "only section C leaves the first round of xcd_head_map"
    mods = set()
    for bs, nbs in M.D_NB.items():
        for nb in nbs:
            L = M.luts("prefix%d" % nb)
            assert L["blocks"] == nb and L["nt_list"][0] == [(i // 6, i % 6) for i in range(nb)]
            mods.add(nb * (bs // 32) ** 2 % 8)
    assert mods == {0, 1, 2, 4, 7}, mods
    assert any(L8 > 6 for L8 in M.D_NB[32]) and max(M.D_NB[64]) * 4 > 8          # more than one walk, a query row change inside a walk
    L, Lt = M.luts("steps"), M.luts("steps_t")
    assert [len(e) for e in L["nn_list"][0]] == list(M.STEP_ROWS) and [len(e) for e in Lt["tn_list"][0]] == list(M.STEP_ROWS)
    assert M.row_lengths(L) == M.row_lengths(Lt, True) == [1, 2, 3, 4, 5, 8, 9, 13]
    assert L["nn_max"] * 2 == 26                                                 # bsize 64: 26 steps, seven for wave 0


def test_kernel_map_covers_every_kernel():
    nts = {M.nt_kernel(c["bs"], c["hs"], c["act"], c["flag"]) for c in M.CASES}
    xns = {M.xn_kernel(c["bs"], c["hs"], c["act"], c["score"], c["flag"]) for c in M.CASES}
    assert nts == {"bst_nt_valu_kernel", "bst_nt_mfma_kernel", "bst_nt_mfma_kernel<SPLIT>", "bst_nt_mfma_direct_kernel"}
    assert xns == {"bst_xn_valu_kernel", "bst_xn_mfma16_kernel", "bst_xn_split_kernel", "bst_xn_mfma_kernel"}
    a = M.section("A")
    assert {(c["act"], c["score"], c["flag"]) for c in a} == set(M.VARIANTS) and len(M.TYPE_PAIRS) == 6
    assert {c["bs"] for c in a} == {8, 16, 32, 64}
    assert M.xn_kernel(32, 40, "bf16", "bf16") == M.xn_kernel(64, 8, "f16", "f16") == "bst_xn_mfma_kernel"      # same-type pairs fall to the widening kernel
    assert M.xn_kernel(32, 96, "f16", "f16") == "bst_xn_mfma16_kernel" and M.nt_kernel(32, 96, "f16") == "bst_nt_mfma_direct_kernel"


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_data_is_normal_with_a_full_significand(dtype):
    rng = np.random.default_rng(5)
    x = M.data((4096,), dtype, rng)
    a = np.abs(x.astype(np.float64))
    assert a.min() >= 2.0 ** -6 and a.max() < 1.0 and (x < 0).any() and (x > 0).any()
    assert np.array_equal(R.round_to(x, dtype), x), "representable in the type"
    sel = M.selectors(4096, rng)
    assert set(np.abs(sel)) == {2.0 ** s for s in range(-3, 4)} and (sel < 0).any()
    prod = np.abs(x.astype(np.float64)[:, None] * sel.astype(np.float64)[None, :64])
    assert prod.min() >= 2.0 ** -9 > 2.0 ** -14 and prod.max() < 8.0            # normal in fp16 (and so in bf16 and fp32)
    assert np.array_equal(R.round_to(prod, dtype).astype(np.float64), prod), "a selected product is exact in the type"
    if dtype == "f32":
        share = M.third_piece_share(x)
        print("FIGURES third piece non-zero: %.3f of the fp32 data" % share)
        assert share >= 0.9
        for p in FP.split3(x):
            assert np.all((p == 0) | (np.abs(p) >= 2.0 ** -40))                    # pieces (and their products with 2^-3) far inside the normal range
        old = R.round_to(rng.uniform(-1, 1, 4096).astype(np.float16).astype(np.float32), "f32")
        assert M.third_piece_share(old) == 0.0, "values drawn through fp16 have no third piece"
    else:
        mant = np.unique(np.frexp(a)[0])
        nsig = 1 << (10 if dtype == "f16" else 7)
        assert len(mant) >= 0.9 * nsig and np.any((mant * 2 * nsig) % 2 == 1), "the significands of the type occur, the last bit included"


def test_fp32_operands_of_the_selector_cases_have_third_pieces():
    for cid, op in (("A-per_head-h2n2-b32-hs64-f32-bf16", "nn"), ("A-shared-h3n1-b64-hs40-f32-f16", "nt_k"), ("E-steps-h2n1-b32-hs40-f32-bf16-full", "tn")):
        inp = M.selector_case(M.BY_ID[cid], op)
        x = inp["B"] if op in ("nn", "tn") else inp["Q"]
        assert M.third_piece_share(x) >= 0.9, (cid, op)


# ---- section A: selector operands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k[0] for k in M.A_KINDS])
@pytest.mark.parametrize("bs,hs", M.A_SHAPES, ids=["b%d-hs%d" % s for s in M.A_SHAPES])
def test_selector_cases_section_a(bs, hs, kind):
    cases = M.section("A", bs=bs, hs=hs, lay=kind)
    assert len(cases) == 7
    _selector_group(cases)


@pytest.mark.parametrize("heads,batch,lkey", M.C_PAIRS, ids=["h%dn%d" % p[:2] for p in M.C_PAIRS])
def test_selector_cases_section_c(heads, batch, lkey):
    cases = M.section("C", heads=heads, batch=batch)
    assert len(cases) == 3
    _selector_group(cases)


@pytest.mark.parametrize("hs", M.D_HS)
@pytest.mark.parametrize("bs", sorted(M.D_NB))
def test_walk_edge_cases_section_d(bs, hs):
    cases = M.section("D", bs=bs, hs=hs)
    assert len(cases) == 4 * len(M.D_NB[bs])
    _selector_group(cases, ("nt_q", "nt_k"))
    for c in cases:
        r = M.random_case(c)
        M.check_units(M.model_nt(c, r["Q"], r["K"]), r["NT"], c, "nt", "model " + c["id"])


@pytest.mark.parametrize("lkey", ["steps", "steps_t"])
@pytest.mark.parametrize("bs,hs", M.E_SHAPES, ids=["b%d-hs%d" % s for s in M.E_SHAPES])
def test_step_edge_cases_section_e(bs, hs, lkey):
    cases = M.section("E", bs=bs, hs=hs, lay=lkey)
    assert len(cases) == 5
    _selector_group(cases, ("nn", "tn"))
    for c in cases:
        _random_xn(c, [1, 2, 3, 4, 5, 8, 9, 13] if lkey == "steps" else None, [1, 2, 3, 4, 5, 8, 9, 13] if lkey == "steps_t" else None)


def _random_xn(c, nn_lengths=None, tn_lengths=None):
    r = M.random_case(c)
    bar = M.f32_unit_bar(c)["bar"] if c["act"] == "f32" else None
    w = M.check_units(M.model_xn(c, r["W"], r["V"], False), r["NN"], c, "nn", "model " + c["id"], bar)
    assert nn_lengths is None or w["lengths"] == nn_lengths
    w = M.check_units(M.model_xn(c, r["W"], r["E"], True), r["TN"], c, "tn", "model " + c["id"], bar)
    assert tn_lengths is None or w["lengths"] == tn_lengths


# ---- section B: random data -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,hs", M.B_SHAPES, ids=["b%d-hs%d" % s for s in M.B_SHAPES])
def test_random_cases_section_b(bs, hs):
    cases = M.section("B", bs=bs, hs=hs)
    assert len(cases) == 8 and sum(c["data"] == "full" for c in cases) == 2
    for c in cases:
        r = M.random_case(c)
        if c["data"] == "full":
            assert min(M.third_piece_share(r[n]) for n in ("Q", "K", "V", "E")) >= 0.9
        M.check_units(M.model_nt(c, r["Q"], r["K"]), r["NT"], c, "nt", "model " + c["id"])
        _random_xn(c)


def test_fp32_unit_bar_sits_between_model_and_mutant():
    """The three numbers behind the fp32 unit bar of every random-data configuration with fp32 activations (profiles/bst_mm_tests.md records a run)."""
    cases = [c for c in M.CASES if c["sec"] in ("B", "E") and c["act"] == "f32" and c.get("data") == "full"]
    assert len(cases) == 8 + 12
    with open(os.path.join(ROOT, "profiles", "bst_mm_tests.md")) as f:
        doc = f.read()
    loose = []
    for c in cases:
        b = M.f32_unit_bar(c)
        print("FIGURES fp32 unit bar %s: model %.3e mutant %.3e bar %.3e%s" % (c["id"], b["noise"], b["mutant"], b["bar"], "" if b["tight"] else " (no factor of 3: the suite's bar)"))
        assert c["id"] in doc, (c["id"], "not recorded in profiles/bst_mm_tests.md")
        assert b["bar"] <= M.F32_SUITE_BAR and b["noise"] * 3.0 <= b["bar"]
        if b["tight"]:
            assert b["mutant"] >= 3.0 * b["bar"]
        else:
            loose.append(c["id"])
    assert len(loose) <= len(cases) // 4, loose
    # a configuration on G.gen_inputs data takes its sibling's bar; its own model stays a factor of 3 below it (checked by the calls above too)
    g = M.BY_ID["B-rect-h3n2-b32-hs40-f32-bf16-gen"]
    assert M.f32_unit_bar(g) == M.f32_unit_bar(M.BY_ID["B-rect-h3n2-b32-hs40-f32-bf16-full"])


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------
A32 = "A-per_head-h2n2-b32-hs64-%s"
CAUGHT_BY = {
    "third piece dropped": [(A32 % "f32-bf16", "nn"), (A32 % "f32-bf16", "tn"), (A32 % "f32-f16", "nt_q"), (A32 % "f32-f16", "nt_k"),
                            ("A-shared-h3n1-b64-hs40-f32-bf16", "nn")],
    # (a selected product rounded to bf16 IS its first piece: the nt kernels show their lower pieces through fp16 scores, or a rare rounding flip)
    "second piece dropped": [(A32 % "f32-bf16", "nn"), (A32 % "f32-f16", "nt_k"), (A32 % "f32-f16", "nt_q")],
    "third piece for the second": [(A32 % "f32-bf16", "tn"), (A32 % "f32-f16", "nt_q"), (A32 % "f32-f16", "nt_k")],
    "score tile transposed": [(A32 % "bf16-bf16", "nt_q"), (A32 % "bf16-bf16", "nn"), (A32 % "f16-bf16", "tn"), ("A-shared-h3n1-b64-hs32-f16-f16", "nn")],
    "key rows j and j^8 exchanged": [(A32 % "bf16-bf16", "nt_q"), (A32 % "bf16-bf16", "nt_k"), (A32 % "f32-bf16", "nn"), (A32 % "f16-f16", "tn")],
    "head h+1 read for head h": [(A32 % "bf16-bf16", op) for op in M.SEL_OPS] + [("A-shared-h3n1-b16-hs24-f32-f16", "nn")],
    "pair hp-8 in the slot of hp": [("C-c_per_head3-h3n3-b32-hs64-bf16-bf16", op) for op in M.SEL_OPS] + [("C-c_shared-h17n1-b64-hs32-f16-f16", "nn"),
                                                                                                     ("C-c_shared-h1n9-b32-hs64-f32-bf16", "nt_k")],
    "fifth step skipped": [("E-steps-h2n1-b32-hs64-bf16-bf16-gen", "nn"), ("E-steps_t-h2n1-b32-hs64-f32-bf16-full", "tn"), ("E-steps-h2n1-b64-hs32-f16-f16-gen", "nn")],
    "Q tile not reloaded": [("D-prefix9-h2n1-b32-hs64-f32-bf16-full", "nt_k"), ("D-prefix9-h2n1-b32-hs64-bf16-bf16-gen", "nt_q"),
                            ("D-prefix3-h2n1-b64-hs32-f16-bf16-gen", "nt_k")],
}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_caught_by_a_named_case(mutant):
    assert set(CAUGHT_BY) == set(M.MUTANTS)
    for cid, op in CAUGHT_BY[mutant]:
        c = M.BY_ID[cid]
        inp = M.selector_case(c, op)
        M.assert_bits(M.model_selector(c, op, inp), inp["want"], cid)               # the true model passes
        bad = M.mismatches(M.model_selector(c, op, inp, mutant), inp["want"])
        print("FIGURES mutant '%s' on %s %s: %d of %d elements differ, first at %s" % (mutant, cid, op, len(bad), inp["want"].size, tuple(bad[0]) if len(bad) else None))
        assert len(bad) > 0, (mutant, cid, op, "not caught")
        with pytest.raises(AssertionError):
            M.assert_bits(M.model_selector(c, op, inp, mutant), inp["want"], cid)


def test_old_inputs_could_not_see_the_third_piece():
    """On values drawn as G.gen_inputs draws them (through fp16: 11 significand bits) the third piece is zero: the model without it is bit-equal.
    The second piece carries three bits there, so the two mutants that lose it do show on the old inputs -- bit for bit; they move a result by
    2^-9, which the whole-tensor bar of 2e-6 saw as well."""
    for cid, op in CAUGHT_BY["third piece dropped"]:
        c = M.BY_ID[cid]
        inp = M.selector_case(c, op, fill="gen")
        M.assert_bits(M.model_selector(c, op, inp), inp["want"], cid)
        M.assert_bits(M.model_selector(c, op, inp, "third piece dropped"), inp["want"], cid + " without the third piece, old inputs")
    c = M.BY_ID[A32 % "f32-bf16"]
    inp = M.selector_case(c, "nn", fill="gen")
    for mutant in ("second piece dropped", "third piece for the second"):
        assert len(M.mismatches(M.model_selector(c, "nn", inp, mutant), inp["want"])) > 0
    # random data: the unit L2 of the model without its third piece on the old inputs is the model's own
    g = M.BY_ID["B-rect-h3n2-b32-hs64-f32-bf16-gen"]
    r = M.random_case(g)
    assert np.array_equal(M.model_xn(g, r["W"], r["V"], False), M.model_xn(g, r["W"], r["V"], False, mutant="third piece dropped"))


def test_first_round_cases_cannot_see_a_wrong_slot():
    """With at most 8 head-batch pairs grp of xcd_head_map is 0: the slot mutant changes nothing on a section A case."""
    c = M.BY_ID[A32 % "bf16-bf16"]
    for op in M.SEL_OPS:
        inp = M.selector_case(c, op)
        M.assert_bits(M.model_selector(c, op, inp, "pair hp-8 in the slot of hp"), inp["want"], c["id"])
