"""CPU tier of the piece-pair tests (tests/_f32_pieces.py): the split restated in NumPy, the gap in the suite's usual fp32 inputs, and -- for
the inputs of every GPU case of tests/test_f32_pieces_gpu.py, same table, same seeds -- that they can tell a wrong or missing piece pair from
fp32 accumulation noise before any kernel runs."""
import itertools

import numpy as np
import pytest

import _f32_pieces as F
import _parity as P

_INPUTS = {}


def _inputs(case):
    if case["id"] not in _INPUTS:
        _INPUTS[case["id"]] = F.make_inputs(case)
    return _INPUTS[case["id"]]


def _is_bf16(a):
    return bool(((np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & 0xFFFF) == 0).all())


def test_split3_pieces_are_bf16_and_sum_to_the_input():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-30, 31, size=200000))).astype(np.float32)
    p = F.split3(x)
    assert all(_is_bf16(q) for q in p)
    assert np.array_equal(sum(q.astype(np.float64) for q in p), x.astype(np.float64))
    # each piece is the bf16 rounding of what the earlier ones left: |p2| <= 2^-8 |p1|, |p3| <= 2^-8 |p2|
    assert (np.abs(p[1]) <= np.abs(p[0]) * 2.0 ** -8).all() and (np.abs(p[2]) <= np.abs(p[1]) * 2.0 ** -8).all()


def test_split3_steps_back_from_inf():
    x = np.array([3.4e38, -3.4e38, 3.3895314e38, 1.0], dtype=np.float32)
    p1, p2, p3 = F.split3(x)
    assert p1.view(np.uint32)[0] == 0x7F7F0000 and p1.view(np.uint32)[1] == 0xFF7F0000
    assert np.isfinite(p1).all() and np.isfinite(p2).all() and np.isfinite(p3).all()
    assert np.array_equal(p1.astype(np.float64) + p2 + p3, x.astype(np.float64))
    assert (p1[3], p2[3], p3[3]) == (1.0, 0.0, 0.0)


def test_the_usual_fp32_inputs_have_no_third_piece_and_these_do():
    W, X, E = P.make_inputs((15, 32, 32), (72, 192), (72, 160), "f32", seed=0)
    for a in (W, X, E):
        assert (F.split3(a)[2] != 0).mean() == 0.0
        assert (np.abs(F.split3(a)[1]) > 0).mean() < 0.9            # ... and a second piece of at most 3 bits
    x, share = F.full_significand((72, 192), 0.1, np.random.default_rng(0), F.SPREAD, with_share=True)
    assert (F.split3(x)[2] != 0).mean() >= 0.90
    assert share <= F.REDRAW_CAP
    assert np.array_equal(sum(q.astype(np.float64) for q in F.split3(x)), x.astype(np.float64))


def test_second_order_operand_and_partner():
    x, share = F.two_piece((72, 192), 0.1, np.random.default_rng(0), F.SPREAD, with_share=True)
    assert share <= F.REDRAW_CAP
    assert ((x.view(np.uint32) & 0x3FF) == 0).all() and (F.split3(x)[2] == 0).all() and (F.split3(x)[1] != 0).mean() > 0.9
    v = F.selector_values(64, 2, np.random.default_rng(1))
    p1, p2, p3 = F.split3(v)
    assert (p3 == 0).all() and np.array_equal(np.abs(p2), np.abs(p1) * 2.0 ** -9) and (np.log2(np.abs(p1)) % 1 == 0).all()


def test_mutant_list():
    m = F.mutants()
    assert len(m) == 12 and all(len(v) in (5, 6) for v in m.values()) and len(set(m.values())) == 12
    assert set(F.PAIRS) == {(i, j) for i in range(3) for j in range(3) if i + j <= 2}


def test_six_pair_product_is_the_product_to_2_pow_minus_24():
    rng = np.random.default_rng(2)
    x, y = F.full_significand(50000, 0.1, rng, F.SPREAD), F.full_significand(50000, 0.1, rng, F.SPREAD)
    want = x.astype(np.float64) * y
    got = F.six_pair_product(F.split3(x), F.split3(y))
    assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want)).all()
    for name, pairs in F.mutants().items():         # every mutant is further off than that on most elements
        assert (np.abs(F.six_pair_product(F.split3(x), F.split3(y), pairs) - want) > 2.0 ** -24 * np.abs(want)).mean() > 0.5, name


def test_noise_and_single_pair_mutants_at_the_reduction_lengths_of_the_cases():
    """1024-element groups of N(0, .1) full-significand data: correct fp32 accumulation sits at 1 .. 3e-7 for lengths 32 .. 128, a missing
    third-order pair at 2 .. 3e-6 -- the gap the tight bar lives in."""
    rng = np.random.default_rng(3)
    for L in (32, 64, 128):
        A, B = F.full_significand((32, L), 0.1, rng, F.SPREAD), F.full_significand((L, 32), 0.1, rng, F.SPREAD)
        assert 3e-8 <= F.fp32_noise(A, B) <= 3e-7, L
        bar = F.tight_bar([(A, B)])
        assert bar["valid"] and 1.5e-6 <= bar["mutant"] <= 4e-6 and bar["hidden"][0] in F.mutants(), (L, bar)


@pytest.mark.parametrize("case", F.CASES, ids=[c["id"] for c in F.CASES])
def test_case_inputs_can_tell_a_wrong_pair_from_noise(case):
    inp = _inputs(case)
    s = F.shapes(case)
    assert inp["redraw"] <= F.REDRAW_CAP, inp["redraw"]
    for k, shp in (("W", s["w"]), ("X", s["i"]), ("E", s["o"])):
        assert inp[k].shape == shp and inp[k].dtype == np.float32
    if case["kind"] == "selector":
        rep = F.selector_mutant_report(case, inp)
        part, full, live = F.selector_elements(case, inp)
        assert rep["exact"] and live.any()
        if case["op"] == "updat" and min(s["C"], s["K"]) > case["N"]:
            assert not live.all()                       # unselected columns: DW must hold exact zeros there
        assert rep["mutants"] and min(rep["mutants"].values()) >= 0.5, rep
        # every order of the live products gives the same fp32 sum (the kernels add them in theirs)
        first, second = (part, full) if case["role"] in ("partner-in-X", "partner-in-W") else (full, part)
        xs, es = F.split3(first[live]), F.split3(second[live])
        want = (first[live].astype(np.float64) * second[live]).astype(np.float32)
        for order in itertools.permutations(F.live_pairs(case)):
            acc = np.zeros_like(want)
            for i, j in order:
                acc = (acc + (xs[i] * es[j]).astype(np.float32)).astype(np.float32)
            assert np.array_equal(acc, want), order
    elif case["kind"] == "tight":
        groups = F.groups_of(case, inp)
        assert max(A.shape[1] for A, _ in groups) <= 128
        bar = F.tight_bar([g for g in groups if g[0].shape[1]])
        assert bar["valid"], bar
    elif case["kind"] == "yardstick(ratio<9)":           # the weaker rule only where the bar does not exist
        assert not F.tight_bar([g for g in F.groups_of(case, inp) if g[0].shape[1]])["valid"]
    elif case["kind"].startswith("alpha-beta"):
        epi, live = F.epilogue_of(case, inp)
        bar = F.tight_bar(F.groups_of(case, inp), epi, live)
        assert bar["valid"] == case["gated"], bar        # (the ungated ones are bsize 8: NO_TIGHT_BAR)
        prod = F.raw_product(case, inp)
        want = np.stack([epi(g, prod[g]) for g in range(len(prod))])
        for g in np.nonzero(live)[0]:                    # the product carries at least half of every live block's norm
            assert np.linalg.norm(want[g] - F.BETA * inp["dw0"][g]) >= 0.5 * np.linalg.norm(want[g])
    else:
        assert case["kind"] == "yardstick" and max(A.shape[1] for A, _ in F.groups_of(case, inp)) > 128
