"""CPU tier of the big-operand tests (tests/_big_operands.py): the conditions on the data that make bit equality the right check on
operands nobody can multiply in float64, asserted by calling the builders the GPU tier calls.

  1. exactness: every partial sum of every output element stays below 2^24 units, for every case of the table;
  2. no two rows whose byte offsets differ by a multiple of 2^31 hold equal contents (why the period is odd);
  3. the period / tail / marker arithmetic of the expected values against the float64 oracle of a WHOLE small operand, and three addressing
     faults -- byte offset mod 2^k, element index clamped as a signed value, rows past a grid limit unwritten -- each failing the comparison
     function of the GPU tier with a coordinate, at a scaled-down wrap distance."""
import numpy as np
import pytest
import torch

import _big_operands as B

IDS = [c["id"] for c in B.CASES]


def test_table_is_ordered_and_bounded():
    sizes = [c["bytes"] for c in B.CASES]
    assert sizes == sorted(sizes)
    assert max(sizes) <= B.MAX_LIVE, [(c["id"], c["bytes"] / B.GIB) for c in B.CASES if c["bytes"] > B.MAX_LIVE]
    assert all(c["P"] % 2 == 1 and c["P"] > 100 for c in B.CASES)
    # both sides of every threshold: each predicate's quantity has a case below and a case at / above it
    def sides(pred, quantity, limit):
        q = [quantity(c) for c in B.CASES if pred(c)]
        return any(v < limit for v in q) and any(v >= limit for v in q)
    E = lambda c: c["N"] * max(c["C"], c["K"])
    assert sides(lambda c: c["bs"] == 32 and c["dtype"] == "bf16" and c["variant"] == 3, E, 1 << 30)           # streaming kernel
    assert sides(lambda c: c["bs"] == 8 and c["dtype"] == "bf16", E, 1 << 30)                                  # s8_big
    assert sides(lambda c: c["bs"] == 64, E, 1 << 30)                                                          # native64
    assert sides(lambda c: c["bs"] == 32 and c["dtype"] == "f32" and c["axis"] == 1, E, 1 << 30)               # fp32 streaming split
    assert sides(lambda c: c["bs"] == 8 and c["dtype"] == "f32", E, 1 << 30)                                   # bsize-8 fp32 split
    assert sides(lambda c: c["bs"] == 16 and c["axis"] == 0 and c["dtype"] == "bf16" and c["C"] == 1024, E, 1 << 31)   # rows_ok
    assert sides(lambda c: c["bs"] == 16 and c["axis"] == 0 and c["dtype"] == "f32", E, 1 << 31)               # fp32 row-owner kernel
    assert sides(lambda c: c["variant"] == 4, lambda c: c["N"] * c["C"] * 2, 1 << 32)                          # mid kernel
    for bs in (32, 16):                                                                                       # staged plans, feature axis 0
        assert sides(lambda c: c["family"] == "rowstride" and c["bs"] == bs, lambda c: c["N"] * 256, 1 << 32)
    assert any(c["N"] * c["C"] > (1 << 31) for c in B.CASES) and any(c["N"] * c["C"] * B.ESZ[c["dtype"]] > (1 << 32) for c in B.CASES)


def test_marker_rows_straddle_every_boundary():
    for c in B.CASES:
        e = B.ESZ[c["dtype"]]
        for F in (c["C"], c["K"]):
            rows = B.marker_rows(c["N"], F, e, c["axis"])
            assert rows[0] == 0 and rows[-1] == c["N"] - 1
            for b in range(B.BOUNDARY, c["N"] * F * e, B.BOUNDARY):
                el = b // e                                    # first element past the boundary, and the one before it
                for x in (el - 1, el):
                    assert (x // F if c["axis"] == 1 else x % c["N"]) in rows, (c["id"], b)
            assert set(rows) <= set(B.case_markers(c))


@pytest.mark.parametrize("case", B.CASES, ids=IDS)
def test_exactness_and_distinct_wrap_partners(case):
    ex = B.expected(case)
    bound = B.exactness(case, ex)
    print("big-operands %s units DW %.0f Y %d DX %d of %d, markers %s" % (case["id"], bound["DW"], bound["Y"], bound["DX"], B.LIMIT_UNITS, ex["markers"]))
    assert bound["DW"] < B.LIMIT_UNITS and bound["Y"] < B.LIMIT_UNITS and bound["DX"] < B.LIMIT_UNITS, (case["id"], bound)
    # the expected values themselves are multiples of their unit and exact in fp32
    for name, unit in (("Yp", B.W_UNIT * B.A_UNIT), ("Ym", B.W_UNIT * B.A_UNIT), ("DXp", B.W_UNIT * B.A_UNIT), ("DW", B.A_UNIT * B.A_UNIT)):
        q = ex[name] / unit
        assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < B.LIMIT_UNITS, (case["id"], name)
    assert np.abs(ex["DW"]).max() / (B.A_UNIT * B.A_UNIT) <= bound["DW"]
    # markers: values no base row holds
    assert np.abs(ex["X"]).max() < B.MARKER * B.A_UNIT and np.abs(ex["E"]).max() < B.MARKER * B.A_UNIT
    assert (np.abs(ex["Xm"]) == B.MARKER * B.A_UNIT).all() and (np.abs(ex["Em"]) == B.MARKER * B.A_UNIT).all()
    assert B.wrap_partners_distinct(case, ex), case["id"]


def test_an_even_period_has_equal_wrap_partners():
    """The check of condition 2 can fail: with a period that divides the wrap distance the partners are copies."""
    c = dict(next(c for c in B.CASES if c["family"] == "long" and c["axis"] == 1 and c["bs"] == 32 and c["N"] > (1 << 21)), P=512)
    ex = B.base_data(c, 2)
    assert not B.wrap_partners_distinct(c, ex)


def _whole(case, ex, what):
    """(the operand pair, the float64 oracle over the WHOLE small operand) in minibatch-major float64."""
    N, P = case["N"], case["P"]
    rows = np.arange(N) % P
    X, E = ex["X"][rows].copy(), ex["E"][rows].copy()
    X[ex["markers"]], E[ex["markers"]] = ex["Xm"], ex["Em"]
    if what == "Y":
        return B._fprop(case, X, ex["W"])
    if what == "DX":
        return B._bprop(case, E, ex["W"])
    return B._updat(case, X, E)


SMALL = [(axis, dtype) for axis in (0, 1) for dtype in ("bf16", "f32")]


@pytest.mark.parametrize("axis,dtype", SMALL, ids=["a%d-%s" % s for s in SMALL])
def test_expected_values_and_mutants(axis, dtype):
    case = B.small_case(axis, dtype)
    ex = B.expected(case, B.SMALL_BOUNDARY)
    marks = ex["markers"]
    assert len(marks) >= 2 + 2 * ((case["N"] * case["C"] * B.ESZ[dtype] - 1) // B.SMALL_BOUNDARY) - 2 and len(marks) > 4
    # the operand the fill makes is the periodic one with its markers
    st = lambda a: B.to_storage(torch, a, dtype)
    x = B.fill(torch, st(ex["X"]), case["N"], axis, marks, st(ex["Xm"]))
    rows = np.arange(case["N"]) % case["P"]
    X = ex["X"][rows].copy()
    X[marks] = ex["Xm"]
    assert np.array_equal(x.float().numpy().astype(np.float64), X if axis else X.T)
    # DW: R * period + tail + marker terms is the oracle of the whole operand
    assert np.array_equal(ex["DW"], _whole(case, ex, "DW"))
    for what, per, mk in (("Y", "Yp", "Ym"), ("DX", "DXp", "DXm")):
        want = _whole(case, ex, what)
        correct = st(want if axis else want.T)
        period, mrows = st(ex[per]), st(ex[mk])
        bad, found = B.count_mismatches(torch, correct, period, axis, marks, mrows)
        assert bad == 0 and not found, (what, bad, found)
        # ... also when the comparison runs in many small chunks
        old = B.COMPARE_CHUNK
        try:
            B.COMPARE_CHUNK = case["P"] * period.shape[1] * 3
            assert B.count_mismatches(torch, correct, period, axis, marks, mrows)[0] == 0
        finally:
            B.COMPARE_CHUNK = old
        # one flipped element is found where it is
        one = correct.clone()
        n, f = case["N"] - 3, 5
        B._bits(torch, one)[(n, f) if axis else (f, n)] ^= 1
        bad, found = B.count_mismatches(torch, one, period, axis, marks, mrows)
        assert bad == 1 and found[0][:2] == (n, f)
        # a marker row that came out as the base row it replaced
        lost = correct.clone()
        m = marks[len(marks) // 2]
        if axis:
            lost[m] = period[m % case["P"]]
        else:
            lost[:, m] = period[m % case["P"]]
        bad, found = B.count_mismatches(torch, lost, period, axis, marks, mrows)
        assert bad > 0 and all(r[0] == m for r in found)
        for kind in B.MUTANTS:
            got = B.mutate(torch, correct, kind, B.SMALL_BOUNDARY)
            bad, found = B.count_mismatches(torch, got, period, axis, marks, mrows)
            print("big-operands mutant %s a%d %s %s: %d mismatches, first %s" % (kind, axis, dtype, what, bad, found[:1]))
            assert bad > 0 and found and len(found[0]) == 4, (kind, what)
            n, f, g, w = found[0]
            assert 0 <= n < case["N"] and 0 <= f < period.shape[1] and g != w
