"""CPU tier of the weight-gradient containment tests (tests/_updat_containment.py): the table covers the routes of updat_path, every case
meets the conditions that make it a test -- the poisoned lines, gate-0 blocks inside and outside them, partner magnitudes, a minibatch that
is ragged against the route's chunk, the dispatch condition where the trace code is ambiguous -- the class arithmetic is what a float64
walk with the reference's skip gives, both mutant models change the classes, and the oracle's gated weight gradient equals the walk."""
import numpy as np
import pytest

import _updat_containment as U
from oracle import bsmm_oracle as O

IDS = [c["id"] for c in U.CASES]
K = U.L


def _sel(**m):
    return [c for c in U.CASES if all(c[k] == v for k, v in m.items())]


def test_the_table_covers_the_routes():
    assert {c["route"] for c in U.CASES} == set(U.ROUTES)
    assert {(c["bs"], c["axis"], c["dtype"]) for c in _sel(route="valu", variant=1)} == {(b, a, d) for b in (32, 16, 8) for a in (0, 1) for d in ("bf16", "f32")}
    assert len(_sel(route="valu", variant=0, unaligned_dw=True)) == 1 and all(not c["unaligned_dw"] for c in U.CASES if c["variant"] != 0)
    b4 = _sel(route="block4")
    assert all(c["variant"] == 2 for c in b4)
    assert {(c["bs"], c["dtype"] != "f32") for c in b4 if c["axis"] == 0} == {(32, True), (16, True), (32, False), (16, False)}
    assert {c["bs"] for c in b4 if c["dtype"] == "f32"} == {32, 16}
    assert [c for c in b4 if c["bs"] == 32 and c["axis"] == 1 and c["dtype"] != "f32" and c["gate"] and c["N"] * c["pairs"] > U.UTS_NMAX]
    for bs, lim in ((32, U.UAW_NMAX // 2), (16, U.UAW_NMAX)):
        rows = [c["N"] * c["pairs"] for c in _sel(route="wave_a0", bs=bs)]
        assert min(rows) <= lim < max(rows), (bs, rows)
    assert all(U.luts(c["lay"], 8)["blocks"] % 2 == 1 and c["axis"] == 0 for c in _sel(route="pairs8")) and _sel(route="pairs8")
    assert {c["gate"] is not None for c in _sel(route="one_wave_tr")} == {True, False}
    assert all(c["N"] * c["pairs"] <= U.UTS_NMAX and c["kv"] == K.KV_ONE_WAVE for c in _sel(route="one_wave_tr"))
    assert {c["bs"] for c in _sel(route="block_tr")} == {32, 16} and all(c["kv"] == 0 and c["gate"] is None for c in _sel(route="block_tr"))
    assert all(c["N"] > U.UTS_NMAX for c in _sel(route="block_tr", bs=32))
    assert {(c["axis"], c["split"], c["bitwise"]) for c in _sel(route="win16")} == {(a, 1, True) for a in (0, 1)} | {(a, 2, False) for a in (0, 1)}
    assert {(c["split"], c["gate"] is not None) for c in _sel(route="rows16")} == {(1, False), (2, False), (0, True)} and all(c["axis"] == 0 for c in _sel(route="rows16"))
    st = _sel(route="stream")
    assert {(c["axis"], c["split"]) for c in st if c["gate"] is None and c["pairs"] == 1 and c["lay"] == "r48"} >= {(0, 1), (1, 1), (0, 0), (1, 0), (1, 2)}
    assert {c["axis"] for c in st if c["gate"] and c["mode"] == "dw"} == {0, 1} and [c for c in st if c["pairs"] == 3]
    assert {c["gate"] is not None for c in st if c["lay"] == "direct"} == {True, False}
    assert {c["axis"] for c in st if c["mode"] == "sums"} == {0, 1} and all(c["gate"] for c in st if c["mode"] == "sums")
    assert {c["axis"] for c in _sel(route="super8")} == {0, 1} and all(c["gate"] is None and c["code"] == K.K_UPDAT_SUPER8 for c in _sel(route="super8"))
    assert {c["axis"] for c in _sel(route="gated-b8")} == {0, 1} and all(c["gate"] and c["code"] != K.K_UPDAT_SUPER8 and c["variant"] == 3 for c in _sel(route="gated-b8"))
    assert {(c["code"], c["kv"]) for c in _sel(route="b64")} == {(K.K_UPDAT_STREAM, None), (K.K_UPDAT_BLOCK_TR, K.KV_ONE_WAVE)}
    assert all(c["gate"] and c["bs"] == 64 and c["axis"] == 1 for c in _sel(route="b64"))
    assert {c["code"] for c in _sel(route="f32split")} == {K.K_UPDAT_STREAM, K.K_UPDAT16_WIN, K.K_UPDAT16_ROWS}
    assert all(c["gate"] and c["dtype"] == "f32" and not c["bitwise"] and c["pairs"] == 1 for c in _sel(route="f32split"))
    # not bitwise: exactly the split windowed calls (atomics) and the fp32 split routes (repair pass)
    assert {c["id"] for c in U.CASES if not c["bitwise"]} == {c["id"] for c in _sel(route="win16", split=2) + _sel(route="f32split")}
    # every weight-gradient family the library reports (K_UPDAT_WIN: retired, no kernel behind it)
    assert {c["code"] for c in U.CASES} == {K.K_UPDAT_VALU, K.K_UPDAT_BLOCK, K.K_UPDAT_BLOCK_TR, K.K_UPDAT16_WIN, K.K_UPDAT16_ROWS, K.K_UPDAT_STREAM, K.K_UPDAT_SUPER8}
    for m in U.MUTANTS:
        assert len(U.NAMED[m]) >= 3 and all(n in U.BY_ID for n in U.NAMED[m])
    first = [U.BY_ID[n] for n in U.NAMED[U.MUTANTS[0]]]
    assert [c for c in first if c["route"] == "stream"] and [c for c in first if c["route"] == "rows16"] and [c for c in first if c["bs"] == 64]


def test_sizes_and_scalars():
    for c in U.CASES:
        assert c["N"] in U.N_AXIS[c["axis"]] or (c["route"] == "wave_a0" and c["bs"] == 32 and c["N"] == 40), c["id"]     # (below UAW_NMAX / 2 = 64)
        assert c["N"] % c["chunk"] != 0 and (c["axis"] == 1 or c["N"] % 8 == 0), c["id"]
        t = U.luts(c["lay"], c["bs"])
        assert c["pairs"] * c["N"] * (t["CB"] + t["KB"]) * c["bs"] * 4 < (8 << 20), c["id"]
        # beta DW0 must be exact in fp32 ("rounded once"); alpha > 0
        assert c["beta"] == 0.0 or np.log2(abs(c["beta"])) == round(np.log2(abs(c["beta"]))), c["id"]
        assert c["alpha"] > 0
    assert any(c["beta"] < 0 for c in U.CASES)


def test_ambiguous_trace_codes_have_their_dispatch_condition():
    """three routes report K_UPDAT_BLOCK: each of their cases names the one it is there for, and the dispatch rules select it"""
    for c in U.CASES:
        assert (c["code"] == K.K_UPDAT_BLOCK) == (c["cond"] is not None), c["id"]
        if c["cond"] is not None:
            assert U.dispatch_kind(c) == c["cond"], (c["id"], U.dispatch_kind(c))
    assert {c["cond"] for c in U.CASES} == {None, "block4", "wave_a0", "pairs8"}
    assert all(c["cond"] == c["route"] or c["id"].endswith("past") for c in U.CASES if c["cond"])


def test_direct_block_cases_poison_direct_blocks():
    """the "direct" layout: the streaming plan has direct blocks (csrc/bsmm_plan.h, header words 28 / 29), the Inf's block row and block
    column each hold some, and in the gated case the row has one that is gated off and one that is live, the column live ones"""
    from blocksparse_amd import matmul as M
    cases = _sel(route="stream", lay="direct")
    assert len(cases) == 2
    for c in cases:
        t, s = U.luts("direct", 32), U.setup(c["id"])
        words = np.asarray(M._host_updat_plan(t["updat_lut"], t["blocks"], t["CB"], t["KB"], 32, K.BF16, 1, 0))
        n, off = int(words[28]), int(words[29])
        direct = words[off:off + 4 * n].reshape(n, 4)
        assert n > 0 and all(tuple(t["updat_list"][w]) == (ci, ki) for w, ci, ki, _ in direct)
        in_row, in_col = [int(w) for w, ci, ki, _ in direct if ci == s["c1"]], [int(w) for w, ci, ki, _ in direct if ki == s["k1"]]
        assert len(in_row) >= 2 and len(in_col) >= 2, (in_row, in_col)
        if c["gate"]:
            g = s["gate"]
            assert any(g[w] == 0 for w in in_row) and any(g[w] != 0 for w in in_row) and any(g[w] != 0 for w in in_col), (g[in_row], g[in_col])


@pytest.mark.parametrize("cid", IDS)
def test_case_conditions_and_classes(cid):
    c = U.BY_ID[cid]
    s, r = U.setup(cid), U.reference(cid)
    t, bs, N = U.luts(c["lay"], c["bs"]), c["bs"], c["N"]
    lay = U.LAYOUTS[c["lay"]] != 0
    ul = t["updat_list"]
    # the poisoned lines
    assert lay[s["c1"]].sum() >= 2 and lay[:, s["k1"]].sum() >= 2 and s["c1"] != s["c2"] and s["k1"] != s["k2"]
    assert lay[s["c2"]].any() and lay[:, s["k2"]].any()
    if bs == 8:
        assert any(lay[q].any() for q in U.CT.partners(s["c1"], 8, lay.shape[0])) and any(lay[:, q].any() for q in U.CT.partners(s["k1"], 8, lay.shape[1]))
        assert s["c1"] // 4 != s["c2"] // 4 and s["k1"] // 4 != s["k2"] // 4
    assert s["pn"] == (2 if c["pairs"] >= 3 else c["pairs"] - 1) and len(r["Xs"]) == c["pairs"]
    g = s["gate"]
    if c["gate"] is not None:
        assert ul[s["off_x"]][0] == s["c1"] and ul[s["on_x"]][0] == s["c1"] and g[s["off_x"]] == 0 and g[s["on_x"]] != 0
        assert ul[s["off_dy"]][1] == s["k1"] and ul[s["on_dy"]][1] == s["k1"] and g[s["off_dy"]] == 0 and g[s["on_dy"]] != 0
        ci, ki = ul[s["off_out"]]
        assert g[s["off_out"]] == 0 and ci not in (s["c1"], s["c2"]) and ki not in (s["k1"], s["k2"])
        kinds = set(np.unique(g))
        assert kinds == {0.0, 1.0} if c["gate"] == "binary" else len(kinds - {0.0, 1.0}) >= 2
    else:
        assert g is None
    # partner magnitudes at the two poisoned minibatch indices; DW0 ordinary and finite
    assert all(a.shape == U.act_shape(c, t["CB"]) for a in r["Xs"]) and all(a.shape == U.act_shape(c, t["KB"]) for a in r["Es"])
    for a in r["Xs"] + r["Es"]:
        assert np.isfinite(a).all()
        for n in (0, N - 1):
            assert (np.abs(U.at(c, a, n)) >= U.PARTNER_MIN).all()
    if c["beta"] != 0.0:
        assert np.isfinite(r["DW0"]).all() and (r["DW0"] != 0).mean() > 0.9
        assert np.array_equal(r["off_values"], O.round_to(c["beta"] * r["DW0"].astype(np.float64), c["dtype"]))
    else:
        assert r["DW0"] is None and not r["off_values"].any() and not np.signbit(r["off_values"]).any()
    assert np.isfinite(r["want64"]).all()
    off = np.zeros(t["blocks"], dtype=bool) if g is None else g == 0
    for side in ("x", "dy"):
        p = r[side]
        assert sum(int((~np.isfinite(a)).sum()) for a in p["Xs"] + p["Es"]) == 2
        bad = p["Xs"] if side == "x" else p["Es"]
        assert np.isposinf(U.at(c, bad[0], N - 1)).sum() == 1 and np.isnan(U.at(c, bad[s["pn"]], 0)).sum() == 1
        cls = p["cls"]
        # the classes are what the float64 walk with the skip leaves; the rest of the walk is the clean walk
        got = U.walk(c, p["Xs"], p["Es"], g, r["DW0"])
        assert np.array_equal(U.classes(got), cls)
        fin = cls == U.FIN
        assert np.array_equal(got[fin], r["want64"][fin])
        # something of every class the case can show, and finite elements in every poisoned block
        assert (cls == U.NAN).any() and ((cls == U.PINF) | (cls == U.NINF)).any() and not cls[off].any()
        assert all(fin[w].any() for w in range(t["blocks"]))
        if c["gate"] == "general" or c["route"] in ("stream", "block4") and c["gate"] is None:
            assert (cls == U.PINF).any() and (cls == U.NINF).any()          # (both signs: the partner's and, with a general gate, the gate's)
        # gate-0 blocks of the walk: beta DW0 exactly
        if off.any():
            assert np.array_equal(got[off], c["beta"] * r["DW0"][off].astype(np.float64) if c["beta"] else np.zeros_like(got[off]))


@pytest.mark.parametrize("cid", IDS)
def test_both_mutants_change_the_classes(cid):
    c, r = U.BY_ID[cid], U.reference(cid)
    for side in ("x", "dy"):
        good = r[side]["cls"]
        if c["gate"] is not None:
            bad = U.expected_classes(c, side, r["Xs"], r["Es"], U.MUTANTS[0])
            assert ((bad != U.FIN) & (good == U.FIN)).any() and np.array_equal(bad[good != U.FIN], good[good != U.FIN])
        bad = U.expected_classes(c, side, r["Xs"], r["Es"], U.MUTANTS[1])          # (N is ragged against the chunk in every case)
        assert np.array_equal(bad != U.FIN, good != U.FIN) and ((bad == U.NAN) & (good != U.NAN)).any()


@pytest.mark.parametrize("mutant", U.MUTANTS)
def test_mutants_on_their_named_cases(mutant):
    """gate as a multiplier: NaN in the gate-0 block of the Inf's line (0 Inf) and nowhere outside the poisoned lines -- on the streaming
    kernel's summing pass, the row-owner kernel's finalize pass, the quadrants of a 64 x 64 block, the bsize-8 pair kernel and a repair pass.
    One-sided tail: every +-Inf of the expectation turns NaN where the last chunk is partial -- on the partial-sum and the directly stored
    form of the streaming kernel, the windowed kernel and the super-block path."""
    for cid in U.NAMED[mutant]:
        c, s, r = U.BY_ID[cid], U.setup(cid), U.reference(cid)
        for side in ("x", "dy"):
            good, bad = r[side]["cls"], U.expected_classes(c, side, r["Xs"], r["Es"], mutant)
            if mutant == U.MUTANTS[0]:
                w = s["off_x"] if side == "x" else s["off_dy"]
                line = bad[w][U.I1, :] if side == "x" else bad[w][:, U.I1]
                assert (line == U.NAN).all() and not good[w].any() and not bad[s["off_out"]].any()
            else:
                inf = (good == U.PINF) | (good == U.NINF)
                assert inf.any() and (bad[inf] == U.NAN).all() and c["N"] % c["chunk"] != 0


@pytest.mark.parametrize("cid", [U.NAMED[U.MUTANTS[0]][i] for i in (0, 1, 2)] + ["stream-r48-b32-a1-bf16-N75-p3", "valu-r12x10-b8-a1-bf16-N40-p1-general"])
def test_oracle_skips_gate_zero_blocks(cid):
    """oracle.updat(gate=...) is the walk: a gate-0 block holds beta DW0 (or 0) whatever its operands hold"""
    c, r = U.BY_ID[cid], U.reference(cid)
    t = U.luts(c["lay"], c["bs"])
    for side in ("x", "dy"):
        p = r[side]
        with np.errstate(invalid="ignore", over="ignore"):
            got = O.updat(t, p["Xs"], p["Es"], c["axis"], alpha=c["alpha"], beta=c["beta"], dw_in=r["DW0"], gate=r["gate"])
        want = U.walk(c, p["Xs"], p["Es"], r["gate"], r["DW0"])
        assert np.array_equal(U.classes(got), p["cls"])
        fin = p["cls"] == U.FIN
        assert np.allclose(got[fin], want[fin], rtol=1e-12, atol=1e-300)
        if r["gate"] is not None:
            off = r["gate"] == 0
            assert np.array_equal(got[off], c["beta"] * r["DW0"][off].astype(np.float64) if c["beta"] else np.zeros_like(got[off]))
