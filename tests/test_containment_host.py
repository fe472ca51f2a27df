"""CPU tier of the containment tests (tests/_containment.py): every case of the table meets the conditions that make it a test -- the poison
reaches something, its row or column also holds finite outputs, the absent-partner block and (gated) the gate-0-only block exist -- the
expected mask is what a float64 walk with the reference's skip leaves non-finite, and every mutant model changes the mask."""
import numpy as np
import pytest

import _containment as C

IDS = [c["id"] for c in C.CASES]


def test_the_table_covers_the_routes():
    routes = {c["route"] for c in C.CASES}
    assert routes == {"valu", "segment", "small", "mid", "staged", "flow", "list16", "pair16", "f32split", "super8", "b64", "gated-segment",
                      "gated-staged", "gated-images", "gated-f32", "gated-b8"}
    sel = lambda **m: [c for c in C.CASES if all(c[k] == v for k, v in m.items())]
    assert {(c["bs"], c["axis"], c["dtype"]) for c in sel(route="valu", unaligned=False)} == {(b, a, d) for b in (32, 16, 8) for a in (0, 1) for d in ("bf16", "f32")}
    assert len(sel(route="valu", unaligned=True, variant=0)) == 1
    assert {(c["bs"], c["N"]) for c in sel(route="segment", segmented=False)} == {(32, 40), (32, 2056), (16, 40), (16, 520), (16, 2056)}
    for bs, N in ((32, 40), (32, 2056), (16, 40), (16, 520), (16, 2056)):
        assert {(c["axis"], c["dtype"]) for c in sel(route="segment", segmented=False, bs=bs, N=N)} == {(a, d) for a in (0, 1) for d in ("bf16", "f16", "f32")}
    assert {c["dtype"] for c in sel(route="segment", segmented=True)} == {"bf16", "f32"}
    assert {(c["bs"], c["axis"], c["N"], c["passes"]) for c in sel(route="small")} == \
        {(b, 1, 40, ("fprop", "bprop")) for b in (32, 16, 8)} | {(b, 1, 70, ("fprop", "bprop")) for b in (32, 8)} | {(16, 1, 70, ("fprop",))} | \
        {(b, 0, 72, ("fprop", "bprop")) for b in (32, 16, 8)}
    for c in sel(route="mid"):                                    # the two workgroup shapes of launch_xmid
        assert (c["N"] * 48 * 32 * 2 <= (5 << 20)) == (c["N"] == 130)
    assert {c["N"] for c in sel(route="mid")} == {130, 1736}
    assert {(c["axis"], c["flow"]) for c in sel(route="staged")} == {(0, True), (1, False)}
    # flow: units of 128 rows >= / < the compute units (launch_xflow), 16 output blocks per group
    for c in sel(route="flow"):
        for which in c["passes"]:
            units128 = -(-c["N"] // 128) * -(-C.feat_blocks(c, which)[1] // 16)
            assert (units128 >= C.FLOW_RT4_CUS) == (c["kv"][which] == 0), (c["id"], which, units128)
    assert {kv for c in sel(route="flow") for kv in c["kv"].values()} == {0, C.L.KV_FLOW_HALF_UNITS}
    dens = lambda c: (C.LAYOUTS[c["lay"]] != 0).mean()
    assert all(dens(c) >= 0.4 for c in sel(route="pair16")) and all(dens(c) < 0.4 for c in sel(route="list16"))      # x7_use_list
    assert {c["axis"] for c in sel(route="list16")} == {0, 1}
    # fp32 split on feature axis 1: one group per XCD at a time when segments % 8 == 0 and ntiles >= 4 (launch_xcol32s), 16 output blocks per group
    xcd = {(-(-C.feat_blocks(c, w)[1] // 16) % 8 == 0 and -(-c["N"] // 128) >= 4) for c in sel(route="f32split", axis=1) for w in c["passes"]}
    assert xcd == {True, False} and len(sel(route="f32split", axis=0)) == 1
    assert {(c["axis"], c["dtype"]) for c in sel(route="super8")} == {(0, "f16"), (1, "f16")}
    assert {(c["bs"], c["axis"], c["dtype"], c["gate"]) for c in sel(route="gated-segment")} == \
        {(b, a, d, g) for b in (32, 16) for a in (0, 1) for d in ("bf16", "f16") for g in ("binary", "general")}
    assert {(c["bs"], c["axis"], c["dtype"], c["gate"]) for c in sel(route="gated-images", variant=3)} == \
        {(b, a, d, g) for b in (32, 16) for a in (0, 1) for d, g in (("bf16", "binary"), ("bf16", "general"), ("f16", "general"))}
    assert all(c["N"] >= C.IMAGES_MIN_N[c["bs"]] and c["images"] and not c["bitwise"] for c in sel(route="gated-images"))
    assert all(c["N"] < 1024 and c["gate"] for c in C.CASES if c["route"].startswith("gated-") and not c["images"])
    for names in C.NAMED.values():
        assert all(n in C.BY_ID for n in names)
    # every xprop kernel family the library reports is asked for by some case (the GPU tier asserts each case's code)
    K = C.L
    assert {c["code"] for c in C.CASES if not c["code_from_ungated"]} == {K.K_XPROP_VALU, K.K_XPROP_SEGMENT, K.K_XPROP_SMALL, K.K_XPROP_MID, K.K_XCOL32_STAGED,
                                                                          K.K_XCOL32_FLOW, K.K_XCOL16_STAGED, K.K_XCOL32_F32SPLIT, K.K_XPROP_SUPER8}


def test_layouts_have_what_their_routes_need():
    t = C.luts("locks24x12", 32)
    assert t["fprop_locks"] > 0 and t["bprop_locks"] > 0
    lay = C.LAYOUTS["small24"] != 0
    for counts in (lay.sum(axis=0), lay.sum(axis=1)):       # entry lists of fprop (per output block k) and of bprop (per c)
        assert any(n % 2 == 1 for n in counts) and any(n % 2 == 0 and n > 0 for n in counts) and counts.max() > 16      # > XS0_NW = 16 >= XSM_NW waves
    for c in C.CASES:
        lay = C.LAYOUTS[c["lay"]]
        assert 12 <= lay.shape[0] <= 64 and 10 <= lay.shape[1] <= 128 or c["lay"] == "r10x12"


@pytest.mark.parametrize("cid", IDS)
def test_case_conditions_and_mask(cid):
    c = C.BY_ID[cid]
    s, r = C.setup(cid), C.reference(cid)
    for which in c["passes"]:
        p, lay, ok = s[which], C.pass_layout(c, which), C.live(c, which)
        n_in, n_out = lay.shape
        m = r[which]["mask"]
        rows = m if c["axis"] else m.T                                      # [minibatch index][output feature]
        assert m.any() and m.shape == C.act_shape(c, n_out)
        assert rows[c["N"] - 1].any() and not rows[c["N"] - 1].all() and rows[0].any() and not rows[0].all()
        assert not rows[1:c["N"] - 1].any()
        # the absent-partner block: c1's partner feeds k_absent, c1 does not
        assert not lay[p["c1"], p["k_absent"]] and any(lay[q, p["k_absent"]] for q in C.partners(p["c1"], c["bs"], n_in))
        if c["bs"] == 8:
            assert all(q // 4 == p["c1"] // 4 for q in C.partners(p["c1"], 8, n_in))
        assert not rows[c["N"] - 1, p["k_absent"] * c["bs"]]
        if c["gate"] is not None:
            # connected to c1 through a gate-0 entry only (a (c, k) pair has one entry): finite; the gate-0 blocks hold NaN weights
            assert lay[p["c1"], p["k_g0"]] and not ok[p["c1"], p["k_g0"]] and not rows[c["N"] - 1, p["k_g0"] * c["bs"]]
            assert ok[p["c1"], p["k_live"]] and rows[c["N"] - 1, p["k_live"] * c["bs"]]
            assert (s["gate"] == 0).any() and np.isnan(r["W"][s["gate"] == 0]).all() and np.isfinite(r["W"][s["gate"] != 0]).all()
            kinds = set(np.unique(s["gate"]))
            assert kinds == {0.0, 1.0} if c["gate"] == "binary" else len(kinds - {0.0, 1.0}) >= 2
        # the mask is what a float64 walk with the reference's skip leaves non-finite; the clean walk is finite
        bad = r[which]["poisoned"]
        assert (~np.isfinite(bad)).sum() == 2 and np.isfinite(r[which]["clean"]).all() and np.isfinite(r[which]["want64"]).all()
        assert np.array_equal(~np.isfinite(C.walk(c, which, bad, r["W"], r["gate"])), m)


@pytest.mark.parametrize("cid", IDS)
def test_every_mutant_changes_the_mask(cid):
    c = C.BY_ID[cid]
    for mutant in C.MUTANTS:
        if mutant == C.MUTANTS[1] and c["gate"] is None:
            continue
        for which in c["passes"]:
            if mutant == C.MUTANTS[3] and 0 not in (C.setup(cid)[which]["c1"], C.setup(cid)[which]["c2"]):
                continue
            good, bad = C.expected_mask(c, which), C.expected_mask(c, which, mutant)
            assert (bad & ~good).any() and not (good & ~bad).any(), (mutant, which)


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_mutants_on_their_named_cases(mutant):
    """the shapes each mutant is about: a zero weight fragment against an absent partner (bsize-16 pair kernel, bsize 8 inside a super-block,
    bsize-32 pair step); the gate as a multiplier (one weight image, two images, in-kernel gate); a leak into row N - 2 where N - 1 is the
    row that the rows past N are clamped onto; the odd tail of a K-concatenated entry list read from block 0 (kernels that take two entries per
    matrix-core step: bsize 16 / 8 small-minibatch, bsize-16 per-segment)."""
    for cid in C.NAMED[mutant]:
        c = C.BY_ID[cid]
        for which in c["passes"]:
            p = C.setup(cid)[which]
            good, bad = C.expected_mask(c, which), C.expected_mask(c, which, mutant)
            rows_g, rows_b = (good, bad) if c["axis"] else (good.T, bad.T)
            if mutant == C.MUTANTS[0]:
                k = p["k_absent"] * c["bs"]
                assert rows_b[c["N"] - 1, k] and not rows_g[c["N"] - 1, k]
            elif mutant == C.MUTANTS[1]:
                k = p["k_g0"] * c["bs"]
                assert rows_b[c["N"] - 1, k] and not rows_g[c["N"] - 1, k]
            elif mutant == C.MUTANTS[2]:
                assert rows_b[c["N"] - 2].any() and not rows_g[c["N"] - 2].any() and c["N"] % 32 != 0
            else:
                lay = C.pass_layout(c, which)
                odd = [k for k in range(lay.shape[1]) if lay[:, k].sum() % 2 == 1 and not lay[0, k]]
                assert p["c1"] == 0 and odd and all(rows_b[c["N"] - 1, k * c["bs"]] and not rows_g[c["N"] - 1, k * c["bs"]] for k in odd)
