"""Every fp32 route that multiplies bf16 pieces, on inputs that HAVE three pieces (tests/_f32_pieces.py; the CPU tier,
test_f32_pieces_host.py, shows that the suite's usual fp32 inputs have none and that these inputs can tell a wrong pair from noise):

  xprop  K_XCOL32_F32SPLIT: feature axis 1 with the split fused into the kernel, feature axis 0 with the pre-split pass (both through the C ABI
         with prepared_w = NULL: the library splits W too), feature axis 1 with the pieces of bsmm_prepare_weights (the product API);
  updat  the four routes of bsmm_updat_dispatch.h::f32_split_route -- K_UPDAT_STREAM (bsize 32), K_UPDAT_SUPER8 (bsize 8, both axes),
         K_UPDAT16_WIN (bsize 16, axis 1), K_UPDAT16_ROWS (bsize 16, axis 0).

Three kinds of check, every one with the plan forced (set_kernel_variant(3)) and the kernel family asserted:
  selector   one operand is zero but for one entry per output element (+-2^s: first order, +-2^s (1 + 2^-9): second order), so every output is
             ONE product whose piece products sum exactly in any order: bit for bit against the float64 oracle, +0 where nothing is selected;
  tight      random full-significand operands, every output group (weight block of DW, feature block of Y / DX) under the bar between the
             fp32 noise model and the best-hidden single-pair mutant (F.tight_bar, computed here from the emulation, never from the kernel);
  yardstick  longer reductions, and the (route, N) where that bar does not exist (F.NO_TIGHT_BAR): the tensor's error at most twice that of
             the per-block fp32 kernels on the same inputs (set_kernel_variant(2)) + 1e-8, and the tensor and every group under the fp32 bar;
  alpha-beta-gate   alpha 0.5, beta 0.25, gates in [0, 2) with a planted 0 and 1, DW0 at the product's own rms: the `tight` criterion on what
             the call stores (bsize 8: the route takes no gate and has no tight bar -- alpha / beta under the `yardstick` rule)."""
import ctypes

import numpy as np
import pytest

import _f32_pieces as F
import _parity as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import BlocksparseMatMul, _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()
    return torch, BlocksparseMatMul, _lib


_OPS = {}


def _operator(BSMM, case):
    key = (case["layout"], case["bs"], case["axis"])
    if key not in _OPS:
        _OPS[key] = BSMM(F.LAYOUTS[case["layout"]], block_size=case["bs"], feature_axis=case["axis"])
    return _OPS[key]


def _abi_xprop(torch, lib, b, op, acts, w):
    """bsmm_fprop / bsmm_bprop with prepared_w = NULL, as test_gpu_parity.py::test_prepared_weights_cache_fp32 makes the call."""
    L = lib.load()
    tabs = b._tables_on(acts.device)
    if op == "fprop":
        N = acts.numel() // b.C
        a = b._args(tabs.fprop, b._dev_tables["fprop"], N, b.C, b.K, acts.dtype, plan=tabs.fprop_plan_f32)
        code, fn, feat = lib.OP_FPROP, L.bsmm_fprop, b.K
    else:
        N = acts.numel() // b.K
        a = b._args(tabs.bprop, b._dev_tables["bprop"], N, b.K, b.C, acts.dtype, plan=tabs.bprop_plan_f32)
        code, fn, feat = lib.OP_BPROP, L.bsmm_bprop, b.C
    ws = torch.empty(max(int(L.bsmm_workspace_bytes(code, ctypes.byref(a))), 16), dtype=torch.uint8, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    out = torch.empty(b._out_shape(acts, feat), dtype=acts.dtype, device="cuda")
    assert fn(acts.data_ptr(), w.data_ptr(), out.data_ptr(), ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    return out


def _run(env, case, inp, variant, scaled=False):
    """(result on the host, trace code) of the case's call under a kernel variant; `scaled`: with the case's alpha / beta / gate / DW0."""
    torch, BSMM, lib = env
    b = _operator(BSMM, case)
    w, x, e = (torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in ("W", "X", "E"))
    op = case["op"]
    lib.set_kernel_variant(variant)
    try:
        if op == "updat":
            if scaled:
                gate = None if inp["gate"] is None else torch.from_numpy(inp["gate"]).cuda()
                out = b.updat(x, e, alpha=F.ALPHA, beta=F.BETA, dw=torch.from_numpy(inp["dw0"].copy()).cuda(), gate=gate)
            else:
                out = b.updat(x, e)
        elif case["how"] == "abi" and variant == 3:
            out = _abi_xprop(torch, lib, b, op, x if op == "fprop" else e, w)
        else:
            b.invalidate_weights()
            out = b.fprop(x, w) if op == "fprop" else b.bprop(e, w)
            if variant == 3:
                assert (lib.OP_FPROP if op == "fprop" else lib.OP_BPROP) in b._prepared_w      # the call ran on prepared pieces
        torch.cuda.synchronize()
        kernel = lib.last_kernel()
    finally:
        lib.set_kernel_variant(0)
    return P.to_host(out), kernel


def _forced(env, case, inp, scaled=False):
    got, kernel = _run(env, case, inp, 3, scaled)
    assert kernel == getattr(env[2], case["kernel"]), (case["id"], "ran kernel family", kernel)
    assert np.isfinite(got).all(), case["id"]
    return got


def _stored(case, inp):
    """The float64 oracle of what the call stores."""
    prod = F.raw_product(case, inp)
    if not case["kind"].startswith("alpha-beta"):
        return prod
    epi, _ = F.epilogue_of(case, inp)
    return np.stack([epi(g, prod[g]) for g in range(len(prod))])


def _selector_diagnosis(case, inp, got, want):
    """Where a selector result differs: how many elements, how many of them where nothing is selected, the mutant pair list that explains
    most of the live ones, and the share whose first piece lies in a higher binade than the element itself."""
    part, full, live = F.selector_elements(case, inp)
    bad = got.view(np.uint32) != want.view(np.uint32)
    rep = {"mismatches": int(bad.sum()), "of": int(bad.size), "where nothing is selected": int((bad & ~live).sum())}
    sel = bad & live
    if sel.any():
        first, second = (part, full) if case["role"] in ("partner-in-X", "partner-in-W") else (full, part)
        xs, es = F.split3(first[sel]), F.split3(second[sel])
        match = {name: float((F.six_pair_product(xs, es, pairs).astype(np.float32) == got[sel]).mean()) for name, pairs in F.mutants().items()}
        best = max(match, key=match.get)
        rep["best mutant"] = (best, match[best])
        p1 = F.split3(full[sel])[0]
        rep["first piece in a higher binade"] = float((np.frexp(p1)[1] > np.frexp(full[sel])[1]).mean())
        i = tuple(np.argwhere(sel)[0])
        rep["first"] = (i, float(got[i]), float(want[i]))
    return rep


def _nearest_pair_list(groups, g, got_g, epi):
    """Which pair list explains a group best: (name, L2 distance of the device result from its emulation, relative to the oracle's norm),
    over the true list and every mutant."""
    A, B = groups[g]
    xs, es = F.split3(A), F.split3(B)
    want = epi(g, A.astype(np.float64) @ B.astype(np.float64))
    lists = dict(F.mutants(), **{"the six pairs": F.PAIRS})
    dist = {name: F._rel(np.asarray(got_g, dtype=np.float64) - epi(g, F.six_pair_product(xs, es, pairs, np.matmul)), want) for name, pairs in lists.items()}
    best = min(dist, key=dist.get)
    return best, dist[best]


def _worst(errs):
    g = int(np.argmax(errs))
    return g, float(errs[g])


@pytest.mark.parametrize("case", F.CASES, ids=[c["id"] for c in F.CASES])
def test_piece_pairs(env, case):
    inp = F.make_inputs(case)
    assert inp["redraw"] <= F.REDRAW_CAP
    want = _stored(case, inp)
    kind = case["kind"]
    if kind == "selector":
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), want)                   # the oracle itself is exact in fp32
        got = _forced(env, case, inp)
        same = got.view(np.uint32) == want32.view(np.uint32)                     # bit for bit: also +0 (not -0) where nothing is selected
        print("f32-pieces %s mismatches %d of %d" % (case["id"], int((~same).sum()), same.size))
        assert same.all(), (case["id"], _selector_diagnosis(case, inp, got, want32))
        return
    got = _forced(env, case, inp, scaled=kind.startswith("alpha-beta"))
    errs = F.group_errors(case, got, want)
    dead = np.array([not np.any(w) for w in F.group_outputs(case, want)])
    assert not errs[dead].any(), (case["id"], "groups with no block are not zero", np.nonzero(dead & (errs > 0))[0])
    g, worst = _worst(np.where(dead, 0.0, errs))
    if kind == "tight" or kind == "alpha-beta-gate":
        groups = F.groups_of(case, inp)
        epi, live = F.epilogue_of(case, inp) if kind != "tight" else (F._identity, [A.shape[1] > 0 for A, _ in groups])
        bar = F.tight_bar(groups, epi, live)
        print("f32-pieces %s worst group %d err %.3e noise %.3e mutant %.3e bar %.3e" % (case["id"], g, worst, bar["noise"], bar["mutant"], bar["bar"]))
        assert bar["valid"], (case["id"], bar)
        assert worst <= bar["bar"], (case["id"], "worst group", g, "error", worst, bar,
                                     "nearest pair list", _nearest_pair_list(groups, g, F.group_outputs(case, got)[g], epi))
        return
    # the yardstick rule
    got2, _ = _run(env, case, inp, 2, scaled=kind.startswith("alpha-beta"))
    l2, l2b = P.errors(got, want)[0], P.errors(got2, want)[0]
    print("f32-pieces %s worst group %d err %.3e tensor %.3e per-block fp32 kernels %.3e" % (case["id"], g, worst, l2, l2b))
    assert l2 <= 2 * l2b + 1e-8, (case["id"], "tensor", l2, "per-block fp32 kernels", l2b)
    assert l2 <= P.L2_BAR["f32"], (case["id"], "tensor", l2)
    assert worst <= P.L2_BAR["f32"], (case["id"], "worst group", g, "error", worst)
