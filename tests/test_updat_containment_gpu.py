"""GPU tier of the weight-gradient containment tests: an Inf / NaN in one element of X or DY reaches exactly the elements of DW that its
feature feeds, in the blocks that are not gated off, with the class a float64 walk gives; a block whose gate is 0 holds +0 (beta == 0) or
beta DW0, whatever X and DY hold -- on every route of updat_path (tests/_updat_containment.py: the table, the poison, the expected classes;
tests/test_updat_containment_host.py: their conditions).  Per case five calls on the kernel the case names (bsmm_args.trace) -- clean,
poisoned X, clean, poisoned DY, clean -- and then
  (a) isnan / isposinf / isneginf of DW == the expectation, element for element;
  (b) on finite elements a poisoned call is the clean call bit for bit -- except where fp32 atomics or a repair pass stand between
      (`bitwise` False): there every finite element meets statement (1) of _parity.block_report against the float64 walk (fp32, which has
      no statement (1): the tensor bar);
  (c) the gate-0 blocks exactly: +0 with beta == 0 (DW0 then holds NaN: it must not be read), else beta DW0 rounded once;
  (d) the clean call passes _parity.assert_blocks;
  (e) the clean call after each poisoned call is the first clean call bit for bit: no flag or workspace state stays behind.
The data-parallel finalize (csrc/bsmm_dist.hip) follows the same gate rule and is not run here."""
import numpy as np
import pytest

import _parity as P
import _updat_containment as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import BlocksparseMatMul, _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()     # fail loudly if the HIP extension is missing
    return torch, BlocksparseMatMul, _lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("cid", [c["id"] for c in U.CASES])
def test_nonfinite_activations_and_gate_zero_blocks_in_the_weight_gradient(env, cid):
    torch, BSMM, lib = env
    c, r = U.BY_ID[cid], U.reference(cid)
    dtype, bs = c["dtype"], c["bs"]
    td = getattr(torch, P.TORCH_DT[dtype])
    opts = 0
    for o in c["opts"]:
        opts |= getattr(lib, o)
    b = BSMM(np.array(U.LAYOUTS[c["lay"]]), block_size=bs, feature_axis=c["axis"], plan_options=opts, updat_split=c["split"])
    blocks = U.luts(c["lay"], bs)["blocks"]
    assert b.w_shape == (blocks, bs, bs)
    if c["code"] == lib.K_UPDAT_BLOCK_TR and bs == 64 or c["cond"] is not None and c["variant"] == 0:
        assert torch.cuda.get_device_properties(0).multi_processor_count == U.CUS      # (what the production-dispatch cases are sized for)
    gate = torch.from_numpy(np.array(r["gate"])).cuda() if r["gate"] is not None else None
    dev = lambda acts: [P.to_dev(np.array(a), dtype, torch) for a in acts]         # (copies: the shared reference arrays are read-only)
    operands = {"clean": (dev(r["Xs"]), dev(r["Es"])), "x": (dev(r["x"]["Xs"]), dev(r["x"]["Es"])), "dy": (dev(r["dy"]["Xs"]), dev(r["dy"]["Es"]))}
    n_el = blocks * bs * bs

    def fresh_dw():
        """DW0 (beta != 0), else NaN in every element: a call with beta == 0 must not read it"""
        buf = torch.empty(n_el + 8, dtype=td, device="cuda")
        v = buf[1:1 + n_el] if c["unaligned_dw"] else buf[:n_el]
        v = v.view(b.w_shape)
        if c["beta"] != 0.0:
            v.copy_(P.to_dev(np.array(r["DW0"]), dtype, torch))
        else:
            v.fill_(float("nan"))
        assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == c["unaligned_dw"]
        return v

    ran = []

    def call(which):
        xs, es = operands[which]
        dw = fresh_dw()
        if c["mode"] == "sums":
            sums = b.updat(xs, es, sums_only=True)
            ran.append((lib.last_kernel(), lib.last_kernel_variant()))
            out = b.updat_finalize(sums, alpha=c["alpha"], beta=c["beta"], dw=dw, gate=gate)
        else:
            out = b.updat(xs, es, alpha=c["alpha"], beta=c["beta"], dw=dw, gate=gate)
            ran.append((lib.last_kernel(), lib.last_kernel_variant()))
        assert out.data_ptr() == dw.data_ptr()
        return P.to_host(out)

    lib.set_kernel_variant(c["variant"])
    try:
        got = {k: call(w) for k, w in (("clean", "clean"), ("x", "x"), ("clean-after-x", "clean"), ("dy", "dy"), ("clean-after-dy", "clean"))}
    finally:
        lib.set_kernel_variant(0)
    print("%s: trace %s (expected %s / %s)" % (cid, ran, c["code"], c["kv"]))
    for k, kv in ran:
        assert k == c["code"] and (c["kv"] is None or kv == c["kv"]), (cid, ran, c["code"], c["kv"])
    want64 = r["want64"]
    off = np.zeros(blocks, dtype=bool) if r["gate"] is None else np.asarray(r["gate"]) == 0
    clean = got["clean"]
    for side in ("x", "dy"):
        dirty, cls = got[side], r[side]["cls"]
        have = U.classes(dirty)
        wrong = np.argwhere(have != cls)
        print("%s poison in %s: non-finite %d (expected %d), wrong class %d, of them in gate-0 blocks %d" %
              (cid, side, (have != U.FIN).sum(), (cls != U.FIN).sum(), len(wrong), int((have != cls)[off].sum())))
        # (a)
        assert len(wrong) == 0, (cid, side, "elements [block, i, j] whose class (0 finite, 1 +Inf, 2 -Inf, 3 NaN) is not the expected one",
                                 [(w.tolist(), int(have[tuple(w)]), int(cls[tuple(w)])) for w in wrong[:8]], len(wrong))
        # (b)
        fin = cls == U.FIN
        if c["bitwise"]:
            differ = int((_bits(dirty)[fin] != _bits(clean)[fin]).sum())
            print("    finite elements whose bits differ from the clean call's: %d" % differ)
            assert differ == 0, (cid, side, differ)
        else:
            filled = np.where(fin, dirty, P.round_to_storage(want64, dtype))
            rep = P.block_report(filled, want64, dtype, blocks)
            print("    finite elements against the float64 walk: %s" % rep)
            assert rep["finite"] and rep["elem_bad"] == 0, (cid, side, rep)
            if dtype == "f32":
                assert rep["tensor_l2"] <= P.L2_BAR[dtype], (cid, side, rep)
        # (e)
        again = got["clean-after-" + side]
        assert int((_bits(again) != _bits(clean)).sum()) == 0, (cid, side, "the clean call after the poisoned one differs from the first")
    # (c)
    for k, a in got.items():
        bad = int((_bits(a)[off] != _bits(r["off_values"])[off]).sum())
        assert bad == 0, (cid, k, "elements of gate-0 blocks that are not %s" % ("+0" if c["beta"] == 0.0 else "beta DW0"), bad)
    # (d)
    P.assert_blocks(clean, want64, dtype, blocks, ctx=(cid, "clean"))
