"""GPU tier of the containment tests: an Inf / NaN in one element of an activation block reaches exactly the outputs that block is connected
to through a live entry, in its own minibatch row or column -- on every fprop / bprop route of the library (tests/_containment.py: the
table, the poison, the expected masks; tests/test_containment_host.py: their conditions).  Per case four calls -- clean and poisoned
fprop, clean and poisoned bprop -- on the kernel family the case names (bsmm_args.trace), and then
  (a) ~isfinite(output) == the expected mask, element for element (Inf against NaN is not compared: the bf16 piece split turns one into the
      other by design);
  (b) on finite elements the poisoned call is the clean call bit for bit -- except where fp32 lock accumulators (atomic order) or a repair
      pass (another kernel rewrites the output when its flag is set) stand between: there every finite element meets statement (1) of
      _parity.block_report against the float64 walk of the clean inputs (fp32, which has no statement (1): the tensor bar);
  (c) the clean call passes _parity.assert_blocks.
test_inf_in_an_unconnected_feature_does_not_reach_the_output (tests/test_gpu_parity.py) poisons whole feature blocks in bf16 on the forced plan
kernels; this file has the single elements, the other types, routes and the gates."""
import numpy as np
import pytest

import _containment as C
import _parity as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import BlocksparseMatMul, _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()     # fail loudly if the HIP extension is missing
    return torch, BlocksparseMatMul, _lib


def _operator(BSMM, c):
    b = BSMM(np.array(C.LAYOUTS[c["lay"]]), block_size=c["bs"], feature_axis=c["axis"], segmented=c["segmented"])
    b.flow = c["flow"]
    if c["images"]:
        b.GATE_IMAGES_MIN_N = dict(C.IMAGES_MIN_N)
    return b


def _dev(torch, a, dtype, unaligned=False):
    t = P.to_dev(np.array(a), dtype, torch)          # (a copy: the shared reference arrays are read-only)
    if unaligned:       # the same values one element into a fresh allocation: not 16-byte aligned
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    return t


def _bits(torch, t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES])
def test_nonfinite_activations_stay_inside_the_blocks_they_feed(env, cid):
    torch, BSMM, lib = env
    c, r = C.BY_ID[cid], C.reference(cid)
    dtype, bs, axis, N = c["dtype"], c["bs"], c["axis"], c["N"]
    b = _operator(BSMM, c)
    w = _dev(torch, r["W"], dtype)
    gate = torch.from_numpy(np.array(r["gate"])).cuda() if r["gate"] is not None else None
    if c["route"] == "flow" and 0 in c["kv"].values():
        assert torch.cuda.get_device_properties(0).multi_processor_count <= C.FLOW_RT4_CUS      # (what the 128-row-unit case is sized for)
    for which in c["passes"]:
        call = getattr(b, which)
        n_out = C.feat_blocks(c, which)[1]
        clean_in, bad_in = (_dev(torch, r[which][k], dtype, c["unaligned"]) for k in ("clean", "poisoned"))
        lib.set_kernel_variant(c["variant"])
        try:
            code = c["code"]
            if c["code_from_ungated"]:                      # the family of the ungated call over one weight image (finite stand-in weights)
                call(clean_in, torch.nan_to_num(w))
                code = lib.last_kernel()
            clean = call(clean_in, w, gate=gate)
            ran = [(lib.last_kernel(), lib.last_kernel_variant())]
            dirty = call(bad_in, w, gate=gate)
            ran.append((lib.last_kernel(), lib.last_kernel_variant()))
        finally:
            lib.set_kernel_variant(0)
        got, got_clean = P.to_host(dirty), P.to_host(clean)
        mask, want64 = r[which]["mask"], r[which]["want64"]
        nonfinite = ~np.isfinite(got)
        print("%s %s: trace %s (expected %s / %s); non-finite %d (expected %d), stray %d, missing %d" %
              (cid, which, ran, code, c["kv"], nonfinite.sum(), mask.sum(), (nonfinite & ~mask).sum(), (mask & ~nonfinite).sum()))
        for k, kv in ran:
            assert k == code and (c["kv"] is None or kv == c["kv"][which]), (cid, which, ran, code, c["kv"])
        # (a)
        stray, missing = np.argwhere(nonfinite & ~mask), np.argwhere(mask & ~nonfinite)
        assert len(stray) == 0 and len(missing) == 0, (cid, which, "stray non-finite outputs", stray[:8].tolist(), len(stray),
                                                       "finite outputs the poison must reach", missing[:8].tolist(), len(missing))
        # (b)
        fin = torch.from_numpy(~mask).cuda()
        if c["bitwise"]:
            differ = int((_bits(torch, dirty)[fin] != _bits(torch, clean)[fin]).sum().item())
            print("    finite elements whose bits differ from the clean call's: %d" % differ)
            assert differ == 0, (cid, which, differ)
        else:
            filled = np.where(mask, P.round_to_storage(want64, dtype), got)
            rep = P.block_report(P.act_blocks(filled, axis, N, n_out, bs), P.act_blocks(want64, axis, N, n_out, bs), dtype, n_out)
            print("    finite elements against the float64 walk: %s" % rep)
            assert rep["finite"] and rep["elem_bad"] == 0, (cid, which, rep)
            if dtype == "f32":
                assert rep["tensor_l2"] <= P.L2_BAR[dtype], (cid, which, rep)
        # (c)
        P.assert_blocks(P.act_blocks(got_clean, axis, N, n_out, bs), P.act_blocks(want64, axis, N, n_out, bs), dtype, n_out, ctx=(cid, which, "clean"))
