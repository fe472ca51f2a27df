"""Matmul operands at and past the 32-bit offset limits (tests/_big_operands.py holds the case table, the data and the reasoning; the CPU
tier, test_big_operands_host.py, shows that the data make bit equality the right check and that the comparison used here catches three
addressing faults).

Every case runs fprop, bprop and updat one after the other, each pass holding only its own tensors, and compares ALL of Y and DX on the
device and DW on the host, bit for bit, with the float64 oracle of one period rounded once.  Where the table names a kernel family the
trace code is asserted: `is` below a threshold, `not` at it.  The row-stride family may be refused instead (a non-zero return code) -- then
the output buffer, filled with a sentinel beforehand, must be untouched.  A case skips only when the device has less free memory than the
table says it needs.

Problems are collected while the tensors live and asserted after they are freed, so a failing case does not keep gigabytes alive in its
traceback for the rest of the suite.  A HIP error ends the session at once: nothing more is started on a device that has faulted."""
import ctypes
import gc
import time

import numpy as np
import pytest

import _big_operands as B

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import BlocksparseMatMul, _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()
    return torch, BlocksparseMatMul, _lib


def _stop_on_fault(case, what, exc):
    text = str(exc)
    code = getattr(exc, "code", 0)          # (a BsmmError that carries a hipError_t: 700 and up are device faults, 1 / 9 a launch HIP refused)
    if "HIP error" in text or "CUDA error" in text or "hipError" in text or "illegal memory access" in text or code >= 700:
        pytest.exit("big-operands %s %s: the device reported %s -- nothing more is run on it" % (case["id"], what, text.splitlines()[0]), returncode=70)


def _kernel_problem(lib, case, what, kernel):
    how, name = case["expect"].get(what, (None, None))
    if how == "is" and kernel != getattr(lib, name):
        return "%s ran kernel family %d, expected %s (%d)" % (what, kernel, name, getattr(lib, name))
    if how == "not" and kernel == getattr(lib, name):
        return "%s still ran %s (%d) past its limit" % (what, name, kernel)
    return None


def _abi_xprop(torch, lib, b, which, inp, w, out):
    """bsmm_fprop / bsmm_bprop into a buffer of the caller's (the product API allocates its own): the return code."""
    L = lib.load()
    tabs = b._tables_on(inp.device)
    op, _, fin, fout, entry = b._XPROP[which]
    Cin, Kout = getattr(b, fin), getattr(b, fout)
    N = inp.numel() // Cin
    a = b._args(getattr(tabs, which), b._dev_tables[which], N, Cin, Kout, inp.dtype, plan=b._xprop_plan(tabs, which, N, Kout, inp.dtype, None))
    ws = torch.empty(max(int(L.bsmm_workspace_bytes(op, ctypes.byref(a))), 16), dtype=torch.uint8, device=inp.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    rc = getattr(L, entry)(inp.data_ptr(), w.data_ptr(), out.data_ptr(), ctypes.byref(a))
    torch.cuda.synchronize()
    return rc


def _untouched(torch, t):
    return int(torch.count_nonzero(B._bits(torch, t) != SENTINEL).item()) == 0


def _xprop_pass(env, case, b, which, w, ex, st, problems):
    torch, _, lib = env
    axis, N = case["axis"], case["N"]
    base, rows, per, mk, feat = ("X", "Xm", "Yp", "Ym", b.K) if which == "fprop" else ("E", "Em", "DXp", "DXm", b.C)
    t0 = time.time()
    inp = B.fill(torch, st(ex[base]), N, axis, ex["markers"], st(ex[rows]))
    out, outcome = None, "ok"
    if case["refusal_ok"]:
        out = torch.empty((N, feat) if axis else (feat, N), dtype=inp.dtype, device=inp.device)
        B._bits(torch, out).fill_(SENTINEL)
        rc = _abi_xprop(torch, lib, b, which, inp, w, out)
        if rc != 0:
            outcome = "refused rc=%d" % rc
            if not _untouched(torch, out):
                problems.append("%s returned %d but wrote into the output" % (which, rc))
    else:
        out = b.fprop(inp, w) if which == "fprop" else b.bprop(inp, w)
        torch.cuda.synchronize()
    kernel = lib.last_kernel()
    t1 = time.time()
    if outcome == "ok":
        problems.append(_kernel_problem(lib, case, which, kernel))
        bad, found = B.count_mismatches(torch, out, st(ex[per]), axis, ex["markers"], st(ex[mk]))
        if bad:
            outcome = "WRONG"
            problems.append("%s (kernel family %d): %d of %d elements differ; (minibatch row, feature, got bits, want bits) %s"
                            % (which, kernel, bad, out.numel(), found))
    print("big-operands %s %s kernel=%d %s call %.2fs check %.2fs" % (case["id"], which, kernel, outcome, t1 - t0, time.time() - t1))


def _updat_pass(env, case, b, ex, st, problems):
    torch, _, lib = env
    axis, N = case["axis"], case["N"]
    t0 = time.time()
    x = B.fill(torch, st(ex["X"]), N, axis, ex["markers"], st(ex["Xm"]))
    e = B.fill(torch, st(ex["E"]), N, axis, ex["markers"], st(ex["Em"]))
    calls64 = []
    if case["native64"] is not None:
        inner = b._updat64
        b._updat64 = lambda *a, **k: (calls64.append(1), inner(*a, **k))[1]
    dw = torch.empty(b.w_shape, dtype=x.dtype, device=x.device)
    B._bits(torch, dw).fill_(SENTINEL)
    outcome = "ok"
    try:
        b.updat(x, e, dw=dw)
        torch.cuda.synchronize()
    except lib.BsmmError as err:
        if not case["refusal_ok"]:
            raise
        outcome = "refused rc=%d" % err.code
        torch.cuda.synchronize()
        if not _untouched(torch, dw):
            problems.append("updat returned %d but wrote into DW" % err.code)
    kernel = lib.last_kernel()
    t1 = time.time()
    if outcome == "ok":
        problems.append(_kernel_problem(lib, case, "updat", kernel))
        if case["native64"] is not None and bool(calls64) == case["native64"]:
            problems.append("bsize 64 updat: native path expected %s, quadrant view called %d times" % (case["native64"], len(calls64)))
        got, want = B._bits(torch, dw.cpu()).numpy(), B._bits(torch, B.to_storage(torch, ex["DW"], case["dtype"])).numpy()
        diff = np.argwhere(got != want)
        if len(diff):
            outcome = "WRONG"
            first = [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in diff[:8]]
            problems.append("updat (kernel family %d): %d of %d elements of DW differ; ((block, row, column), got bits, want bits) %s"
                            % (kernel, len(diff), got.size, first))
    print("big-operands %s updat kernel=%d %s call %.2fs check %.2fs" % (case["id"], kernel, outcome, t1 - t0, time.time() - t1))


@pytest.mark.parametrize("case", B.CASES, ids=[c["id"] for c in B.CASES])
def test_big_operands(env, case):
    torch, BSMM, lib = env
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < case["bytes"]:
        pytest.skip("%s needs %.2f GiB of device memory, %.2f GiB are free: %.2f GiB short"
                    % (case["id"], case["bytes"] / B.GIB, free / B.GIB, (case["bytes"] - free) / B.GIB))
    t0 = time.time()
    ex = B.expected(case)
    t_host = time.time() - t0
    problems = []
    state = {}
    try:
        state["b"] = b = BSMM(B.layout(case["layout"]), block_size=case["bs"], feature_axis=case["axis"], segmented=case["segmented"])
        if case["segmented"]:
            assert b._dev_tables["fprop"]["locks"] > 0 and b._dev_tables["bprop"]["locks"] > 0
        st = lambda a: B.to_storage(torch, a, case["dtype"], "cuda")
        state["w"] = w = st(ex["W"])
        lib.set_kernel_variant(case["variant"])
        what = "fprop"
        try:
            _xprop_pass(env, case, b, "fprop", w, ex, st, problems)
            b._workspaces.clear()             # (an operator keeps one scratch per pass: the fp32 image of locked outputs is 8 GiB here)
            what = "bprop"
            _xprop_pass(env, case, b, "bprop", w, ex, st, problems)
            b._workspaces.clear()
            what = "updat"
            _updat_pass(env, case, b, ex, st, problems)
        except (RuntimeError, lib.BsmmError) as exc:
            _stop_on_fault(case, what, exc)
            problems.append("%s raised %s: %s" % (what, type(exc).__name__, str(exc).splitlines()[0]))
        peak = torch.cuda.max_memory_allocated()
    finally:
        lib.set_kernel_variant(0)
        state.clear()
        b = w = st = None
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    problems = [p for p in problems if p]
    print("big-operands %s table %.2f GiB, peak allocated %.2f GiB, host oracle %.2fs, wall %.2fs, %s"
          % (case["id"], case["bytes"] / B.GIB, peak / B.GIB, t_host, time.time() - t0, "FAILED" if problems else "passed"))
    assert peak <= case["bytes"], (case["id"], "the table understates the device bytes", peak, case["bytes"])
    assert not problems, (case["id"], problems)
