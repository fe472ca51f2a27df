"""Times the block-reduced full weight gradient (BlocksparseMatMul.block_reduced_full_dw) against what a user could compose from torch
today, and against ``exact=True``, and writes a markdown table.

    python scripts/bench_sparsity.py --out profiles/sparsity_bench.md

Shapes: the headline (4096 x 4096, block size 32, feature axis 1, bf16, minibatch 8192) with 1 and 8 (x, dy) pairs, and BASELINE configs[2]
(block size 16, feature axis 0, density 10 %) with 1 pair.  Every shape runs in a child process of its own under a time limit
(``--case`` is the child's entry); the parent stops at the first child that fails.  Times are device events around a window of calls that
is at least ``--window`` seconds long, after a warm-up of every shape; a measurement path that finds no GPU fails.  The reduce kernel's
rate is its algorithmic bytes s (C + K) N pairs (one read of X and DY; the reduced outputs, 1 / bsize of that, are not counted) over the
event time of the two bsmm_feature_reduce calls."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29          # measured device-to-device copy rate of the MI355X (read + write bytes), the ceiling of a streaming kernel
CASES = {
    # name: (hidden, bsize, axis, density, dtype, minibatch, pairs)
    "headline-p1": (4096, 32, 1, 0.20, "bf16", 8192, 1),
    "headline-p8": (4096, 32, 1, 0.20, "bf16", 8192, 8),
    "cfg2-p1": (4096, 16, 0, 0.10, "bf16", 8192, 1),
}


def _time(torch, fn, window):
    """Seconds per call: device events around enough calls to fill `window` seconds (at least 10), after a warm-up."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    per = max(a.elapsed_time(b) / 3e3, 1e-6)
    iters = max(10, int(window / per))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / iters, iters


def run_case(name, window):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_sparsity needs a ROCm device"
    from blocksparse_amd import BlocksparseMatMul, sparsity
    hidden, bs, axis, density, dtype, N, pairs = CASES[name]
    td = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[dtype]
    CB = hidden // bs
    lay = (np.random.default_rng(0).random((CB, CB)) < density).astype(np.int32)
    lay[np.arange(CB), np.arange(CB)] = 1
    bsmm = BlocksparseMatMul(lay, block_size=bs, feature_axis=axis)
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [(torch.randn(bsmm.i_shape(N), device="cuda", generator=g) * 0.1).to(td) for _ in range(pairs)]
    dys = [(torch.randn(bsmm.o_shape(N), device="cuda", generator=g) * 0.1).to(td) for _ in range(pairs)]

    def composed():          # what a user writes today: reshape, abs, amax, concatenate the pairs along the contraction, one matmul
        if axis == 1:
            xr = torch.cat([x.abs().view(N, CB, bs).amax(-1) for x in xs], 0)
            yr = torch.cat([y.abs().view(N, CB, bs).amax(-1) for y in dys], 0)
            return (xr.t() @ yr).float()
        xr = torch.cat([x.abs().view(CB, bs, N).amax(1) for x in xs], 1)
        yr = torch.cat([y.abs().view(CB, bs, N).amax(1) for y in dys], 1)
        return (xr @ yr.t()).float()

    def reduce_only():
        sparsity.feature_reduce(xs, bs, axis, "max")
        sparsity.feature_reduce(dys, bs, axis, "max")

    ours = bsmm.block_reduced_full_dw(xs, dys)
    ref = composed()
    rel = float((ours - ref).norm() / ref.norm())       # (the composition's matmul accumulates and rounds in its own way: bf16-level agreement)
    exact = bsmm.block_reduced_full_dw(xs, dys, exact=True)
    ratio = float((ours / exact).median())
    t_ours, n1 = _time(torch, lambda: bsmm.block_reduced_full_dw(xs, dys), window)
    t_comp, n2 = _time(torch, composed, window)
    t_exact, n3 = _time(torch, lambda: bsmm.block_reduced_full_dw(xs, dys, exact=True), window)
    t_red, n4 = _time(torch, reduce_only, window)
    es = 4 if dtype == "f32" else 2
    nbytes = es * (bsmm.C + bsmm.K) * N * pairs
    return {"case": name, "shape": "%d x %d, bsize %d, axis %d, %s, N %d, %d pair(s)" % (hidden, hidden, bs, axis, dtype, N, pairs),
            "reduced_us": t_ours * 1e6, "composed_us": t_comp * 1e6, "exact_us": t_exact * 1e6, "reduce_us": t_red * 1e6,
            "reduce_bytes": nbytes, "reduce_tbs": nbytes / t_red / 1e12, "rel_diff_vs_composed": rel, "median_reduced_over_exact": ratio,
            "calls": [n1, n2, n3, n4]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--case", choices=sorted(CASES), help="run one shape in this process and print its JSON line")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparsity_bench.md"))
    p.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    p.add_argument("--timeout", type=int, default=150, help="time limit of one shape's child process, seconds")
    a = p.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window)))
        return 0
    rows = []
    for name in ("headline-p1", "headline-p8", "cfg2-p1"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_sparsity: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    out = ["# Block-reduced full dW: measured times (one MI355X)", "",
           "Written by `scripts/bench_sparsity.py`.  Call times from device events over windows of >= %.1f s after a warm-up, one process per" % a.window,
           "shape.  `reduced` = `block_reduced_full_dw` (two `bsmm_feature_reduce` launches + `bsmm_reduced_dw`), `composed` = the torch composition",
           "`x.abs().view(N, CB, bs).amax(-1)` + concatenation + one matmul, `exact` = `block_reduced_full_dw(exact=True)` (dense weight gradient of the",
           "all-ones twin + block norms).  Reduce rate = algorithmic bytes s (C + K) N pairs over the time of the two reduce calls; the ceiling is",
           "the measured device copy rate, %.2f TB/s." % COPY_CEILING_TBS, "",
           "| shape | reduced us | composed us | exact us | composed / reduced | reduce calls us | reduce bytes | reduce TB/s | of the %.2f TB/s ceiling |" % COPY_CEILING_TBS,
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %s | %.1f | %.1f | %.1f | %.2f | %.1f | %.1f MB | %.2f | %.0f %% |" % (
            r["shape"], r["reduced_us"], r["composed_us"], r["exact_us"], r["composed_us"] / r["reduced_us"], r["reduce_us"], r["reduce_bytes"] / 1e6,
            r["reduce_tbs"], 100.0 * r["reduce_tbs"] / COPY_CEILING_TBS))
    out += ["", "Agreement on the timed inputs: relative L2 difference reduced vs composed %s; median reduced / exact %s (the reduced score is an"
            % (", ".join("%.1e" % r["rel_diff_vs_composed"] for r in rows), ", ".join("%.1f" % r["median_reduced_over_exact"] for r in rows)),
            "upper bound of the block norm, not an estimate of it).  `exact` takes its norms of the fp32 sums of the streaming weight-gradient kernel at",
            "bsize 32; at bsize 16 it runs the fp32 weight gradient of fp32 copies of the activations.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
