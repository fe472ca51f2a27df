"""Times layer_norm (forward, and forward plus backward) against what a user could compose from torch today, and writes a markdown table.

    python scripts/bench_norms.py --out profiles/norms_bench.md

Shapes: the headline activation, 4096 features x 8192 samples in bf16, in both layouts, the small minibatch N = 64 on feature axis 0, and
rows of 16384 features on axis 1, which are streamed rather than kept in registers;
ReLU fused on our side, a separate ``relu`` on torch's.  Every shape runs in a child process of its own under a time limit (``--case`` is
the child's entry); the parent stops at the first child that fails.  Each timed function is captured into a graph of ``INNER`` calls (no
host time between launches), warmed up, and replayed in windows of at least ``--window`` seconds between device events; the figure is the
median of ``--repeats`` windows.  A measurement path that finds no GPU fails.  Rates are algorithmic bytes over that time: 2 s K N for the
forward (read x, write y), 3 s K N for the backward (read x and dy, write dx); statistics, gain and bias are not counted.

torch baselines: axis 1 ``F.layer_norm`` + ``relu`` (backward through autograd); axis 0 ``x.t().contiguous()`` -> ``F.layer_norm`` -> ``relu`` ->
``.t().contiguous()``, and the form composed from ``mean`` / ``var`` over dim 0 in fp32."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29          # measured device copy rate of the MI355X (profiles/optimize_bench.md)
INNER = 8
CASES = {
    # name: (K, N, axis, dtype)
    "axis0-N8192": (4096, 8192, 0, "bf16"),
    "axis1-N8192": (4096, 8192, 1, "bf16"),
    "axis0-N64": (4096, 64, 0, "bf16"),
    "axis1-K16384": (16384, 2048, 1, "bf16"),
}


def _time(torch, fn, window, repeats):
    """Median seconds per call of `fn`, replayed from a graph of INNER calls; ("eager", ...) if the function cannot be captured."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    mode = "graph"
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(INNER):
                fn()
        run = graph.replay
    except Exception as e:          # (a torch composition that allocates in a way a capture refuses: timed eagerly, and the table says so)
        sys.stderr.write("capture failed, timing eagerly: %r\n" % (e,))
        torch.cuda.synchronize()
        mode = "eager"

        def run():
            for _ in range(INNER):
                fn()
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        run()
    b.record()
    torch.cuda.synchronize()
    per = max(a.elapsed_time(b) / 3e3, 1e-6)
    iters = max(5, int(window / per))
    times = []
    for _ in range(repeats):
        a.record()
        for _ in range(iters):
            run()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3 / iters / INNER)
    return statistics.median(times), mode


def run_case(name, window, repeats):
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "bench_norms needs a ROCm device"
    from blocksparse_amd import norms
    K, N, axis, dtype = CASES[name]
    td = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[dtype]
    gen = torch.Generator(device="cuda").manual_seed(1)
    shape = (K, N) if axis == 0 else (N, K)
    x = torch.randn(shape, device="cuda", generator=gen).to(td)
    dy = torch.randn(shape, device="cuda", generator=gen).to(td)
    g = torch.randn(K, device="cuda", generator=gen)
    b = torch.randn(K, device="cuda", generator=gen)
    g16, b16 = g.to(td), b.to(td)
    eps = 1e-6

    def ours_fwd():
        return norms.layer_norm_fwd(x, g, b, axis=axis, epsilon=eps, relu=True)

    def ours_both():
        y, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, epsilon=eps, relu=True)
        return norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, epsilon=eps, relu=True)

    def with_grad(fwd):
        xr, gr, br = x.detach().requires_grad_(True), g16.detach().requires_grad_(True), b16.detach().requires_grad_(True)

        def both():
            return torch.autograd.grad(fwd(xr, gr, br), (xr, gr, br), dy)
        return both

    baselines = {}
    if axis == 1:
        f1 = lambda xx, gg, bb: F.relu(F.layer_norm(xx, (K,), gg, bb, eps))
        baselines["F.layer_norm + relu"] = (lambda: f1(x, g16, b16), with_grad(f1))
    else:
        f0 = lambda xx, gg, bb: F.relu(F.layer_norm(xx.t().contiguous(), (K,), gg, bb, eps)).t().contiguous()

        def fc(xx, gg, bb):
            xf = xx.float()
            mean = xf.mean(0, keepdim=True)
            var = xf.var(0, unbiased=False, keepdim=True)
            return F.relu((xf - mean) * torch.rsqrt(var + eps) * gg.float()[:, None] + bb.float()[:, None]).to(xx.dtype)
        baselines["transpose, F.layer_norm + relu, transpose"] = (lambda: f0(x, g16, b16), with_grad(f0))
        baselines["composed mean / var"] = (lambda: fc(x, g16, b16), with_grad(fc))
    # agreement on the timed inputs (bf16-level: torch rounds its gain, bias and intermediate results in its own places)
    ref = list(baselines.values())[0][0]().float()
    rel = float((ours_fwd()[0].float() - ref).norm() / ref.norm())
    es = 4 if dtype == "f32" else 2
    nb = {"fwd": 2 * es * K * N, "fwd+bwd": 5 * es * K * N}
    out = {"case": name, "shape": "%d features x %d samples, axis %d, %s" % (K, N, axis, dtype), "rel_diff_vs_torch": rel, "rows": []}
    for what, fn in (("fwd", ours_fwd), ("fwd+bwd", ours_both)):
        t, mode = _time(torch, fn, window, repeats)
        row = {"what": what, "us": t * 1e6, "mode": mode, "bytes": nb[what], "gbs": nb[what] / t / 1e9, "baselines": {}}
        for bname, (bf, bb) in baselines.items():
            tb, bmode = _time(torch, bf if what == "fwd" else bb, window, repeats)
            row["baselines"][bname] = {"us": tb * 1e6, "mode": bmode}
        out["rows"].append(row)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--case", choices=sorted(CASES), help="run one shape in this process and print its JSON line")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "norms_bench.md"))
    p.add_argument("--window", type=float, default=0.3, help="seconds of timed work per window")
    p.add_argument("--repeats", type=int, default=5, help="windows per measurement (the median is reported)")
    p.add_argument("--timeout", type=int, default=170, help="time limit of one shape's child process, seconds")
    a = p.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window, a.repeats)))
        return 0
    results = []
    for name in ("axis0-N8192", "axis1-N8192", "axis0-N64", "axis1-K16384"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window), "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_norms: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        results.append(json.loads(line[0][7:]))
        print(line[0])
    out = ["# Layer norm: measured times (one MI355X)", "",
           "Written by `scripts/bench_norms.py`.  Each function is captured into a graph of %d calls, warmed up and replayed in windows of" % INNER,
           ">= %.1f s between device events; the figure is the median of %d windows, one process per shape.  `ours` = `layer_norm_fwd` with the" % (a.window, a.repeats),
           "fused ReLU (`fwd`) and `layer_norm_fwd` + `layer_norm_bwd` (`fwd+bwd`); the torch columns are what a user composes today, with a",
           "separate `relu` and the backward through autograd.  GB/s = algorithmic bytes (2 s K N forward, 3 s K N backward) over the time;",
           "the ceiling is the measured device copy rate, %.2f TB/s." % COPY_CEILING_TBS, "",
           "| shape | pass | ours us | bytes | GB/s | of the %.2f TB/s ceiling | torch baseline | torch us | torch / ours |" % COPY_CEILING_TBS,
           "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for row in r["rows"]:
            for bname, bl in row["baselines"].items():
                out.append("| %s | %s | %.1f%s | %.1f MB | %.0f | %.0f %% | %s | %.1f%s | %.2f |" % (
                    r["shape"], row["what"], row["us"], "" if row["mode"] == "graph" else " (eager)", row["bytes"] / 1e6, row["gbs"],
                    100.0 * row["gbs"] / (COPY_CEILING_TBS * 1e3), bname, bl["us"], "" if bl["mode"] == "graph" else " (eager)", bl["us"] / row["us"]))
    out += ["", "Agreement on the timed inputs (relative L2 difference of the forward results, ours vs the first torch baseline; torch takes bf16 gain and",
            "bias): %s." % ", ".join("%.1e" % r["rel_diff_vs_torch"] for r in results), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
