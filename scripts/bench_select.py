"""Times the fused row selection -- the softmax over the k largest scores of a row, forward and backward -- against the eager torch
composition and writes a markdown table:

    python scripts/bench_select.py --out profiles/select_bench.md

  torch      what a user composes without the operator: the mask product and the scale, ``topk``, a ``-inf`` fill with the kept scores
             scattered into it, ``softmax`` (k = K: the product and ``softmax`` alone); the backward is the same formula the fused gradient
             evaluates, written with torch ops
  fused      ``masked_top_k_softmax_fwd`` and ``masked_softmax_bwd``, one launch each

Shape: x = (8, 16, 1024, 1024) bf16 -- R = 8 * 16 * 1024 rows of K = 1024 --, k = 32 and k = K, with and without a (1, 1, T, K) fp32 mask.
Beside them a device copy of one such tensor, timed in the same process: its rate (bytes read + written) is the yardstick.  Each case runs
in a child process under a time limit (``--case`` is the child's entry).  Times are device events around a window of calls that is at least
``--window`` seconds long, after a warm-up; a measurement path that finds no GPU fails.  Bytes are algorithmic: with A = the bytes of x the
forward moves 2 A (x read, y written) and the backward 3 A (dy and y read, dx written); the 4 MB mask stays in cache.  The torch form is
charged the same bytes, so its rate shows what the extra passes cost.  The count steps of the selection are the same 32 whatever k is, so
the k = K rows (no selection at all) against the k = 32 rows show what they cost on top of the memory stream."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, T, K, SCALE = 8, 16, 1024, 1024, 0.125
CASES = {"k32": (32, False), "k32-mask": (32, True), "kK": (K, False), "kK-mask": (K, True)}


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
    return a.elapsed_time(b) / 1e3 / iters


def run_case(name, window):
    import torch
    assert torch.cuda.is_available(), "bench_select needs a ROCm device"
    from blocksparse_amd import select
    k, with_mask = CASES[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((B, H, T, K), device="cuda", generator=gen).bfloat16()
    dy = torch.randn((B, H, T, K), device="cuda", generator=gen).bfloat16()
    mask = torch.tril(torch.ones(T, K, device="cuda")).view(1, 1, T, K) if with_mask else None
    assert select.select_path(K, x.dtype, True) == "wave16-wide"

    def torch_fwd():
        v = (x * mask * SCALE) if with_mask else (x * SCALE)
        if with_mask:
            v = v.masked_fill(mask == 0, float("-inf"))
        if k < K:
            top = v.topk(k, dim=-1)
            v = torch.full_like(v, float("-inf")).scatter_(-1, top.indices, top.values)
        return torch.softmax(v, dim=-1)

    y = select.masked_top_k_softmax_fwd(x, k, mask, SCALE)

    def torch_bwd():
        g = (dy - (dy * y).sum(dim=-1, keepdim=True)) * y
        return (g * mask * SCALE) if with_mask else (g * SCALE)

    copy_dst = torch.empty_like(x)
    t = {
        "copy": _time(torch, lambda: copy_dst.copy_(x), window),
        "torch_fwd": _time(torch, torch_fwd, window),
        "fused_fwd": _time(torch, lambda: select.masked_top_k_softmax_fwd(x, k, mask, SCALE), window),
        "torch_bwd": _time(torch, torch_bwd, window),
        "fused_bwd": _time(torch, lambda: select.masked_softmax_bwd(dy, y, mask, SCALE), window),
    }
    # both forms computed the same thing; the selected sets are compared row by row and the share of equal rows is reported, not asserted:
    # bf16 scores tie at the k-th position in many rows, and there torch.topk keeps whichever of the equal scores its launch found
    ty = torch_fwd()
    same_set = float(((ty != 0) == (y != 0)).all(dim=-1).float().mean())
    diff = lambda p, q: float((p.float() - q.float()).norm() / q.float().norm())
    agree = {"rows_with_the_same_set": same_set, "dx": diff(select.masked_softmax_bwd(dy, y, mask, SCALE), torch_bwd())}
    assert agree["dx"] < 0.05, agree
    A = x.numel() * x.element_size()
    return {"case": name, "k": k, "mask": with_mask, "us": {n: v * 1e6 for n, v in t.items()}, "A": A, "fwd_bytes": 2 * A, "bwd_bytes": 3 * A,
            "copy_bytes": 2 * A, "agree": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), help="run one case in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.md"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one case's child process, seconds")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window)))
        return 0
    rows = []
    for name in ("k32", "k32-mask", "kK", "kK-mask"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_select: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    tbs = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12
    out = ["# Fused row selection: measured times (one MI355X)", "",
           "Written by `scripts/bench_select.py`.  x = (%d, %d, %d, %d) bf16: R = %d rows of K = %d (A = %.0f MB), scale %.3f, the mask a" % (
               B, H, T, K, B * H * T, K, rows[0]["A"] / 1e6, SCALE),
           "(1, 1, T, K) fp32 lower triangle.  Call times from device events over windows of >= %.1f s after a warm-up, one process per row pair," % a.window,
           "both forms in that process.  `torch` = mask product, scale, `topk`, `scatter_` into a `-inf` fill, `softmax` (k = K: product and",
           "`softmax`), and the gradient formula in torch ops; `fused` = `masked_top_k_softmax_fwd` / `masked_softmax_bwd`, one launch each (path",
           "`wave16-wide`).  Both forms are charged the fused form's algorithmic bytes: 2 A forward, 3 A backward; `copy` is `dst.copy_(src)` of",
           "one such tensor (2 A) in the same process.  Eager calls: the times include whatever the host adds when it cannot keep ahead of the",
           "device.", "",
           "| k, mask | pass | MB moved | torch us | fused us | torch / fused | fused TB/s | copy us | copy TB/s | fused rate / copy rate |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us"]
        copy_rate = tbs(r["copy_bytes"], u["copy"])
        for p, label in (("fwd", "forward"), ("bwd", "backward")):
            rate = tbs(r[p + "_bytes"], u["fused_" + p])
            out.append("| k = %d, %s | %s | %.0f | %.1f | %.1f | %.2f | %.2f | %.1f | %.2f | %.0f %% |" % (
                r["k"], "mask" if r["mask"] else "no mask", label, r[p + "_bytes"] / 1e6, u["torch_" + p], u["fused_" + p],
                u["torch_" + p] / u["fused_" + p], rate, u["copy"], copy_rate, 100.0 * rate / copy_rate))
    by = dict((r["case"], r["us"]["fused_fwd"]) for r in rows)
    out += ["",
            "Which part dominates the forward: the k = K rows run no selection at all (the same loads, exponentials and stores), so",
            "`fused us (k = 32) - fused us (k = K)` is what the 32 count steps and the tie prefix add to the memory stream: %.1f us on %.1f us" % (
                by["k32"] - by["kK"], by["kK"]),
            "without a mask, %.1f us on %.1f us with one (measured, this run).  %s" % (
                by["k32-mask"] - by["kK-mask"], by["kK-mask"],
                "The count steps dominate the top-k forward." if by["k32"] > 2 * by["kK"] else "The memory stream dominates the top-k forward."
                if by["k32"] < 1.5 * by["kK"] else "Count steps and memory stream weigh about the same in the top-k forward."),
            ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
