"""Times the two operators at the ends of a model -- softmax cross-entropy and the embedding lookup, forward and backward -- against the
torch composition and writes a markdown table:

    python scripts/bench_ends.py --out profiles/ends_bench.md

  xent-bytes   N = 65536 x K = 256 (a byte-level vocabulary), bf16
  xent-words   N = 8192 x K = 32768 (a word-level one), bf16
  xent-long    N = 2048 x K = 65536, bf16: rows beyond the registers, the streamed kernel (BSMM_XENT_LONG)
  embed-bytes-skew / embed-bytes-tiled      C = 256,   K = 1024, nIdx = 65536, bf16
  embed-words-skew / embed-words-tiled      C = 50257, K = 1024, nIdx = 65536, bf16
      skew: a seeded byte-like histogram (one index holds about a sixth, the rest fall off like 1 / rank); tiled: arange(1024) tiled over
      the batch, the positional table

torch = ``F.cross_entropy(reduction='none')`` and its autograd backward, resp. ``F.embedding`` and its autograd backward.  Beside them a device
copy of the largest tensor of the case, timed in the same process: its rate (bytes read + written) is the yardstick.  Each case runs in a
child process under a time limit (``--case`` is the child's entry).  Times are device events around a window of calls that is at least
``--window`` seconds long, after a warm-up; a measurement path that finds no GPU fails.  Bytes are algorithmic, with A = the bytes of the
(N, K) resp. (nIdx, K) tensor: cross-entropy forward 2 A (x read, g written), backward 2 A; embedding forward 2 A (rows read, y written),
backward A + 4 C K (dy read, fp32 dw written; the sort is timed inside the forward, where the Python layer runs it).  The last case,
``xent-fp32-bound``, times nothing: it evaluates the per-element bound of the fp32 stash (tests/test_ends_gpu.py) against float64 on the
device and reports the worst ratio."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XENT = {"xent-bytes": (65536, 256), "xent-words": (8192, 32768), "xent-long": (2048, 65536)}
EMBED = {"embed-bytes-skew": (256, "skew"), "embed-bytes-tiled": (256, "tiled"), "embed-words-skew": (50257, "skew"), "embed-words-tiled": (50257, "tiled")}
EK, ENIDX, CTX = 1024, 65536, 1024
BOUND = "xent-fp32-bound"
BOUND_SHAPES = ((64, 256), (16, 1031), (8, 8192), (4, 32768), (2, 70001))
ORDER = ("xent-bytes", "xent-words", "xent-long", "embed-bytes-skew", "embed-bytes-tiled", "embed-words-skew", "embed-words-tiled", BOUND)


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


def run_xent(name, window):
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "bench_ends needs a ROCm device"
    from blocksparse_amd import xent
    N, K = XENT[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = (4.0 * torch.randn((N, K), device="cuda", generator=gen)).bfloat16()
    labels = torch.randint(0, K, (N,), device="cuda", generator=gen)
    dy = torch.rand(N, device="cuda", generator=gen) + 0.5
    loss, g = xent.softmax_cross_entropy_fwd(x, labels)
    xr = x.clone().requires_grad_(True)
    tl = F.cross_entropy(xr, labels, reduction="none")
    copy_dst = torch.empty_like(x)
    t = {
        "copy": _time(torch, lambda: copy_dst.copy_(x), window),
        "torch_fwd": _time(torch, lambda: F.cross_entropy(x, labels, reduction="none"), window),
        "ours_fwd": _time(torch, lambda: xent.softmax_cross_entropy_fwd(x, labels), window),
        "torch_bwd": _time(torch, lambda: torch.autograd.grad(tl, xr, dy.to(tl.dtype), retain_graph=True), window),
        "ours_bwd": _time(torch, lambda: xent.softmax_cross_entropy_bwd(g, dy), window),
    }
    # the two forms computed the same loss
    ref = F.cross_entropy(x.double(), labels, reduction="none")
    err = float(((loss.double() - ref).norm() / ref.norm()).item())
    assert err < 2e-6, err
    A = x.numel() * x.element_size()
    return {"case": name, "what": "xent N %d x K %d" % (N, K), "us": {k: v * 1e6 for k, v in t.items()}, "fwd_bytes": 2 * A, "bwd_bytes": 2 * A,
            "copy_bytes": 2 * A, "path": xent.xent_path(x)}


def _indices(torch, C, pattern):
    import numpy as np
    if pattern == "tiled":
        return torch.arange(ENIDX, device="cuda") % min(CTX, C)
    rng = np.random.RandomState(7)
    ranks = np.arange(1, min(C, 256) + 1, dtype=np.float64)
    p = 1.0 / ranks
    p[0] = p[1:].sum() / 5.0                     # one index holds a sixth
    p /= p.sum()
    symbols = rng.permutation(C)[:ranks.size]
    return torch.from_numpy(symbols[rng.choice(ranks.size, size=ENIDX, p=p)]).to("cuda")


def run_embed(name, window):
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "bench_ends needs a ROCm device"
    from blocksparse_amd import embed
    C, pattern = EMBED[name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    w = torch.randn((C, EK), device="cuda", generator=gen).bfloat16()
    dy = torch.randn((ENIDX, EK), device="cuda", generator=gen).bfloat16()
    idx = _indices(torch, C, pattern)
    y, order = embed.embedding_lookup_fwd(w, idx)
    wr = w.clone().requires_grad_(True)
    ty = F.embedding(idx, wr)
    copy_dst = torch.empty_like(dy)
    t = {
        "copy": _time(torch, lambda: copy_dst.copy_(dy), window),
        "torch_fwd": _time(torch, lambda: F.embedding(idx, w), window),
        "ours_fwd": _time(torch, lambda: embed.embedding_lookup_fwd(w, idx), window),
        "ours_fwd_nosort": _time(torch, lambda: embed.embedding_lookup_fwd(w, idx, want_order=False), window),
        "torch_bwd": _time(torch, lambda: torch.autograd.grad(ty, wr, dy, retain_graph=True), window),
        "ours_bwd": _time(torch, lambda: embed.embedding_lookup_bwd(dy, idx, C, order=order), window),
    }
    assert torch.equal(y, F.embedding(idx, w))
    dw = embed.embedding_lookup_bwd(dy, idx, C, order=order)
    ref = torch.zeros((C, EK), dtype=torch.float64, device="cuda").index_add_(0, idx, dy.double())
    err = float(((dw.double() - ref).norm() / ref.norm()).item())
    assert err < 2e-6, err
    assert torch.equal(dw, embed.embedding_lookup_bwd(dy, idx, C, order=order))
    A = dy.numel() * dy.element_size()
    top = int(torch.bincount(idx).max().item())
    return {"case": name, "what": "embed C %d, %s (largest run %d)" % (C, pattern, top), "us": {k: v * 1e6 for k, v in t.items()}, "fwd_bytes": 2 * A,
            "bwd_bytes": A + 4 * C * EK, "copy_bytes": 2 * A}


def run_bound():
    import torch
    assert torch.cuda.is_available(), "bench_ends needs a ROCm device"
    from blocksparse_amd import xent
    gen = torch.Generator(device="cuda").manual_seed(3)
    worst = {"ratio": 0.0}
    for N, K in BOUND_SHAPES:
        for dist in ("normal", "uniform"):
            x = torch.randn((N, K), device="cuda", generator=gen) if dist == "normal" else 40.0 * torch.rand((N, K), device="cuda", generator=gen) - 20.0
            labels = torch.randint(0, K, (N,), device="cuda", generator=gen)
            _, g = xent.softmax_cross_entropy_fwd(x, labels)
            xd = x.double()
            m = xd.max(dim=1, keepdim=True)[0]
            p = torch.softmax(xd, dim=1)
            want = p.clone()
            want[torch.arange(N, device="cuda"), labels] -= 1.0
            bound = (4.0 + 2.0 * (xd - m).abs()) * 2.0 ** -22 * p + 2.0 ** -23 * want.abs() + 2.0 ** -149
            ratio = ((g.double() - want).abs() / bound).reshape(-1)
            at = int(ratio.argmax().item())
            if float(ratio[at]) > worst["ratio"]:
                worst = {"ratio": float(ratio[at]), "N": N, "K": K, "dist": dist, "row": at // K, "col": at % K, "x_minus_max": float((xd - m).reshape(-1)[at]),
                         "p": float(p.reshape(-1)[at])}
    return {"case": BOUND, "worst": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=ORDER, help="run one case in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends_bench.md"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one case's child process, seconds")
    a = ap.parse_args()
    if a.case:
        res = run_bound() if a.case == BOUND else (run_xent(a.case, a.window) if a.case in XENT else run_embed(a.case, a.window))
        print("RESULT " + json.dumps(res))
        return 0
    rows = []
    for name in ORDER:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_ends: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    tbs = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12
    out = ["# Embedding lookup and softmax cross-entropy: measured times (one MI355X)", "",
           "Written by `scripts/bench_ends.py`.  bf16 tensors; the embedding cases have K = %d features and nIdx = %d indices.  Call times from" % (EK, ENIDX),
           "device events over windows of >= %.1f s after a warm-up, one process per case, all forms in that process.  `torch` =" % a.window,
           "`F.cross_entropy(reduction='none')` resp. `F.embedding`, and autograd's backward of each; `ours` = the low-level pairs of",
           "`blocksparse_amd.xent` and `blocksparse_amd.embed`.  Bytes are algorithmic (A = the (N, K) resp. (nIdx, K) tensor): cross-entropy 2 A each",
           "way, embedding forward 2 A, backward A + the fp32 table; `copy` is `dst.copy_(src)` of that tensor (2 A) in the same process.  The",
           "embedding's forward includes the stable sort that builds the inverted index (`no sort` = the lookup alone).  Eager calls: the times",
           "include whatever the host adds when it cannot keep ahead of the device.", "",
           "| case | pass | torch us | ours us | torch / ours | ours TB/s | copy us | copy TB/s | ours rate / copy rate |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["case"] == BOUND:
            continue
        u = r["us"]
        copy_rate = tbs(r["copy_bytes"], u["copy"])
        passes = [("fwd", "forward")] + ([("fwd_nosort", "forward, no sort")] if "ours_fwd_nosort" in u else []) + [("bwd", "backward")]
        for p, label in passes:
            tp = "fwd" if p == "fwd_nosort" else p
            rate = tbs(r[tp + "_bytes"], u["ours_" + p])
            out.append("| %s | %s | %.1f | %.1f | %.2f | %.2f | %.1f | %.2f | %.0f %% |" % (
                r["what"], label, u["torch_" + tp], u["ours_" + p], u["torch_" + tp] / u["ours_" + p], rate, u["copy"], copy_rate, 100.0 * rate / copy_rate))
    w = [r for r in rows if r["case"] == BOUND][0]["worst"]
    out += ["", "## The fp32 stash against its per-element bound", "",
            "`|got - want| <= (4 + 2 |x - max|) 2^-22 p + 2^-23 |want| + 2^-149` against float64, over the shapes %s with N(0, 1) and U(-20, 20) logits:" % (
                ", ".join("%d x %d" % s for s in BOUND_SHAPES)),
            "worst ratio to the bound **%.3f**, at N %d x K %d (%s), row %d, class %d, x - max = %.3f, p = %.3e." % (
                w["ratio"], w["N"], w["K"], w["dist"], w["row"], w["col"], w["x_minus_max"], w["p"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
