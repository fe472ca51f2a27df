"""Times the fused weight update (clip_by_global_norm over one tensor + adam_step with a bf16 working copy and a 0/1 gate + ema_step) against
what a user could compose from torch today, and writes a markdown table.

    python scripts/bench_optimize.py --out profiles/optimize_bench.md

Shape: the headline weight tensor (4096 x 4096, block size 32, density 20 %: ~3.36 M fp32 elements, fp32 gradients on both sides) with every
block live and with a quarter of the blocks gated off.  The torch composition is ``clip_grad_norm_`` + ``torch.optim.Adam(fused=True)`` +
re-masking (``p.mul_(mask)``) + ``p16.copy_(p)`` + ``ema.lerp_``; it always touches every block.  The measurement runs in a child process
under a time limit (``--case`` is the child's entry).  Times are device events around a window of calls that is at least ``--window`` seconds
long, after a warm-up; a measurement path that finds no GPU fails.  Bytes are algorithmic bytes of the live elements: clip 4 (one read of
the gradient), Adam 4 + 12 read and 12 + 2 written, the average 8 read and 4 written."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29          # measured device-to-device copy rate of the MI355X (read + write bytes), profiles/sparsity_bench.md
CASES = {
    # name: (hidden, bsize, density, fraction of the blocks whose gate is 1)
    "headline-live": (4096, 32, 0.20, 1.0),
    "headline-gated": (4096, 32, 0.20, 0.75),
}
BYTES = {"clip": 4, "adam": 30, "ema": 12}


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
    assert torch.cuda.is_available(), "bench_optimize needs a ROCm device"
    from blocksparse_amd import adam_step, clip_by_global_norm, ema_step
    hidden, bs, density, live_frac = CASES[name]
    CB = hidden // bs
    blocks = int((np.random.default_rng(1234).random((CB, CB)) < density).sum())          # the layout bench.py times: 3279 blocks
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda scale: torch.randn((blocks, bs, bs), device="cuda", generator=gen) * scale
    w, g = rnd(0.01), rnd(0.1)
    gate = (torch.rand(blocks, device="cuda", generator=gen) < live_frac).float()
    live = float(gate.mean())
    # ours
    p, m, v, e, p16 = w.clone(), torch.zeros_like(w), torch.zeros_like(w), w.clone(), w.to(torch.bfloat16)

    def fused():
        _, scale = clip_by_global_norm([g], clip_norm=1.0)
        adam_step(p, g, m, v, 3e-4, gate=gate, norm_scale=scale, param16=p16)
        ema_step(e, p, 0.999, gate=gate)

    scale1 = clip_by_global_norm([g], clip_norm=1.0)[1]
    # the torch composition
    tp = torch.nn.Parameter(w.clone())
    tp.grad = g.clone()
    opt = torch.optim.Adam([tp], lr=3e-4, fused=True)
    te, tp16, mask = w.clone(), w.to(torch.bfloat16), gate.view(-1, 1, 1)

    def composed():
        torch.nn.utils.clip_grad_norm_([tp], 1.0)
        opt.step()
        with torch.no_grad():
            tp.mul_(mask)
            tp16.copy_(tp)
            te.lerp_(tp, 1.0 - 0.999)

    t_fused, n1 = _time(torch, fused, window)
    t_comp, n2 = _time(torch, composed, window)
    t_clip, n3 = _time(torch, lambda: clip_by_global_norm([g], clip_norm=1.0), window)
    t_adam, n4 = _time(torch, lambda: adam_step(p, g, m, v, 3e-4, gate=gate, norm_scale=scale1, param16=p16), window)
    t_ema, n5 = _time(torch, lambda: ema_step(e, p, 0.999, gate=gate), window)
    n = blocks * bs * bs
    by = {"clip": BYTES["clip"] * n, "adam": BYTES["adam"] * n * live, "ema": BYTES["ema"] * n * live}
    return {"case": name, "shape": "%d x %d, bsize %d, %d blocks (%.2f M elements), %.0f %% of the gates 1" % (hidden, hidden, bs, blocks, n / 1e6, 100 * live),
            "fused_us": t_fused * 1e6, "composed_us": t_comp * 1e6, "clip_us": t_clip * 1e6, "adam_us": t_adam * 1e6, "ema_us": t_ema * 1e6,
            "bytes": by, "fused_bytes": sum(by.values()), "calls": [n1, n2, n3, n4, n5]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), help="run one shape in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimize_bench.md"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one shape's child process, seconds")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window)))
        return 0
    rows = []
    for name in ("headline-live", "headline-gated"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_optimize: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    tbs = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12
    out = ["# Fused weight update: measured times (one MI355X)", "",
           "Written by `scripts/bench_optimize.py`.  Call times from device events over windows of >= %.1f s after a warm-up, one process per" % a.window,
           "shape, both sides in that process.  `fused` = `clip_by_global_norm` over the one tensor + `adam_step` (fp32 gradient, bf16 working copy,",
           "0/1 gate, the clip's `norm_scale`) + `ema_step`: four launches.  `composed` = `clip_grad_norm_` + `torch.optim.Adam(fused=True)` +",
           "`p.mul_(mask)` + `p16.copy_(p)` + `ema.lerp_`, which touches every block whatever the gate.  Bytes are algorithmic bytes of the live",
           "elements (clip 4, Adam 30, average 12 per element); the ceiling is the measured device copy rate, %.2f TB/s.  Eager calls: the times" % COPY_CEILING_TBS,
           "include whatever the host adds when it cannot keep ahead of the device.", "",
           "| shape | fused us | composed us | composed / fused | fused bytes | fused TB/s | of the %.2f TB/s ceiling |" % COPY_CEILING_TBS,
           "|---|---|---|---|---|---|---|"]
    for r in rows:
        rate = tbs(r["fused_bytes"], r["fused_us"])
        out.append("| %s | %.1f | %.1f | %.2f | %.1f MB | %.2f | %.0f %% |" % (r["shape"], r["fused_us"], r["composed_us"], r["composed_us"] / r["fused_us"],
                                                                               r["fused_bytes"] / 1e6, rate, 100.0 * rate / COPY_CEILING_TBS))
    out += ["", "Each call on its own (back to back calls of one kind).  The clip is two dependent launches -- the sum of squares, then one workgroup --",
            "and two small allocations: its time is what issuing them costs, not its bytes.  The fused sequence is four eager launches from Python and",
            "is bound the same way wherever the row with fewer live blocks is no faster than the row with all of them:", "",
            "| shape | call | us | bytes | TB/s |", "|---|---|---|---|---|"]
    for r in rows:
        for k in ("clip", "adam", "ema"):
            out.append("| %s | %s | %.1f | %.1f MB | %.2f |" % (r["shape"], k, r[k + "_us"], r["bytes"][k] / 1e6, tbs(r["bytes"][k], r[k + "_us"])))
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
