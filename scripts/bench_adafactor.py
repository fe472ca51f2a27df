"""Times ``adafactor_step`` against the torch composition of the same arithmetic and against ``adam_step`` on the same tensor, and writes a
markdown table.

    python scripts/bench_adafactor.py --out profiles/adafactor_bench.md

Tensors: a dense 4096 x 4096 with a bf16 gradient, the headline block-sparse weight (3277 blocks of 32 x 32, fp32 gradient) with every
block live and with a quarter of the blocks gated off, and a 1-d tensor of 4096.  Every call writes a bf16 working copy.  The torch
composition (which always touches every block, whatever the gate) is written out in ``_composed``.  Each measurement runs in a child
process under a time limit (``--case`` is the child's entry).  Times are device events around a window of calls that is at least
``--window`` seconds long, after a warm-up; a measurement path that finds no GPU fails.  Bytes are the bytes the form must move per live
element: the gradient as often as the form reads it (3 / 2 / 2 times for the 2-d / 1-d / block form), param read and written, the 16-bit
copy written; the moments and the workspace are left out.  No figure here is a pass condition."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29          # measured device-to-device copy rate of the MI355X (read + write bytes), profiles/sparsity_bench.md
CASES = {
    # name: (form, rows, cols or bsize, gradient dtype, fraction of the blocks whose gate is 1)
    "dense-4096x4096-bf16": ("2d", 4096, 4096, "bfloat16", 1.0),
    "headline-blocks-live": ("block", 3277, 32, "float32", 1.0),
    "headline-blocks-gated": ("block", 3277, 32, "float32", 0.75),
    "vector-4096": ("1d", 1, 4096, "float32", 1.0),
}
GRAD_READS = {"2d": 3, "1d": 2, "block": 2}
LAUNCHES = {"2d": 4, "1d": 2, "block": 2}
KW = dict(lr=1e-3, decay=0.99, epsilon=1e-30, clip_thresh=1.0)


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


def _composed(torch, form, p, p16, g, cv, rv, mask):
    """The same arithmetic from torch operators, in place on p / cv / rv / p16."""
    lr, d, eps, clip = KW["lr"], KW["decay"], KW["epsilon"], KW["clip_thresh"]
    gf = g.float()
    s = gf * gf + eps
    if form == "1d":
        cv.mul_(d).add_(s, alpha=1 - d)
        x = gf * cv.rsqrt()
    else:
        rv.mul_(d).add_(s.mean(dim=-1), alpha=1 - d)
        cv.mul_(d).add_(s.mean(dim=-2), alpha=1 - d)
        m = rv.mean(dim=-1, keepdim=True)
        x = gf * ((rv / m).rsqrt().unsqueeze(-1) * cv.rsqrt().unsqueeze(-2))
    rate = lr / torch.clamp(x.square().mean().sqrt() / clip, min=1.0)
    p.sub_(rate * x)
    if mask is not None:
        p.mul_(mask)
    p16.copy_(p)


def run_case(name, window):
    import torch
    assert torch.cuda.is_available(), "bench_adafactor needs a ROCm device"
    from blocksparse_amd import adafactor_step, adam_step
    form, rows, second, gdt, live_frac = CASES[name]
    shape = {"2d": (rows, second), "1d": (second,), "block": (rows, second, second)}[form]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda scale: torch.randn(shape, device="cuda", generator=gen) * scale
    w, g = rnd(0.01), rnd(0.1).to(getattr(torch, gdt))
    gate = (torch.rand(rows, device="cuda", generator=gen) < live_frac).float() if form == "block" else None
    live = float(gate.mean()) if gate is not None else 1.0
    zeros = lambda *s: torch.zeros(s, device="cuda")
    slots = lambda: {"2d": (zeros(second), zeros(rows)), "1d": (zeros(second), None), "block": (zeros(rows, second), zeros(rows, second))}[form]
    p, p16, (cv, rv) = w.clone(), w.to(torch.bfloat16), slots()
    tp, tp16, (tcv, trv) = w.clone(), w.to(torch.bfloat16), slots()
    ap, ap16, am, av = w.clone(), w.to(torch.bfloat16), torch.zeros_like(w), torch.zeros_like(w)
    mask = gate.view(-1, 1, 1) if gate is not None else None
    t_ours, n1 = _time(torch, lambda: adafactor_step(p, g, cv, rv, gate=gate, param16=p16, **KW), window)
    t_comp, n2 = _time(torch, lambda: _composed(torch, form, tp, tp16, g, tcv, trv, mask), window)
    t_adam, n3 = _time(torch, lambda: adam_step(ap, g, am, av, 1e-3, gate=gate, param16=ap16), window)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(tp).all())
    n = w.numel()
    nbytes = (GRAD_READS[form] * g.element_size() + 4 + 4 + 2) * n * live
    return {"case": name, "form": form, "shape": "%s, %s gradient, %.0f %% live" % (" x ".join(str(s) for s in shape), gdt, 100 * live),
            "adafactor_us": t_ours * 1e6, "composed_us": t_comp * 1e6, "adam_us": t_adam * 1e6, "bytes": nbytes, "calls": [n1, n2, n3],
            "state_floats": (cv.numel() + (rv.numel() if rv is not None else 0)), "adam_state_floats": 2 * n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), help="run one tensor in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adafactor_bench.md"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one tensor's child process, seconds")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window)))
        return 0
    rows = []
    for name in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_adafactor: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    out = ["# Adafactor step: measured times (one MI355X)", "",
           "Written by `scripts/bench_adafactor.py`.  Call times from device events over windows of >= %.1f s after a warm-up, one process per" % a.window,
           "tensor, all three sides in that process.  `adafactor` = one `adafactor_step` with a bf16 working copy (its workspace allocation",
           "included); `composed` = the same arithmetic from torch operators, which touches every block whatever the gate; `adam` = `adam_step` on",
           "the same tensor.  Bytes: what the form must move per live element -- the gradient 3 / 2 / 2 times (2-d / 1-d / block form), param read",
           "and written, the 16-bit copy written; the ceiling is the measured device copy rate, %.2f TB/s.  Eager calls: the times include" % COPY_CEILING_TBS,
           "whatever the host adds when it cannot keep ahead of the device (2 to 4 launches and one allocation per call).  No figure is a pass",
           "condition.", "",
           "| tensor | launches | adafactor us | composed us | composed / adafactor | adam us | bytes | TB/s | of the %.2f TB/s ceiling | state floats (Adam's) |" % COPY_CEILING_TBS,
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        rate = r["bytes"] / (r["adafactor_us"] * 1e-6) / 1e12
        out.append("| %s | %d | %.1f | %.1f | %.2f | %.1f | %.1f MB | %.2f | %.0f %% | %d (%d) |" % (
            r["shape"], LAUNCHES[r["form"]], r["adafactor_us"], r["composed_us"], r["composed_us"] / r["adafactor_us"], r["adam_us"], r["bytes"] / 1e6,
            rate, 100.0 * rate / COPY_CEILING_TBS, r["state_floats"], r["adam_state_floats"]))
    out.append("")
    if os.path.exists(a.out):                                # a hand-kept "## Notes" section (per-launch times from a profiler run) survives a rewrite
        old = open(a.out).read()
        if "\n## Notes" in old:
            out.append(old[old.index("\n## Notes") + 1:].rstrip("\n"))
            out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
