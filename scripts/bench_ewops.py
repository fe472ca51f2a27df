"""Times the epilogue of a block-sparse layer -- bias -> activation -> dropout -> + residual, forward and backward -- in three forms and
writes a markdown table:

    python scripts/bench_ewops.py --out profiles/ewops_bench.md

  torch      what a user composes today: ``x + b``, the activation, ``F.dropout``, ``+ residual``; the backward is autograd's
  separate   this library's separate calls: ``bias_relu_fwd``, ``dropout`` (mask made and applied in one launch), a torch add;
             backward ``apply_dropout_mask`` on dy, then ``bias_relu_bwd``
  fused      ``bias_dropout_fwd`` with the residual (one launch) and ``bias_dropout_bwd`` (one launch and the sum of the partials)

Shape: the headline activation, 4096 features x 8192 samples, bf16, in both layouts, with ReLU and with fast-GELU.  Beside them a device copy
of one activation, timed in the same process: its rate (bytes read + written) is the yardstick.  Each case runs in a child process under a
time limit (``--case`` is the child's entry).  Times are device events around a window of calls that is at least ``--window`` seconds long,
after a warm-up; a measurement path that finds no GPU fails.  Bytes are algorithmic: with A = the bytes of one activation, the fused forward
moves 3 A + A / 16 (x and the residual read, y and the 1-bit mask written) and the fused backward the same (dy, x and the mask read, dx
written); the separate and torch forms are charged the same bytes, so their rate shows what the extra passes cost."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N, KEEP = 4096, 8192, 0.9
CASES = {"axis0-relu": (0, "relu"), "axis0-fast_gelu": (0, "fast_gelu"), "axis1-relu": (1, "relu"), "axis1-fast_gelu": (1, "fast_gelu")}


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
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "bench_ewops needs a ROCm device"
    from blocksparse_amd import ewops
    axis, act = CASES[name]
    kw = {act: True}
    shape = (K, N) if axis == 0 else (N, K)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda: torch.randn(shape, device="cuda", generator=gen).bfloat16()
    x, r, dy = rnd(), rnd(), rnd()
    b = torch.randn(K, device="cuda", generator=gen)
    bb = (b.view(K, 1) if axis == 0 else b).bfloat16()               # (torch adds the bias in the activation's type)
    ewops.set_entropy(1234)
    fn = (lambda z: torch.relu(z)) if act == "relu" else (lambda z: z * torch.sigmoid(1.702 * z))

    def torch_fwd(xx=x, bias=bb, res=r):
        return F.dropout(fn(xx + bias), 1.0 - KEEP, training=True) + res

    xr, br, rr = x.clone().requires_grad_(True), bb.clone().requires_grad_(True), r.clone().requires_grad_(True)
    ty = torch_fwd(xr, br, rr)

    def separate_fwd():
        y1 = ewops.bias_relu_fwd(x, b, axis=axis, **kw)
        y2, mask = ewops.bias_dropout_fwd(y1, None, KEEP, axis=axis)
        return y1, y2 + r, mask

    y1, _, mask = separate_fwd()
    kept = y1 if act == "relu" else x

    def separate_bwd():
        return ewops.bias_relu_bwd(ewops.apply_dropout_mask(dy, mask, KEEP), kept, b, axis=axis, **kw)

    copy_dst = torch.empty_like(x)
    t = {
        "copy": _time(torch, lambda: copy_dst.copy_(x), window),
        "torch_fwd": _time(torch, lambda: torch_fwd(), window),
        "separate_fwd": _time(torch, separate_fwd, window),
        "fused_fwd": _time(torch, lambda: ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, residual=r, **kw), window),
        "torch_bwd": _time(torch, lambda: torch.autograd.grad(ty, (xr, br, rr), dy, retain_graph=True), window),
        "separate_bwd": _time(torch, separate_bwd, window),
        "fused_bwd": _time(torch, lambda: ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, **kw), window),
    }
    # the three forms computed the same thing (each under its own mask): the kept share and the gradients' size agree
    fy, fmask = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, residual=r, **kw)
    share = float(ewops.unpack_mask(fmask.cpu().numpy(), x.numel()).mean())
    assert abs(share - KEEP) < 1e-3, share
    A = x.numel() * x.element_size()
    return {"case": name, "axis": axis, "act": act, "us": {k: v * 1e6 for k, v in t.items()}, "A": A, "fused_bytes": 3 * A + A // 16, "copy_bytes": 2 * A,
            "kept_share": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), help="run one case in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ewops_bench.md"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one case's child process, seconds")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window)))
        return 0
    rows = []
    for name in ("axis0-relu", "axis0-fast_gelu", "axis1-relu", "axis1-fast_gelu"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_ewops: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    tbs = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12
    out = ["# Layer epilogue (bias, activation, dropout, residual): measured times (one MI355X)", "",
           "Written by `scripts/bench_ewops.py`.  Activation %d features x %d samples, bf16 (A = %.0f MB), keep_prob %.1f.  Call times from device" % (
               K, N, rows[0]["A"] / 1e6, KEEP),
           "events over windows of >= %.1f s after a warm-up, one process per row, all forms in that process.  `torch` = `x + b`, the activation," % a.window,
           "`F.dropout`, `+ residual` and autograd's backward; `separate` = `bias_relu_fwd`, `dropout`, a torch add, and `apply_dropout_mask` +",
           "`bias_relu_bwd` backward; `fused` = `bias_dropout_fwd` / `bias_dropout_bwd`.  Every form is charged the fused form's algorithmic bytes,",
           "3 A + A / 16 = %.0f MB each way; `copy` is `dst.copy_(src)` of one activation (2 A) in the same process.  Eager calls: the times include" % (
               rows[0]["fused_bytes"] / 1e6),
           "whatever the host adds when it cannot keep ahead of the device.", "",
           "| layout, activation | pass | torch us | separate us | fused us | torch / fused | fused TB/s | copy us | copy TB/s | fused rate / copy rate |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us"]
        copy_rate = tbs(r["copy_bytes"], u["copy"])
        for p, label in (("fwd", "forward"), ("bwd", "backward")):
            rate = tbs(r["fused_bytes"], u["fused_" + p])
            out.append("| axis %d (%s), %s | %s | %.1f | %.1f | %.1f | %.2f | %.2f | %.1f | %.2f | %.0f %% |" % (
                r["axis"], "C, N" if r["axis"] == 0 else "N, C", r["act"], label, u["torch_" + p], u["separate_" + p], u["fused_" + p],
                u["torch_" + p] / u["fused_" + p], rate, u["copy"], copy_rate, 100.0 * rate / copy_rate))
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
