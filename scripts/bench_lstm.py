"""Times the fused LSTM gates -- the cell update between two matmuls of a recurrent model, forward and backward -- against the eager torch
composition and writes a markdown table:

    python scripts/bench_lstm.py --out profiles/lstm_bench.md

  torch      what a user composes without the operator: the bias add, ``sigmoid`` / ``tanh`` on the four slices of the gate tensor, the
             products and the sum; the backward is autograd's
  fused      ``fused_lstm_gates_fwd`` (one launch) and ``fused_lstm_gates_bwd`` (one launch; with a bias one more, the bias gradient
             ``bias_relu_bwd`` on the stored gate gradients)

Shape: the headline activation as c, 4096 cells x 8192 samples, bf16, in both layouts, the fused gate tensor with and without a bias.  Beside
them a device copy of one activation, timed in the same process: its rate (bytes read + written) is the yardstick.  Each case runs in a
child process under a time limit (``--case`` is the child's entry).  Times are device events around a window of calls that is at least
``--window`` seconds long, after a warm-up; a measurement path that finds no GPU fails.  Bytes are algorithmic: with A = the bytes of c, the
forward moves 7 A (c and four gates read, c_next and h_next written) and the backward 12 A (c, four gates, eh, ec read, dc and four gate
gradients written); with a bias the backward is charged 4 A more, the gate gradients read again for db.  The torch form is charged the same
bytes, so its rate shows what the extra passes cost."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N, FB = 4096, 8192, 1.0
CASES = {"axis0": (0, False), "axis0-bias": (0, True), "axis1": (1, False), "axis1-bias": (1, True)}


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
    assert torch.cuda.is_available(), "bench_lstm needs a ROCm device"
    from blocksparse_amd import ewops, lstm
    axis, with_bias = CASES[name]
    ax = 0 if axis == 0 else -1
    shape, hshape = ((K, N), (4 * K, N)) if axis == 0 else ((N, K), (N, 4 * K))
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda s: torch.randn(s, device="cuda", generator=gen).bfloat16()
    c, h, eh, ec = rnd(shape), rnd(hshape), rnd(shape), rnd(shape)
    b = torch.randn(4 * K, device="cuda", generator=gen) if with_bias else None
    bb = None if b is None else (b.view(4 * K, 1) if axis == 0 else b).bfloat16()     # (torch adds the bias in the activation's type)

    def torch_fwd(cc=c, hh=h, bias=bb):
        i, u, f, o = torch.chunk(hh if bias is None else hh + bias, 4, dim=ax)
        cn = torch.sigmoid(f + FB) * cc + torch.sigmoid(i) * torch.tanh(u)
        return cn, torch.sigmoid(o) * torch.tanh(cn)

    leaves = [c.clone().requires_grad_(True), h.clone().requires_grad_(True)] + ([] if bb is None else [bb.clone().requires_grad_(True)])
    tcn, thn = torch_fwd(*leaves)

    def fused_bwd():
        dc, dh = lstm.fused_lstm_gates_bwd(c, h, eh=eh, ec=ec, bias=b, forget_bias=FB, axis=ax)
        return dc, dh, (ewops.bias_relu_bwd(dh, None, b, axis=ax)[1] if with_bias else None)

    copy_dst = torch.empty_like(c)
    t = {
        "copy": _time(torch, lambda: copy_dst.copy_(c), window),
        "torch_fwd": _time(torch, lambda: torch_fwd(), window),
        "fused_fwd": _time(torch, lambda: lstm.fused_lstm_gates_fwd(c, h, bias=b, forget_bias=FB, axis=ax), window),
        "torch_bwd": _time(torch, lambda: torch.autograd.grad((tcn, thn), leaves, (ec, eh), retain_graph=True), window),
        "fused_bwd": _time(torch, fused_bwd, window),
    }
    # both forms computed the same thing: the L2-relative difference of h_next and of dc
    fcn, fhn = lstm.fused_lstm_gates_fwd(c, h, bias=b, forget_bias=FB, axis=ax)
    tdc = torch.autograd.grad((tcn, thn), leaves, (ec, eh), retain_graph=True)[0]
    diff = lambda p, q: float((p.float() - q.float()).norm() / q.float().norm())
    agree = {"h_next": diff(fhn, thn.detach()), "dc": diff(fused_bwd()[0], tdc)}
    assert max(agree.values()) < 0.05, agree            # (the torch form rounds every intermediate to bf16)
    A = c.numel() * c.element_size()
    return {"case": name, "axis": axis, "bias": with_bias, "us": {k: v * 1e6 for k, v in t.items()}, "A": A, "fwd_bytes": 7 * A,
            "bwd_bytes": (16 if with_bias else 12) * A, "copy_bytes": 2 * A, "agree": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), help="run one case in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_bench.md"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per measurement")
    ap.add_argument("--timeout", type=int, default=150, help="time limit of one case's child process, seconds")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.window)))
        return 0
    rows = []
    for name in ("axis0", "axis0-bias", "axis1", "axis1-bias"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--window", str(a.window)], capture_output=True, text=True,
                           timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print("bench_lstm: %s failed with exit code %d; stopping" % (name, r.returncode))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(line[0])
    tbs = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12
    out = ["# Fused LSTM gates: measured times (one MI355X)", "",
           "Written by `scripts/bench_lstm.py`.  c = %d cells x %d samples, bf16 (A = %.0f MB), the fused gate tensor of 4 A, forget_bias %.1f.  Call" % (
               K, N, rows[0]["A"] / 1e6, FB),
           "times from device events over windows of >= %.1f s after a warm-up, one process per row pair, both forms in that process.  `torch` =" % a.window,
           "the bias add, `sigmoid` / `tanh` on the four slices, the products and the sum, and autograd's backward; `fused` =",
           "`fused_lstm_gates_fwd` / `fused_lstm_gates_bwd` (with a bias: plus `bias_relu_bwd` for db, a second launch).  Both forms are charged the",
           "fused form's algorithmic bytes: 7 A forward, 12 A backward (16 A with a bias: the gate gradients are read again for db); `copy` is",
           "`dst.copy_(src)` of one activation (2 A) in the same process.  Eager calls: the times include whatever the host adds when it cannot",
           "keep ahead of the device.", "",
           "| layout, bias | pass | MB moved | torch us | fused us | torch / fused | fused TB/s | copy us | copy TB/s | fused rate / copy rate |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        u = r["us"]
        copy_rate = tbs(r["copy_bytes"], u["copy"])
        for p, label in (("fwd", "forward"), ("bwd", "backward")):
            rate = tbs(r[p + "_bytes"], u["fused_" + p])
            out.append("| axis %d (%s), %s | %s | %.0f | %.1f | %.1f | %.2f | %.2f | %.1f | %.2f | %.0f %% |" % (
                r["axis"], "K, N" if r["axis"] == 0 else "N, K", "bias" if r["bias"] else "no bias", label, r[p + "_bytes"] / 1e6, u["torch_" + p],
                u["fused_" + p], u["torch_" + p] / u["fused_" + p], rate, u["copy"], copy_rate, 100.0 * rate / copy_rate))
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote " + a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
