#!/usr/bin/env python
"""bench.py -- block-sparse matmul hot path on MI355X: effective TFLOP/s (+ GB/s, roofline, CPU baseline).

    python bench.py [--gpus N --steps K --warmup W] [--config headline|cfg2|cfg3] [--dump-outputs DIR] [--full]

A plain run sets up the timed workload, warms it up, times K steps and prints one JSON line (`value` = effective TFLOP/s,
`ms_per_step` = milliseconds of one timed step).  `--full` adds everything else the line can carry: the CPU baseline, the other
densities, configurations and precisions, the attention operators, the sampled parity check against the oracle and, on more than
one rank, the gradient reduction timed on its own.  `--dump-outputs DIR` writes what the last timed step computed (see dump_outputs).

`--gpus N` with N > 1 spawns the N ranks itself (re-exec under torch.distributed.run, one process per GPU, rendezvous on
127.0.0.1) unless it already runs under a launcher (WORLD_SIZE set), so both `python bench.py --gpus 8` and the driver's
`python -m torch.distributed.run --nproc-per-node 8 bench.py --gpus 8` give the same 8-rank run.

Workloads
  headline (BASELINE.json metric): bsmm 4096x4096 bs=32 @ {10, 20, 50} % density, bf16 storage / fp32 accumulate, one STEP =
      fprop + bprop + updat of a minibatch of 8192 rows per GPU (weak scaling).  `value` is the 20 % figure; the three
      densities sit side by side in "densities".  On one GPU the default line also carries BASELINE configs[2] ("cfg2"),
      configs[3] on one GPU ("cfg3"), configs[1] ("fp32_fprop_axis1") and configs[4] ("attention").
  cfg2 (BASELINE configs[2]): 4096x4096 bs=16 feature_axis=0 @ 10 %, bf16, minibatch 8192 per GPU.
  cfg3 (BASELINE configs[3]): 8192x8192 bs=32 @ 5 %, GLOBAL minibatch 4096 sharded over the ranks (strong scaling; the
      N = 1 line is the whole minibatch on one GPU).
Multi-GPU = data parallel: tables and W replicated, minibatch sharded, the weight gradient reduced once per step by the LIBRARY's
own RCCL communicator (include/bsmm_dist.h: reduce-scatter of the fp32 sums, finalize of 1 / world of the blocks per rank,
all-gather of the finished shards) on a side stream, overlapped with bprop AND the next step's fprop; torch.distributed (gloo)
only carries the bootstrap id, the barriers and the max-over-ranks of the timings.  Synthetic inputs are resident in HBM before
the timed region.  Effective FLOPs per pass = 2 * blocks * bs^2 * N (nonzero blocks only; the reference's own definition,
src/gpu_types.cc:48, src/blocksparse_matmul_op.cc:102,182).
The CPU legs run FIRST, the GPU legs to the end of the process.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3}   # dense TFLOP/s, MI355X_MICROARCH.md
PEAK_HBM = 8000.0                                            # GB/s (spec)
PROFILE_ROUND = "r06"
CLOCK_GHZ = 2.4                                              # nominal shader clock the per-clock figures are quoted at
L2_TO_LDS_CEILING = 52.0                                     # B/clk/CU: the L2-resident LDS-DMA streaming micro-benchmark (scripts/micro/l2_bw.hip)


def ba_layout(n, m, seed):
    """Barabasi-Albert adjacency + I (the reference's own bench layout, test/blocksparse_matmul_bench.py:66-68; same generator as
    tests/_parity.py, without networkx)"""
    rng = np.random.RandomState(seed)
    lay = np.eye(n, dtype=np.int32)
    targets = list(range(m))
    repeated = []
    for src in range(m, n):
        for t in set(targets):
            lay[src, t] = lay[t, src] = 1
        repeated.extend(targets)
        repeated.extend([src] * m)
        targets = []
        while len(targets) < m:
            x = repeated[rng.randint(len(repeated))]
            if x not in targets:
                targets.append(x)
    lay[:m, :m] = 1
    return lay


def delivery_roof(layout, bsize, N, kernel_ms, cus):
    """The roof DESIGN.md argues is binding for the bsize-32 xprop kernels: bytes one pass moves through the L2 -> LDS path (every
    (row tile of 128, group of 16 output blocks) unit stages the 16 KiB slab of each input-block pair its group touches and the 2 KiB of
    each of its weight blocks), per clock and CU, against the L2-resident LDS-DMA streaming rate measured on this part."""
    if bsize != 32:
        return None
    lay = np.asarray(layout) != 0
    CB, KB = lay.shape
    tiles = (N + 127) // 128
    per_tile = 0
    for g0 in range(0, KB, 16):
        sub = lay[:, g0:g0 + 16]
        rows = np.nonzero(sub.any(axis=1))[0]
        per_tile += len(set((rows // 2).tolist())) * 16384 + int(sub.sum()) * 2048
    byts = tiles * per_tile
    rate = byts / (kernel_ms * 1e-3 * CLOCK_GHZ * 1e9 * cus)
    return {"bytes_l2_to_lds": int(byts), "b_per_clk_per_cu": round(rate, 2), "ceiling_b_per_clk": L2_TO_LDS_CEILING, "frac": round(rate / L2_TO_LDS_CEILING, 4),
            "clock_ghz": CLOCK_GHZ, "kernel": "bsmm_xprop(fprop)", "note": "analytic bytes of the plan (slabs + weight blocks per unit) / HIP-event time of the pass"}


def delivery_roof_updat(plan_host, N, kernel_ms, cus, kernel_code=None):
    """The same for the weight gradient.  Streaming kernel ('BSU2' plan: header word 2 = window side in blocks, word 4 = work items): every
    item stages, per minibatch row, one row piece of the window's X features and one of its DY features (window side x 64 B each).
    bsize 16 ('BSUP' plan): the windowed kernel's items stage 256 + 256 feature rows per minibatch entry; when the call ran the row-owner
    kernel (kernel_code = K_UPDAT16_ROWS: the 'BSU6' section behind the items, header word 8) a window is 512 X features, read straight into
    registers, and 16 WK DY features through LDS -- both counted, both come through the same L2 -> CU path."""
    if plan_host is None:
        return None
    magic = int(plan_host[0])
    if magic == 0x42535532:
        ws, items = int(plan_host[2]), int(plan_host[4])
        byts = items * N * ws * 64 * 2
        what = {"window_side_blocks": ws, "items": items}
    elif magic == 0x42535550 and int(plan_host[2]) == 16:
        off = int(plan_host[8])
        if kernel_code == 23 and off > 0:
            wk, items = int(plan_host[off + 3]), int(plan_host[off + 4])
            byts = items * N * (32 * 16 + wk * 16) * 2
            what = {"window_features": [512, 16 * wk], "items": items, "kernel_family": "row-owner (X rows straight into registers)"}
        else:
            isz = 4 + int(plan_host[7]) * int(plan_host[3]) * 2
            live = int((np.asarray(plan_host[int(plan_host[6]):int(plan_host[6]) + int(plan_host[4]) * isz]).reshape(-1, isz)[:, 2] & 0xffff > 0).sum())
            byts = live * N * (256 + 256) * 2
            what = {"window_features": [256, 256], "items": live, "kernel_family": "windowed"}
    else:
        return None
    rate = byts / (kernel_ms * 1e-3 * CLOCK_GHZ * 1e9 * cus)
    out = {"bytes_l2_to_cu": int(byts), "b_per_clk_per_cu": round(rate, 2), "ceiling_b_per_clk": L2_TO_LDS_CEILING, "frac": round(rate / L2_TO_LDS_CEILING, 4),
           "clock_ghz": CLOCK_GHZ, "kernel": "bsmm_updat",
           "note": "analytic bytes of the plan (X and DY rows of every work item over the whole minibatch; the time includes the summing pass)"}
    out.update(what)
    return out


def random_layout(CB, KB, density, seed):
    """rng.random < density with at least one block per row and column (same generator as tests/_parity.py)."""
    rng = np.random.default_rng(seed)
    lay = (rng.random((CB, KB)) < density).astype(np.int32)
    for r in np.nonzero(lay.sum(axis=1) == 0)[0]:
        lay[r, rng.integers(0, KB)] = 1
    for c in np.nonzero(lay.sum(axis=0) == 0)[0]:
        lay[rng.integers(0, CB), c] = 1
    return lay


DUMP_BYTES = 60 * 10 ** 6          # --dump-outputs writes at most this much array data in all


def dump_outputs(d, named, budget=DUMP_BYTES):
    """Write each tensor of `named` ({name: tensor}) as d/<name>.npy in float32.  A tensor larger than its share of `budget` is
    written as a fixed sample of its leading-axis slices (sorted indices drawn by default_rng(0)), so two runs with the same
    arguments write the same elements."""
    os.makedirs(d, exist_ok=True)
    share = budget // len(named)
    for name, t in named.items():
        t = t.detach()
        if t.numel() * 4 > share:
            if t.dim() < 2 or t[0].numel() * 4 > share:
                t = t.reshape(-1)
            k = max(1, share // (t[0].numel() * 4))
            idx = np.sort(np.random.default_rng(0).choice(t.shape[0], k, replace=False))
            t = t[idx.tolist()]
        np.save(os.path.join(d, name + ".npy"), t.float().cpu().numpy())


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200, help="timed steps")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--config", default="headline", choices=["headline", "cfg2", "cfg3"])
    p.add_argument("--prewarm-seconds", type=float, default=0.5,
                   help="untimed steps run for this long before the warmup steps: the GPU needs a few hundred ms of sustained load "
                        "to reach its boost clock")
    p.add_argument("--hidden", type=int, default=None)
    p.add_argument("--bsize", type=int, default=None)
    p.add_argument("--density", type=float, default=None, help="headline density (default 0.2; cfg3: 0.05)")
    p.add_argument("--axis", type=int, default=None)
    p.add_argument("--dtype", default=None, choices=["bf16", "f16", "f32"])
    p.add_argument("--n-local", type=int, default=None, help="minibatch rows per GPU (headline; default 8192)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-seconds", type=float, default=6.0)
    p.add_argument("--no-attention", action="store_true", help="skip the BASELINE configs[4] (block-sparse attention) extra")
    p.add_argument("--no-densities", action="store_true", help="skip the 10 %% / 50 %% runs of the headline metric")
    p.add_argument("--no-extras", action="store_true", help="with --full: the headline line only (no fp32 / attention / other densities / CPU baseline)")
    p.add_argument("--master-port", type=int, default=29533)
    p.add_argument("--full", action="store_true",
                   help="also run the CPU baseline, the other densities / configurations / precisions, the attention operators, the parity "
                        "check against the oracle and the gradient reduction on its own (a plain run times the headline workload only)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write y (fprop), dx (bprop) and dw (updat) of the last timed step as DIR/<name>.npy "
                        "(float32; larger outputs as a fixed, seeded sample of rows, %d MB at most in all)" % (DUMP_BYTES // 10 ** 6))
    a = p.parse_args()
    if a.steps < 1:
        p.error("--steps must be at least 1")
    a.bsize_given, a.axis_given, a.dtype_given = a.bsize is not None, a.axis is not None, a.dtype is not None
    return a


def respawn_under_launcher(a):
    """`python bench.py --gpus N` outside a launcher: become N ranks (one per GPU) of one node."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(a.master_port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env)
    sys.exit(r.returncode)


def alg_bytes_xprop(b, N, s):
    segs = b._dev_tables["fprop"]["segments"]
    return s * (b.C * N + b.K * N + b.blocks * b.bsize ** 2) + 4 * (4 * segs + 2 * b.blocks)


def alg_bytes_updat(b, N, s):
    return s * (b.C * N + b.K * N) + s * b.blocks * b.bsize ** 2 + 8 * b.blocks


def roofline_of(dom, d_ms, d_flops, d_bytes, dtype):
    ai = d_flops / d_bytes
    ridge = PEAK_MFMA[dtype] * 1e12 / (PEAK_HBM * 1e9)
    if ai >= ridge:
        roof = {"bound": "mfma", "achieved": round(d_flops / (d_ms * 1e-3) / 1e12, 2), "peak": PEAK_MFMA[dtype], "unit": "TFLOP/s"}
    else:
        roof = {"bound": "hbm", "achieved": round(d_bytes / (d_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM, "unit": "GB/s"}
    roof["frac"] = round(roof["achieved"] / roof["peak"], 4)
    roof["traffic"] = None
    roof["kernel"] = dom
    roof["kernel_ms"] = round(d_ms, 4)
    roof["arithmetic_intensity"] = round(ai, 1)
    return roof


def attention_extra(a):
    """BASELINE configs[4]: block-sparse attention, batch 4, 16 heads x 64, ctx 4096, bsize 32, local(4)+strided(8) causal
    layout (1466 blocks per head), fp32 activations / bf16 scores (the reference's fp32 pathway).  Reported per op:
    ms, effective TFLOP/s (2 * blocks * 32 * 32 * 64 per head and batch entry), algorithmic GB/s, and the bound of the arithmetic the kernel
    actually runs: the fp32 products are computed as six bf16 piece products on the 16-bit matrix core, so the bound is
    max(6 * flops / 2.5 PF, algorithmic bytes / 8 TB/s) -- HBM for every operator here (the fp32-MFMA peak these lines were
    priced against in rounds 3-5 is not the instruction that runs).  `nt_softmax_fused` (round 6) is scores + softmax as one launch: the raw
    scores never reach memory; `nt_softmax_grad_fused` the backward pair (scores of (dy, v) + softmax gradient).  `fwd_ms` / `fwd_bwd_ms` use them
    (BlocksparseTransformer.attention), `fwd_ms_two_launches` / `fwd_bwd_ms_composed_backward` are the composed forms.
    CPU baseline: the oracle (NumPy, fp32) on one batch entry and two heads."""
    import torch
    from blocksparse_amd import BlocksparseTransformer
    B, H, HS, BS, CTX = 4, 16, 64, 32, 128
    qi, ki = np.indices((CTX, CTX))
    lay = ((ki <= qi) & ((qi - ki < 4) | ((qi - ki) % 8 == 0))).astype(np.int32)      # local 4 blocks + every 8th, causal

    def causal(blk_shape, head, q, k, b):                                            # diagonal blocks: lower triangle
        m = np.ones(blk_shape, dtype=bool)
        return np.tril(m) if q == k else m

    bst = BlocksparseTransformer(lay, block_size=BS, heads=H, mask_callback=causal)
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.rand(B, CTX * BS, H * HS, device="cuda", generator=g) * 2 - 1 for _ in range(3))
    sd = torch.bfloat16
    mask = bst._table("mask", "cuda")
    scale = 1.0 / np.sqrt(HS)
    w = bst._nt(q, k, sd)
    p = bst._softmax_fwd(w, scale, mask, sd)
    dp = torch.randn(p.shape, device="cuda", generator=g).to(sd)

    def timeit(fn, reps=100):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    flops = 2.0 * B * H * bst.blocks * BS * BS * HS
    sbytes = B * H * bst.blocks * BS * BS * 2
    abytes = q.numel() * 4
    assert bst._nt_softmax(q, k, scale, mask, sd) is not None, "configs[4] is what the fused kernel is for"
    ops = [("nt", lambda: bst._nt(q, k, sd), flops, 2 * abytes + sbytes),
           ("nt_softmax_fused", lambda: bst._nt_softmax(q, k, scale, mask, sd), flops, 2 * abytes + sbytes),
           ("masked_softmax", lambda: bst._softmax_fwd(w, scale, mask, sd), 0.0, 2 * sbytes),
           ("nn", lambda: bst._xn(p, v, False), flops, 2 * abytes + sbytes),
           ("tn", lambda: bst._xn(p, q, True), flops, 2 * abytes + sbytes),
           ("softmax_grad", lambda: bst._softmax_bwd(dp, p, scale), 0.0, 3 * sbytes),
           ("nt_softmax_grad_fused", lambda: bst._nt_softmax_grad(q, v, p, scale), flops, 2 * abytes + 2 * sbytes)]
    res = {}
    for name, fn, fl, by in ops:
        ms = timeit(fn)
        t_mfma, t_hbm = 6.0 * fl / (PEAK_MFMA["bf16"] * 1e12), by / (PEAK_HBM * 1e9)     # six bf16 piece products per fp32 product
        bound = max(t_mfma, t_hbm) * 1e3
        res[name] = {"ms": round(ms, 4), "tflops": round(fl / ms / 1e9, 2), "gbps": round(by / ms / 1e6, 1),
                     "bound": "mfma" if t_mfma > t_hbm else "hbm", "bound_ms": round(bound, 4), "frac": round(bound / ms, 4)}
    # forward + backward of one attention layer = [nt + softmax] (one launch), nn | tn(dv), nt(dp), softmax_grad, nn(dq), tn(dk)
    fwd2 = res["nt"]["ms"] + res["masked_softmax"]["ms"] + res["nn"]["ms"]
    fwd = res["nt_softmax_fused"]["ms"] + res["nn"]["ms"]
    fb2 = fwd + res["nt"]["ms"] + res["softmax_grad"]["ms"] + res["nn"]["ms"] + res["tn"]["ms"] * 2
    fb = fwd + res["nt_softmax_grad_fused"]["ms"] + res["nn"]["ms"] + res["tn"]["ms"] * 2
    # the same operators with bf16 activations (native 16-bit MFMA, HBM-bound): not the BASELINE configuration, for reference
    qb, kb, vb = q.bfloat16(), k.bfloat16(), v.bfloat16()
    res16 = {}
    for name, fn in (("nt", lambda: bst._nt(qb, kb, sd)), ("nt_softmax_fused", lambda: bst._nt_softmax(qb, kb, scale, mask, sd)),
                     ("nn", lambda: bst._xn(p, vb, False)), ("tn", lambda: bst._xn(p, qb, True))):
        ms = timeit(fn)
        by = 2 * qb.numel() * 2 + sbytes
        res16[name] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 2), "gbps": round(by / ms / 1e6, 1), "bound": "hbm",
                       "bound_ms": round(by / (PEAK_HBM * 1e9) * 1e3, 4), "frac": round(by / (PEAK_HBM * 1e9) * 1e3 / ms, 4)}
    out = {"workload": "BASELINE configs[4]: block-sparse attention batch %d heads %d x %d ctx %d bsize %d, %d blocks/head, fp32 activations, bf16 scores"
                       % (B, H, HS, CTX * BS, BS, bst.blocks),
           "ops": res, "fwd_ms": round(fwd, 4), "fwd_ms_two_launches": round(fwd2, 4), "fwd_bwd_ms": round(fb, 4), "fwd_bwd_ms_composed_backward": round(fb2, 4),
           "fwd_bwd_tflops": round(6 * flops / fb / 1e9, 2), "ops_bf16_activations": res16}
    if not a.no_cpu_baseline:
        from oracle import bst_oracle as O            # the oracle is only the timed CPU baseline here
        L = O.build_luts(lay)
        qc, kc, vc = (t[:1, :, :2 * HS].float().cpu().numpy() for t in (q, k, v))
        t0 = time.perf_counter()
        W = O.nt(L, qc, kc, BS, 2)
        P = O.masked_softmax(L, W, BS, scale, bst.softmax_mask_np)
        O.nn(L, P, vc, BS, 2)
        el = time.perf_counter() - t0
        fl_s = 2 * 2.0 * 2 * bst.blocks * BS * BS * HS          # nt + nn of 1 batch entry x 2 heads
        out["cpu_baseline"] = {"value": round(fl_s / el / 1e9, 3), "unit": "GFLOP/s (nt + softmax + nn, forward)", "cores": 1, "kind": "port",
                               "sample": "1 of 4 batch entries, 2 of 16 heads, float64 NumPy oracle, %.2f s" % el}
    return out


def blas_threads():
    try:
        from threadpoolctl import threadpool_info
        info = threadpool_info()
        return int(max([i.get("num_threads", 1) for i in info] or [os.cpu_count()])), ",".join(sorted(set(i.get("internal_api", "?") for i in info)))
    except Exception:
        return int(os.cpu_count() or 1), "?"


def cpu_baseline(layout, bs, axis, N, seconds):
    """The CPU baseline north_star names: NumPy fp32 DENSE-EQUIVALENT of the three passes on the host cores -- fprop X @ Wd,
    bprop DY @ Wd^T, updat X^T @ DY (dense, then block gather) with Wd = to_dense(W) -- at the headline minibatch, all BLAS
    threads, bounded to `seconds`.  `value` counts only the nonzero-block FLOPs (the same definition as the GPU line), the
    dense rate is given next to it; the oracle's gathered-block port (work-efficient, batched small GEMMs) is a second field."""
    from oracle import bsmm_oracle as orc
    t = orc.build_layout_luts(layout, bs)
    rng = np.random.default_rng(0)
    CB, KB = layout.shape
    C, K = CB * bs, KB * bs
    W = rng.normal(0, 0.01, (t["blocks"], bs, bs)).astype(np.float32)
    X = rng.normal(0, 0.1, (N, C) if axis else (C, N)).astype(np.float32)
    E = rng.normal(0, 0.1, (N, K) if axis else (K, N)).astype(np.float32)
    Wd = np.ascontiguousarray(orc.to_dense(t, W).astype(np.float32))
    ul = t["updat_lut"]

    def dense_step():
        if axis:
            y = X @ Wd
            dx = E @ Wd.T
            dwd = X.T @ E
        else:
            y = Wd.T @ X
            dx = Wd @ E
            dwd = X @ E.T
        dw = dwd.reshape(CB, bs, KB, bs).transpose(0, 2, 1, 3)[ul[:, 0], ul[:, 1]]
        return y, dx, dw

    dense_step()                                        # warm up BLAS threads
    t0 = time.perf_counter()
    steps, times = 0, []
    while True:
        t1 = time.perf_counter()
        dense_step()
        times.append(time.perf_counter() - t1)
        steps += 1
        if time.perf_counter() - t0 >= seconds * 0.75 or steps >= 30:
            break
    med = float(np.median(times))
    dense_flops = 3 * 2.0 * C * K * N
    eff_flops = 3 * 2.0 * t["blocks"] * bs * bs * N
    threads, api = blas_threads()
    out = {"value": round(eff_flops / med / 1e12, 4), "unit": "TFLOP/s", "cores": threads, "kind": "port",
           "sample": "NumPy fp32 dense-equivalent (X @ to_dense(W), DY @ Wd^T, X^T @ DY + block gather), same layout, minibatch %d, "
                     "median of %d steps of fprop+bprop+updat (%.2f s each), %d BLAS threads (%s) on %d host cores"
                     % (N, steps, med, threads, api, os.cpu_count() or 0),
           "dense_tflops": round(dense_flops / med / 1e12, 4), "host_cores": int(os.cpu_count() or 0)}
    # second figure: the oracle's gathered-block port (only nonzero blocks are multiplied), smaller minibatch sample
    Ns = min(N, 1024)
    Xs, Es = (X[:Ns], E[:Ns]) if axis else (X[:, :Ns], E[:, :Ns])
    Xs, Es = np.ascontiguousarray(Xs), np.ascontiguousarray(Es)
    orc.fprop_fast(t, Xs, W, axis)
    t0 = time.perf_counter()
    reps = 0
    while True:
        orc.fprop_fast(t, Xs, W, axis)
        orc.bprop_fast(t, Es, W, axis)
        orc.updat_fast(t, Xs, Es, axis)
        reps += 1
        if time.perf_counter() - t0 >= seconds * 0.25 or reps >= 20:
            break
    el = time.perf_counter() - t0
    out["gathered_blocks_port"] = {"value": round(3 * 2.0 * t["blocks"] * bs * bs * Ns * reps / el / 1e12, 4), "unit": "TFLOP/s",
                                   "sample": "oracle *_fast (batched BLAS over gathered blocks), minibatch %d, %d steps in %.1f s" % (Ns, reps, el)}
    return out


def parity_check(torch, b, layout, w, x, dy, dtype):
    """One sampled-block check of what was just timed, against the float64 oracle (tests/ hold the full parity suite)."""
    from oracle import bsmm_oracle as orc
    t = orc.build_layout_luts(layout, b.bsize)
    bs, axis = b.bsize, b.axis
    W, X, E = (v.float().cpu().numpy() for v in (w, x, dy))
    y, dx, dw = (v.float().cpu().numpy() for v in (b.fprop(x, w), b.bprop(dy, w), b.updat(x, dy)))
    worst = 0.0

    def blk(a, i):
        return a[:, i * bs:(i + 1) * bs] if axis else a[i * bs:(i + 1) * bs, :]

    def l2(got, ref):
        ref = orc.round_to(ref, dtype)
        return float(np.linalg.norm(got.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))
    ks = [0, b.KB // 3 + 1, b.KB - 1]
    for k, ref in orc.fprop_cols(t, X, W, axis, ks).items():
        worst = max(worst, l2(blk(y, k), ref))
    cs = [1, b.CB // 2, b.CB - 2]
    for c, ref in orc.bprop_rows(t, E, W, axis, cs).items():
        worst = max(worst, l2(blk(dx, c), ref))
    ws = list(range(0, b.blocks, max(1, b.blocks // 16)))[:16]
    for i, ref in orc.updat_blocks(t, X, E, axis, ws).items():
        worst = max(worst, l2(dw[i], ref))
    bar = 2e-6 if dtype == "f32" else 1e-3
    return {"parity_checked": bool(worst <= bar), "parity_worst_l2": float("%.3e" % worst), "parity_bar": bar,
            "parity_sample": "fprop 3 block columns, bprop 3 block rows, updat 16 blocks vs oracle/bsmm_oracle.py (float64)"}


CONFIGS = {
    # name: (hidden, bsize, axis, density, dtype, minibatch per GPU or None = global 4096 split over the ranks)
    "headline": (4096, 32, 1, 0.20, "bf16", 8192),     # BASELINE.json metric: 4096^2 bs 32 @ 20 % (10 / 50 % ride along)
    "cfg2": (4096, 16, 0, 0.10, "bf16", 8192),         # BASELINE configs[2]
    "cfg3": (8192, 32, 1, 0.05, "bf16", None),         # BASELINE configs[3]: global minibatch 4096, strong scaling
}


def git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip() or None
    except Exception:
        return None


def kernel_sources_digest():
    """sha256 over the kernel sources the profiled numbers depend on (the GPU box has no .git: this is what ties a counters file to a tree)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "blocksparse_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip")):
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def measured_counters():
    """per-workload MFMA busy / measured HBM GB/s / HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/), USED ONLY when
    the file was taken on this tree's kernels: scripts/make_counters_json.py stamps the digest of blocksparse_amd/csrc and the profiled
    kernel names; a mismatch drops the block and says why."""
    try:
        c = json.load(open(os.path.join(ROOT, "profiles", PROFILE_ROUND + "_counters.json")))
    except Exception:
        return {}, "no profiles/%s_counters.json" % PROFILE_ROUND
    stamp = c.get("_stamp", {})
    if stamp.get("csrc_digest") != kernel_sources_digest():
        return {}, "profiles/%s_counters.json was taken on other kernel sources (digest %s, tree %s): not quoted" % (PROFILE_ROUND, stamp.get("csrc_digest"), kernel_sources_digest())
    return c, None


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_launcher(a)
    import torch
    import torch.distributed as dist
    from blocksparse_amd import BlocksparseMatMul, _lib
    from blocksparse_amd.dist import DwReduce, DwAllReduce

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs a ROCm device"
    if a.gpus != world and rank == 0:
        print("bench.py: --gpus %d but the launcher started %d ranks; reporting n_gpus = %d" % (a.gpus, world, world), file=sys.stderr)
    torch.cuda.set_device(local)
    force_dist = os.environ.get("BSMM_FORCE_DIST") == "1"             # run the RCCL path at world size 1 (self-test)
    use_dist = world > 1 or force_dist
    if world > 1:
        # gloo carries the bootstrap (the 128-byte RCCL id), the barriers and the max-over-ranks of the timings; the ONLY RCCL
        # instance on the devices is the library's own communicator (include/bsmm_dist.h), which moves the gradients
        dist.init_process_group("gloo")
    _lib.load()

    def barrier():
        if world > 1:
            dist.barrier()

    if a.no_extras or not a.full:
        a.no_densities = a.no_attention = a.no_cpu_baseline = a.no_extras = True
    td_of = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

    # ---- CPU legs first: the GPU legs then run to the end of the process (a utilisation sampler next to this run sees them) ----
    cpu_out = None
    hidden0, bsize0, axis0, dens0, dtype0, nloc0 = CONFIGS[a.config]
    hidden0 = a.hidden or hidden0
    bsize0 = a.bsize if a.bsize_given else bsize0
    axis0 = a.axis if a.axis_given else axis0
    dens0 = a.density if a.density is not None else dens0
    dtype0 = a.dtype if a.dtype_given else dtype0
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        n_cpu = min(a.n_local or nloc0 or 4096, 8192)
        cpu_out = cpu_baseline(random_layout(hidden0 // bsize0, hidden0 // bsize0, dens0, seed=1234), bsize0, axis0, n_cpu, a.cpu_seconds)

    def setup(hidden, bsize, axis, dens, dtype, n_local):
        td = td_of[dtype]
        CB = hidden // bsize
        layout = random_layout(CB, CB, dens, seed=1234)
        b = BlocksparseMatMul(layout, block_size=bsize, feature_axis=axis)
        g = torch.Generator(device="cuda").manual_seed(1 + rank)
        w = (torch.randn(b.w_shape, device="cuda", generator=g) * 0.01).to(td)
        x = (torch.randn(b.i_shape(n_local), device="cuda", generator=g) * 0.1).to(td)
        dy = (torch.randn(b.o_shape(n_local), device="cuda", generator=g) * 0.1).to(td)
        return layout, b, w, x, dy

    def run(b, w, x, dy, steps, warmup, prewarm):
        """(seconds for `steps` steps [max over ranks], mean ms of fprop / updat / bprop from HIP events on the launch stream).
        Data-parallel step: fprop | wait for the PREVIOUS step's dw | updat -> raw fp32 sums | start their reduction (library RCCL
        handle, side stream) | bprop -- the reduction of step i overlaps with bprop(i) and fprop(i + 1); dw is not needed before the
        optimiser, which would sit where the wait is."""
        td = w.dtype
        fused = use_dist and b.bsize == 32 and b.axis == 1 and td != torch.float32   # the streaming updat kernel hands over fp32 sums
        dws = [torch.empty(b.w_shape, dtype=td, device="cuda") for _ in range(2)]
        red = DwReduce(b, force=use_dist) if fused else DwAllReduce(accumulate_fp32=True, force=use_dist)
        state = {"i": 0, "pending": False}

        def step(ev=None):
            i = state["i"]
            if ev: ev[0].record()
            y = b.fprop(x, w)
            if ev: ev[1].record()
            if state["pending"]:
                red.wait()                                 # dw of the previous step is complete here
                state["pending"] = False
            if fused:
                sums = b.updat(x, dy, sums_only=True, slot=i & 1)
                if ev: ev[2].record()
                red.start(sums, dws[i & 1])                # reduce-scatter f32 -> finalize 1/world -> all-gather, side stream
            else:
                b.updat(x, dy, dw=dws[i & 1])
                if ev: ev[2].record()
                if i == 0: b._bench_updat_kernel = _lib.last_kernel()      # (which weight-gradient kernel family the call took: roofline.delivery_updat)
                if use_dist:
                    red.start(dws[i & 1])                  # generic path: all-reduce through an fp32 copy
            state["pending"] = use_dist
            dx = b.bprop(dy, w)
            if ev: ev[3].record()
            state["i"] = i + 1
            return y, dx, dws[i & 1]

        def drain():
            if state["pending"]:
                red.wait()
                state["pending"] = False

        if prewarm > 0:
            t_pre = time.perf_counter()
            while time.perf_counter() - t_pre < prewarm:
                for _ in range(10):
                    step()
                torch.cuda.synchronize()
        for _ in range(warmup):
            step()
        drain()
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps - 1):
            step(evs[i])
        y, dx, dw = step(evs[steps - 1])
        drain()                                            # the last step's gradient belongs to the timed region
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        per = [float(np.mean([e[i].elapsed_time(e[i + 1]) for e in evs])) for i in range(3)]   # ms: fprop, updat, bprop
        via = red.via if use_dist else None
        return el, per, via, {"y": y, "dx": dx, "dw": dw}

    cus = torch.cuda.get_device_properties(local).multi_processor_count

    def summarize(b, n_local, dtype, el, per, steps, layout=None):
        """metrics of one workload: whole-job TFLOP/s, per-pass times, roofline of the dominant kernel"""
        s = 4 if dtype == "f32" else 2
        flops_pass = 2.0 * b.blocks * b.bsize ** 2 * n_local
        f_ms, u_ms, b_ms = per
        # bprop is ONE launch of the xprop kernel (fprop = the same kernel, for some kernel families + a small weight-transpose
        # launch); updat is one launch of the updat kernel (+ a summing pass when the minibatch is split).  HIP events on the
        # launch stream.
        cand = {"bsmm_xprop(bprop)": (b_ms, flops_pass, alg_bytes_xprop(b, n_local, s)), "bsmm_updat": (u_ms, flops_pass, alg_bytes_updat(b, n_local, s))}
        dom = max(cand, key=lambda k: cand[k][0])
        roof = roofline_of(dom, *cand[dom], dtype)
        if layout is not None and b.axis == 1 and dtype != "f32":
            dl = delivery_roof(layout, b.bsize, n_local, f_ms, cus)
            if dl:
                roof["delivery"] = dl
        if layout is not None and dtype != "f32" and (b.axis == 1 or b.bsize == 16):
            try:
                up = b._tables_on(torch.device("cuda", local)).updat_plan
                du = delivery_roof_updat(up.host if up is not None else None, n_local, u_ms, cus, kernel_code=getattr(b, "_bench_updat_kernel", None))
            except Exception:
                du = None
            if du:
                roof["delivery_updat"] = du
        return {"blocks": int(b.blocks), "value": round(3 * flops_pass * world * steps / el / 1e12, 3), "ms_per_step": round(el / steps * 1e3, 4),
                "pass_ms": {"fprop": round(f_ms, 4), "bprop": round(b_ms, 4), "updat": round(u_ms, 4)},
                "pass_tflops": {"fprop": round(flops_pass / f_ms / 1e9, 2), "bprop": round(flops_pass / b_ms / 1e9, 2),
                                "updat": round(flops_pass / u_ms / 1e9, 2)},
                "gbps_algorithmic": round((2 * alg_bytes_xprop(b, n_local, s) + alg_bytes_updat(b, n_local, s)) / (el / steps) / 1e9, 1),
                "roofline": roof}

    def workload_string(hidden, bsize, axis, dens, n_local):
        return ("bsmm fprop+bprop+updat %dx%d block_size=%d density=%.0f%% feature_axis=%d, minibatch %d per GPU, "
                "layout default_rng(1234)" % (hidden, hidden, bsize, dens * 100, axis, n_local))

    counters, counters_why = measured_counters()

    def attach_counters(rec, workload):
        """measured HBM bytes / GB/s and MFMA busy of the dominant kernel, when the committed PMC passes are of exactly this workload AND
        of this tree's kernels"""
        if world != 1:
            return
        if counters_why:
            rec["measured"] = {"dropped": counters_why}
            return
        c = counters.get(workload)
        if not c:
            return
        k = c.get(rec["roofline"]["kernel"])
        if k:
            rec["roofline"]["traffic"] = k.get("hbm_bytes")
            rec["measured"] = {"source": "profiles/%s_counters.json (rocprofv3 --pmc, separate passes; csrc digest %s)" % (PROFILE_ROUND, counters.get("_stamp", {}).get("csrc_digest")),
                               "kernels_profiled": k.get("kernel_names"),
                               #  the committed passes ran with the profiler attached, at its clock: their GB/s is bytes / THEIR
                               # kernel time; the bytes per launch do not depend on the clock, so they are also divided by this run's kernel time
                               "hbm_gbps_at_profiled_clock": k.get("hbm_gbps"), "mfma_busy": k.get("mfma_busy"), "kernel_us_profiled": k.get("time_us"),
                               "hbm_gbps_this_run": (round(k.get("hbm_bytes") / (rec["roofline"]["kernel_ms"] * 1e-3) / 1e9, 1)
                                                     if k.get("hbm_bytes") and rec["roofline"].get("kernel_ms") else None)}

    # ---- the main workload of this run ----
    cfg3 = a.config == "cfg3"
    if nloc0 is None:
        n_global = 4096
        assert n_global % world == 0, "cfg3: the 4096-row minibatch must divide over the ranks"
        n_local = a.n_local or n_global // world
    else:
        n_local = a.n_local or nloc0
    n_global = n_local * world
    layout, b, w, x, dy = setup(hidden0, bsize0, axis0, dens0, dtype0, n_local)
    el, per, via, outputs = run(b, w, x, dy, a.steps, a.warmup, a.prewarm_seconds)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, outputs)
    del outputs
    head = summarize(b, n_local, dtype0, el, per, a.steps, layout)
    dname = "d%d" % round(dens0 * 100)
    workload_name = workload_string(hidden0, bsize0, axis0, dens0, n_local)
    attach_counters(head, workload_name)
    roof = head["roofline"]
    out = {
        "metric": "bsmm_effective_tflops_%dx%d_bs%d_%s" % (hidden0, hidden0, bsize0, dname),
        "value": head["value"], "unit": "TFLOP/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "strong" if cfg3 else "weak", "vs_baseline": None,
        "dtype": dtype0, "data": "synthetic",
        "config": {"workload": workload_name, "blocks": int(b.blocks), "global_minibatch": n_global,
                   "parallelism": ("dp%d (minibatch sharded; dw: reduce-scatter of fp32 sums + shard finalize + all-gather over RCCL, "
                                   "overlapped with bprop and the next fprop)" % world) if world > 1 else "single GPU"},
        "gbps_algorithmic": head["gbps_algorithmic"],
        # what a dense GEMM of the same shapes would have to sustain to take the same time (reported alongside,
        # never the headline)
        "dense_equivalent_tflops": round(3 * 2.0 * hidden0 * hidden0 * n_global * a.steps / el / 1e12, 1),
        "pass_ms": head["pass_ms"], "pass_tflops": head["pass_tflops"],
        "roofline": roof,
    }
    if "measured" in head:
        out["measured"] = head["measured"]
    if rank == 0 and a.full:
        out.update(parity_check(torch, b, layout, w, x, dy, dtype0))
    if use_dist and a.full:
        # the gradient reduction on its own (inside the step it overlaps with bprop and the next fprop): time alone, and how much
        # of it the step does not hide
        fused = b.bsize == 32 and b.axis == 1 and dtype0 != "f32"
        sums_t = b.updat(x, dy, sums_only=True) if fused else torch.zeros(b.w_shape, dtype=torch.float32, device="cuda")
        dw_t = torch.empty(b.w_shape, dtype=td_of[dtype0], device="cuda")
        red = DwReduce(b, force=True) if fused else DwAllReduce(accumulate_fp32=True, force=True)

        def once():
            if fused:
                red.start(sums_t, dw_t)
            else:
                red.start(sums_t)
            red.wait()
        for _ in range(5):
            once()
        torch.cuda.synchronize()
        barrier()
        t_ar = time.perf_counter()
        for _ in range(20):
            once()
        torch.cuda.synchronize()
        ar_ms = (time.perf_counter() - t_ar) / 20 * 1e3
        if world > 1:
            tt = torch.tensor([ar_ms], dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ar_ms = float(tt.item())
        compute_ms = sum(per)
        ms_step = head["ms_per_step"]
        shard = int(b.blocks * b.bsize ** 2 / max(1, world))
        out["allreduce"] = {"via": via, "wire_bytes_per_rank": int((world - 1) * shard * (4 + (2 if dtype0 != "f32" else 4))) if fused
                            else int(2 * (world - 1) * shard * 4),
                            "sums_dtype": "f32", "ms_alone": round(ar_ms, 4), "compute_ms": round(compute_ms, 4),
                            "exposed_ms": round(max(0.0, ms_step - compute_ms), 4),
                            "hidden_frac": round(max(0.0, min(1.0, 1.0 - max(0.0, ms_step - compute_ms) / max(ar_ms, 1e-9))), 3),
                            "scaling_curve": "unmeasured on hardware until a multi-GPU node runs this (1-GPU leases only so far)"}
    extras = rank == 0 and world == 1 and not a.no_extras and a.config == "headline"
    # the other densities of the BASELINE metric (10 % and 50 %; the headline run above is the 20 % one), same shape and minibatch
    if a.config == "headline" and not a.no_densities:
        dens = {dname: {k: head[k] for k in ("blocks", "value", "ms_per_step", "pass_ms", "pass_tflops", "roofline")}}
        dens[dname]["roofline"] = dict(roof)
        if "measured" in head:
            dens[dname]["measured"] = head["measured"]
        for d in (0.1, 0.5):
            if abs(d - dens0) < 1e-9:
                continue
            lay2, b2, w2, x2, dy2 = setup(hidden0, bsize0, axis0, d, dtype0, n_local)
            st2 = max(10, a.steps // 2)
            el2, per2, _, _ = run(b2, w2, x2, dy2, st2, max(3, a.warmup // 2), min(a.prewarm_seconds, 0.2))
            r = summarize(b2, n_local, dtype0, el2, per2, st2, lay2)
            attach_counters(r, workload_string(hidden0, bsize0, axis0, d, n_local))
            key = "d%d" % round(d * 100)
            dens[key] = {k: r[k] for k in ("blocks", "value", "ms_per_step", "pass_ms", "pass_tflops", "roofline") }
            if "measured" in r:
                dens[key]["measured"] = r["measured"]
            del b2, w2, x2, dy2
        out["densities"] = dens
    # the other BASELINE configurations that fit one GPU, measured by the same machinery (fewer steps): configs[2] and configs[3]
    if extras:
        for name in ("cfg2", "cfg3"):
            hid, bsz, ax, dn, dt, nl = CONFIGS[name]
            nl = nl or 4096
            lay2, b2, w2, x2, dy2 = setup(hid, bsz, ax, dn, dt, nl)
            st2 = max(10, a.steps // 4)
            el2, per2, _, _ = run(b2, w2, x2, dy2, st2, 5, 0.2)
            r = summarize(b2, nl, dt, el2, per2, st2, lay2)
            wl = workload_string(hid, bsz, ax, dn, nl)
            attach_counters(r, wl)
            r["workload"] = "BASELINE configs[%s]: %s%s" % (name[3], wl, " (the whole global minibatch on one GPU)" if name == "cfg3" else "")
            r.update(parity_check(torch, b2, lay2, w2, x2, dy2, dt))
            out[name] = r
            del b2, w2, x2, dy2
    # the reference's own bench layout (Barabasi-Albert + I, test/blocksparse_matmul_bench.py:66-68) at the headline size, the small
    # minibatches of its bench (:78: N = 64; BASELINE configs[3]'s per-GPU shard: 512), and bsize 8 (north_star) -- each with its roofline
    if extras:
        def side_row(name, layout_x, bsz, ax, nl, what, steps_x=30):
            td = td_of["bf16"]
            bx = BlocksparseMatMul(layout_x, block_size=bsz, feature_axis=ax)
            gx = torch.Generator(device="cuda").manual_seed(11)
            wx = (torch.randn(bx.w_shape, device="cuda", generator=gx) * 0.01).to(td)
            xx = (torch.randn(bx.i_shape(nl), device="cuda", generator=gx) * 0.1).to(td)
            dyx = (torch.randn(bx.o_shape(nl), device="cuda", generator=gx) * 0.1).to(td)
            elx, perx, _, _ = run(bx, wx, xx, dyx, steps_x, 5, 0.1)
            r = summarize(bx, nl, "bf16", elx, perx, steps_x, layout_x)
            r["workload"] = what
            r.update(parity_check(torch, bx, layout_x, wx, xx, dyx, "bf16"))
            out[name] = r
        lay_ba = ba_layout(hidden0 // 32, 14, seed=1)
        side_row("ba", lay_ba, 32, 1, n_local, "Barabasi-Albert(%d, 14) + I layout (the reference's bench layout), block_size=32 feature_axis=1 bf16, minibatch %d, "
                 "fprop+bprop+updat" % (hidden0 // 32, n_local))
        def graph_us(fn, K=20):
            """us per call of fn as a hipGraph replay of K back-to-back calls: at small minibatches the eager Python call path (~10 us per call)
            is longer than the kernels"""
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(K):
                    fn()
            for _ in range(5):
                g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                g.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 20 / K * 1e6

        small = {}
        for hid_s, dens_s, nn in ((hidden0, dens0, 64), (hidden0, dens0, 512), (hidden0, dens0, 2048), (8192, 0.05, 512)):
            lay_s = layout if hid_s == hidden0 else random_layout(hid_s // 32, hid_s // 32, dens_s, seed=1234)
            bs_ = BlocksparseMatMul(lay_s, block_size=32, feature_axis=1)
            gs_ = torch.Generator(device="cuda").manual_seed(13)
            ws_ = (torch.randn(bs_.w_shape, device="cuda", generator=gs_) * 0.01).bfloat16()
            xs_ = (torch.randn(bs_.i_shape(nn), device="cuda", generator=gs_) * 0.1).bfloat16()
            dys_ = (torch.randn(bs_.o_shape(nn), device="cuda", generator=gs_) * 0.1).bfloat16()
            dws_ = torch.empty(bs_.w_shape, dtype=torch.bfloat16, device="cuda")
            # (two graphs per pass, the faster one: the first graph of a fresh object has once come out 10x slow for reasons outside the kernels)
            f_us = min(graph_us(lambda: bs_.fprop(xs_, ws_)) for _ in range(2))
            b_us = min(graph_us(lambda: bs_.bprop(dys_, ws_)) for _ in range(2))
            u_us = min(graph_us(lambda: bs_.updat(xs_, dys_, dw=dws_)) for _ in range(2))
            step_us = graph_us(lambda: (bs_.fprop(xs_, ws_), bs_.updat(xs_, dys_, dw=dws_), bs_.bprop(dys_, ws_)), K=10)
            eager_us = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                bs_.fprop(xs_, ws_); bs_.updat(xs_, dys_, dw=dws_); bs_.bprop(dys_, ws_)
            torch.cuda.synchronize()
            eager_us = (time.perf_counter() - t0) / 50 * 1e6
            fl = 2.0 * bs_.blocks * 1024 * nn
            cand = {"bsmm_xprop(bprop)": (b_us * 1e-3, fl, alg_bytes_xprop(bs_, nn, 2)), "bsmm_updat": (u_us * 1e-3, fl, alg_bytes_updat(bs_, nn, 2))}
            dom = max(cand, key=lambda k: cand[k][0])
            r = {"workload": "%dx%d bs 32 %.0f%% feature_axis=1 bf16, minibatch %d%s" % (hid_s, hid_s, dens_s * 100, nn, " (BASELINE configs[3]'s per-GPU shard)" if hid_s == 8192 else ""),
                 "timing": "hipGraph replay (20 calls per graph); eager_us_per_step = the same step through the Python call path",
                 "blocks": int(bs_.blocks), "pass_us": {"fprop": round(f_us, 2), "bprop": round(b_us, 2), "updat": round(u_us, 2)},
                 "us_per_step": round(step_us, 2), "eager_us_per_step": round(eager_us, 1), "value": round(3 * fl / step_us / 1e6, 2), "unit": "TFLOP/s",
                 "roofline": roofline_of(dom, *cand[dom], "bf16")}
            r.update(parity_check(torch, bs_, lay_s, ws_, xs_, dys_, "bf16"))
            small["%d_n%d" % (hid_s, nn)] = r
            del bs_, ws_, xs_, dys_, dws_
        out["small_n"] = small
        # gated fprop / bprop (per-block gates; round 6: gated weight images + the ungated kernels, blocksparse_amd/matmul.py::_gated_xprop)
        try:
            def ev_us(fn, reps=40, warm=10):
                for _ in range(warm):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps * 1e3
            gg = torch.Generator(device="cuda").manual_seed(17)
            gen_gate = torch.rand(b.blocks, device="cuda", generator=gg) * 2 - 0.5
            gen_gate[::7] = 0
            mask_gate = (torch.rand(b.blocks, device="cuda", generator=gg) < 0.8).float()
            grow = {}
            for gname, gt in (("ungated", None), ("mask_0_1", mask_gate), ("general", gen_gate)):
                grow[gname] = {"fprop_us": round(ev_us(lambda: b.fprop(x, w, gate=gt)), 1), "bprop_us": round(ev_us(lambda: b.bprop(dy, w, gate=gt)), 1)}
            grow["workload"] = "headline shape, fprop / bprop with per-block gates: a 0/1 mask (80 % ones: one exact weight image) and arbitrary fp32 gates (bf16: hi + lo images over doubled tables)"
            out["gated"] = grow
        except Exception as e:          # an extra line must never cost the headline
            out["gated"] = {"error": str(e)[:200]}
        # the reference's OWN benchmark shapes (test/blocksparse_matmul_bench.py:37-78): hidden = k * 2560, Barabasi-Albert + I at the listed sparsity
        # (k = 1: dense), block sizes 32 / 16 / 8 on feature axis 0, minibatch 64, bf16 -- one read of ~13 MB of weights per pass (round 6:
        # csrc/bsmm_xsmall0.h, the per-block weight-gradient kernels; all 18 shapes before / after: profiles/r06_ref_bench_shapes.txt)
        try:
            refb = {}
            for kmul, spars in ((1, 100.0), (3, 11.25), (8, 1.41)):
                for bs_r in (32, 16, 8):
                    n_r = kmul * 2560 // bs_r
                    if spars == 100.0:
                        lay_r = np.ones((n_r, n_r), dtype=np.int32)
                    else:
                        for m_r in range(1, n_r // 2):
                            if 100.0 * (2 * m_r * (n_r - m_r) + m_r * m_r + n_r - m_r) / n_r ** 2 >= spars:
                                break
                        lay_r = ba_layout(n_r, m_r, seed=1)
                    br = BlocksparseMatMul(lay_r, block_size=bs_r, feature_axis=0)
                    gr = torch.Generator(device="cuda").manual_seed(19)
                    wr = (torch.randn(br.w_shape, device="cuda", generator=gr) * 0.05).bfloat16()
                    xr = (torch.randn(br.i_shape(64), device="cuda", generator=gr) * 0.1).bfloat16()
                    er = (torch.randn(br.o_shape(64), device="cuda", generator=gr) * 0.1).bfloat16()
                    dwr = torch.empty(br.w_shape, dtype=torch.bfloat16, device="cuda")
                    fu, bu, uu = graph_us(lambda: br.fprop(xr, wr)), graph_us(lambda: br.bprop(er, wr)), graph_us(lambda: br.updat(xr, er, dw=dwr))
                    wbytes = br.blocks * bs_r * bs_r * 2
                    refb["hidden%d_bs%d" % (kmul * 2560, bs_r)] = {"blocks": int(br.blocks), "density_pct": round(100.0 * br.blocks / n_r ** 2, 2), "w_mb": round(wbytes / 1e6, 1),
                                                                   "pass_us": {"fprop": round(fu, 1), "bprop": round(bu, 1), "updat": round(uu, 1)},
                                                                   "tflops": round(3 * 2.0 * br.blocks * bs_r * bs_r * 64 / (fu + bu + uu) / 1e6, 1),
                                                                   "w_stream_gbps": round(3 * wbytes / (fu + bu + uu) / 1e3, 0)}
                    del br, wr, xr, er, dwr
            refb["workload"] = "the reference benchmark's shapes: feature_axis=0, minibatch 64, bf16, hidden k * 2560 (Barabasi-Albert + I; k = 1 dense), hipGraph replays"
            out["ref_bench_n64"] = refb
        except Exception as e:
            out["ref_bench_n64"] = {"error": str(e)[:200]}
        side_row("bs8", random_layout(hidden0 // 8, hidden0 // 8, 0.10, seed=1234), 8, 0, n_local,
                 "4096x4096 block_size=8 density=10%% feature_axis=0 bf16, minibatch %d, fprop+bprop+updat (super-block path)" % n_local, steps_x=20)
    # BASELINE.json configs[1]: same layout, fp32, feature_axis=1, fprop only.  Priced against the fp32 matrix-core peak
    # (157.3 TF; AI 195 > ridge 20) although the kernel computes the fp32 result exactly from bf16 pieces on the 16-bit
    # matrix cores (six MFMAs per product, bsmm_xcols.h), whose ceiling for this formulation is 2500 / 6 = 417 TF.
    if extras:
        N = n_local
        b32 = BlocksparseMatMul(layout, block_size=bsize0, feature_axis=1)
        g32 = torch.Generator(device="cuda").manual_seed(7)
        w32 = torch.randn(b32.w_shape, device="cuda", generator=g32) * 0.01
        x32 = torch.randn(b32.i_shape(N), device="cuda", generator=g32) * 0.1
        def time32(bump):
            for _ in range(20):
                b32.fprop(x32, w32)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                if bump:
                    b32.invalidate_weights()           # a training step sees every weights version once per op: no cache hit
                b32.fprop(x32, w32)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 50
        ms32_cached = time32(False)
        ms32 = time32(True)
        # the other two passes in fp32 (not part of configs[1]): bprop on the same fused-split kernel, updat through the bf16 streaming
        # kernel (six piece products as six pairs of one launch; the per-block fp32 kernel it replaces ran 2.2 ms on this axis)
        dy32 = torch.randn(b32.o_shape(N), device="cuda", generator=g32) * 0.1
        def time_pass(fn):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 20
        ms32_bprop = time_pass(lambda: b32.bprop(dy32, w32))
        ms32_updat = time_pass(lambda: b32.updat(x32, dy32))
        del dy32
        tf32 = 2.0 * b32.blocks * bsize0 ** 2 * N / ms32 / 1e9
        out["fp32_fprop_axis1"] = {"workload": "BASELINE configs[1]: %dx%d bs%d d%.0f%% fp32 feature_axis=1 fprop, minibatch %d" %
                                               (hidden0, hidden0, bsize0, dens0 * 100, N),
                                   "kernel": "exact three-piece bf16 split on v_mfma_f32_32x32x16_bf16; round 4: the activations are split INSIDE the "
                                             "kernel (fp32 slabs staged by LDS-DMA, pieces made between LDS and LDS: xcol32sf_kernel), no activation "
                                             "pre-pass, no pieces in the workspace; `ms` includes the split of the weights (one launch per weights "
                                             "version: what a training step pays), `ms_weights_cached` does not (bsmm_prepare_weights once)",
                                   "ms": round(ms32, 4), "ms_weights_cached": round(ms32_cached, 4), "bprop_ms": round(ms32_bprop, 4), "updat_ms": round(ms32_updat, 4),
                                   "tflops": round(tf32, 2), "peak": PEAK_MFMA["f32"],
                                   "frac": round(tf32 / PEAK_MFMA["f32"], 4),
                                   "peak_bf16_six_products": round(PEAK_MFMA["bf16"] / 6, 1),
                                   "frac_bf16_six_products": round(tf32 / (PEAK_MFMA["bf16"] / 6), 4)}
        del b32, w32, x32
    if rank == 0 and world == 1 and a.config == "headline" and not a.no_attention:
        out["attention"] = attention_extra(a)
    out["cpu_baseline"] = cpu_out
    # The JSON line must be the LAST thing on stdout.  RCCL's version banner (NCCL_DEBUG=VERSION) sits in every rank's C stdio
    # buffer and would otherwise be flushed at process exit, after Python's own output: push it out on ALL ranks first, meet at
    # a barrier, and only then let rank 0 print.
    import ctypes

    def flush_c_stdio():
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()

    flush_c_stdio()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        flush_c_stdio()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
