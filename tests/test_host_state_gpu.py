"""The host layer's per-tensor state under mutation and stream capture: BlocksparseMatMul keeps a binary / general verdict per gate tensor, the
prepared fp32 pieces per weight tensor and the bsize-64 quadrant view per weight tensor.  The contract pinned here:

  C1  a graph replay reflects the CURRENT contents of every tensor the captured call was given (w, gate, x): nothing derived from their old
      contents is baked into the graph;
  C2  capturing never leaves a cache entry that describes work which has not run: an eager call after a capture returns what a fresh operator
      object returns, before or after a replay;
  C3  a mutation that ``_version`` sees is always picked up; one it cannot see (``.data``) is picked up after ``invalidate_weights()``, which
      forgets the gate verdict too.

Gated results are held to the float64 oracle (oracle/bsmm_oracle.py) at the suite's bar; the cache tests compare bit for bit with a fresh operator
object.  Captures are single linear chains; every buffer read here is a live allocation."""
import functools

import numpy as np
import pytest

import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import BlocksparseMatMul, _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()
    return torch, BlocksparseMatMul, _lib


def _side_stream_warmup(torch, fn):
    """Run ``fn`` once on a side stream, ordered after and before the current stream: table uploads, plans and function attributes are host /
    first-call work that must not fall into a capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return side


# ---------------------------------------------------------------------------------------------------------------- gate kind
GATE_LAYOUTS = {32: (40, 24, 0.3, 21), 16: (72, 56, 0.15, 22)}      # the shapes of test_gating.test_gated_calls_run_the_ungated_kernels
GATE_N = 1024
BAR = P.L2_BAR["bf16"]


def _general_gate(blocks, seed):
    """Learned-looking gates: uniform in [0.1, 1.9], a fifth exactly 0, a fifth exactly 1."""
    rs = np.random.RandomState(seed)
    g = rs.uniform(0.1, 1.9, blocks).astype(np.float32)
    pick = rs.rand(blocks)
    g[pick < 0.2] = 0.0
    g[(pick >= 0.2) & (pick < 0.4)] = 1.0
    return g


def _mask_gate(blocks, seed):
    return (np.random.RandomState(seed).rand(blocks) < 0.7).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _gate_case(bs):
    """Host side of the gate tests, computed once per block size and never written again: inputs, three gates, and per pass the rounded float64
    oracle under each gate plus the ONE-image result (the ungated oracle over round_to(g w, bf16)) a stale "binary" verdict would compute."""
    CB, KB, dens, seed = GATE_LAYOUTS[bs]
    lay = P.random_layout(CB, KB, dens, seed=seed)
    t = orc.build_layout_luts(lay, bs)
    W, X, E = P.make_inputs((t["blocks"], bs, bs), (GATE_N, CB * bs), (GATE_N, KB * bs), "bf16", seed=3)
    gates = {"mask": _mask_gate(t["blocks"], 2), "general": _general_gate(t["blocks"], 4), "mask2": _mask_gate(t["blocks"], 6)}
    rnd = lambda a: orc.round_to(a, "bf16")
    W1 = rnd(gates["general"][:, None, None] * np.asarray(W, dtype=np.float32))
    refs = {}
    for which, fn, inp in (("fprop", orc.fprop, X), ("bprop", orc.bprop, E)):
        refs[which] = {name: rnd(fn(t, inp, W, 1, gate=g)) for name, g in gates.items()}
        refs[which]["one_image"] = rnd(fn(t, inp, W1, 1))
    for a in [W, X, E] + list(gates.values()) + [r for d in refs.values() for r in d.values()]:
        a.setflags(write=False)
    return lay, W, X, E, gates, refs


def _gate_setup(env, bs, which):
    torch, BSMM, lib = env
    lay, W, X, E, gates, refs = _gate_case(bs)
    b = BSMM(lay, block_size=bs, feature_axis=1)
    b.GATE_IMAGES_MIN_N = {32: 1024, 16: 1024}      # (bsize 16 takes the images from 2048 rows by default: a measured rule, not a limit)
    w = P.to_dev(np.array(W), "bf16", torch)                        # (copies: the shared host arrays are read-only)
    inp = P.to_dev(np.array(X if which == "fprop" else E), "bf16", torch)
    dev = {k: torch.from_numpy(np.array(g)).cuda() for k, g in gates.items()}
    return b, getattr(b, which), w, inp, dev, refs[which]


def _l2(got, ref):
    return P.errors(P.to_host(got), ref)[0]


@pytest.mark.parametrize("which", ["fprop", "bprop"])
@pytest.mark.parametrize("bs", [32, 16])
def test_captured_gated_call_follows_the_gate_buffer(env, bs, which):
    """C1 for the gate.  The usual order of events: an eager call with a pruning mask (the verdict "binary" is cached for that tensor), a capture
    of the same call, then the gate buffer refilled in place with learned values and a replay.  A verdict baked into the graph multiplies with
    ONE bf16 image round(g w): 2.4e-3 from the gated float64 result (asserted on the host below, so that this test can tell the two paths
    apart), against the bar of 1e-3 that the hi + lo image pair meets."""
    torch, BSMM, lib = env
    b, call, w, inp, gates, ref = _gate_setup(env, bs, which)
    one = P.errors(ref["one_image"], ref["general"])[0]
    print("bs %d %s: one image against the gated oracle: L2 %.3e (bar %.1e)" % (bs, which, one, BAR))
    assert one >= 2 * BAR, (bs, which, one)
    g = gates["mask"].clone()
    assert _l2(call(inp, w, gate=g), ref["mask"]) <= BAR
    assert b._gate_kind_hit is not None and b._gate_kind_hit[0]() is g and b._gate_kind_hit[2] == "binary"      # the verdict a capture must not use
    _side_stream_warmup(torch, lambda: call(inp, w))                                           # the ungated tables / plans
    b._doubled()._tables_on(inp.device)                                                        # (plans are host work: built before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call(inp, w, gate=g)
    g.copy_(gates["general"])
    graph.replay()
    torch.cuda.synchronize()
    err = _l2(got, ref["general"])
    print("bs %d %s: replay after g.copy_(general): L2 %.3e" % (bs, which, err))
    assert err <= BAR, (bs, which, "general gates in the captured buffer", err)
    g.copy_(gates["mask2"])
    graph.replay()
    torch.cuda.synchronize()
    err = _l2(got, ref["mask2"])
    assert err <= BAR, (bs, which, "another mask in the captured buffer", err)


@pytest.mark.parametrize("bs", [32, 16])
def test_gate_kind_follows_mutations(env, bs):
    """C3 for the gate, eagerly: an in-place refill the version counter sees; one it cannot see, followed by invalidate_weights(); a new gate
    tensor that the allocator puts at a freed gate's address (the construction of test_prepared_weights_cache_fp32)."""
    torch, BSMM, lib = env
    for which in ("fprop", "bprop"):
        b, call, w, inp, gates, ref = _gate_setup(env, bs, which)
        g = gates["mask"].clone()
        assert _l2(call(inp, w, gate=g), ref["mask"]) <= BAR and b._gate_kind_hit[2] == "binary"
        g.copy_(gates["general"])                                    # _version moves
        err = _l2(call(inp, w, gate=g), ref["general"])
        assert err <= BAR, (bs, which, "copy_", err)

        g2 = gates["mask"].clone()
        assert _l2(call(inp, w, gate=g2), ref["mask"]) <= BAR and b._gate_kind_hit[0]() is g2 and b._gate_kind_hit[2] == "binary"
        version = g2._version
        g2.data.copy_(gates["general"])                              # _version does not
        assert g2._version == version
        b.invalidate_weights()
        assert b._gate_kind_hit is None
        err = _l2(call(inp, w, gate=g2), ref["general"])
        assert err <= BAR, (bs, which, ".data.copy_ + invalidate_weights", err)

        ga = (gates["mask"] * 1.0).contiguous()
        assert _l2(call(inp, w, gate=ga), ref["mask"]) <= BAR and b._gate_kind_hit[2] == "binary"
        ptr, ver = ga.data_ptr(), ga._version
        del ga
        gb = (gates["general"] * 1.0).contiguous()                   # same size: usually the same block
        recycled = gb.data_ptr() == ptr and gb._version == ver
        err = _l2(call(inp, w, gate=gb), ref["general"])
        assert err <= BAR, (bs, which, "a new gate tensor is a new tensor", recycled, err)


# ---------------------------------------------------------------------------------------------------------------- prepared fp32 pieces
def _f32_setup(env, which):
    """bsize 32, feature axis 1, fp32 with the plan forced: the kernel that multiplies with prepared bf16 pieces of W (the caller sets the
    kernel variant).  Returns the operator, a factory of fresh ones, the pass, w and two inputs."""
    torch, BSMM, lib = env
    lay = P.random_layout(40, 40, 0.2, seed=5)
    fresh = lambda: BSMM(lay, block_size=32, feature_axis=1)
    b = fresh()
    N = 256
    gen = P.gen(torch, 2)
    w = torch.randn(b.w_shape, device="cuda", generator=gen) * 0.05
    shape = b.i_shape(N) if which == "fprop" else b.o_shape(N)
    x = torch.randn(shape, device="cuda", generator=gen) * 0.1
    x2 = torch.randn(shape, device="cuda", generator=gen) * 0.1
    return b, fresh, w, x, x2


def _fresh_result(env, fresh, which, x, w):
    """What a new operator object computes eagerly -- first checked to be reproducible bit for bit, or torch.equal below would prove nothing."""
    torch, BSMM, lib = env
    y1, y2 = getattr(fresh(), which)(x, w), getattr(fresh(), which)(x, w)
    assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT
    torch.cuda.synchronize()
    assert torch.equal(y1, y2), "two eager calls on fresh operator objects differ"
    return y1


@pytest.mark.parametrize("which", ["fprop", "bprop"])
def test_capture_after_warmup_on_the_capture_stream(env, which):
    """C1 for the weights: the warm-up on the capture stream leaves prepared pieces whose key the captured call matches.  Served from the cache,
    the capture would not contain the preparation, and a replay after an optimizer step would multiply with the old pieces."""
    torch, BSMM, lib = env
    op = lib.OP_FPROP if which == "fprop" else lib.OP_BPROP
    lib.set_kernel_variant(3)
    try:
        b, fresh, w, x, _ = _f32_setup(env, which)
        call = getattr(b, which)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call(x, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT and op in b._prepared_w and b._prepared_w[op][0]() is w      # else: vacuous
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            y = call(x, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT
        w.mul_(2.0)                                                  # optimizer step
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, _fresh_result(env, fresh, which, x, w))
    finally:
        lib.set_kernel_variant(0)


@pytest.mark.parametrize("which", ["fprop", "bprop"])
def test_second_graph_on_one_stream_prepares_its_own_pieces(env, which):
    """Two graphs captured on one stream (one per minibatch bucket): the second must not be served by what the first one's capture left behind
    -- its preparation would be missing from the graph, and the pieces it reads were only recorded, never made."""
    torch, BSMM, lib = env
    op = lib.OP_FPROP if which == "fprop" else lib.OP_BPROP
    lib.set_kernel_variant(3)
    try:
        b, fresh, w, x, x2 = _f32_setup(env, which)
        call = getattr(b, which)
        _side_stream_warmup(torch, lambda: call(x, w))
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT and op in b._prepared_w
        s = torch.cuda.Stream()
        graph_a, graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph_a, stream=s):
            y_a = call(x, w)
        with torch.cuda.graph(graph_b, stream=s):
            y_b = call(x2, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT
        w.mul_(2.0)
        torch.cuda.synchronize()
        graph_b.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_b, _fresh_result(env, fresh, which, x2, w))
        del y_a
    finally:
        lib.set_kernel_variant(0)


@pytest.mark.parametrize("which", ["fprop", "bprop"])
def test_eager_call_after_a_capture_is_not_served_from_the_capture(env, which):
    """C2: a capture that has not been replayed has prepared nothing.  An eager call on the capture stream with the same weights must make its
    own pieces (a cache entry left by the capture would point it at the warm-up's pieces of OTHER weights); and again after a replay."""
    torch, BSMM, lib = env
    op = lib.OP_FPROP if which == "fprop" else lib.OP_BPROP
    lib.set_kernel_variant(3)
    try:
        b, fresh, w, x, _ = _f32_setup(env, which)
        call = getattr(b, which)
        w_warm = w * 0.5                          # (other weights: the buffer a miss reuses must not hold the pieces of w by accident)
        _side_stream_warmup(torch, lambda: call(x, w_warm))
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT and op in b._prepared_w and b._prepared_w[op][0]() is w_warm
        want = _fresh_result(env, fresh, which, x, w)
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            y_g = call(x, w)
        for replayed in (False, True):
            if replayed:
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(y_g, want)
            with torch.cuda.stream(s):
                y = call(x, w)
            assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT
            torch.cuda.synchronize()
            assert torch.equal(y, want), ("eager call on the capture stream", "after a replay" if replayed else "before any replay")
    finally:
        lib.set_kernel_variant(0)


# ---------------------------------------------------------------------------------------------------------------- bsize-64 quadrant view
def _b64_setup(env, which):
    torch, BSMM, lib = env
    lay = P.random_layout(20, 12, 0.3, seed=6)

    def fresh():
        b = BSMM(lay, block_size=64, feature_axis=1)
        b.native64 = False                       # always the host-side quadrant view of W
        return b
    b = fresh()
    N = 128
    W, X, E = P.make_inputs(b.w_shape, b.i_shape(N), b.o_shape(N), "bf16", seed=8)
    w = P.to_dev(W, "bf16", torch)
    x = P.to_dev(X if which == "fprop" else E, "bf16", torch)
    return b, fresh, w, x


def _fresh64(torch, fresh, which, x, w):
    y1, y2 = getattr(fresh(), which)(x, w), getattr(fresh(), which)(x, w)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2), "two eager calls on fresh operator objects differ"
    return y1


@pytest.mark.parametrize("which", ["fprop", "bprop"])
def test_quadrant_view_capture_after_warmup(env, which):
    """C1 for the bsize-64 quadrant view: its cache key has no stream, so any eager warm-up with the same weights makes the captured call a hit
    -- the gather would be missing from the graph and a replay after ``w.mul_()`` would multiply with the old quadrants."""
    torch, BSMM, lib = env
    b, fresh, w, x = _b64_setup(env, which)
    call = getattr(b, which)
    call(x, w)
    assert b._split64_hit is not None and b._split64_hit[0]() is w      # else: vacuous
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = call(x, w)
    w.mul_(2.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, _fresh64(torch, fresh, which, x, w))


@pytest.mark.parametrize("which", ["fprop", "bprop"])
def test_quadrant_view_eager_call_after_a_capture(env, which):
    """C2 for the quadrant view: a capture that met these weights for the first time recorded the gather without running it; an eager call
    afterwards -- on any stream -- must not find that view in the cache.  Before a replay, and after one."""
    torch, BSMM, lib = env
    b, fresh, w, x = _b64_setup(env, which)
    call = getattr(b, which)
    w_warm = w.clone()
    call(x, w_warm)                               # tables, plans, the permutation: everything but a view of w
    assert b._split64_hit is not None and b._split64_hit[0]() is w_warm
    want = _fresh64(torch, fresh, which, x, w)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = call(x, w)
    for replayed in (False, True):
        if replayed:
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y_g, want)
        y = call(x, w)
        torch.cuda.synchronize()
        assert torch.equal(y, want), "after a replay" if replayed else "before any replay"
