"""Host state of BlocksparseMatMul that needs no device to check (the device side: tests/test_host_state_gpu.py): the one rule of the
per-tensor caches as the bsize-64 quadrant view applies it, and the doubled-table operator of gated calls as a complete operator."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def test_quadrant_view_follows_the_cache_rule(monkeypatch):
    """BlocksparseMatMul._split64_cached: one entry (weakref, key, view) per operator, hit only for the same tensor object at the same
    version; under stream capture the entry is neither used nor replaced; a mutation the version counter cannot see is stale until
    invalidate_weights(); a tensor that autograd follows bypasses the cache (the gather is part of its graph)."""
    import torch
    from blocksparse_amd import BlocksparseMatMul
    b = BlocksparseMatMul(np.ones((2, 2), dtype=np.int32), block_size=64, feature_axis=1)
    w = torch.from_numpy(np.random.RandomState(0).normal(size=b.w_shape).astype(np.float32))
    v = b._split64_cached(w)
    hit = b._split64_hit
    assert hit is not None and hit[0]() is w and hit[2] is v and torch.equal(v, b._split64(w))
    assert b._split64_cached(w) is v and b._split64_hit is hit                       # a hit leaves the entry in place
    w.mul_(2)                                                                        # a mutation the version counter sees
    v2 = b._split64_cached(w)
    hit = b._split64_hit
    assert v2 is not v and hit[0]() is w and hit[2] is v2 and torch.equal(v2, b._split64(w))
    other = torch.ones(b.w_shape)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        v3 = b._split64_cached(w)
        assert v3 is not v2 and torch.equal(v3, v2)                                  # the stored view is not used ...
        assert torch.equal(b._split64_cached(other), b._split64(other))
        assert b._split64_hit is hit                                                 # ... and not replaced
        b2 = BlocksparseMatMul(np.ones((2, 2), dtype=np.int32), block_size=64, feature_axis=1)
        assert torch.equal(b2._split64_cached(w), v2) and b2._split64_hit is None    # ... nor is one stored
    assert b._split64_cached(w) is v2 and b._split64_hit is hit
    w.data.mul_(2)                                                                   # one it cannot see: stale until ...
    assert b._split64_cached(w) is v2 and not torch.equal(v2, b._split64(w))
    b.invalidate_weights()
    assert b._split64_hit is None and torch.equal(b._split64_cached(w), b._split64(w))
    assert b._split64_cached(other) is b._split64_hit[2] and b._split64_hit[0]() is other      # another tensor takes the entry over
    hit = b._split64_hit
    w.requires_grad_()
    v4 = b._split64_cached(w)
    assert v4.requires_grad and torch.equal(v4.detach(), b._split64(w.detach())) and b._split64_hit is hit
    with torch.no_grad():                                                            # (nothing to follow: cached again)
        assert b._split64_cached(w) is b._split64_hit[2] and b._split64_hit[0]() is w


# what __init__ derives from a LAYOUT (the reference-policy tables and their statistics): everything else an operator holds is state
TABLE_ATTRS = {"updat_lut", "updat_list", "fprop_list", "fprop_lut", "l2_lut", "fprop_shared", "l2_shared", "fprop_segments", "fprop_locks",
               "bprop_list", "bprop_lut", "bprop_shared", "bprop_segments", "bprop_locks", "sparsity", "layout"}


@pytest.mark.parametrize("bs", [16, 32])
def test_doubled_operator_is_a_complete_operator(bs):
    """BlocksparseMatMul._doubled() (gated calls over two weight images) holds every attribute a constructed operator holds besides
    the layout's own tables, over 2 x blocks weights of the same features; it is never gated itself; invalidate_weights() reaches it."""
    from blocksparse_amd import BlocksparseMatMul
    lay = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.int32)
    b = BlocksparseMatMul(lay, block_size=bs, feature_axis=1)
    d = b._doubled()
    state = set(vars(BlocksparseMatMul(lay, block_size=bs, feature_axis=1))) - TABLE_ATTRS
    assert {"count", "_l2_dev", "_workspaces", "_args_cache", "_prepared_w", "_device_cache", "_split64_hit", "_gate_kind_hit", "cache_prepared",
            "native64", "flow", "gate_images", "gate_kind", "_inner", "_dbl", "_xprop_only"} <= state
    assert state <= set(vars(d)), sorted(state - set(vars(d)))
    assert b._doubled() is d and d.name == b.name + "/gated2"
    assert d.blocks == 2 * b.blocks and d.w_shape == (2 * b.blocks, bs, bs) and d.g_shape == (2 * b.blocks,)
    assert (d.C, d.K, d.CB, d.KB) == (b.C, b.K, b.CB, b.KB) and (d.bsize, d.axis) == (b.bsize, b.axis)
    assert d._xprop_only is True and d.gate_images is False and d.gate_kind == "general" and d._inner is None and d._dbl is None
    b.flow = False
    assert b._doubled().flow is False                                                # the parent's kernel choice, on every call
    stale = (lambda: None, None, "binary")
    d._gate_kind_hit = d._split64_hit = d._prepared_w[0] = stale
    b.invalidate_weights()
    assert d._gate_kind_hit is None and d._split64_hit is None and not d._prepared_w
