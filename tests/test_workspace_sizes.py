"""CPU tier: bsmm_workspace_bytes(), bsmm_prepared_bytes() and the five descriptor fields bsmm_plan_attach() writes, over a grid of argument
blocks, against digests recorded from the library BEFORE the dispatch layer was restructured (tests/golden/workspace_sizes.json).  All three
are host-only (without a device the cost models see 256 compute units, the MI355X's own count), so a refactor of the dispatch that changes
one answer -- a size, a route the sizing assumes, a packed descriptor bit -- fails here and names the (bsize, axis, dtype, op) group.

`python tests/test_workspace_sizes.py --record` rewrites the digests from the library in the tree: only ever from a commit whose answers are
the reference (the parent of a refactor), never to make a failure go away."""
import ctypes
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
NS = (1, 64, 255, 256, 768, 769, 2048, 4097, 8192)      # around every minibatch threshold of the sizing (256: fp32 split; 768 x pairs: one wave)
FLAGS = (0, 2, 4, 8, 16, 1)                             # production, FORCE_VALU, NO_PLAN, FORCE_PLAN, DW_SUMS, GATED_DW


def _tables():
    """{(bsize, axis, dtype, op): [rows]} -- one row per argument block: the inputs, the descriptor and the two sizes"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib as lib
    from blocksparse_amd import lut as LT
    from blocksparse_amd.matmul import _host_plan, _host_updat_plan
    import _parity as P
    L = lib.load()
    ip = ctypes.POINTER(ctypes.c_int32)
    layouts = {"r37x53": P.random_layout(37, 53, 0.15, seed=11), "d8": np.ones((8, 8), dtype=np.int32), "hubs": P.ba_layout(40, 3, seed=1)}
    groups = {}
    for (lname, lay), bs, axis, dt, seg in itertools.product(sorted(layouts.items()), (8, 16, 32, 64), (0, 1), (lib.F32, lib.F16, lib.BF16), (False, True)):
        if bs == 64 and axis == 0:
            continue
        t = LT.build_tables(lay, z_order=True, segmented=seg)
        B, CB, KB = t["blocks"], t["CB"], t["KB"]
        for opts in (0, lib.PLAN_XCOL_FLOW, lib.PLAN_UPDAT_NO_DIRECT, lib.PLAN_STREAM_8, lib.PLAN_UPDAT16_WINDOWED, None):
            plans = {}
            if opts is not None:
                plans[lib.OP_FPROP] = _host_plan(t["fprop"]["lut"], t["fprop"]["segments"], B, KB, bs, dt, axis, opts)
                plans[lib.OP_BPROP] = _host_plan(t["bprop"]["lut"], t["bprop"]["segments"], B, CB, bs, dt, axis, opts)
                plans[lib.OP_UPDAT] = _host_updat_plan(t["updat_lut"], B, CB, KB, bs, lib.BF16 if dt == lib.F32 else dt, axis, opts)
            for op, N, fl, gate, split, pc, prep in itertools.product((lib.OP_FPROP, lib.OP_BPROP, lib.OP_UPDAT), NS, FLAGS, (0, 16), (0, 4), (1, 3), (0, 8192)):
                if op != lib.OP_UPDAT and (split or pc != 1 or fl in (16, 1)):
                    continue
                if op == lib.OP_UPDAT and prep:
                    continue
                a = lib.BsmmArgs()
                side = t["fprop"] if op != lib.OP_BPROP else t["bprop"]
                a.lut = 4096
                a.blocks, a.bsize, a.dtype, a.N, a.axis = B, bs, dt, N, axis
                a.segments, a.locks, a.shared = side["segments"], side["locks"], side["shared"]
                a.C, a.K = (CB * bs, KB * bs) if op != lib.OP_BPROP else (KB * bs, CB * bs)
                a.flags, a.split, a.pcount = fl, split, pc
                a.gate = gate or None
                rc = 0
                p = plans.get(op)
                if p is not None:
                    rc = L.bsmm_plan_attach(ctypes.byref(a), p.ctypes.data_as(ip), p.size, ctypes.c_void_p(4096))
                a.prepared_w = prep or None
                groups.setdefault((bs, axis, dt, op), []).append(
                    (lname, int(seg), -1 if opts is None else opts, N, fl, gate, split, pc, prep, rc, a.plan_magic, a.plan_width, a.plan_waves,
                     a.plan_items, a.plan_inner, int(L.bsmm_workspace_bytes(op, ctypes.byref(a))),
                     int(L.bsmm_prepared_bytes(op, ctypes.byref(a))) if op != lib.OP_UPDAT else 0))
    return groups


def _digests():
    return {"bs%d-a%d-dt%d-op%d" % k: [len(rows), hashlib.sha256(repr(rows).encode()).hexdigest()[:24]] for k, rows in sorted(_tables().items())}


@pytest.fixture(scope="module")
def digests():
    return _digests()


def test_every_group_is_recorded(digests):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(digests)
    assert len(want) == 7 * 3 * 3           # (bsize, axis) pairs x dtypes x ops


def test_sizes_and_descriptors_match_the_record(digests):
    want = json.load(open(GOLDEN))
    bad = [k for k in sorted(want) if digests.get(k) != want[k]]
    assert not bad, "workspace sizes / prepared sizes / plan descriptors changed in: " + ", ".join(bad)


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        with open(GOLDEN, "w") as f:
            json.dump(_digests(), f, indent=0, sort_keys=True)
            f.write("\n")
    else:
        print(json.dumps(_digests(), indent=0, sort_keys=True))
