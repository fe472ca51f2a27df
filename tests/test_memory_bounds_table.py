"""CPU tier: the case table of tests/test_memory_bounds_gpu.py against the trace codes of blocksparse_amd/_lib.py and the dispatch thresholds
of csrc/bsmm_xprop_dispatch.h and csrc/bsmm_updat_dispatch.h.  A kernel family (or trace variant) added to the library must get a case in the memory-contract tier, or this fails."""
import os
import re

import test_memory_bounds_gpu as T
from blocksparse_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blocksparse_amd", "csrc")

# Codes the library defines and never reports.  K_XCOL32_ROWS: the row-split kernel of round 5, retired in round 6.  K_XCOL16, K_XCOL32_F32MFMA and
# K_UPDAT_WIN: kernels retired in round 4 (include/bsmm.h: "never reported any more").  The set is not taken on trust: the test below derives
# it from the trace() sites of the source, so a code that is emitted again needs a case.
RETIRED = {"K_XCOL32_ROWS", "K_XCOL16", "K_XCOL32_F32MFMA", "K_UPDAT_WIN"}


def _emitted():
    """Trace-code names some trace(a, BSMM_K_...) site of the library can report."""
    names = set()
    for fn in sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))):
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        for m in re.finditer(r"\btrace\(\s*a\s*,([^;]*);", src):
            names.update("K_" + n for n in re.findall(r"BSMM_K_([A-Z0-9_]+)", m.group(1)))
    return names


def test_table_covers_every_trace_code():
    defined = {n for n in dir(_lib) if re.match(r"K_[A-Z0-9_]+$", n)}
    assert RETIRED <= defined
    emitted = _emitted()
    assert emitted <= defined, emitted - defined                   # the binding knows every code the library reports
    assert defined - emitted == RETIRED, (defined - emitted, RETIRED)
    fams, variants = T.expected_codes()
    assert fams == defined - RETIRED, ("families without a case", defined - RETIRED - fams, "cases for unknown codes", fams - defined)
    kv = {n for n in dir(_lib) if re.match(r"KV_[A-Z0-9_]+$", n)}
    assert {v for _, v in variants} == kv, (kv, variants)
    assert ("K_UPDAT_BLOCK_TR", "KV_ONE_WAVE") in variants and ("K_XCOL32_FLOW", "KV_FLOW_HALF_UNITS") in variants
    exp = [e for c in T.CASES for e in c.exp if e]
    assert "K_XCOL32_FLOW/0" in exp and "K_UPDAT_BLOCK_TR/0" in exp       # ... and the plain variants of both


def test_table_is_explicit_and_stable():
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids)) and all(re.match(r"[a-z0-9x-]+$", i, re.I) for i in ids)
    for c in T.CASES:
        assert any(e is not None for e in c.exp) and c.dt in ("bf16", "f16", "f32") and 1 <= c.pairs <= 8
        lay = T.layouts(c.lay)
        assert lay.sum() > 0
        assert max(lay.shape) <= 70 or c.lay == "8x128", c.id               # (the one family that needs more workgroups to be chosen at all)
        assert (T.layouts(c.lay) == lay).all()                             # deterministic
    fam_types = {}
    for c in T.CASES:
        for e in c.exp:
            if e:
                fam_types.setdefault(e.partition("/")[0], set()).add(c.dt)
    both16 = {"K_XPROP_SMALL", "K_XPROP_MID", "K_XCOL32_FLOW", "K_XCOL32_STAGED", "K_XCOL16_STAGED", "K_XPROP_SUPER8", "K_UPDAT_STREAM",
              "K_UPDAT16_WIN", "K_UPDAT16_ROWS", "K_UPDAT_SUPER8", "K_UPDAT_BLOCK_TR", "K_XPROP_SEGMENT", "K_XPROP_VALU", "K_UPDAT_VALU", "K_UPDAT_BLOCK"}
    for fam in both16:
        assert {"bf16", "f16"} <= fam_types[fam], (fam, fam_types[fam])
    for fam in ("K_XCOL32_F32SPLIT", "K_XPROP_SEGMENT", "K_XPROP_VALU", "K_UPDAT_VALU", "K_UPDAT_STREAM", "K_UPDAT16_WIN", "K_UPDAT16_ROWS", "K_UPDAT_SUPER8", "K_UPDAT_BLOCK"):
        assert "f32" in fam_types[fam], fam
    # the five small-minibatch kernels of launch_xsmall: the narrow one (bsize 8 and 16 on feature axis 1), bsize 8 / 16 / 32 on feature axis 0, bsize 32 on axis 1
    small = {(c.bs, c.axis) for c in T.CASES if c.exp[0] == "K_XPROP_SMALL" and c.exp[1] == "K_XPROP_SMALL"}
    assert small >= {(8, 1), (16, 1), (8, 0), (16, 0), (32, 0), (32, 1)}, small
    # the streaming weight gradient with and without direct blocks, the raw-sums form, the fp32 split routes of bsize 8 / 16 / 32, bsize 64, both gate routes
    ids = " ".join(c.id for c in T.CASES)
    for word in ("stream-direct", "stream-nodirect", "stream-sums", "b8-f32-updat-split", "b16-f32-updat-split", "b32-f32-updat-split", "b16-f32-rows", "a1-b64-",
                 "gated-staged", "gated-images2", "gated-image1", "locked"):
        assert word in ids, word
    assert any(c.dt == "f32" and c.axis == 0 and c.N % 4 for c in T.CASES)       # fp32 rows that are no multiple of 16 bytes
    assert sum(1 for c in T.CASES if c.mis) >= 3
    assert {c.pairs for c in T.CASES if c.exp[2]} >= {1, 3, 8}
    assert any(c.lay == "holes" for c in T.CASES) and any(c.lay == "one" for c in T.CASES)


def test_thresholds_match_the_source():
    xsrc, usrc = (open(os.path.join(CSRC, fn)).read() for fn in ("bsmm_xprop_dispatch.h", "bsmm_updat_dispatch.h"))
    for name, val, src in (("XS0_NMAX", T.XS0_NMAX, xsrc), ("XSN_NMAX", T.XSN_NMAX, xsrc), ("UAW_NMAX", T.UAW_NMAX, usrc), ("UTS_NMAX", T.UTS_NMAX, usrc),
                           ("BSMM_SMALL_N_MAX", T.SMALL_N_MAX, xsrc)):
        m = re.search(r"#define %s (\d+)" % name, src)
        assert m and int(m.group(1)) == val, (name, m and m.group(1), val)
    ns = {(c.bs, c.axis): set() for c in T.CASES}
    for c in T.CASES:
        ns[(c.bs, c.axis)].add(c.N)
    assert {T.XSN_NMAX // 8, T.XSN_NMAX // 8 + 1, T.XSN_NMAX // 2, T.XSN_NMAX // 2 + 1} <= ns[(16, 1)]
    assert {T.XSN_NMAX, T.XSN_NMAX + 1} <= ns[(8, 1)]
    assert {1, 33, 63, 64, 65, 127, 128, 129, T.UTS_NMAX, T.UTS_NMAX + 1, T.SMALL_N_MAX, T.SMALL_N_MAX + 1, 1024, 1025} <= ns[(32, 1)]
    for bs in (32, 16, 8):
        assert {8, 40} <= ns[(bs, 0)] and any(n % 8 for n in ns[(bs, 0)]), bs
        assert {200, 264} & ns[(bs, 0)], bs
    assert {T.XS0_NMAX, T.XS0_NMAX + 8, 2 * T.XS0_NMAX, 2 * T.XS0_NMAX + 8} <= ns[(32, 0)]
    assert {T.UAW_NMAX // 2, T.UAW_NMAX // 2 + 8} <= ns[(32, 0)] and {T.UAW_NMAX, T.UAW_NMAX + 8} <= ns[(16, 0)]
    assert {2047, 2049} <= ns[(16, 1)]                                      # GATE_IMAGES_MIN_N of bsize 16 (2048); bsize 32: 1024 / 1025 above


def test_direct_block_cases_have_direct_blocks():
    """The 'stream-direct' case runs a streaming plan WITH direct blocks (header word [28] of a 'BSU2' plan, as tests/test_updat_direct_gpu.py reads
    it), the 'stream-nodirect' case the same layout's plan without: the two cannot quietly become one case."""
    from blocksparse_amd import lut as L
    from blocksparse_amd.matmul import _host_updat_plan
    U2_MAGIC, U2_DIRECT_WORD = 0x42535532, 28
    for c in T.CASES:
        if "stream-direct" not in c.id and "stream-nodirect" not in c.id:
            continue
        lay = T.layouts(c.lay)
        opts = 0
        for o in c.opts:
            opts |= getattr(_lib, o)
        t = L.build_tables(lay, z_order=True, segmented=False)
        hp = _host_updat_plan(t["updat_lut"], t["blocks"], t["CB"], t["KB"], c.bs, _lib.BF16, c.axis, opts)
        assert hp is not None and int(hp[0]) == U2_MAGIC
        assert (int(hp[U2_DIRECT_WORD]) > 0) == ("stream-direct" in c.id), (c.id, int(hp[U2_DIRECT_WORD]))
