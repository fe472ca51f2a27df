"""CPU tier of the tensor-list weight update (include/bsmm_optim_list.h): the exported symbols, the struct mirrors, the table builder on
dummy addresses (a host function: nothing it rejects or accepts is ever launched) and the null checks of the launch functions, which
answer before any launch.  No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUP, WS = -1, -2, -3
ROW_BYTES = 96                      # one packed row of the table: the 88 bytes of bsmm_opt_tensor, the access paths, padding to 16
SS_SLOTS = 1024                     # OPT_SS_SLOTS: the per-tensor workgroup cap of the sum of squares
CUS = 256                           # compute units of the MI355X: the caps are workgroups per CU times this


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_optim_list.h")).read()


def test_list_header_symbols_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.OPTIM_LIST_SYMBOLS), declared ^ set(lib.OPTIM_LIST_SYMBOLS)
    assert len(lib.OPTIM_LIST_SYMBOLS) == 6
    for other in (lib.SYMBOLS, lib.DIST_SYMBOLS, lib.SPARSITY_SYMBOLS, lib.OPTIM_SYMBOLS, lib.BST_SYMBOLS):
        assert not declared & set(other)
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION          # new symbols only: bsmm.h and its version stay as they were


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    lines = [ln for ln in body.splitlines() if ";" in ln]
    names = [re.search(r"(\w+)\s*;", ln).group(1) for ln in lines]
    kinds = {"ptr": 0, "size_t": 0, "int32_t": 0, "float": 0}
    for ln in lines:
        kinds["ptr" if "*" in ln else re.search(r"(size_t|int32_t|float)", ln).group(1)] += 1
    return names, kinds


def test_struct_layouts_match_the_header(lib):
    names, kinds = _fields("bsmm_opt_tensor")
    assert names == [f[0] for f in lib.BsmmOptTensor._fields_]
    assert kinds == {"ptr": 8, "size_t": 1, "int32_t": 4, "float": 0}
    assert ctypes.sizeof(lib.BsmmOptTensor) == 8 * 8 + 8 + 4 * 4
    assert lib.BsmmOptTensor.ema.offset == 56 and lib.BsmmOptTensor.size.offset == 64 and lib.BsmmOptTensor.ema_dtype.offset == 84
    names, kinds = _fields("bsmm_opt_list")
    assert names == [f[0] for f in lib.BsmmOptList._fields_]
    assert kinds == {"ptr": 0, "size_t": 1, "int32_t": 4, "float": 0}
    assert ctypes.sizeof(lib.BsmmOptList) == 24 and lib.BsmmOptList.count.offset == 8 and lib.BsmmOptList.sum_squared_grid.offset == 20
    names, kinds = _fields("bsmm_opt_state")
    assert names == [f[0] for f in lib.BsmmOptState._fields_] == ["step", "lr_t", "lr_new_t", "reserved"]
    assert kinds == {"ptr": 0, "size_t": 0, "int32_t": 2, "float": 2}
    assert ctypes.sizeof(lib.BsmmOptState) == 16 and lib.BsmmOptState.lr_t.offset == 4 and lib.BsmmOptState.lr_new_t.offset == 8
    names, kinds = _fields("bsmm_adam_settings")
    assert names == [f[0] for f in lib.BsmmAdamSettings._fields_]
    assert kinds == {"ptr": 0, "size_t": 0, "int32_t": 2, "float": 6}
    assert ctypes.sizeof(lib.BsmmAdamSettings) == 32 and lib.BsmmAdamSettings.saturate.offset == 20 and lib.BsmmAdamSettings.zero_infs.offset == 24


def test_list_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_optim_list.hip", "bsmm_optim_list_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    # the per-tensor kernels' header holds the one body of every loop and the arithmetic it calls; the list sources call the bodies
    kern = open(os.path.join(ROOT, "blocksparse_amd", "csrc", "bsmm_optim_kernels.h")).read()
    assert '#include "bsmm_optim_kernels.h"' in src
    for body in ("opt_adam_row", "opt_ema_row", "opt_sum_squared_row"):
        assert kern.count("void %s(" % body) == 1 and "void %s(" % body not in src and body + "<" in src, body
    assert "adam_elem(" in kern and "ema_elem(" in kern and "opt_group_sum(" in kern
    assert "sqrtf" not in src and "adam_elem(" not in src and "ema_elem(" not in src      # the arithmetic is called, not restated
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "hipMemcpy", "Synchronize", "atomic", "static "):
        assert word not in src, word
    build = open(os.path.join(ROOT, "blocksparse_amd", "build.py")).read()
    assert "bsmm_optim_list.hip" in build and "bsmm_optim_list.h" in build


def _row(lib, **kw):
    r = dict(param=256, mean=512, var=768, grad=1024, size=4 * 1024, bsize=32, grad_dtype=lib.F32)
    r.update(kw)
    return r


def _build(lib, rows, count=None, nbytes=None):
    """(code, info, table bytes) of bsmm_opt_list_build over `rows` (dicts of bsmm_opt_tensor fields)."""
    L = lib.load()
    arr = (lib.BsmmOptTensor * max(len(rows), 1))()
    for a, r in zip(arr, rows):
        for k, v in r.items():
            setattr(a, k, v)
    count = len(rows) if count is None else count
    need = int(L.bsmm_opt_list_bytes(len(rows)))
    buf = (ctypes.c_ubyte * max(need, 16))(*([0xAB] * max(need, 16)))
    info = lib.BsmmOptList()
    rc = L.bsmm_opt_list_build(arr, count, buf, need if nbytes is None else nbytes, ctypes.byref(info))
    return rc, info, bytes(buf)[:need]


def test_build_rejects_what_the_per_tensor_calls_reject(lib):
    L = lib.load()
    good = _row(lib)
    defects = [(dict(param=None), ARG), (dict(mean=None), ARG), (dict(var=None), ARG), (dict(grad=None), ARG),
               (dict(size=0), ARG),
               (dict(size=4 * 1024 + 8), ARG), (dict(size=63, bsize=8), ARG),                 # no multiple of bsize^2
               (dict(bsize=0, gate=256), ARG), (dict(bsize=0, lr_select=256), ARG),           # a flat row takes neither
               (dict(bsize=12, size=144), UNSUP), (dict(bsize=-8), UNSUP),
               (dict(grad_dtype=3), UNSUP),
               (dict(param16=256, param16_dtype=lib.F32), UNSUP), (dict(param16=256, param16_dtype=9), UNSUP),
               (dict(ema=256, ema_dtype=5), UNSUP)]
    for kw, want in defects:
        # the same defect through the per-tensor entry point: the same code (stream NULL, never reached)
        a = lib.BsmmAdamArgs()
        for k, v in _row(lib, **kw).items():
            if k not in ("ema", "ema_dtype"):
                setattr(a, k, v)
        a.lr, a.beta1, a.beta2, a.epsilon, a.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 1.0
        if "ema" in kw:
            assert L.bsmm_ema(256, 256, None, 0.99, 4 * 1024, 32, kw["ema_dtype"], None) == want
        else:
            assert L.bsmm_adam(ctypes.byref(a)) == want, kw
        for pos in (0, 2):                                  # the defective row first and last of three
            rows = [dict(good), dict(good), dict(good)]
            rows[pos] = _row(lib, **kw)
            rc, info, table = _build(lib, rows)
            assert rc == want, (kw, pos, rc)
            assert info.count == 0 and info.adam_grid == 0 and info.table_bytes == 0          # nothing to launch with
            assert table == b"\xab" * len(table)                                                # and no table written
    assert _build(lib, [good], count=0)[0] == ARG and _build(lib, [good], count=-3)[0] == ARG
    need = int(L.bsmm_opt_list_bytes(1))
    assert _build(lib, [good], nbytes=need - 1)[0] == WS and _build(lib, [good], nbytes=0)[0] == WS
    info = lib.BsmmOptList()
    arr = (lib.BsmmOptTensor * 1)()
    buf = (ctypes.c_ubyte * need)()
    assert L.bsmm_opt_list_build(None, 1, buf, need, ctypes.byref(info)) == ARG
    assert L.bsmm_opt_list_build(arr, 1, None, need, ctypes.byref(info)) == ARG                  # (an all-zero row: null param)
    assert L.bsmm_opt_list_build(arr, 1, buf, need, None) == ARG
    assert L.bsmm_opt_list_bytes(0) == 0 and L.bsmm_opt_list_bytes(-1) == 0
    last = 0
    for cnt in (1, 2, 3, 7, 48, 70, 1000):
        b = L.bsmm_opt_list_bytes(cnt)
        assert b > last and b % 16 == 0 and b >= cnt * ROW_BYTES + 3 * (cnt + 1) * 4
        last = b


def _prefixes(table, count):
    import numpy as np
    p = np.frombuffer(table, dtype=np.int32, offset=count * ROW_BYTES, count=3 * (count + 1)).reshape(3, count + 1)
    return p


def test_table_of_a_mixed_list(lib):
    """Workgroups per row and stage: what the per-tensor launches use as their grids.  Sum of squares: min(1024, ceil(ceil(size / W) / 256))
    with W = 4 (fp32) / 8 (16-bit) on the 16-byte path and 1 on the element path; Adam and the average (cap 2048):
    min(cap, ceil(ceil(size / 4) / 256)) on the 16-byte path, ceil(size / 256) capped likewise on the element path, nothing for a row
    without an average.  The Adam stage's cap is a tuning choice of the library (whole workgroups per CU, at most the 8 of the per-tensor
    launch): it is read off the largest row here, not pinned."""
    import numpy as np
    big = 1024 * 256 * 4 + 1027
    A = 1 << 20                                             # an aligned dummy base; + 4: one fp32 element off
    rows = [
        _row(lib, size=1, bsize=0),
        _row(lib, size=63, bsize=0, grad_dtype=lib.BF16, ema=A, ema_dtype=lib.F16),
        _row(lib, size=4097, bsize=0, grad_dtype=lib.F16, grad=A + 2, ema=A, ema_dtype=lib.F32),            # a misaligned 16-bit grad
        _row(lib, size=37 * 64 * 64, bsize=64, grad_dtype=lib.BF16, gate=A, param16=A, param16_dtype=lib.BF16, ema=A + 4, ema_dtype=lib.F32),
        _row(lib, size=big, bsize=0, ema=A, ema_dtype=lib.BF16),
        _row(lib, size=big, bsize=0, param=A + 4, ema=A, ema_dtype=lib.BF16),                                # param off: Adam and the average by element
        _row(lib, size=37 * 64, bsize=8, grad_dtype=lib.F16, param16=A + 2, param16_dtype=lib.F16),          # only the working copy off
    ]
    rc, info, table = _build(lib, rows)
    assert rc == 0 and info.count == len(rows) and info.table_bytes == len(table) == lib.load().bsmm_opt_list_bytes(len(rows))
    ceil = lambda a, b: -(-a // b)
    pre = _prefixes(table, len(rows))
    adam_cap = int(pre[0][6] - pre[0][5])                   # the row of 4100 element-path lane-steps: it has what a row can have at most
    assert adam_cap % CUS == 0 and 1 <= adam_cap // CUS <= 8, adam_cap
    want_ss, want_adam, want_ema = [], [], []
    for r in rows:
        w16 = 4 if r["grad_dtype"] == lib.F32 else 8
        W = w16 if r["grad"] % 16 == 0 else 1
        want_ss.append(min(SS_SLOTS, ceil(ceil(r["size"], W), 256)))
        vec = all(r.get(k, 0) % 16 == 0 for k in ("param", "mean", "var", "grad", "param16"))
        want_adam.append(min(adam_cap, ceil(ceil(r["size"], 4 if vec else 1), 256)))
        vec = r["param"] % 16 == 0 and r.get("ema", 0) % 16 == 0
        want_ema.append(min(2048, ceil(ceil(r["size"], 4 if vec else 1), 256)) if r.get("ema") else 0)
    assert want_ss == [1, 1, 17, 74, 1024, 1024, 2] and want_ema[0] == 0 and want_adam[4] == min(adam_cap, 1026) and want_adam[6] == 10      # (the cases meant)
    assert np.diff(pre[0]).tolist() == want_adam and np.diff(pre[1]).tolist() == want_ema and np.diff(pre[2]).tolist() == want_ss
    assert pre[:, 0].tolist() == [0, 0, 0]
    assert (info.adam_grid, info.ema_grid, info.sum_squared_grid) == (sum(want_adam), sum(want_ema), sum(want_ss))
    # the rows: the caller's fields, bit for bit
    for i, r in enumerate(rows):
        got = lib.BsmmOptTensor.from_buffer_copy(table[i * ROW_BYTES:i * ROW_BYTES + ctypes.sizeof(lib.BsmmOptTensor)])
        for k, v in r.items():
            assert getattr(got, k) == v, (i, k)
    # no row with an average at all: the stage has no workgroups
    rc, info, _t = _build(lib, [_row(lib), _row(lib, size=5, bsize=0)])
    assert rc == 0 and info.ema_grid == 0 and info.adam_grid == 5 and info.sum_squared_grid == 5


def test_launch_functions_check_their_arguments_before_any_launch(lib):
    L = lib.load()
    rc, info, _table = _build(lib, [_row(lib, ema=256, ema_dtype=lib.F32)])
    assert rc == 0
    pinfo = ctypes.byref(info)
    one = ctypes.c_void_p(256)                              # a non-null, aligned dummy address: never dereferenced
    s = lib.BsmmAdamSettings()
    ps = ctypes.byref(s)
    need = L.bsmm_sum_squared_workspace_bytes(1)
    assert L.bsmm_opt_advance(None, one, None, 0.9, 0.999, 0, None) == ARG
    assert L.bsmm_opt_advance(one, None, None, 0.9, 0.999, 0, None) == ARG
    assert L.bsmm_opt_advance(ctypes.c_void_p(258), one, None, 0.9, 0.999, 0, None) == ARG
    assert L.bsmm_adam_list(None, one, one, None, ps, None) == ARG
    assert L.bsmm_adam_list(pinfo, None, one, None, ps, None) == ARG
    assert L.bsmm_adam_list(pinfo, one, None, None, ps, None) == ARG
    assert L.bsmm_adam_list(pinfo, one, one, None, None, None) == ARG
    assert L.bsmm_adam_list(pinfo, ctypes.c_void_p(260), one, None, ps, None) == ARG           # a table off its 16 bytes
    assert L.bsmm_ema_list(None, one, 0.99, None) == ARG
    assert L.bsmm_ema_list(pinfo, None, 0.99, None) == ARG
    assert L.bsmm_sum_squared_list(None, one, 1.0, 0.0, 0, 0, one, need, None) == ARG
    assert L.bsmm_sum_squared_list(pinfo, None, 1.0, 0.0, 0, 0, one, need, None) == ARG
    assert L.bsmm_sum_squared_list(pinfo, one, 1.0, 0.0, 0, 0, None, need, None) == WS
    assert L.bsmm_sum_squared_list(pinfo, one, 1.0, 0.0, 0, 0, one, need - 1, None) == WS
    blank = lib.BsmmOptList()                               # a descriptor no build has filled
    assert L.bsmm_adam_list(ctypes.byref(blank), one, one, None, ps, None) == ARG
    assert L.bsmm_ema_list(ctypes.byref(blank), one, 0.99, None) == ARG
    assert L.bsmm_sum_squared_list(ctypes.byref(blank), one, 1.0, 0.0, 0, 0, one, need, None) == ARG


def test_public_surface():
    import inspect
    import blocksparse_amd
    from blocksparse_amd import AdamOptimizer, PreparedStep
    assert list(inspect.signature(AdamOptimizer.prepare).parameters)[:6] == ["self", "grads", "clip_norm", "ema", "lr_select", "lr_new"]
    for name in ("run", "rates", "sync_host"):
        assert callable(getattr(PreparedStep, name)), name
    assert blocksparse_amd.optimize.PreparedStep is PreparedStep


def test_adam_stage_cap_fits_what_a_cu_admits(lib):
    """A row's workgroups in the Adam stage are meant to be resident together.  A CU admits min(8, floor(512 / vgprs), floor(800 / (ceil16(sgprs)
    + 16))) workgroups of 256 threads (four waves, one per SIMD; the scalar-register term is the measured admission rule of the MI355X): the cap
    the builder uses, read off a table, must not exceed that for the kernel as built."""
    import _codeobj as C
    import numpy as np
    meta = C.kernel_metadata(lib.LIB_PATH)
    mine = [k for n, k in meta.items() if "opt_adam_list_kernel" in n]
    assert len(mine) == 1
    vgpr = mine[0].get(".vgpr_count", 0) + mine[0].get(".agpr_count", 0)
    sgpr = mine[0].get(".sgpr_count", 0)
    admitted = min(8, 512 // (-(-vgpr // 8) * 8), 800 // (-(-sgpr // 16) * 16 + 16))
    rc, info, table = _build(lib, [_row(lib, size=4096 * 4096, bsize=0)])
    assert rc == 0
    cap = int(np.diff(_prefixes(table, 1)[0])[0])
    assert cap % CUS == 0 and 1 <= cap // CUS <= admitted, (cap, vgpr, sgpr, admitted)
