"""The route table of tests/dense_edges.py on a machine without a device: the host path of a dense entry point runs to the
kernel launch with host pointers, fails there (LOTUS_E_LAUNCH) and has recorded by then which kernel it chose.  Every row of
the table is called with buffers of the sizes, alignments and options the GPU tests use, so the routes those tests assert
are pinned before any of them runs."""
import ctypes

import numpy as np
import pytest
import torch

import dense_edges as de
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, ops

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="launches with host pointers: only meaningful (and safe) without a device")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib()


def _host(n, off4=False):
    """-> (keep-alive array, address) of n floats, 16-byte aligned or 4 bytes past that."""
    a = np.zeros(n + 8, dtype=np.float32)
    addr = a.ctypes.data
    addr += (-addr) % 16 + (4 if off4 else 0)
    return a, addr


def _route(L, entry="lotus_dense_last_route"):
    out = (ctypes.c_int * 8)()
    assert L.fn[entry](ctypes.addressof(out)) == 0
    return tuple(out)


def call_on_host(L, case):
    keep, ptr = [], {}
    for name, (rows, cols, _) in de.buffers(case).items():
        a, addr = _host(rows * cols, off4=(name == de.misaligned(case)))
        keep.append(a)
        ptr[name] = addr
    if "dwdb" in ptr:
        ptr["dwdb_db"] = ptr["dwdb"] + 4 * case.N * case.K
    ws = ws_bytes = None
    q = de.workspace_query(case)
    if q:
        ws_bytes = L.fn[de.entry(case, q[0])](*q[1])
        a, ws = _host(ws_bytes // 4 + 4)
        keep.append(a)
    a, cnt = _host(L.fn["lotus_splitk_counters_bytes"]() // 4)
    keep.append(a)
    ln_ws = ln_bytes = nparts = None
    if case.call == "dgrad_ln":
        ln_bytes = L.fn["lotus_layernorm_bwd_workspace"](case.M, case.K)
        a, ln_ws = _host(ln_bytes // 4 + 4)
        nparts = np.zeros(1, dtype=np.int32)
        keep += [a, nparts]
    args = de.arguments(case, ptr, ws, ws_bytes or 0, cnt, ln_ws, ln_bytes or 0, None if nparts is None else nparts.ctypes.data)
    rc = L.fn[de.entry(case)](*args, None)
    return rc, _route(L, de.entry(case, "lotus_dense_last_route")), nparts


@pytest.mark.parametrize("group", ["GRID", "SPLIT", "WGRAD", "PRECISION", "DMA", "FEW", "TAIL", "TWIN", "BOUNDS"])
def test_every_row_of_the_table_takes_its_route(lib, group):
    cases = getattr(de, group)
    assert cases
    wrong = []
    for case in cases:
        rc, got, nparts = call_on_host(lib, case)
        assert rc == -2, (case.id, rc, lib.last_error())
        if got[:7] != tuple(de.default_route(case)):
            wrong.append((case.id, tuple(de.default_route(case)), got))
        if "depth" in case.opts and got[7] != case.opts["depth"]:
            wrong.append((case.id, "ring depth %d" % case.opts["depth"], got))
        if case.opts.get("ln_fused"):
            assert int(nparts[0]) == (case.M + 127) // 128, case.id
    assert not wrong, "\n".join(f"{i}: expected {e}, recorded {g}" for i, e, g in wrong[:20])


def test_the_table_holds_what_it_says():
    """The rows the table promises are there: both calls on every (rows, pair), the split shapes with and without counters, the
    weight-gradient variants on every route, the smallest routed LDS-DMA shapes."""
    assert len(de.GRID) == 2 * (len(de.PAIRS) * len(de.ROWS) * 2 + 4 * len(de.ROWS))
    assert {c.route.nz for c in de.SPLIT} == {1, 2, 4, 16} and {c.route.fused for c in de.SPLIT} == {0, 1}
    assert not [c for c in de.SPLIT if c.route.fused and not c.route.fast]
    acc = [c for c in de.WGRAD if c.opts.get("accumulate")]
    assert {(min(c.route.nz, 8), c.route.fused) for c in acc if c.route.fast} == {(1, 0), (2, 1), (4, 1), (8, 0), (2, 0), (4, 0)}
    assert {(c.route.bm, c.route.bn) for c in de.DMA if c.call == "wgrad"} == {(128, 128), (128, 64), (64, 128), (64, 64)}
    assert all(c.route.family == 2 for c in de.DMA + de.FEW) and all(c.route.family == 1 for c in de.GRID + de.SPLIT + de.WGRAD + de.PRECISION + de.TAIL + de.TWIN)
    assert all(de.default_route(c).family == 1 for c in de.FEW)
    assert {(c.call, c.M, c.opts["prec"]) for c in de.TWIN if c.M != 228 and c.route.fast} == {(call, m, p) for call in ("fwd", "dgrad", "wgrad") for m in (5, 64, 65) for p in (0, 1)}
    # BOUNDS: for both calls the grid of 64 x 64 output tiles exactly on each of gemm_kernel's three thresholds and the first
    # grid past it (one more row tile or one more column tile); the twin's ring threshold on both sides for every call
    for call in ("fwd", "dgrad"):
        grids = {(-(-c.M // 64), -(-(c.N if call == "fwd" else c.K) // 64)) for c in de.BOUNDS if c.call == call and not c.opts.get("b16")}
        for t in (512, 2048, 8192):
            on = {g for g in grids if g[0] * g[1] == t}
            assert on and any((r + 1, c) in grids or (r, c + 1) in grids for r, c in on), (call, t)
    assert {(c.call, c.M) for c in de.BOUNDS if c.opts.get("b16")} == {(call, m) for call in ("fwd", "dgrad", "wgrad") for m in (8192, 8193)}
    assert not set(c.id for c in de.BOUNDS) & set(de.BY_ID)


def test_the_record_is_the_last_product_and_has_a_twin(lib):
    """An entry point that launches several products leaves the last one; ops.last_dense_route names the fields; the
    bf16-storage twin reads the same record."""
    a, x = _host(100 * 64)
    b, w = _host(32 * 64)
    c, y = _host(100 * 32)
    rc = lib.fn["lotus_linear_fwd"](x, w, None, None, y, None, 100, 32, 64, 0, 0.0, 0, 0, None, 0, None, None)
    assert rc == -2
    r = ops.last_dense_route()
    assert r == ops.DenseRoute(family=ops.FAMILY_GEMM, bm=64, bn=64, bk=64, nz=1, fast=1, fused=0, depth=2)
    assert _route(lib, "lotus_b16_dense_last_route") == tuple(r)
    assert lib.fn["lotus_dense_last_route"](None) == -1


def test_few_rows_routes_under_the_documented_switches(lib):
    """The FEW rows in a fresh interpreter with de.FEW_ENV (the thresholds are read once per process): every one on
    gemm_dma_kernel, weight gradients fused over four (two) ranges."""
    import os
    import subprocess
    import sys

    code = ("import sys; sys.path[:0] = %r\nimport dense_edges as de, test_dense_routes_host as h\n"
            "from robot_3dlotus_amd import _capi\nL = _capi.lib()\n"
            "bad = [(c.id, tuple(c.route), r) for c in de.FEW for rc, r, _ in [h.call_on_host(L, c)] if rc != -2 or r[:7] != tuple(c.route)]\n"
            "assert not bad, bad[:10]\nprint('few rows ok', len(de.FEW))\n") % ([os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             os.path.dirname(os.path.abspath(__file__))],)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **de.FEW_ENV))
    assert r.returncode == 0 and "few rows ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
