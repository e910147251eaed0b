"""The route table of tests/conv_edges.py on a machine without a device: the host path of lotus_subm_conv /
lotus_subm_conv_wgrad runs to the kernel launch with host pointers, fails there (LOTUS_E_LAUNCH) and has recorded by then which
kernel it chose.  Every row is called with buffers of the sizes and alignments, the workspace and the options the GPU tests
use, so the routes those tests assert are pinned before any of them runs; the refusals must return before a route is noted."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_edges as ce
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, ops

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="launches with host pointers: only meaningful (and safe) without a device")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib()


def _host(nbytes):
    """-> (keep-alive array, 16-byte aligned address) of nbytes zero bytes."""
    a = np.zeros(nbytes // 4 + 8, dtype=np.float32)
    addr = a.ctypes.data
    return a, addr + (-addr) % 16


def _route(L, entry="lotus_conv_last_route"):
    out = (ctypes.c_int * 8)()
    assert L.fn[entry](ctypes.addressof(out)) == 0
    return tuple(out)


def call_on_host(L, row):
    sc = ce.scene(row.scene)
    keep, ptr = [sc.nbr], {"nbr": sc.nbr.ctypes.data}
    for name, (rows, cols, _, kind) in ce.buffers(row).items():
        a, ptr[name] = _host(rows * cols * (2 if (row.opts.get("b16") and kind == "act") else 4))
        keep.append(a)
    if "dwdb" in ptr:
        ptr["dwdb_db"] = ptr["dwdb"] + 4 * row.cout * row.T * row.cin
    ri = ce.rowidx_of(row)
    if ri is not None:
        keep.append(ri)
        ptr["rowidx"] = ri.ctypes.data
    if row.opts.get("tap_plan"):
        a, ptr["tap_plan"] = _host(4 * L.fn["lotus_fe_tap_plan_ints"](sc.n))
        keep.append(a)
    nbytes = ce.workspace_bytes(row, lambda name, *a: L.fn[name](*a))
    ws = None
    if nbytes:
        a, ws = _host(nbytes)
        keep.append(a)
    if row.call == "transpose":
        return L.fn["lotus_conv_weight_transpose"](ptr["w"], _host(8 * row.cout * row.T * row.cin)[1], row.cout, row.T, row.cin, 0, None)
    return L.fn[ce.entry(row)](*ce.arguments(row, ptr, ws, nbytes), None)


def wrong_routes(L, rows, environ):
    bad = []
    for row in rows:
        rc = call_on_host(L, row)
        got, want = _route(L, ce.entry(row, "lotus_conv_last_route")), tuple(ce.expected_route(row, environ))
        if rc != -2 or got != want:
            bad.append(f"{row.id}: rc {rc}, expected {want}, recorded {got}")
    return bad


@pytest.mark.parametrize("group", list(ce.GROUPS))
def test_every_row_of_the_table_takes_its_route(lib, group):
    rows = ce.GROUPS[group]
    assert rows
    bad = wrong_routes(lib, rows, {})
    assert not bad, "\n".join(bad[:20])


def test_the_table_holds_what_it_says():
    fam = lambda g: {r.route.family for r in ce.GROUPS[g]}  # noqa: E731
    assert fam("GENERIC") == {1} and fam("STEM") == {1, 2} and fam("PAIRS") == fam("OVERFLOW") == fam("PREC") == fam("OSF32") == {3}
    assert fam("OS") == {4} and fam("WGRAD") == {6, 7, 8} and fam("TWIN") == {1, 3, 4, 7}
    assert {r.route.aux for r in ce.STEM if r.route.family == 2} == {0, 4, 6, 7, 8}
    assert {(r.route.cols, r.route.nz) for r in ce.PAIRS} == {(c, z) for c in (64, 128) for z in (1, 3, 9)}
    assert {r.route.prec for r in ce.PREC} == {1, 3} and {(r.route.prec, r.route.aux) for r in ce.OS} == {(1, 64), (1, 128), (3, 64)}
    assert {r.route.nz for r in ce.OS} == {1, 3, 9} and all(r.opts["os0"].family == 3 for r in ce.OS) and all(r.opts["osf32"].family == 4 for r in ce.OSF32)
    assert {ce.scene(r.scene).n for r in ce.WGRAD if (r.cin, r.cout) == (32, 32) and r.scene.startswith("rand")} == set(ce.WG_ROWS)
    assert not [r for r in ce.WGRAD if r.opts["accumulate"] and r.route.aux], "accumulate never writes directly"
    assert {(r.route.nz, r.route.aux) for r in ce.WGRAD} == {(1, 1), (1, 0), (2, 0), (3, 0)}
    total4 = {3 * k % 8 for k in range(1, 8)}
    assert total4 == set(range(1, 8)) and len([r for r in ce.PAIRS if r.cout == 384]) == 7
    assert max(ce.scene(r.scene).n * max(r.cin, r.cout) for r in ce.TABLE) <= 98304 * 768 // 8


def test_refusals_return_before_a_route_is_noted(lib):
    ok = ce.BY_ID["a-fwd-n65-64x64-no_wt"]
    assert call_on_host(lib, ok) == -2
    before = _route(lib)
    assert before == tuple(ok.route)
    for row in ce.REFUSE:
        assert call_on_host(lib, row) == row.opts["refuse"], (row.id, lib.last_error())
        assert _route(lib) == before, row.id
    assert lib.fn["lotus_conv_last_route"](None) == -1


def test_the_record_has_a_twin_and_names(lib):
    row = ce.BY_ID["f-wgrad-rand_1025_27_30-32x32-acc0_dbtail"]
    assert call_on_host(lib, row) == -2
    r = ops.last_conv_route()
    assert r == ops.ConvRoute(family=ops.CONV_WGRAD, mode=2, rows=64, cols=64, prec=0, nz=2, tpz=1024, aux=0)
    assert _route(lib, "lotus_b16_conv_last_route") == tuple(r)
    n0 = ce.BY_ID["a-fwd-n65-64x64-no_wt"]
    sc = ce.scene(n0.scene)
    args = list(ce.arguments(n0, {k: 16 for k in ("x", "w", "y", "nbr")}, None, 0))
    args[9] = 0      # n == 0: nothing is launched, the record stays
    assert lib.fn["lotus_subm_conv"](*args, None) == 0 and tuple(ops.last_conv_route()) == tuple(r) and sc.n == 65


@pytest.mark.parametrize("env,group", [("OS_ENV", "OS"), ("OSF32_ENV", "OSF32")])
def test_routes_under_the_documented_switches(lib, env, group):
    """LOTUS_CONV_OS=0 / LOTUS_CONV_OS_F32=1 are read once per process: a fresh interpreter per switch."""
    code = ("import sys; sys.path[:0] = %r\nimport conv_edges as ce, test_conv_routes_host as h\nfrom robot_3dlotus_amd import _capi\n"
            "bad = h.wrong_routes(_capi.lib(), ce.GROUPS[%r], ce.%s)\nassert not bad, bad[:10]\nprint('rows ok', len(ce.GROUPS[%r]))\n"
            ) % ([os.path.dirname(HERE), HERE], group, env, group)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **getattr(ce, env)))
    assert r.returncode == 0 and "rows ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
