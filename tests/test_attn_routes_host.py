"""The attention dispatch on a machine without a device: the host path of lotus_attention_fwd / _bwd (and the lotus_b16_ twins)
runs to the kernel launch with host pointers, fails there (LOTUS_E_LAUNCH) and has recorded by then which kernel it chose
(lotus_attention_last_route; fields in include/lotus_hip.h).  Every row below is a call and the literal record it must leave,
written down from the rules of the dispatch and not computed by it:

  no q/k norm      always the tile kernels, attn_fwd_kernel<0, false> / attn_bwd2_kernel<false>; no norm-gradient reduction
  query per lane   d in {32, 24, 16}, no atomic accumulation, and a short key side (0 < k_max <= 32) unless LOTUS_XQ=0, or a
                   long / unknown one at precision 0 with fp32 storage under LOTUS_XQ=2.  xq2_*_kernel<4> iff d == 32, short,
                   no owner flags, no borrowed rows (backward) and LOTUS_XQ != 3; else xq_*_kernel<d>.  Reported precision: 0.
  otherwise tiles  precision 3 / 1: attn_fwd_kernel<3 | 1>, attn_bwd_kernel<3 | 1>; any other value, 5 included:
                   attn_fwd_kernel<0>, attn_bwd2_kernel<true>
  backward tail    bit 0 (fix-up) iff borrowed rows with a side buffer, bit 1 (norm-gradient reduction) iff with the norm

The sizes are the smallest valid ones (H = 2, one tile, one block, one query and one key): no buffer is ever read on the host."""
import collections
import concurrent.futures
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, ops

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="launches with host pointers: only meaningful (and safe) without a device")
HERE = os.path.dirname(os.path.abspath(__file__))
H = 2
FWD_LDS, BWD_LDS = 53760, 72192  # dynamic LDS of the tile kernels: three / four [128][33] row images + the small arrays

# a call: direction, twin (bf16 storage), head width, k_max, precision, owner flags, borrowed rows, q/k norm, atomic_out
Call = collections.namedtuple("Call", "bwd b16 d k_max precision owner extra norm atomic_out", defaults=(0, False, False, 1, 0))
R = ops.AttnRoute


def fwd(d, k_max, precision=0, **kw):
    return Call(0, kw.pop("b16", False), d, k_max, precision, **kw)


def bwd(d, k_max, precision=0, **kw):
    return Call(1, kw.pop("b16", False), d, k_max, precision, **kw)


# family, direction, targ, precision, norm, threads, lds_bytes, tail
ROWS = [
    # ---- forward, with the norm: the key side decides (k_max 0 = unknown, 1 and 32 short, 33 and 78 long)
    (fwd(32, 0), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    (fwd(32, 1), R(5, 0, 4, 0, 1, 256, 0, 0)),
    (fwd(32, 32), R(5, 0, 4, 0, 1, 256, 0, 0)),
    (fwd(32, 33), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    (fwd(32, 78), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    (fwd(32, 32, owner=True), R(4, 0, 32, 0, 1, 128, 0, 0)),
    (fwd(24, 32), R(4, 0, 24, 0, 1, 128, 0, 0)),
    (fwd(24, 1, owner=True), R(4, 0, 24, 0, 1, 128, 0, 0)),
    (fwd(16, 1), R(4, 0, 16, 0, 1, 128, 0, 0)),
    (fwd(16, 33), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    (fwd(8, 32), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    # the query-per-lane kernels are exact fp32 whatever `precision` says
    (fwd(32, 32, 1), R(5, 0, 4, 0, 1, 256, 0, 0)),
    (fwd(32, 32, 3), R(5, 0, 4, 0, 1, 256, 0, 0)),
    (fwd(32, 32, 5), R(5, 0, 4, 0, 1, 256, 0, 0)),
    (fwd(24, 32, 3), R(4, 0, 24, 0, 1, 128, 0, 0)),
    # the tile kernels take their operand mode from it
    (fwd(32, 0, 1), R(1, 0, 0, 1, 1, 256, FWD_LDS, 0)),
    (fwd(32, 0, 3), R(1, 0, 0, 3, 1, 256, FWD_LDS, 0)),
    (fwd(32, 0, 5), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    (fwd(8, 32, 3), R(1, 0, 0, 3, 1, 256, FWD_LDS, 0)),
    (fwd(24, 78, 1, owner=True), R(1, 0, 0, 1, 1, 256, FWD_LDS, 0)),
    # ---- forward without the norm: the tile kernel whatever k_max says
    (fwd(32, 0, norm=0), R(1, 0, 0, 0, 0, 256, FWD_LDS, 0)),
    (fwd(32, 32, norm=0), R(1, 0, 0, 0, 0, 256, FWD_LDS, 0)),
    (fwd(16, 1, norm=0, owner=True), R(1, 0, 0, 0, 0, 256, FWD_LDS, 0)),
    # ---- backward, with the norm
    (bwd(32, 0), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
    (bwd(32, 0, 1), R(2, 1, 0, 1, 1, 256, BWD_LDS, 2)),
    (bwd(32, 0, 3), R(2, 1, 0, 3, 1, 256, BWD_LDS, 2)),
    (bwd(32, 0, 5), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
    (bwd(32, 0, owner=True, extra=True), R(3, 1, 0, 0, 1, 256, BWD_LDS, 3)),
    (bwd(32, 0, 3, owner=True, extra=True), R(2, 1, 0, 3, 1, 256, BWD_LDS, 3)),
    (bwd(32, 1), R(5, 1, 4, 0, 1, 256, 0, 2)),
    (bwd(32, 32), R(5, 1, 4, 0, 1, 256, 0, 2)),
    (bwd(32, 33), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
    (bwd(32, 78, 1), R(2, 1, 0, 1, 1, 256, BWD_LDS, 2)),
    (bwd(32, 32, 1), R(5, 1, 4, 0, 1, 256, 0, 2)),
    (bwd(32, 32, 3), R(5, 1, 4, 0, 1, 256, 0, 2)),
    (bwd(32, 32, 5), R(5, 1, 4, 0, 1, 256, 0, 2)),
    (bwd(32, 32, owner=True), R(4, 1, 32, 0, 1, 128, 0, 2)),
    (bwd(32, 32, extra=True), R(4, 1, 32, 0, 1, 128, 0, 3)),      # borrowed rows move xq2 -> xq<32> and set the tail
    (bwd(24, 32), R(4, 1, 24, 0, 1, 128, 0, 2)),
    (bwd(24, 1, 3, owner=True), R(4, 1, 24, 0, 1, 128, 0, 2)),
    (bwd(16, 32, extra=True), R(4, 1, 16, 0, 1, 128, 0, 3)),
    (bwd(8, 32), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
    (bwd(8, 32, 1), R(2, 1, 0, 1, 1, 256, BWD_LDS, 2)),
    (bwd(32, 32, atomic_out=1), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),     # atomic accumulation: never the query-per-lane kernels
    (bwd(24, 32, 3, atomic_out=1), R(2, 1, 0, 3, 1, 256, BWD_LDS, 2)),
    # ---- backward without the norm: no reduction; the fix-up iff borrowed rows
    (bwd(32, 0, norm=0), R(3, 1, 0, 0, 0, 256, BWD_LDS, 0)),
    (bwd(32, 32, norm=0), R(3, 1, 0, 0, 0, 256, BWD_LDS, 0)),
    (bwd(16, 0, norm=0, owner=True, extra=True), R(3, 1, 0, 0, 0, 256, BWD_LDS, 1)),
    # ---- the bf16-storage twin: the same rules (precision 0 still means fp32 products)
    (fwd(32, 0, 1, b16=True), R(1, 0, 0, 1, 1, 256, FWD_LDS, 0)),
    (fwd(32, 0, 0, b16=True), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
    (fwd(32, 32, 1, b16=True), R(5, 0, 4, 0, 1, 256, 0, 0)),
    (fwd(16, 32, 1, b16=True, owner=True), R(4, 0, 16, 0, 1, 128, 0, 0)),
    (bwd(32, 0, 1, b16=True), R(2, 1, 0, 1, 1, 256, BWD_LDS, 2)),
    (bwd(32, 0, 3, b16=True, owner=True, extra=True), R(2, 1, 0, 3, 1, 256, BWD_LDS, 3)),
    (bwd(32, 0, 0, b16=True), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
    (bwd(32, 32, 1, b16=True), R(5, 1, 4, 0, 1, 256, 0, 2)),
    (bwd(24, 32, 1, b16=True, owner=True), R(4, 1, 24, 0, 1, 128, 0, 2)),
]

# LOTUS_XQ is read once per process: the rows that differ under each value, and (last of each list) one that does not
XQ_ROWS = {
    "0": [  # tile kernels everywhere
        (fwd(32, 32), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
        (fwd(24, 1, 3, owner=True), R(1, 0, 0, 3, 1, 256, FWD_LDS, 0)),
        (bwd(32, 32), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
        (bwd(16, 32, 1, extra=True), R(2, 1, 0, 1, 1, 256, BWD_LDS, 3)),
        (fwd(32, 32, 1, b16=True), R(1, 0, 0, 1, 1, 256, FWD_LDS, 0)),
        (bwd(32, 0, norm=0), R(3, 1, 0, 0, 0, 256, BWD_LDS, 0)),
    ],
    "2": [  # also a long / unknown key side at precision 0 with fp32 storage (never xq2: that needs a short one)
        (fwd(32, 0), R(4, 0, 32, 0, 1, 128, 0, 0)),
        (fwd(32, 78), R(4, 0, 32, 0, 1, 128, 0, 0)),
        (fwd(24, 33, owner=True), R(4, 0, 24, 0, 1, 128, 0, 0)),
        (bwd(32, 0, owner=True, extra=True), R(4, 1, 32, 0, 1, 128, 0, 3)),
        (bwd(16, 0), R(4, 1, 16, 0, 1, 128, 0, 2)),
        (fwd(8, 0), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
        (fwd(32, 0, 1), R(1, 0, 0, 1, 1, 256, FWD_LDS, 0)),
        (bwd(32, 0, 5), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
        (bwd(32, 0, atomic_out=1), R(3, 1, 0, 0, 1, 256, BWD_LDS, 2)),
        (fwd(32, 0, 0, b16=True), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
        (fwd(32, 0, norm=0), R(1, 0, 0, 0, 0, 256, FWD_LDS, 0)),
        (bwd(32, 0, norm=0, extra=True), R(3, 1, 0, 0, 0, 256, BWD_LDS, 1)),
        (bwd(32, 32), R(5, 1, 4, 0, 1, 256, 0, 2)),
    ],
    "3": [  # as the default, but the cross attention proper on xq_*_kernel<32>
        (fwd(32, 32), R(4, 0, 32, 0, 1, 128, 0, 0)),
        (bwd(32, 1, 3), R(4, 1, 32, 0, 1, 128, 0, 2)),
        (bwd(32, 32, 1, b16=True), R(4, 1, 32, 0, 1, 128, 0, 2)),
        (fwd(32, 33), R(1, 0, 0, 0, 1, 256, FWD_LDS, 0)),
        (bwd(24, 32), R(4, 1, 24, 0, 1, 128, 0, 2)),
    ],
}


# The library's error string and the route record are per thread.  Every call here fails on purpose, so the tests run on a worker
# thread of their own: the error string of pytest's thread stays as the other test modules expect to find it.
_WORKER = concurrent.futures.ThreadPoolExecutor(max_workers=1)


def on_worker(test):
    @functools.wraps(test)
    def run(*args, **kwargs):
        return _WORKER.submit(test, *args, **kwargs).result()
    return run


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib()


_KEEP = []


def _host(nbytes=1024):
    """-> 16-byte aligned address of nbytes zero bytes on the host (kept alive for the process)."""
    a = np.zeros(nbytes // 4 + 8, dtype=np.float32)
    _KEEP.append(a)
    return a.ctypes.data + (-a.ctypes.data) % 16


def call_on_host(L, c, **override):
    """One tile / one block of one query and one key, H heads of width c.d; -> the entry point's return code."""
    name = ("lotus_b16_" if c.b16 else "lotus_") + ("attention_bwd" if c.bwd else "attention_fwd")
    C = H * c.d
    ints = np.array([0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.int32)  # tiles[1][4] | blocks[1][6] | owner, kext, ext_pos
    _KEEP.append(ints)
    at = ints.ctypes.data
    norm = {k: (_host() if c.norm else None) for k in ("qn_w", "qn_b", "kn_w", "kn_b")}
    a = dict(q=_host(), q_ld=C, q_off=0, kv=_host(), kv_ld=2 * C, k_off=0, v_off=C, qidx=None, kidx=at + 48 if c.extra else None,
             owner=at + 40 if c.owner else None, tiles=at, ntiles=1, blocks=at + 16, nblocks=1, out=_host(), out_ld=C, lse=_host(), H=H, d=c.d,
             scale=c.d ** -0.5, eps=1e-6, drop_p=0.0, drop_seed=0, precision=c.precision, k_max=c.k_max, **norm)
    if c.bwd:
        a.update(dout=_host(), dq=_host(), dq_ld=C, dq_off=0, dkv=_host(), dkv_ld=2 * C, dk_off=0, dv_off=C, dkv_part_stride=0,
                 atomic_out=c.atomic_out, kext=at + 44 if c.extra else None, ext_pos=at + 48 if c.extra else None, n_extra=1 if c.extra else 0,
                 dkv_extra=_host() if c.extra else None, accumulate=0, workspace=_host(4096), workspace_bytes=4096,
                 **{"d" + k: (_host() if c.norm else None) for k in norm})
    a.update(override, stream=None)
    return L.fn[name](*[a[n] for n in L.protos[name][2]])


def _route(L, entry="lotus_attention_last_route"):
    out = (ctypes.c_int * 8)()
    assert L.fn[entry](ctypes.addressof(out)) == 0
    return R(*out)


def wrong_routes(L, rows):
    bad = []
    for c, want in rows:
        rc = call_on_host(L, c)
        got = _route(L, "lotus_b16_attention_last_route" if c.b16 else "lotus_attention_last_route")
        if rc != -2 or got != want:
            bad.append(f"{c}: rc {rc} ({L.last_error()}), expected {want}, recorded {got}")
    return bad


@on_worker
def test_every_row_takes_its_route(lib):
    bad = wrong_routes(lib, ROWS)
    assert not bad, "\n".join(bad)


def test_the_table_holds_what_it_says():
    reach = {(r.family, r.direction) for _, r in ROWS}
    assert reach == {(1, 0), (2, 1), (3, 1), (4, 0), (4, 1), (5, 0), (5, 1)}, "all five families, in both directions where they exist"
    for rows in [ROWS] + list(XQ_ROWS.values()):
        for c, r in rows:
            assert r.direction == c.bwd and r.norm == c.norm, (c, r)
            assert r.threads == (128 if r.family == 4 else 256) and r.lds_bytes == {1: FWD_LDS, 2: BWD_LDS, 3: BWD_LDS, 4: 0, 5: 0}[r.family]
            assert r.targ == {4: c.d, 5: 4}.get(r.family, 0) and (r.precision == 0 or r.family in (1, 2)), (c, r)
            assert r.tail == (c.bwd and (1 if c.extra else 0) | (2 if c.norm else 0)), (c, r)
    calls = [c for c, _ in ROWS]
    assert {c.d for c in calls} == {32, 24, 16, 8} and {c.k_max for c in calls} == {0, 1, 32, 33, 78}
    assert {c.precision for c in calls} == {0, 1, 3, 5} and {c.owner for c in calls} == {True, False}
    assert {(c.extra, r.family) for c, r in ROWS if c.bwd and c.norm and c.d == 32 and c.k_max == 32 and not c.owner and not c.atomic_out} == {(False, 5), (True, 4)}
    assert not [r for c, r in ROWS if c.d == 8 and r.family > 3], "d = 8 never takes the per-lane kernels"


@on_worker
def test_refusals_return_before_a_route_is_noted(lib):
    ok = bwd(24, 32, owner=True)
    assert call_on_host(lib, ok) == -2
    before = _route(lib)
    assert before == R(4, 1, 24, 0, 1, 128, 0, 2)
    refused = [
        (fwd(32, 0), dict(kn_b=None), "all given or all null"),                # mixed norm pointers
        (bwd(32, 0), dict(qn_w=None), "all given or all null"),
        (fwd(32, 0, 1, norm=0), {}, "precision 0 (fp32) only"),                # no norm at another precision
        (bwd(32, 0, 3, norm=0), {}, "precision 0 (fp32) only"),
        (fwd(32, 0, norm=0, b16=True), {}, "bf16 activation storage"),         # no norm on the twin
        (bwd(32, 0, norm=0, b16=True), {}, "bf16 activation storage"),
        (bwd(32, 0, 1, b16=True, atomic_out=1), {}, "atomic_out"),             # the twin cannot accumulate atomically
        (bwd(32, 32, b16=True, atomic_out=1), {}, "atomic_out"),
        (fwd(6, 0), {}, "bad arguments"),                                      # head width not a multiple of 4
        (bwd(32, 0, extra=True), dict(dkv_extra=None), "borrowed-row buffer"),
    ]
    for c, override, why in refused:
        assert call_on_host(lib, c, **override) == -1 and why in lib.last_error(), (c, lib.last_error())
        assert _route(lib) == before, c
    # nothing to launch: success, and the record stays
    assert call_on_host(lib, fwd(32, 0), ntiles=0) == 0 and call_on_host(lib, bwd(32, 0, 1), nblocks=0) == 0
    assert call_on_host(lib, fwd(32, 0, 1, b16=True), ntiles=0) == 0 and _route(lib) == before
    assert lib.fn["lotus_attention_last_route"](None) == -1 and lib.fn["lotus_b16_attention_last_route"](None) == -1


@on_worker
def test_the_record_has_a_twin_and_names(lib):
    assert call_on_host(lib, bwd(32, 32, 3, extra=True)) == -2
    r = ops.last_attn_route()
    assert r == ops.AttnRoute(family=ops.ATTN_XQ, direction=1, targ=32, precision=0, norm=1, threads=128, lds_bytes=0, tail=3)
    assert _route(lib, "lotus_b16_attention_last_route") == r
    assert call_on_host(lib, fwd(32, 0, 1, b16=True)) == -2            # ... and what the twin notes, the fp32 entry point reads
    assert ops.last_attn_route() == R(ops.ATTN_FWD, 0, 0, 1, 1, 256, FWD_LDS, 0)
    assert (ops.ATTN_FWD, ops.ATTN_BWD, ops.ATTN_BWD2, ops.ATTN_XQ, ops.ATTN_XQ2) == (1, 2, 3, 4, 5)


@pytest.mark.parametrize("mode", sorted(XQ_ROWS))
def test_routes_under_lotus_xq(lib, mode):
    """LOTUS_XQ is read once per process: a fresh interpreter per value."""
    code = ("import sys; sys.path[:0] = %r\nimport test_attn_routes_host as h\nfrom robot_3dlotus_amd import _capi\n"
            "bad = h.wrong_routes(_capi.lib(), h.XQ_ROWS[%r])\nassert not bad, bad\nprint('rows ok', len(h.XQ_ROWS[%r]))\n"
            ) % ([os.path.dirname(HERE), HERE], mode, mode)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, LOTUS_XQ=mode))
    assert r.returncode == 0 and "rows ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
