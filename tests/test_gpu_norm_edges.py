"""The normalisation kernels on the edge shapes of tests/norm_edges.py: LayerNorm on both sides of every lane rule, around the
rows per block of both geometries, behind the 1024-block cap of the backward, with the deferred parameter gradients, accumulate,
the dz hand-over and no saved statistics; BatchNorm over 1 .. 10923 rows on every grid of the fused last-arrival statistics
(1, 16, 17, 255, 256 blocks, capped), widths that leave threads idle or need column slabs, every activation, train and eval,
every forward and apply variant bit-compared; the adaptive norms on 1 - 5 and 100 clouds, 2 - 64 chunks, empty clouds, both
BatchNorm routes; the bf16-storage twin on a subset.

Each row first asserts its launch plan (lotus_norm_plan / lotus_adanorm_plan against the table's literal numbers), then runs the
raw C-ABI calls into guarded caller-owned buffers, twice (tests/norm_run.py: references, bars, input conditions).  Measured
errors: ledger, norm_edges/<row id>."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import ledger  # noqa: E402
import norm_edges as ne  # noqa: E402
import norm_run as nr  # noqa: E402


@pytest.fixture(scope="module")
def counters():
    from robot_3dlotus_amd import _capi

    c = torch.zeros(_capi.query("lotus_splitk_counters_bytes"), dtype=torch.uint8, device="cuda")
    yield c
    assert bool((c == 0).all())


def _assert_plan(row):
    from robot_3dlotus_amd import _capi

    L = _capi.lib()
    for key, entry, args in ne.plan_queries(row):
        if row.opts.get("b16") and entry == "lotus_norm_plan":
            entry = "lotus_b16_norm_plan"
        out = (ctypes.c_int * 8)()
        assert L.fn[entry](*args, ctypes.addressof(out)) == 0, (row.id, key)
        assert tuple(out[:ne.PLAN_FIELDS[key]]) == tuple(ne.PLAN[row.id][key]), (row.id, key, tuple(out))


@pytest.mark.parametrize("row_id", [r.id for r in ne.ROWS])
def test_norm_edge(row_id, counters):
    row = ne.BY_ID[row_id]
    _assert_plan(row)
    rec, fails = nr.run(row, counters)
    ledger.record("norm_edges/" + row.id, **rec)
    assert not fails, "\n".join(fails[:40])
