"""The overflow phases of conv_pairs_kernel, pinned without a device.  A 64-row tile whose tap range names more than 256
distinct neighbour rows halves the range and runs in phases; which rows of tests/conv_edges.py do that, and in which sequence,
is written in the table as literals.  This file restates the kernel's tiling in numpy (ce.phase_plan: 64-row tiles in rowidx
order, tpz = ceil(27 / nz) taps per tap group, one attempt per span, overflow when any row tile of the block has more than 256
distinct ids, the span halved down to 1) and asserts every literal against it — without this the float64 reference alone would
pass on an input that never overflows."""
import numpy as np
import pytest

import conv_edges as ce

PHASED = [r for r in ce.TABLE if "phases" in r.opts]
GEOMETRY = [r for r in ce.TABLE if "overflowing" in r.opts]


def _nd(row):
    return ce.dims(row)[2]


def _tile_rows(row, tile):
    n = ce.scene(row.scene).n
    order = ce.rowidx_of(row)
    order = np.arange(n) if order is None else order
    return order[tile * 64:tile * 64 + 64]


def test_the_table_has_the_overflow_rows():
    ids = {r.id for r in PHASED}
    assert len(PHASED) >= 10 and len(GEOMETRY) == 2
    assert {tuple(r.opts["phases"][(0, 0)]) for r in PHASED} >= {(9,), (-9, 4, 4, 1), (-27, -13, -6) + (3,) * 9}
    assert any(r.route.cols == 64 for r in PHASED) and any(r.opts.get("b16") for r in PHASED) and any(r.call == "dgrad" for r in PHASED), ids


@pytest.mark.parametrize("rid", [r.id for r in PHASED])
def test_phase_sequence_and_distinct_counts(rid):
    row = ce.BY_ID[rid]
    sc = ce.scene(row.scene)
    ce.check_table(sc.nbr)
    assert row.route.family == 3
    want = row.opts["phases"]
    got = ce.phase_plan(sc.nbr, ce.rowidx_of(row), _nd(row), row.route.nz, blocks=sorted({b for b, _ in want}))
    for key, seq in want.items():
        assert got[key] == seq, (rid, key, got[key], seq)
    for (tile, t0, t1), count in row.opts["distinct"].items():
        d = ce.distinct_rows(sc.nbr, _tile_rows(row, tile), t0, t1)
        assert (d <= ce.HT) if count is None else (d == count), (rid, tile, t0, t1, d, count)


def test_partial_last_tile_sits_in_an_overflowing_block():
    row = ce.BY_ID["d-fwd-ovfncs2-32x64"]
    n = ce.scene(row.scene).n
    assert n % 64 == 10 and -(-n // 64) == 512 and n >= 32641
    plan = ce.phase_plan(ce.scene(row.scene).nbr, None, 64, 3, blocks=[255])
    assert plan[(255, 0)][0] == -9 and len(_tile_rows(row, 511)) == 10
    # only the three planted tiles overflow: the neighbour tile of each is re-phased by the shared flag, not by its own rows
    assert ce.distinct_rows(ce.scene(row.scene).nbr, _tile_rows(row, 1), 0, 9) <= ce.HT
    assert ce.distinct_rows(ce.scene(row.scene).nbr, _tile_rows(row, 2), 0, 9) <= ce.HT


def test_empty_half_phase_has_no_pairs():
    for row in (r for r in PHASED if r.scene == "ovfempty"):
        nbr = ce.scene(row.scene).nbr
        assert (nbr[0:4, 0:64] < 0).all() and (nbr[4:9, 0:64] >= 0).sum(1).tolist() == [64, 48, 64, 48, 64]
        assert row.cin // 32 in (2, 3), "nkc > 1: the fill loop of the ngr == 0 branch runs"


def test_planted_tiles_need_the_compacted_row_list():
    """In every planted tile some tap has holes, so the k-th pair of that tap is not the k-th row of the tile: a later phase that
    looked a pair's row up without the compacted list would gather other rows (a library mutated that way passed the rows whose
    planted taps were all full)."""
    for row in PHASED:
        nbr, nrt = ce.scene(row.scene).nbr, 2 if _nd(row) == 64 else 1
        planted = {tile for tile, _, _ in row.opts["distinct"]}
        for (b, z), seq in row.opts["phases"].items():
            if seq[0] > 0:
                continue                     # a single phase reads the ids it compacted itself
            shifted = 0
            for tile in planted & set(range(b * nrt, b * nrt + nrt)):
                for t in range(z * row.route.tpz, min(27, (z + 1) * row.route.tpz)):
                    act = np.nonzero(nbr[t, tile * 64:tile * 64 + 64] >= 0)[0]
                    shifted += int(len(act) > 0 and (act != np.arange(len(act))).any())
            assert shifted >= 2, (row.id, b, z)


def test_hash_wrap_precondition():
    """All 256 ids of tile 0 have their home slot in 192 .. 255: 256 keys into 64 home slots overrun the end of the table."""
    sc = ce.scene("ovfwrap")
    ids = sc.extra["ids"]
    assert sc.extra["qualifying"] == 2045 and len(np.unique(ids)) == 256 and int(ids.max()) < 8192
    assert (ce.hash_bucket(ids) >= 192).all()
    used = sc.nbr[0:9, 0:64]
    assert set(np.unique(used[used >= 0]).tolist()) == set(ids.tolist())
    assert int(ce.hash_bucket(np.array([1]))[0]) == ((2654435761 >> 16) % 256)


@pytest.mark.parametrize("rid", [r.id for r in GEOMETRY])
def test_solid_block_overflows(rid):
    row = ce.BY_ID[rid]
    sc = ce.scene(row.scene)
    assert sc.n == 21 ** 3
    interior = (sc.nbr >= 0).all(0)
    assert int(interior.sum()) == 19 ** 3
    plan = ce.phase_plan(sc.nbr, ce.rowidx_of(row), _nd(row), row.route.nz)
    over = [k for k, seq in plan.items() if seq[0] < 0]
    if row.opts["overflowing"] == "all":
        assert row.route.nz == 3 and len(over) == len(plan) == 3 * 145, f"{len(plan) - len(over)} of {len(plan)} (tile, tap group) pairs fit"
        assert all(seq == [-9, 4, 4, 1] for seq in plan.values())
    else:
        np.testing.assert_array_equal(np.sort(ce.rowidx_of(row)), np.arange(sc.n))
        assert row.route.nz == 1 and len(plan) == 145 and len(over) == row.opts["overflowing"] >= 1
        assert all(plan[k] == [-27, 13, 13, 1] for k in over)


def test_no_other_pair_row_overflows():
    """Rows that do not name an overflow must not have one (3 taps x 64 rows cannot; the split boundaries are checked)."""
    for row in ce.TABLE:
        if row.route.family != 3 or "phases" in row.opts or "overflowing" in row.opts or row.route.nz == 9:
            continue
        sc = ce.scene(row.scene)
        plan = ce.phase_plan(sc.nbr, ce.rowidx_of(row), _nd(row), row.route.nz)
        assert all(seq[0] > 0 for seq in plan.values()), row.id


def test_every_scene_is_a_legal_table():
    import edge_layouts as el

    el.self_check()
    for name in sorted({r.scene for r in ce.TABLE + ce.REFUSE}):
        sc = ce.scene(name)
        ce.check_table(sc.nbr)
        assert sc.nbr.shape[1] == sc.n and sc.nbr.shape[0] in (27, 125)
    assert (ce.scene("emptytap:1025").nbr[5] < 0).all()
    bare = ce.scene("centreonly:2049").nbr[:, 1024:2048]
    assert (np.delete(bare, 13, 0) < 0).all() and (bare[13] >= 0).all()
    assert ce.scene("el:solid:5").nbr.shape == (125, 1728) and int((ce.scene("el:solid:5").nbr >= 0).all(0).sum()) == 8 ** 3
    assert int((ce.scene("el:isolated:3").nbr >= 0).any(1).sum()) == 1
