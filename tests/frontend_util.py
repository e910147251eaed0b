"""Checkers shared by the front-end tests (test infrastructure): bit-exact comparison of a FrontEnd result with the oracle's
levels, the tile lists of a level, and the invariants of a tap plan."""
import numpy as np

from oracle import front_end as fe


def check_tap_plan(plan, nbr, n, rowidx=None):
    """plan: int32 [lotus_fe_tap_plan_ints(n)] (host), nbr: int32 [27][n] (host), rowidx: the processing order or None.
    The plan is a permutation-free compaction of the neighbour table: counts, the pair (row, neighbour) of every position,
    padding that gathers a valid row, and in[] listing the pairs in `rowidx` order."""
    n64 = (n + 63) // 64 * 64
    assert plan.shape[0] == 32 + 27 * n64 + 27 * n
    cnt, tin, pos = plan[:27], plan[32:32 + 27 * n64].reshape(27, n64), plan[32 + 27 * n64:].reshape(27, n)
    np.testing.assert_array_equal(cnt, (nbr >= 0).sum(1))
    walk = np.arange(n) if rowidx is None else np.asarray(rowidx)
    for t in range(27):
        rows = np.nonzero(pos[t] >= 0)[0]
        assert len(rows) == cnt[t] and set((pos[t][rows] - t * n64).tolist()) == set(range(cnt[t]))
        np.testing.assert_array_equal(tin[t][pos[t][rows] - t * n64], nbr[t][rows])   # the pair (row, neighbour) survives
        assert (tin[t][cnt[t]:(cnt[t] + 63) // 64 * 64] == 0).all()                      # padding gathers a valid row
        np.testing.assert_array_equal(pos[t] >= 0, nbr[t] >= 0)
        ordered = walk[nbr[t][walk] >= 0]                                               # rows with a pair, in processing order
        np.testing.assert_array_equal(tin[t][:cnt[t]], nbr[t][ordered], err_msg=f"tap {t}: in[] order")
        np.testing.assert_array_equal(pos[t][ordered], t * n64 + np.arange(cnt[t]), err_msg=f"tap {t}: pos[]")


def check_kext(kext, ext_pos, owner, n):
    """kext / ext_pos (host arrays) of a level with n points: -1 on owned rows, a bijection of the borrowed rows onto
    range(npad - n) whose inverse is ext_pos."""
    npad = len(owner)
    borrowed = np.nonzero(owner == 0)[0]
    assert len(borrowed) == npad - n
    assert (kext[owner != 0] == -1).all()
    e = kext[borrowed]
    np.testing.assert_array_equal(np.sort(e), np.arange(npad - n))
    np.testing.assert_array_equal(ext_pos[:npad - n][e], borrowed)


def check_tiles(g, counts, ctx_counts):
    """self_tiles / ca_tiles / ca_blocks of Level `g` tile the level exactly (counts: points per cloud of this level)."""
    counts = np.asarray(counts, dtype=np.int64)
    ctx_counts = np.asarray(ctx_counts, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    ctx_off = np.concatenate([[0], np.cumsum(ctx_counts)])
    n = int(off[-1])
    cloud_of = np.repeat(np.arange(len(counts)), counts)
    # self-attention tiles partition the padded rows [0, npad) into patches of <= K
    st = g.self_tiles.cpu().numpy()
    assert st.shape[0] == g.n_self_tiles
    assert st[0, 0] == 0 and (st[1:, 0] == st[:-1, 0] + st[:-1, 1]).all() and st[-1, 0] + st[-1, 1] == g.npad
    np.testing.assert_array_equal(st[:, 2:], st[:, :2])
    # cross-attention tiles: row ranges partition [0, n), <= 128 rows, never across a cloud, context = the cloud's tokens
    ct = g.ca_tiles.cpu().numpy()
    assert ct.shape[0] == g.n_ca_tiles
    assert ct[0, 0] == 0 and (ct[1:, 0] == ct[:-1, 0] + ct[:-1, 1]).all() and ct[-1, 0] + ct[-1, 1] == n
    assert (ct[:, 1] >= 1).all() and (ct[:, 1] <= 128).all()
    first, last = cloud_of[ct[:, 0]], cloud_of[ct[:, 0] + ct[:, 1] - 1]
    np.testing.assert_array_equal(first, last)
    np.testing.assert_array_equal(ct[:, 2], ctx_off[first])
    np.testing.assert_array_equal(ct[:, 3], ctx_counts[first])
    # a cloud's tiles are as few as 128-row tiles allow
    np.testing.assert_array_equal(np.bincount(first, minlength=len(counts)), (counts + 127) // 128)
    # backward blocks: every group walks tiles first, first + stride, ... of ONE cloud; together they walk each tile once
    cb = g.ca_blocks.cpu().numpy()
    assert cb.shape[0] == g.n_ca_blocks
    seen = np.zeros(len(ct), dtype=np.int64)
    slots = set()
    for t0, cnt, stride, grp, co, cc in cb.tolist():
        assert stride == g.ca_groups and 0 <= grp < stride
        walked = t0 + stride * np.arange(cnt)
        if cnt:
            assert walked[-1] < len(ct)
            seen[walked] += 1
            clouds = first[walked]
            assert (clouds == clouds[0]).all()
            assert co == ctx_off[clouds[0]] and cc == ctx_counts[clouds[0]]
            assert (clouds[0], grp) not in slots   # one key-side partial slot per (cloud, group)
            slots.add((clouds[0], grp))
    assert (seen == 1).all()


def assert_levels_equal(ref, got, n_levels, ctx_counts=None):
    """Every integer table of FrontEnd levels `got` against the oracle's `ref` (fe.build_all_levels): bit-exact."""
    assert len(ref) == len(got) == n_levels
    for s, (r, g) in enumerate(zip(ref, got)):
        assert g.n == r["grid"].shape[0], f"level {s} size"
        assert g.depth == r["depth"]
        np.testing.assert_array_equal(g.grid.cpu().numpy(), r["grid"], err_msg=f"L{s} grid")
        np.testing.assert_array_equal(g.batch.cpu().numpy(), r["batch"], err_msg=f"L{s} batch")
        np.testing.assert_array_equal(g.code.cpu().numpy(), r["code"], err_msg=f"L{s} code")
        np.testing.assert_array_equal(g.order.cpu().numpy(), r["order"], err_msg=f"L{s} order")
        np.testing.assert_array_equal(g.inverse.cpu().numpy(), r["inverse"], err_msg=f"L{s} inverse")
        np.testing.assert_array_equal(np.asarray(g.counts), r["counts"], err_msg=f"L{s} counts")
        np.testing.assert_array_equal(g.nbr27.cpu().numpy().T, r["nbr27"], err_msg=f"L{s} nbr27")
        # patch tables: gidx = order[pad]; owner positions = unpad[inverse]
        gidx = r["order"][0][r["pad"]]
        np.testing.assert_array_equal(g.gidx.cpu().numpy(), gidx, err_msg=f"L{s} gidx")
        owner = np.zeros(len(r["pad"]), dtype=np.int32)
        owner[r["unpad"][r["inverse"][0]]] = 1
        np.testing.assert_array_equal(g.owner.cpu().numpy(), owner, err_msg=f"L{s} owner")
        assert g.npad == len(r["pad"]) and g.n_extra == g.npad - g.n
        check_kext(g.kext.cpu().numpy(), g.ext_pos.cpu().numpy(), owner, g.n)
        cu = r["cu_seqlens"]
        tiles = g.self_tiles.cpu().numpy()
        np.testing.assert_array_equal(tiles[:, 0], cu[:-1])
        np.testing.assert_array_equal(tiles[:, 1], np.diff(cu))
        if ctx_counts is not None:
            check_tiles(g, r["counts"], ctx_counts)
        if s > 0:
            np.testing.assert_array_equal(g.cluster.cpu().numpy(), r["cluster"], err_msg=f"L{s} cluster")
            # CSR covers every parent exactly once and groups by cluster
            seg, mem = g.seg_start.cpu().numpy(), g.members.cpu().numpy()
            assert seg[0] == 0 and seg[-1] == len(mem) and (np.diff(seg) > 0).all()
            assert (r["cluster"][mem] == np.repeat(np.arange(g.n), np.diff(seg))).all()
            np.testing.assert_array_equal(np.sort(mem), np.arange(len(mem)))
    np.testing.assert_array_equal(got[0].nbr125.cpu().numpy().T, ref[0]["nbr125"])


def count_duplicates(grid, batch):
    """Points that share (cloud, voxel) with a lower-indexed point."""
    key = np.concatenate([batch.astype(np.int64)[:, None], grid.astype(np.int64)], 1)
    return len(key) - len(np.unique(key, axis=0))


__all__ = ["fe", "check_tap_plan", "check_kext", "check_tiles", "assert_levels_equal", "count_duplicates"]
