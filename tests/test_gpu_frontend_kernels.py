"""Every `lotus_fe_*` entry point of csrc/front_end.hip on its own, against numpy / the oracle: bit-exact, no tolerance.

The inputs are constructed integer tables, not clouds, so that each kernel sees the edges its pipeline neighbours never
produce: more than 65 536 keys (the radix histogram scan leaves its first 16 384-counter segment, the pooling carry loop
its first round of 64 blocks), every serialisation depth 1..16, 7 batch bits, hash tables at the tightest load the sizing
rule allows, coordinates at 0 and 65 535, clouds of 1 .. 2 K + 1 points around the patch size K.

Outputs are pre-filled with a sentinel; rows an entry point has no business writing must keep it.  The case constructors
(`*_case` / `*_cases`) are plain numpy and run without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from frontend_util import fe, check_tap_plan, check_kext, count_duplicates  # noqa: E402

SENT = -7  # sentinel of every pre-filled output


def _capi():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi as c
    return c


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _full(shape, dtype):
    return torch.full(shape, SENT, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ lotus_fe_sort
SORT_N = [1, 63, 64, 65, 1023, 1024, 1025, 4097, 65536, 65537, 100003, 262144, 524288]
SORT_BITS = [1, 7, 8, 9, 16, 22, 28, 33, 40, 55, 63]
# (n, n_max, key_bits): every n with one width; every width at 65 537 keys (68 tiles x 256 digits = 17 408 counters: the first
# size whose histogram scan needs a second segment) and at 1025; n < n_max (n is read from device memory)
SORT_CASES = [(n, n, SORT_BITS[i % len(SORT_BITS)]) for i, n in enumerate(SORT_N)] \
    + [(65537, 65537, b) for b in SORT_BITS] + [(1025, 1025, b) for b in SORT_BITS] \
    + [(524288, 524288, 55), (262144, 262144, 63), (100003, 100003, 9)] \
    + [(1, 1025, 16), (1000, 65537, 28), (65537, 100003, 40), (100003, 524288, 55), (65536, 65537, 33)]


def random_keys(rng, n, key_bits):
    """int64 [4][n], four DIFFERENT rows of non-negative keys below 2**key_bits."""
    return rng.integers(0, 1 << key_bits, size=(4, n), dtype=np.int64, endpoint=False)


def sort_expected(keys):
    order = np.stack([np.argsort(keys[k], kind="stable") for k in range(4)]).astype(np.int32)
    skeys = np.take_along_axis(keys, order.astype(np.int64), 1)
    return skeys, order, fe.inverse_perm(order)


def _run_sort(keys, n_max, key_bits, seed=0):
    c = _capi()
    n = keys.shape[1]
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 1 << key_bits, size=(4, n_max), dtype=np.int64)  # rows >= n: keys that must not be read
    code[:, :n] = keys
    skeys, order, inverse = _full((4, n_max), torch.int64), _full((4, n_max), torch.int32), _full((4, n_max), torch.int32)
    ws = torch.zeros(c.query("lotus_fe_sort_workspace", n_max), dtype=torch.uint8, device="cuda")
    code_d, n_d = _dev(code), _dev(np.array([n], np.int32))
    e_skeys, e_order, e_inverse = sort_expected(keys)
    # First without `inverse` (optional): the scatter of the inverse permutation is the one consumer of `order` on the device,
    # so the order is compared on the host before anything indexes with it.
    c.call("lotus_fe_sort", code_d, n_max, n_d, n_max, key_bits, skeys, order, None, ws, ws.numel())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(order.cpu().numpy()[:, :n], e_order, err_msg=f"order n={n} n_max={n_max} key_bits={key_bits}")
    skeys.fill_(SENT)
    order.fill_(SENT)
    c.call("lotus_fe_sort", code_d, n_max, n_d, n_max, key_bits, skeys, order, inverse, ws, ws.numel())
    torch.cuda.synchronize()
    for name, got, exp in (("skeys", skeys, e_skeys), ("order", order, e_order), ("inverse", inverse, e_inverse)):
        got = got.cpu().numpy()
        np.testing.assert_array_equal(got[:, :n], exp, err_msg=f"{name} n={n} n_max={n_max} key_bits={key_bits}")
        assert (got[:, n:] == SENT).all(), f"{name}: rows >= n were written"


@pytest.mark.parametrize("n,n_max,key_bits", SORT_CASES)
def test_sort_against_stable_argsort(n, n_max, key_bits):
    rng = np.random.default_rng(n * 67 + key_bits)
    _run_sort(random_keys(rng, n, key_bits), n_max, key_bits)


def sort_stability_cases(n):
    """name -> (keys int64 [4][n], key_bits): inputs whose order is decided by the tie rule (ties by index)."""
    rng = np.random.default_rng(n)
    out = {"all_equal": (np.broadcast_to(np.array([[5], [0], [(1 << 22) - 1], [77]], np.int64), (4, n)).copy(), 22)}
    vals = np.array([3, 1 << 9, (1 << 21) + 1], np.int64)
    out["three_values"] = (vals[rng.integers(0, 3, size=(4, n))], 22)
    # 22 bits = 3 passes.  Equal in the digit of the LAST pass only: that pass must keep the order the first two built
    out["equal_in_last_digit"] = ((np.int64(0x2a) << 16) | rng.integers(0, 1 << 16, size=(4, n), dtype=np.int64), 22)
    # ... and differing in the last digit only: 64 groups of ties, each in index order
    out["differ_in_last_digit"] = ((rng.integers(0, 64, size=(4, n), dtype=np.int64) << 16) | 0x1234, 22)
    # an even pass count with ties (the other leg of the ping-pong)
    out["ties_two_passes"] = (rng.integers(0, 300, size=(4, n), dtype=np.int64), 16)
    return out


@pytest.mark.parametrize("n", [1025, 100003])
@pytest.mark.parametrize("name", ["all_equal", "three_values", "equal_in_last_digit", "differ_in_last_digit", "ties_two_passes"])
def test_sort_is_stable(name, n):
    keys, key_bits = sort_stability_cases(n)[name]
    _run_sort(keys, n, key_bits)


# ------------------------------------------------------------------------------------------------ lotus_fe_encode
ENCODE_PERMS = [[0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]]


def encode_case(depth, n=3001, seed=0):
    """Random grid in [0, 2**depth) with one row at 2**depth - 1 (so that gmax yields `depth`), batch ids up to 127."""
    rng = np.random.default_rng(1000 * depth + seed)
    grid = rng.integers(0, 1 << depth, size=(n, 3)).astype(np.int32)
    grid[rng.integers(0, n)] = (1 << depth) - 1
    batch = rng.integers(0, 128, size=n).astype(np.int32)
    batch[:2] = (0, 127)
    return grid, batch


def _run_encode(grid, batch, perm4, depth_bound, stride):
    c = _capi()
    n = grid.shape[0]
    gmax = _dev(np.array([grid.max()], np.int32))
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    code = _full((4, stride), torch.int64)
    pm = np.asarray(perm4, dtype=np.int32)
    c.call("lotus_fe_encode", _dev(grid), _dev(batch), n, gmax, pm.ctypes.data, depth_bound, state, code, stride)
    torch.cuda.synchronize()
    return code.cpu().numpy(), state.cpu().numpy()


@pytest.mark.parametrize("depth", list(range(1, 17)))
def test_encode_every_depth(depth):
    grid, batch = encode_case(depth)
    n, stride = grid.shape[0], grid.shape[0] + 5
    assert fe.serialized_depth(grid) == depth
    for perm4 in ENCODE_PERMS:
        code, state = _run_encode(grid, batch, perm4, depth, stride)
        exp = np.stack([fe.encode(grid, batch, depth, fe.ORDERS[j]) for j in perm4])
        np.testing.assert_array_equal(code[:, :n], exp, err_msg=f"depth {depth} perm {perm4}")
        assert (code[:, n:] == SENT).all()
        assert state[1] == depth and (state[0] & 1) == 0 and (state[2:] == 0).all()
    # the bound at its loosest is as good; one below the depth raises the device flag (codes still those of the true depth)
    code, state = _run_encode(grid, batch, ENCODE_PERMS[0], 16, stride)
    assert state[1] == depth and (state[0] & 1) == 0
    code, state = _run_encode(grid, batch, ENCODE_PERMS[0], depth - 1, stride)
    assert state[1] == depth and (state[0] & 1) == 1


def test_encode_depth_17_raises_the_flag():
    grid, batch = encode_case(17)
    code, state = _run_encode(grid, batch, ENCODE_PERMS[0], 16, grid.shape[0])   # (codes unspecified at depth > 16)
    assert state[1] == 17 and (state[0] & 1) == 1
    code, state = _run_encode(grid, batch, ENCODE_PERMS[0], 17, grid.shape[0])   # ... whatever the bound says
    assert state[1] == 17 and (state[0] & 1) == 1


# ------------------------------------------------------------------------------------------------ lotus_fe_grid
GRID_SIZE = float(np.float32(0.01))


def near_integer_points(base, ks):
    """float32 coordinates x with (x - base) / 0.01f within a few ulp of the integers `ks`, from both sides."""
    base = np.float32(base)
    t = (ks.astype(np.float32) * np.float32(0.01)).astype(np.float32)
    x = (base + t).astype(np.float32)
    out = [x]
    for _ in range(2):
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    lo = x
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf))
        out.append(lo)
    return np.concatenate(out)


def grid_cases():
    """name -> (coord float32 [n][ld], ld)."""
    rng = np.random.default_rng(7)
    cases = {}
    c = rng.uniform(-0.4, 0.6, size=(5000, 7)).astype(np.float32)   # negative and positive coordinates, row stride 7
    cases["stride7"] = c
    cases["stride4"] = np.ascontiguousarray(c[:, :4])
    cases["plus50m"] = (c + np.float32(50.0)).astype(np.float32)
    cases["minus50m"] = (c - np.float32(50.0)).astype(np.float32)
    cases["n1"] = np.array([[0.3, -0.2, 5.0, 1.0, 1.0, 1.0, 1.0]], np.float32)
    ks = np.arange(1, 1500)
    for name, base in (("near_integer", -0.3217), ("near_integer_origin", 0.0), ("near_integer_far", 3.75)):
        cols = [near_integer_points(base, ks) for _ in range(3)]
        pts = np.stack([cols[0], rng.permutation(cols[1]), rng.permutation(cols[2])], 1)
        pts = np.concatenate([np.full((1, 3), base, np.float32), pts])   # the batch minimum is `base` itself
        cases[name] = np.ascontiguousarray(pts, dtype=np.float32)
    return cases


def grid_expected(coord):
    c = np.ascontiguousarray(coord[:, :3], dtype=np.float32)
    d = (c - c.min(0)).astype(np.float32)
    return np.trunc(d / np.float32(0.01)).astype(np.float32).astype(np.int32)


@pytest.mark.parametrize("name", ["stride7", "stride4", "plus50m", "minus50m", "n1", "near_integer", "near_integer_origin",
                                  "near_integer_far"])
def test_grid_coordinates(name):
    c = _capi()
    coord = grid_cases()[name]
    n, ld = coord.shape
    exp = grid_expected(coord)
    np.testing.assert_array_equal(exp, fe.grid_coord(coord[:, :3]))
    if name.startswith("near_integer"):  # the construction does what it says: quotients on both sides of an integer
        q = ((coord[:, :3] - coord[:, :3].min(0)).astype(np.float32) / np.float32(0.01)).astype(np.float32)
        assert ((q - np.round(q) == 0).sum() > 100) and ((q < np.round(q)).sum() > 100) and ((q > np.round(q)).sum() > 100)
        assert (np.abs(q - np.round(q))[1:] < 1e-3).all()
    grid = _full((n + 3, 3), torch.int32)
    scratch = _full((8,), torch.int32)
    gmax = scratch[4:5]
    c.call("lotus_fe_grid", _dev(coord), ld, n, GRID_SIZE, grid, gmax, scratch)
    torch.cuda.synchronize()
    grid = grid.cpu().numpy()
    np.testing.assert_array_equal(grid[:n], exp, err_msg=name)
    assert (grid[n:] == SENT).all()
    assert int(gmax.item()) == int(exp.max())


# ------------------------------------------------------------------------------------------------ lotus_fe_neighbours
def _distinct_voxels(rng, n, box):
    cells = rng.permutation(box ** 3)[:n]
    return np.stack([cells // (box * box), (cells // box) % box, cells % box], 1).astype(np.int32)


def neighbour_case(name):
    """-> (grid int32 [n][3], batch int32 [n])."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "solid_block":            # all 27 / 125 taps present inside, long linear-probe chains
        g = np.stack(np.meshgrid(*[np.arange(40)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
        g = g[rng.permutation(len(g))] + 11
        return g, np.zeros(len(g), np.int32)
    if name in ("pow2_32768", "pow2_65536"):  # cap == 2 n: the tightest table the sizing rule allows
        n = int(name.split("_")[1])
        return _distinct_voxels(rng, n, 64), np.sort(rng.integers(0, 16, size=n)).astype(np.int32)
    if name == "faces":                 # patches on the faces x, y, z in {0, 65535}, corners included
        pts = []
        sq = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
        for a in range(3):
            for v in (0, 65535):
                for ou in (0, 65516):
                    for ov in (0, 65516):
                        p = np.empty((len(sq), 3), np.int64)
                        p[:, a] = v
                        p[:, (a + 1) % 3] = sq[:, 0] + ou
                        p[:, (a + 2) % 3] = sq[:, 1] + ov
                        pts.append(p)
        g = np.unique(np.concatenate(pts), axis=0).astype(np.int32)
        g = g[rng.permutation(len(g))]
        return g, (np.arange(len(g)) % 2).astype(np.int32)
    if name == "same_shape_128_clouds":  # only the cloud field of the key differs
        shape = _distinct_voxels(rng, 500, 12)
        return np.tile(shape, (128, 1)), np.repeat(np.arange(128), 500).astype(np.int32)
    if name == "duplicates":            # 10 % exact duplicates, half at LOWER and half at HIGHER indices than their twin
        base = _distinct_voxels(rng, 20000, 40)
        bb = np.sort(rng.integers(0, 2, size=len(base))).astype(np.int32)
        pick = rng.permutation(len(base))[:2000]
        lo, hi = pick[:1000], pick[1000:]
        return np.concatenate([base[lo], base, base[hi]]), np.concatenate([bb[lo], bb, bb[hi]])
    if name == "n1":
        return np.array([[5, 0, 65535]], np.int32), np.array([3], np.int32)
    if name == "synth_128x4096":
        import robot_3dlotus_amd  # noqa: F401
        from robot_3dlotus_amd import synth
        b = synth.synth_batch(128, 4096, seed=21)
        return fe.grid_coord(b["pc_fts"][:, :3].numpy()), fe.offset2batch(b["npoints_in_batch"]).astype(np.int32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["solid_block", "pow2_32768", "pow2_65536", "faces", "same_shape_128_clouds", "duplicates",
                                  "n1", "synth_128x4096"])
def test_neighbour_tables(name):
    c = _capi()
    grid, batch = neighbour_case(name)
    n = len(grid)
    if name == "synth_128x4096":
        assert n == 524288
    if name == "duplicates":
        assert count_duplicates(grid, batch) == 2000
    ws = torch.empty(c.query("lotus_fe_neighbours_workspace", n), dtype=torch.uint8, device="cuda")
    if name.startswith("pow2"):
        assert ws.numel() == 2 * n * 16
    g, b = _dev(grid), _dev(batch)
    for ksize in (3, 5):
        nbr = _full((ksize ** 3 + 1, n), torch.int32)
        c.call("lotus_fe_neighbours", g, b, n, ksize, nbr, ws, ws.numel())
        torch.cuda.synchronize()
        nbr = nbr.cpu().numpy()
        exp = fe.neighbour_table(grid, batch, ksize)
        np.testing.assert_array_equal(nbr[:-1].T, exp, err_msg=f"{name} k={ksize}")
        assert (nbr[-1] == SENT).all()
        if name == "solid_block":
            inner = ((grid >= 11 + 2) & (grid < 11 + 40 - 2)).all(1)
            assert (exp[inner] >= 0).all()


# ------------------------------------------------------------------------------------------------ lotus_fe_pool
def pool_case(name):
    """-> (grid int32 [n][3], batch int32 [n] (clouds contiguous), depth, n_max, perm4)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("over_65536_parents", "n_below_n_max"):  # 100 000 parents: 98 blocks of 1024, second round of the carry loop
        n = 100000
        g = _distinct_voxels(rng, n - 3000, 128)
        b = rng.integers(0, 8, size=len(g)).astype(np.int32)
        twin = rng.permutation(len(g))[:3000]                        # and 3000 duplicate (cloud, voxel) pairs (n_dup)
        g, b = np.concatenate([g, g[twin]]), np.concatenate([b, b[twin]])
        by_cloud = np.argsort(b, kind="stable")
        return g[by_cloud], b[by_cloud], 7, n + (5000 if name == "n_below_n_max" else 0), [2, 0, 3, 1]
    if name == "all_singletons":        # one point per 2 x 2 x 2 cell
        n = 5000
        g = 2 * _distinct_voxels(rng, n, 30) + rng.integers(0, 2, size=(n, 3)).astype(np.int32)
        return g, np.sort(rng.integers(0, 5, size=n)).astype(np.int32), 6, n, [0, 1, 2, 3]
    if name == "all_eight":             # a solid 16^3 block at an even origin: 512 clusters of 8
        g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32) + 6
        return g[rng.permutation(len(g))], np.zeros(len(g), np.int32), 5, len(g), [3, 2, 1, 0]
    if name == "100_clouds_of_3":       # a wave of children spans ~20 clouds: the per-lane atomic branch of the count
        g = np.concatenate([2 * _distinct_voxels(rng, 3, 4) for _ in range(100)])
        return g, np.repeat(np.arange(100), 3).astype(np.int32), 3, 300, [1, 3, 0, 2]
    raise KeyError(name)


def pool_inputs_and_expected(grid, batch, depth, perm4):
    n = len(grid)
    assert fe.serialized_depth(grid) <= depth
    code = np.stack([fe.encode(grid, batch, depth, o) for o in fe.ORDERS])
    order0 = np.argsort(code[0], kind="stable").astype(np.int32)
    skey0 = code[0][order0]
    exp = fe.pooling_tables(code, grid, batch, depth, perm=perm4)
    exp["n_dup"] = int((skey0[1:] == skey0[:-1]).sum())
    exp["counts"] = np.bincount(exp["batch"], minlength=int(batch.max()) + 1)
    return code, skey0, order0, exp


@pytest.mark.parametrize("name", ["over_65536_parents", "n_below_n_max", "all_singletons", "all_eight", "100_clouds_of_3"])
def test_pooling_tables(name):
    c = _capi()
    grid, batch, depth, n_max, perm4 = pool_case(name)
    n, B = len(grid), int(batch.max()) + 1
    code, skey0, order0, exp = pool_inputs_and_expected(grid, batch, depth, perm4)
    assert exp["n_dup"] == count_duplicates(grid, batch)
    nc = len(exp["head"])
    if name == "all_singletons":
        assert nc == n
    if name == "all_eight":
        assert (exp["cluster_counts"] == 8).all()
    if name.startswith("over"):
        assert n > 65536 and exp["n_dup"] == 3000

    def padded(a, fill=SENT):  # [.., n] -> [.., n_max]; the rows >= n hold the sentinel and must not be read
        out = np.full(a.shape[:-1] + (n_max,), fill, dtype=a.dtype)
        out[..., :n] = a
        return out

    pgrid = np.full((n_max, 3), SENT, np.int32)
    pgrid[:n] = grid
    cluster, seg = _full((n_max,), torch.int32), _full((n_max + 1,), torch.int32)
    ccode, cgrid, cbatch = _full((4, n_max), torch.int64), _full((n_max, 3), torch.int32), _full((n_max,), torch.int32)
    ccounts = _full((B + 2,), torch.int32)
    scal = torch.zeros(4, dtype=torch.int32, device="cuda")   # [0] n_child, [1] n_dup (zeroed by the caller)
    scal[0] = SENT
    pm = np.asarray(perm4, dtype=np.int32)
    c.call("lotus_fe_pool", _dev(padded(code)), _dev(padded(skey0)), _dev(padded(order0)), _dev(pgrid), _dev(padded(batch)),
           _dev(np.array([n], np.int32)), n_max, pm.ctypes.data, B, cluster, seg, scal[0:1], ccode, cgrid, cbatch, ccounts[:B],
           scal[1:2])
    torch.cuda.synchronize()
    scal = scal.cpu().numpy()
    assert scal[0] == nc and scal[1] == exp["n_dup"]
    cluster, seg = cluster.cpu().numpy(), seg.cpu().numpy()
    np.testing.assert_array_equal(cluster[:n], exp["cluster"])
    assert (cluster[n:] == SENT).all()
    # CSR: seg_start indexes order0, one non-empty run per child, runs group the parents by cluster
    np.testing.assert_array_equal(seg[:nc + 1], exp["idx_ptr"])
    assert seg[0] == 0 and seg[nc] == n and (np.diff(seg[:nc + 1]) > 0).all() and (seg[nc + 1:] == SENT).all()
    np.testing.assert_array_equal(exp["cluster"][order0], np.repeat(np.arange(nc), np.diff(seg[:nc + 1])))
    ccode, cgrid, cbatch = ccode.cpu().numpy(), cgrid.cpu().numpy(), cbatch.cpu().numpy()
    np.testing.assert_array_equal(ccode[:, :nc], exp["code"])
    np.testing.assert_array_equal(cgrid[:nc], exp["grid"])
    np.testing.assert_array_equal(cbatch[:nc], exp["batch"])
    assert (ccode[:, nc:] == SENT).all() and (cgrid[nc:] == SENT).all()
    # (cbatch doubles as the per-block scratch of the head count: only its first n_child rows are specified)
    ccounts = ccounts.cpu().numpy()
    np.testing.assert_array_equal(ccounts[:B], exp["counts"])
    assert (ccounts[B:] == SENT).all()


# ------------------------------------------------------------------------------------------------ lotus_fe_patch
PATCH_CASES = {"edges": [1, 2, 127, 128, 129, 255, 256, 257, 1, 4096], "seven_patches": [128 * 7]}


def patch_expected(counts, K, order):
    pad, unpad, cu = fe.padding_tables(counts, K)
    owner = np.zeros(len(pad), np.int32)
    owner[unpad] = 1
    return order[pad], owner


@pytest.mark.parametrize("name", ["edges", "seven_patches"])
def test_patch_tables(name):
    c = _capi()
    counts, K = np.asarray(PATCH_CASES[name], np.int64), 128
    B, n = len(counts), int(counts.sum())
    rng = np.random.default_rng(B)
    off = np.concatenate([[0], np.cumsum(counts)])
    cpad = np.where(counts > K, (counts + K - 1) // K * K, counts)
    offp = np.concatenate([[0], np.cumsum(cpad)])
    npad = int(offp[-1])
    # a serialisation order: a permutation of every cloud's own rows
    order = np.concatenate([off[i] + rng.permutation(counts[i]) for i in range(B)]).astype(np.int32)
    e_gidx, e_owner = patch_expected(counts, K, order)
    assert len(e_gidx) == npad
    gidx, owner, kext = _full((npad + 4,), torch.int32), _full((npad + 4,), torch.int32), _full((npad + 4,), torch.int32)
    ext_pos = _full((npad - n + 4,), torch.int32)
    c.call("lotus_fe_patch", _dev(order), _dev(off, torch.int32), _dev(offp, torch.int32), B, K, npad, gidx, owner, kext, ext_pos)
    torch.cuda.synchronize()
    gidx, owner, kext, ext_pos = (t.cpu().numpy() for t in (gidx, owner, kext, ext_pos))
    np.testing.assert_array_equal(gidx[:npad], e_gidx)
    np.testing.assert_array_equal(owner[:npad], e_owner)
    check_kext(kext[:npad], ext_pos[:npad - n], e_owner, n)
    for t, m in ((gidx, npad), (owner, npad), (kext, npad), (ext_pos, npad - n)):
        assert (t[m:] == SENT).all()
    # the edges by hand: nothing is padded up to K; K + 1 borrows K - 1 rows; a multiple of K borrows nothing
    borrowed = np.array([int((e_owner[offp[i]:offp[i + 1]] == 0).sum()) for i in range(B)])
    np.testing.assert_array_equal(borrowed, np.where(counts > K, (-counts) % K, 0))
    if name == "edges":
        assert borrowed.tolist() == [0, 0, 0, 0, 127, 1, 0, 127, 0, 0]
    # a borrowed row repeats the row K places before it, of the same cloud
    rows = np.nonzero(owner[:npad] == 0)[0]
    np.testing.assert_array_equal(gidx[rows], gidx[rows - K])
    # without kext / ext_pos (both optional) the other two tables are the same
    gidx2, owner2 = _full((npad,), torch.int32), _full((npad,), torch.int32)
    c.call("lotus_fe_patch", _dev(order), _dev(off, torch.int32), _dev(offp, torch.int32), B, K, npad, gidx2, owner2, None, None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gidx2.cpu().numpy(), e_gidx)
    np.testing.assert_array_equal(owner2.cpu().numpy(), e_owner)


# ------------------------------------------------------------------------------------------------ lotus_fe_tap_plan
def tap_case(n, seed=0):
    """A 27 x n neighbour table with every density: tap 0 has no pair, tap 13 pairs every row with itself, tap 26 pairs every
    row with a random one, the others are 5 .. 95 % full."""
    rng = np.random.default_rng(n + seed)
    nbr = rng.integers(0, n, size=(27, n)).astype(np.int32)
    for t in range(27):
        nbr[t][rng.random(n) >= 0.05 + 0.9 * t / 26] = -1
    nbr[0] = -1
    nbr[13] = np.arange(n)
    nbr[26] = rng.integers(0, n, size=n)
    return nbr, rng.permutation(n).astype(np.int32)


@pytest.mark.parametrize("with_rowidx", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 262144])
def test_tap_plan(n, with_rowidx):
    c = _capi()
    nbr, rowidx = tap_case(n)
    assert (nbr[0] < 0).all() and (nbr[13] >= 0).all()
    ints = c.query("lotus_fe_tap_plan_ints", n)
    plan = _full((ints + 8,), torch.int32)
    c.call("lotus_fe_tap_plan", _dev(nbr), _dev(rowidx) if with_rowidx else None, n, plan)
    torch.cuda.synchronize()
    plan = plan.cpu().numpy()
    assert (plan[ints:] == SENT).all()
    check_tap_plan(plan[:ints], nbr, n, rowidx if with_rowidx else None)
