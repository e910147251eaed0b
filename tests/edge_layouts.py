"""Edge layouts for the float kernels (test infrastructure, not collected): clouds shorter than a patch, instructions of
1 .. 78 tokens, convolution scenes with empty and with full taps, pooling scenes of singletons and of full cells.

Every builder works from an INTEGER voxel grid and returns `(pc_fts, counts, txt_lens)`.  A voxel g becomes the coordinate
g * 0.01 + 0.005 (the cell centre), except on the axis minimum of the batch, which sits on the cell's lower face
(g_min * 0.01): the front end subtracts the batch minimum, so a centred minimum would put every other point ON a cell
face, one float32 rounding away from the wrong cell.  Each builder asserts on the CPU that `oracle.front_end.grid_coord`
gives back the intended grid (the grid relative to its minimum); `self_check()` runs them all (tests/test_gpu_edge_layouts.py
does at import, 0.1 s)."""
import numpy as np
import torch

from frontend_util import fe, count_duplicates
from test_gpu_frontend_kernels import _distinct_voxels, pool_case  # (shared case constructors)

PATCH_COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1, 384]
CTX_POINTS = [1, 5, 127, 128, 129, 300, 64, 2]
CTX_LAYOUTS = {"short": [1, 2, 31, 32, 7, 32, 1, 19],     # max 32: the key-tile-in-registers kernels
               "long": [1, 2, 31, 32, 33, 64, 77, 78]}    # max > 32: the 128 x 128 tile kernels
CONV_SCENES = ["isolated", "line", "solid", "n1", "n63", "n64", "n65", "many_tiny", "dups"]
POOL_SCENES = ["all_singletons", "all_eight", "100_clouds_of_3"]
HEAD_COUNTS = [[1, 63, 64, 65, 257], [40, 1, 4099, 1, 129]]


def from_grid(grid, counts, txt_lens=None, seed=0):
    """grid: int [N][3] in ONE frame for the whole batch, clouds contiguous.  -> (pc_fts f32 [N][7], counts, txt_lens,
    grid relative to the batch minimum)."""
    grid = np.asarray(grid, dtype=np.int64)
    counts = [int(c) for c in counts]
    assert grid.shape == (sum(counts), 3)
    rel = (grid - grid.min(0)).astype(np.int32)
    xyz = grid.astype(np.float64) * 0.01 + np.where(rel == 0, 0.0, 0.005)
    rng = np.random.default_rng(seed)
    pc = np.concatenate([xyz, rng.standard_normal((len(grid), 4))], 1).astype(np.float32)
    np.testing.assert_array_equal(fe.grid_coord(pc[:, :3]), rel, err_msg="the coordinates do not land in the intended voxels")
    if txt_lens is None:
        txt_lens = [7] * len(counts)
    assert len(txt_lens) == len(counts)
    return torch.from_numpy(pc), counts, [int(t) for t in txt_lens], rel


def _random_clouds(counts, box, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([_distinct_voxels(rng, c, box) for c in counts])


def patch_edges():
    """One level; every patch length from 1 to 128, 127 borrowed rows (129), one (255), none (128, 256)."""
    counts = PATCH_COUNTS
    pc, counts, txt, _ = from_grid(_random_clouds(counts, 12, 11), counts, seed=11)
    pad, unpad, cu = fe.padding_tables(counts, 128)
    assert set(np.diff(cu).tolist()) == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128}
    owner = np.zeros(len(pad), np.int32)
    owner[unpad] = 1
    c = np.asarray(counts)
    offp = np.concatenate([[0], np.cumsum(np.where(c > 128, (c + 127) // 128 * 128, c))])
    borrowed = np.array([int((owner[offp[i]:offp[i + 1]] == 0).sum()) for i in range(len(c))])
    np.testing.assert_array_equal(borrowed, np.where(c > 128, (-c) % 128, 0))
    assert borrowed.tolist() == [0] * 10 + [127, 1, 0, 127, 0, 0]
    return pc, counts, txt


def ctx_edges(layout):
    """Clouds of 1 .. 300 points against instructions of 1 .. 32 (`short`) or 1 .. 78 (`long`) tokens; `full`: one cloud with
    128 tokens, the most the key image of the tile kernels holds, and one with a single token."""
    if layout == "full":
        points, ctx = [129, 5], [128, 1]
    else:
        points, ctx = CTX_POINTS, CTX_LAYOUTS[layout]
    pc, counts, txt, _ = from_grid(_random_clouds(points, 12, 23), points, ctx, seed=23)
    assert (max(txt) == 32) if layout == "short" else (max(txt) > 32)
    return pc, counts, txt


def conv_scenes(name):
    """-> (pc_fts, counts, txt_lens).  n_levels the scene supports: 1 everywhere; 2 where the extent is >= 2 voxels."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "isolated":          # 70 voxels three apart: only the centre tap has pairs
        g = np.zeros((70, 3), np.int64)
        g[:, 0] = 3 * np.arange(70)
        g, counts = g[rng.permutation(70)], [70]
    elif name == "line":            # 65 adjacent voxels along x: taps 4, 13 and 22
        g = np.zeros((65, 3), np.int64)
        g[:, 0] = np.arange(65)
        g, counts = g[rng.permutation(65)], [65]
    elif name in ("solid", "dups"):  # a 12^3 block: all 27 taps for the 10^3 interior
        g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
        g = g[rng.permutation(len(g))]
        counts = [len(g)]
        if name == "dups":          # + 10 % exact duplicates, half at LOWER and half at HIGHER indices than their twin
            pick = rng.permutation(len(g))[:172]
            g = np.concatenate([g[pick[:86]], g, g[pick[86:]]])
            counts = [len(g)]
    elif name in ("n1", "n63", "n64", "n65"):
        n = int(name[1:])
        g, counts = _distinct_voxels(rng, n, 6), [n]
    elif name == "many_tiny":       # 100 clouds of 3
        g, b, _, _, _ = pool_case("100_clouds_of_3")
        counts = np.bincount(b).tolist()
        assert counts == [3] * 100
    else:
        raise KeyError(name)
    pc, counts, txt, rel = from_grid(g, counts, seed=len(name))
    batch = fe.offset2batch(counts).astype(np.int32)
    nbr = fe.neighbour_table(rel, batch, 3)
    per_tap = (nbr >= 0).sum(0)
    if name == "isolated":
        assert (np.delete(per_tap, 13) == 0).all() and per_tap[13] == 70, "26 empty taps"
    if name == "line":
        assert sorted(np.nonzero(per_tap)[0].tolist()) == [4, 13, 22] and per_tap[4] == per_tap[22] == 64
    if name == "solid":
        inner = ((rel >= 1) & (rel < 11)).all(1)
        assert inner.sum() == 1000 and (nbr[inner] >= 0).all(), "every tap is full for the interior"
        assert per_tap.min() == 11 ** 3 and per_tap[13] == 12 ** 3
    if name == "dups":
        assert count_duplicates(rel, batch) == 172
        rep = nbr[:, 13]
        twins = np.nonzero(rep != np.arange(len(rep)))[0]
        assert len(twins) == 172 and (twins >= 86).all()   # every duplicate points at its LOWEST-indexed twin ...
        assert (rep[twins] < 86).sum() == 86                # ... which for half of them is one of the prepended rows
    return pc, counts, txt


def pool_scenes(name):
    """Two-level builds of the integer pooling cases: singletons only, full cells only, 100 clouds of 3."""
    g, b, _, _, _ = pool_case(name)
    assert (np.diff(b) >= 0).all()
    counts = np.bincount(b).tolist()
    pc, counts, txt, rel = from_grid(g, counts, seed=len(name))
    assert (g.min(0) % 2 == 0).all(), "the 2 x 2 x 2 cells must survive the shift to the batch minimum"
    cells = np.unique(np.concatenate([b[:, None].astype(np.int64), rel >> 1], 1), axis=0, return_counts=True)[1]
    if name == "all_singletons":
        assert len(cells) == len(g)
    if name == "all_eight":
        assert (cells == 8).all()
    return pc, counts, txt


def head_counts(i):
    """Clouds for the published head; nothing but the counts matters to it."""
    return [int(c) for c in HEAD_COUNTS[i]]


def self_check():
    """Every builder once: their CPU assertions are the check."""
    patch_edges()
    for layout in ("short", "long", "full"):
        ctx_edges(layout)
    for name in CONV_SCENES:
        conv_scenes(name)
    for name in POOL_SCENES:
        pool_scenes(name)
