"""Shared helpers of the SimplePolicyPTV3Concat tests (test infrastructure, not collected): the numpy / float64 restatement of
the context tap sum of csrc/ctx_stem.hip and of the dense convolution it replaces, the rows of the kernel tests with their
self-check, the scenes whose neighbour tables the front end makes, and the case table / batch / configuration of the fixtures of
tests/golden/make_golden_concat.py.  No reference import here (the GPU tests use this module too)."""
import collections
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the geometry the rows are built around (csrc/ctx_stem.hip; lotus_ctx_taps_plan reports it)
CT_ROWS, CT_SPLITS, CT_TILE, CT_BTILE, CT_MAX_TC, CT_TMAX = 128, 32, 128, 512, 32768, 128
KERNEL_TOL = 2e-5  # x max(1, |ref|max): the project's per-kernel bar


def max_width(T):
    return CT_MAX_TC // T // 4 * 4


# ------------------------------------------------------------------------------------------ float64 restatement
def cloud_of(counts):
    return np.repeat(np.arange(len(counts)), counts)


def taps_fwd(P, nbr, counts, add=None):
    """y_i = add_i + sum_{t, nbr[t][i] >= 0} P[b(i)][t];  P [B][T][C], nbr [T][n] (only the sign is read) -> float64 [n][C]."""
    P = np.asarray(P, np.float64)
    T, n = nbr.shape
    b = cloud_of(counts)
    y = np.zeros((n, P.shape[2])) if add is None else np.asarray(add, np.float64).copy()
    for t in range(T):
        rows = np.nonzero(nbr[t] >= 0)[0]
        y[rows] += P[b[rows], t]
    return y


def taps_bwd(dy, nbr, counts):
    """dP[b][t] = sum_{i in cloud b, nbr[t][i] >= 0} dy_i -> float64 [B][T][C]."""
    dy = np.asarray(dy, np.float64)
    off = np.concatenate([[0], np.cumsum(counts)])
    pres = (nbr >= 0).astype(np.float64)
    return np.stack([pres[:, s:e] @ dy[s:e] for s, e in zip(off[:-1], off[1:])])


def dense_conv(W, x, nbr):
    """SubMConv3d through a neighbour table: y_i = sum_t W[:, t, :] x[nbr[t][i]];  W [cout][T][cin], float64."""
    W, x = np.asarray(W, np.float64), np.asarray(x, np.float64)
    y = np.zeros((x.shape[0], W.shape[0]))
    for t in range(nbr.shape[0]):
        rows = np.nonzero(nbr[t] >= 0)[0]
        y[rows] += x[nbr[t][rows]] @ W[:, t, :].T
    return y


def dense_conv_grads(W, x, nbr, dy):
    """-> (dW [cout][T][cin], dx [n][cin]) of dense_conv for the output gradient dy."""
    W, x, dy = np.asarray(W, np.float64), np.asarray(x, np.float64), np.asarray(dy, np.float64)
    dW, dx = np.zeros_like(W), np.zeros_like(x)
    for t in range(nbr.shape[0]):
        rows = np.nonzero(nbr[t] >= 0)[0]
        dW[:, t, :] = dy[rows].T @ x[nbr[t][rows]]
        np.add.at(dx, nbr[t][rows], dy[rows] @ W[:, t, :])
    return dW, dx


def repeat_context(cvec, counts):
    return np.repeat(np.asarray(cvec), counts, axis=0)


def tap_table(cvec, W_ctx):
    """P[b][t] = W_ctx[:, t, :] ctx_b;  W_ctx [cout][T][Cc] -> [B][T][cout]."""
    return np.einsum("otc,bc->bto", np.asarray(W_ctx, np.float64), np.asarray(cvec, np.float64))


# ------------------------------------------------------------------------------------------ scenes (real tables)
def _cube():
    g = np.arange(5)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def scene(name):
    """-> (pc_fts f32 [N][7], counts, txt_lens, relative grid).  'cube': every cloud holds a full 5x5x5 block of voxels (its centre
    row has all 125 taps) plus scattered voxels; 'isolated': voxels 6 cells apart (the centre tap only); 'dups': random points in
    a small box, many sharing a voxel."""
    import edge_layouts as el

    rng = np.random.default_rng({"cube": 5, "isolated": 6, "dups": 7}[name])
    if name == "cube":
        counts, grids = [125, 200, 1150], []
        for c in counts:
            extra = el._distinct_voxels(rng, c - 125, 14) + np.array([6, 0, 0])   # beside the cube, the nearest within its taps
            grids.append(np.concatenate([_cube(), extra])[rng.permutation(c)])
        return el.from_grid(np.concatenate(grids), counts, [1] * 3, seed=5)
    if name == "isolated":
        counts = [1, 63, 64, 65, 257]
        grids = [el._distinct_voxels(rng, c, 8) * 6 for c in counts]
        return el.from_grid(np.concatenate(grids), counts, [1] * 5, seed=6)
    counts = [300, 77, 1030]
    grids = [rng.integers(0, 6, size=(c, 3)) for c in counts]
    return el.from_grid(np.concatenate(grids), counts, [1] * 3, seed=7)


def scene_table(name):
    """The oracle's 5^3 neighbour table of the scene, [125][n] int32, with the properties the scene is there for asserted."""
    from frontend_util import count_duplicates, fe

    pc, counts, txt, rel = scene(name)
    batch = cloud_of(counts).astype(np.int32)
    nbr = np.ascontiguousarray(fe.neighbour_table(rel, batch, 5).T.astype(np.int32))
    taps = (nbr >= 0).sum(0)
    off = np.concatenate([[0], np.cumsum(counts)])
    if name == "cube":
        assert all((taps[s:e] == 125).any() for s, e in zip(off[:-1], off[1:])), "a cloud without a row of 125 taps"
    elif name == "isolated":
        assert (taps == 1).all() and (nbr[62] >= 0).all()
    else:
        assert count_duplicates(rel, batch) > 100
    for s, e in zip(off[:-1], off[1:]):     # a neighbour is always in the same cloud
        v = nbr[:, s:e]
        assert ((v < 0) | ((v >= s) & (v < e))).all()
    return pc, counts, nbr


# ------------------------------------------------------------------------------------------ kernel rows
Row = collections.namedtuple("Row", "id counts T C table add why")

LAYOUTS = {"one": [1], "head": [1, 63, 64, 65, 257], "mixed": [40, 1, 4099, 1, 129], "big": [70001], "tiny70": [3] * 70,
           "chunk": [CT_ROWS - 1, CT_ROWS, CT_ROWS + 1],
           "btile": [CT_SPLITS * CT_BTILE - 1, CT_SPLITS * (CT_BTILE + 1)]}


def _r(layout, T, C, add, why, table="random"):
    return Row(f"{layout}-T{T}-C{C}-{'add' if add else 'null'}" + ("" if table == "random" else "-" + table),
               tuple(LAYOUTS[layout]) if table == "random" else None, T, C, table, add, why)


ROWS = [
    _r("one", 1, 4, False, "one row, one tap, one quad: 255 idle threads, 31 of 32 backward chunks empty"),
    _r("one", 125, max_width(125), True, f"the widest C at T = 125 ({max_width(125)}): 127 KB of LDS forward, 135 KB backward (the raised limit)"),
    _r("head", 27, 32, True, "clouds of 1, 63, 64, 65, 257 rows: chunks of one wave of rows -1, +0, +1, two chunks + 1 row; hi word empty"),
    _r("head", 125, 68, False, "C = 68: 17 quads per row, a row's quads straddle waves; both presence words"),
    _r("mixed", 125, 32, True, "a cloud of 4099 rows: 33 forward chunks, the last of 3 rows; backward chunks of 128 - 129 rows"),
    _r("mixed", 27, 64, False, "clouds of one row between large ones: blocks that return at once beside working ones"),
    _r("big", 125, 32, True, "70 001 rows: 547 forward chunks, backward chunks of 2187 - 2188 rows in 5 mask tiles"),
    _r("big", 1, 4, False, "70 001 rows of one quad: items = rows"),
    _r("tiny70", 125, 64, True, "70 clouds of 3 rows: more clouds than rows per cloud, 29 of 32 backward chunks empty"),
    _r("chunk", 125, 64, True, f"clouds of {CT_ROWS - 1}, {CT_ROWS}, {CT_ROWS + 1} rows: one chunk short, exactly one, one chunk + 1 row"),
    _r("chunk", 27, 4, False, "... at one quad per row"),
    _r("btile", 27, 32, True, f"backward chunks of {CT_BTILE - 1} - {CT_BTILE} rows (one mask tile) and of {CT_BTILE + 1} (a second tile of one row)"),
    _r("cube", 125, 32, True, "front-end table, full 5x5x5 blocks: rows with all 125 taps", table="cube"),
    _r("isolated", 125, 64, False, "front-end table, isolated voxels: the centre tap (62) only, 124 exact-zero dP rows", table="isolated"),
    _r("dups", 125, 32, True, "front-end table with duplicate voxels", table="dups"),
]


def absent_tap(b, T):
    """The tap that the random table of cloud b never sets (T = 1: clouds with an odd index have no tap at all)."""
    return (7 * b + 3) % T if T > 1 else (0 if b % 2 == 1 else None)


def row_table(row):
    """-> (counts, nbr int32 [T][n]).  Random tables: presence with probability 0.3, present entries hold arbitrary non-negative
    values (only the sign is read), absent_tap(b, T) never occurs in cloud b."""
    if row.table != "random":
        _, counts, nbr = scene_table(row.table)
        return counts, nbr
    counts = list(row.counts)
    n = sum(counts)
    rng = np.random.default_rng([row.T, row.C, n])
    nbr = np.where(rng.random((row.T, n)) < 0.3, rng.integers(0, 2 ** 31 - 1, size=(row.T, n)), -1).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(counts)])
    for b, (s, e) in enumerate(zip(off[:-1], off[1:])):
        t = absent_tap(b, row.T)
        if t is not None:
            nbr[t, s:e] = -rng.integers(1, 1000, size=e - s)
    return counts, nbr


def row_inputs(row, counts):
    """-> (P [B][T][C], add [n][C] | None, dy [n][C]) float32."""
    B, n = len(counts), sum(counts)
    rng = np.random.default_rng([17, row.T, row.C, n])
    P = rng.standard_normal((B, row.T, row.C)).astype(np.float32)
    add = rng.standard_normal((n, row.C)).astype(np.float32) if row.add else None
    return P, add, rng.standard_normal((n, row.C)).astype(np.float32)


def self_check():
    """Every row enters the branch it names, under the geometry constants above."""
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids)
    assert {r.C for r in ROWS} >= {4, 32, 64, 68, max_width(125)} and {r.T for r in ROWS} == {1, 27, 125}
    assert max_width(125) == 260 and 125 * (max_width(125) + 4) > CT_MAX_TC and max_width(128) == 256
    assert {r.table for r in ROWS} == {"random", "cube", "isolated", "dups"}
    assert any(r.add for r in ROWS) and any(not r.add for r in ROWS)
    layouts = {r.counts for r in ROWS if r.counts}
    assert layouts == {tuple(v) for v in LAYOUTS.values()}
    for r in ROWS:
        assert r.C % 4 == 0 and 0 < r.T <= CT_TMAX and r.T * r.C <= CT_MAX_TC, r.id
        counts, nbr = row_table(r)
        assert nbr.shape == (r.T, sum(counts)) and nbr.dtype == np.int32
        if r.table == "random":
            off = np.concatenate([[0], np.cumsum(counts)])
            for b, (s, e) in enumerate(zip(off[:-1], off[1:])):
                t = absent_tap(b, r.T)
                assert t is None or not (nbr[t, s:e] >= 0).any()
            assert (nbr >= 0).any() or sum(counts) == 1
    big = LAYOUTS["big"][0]
    assert -(-big // CT_ROWS) == 547 and 4 * CT_BTILE < big // CT_SPLITS == 2187 < 5 * CT_BTILE
    assert -(-4099 // CT_ROWS) == 33 and 4099 - 32 * CT_ROWS == 3 and 4099 // CT_SPLITS == 128
    a, b = LAYOUTS["btile"]
    assert {a * (s + 1) // CT_SPLITS - a * s // CT_SPLITS for s in range(CT_SPLITS)} == {CT_BTILE - 1, CT_BTILE}
    assert {b * (s + 1) // CT_SPLITS - b * s // CT_SPLITS for s in range(CT_SPLITS)} == {CT_BTILE + 1}
    return len(ROWS)


# ------------------------------------------------------------------------------------------ fixtures
# name: (configuration, clouds, points, ragged, data seed, weight seed, train, the reference's own forward)
#   'tiny': the tiny networks with use_ee_pose and use_step_id on, qk_norm True, 7 + 256 input channels (two stages: the head is
#           called as forward does);  'yaml_dp0': the YAML's MODEL section with model_class Concat, in_channels 262 and the three
#           PDNorm flags off, drop_path 0 (DropPath draws cannot be shared between implementations);  'yaml': the same, drop_path
#           untouched (the identity in eval mode)
CASES = {
    "concat_tiny_train": ("tiny", 2, 512, True, 81, 91, True, False),
    "concat_yaml_train": ("yaml_dp0", 2, 1024, True, 82, 92, True, True),
    "concat_yaml_eval": ("yaml", 2, 1024, True, 83, 92, False, True),
}


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    kind = CASES[name][0]
    if kind == "tiny":
        return lcfg.preset("concat_tiny")
    cfg = lcfg.preset("concat_yaml")
    if kind == "yaml_dp0":
        cfg.ptv3_config.drop_path = 0.0
    return cfg


def case_batch(name):
    """The synth batch of the case with one instruction token per cloud; the YAML cases keep 6 input channels (xyz, rgb) and take
    'euler' labels that reach both branches of the closest-of-two selection."""
    from robot_3dlotus_amd import synth
    import adanorm_util as au
    import reghead_util as ru

    kind, B, n, ragged, dseed = CASES[name][:5]
    batch = au.last_token_batch(synth.synth_batch(B, n, ragged=ragged, seed=dseed))
    if kind != "tiny":
        batch["pc_fts"] = batch["pc_fts"][:, :6].contiguous()
        gt = batch["gt_actions"]
        batch["gt_actions"] = torch.cat([gt[:, :3], torch.from_numpy(ru.rot_labels("euler", B, dseed)), gt[:, -1:]], 1)
    return batch


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
