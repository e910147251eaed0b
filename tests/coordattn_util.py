"""Shared helpers of the tests of the coordinate term of the patch attention (add_coords_in_attn 'qk' / 'qkv',
PointTransformerV3/model.py:396-398, 484-495; csrc/coord_attn.hip): float64 restatements of the two kernels and of the two modes
of one attention input, the geometry of the kernels' launch plan restated as data, a float32 simulation of the weight gradient's
summation order, the table of kernel rows, and the case table / batch / configuration of the fixtures of
tests/golden/make_golden_coordattn.py.  No reference import here (the GPU tests use this module too)."""
import collections
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KERNEL_TOL = 2e-5  # x max(1, |ref|max): the project's per-kernel bar

# geometry of csrc/coord_attn.hip (lotus_coord_add_plan reports it; tests/test_gpu_coord_add.py compares)
CA_ROWS = 64      # rows per forward block
CA_RPT = 16       # rows a weight-gradient thread sums in fp32 before the sum goes into float64
CA_SPLITS = 256   # most row ranges of the weight gradient
CA_MAX_C = 2048


def quad_lanes(Cw):
    qx = 1
    while qx < 64 and qx < Cw // 4:
        qx *= 2
    return qx


def plan(n, W, Cw):
    """What lotus_coord_add_plan(n, W, Cw) reports: [rows per forward block, forward blocks, row ranges (splits) of the weight
    gradient, rows per thread and fp32 chunk, quad lanes, row lanes]."""
    qx = quad_lanes(Cw)
    rl = 256 // qx
    s = min(max(-(-n // (rl * CA_RPT)), 1), CA_SPLITS)
    return [CA_ROWS, -(-n // CA_ROWS), s, CA_RPT, qx, rl]


def chunks_per_thread(n, W, Cw):
    """Most fp32 chunks a weight-gradient thread folds into its float64 accumulator (1: the range fits one chunk per thread)."""
    _, _, S, rpt, _, rl = plan(n, W, Cw)
    rows = max((n * (s + 1) // S - n * s // S for s in range(S)), default=0)
    return -(-(-(-rows // rl)) // rpt)


# ------------------------------------------------------------------------------------------ float64 restatements
def coord_add_fwd(y, W, Cw, coord, P):
    """y[i][j] + sum_k coord[i][k] P[j % Cw][k] for j < W, the other columns as they are -> float64 [n][ld]."""
    out = np.array(y, dtype=np.float64)
    t = np.asarray(coord, np.float64) @ np.asarray(P, np.float64).T
    for h in range(W // Cw):
        out[:, h * Cw:(h + 1) * Cw] += t
    return out


def coord_add_wgrad(dy, W, Cw, coord):
    """dP[c][k] = sum_i sum_{h: c + h Cw < W} dy[i][c + h Cw] coord[i][k] -> float64 [Cw][3]."""
    dy = np.asarray(dy, np.float64)
    g = sum(dy[:, h * Cw:(h + 1) * Cw] for h in range(W // Cw))
    return g.T @ np.asarray(coord, np.float64)


def attn_input(mode, normed, coord, P, wqkv, bqkv):
    """qkv [n][3C] of one SerializedAttention in float64 (model.py:484-495): 'qkv' projects normed + coord P^T, 'qk' adds
    coord P^T to the q and the k columns of the projection, None / 'none' is the plain projection."""
    x, c, P, w, b = (np.asarray(t, np.float64) for t in (normed, coord, P, wqkv, bqkv))
    C = x.shape[1]
    t = c @ P.T
    if mode == "qkv":
        return (x + t) @ w.T + b
    qkv = x @ w.T + b
    if mode == "qk":
        qkv[:, :C] += t
        qkv[:, C:2 * C] += t
    return qkv


# ------------------------------------------------------------------------------------------ float32 simulation of the plan
def _fma32(a, b, c):
    # (the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32, which differs from a
    # fused multiply-add in rare double-rounding cases only: this simulation bounds the error of the order, it is not a bit model)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def wgrad_plan_sim(dy, W, Cw, coord):
    """lotus_coord_add_wgrad's summation order on the CPU: per row range, thread (quad, row lane) takes rows lane, lane + RL, ...,
    sums CA_RPT of them at a time in float32 (h = 0 then h = 1 within a row), and everything above — a thread's chunks, the row
    lanes, the ranges — in float64 -> float64 [Cw][3]."""
    n = dy.shape[0]
    _, _, S, rpt, _, rl = plan(n, W, Cw)
    nh = W // Cw
    total = np.zeros((Cw, 3), np.float64)
    for s in range(S):
        r0, r1 = n * s // S, n * (s + 1) // S
        rows = r1 - r0
        if rows == 0:
            continue
        T = -(-rows // rl)
        T = -(-T // rpt) * rpt
        d = np.zeros((T * rl, nh, Cw), np.float32)     # rows past the range add an exact +0
        c = np.zeros((T * rl, 3), np.float32)
        d[:rows] = dy[r0:r1, :W].reshape(rows, nh, Cw)
        c[:rows] = coord[r0:r1]
        d = d.reshape(T // rpt, rpt, rl, nh, Cw)
        c = c.reshape(T // rpt, rpt, rl, 3)
        acc = np.zeros((T // rpt, rl, Cw, 3), np.float32)
        for t in range(rpt):
            for h in range(nh):
                acc = _fma32(d[:, t, :, h, :, None], c[:, t, :, None, :], acc)
        total += acc.astype(np.float64).sum(axis=(0, 1))
    return total


# ------------------------------------------------------------------------------------------ kernel rows
Row = collections.namedtuple("Row", "id n Cw form coord_ld coords why branch")
# form 'qk': y = [q | k | v], ld = 3 Cw, W = 2 Cw (the v columns must stay as they are); 'qkv': y = the normed rows, ld = W = Cw
# coords 'unit': randn; 'zero': all zero; 'wide': uniform in [-50, 50] (xyz_norm False: metres times the voxel scale)
# branch = (forward blocks, weight-gradient ranges, most fp32 chunks per thread)


def dims(row):
    return (3 * row.Cw, 2 * row.Cw) if row.form == "qk" else (row.Cw, row.Cw)


def _r(n, Cw, form, coord_ld, why, branch, coords="unit"):
    return Row(f"n{n}-C{Cw}-{form}-ld{coord_ld}" + ("" if coords == "unit" else "-" + coords), n, Cw, form, coord_ld, coords, why,
               branch)


ROWS = [
    _r(1, 4, "qk", 3, "one row of two quads: 254 idle threads forward; one live thread in the weight gradient", (1, 1, 1)),
    _r(63, 36, "qkv", 7, "a forward block one row short; 9 quads under 16 quad lanes (7 idle), coordinates inside pc_fts", (1, 1, 1)),
    _r(64, 36, "qk", 3, "exactly one forward block; 18 quads per row, the k half re-reads the projection's quads", (1, 1, 1)),
    _r(65, 64, "qk", 7, "a second forward block of one row", (2, 1, 1)),
    _r(65, 2048, "qkv", 3, "the widest projection (24 KB of LDS); 8 column tiles of 64 quad lanes, 4 row lanes: two ranges", (2, 2, 1)),
    _r(64, 512, "qkv", 3, "C = 512: a range of 4 row lanes x 16 rows, exactly one", (1, 1, 1)),
    _r(65, 512, "qkv", 7, "C = 512: one row more than a range, two ranges of 32 and 33 rows", (2, 2, 1)),
    _r(256, 64, "qk", 3, "C = 64: 16 row lanes x 16 rows, exactly one range", (4, 1, 1)),
    _r(257, 64, "qkv", 3, "C = 64: one row over a range -> two ranges", (5, 2, 1)),
    _r(256, 36, "qkv", 3, "C = 36 under the geometry of C = 64 (16 quad lanes, 7 idle): exactly one range", (4, 1, 1)),
    _r(257, 36, "qk", 7, "... one row more: two ranges", (5, 2, 1)),
    _r(257, 64, "qk", 3, "all-zero coordinates: y comes back bit for bit, dP is an exact 0", (5, 2, 1), coords="zero"),
    _r(4096, 4, "qk", 3, "C = 4: 256 row lanes x 16 rows, exactly one range", (64, 1, 1)),
    _r(4099, 4, "qkv", 7, "C = 4: three rows over a range -> two ranges; items = rows forward", (65, 2, 1)),
    _r(4099, 512, "qk", 3, "65 ranges of 63 - 64 rows, two column tiles; the last forward block has 3 rows", (65, 65, 1)),
    _r(4099, 64, "qk", 7, "|coord| up to 50 (xyz_norm False)", (65, 17, 1), coords="wide"),
    _r(16384, 512, "qkv", 3, "C = 512: 256 ranges of exactly one chunk per thread (the range count stops growing here)", (256, 256, 1)),
    _r(16385, 512, "qkv", 3, "... one row more: a range of 65 rows, a thread with 17 rows folds a second chunk", (257, 256, 2)),
    _r(65536, 64, "qkv", 3, "C = 64: 256 ranges of exactly one chunk per thread", (1024, 256, 1)),
    _r(65537, 64, "qkv", 7, "... one row more: a second chunk", (1025, 256, 2)),
    _r(70001, 64, "qk", 7, "70 001 rows: ranges of 273 - 274 rows, 18 rows per thread in two chunks", (1094, 256, 2)),
    _r(70001, 4, "qkv", 3, "70 001 rows of one quad: 18 ranges of 3888 - 3889 rows", (1094, 18, 1)),
]


def row_inputs(row):
    """-> (y [n][ld], coordinate buffer [n][coord_ld] (the coordinates are its first three columns), P [Cw][3], dy [n][ld]),
    float32."""
    ld, _ = dims(row)
    rng = np.random.default_rng([23, row.n, row.Cw, ld, row.coord_ld])
    y = rng.standard_normal((row.n, ld)).astype(np.float32)
    buf = rng.standard_normal((row.n, row.coord_ld)).astype(np.float32)
    if row.coords == "zero":
        buf[:, :3] = 0.0
    elif row.coords == "wide":
        buf[:, :3] = rng.uniform(-50.0, 50.0, size=(row.n, 3)).astype(np.float32)
    P = (rng.standard_normal((row.Cw, 3)) * 0.5).astype(np.float32)
    dy = rng.standard_normal((row.n, ld)).astype(np.float32)
    return y, buf, P, dy


def self_check():
    """Every row lands in the branch it names under the geometry above, the rows cover what they are there for, and the
    float32 summation order of the weight-gradient plan alone stays under a quarter of the bar on every row's inputs."""
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids)
    assert {r.n for r in ROWS} >= {1, 63, 64, 65, 257, 4099, 70001}
    assert {r.Cw for r in ROWS} >= {4, 36, 64, 512} and max(r.Cw for r in ROWS) == CA_MAX_C
    assert {r.form for r in ROWS} == {"qk", "qkv"} and {r.coord_ld for r in ROWS} == {3, 7}
    assert {r.coords for r in ROWS} == {"unit", "zero", "wide"}
    assert [quad_lanes(c) for c in (4, 8, 36, 64, 256, 512, 2048)] == [1, 2, 16, 16, 64, 64, 64]
    for Cw in (4, 36, 64, 512):  # one below and one above every boundary of the plan, per width
        ns = {r.n for r in ROWS if r.Cw == Cw}
        per = 256 // quad_lanes(Cw) * CA_RPT
        assert {per, per + 1} <= ns or {per, per + 3} <= ns, (Cw, per)          # one range | two
    for Cw in (64, 512):
        ns = {r.n for r in ROWS if r.Cw == Cw}
        per = 256 // quad_lanes(Cw) * CA_RPT
        assert {CA_SPLITS * per, CA_SPLITS * per + 1} <= ns, Cw                     # one chunk per thread | two
    assert {CA_ROWS - 1, CA_ROWS, CA_ROWS + 1} <= {r.n for r in ROWS}               # forward blocks
    worst = 0.0
    for r in ROWS:
        ld, W = dims(r)
        assert r.Cw % 4 == 0 and r.Cw <= CA_MAX_C and W in (r.Cw, 2 * r.Cw) and ld >= W
        p = plan(r.n, W, r.Cw)
        assert (p[1], p[2], chunks_per_thread(r.n, W, r.Cw)) == r.branch, (r.id, p, chunks_per_thread(r.n, W, r.Cw))
        y, buf, P, dy = row_inputs(r)
        coord = buf[:, :3]
        ref = coord_add_wgrad(dy[:, :W], W, r.Cw, coord)
        sim = wgrad_plan_sim(dy, W, r.Cw, coord)
        rel = float(np.abs(sim - ref).max()) / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, rel)
        assert rel <= 0.25 * KERNEL_TOL, (r.id, rel)
        if r.coords == "zero":
            assert not ref.any() and not sim.any()
    return len(ROWS), worst


# ------------------------------------------------------------------------------------------ fixtures
# name: (family, preset, clouds, points, ragged, data seed, weight seed, train, the reference's own forward)
#   family 'adanorm' / 'concat': SimplePolicyPTV3AdaNorm / SimplePolicyPTV3Concat, 'mp_ada': MotionPlannerPTV3AdaNorm.  The tiny
#   cases have two stages (the pooled coordinates of level 1 enter the term) and call the head as forward does; the YAML case is
#   simple_policy_ptv3.yaml with add_coords_in_attn 'qk', untouched otherwise, in eval mode through the reference's own forward.
CASES = {
    "coord_adanorm_tiny_qk_train": ("adanorm", "adanorm_tiny_qk", 2, 512, False, 41, 51, True, False),
    "coord_adanorm_tiny_qkv_train": ("adanorm", "adanorm_tiny_qkv", 2, 512, True, 42, 52, True, False),
    "coord_concat_tiny_qk_train": ("concat", "concat_tiny_qk", 2, 512, True, 43, 53, True, False),
    "coord_concat_tiny_qkv_train": ("concat", "concat_tiny_qkv", 2, 512, False, 44, 54, True, False),
    "coord_mp_ada_tiny_qkv_train": ("mp_ada", "mp_ada_tiny_qkv", 2, 512, True, 45, 55, True, True),
    "coord_adanorm_yaml_qk_eval": ("adanorm", "adanorm_yaml_qk", 2, 1024, True, 46, 56, False, True),
}
# the fixture each one may not outgrow (tests/golden/plain_adanorm_*.npz)
SIZE_PEER = {name: ("plain_adanorm_yaml_eval" if name.endswith("_eval") else "plain_adanorm_tiny_train") for name in CASES}


XT_SAMPLE = 12288  # position logits kept by a train-mode fixture: fewer than adanorm_util.XT_SAMPLE, which pays for the extra
#                    gradient entries of coords_proj (a fixture here is no larger than its plain_adanorm_* counterpart)


def xt_sample_index(numel):
    """Fixed positions (sorted) of the flattened position logits that a train-mode fixture stores."""
    return np.sort(np.random.default_rng([29, numel]).choice(numel, min(XT_SAMPLE, numel), replace=False))


def case_mode(name):
    return "qkv" if "_qkv_" in name else "qk"


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    cfg = lcfg.preset(CASES[name][1])
    if CASES[name][0] != "mp_ada":
        cfg.action_config.txt_reduce = "mean"
    return cfg


def case_batch(name):
    """The synth batch of the case with one instruction token per cloud (txt_reduce 'mean'); the YAML case keeps 6 input channels
    (xyz, rgb) and takes 'euler' labels, as the plain_adanorm_yaml cases do."""
    import torch
    from robot_3dlotus_amd import synth
    import adanorm_util as au
    import mp_ada_util as mu
    import reghead_util as ru

    family, preset, B, n, ragged, dseed = CASES[name][:6]
    if family == "mp_ada":
        return mu.mp_batch(B, n, ragged, dseed, 4)
    batch = au.last_token_batch(synth.synth_batch(B, n, ragged=ragged, seed=dseed))
    if "yaml" in preset:
        batch["pc_fts"] = batch["pc_fts"][:, :6].contiguous()
        gt = batch["gt_actions"]
        batch["gt_actions"] = torch.cat([gt[:, :3], torch.from_numpy(ru.rot_labels("euler", B, dseed)), gt[:, -1:]], 1)
    return batch


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
