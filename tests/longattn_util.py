"""Shared helpers of the tests of patch sizes above 128 (PointTransformerV3/model.py:529-551; csrc/attention_long.hip): a float64
restatement of the patch attention over a tile list with arbitrary q_len / k_len (torch, differentiable; the shape of
rpe_util.attention_ref without the position term), the dropout mask of the long kernels restated in numpy from the numbering in
include/lotus_hip.h, the table of kernel rows — each names the branch it drives —, their CPU self-check, and the case table /
batch / configuration of the fixtures of tests/golden/make_golden_longattn.py.  No reference import here (the GPU tests use this
module too)."""
import collections
import os

import numpy as np
import torch

import rpe_util as ru
from oracle import front_end as fe

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LONG_MAX = 1024  # LOTUS_ATTN_LONG_MAX
IMG = 128        # rows of a key image / a query slab
FWD_LDS, BWD_LDS = 57344, 75264  # dynamic LDS of the long kernels (include/lotus_hip.h, families 8 / 9)


# ------------------------------------------------------------------------------------------ the dropout mask
def drop_threshold(drop_p):
    """The 32-bit threshold the kernels compare with: (uint32)(drop_p * 2^32) of the float32 rate, at least 1."""
    return max(1, int(float(np.float32(drop_p)) * 4294967296.0))


def keep_mask(tile, H, Lq, Lk, seed, drop_p):
    """0 / 1 float64 [H][Lq][Lk] of one tile: element (tile, h, i, j) has idx = ((tile * H + h) * 1024 + i) * 1024 + j;
    x = lo(idx) * 0x9E3779B1 + lo(seed); x ^= hi(idx) * 0x7FEB352D + hi(seed); x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15;
    keep iff x >= threshold (all in uint32)."""
    M = np.uint64(0xFFFFFFFF)
    h = np.arange(H, dtype=np.uint64)[:, None, None]
    i = np.arange(Lq, dtype=np.uint64)[None, :, None]
    j = np.arange(Lk, dtype=np.uint64)[None, None, :]
    idx = ((np.uint64(tile) * np.uint64(H) + h) * np.uint64(LONG_MAX) + i) * np.uint64(LONG_MAX) + j
    lo, hi = idx & M, idx >> np.uint64(32)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    x = (lo * np.uint64(0x9E3779B1) + s_lo) & M
    x ^= (hi * np.uint64(0x7FEB352D) + s_hi) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    return (x >= np.uint64(drop_threshold(drop_p))).astype(np.float64)


# ------------------------------------------------------------------------------------------ float64 patch attention
def attention_ref(qkv, gidx, owner_pos, tiles, H, qn=None, kn=None, keep=None, drop_p=0.0):
    """Patch attention over a tile list in float64 (torch; differentiable in qkv and the norm parameters).  qkv [n][3C]; gidx
    [npad]: the row of every position; owner_pos [n]: the position whose output row i takes; tiles [nt][4] = q_start, q_len,
    k_start, k_len in positions (any lengths); keep: None or one 0 / 1 array [H][q_len][k_len] per tile (dropout on the
    probabilities, scaled 1 / (1 - drop_p)).  Every position is a query of exactly one tile.
    -> (out [n][C], lse [npad][H])."""
    n, C3 = qkv.shape
    C = C3 // 3
    d = C // H
    x = qkv[torch.as_tensor(np.asarray(gidx), dtype=torch.long)].reshape(-1, 3, H, d)
    q, k, v = x.unbind(1)
    if qn is not None:
        q = torch.nn.functional.layer_norm(q, (d,), qn[0], qn[1], 1e-6)
        k = torch.nn.functional.layer_norm(k, (d,), kn[0], kn[1], 1e-6)
    npad = x.shape[0]
    out = [None] * len(tiles)
    lse = [None] * len(tiles)
    covered = np.zeros(npad, np.int64)
    for t, (qs, ql, ks, kl) in enumerate(np.asarray(tiles).tolist()):
        s = (q[qs:qs + ql].transpose(0, 1) * d ** -0.5) @ k[ks:ks + kl].transpose(0, 1).transpose(1, 2)   # [H][ql][kl]
        lse[t] = torch.logsumexp(s, -1).transpose(0, 1)
        p = torch.softmax(s, -1)
        if keep is not None:
            p = p * torch.from_numpy(keep[t]) / (1.0 - float(np.float32(drop_p)))
        out[t] = (p @ v[ks:ks + kl].transpose(0, 1)).transpose(0, 1).reshape(ql, C)
        covered[qs:qs + ql] += 1
    assert (covered == 1).all(), "every position is a query of exactly one tile, in order"
    starts = [int(t[0]) for t in np.asarray(tiles)]
    assert starts == sorted(starts)
    out, lse = torch.cat(out, 0), torch.cat(lse, 0)
    return out[torch.as_tensor(np.asarray(owner_pos), dtype=torch.long)], lse


# ------------------------------------------------------------------------------------------ kernel rows
Row = collections.namedtuple("Row", "id counts K H d norm drop wide why")
ROWS = [
    Row("k129", [129], 256, 1, 16, False, 0.0, False, "one tile of 129 rows: the smallest second key image, one key in it"),
    Row("k256", [256], 256, 4, 32, True, 0.0, False, "one full patch of 256: two full images and slabs; head width 32, four heads"),
    Row("k257", [257], 512, 1, 24, True, 0.0, False, "257 = 2 * 128 + 1: a third image and a third slab of one row; head width 24"),
    Row("one_and_200", [1, 200], 256, 4, 16, True, 0.0, False,
        "a one-row cloud next to a short cloud that is one tile of 200 rows (no multiple of 128)"),
    Row("k1024", [1024], 1024, 1, 32, True, 0.0, False, "the longest tile: eight images, eight slabs"),
    Row("borrowed", [300, 131], 256, 4, 24, True, 0.0, False,
        "a padded cloud whose tail patch borrows 212 rows (dkv_extra) and a 131-row cloud that is one tile"),
    Row("dropout", [260], 256, 2, 16, False, 0.1, False, "dropout 0.1 on the probabilities; the tail patch borrows 252 rows"),
    Row("wide", [258], 512, 1, 16, False, 0.0, True,
        "scores spanning a wide range: q and k are laid out so that the running maximum rises at every key image (the rescale)"),
]
ROW = {r.id: r for r in ROWS}
DETERMINISM_ROWS = ("k257", "borrowed", "dropout")
SHORT_ROWS = [  # tiles of at most 128 rows given to the long entry points: they must agree with the 128-row exact-fp32 kernels
    Row("short_full", [128], 128, 2, 16, True, 0.0, False, "one full 128 x 128 tile"),
    Row("short_borrowed", [150, 77], 128, 4, 8, False, 0.0, False, "the tail patch borrows 106 rows; a 77-row cloud"),
]
SHORT_ROW = {r.id: r for r in SHORT_ROWS}
WIDE_STEP = 6.0  # score units by which an image's maximum exceeds the previous one's in the 'wide' row


def row_inputs(row):
    """-> dict of float32 / int tensors (CPU): qkv [n][3C], dout [n][C], qn / kn (weight, bias) or None, order (a serialised order:
    a permutation inside every cloud), the patch tables (rpe_util.patch_tables), gidx, owner_pos, seed."""
    n, C = sum(row.counts), row.H * row.d
    g = torch.Generator().manual_seed(2000 + n + row.K + row.H)
    qkv = torch.randn(n, 3 * C, generator=g) * 1.5
    dout = torch.randn(n, C, generator=g)
    qn = kn = None
    if row.norm:
        qn = (torch.rand(row.d, generator=g) + 0.5, torch.randn(row.d, generator=g) * 0.2)
        kn = (torch.rand(row.d, generator=g) + 0.5, torch.randn(row.d, generator=g) * 0.2)
    rng = np.random.default_rng([43, n, row.K])
    off = np.concatenate([[0], np.cumsum(row.counts)])
    order = np.concatenate([off[i] + rng.permutation(c) for i, c in enumerate(row.counts)])
    inverse = np.empty_like(order)
    inverse[order] = np.arange(n)
    t = ru.patch_tables(row.counts, row.K)
    gidx = order[t["pad"]].astype(np.int32)
    if row.wide:
        # one cloud, one tile, no norm: column 0 of every query is 4 sqrt(d) / 4 ... the score of (query, key at position p) gets
        # WIDE_STEP * (p // 128) on top of a term within +-1: the maximum of image j + 1 exceeds that of image j for every query
        assert not row.norm and len(row.counts) == 1 and row.counts[0] <= row.K
        pos = inverse  # position of every point inside its (single) tile
        qkv[:, :2 * C] *= 0.25
        for h in range(row.H):
            qkv[:, h * row.d] = 4.0                                             # q column 0 of head h
            qkv[:, C + h * row.d] = torch.from_numpy((pos // IMG).astype(np.float32)) * (WIDE_STEP * row.d ** 0.5 / 4.0)
    return dict(qkv=qkv, dout=dout, qn=qn, kn=kn, order=order, tabs=t, gidx=gidx, owner_pos=t["unpad"][inverse],
                seed=777000 + n)


def row_keep(row, tabs, seed):
    """The dropout masks of the row's tiles (None without dropout)."""
    if not row.drop:
        return None
    return [keep_mask(t, row.H, int(ql), int(kl), seed, row.drop) for t, (_, ql, _, kl) in enumerate(tabs["tiles"])]


def reference(row, v=None):
    """float64 forward and backward of a row -> dict(out, lse, dqkv, norm = [dqn_w, dqn_b, dkn_w, dkn_b] or [])."""
    v = v or row_inputs(row)
    qd = v["qkv"].double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (*v["qn"], *v["kn"])] if row.norm else []
    qn, kn = ((pr[0], pr[1]), (pr[2], pr[3])) if row.norm else (None, None)
    out, lse = attention_ref(qd, v["gidx"], v["owner_pos"], v["tabs"]["tiles"], row.H, qn, kn, row_keep(row, v["tabs"], v["seed"]),
                             row.drop)
    out.backward(v["dout"].double())
    return dict(out=out.detach(), lse=lse.detach(), dqkv=qd.grad, norm=[p.grad for p in pr])


def _sdpa_check(row):
    """The restatement against torch's own attention under autograd, float64, per patch (no dropout)."""
    v = row_inputs(row)
    ref = reference(row, v)
    H, d, C = row.H, row.d, row.H * row.d
    qd = v["qkv"].double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (*v["qn"], *v["kn"])] if row.norm else []
    x = qd[torch.as_tensor(v["gidx"], dtype=torch.long)].reshape(-1, 3, H, d)
    q, k, val = x.unbind(1)
    if row.norm:
        q = torch.nn.functional.layer_norm(q, (d,), pr[0], pr[1], 1e-6)
        k = torch.nn.functional.layer_norm(k, (d,), pr[2], pr[3], 1e-6)
    outs = []
    for qs, ql, ks, kl in v["tabs"]["tiles"].tolist():
        o = torch.nn.functional.scaled_dot_product_attention(q[qs:qs + ql].transpose(0, 1)[None], k[ks:ks + kl].transpose(0, 1)[None],
                                                             val[ks:ks + kl].transpose(0, 1)[None])
        outs.append(o[0].transpose(0, 1).reshape(ql, C))
    out = torch.cat(outs, 0)[torch.as_tensor(v["owner_pos"], dtype=torch.long)]
    out.backward(v["dout"].double())
    worst = float((out.detach() - ref["out"]).abs().max())
    worst = max(worst, float((qd.grad - ref["dqkv"]).abs().max()))
    for a, b in zip(pr, ref["norm"]):
        worst = max(worst, float((a.grad - b).abs().max()))
    return worst


def self_check():
    """The rows are what they say and the restatement is the attention (CPU)."""
    assert len({r.id for r in ROWS + SHORT_ROWS}) == len(ROWS) + len(SHORT_ROWS)
    from robot_3dlotus_amd import frontend
    for r in ROWS:
        assert r.K in frontend.LONG_PATCH_SIZES and r.d % 4 == 0 and 4 <= r.d <= 32, r.id
        t = ru.patch_tables(r.counts, r.K)
        assert t["tiles"][:, 1].max() > IMG and t["tiles"][:, 1].max() <= r.K, r.id
    lens = {r.id: ru.patch_tables(r.counts, r.K)["tiles"][:, 1].tolist() for r in ROWS}
    assert lens["k129"] == [129] and lens["k256"] == [256] and lens["k257"] == [257] and lens["k1024"] == [1024]
    assert lens["one_and_200"] == [1, 200] and lens["borrowed"] == [256, 256, 131] and lens["dropout"] == [256, 256]
    assert ru.patch_tables(ROW["borrowed"].counts, 256)["n_extra"] == 212 and ru.patch_tables(ROW["dropout"].counts, 256)["n_extra"] == 252
    assert {r.d for r in ROWS} == {16, 24, 32} and {r.H for r in ROWS} >= {1, 4} and {r.norm for r in ROWS} == {True, False}
    assert sum(sum(r.counts) for r in ROWS) <= 2900 and max(sum(r.counts) for r in ROWS) <= LONG_MAX
    for r in SHORT_ROWS:
        assert ru.patch_tables(r.counts, r.K)["tiles"][:, 1].max() <= IMG, r.id
    # the wide row: the running maximum rises at every key image, for every query
    w = ROW["wide"]
    v = row_inputs(w)
    x = v["qkv"].double()[torch.as_tensor(v["gidx"], dtype=torch.long)].reshape(-1, 3, w.H, w.d)
    s = (x[:, 0].transpose(0, 1) * w.d ** -0.5) @ x[:, 1].transpose(0, 1).transpose(1, 2)   # [H][258][258]
    m = torch.stack([s[:, :, j:j + IMG].max(-1).values for j in range(0, s.shape[-1], IMG)], -1)
    assert m.shape[-1] == 3 and bool((m[..., 1:] - m[..., :-1] > WIDE_STEP - 3.0).all()), "the running maximum does not move"
    assert float(s.max() - s.min()) > 2 * WIDE_STEP
    # the mask: the kept fraction, and no two tiles / heads alike
    k0, k1 = keep_mask(0, 2, 256, 256, 5, 0.1), keep_mask(1, 2, 256, 256, 5, 0.1)
    assert abs(k0.mean() - 0.9) < 0.01 and abs(k1.mean() - 0.9) < 0.01 and (k0 != k1).mean() > 0.1 and (k0[0] != k0[1]).mean() > 0.1
    assert drop_threshold(0.1) == int(float(np.float32(0.1)) * 2 ** 32) and drop_threshold(1e-12) == 1
    # the restatement against torch's own attention under autograd
    worst = max(_sdpa_check(r) for r in (ROW["k129"], ROW["borrowed"], ROW["one_and_200"], SHORT_ROW["short_borrowed"]))
    assert worst < 1e-10, worst
    return len(ROWS)


# ------------------------------------------------------------------------------------------ the host plan
PLAN_COUNTS = [[256], [300, 131], [700, 200], [1, 513]]


def plan_ref(counts, K):
    """What FrontEnd.patch_plan must return for clouds of `counts` points at patch size K, from the restatement of
    get_padding_and_inverse (oracle.front_end.padding_tables through rpe_util.patch_tables)."""
    t = ru.patch_tables(counts, K)
    return t["off"], t["offp"], t["tiles"], t["blocks"]


# ------------------------------------------------------------------------------------------ fixtures
# name: (family, preset, clouds, points, ragged, data seed, weight seed, train, the reference's own forward) — as rpe_util.CASES
CASES = {
    "long_adanorm_tiny_p256_train": ("adanorm", "adanorm_tiny_p256", 2, 420, True, 23, 81, True, False),
    "long_adanorm_tiny_plain_p256_train": ("adanorm", "adanorm_tiny_plain_p256", 2, 420, True, 35, 82, True, False),
    "long_concat_tiny_p256_train": ("concat", "concat_tiny_p256", 2, 420, True, 81, 83, True, False),
    "long_mp_ada_tiny_p256_train": ("mp_ada", "mp_ada_tiny_p256", 2, 420, True, 82, 84, True, True),
    "long_adanorm_yaml_p1024_eval": ("adanorm", "adanorm_yaml_p1024", 2, 1400, True, 66, 85, False, True),
}
SIZE_PEER = {name: ("plain_adanorm_yaml_eval" if name.endswith("_eval") else "plain_adanorm_tiny_train") for name in CASES}
GRAD_FLOOR = ru.GRAD_FLOOR
XT_SAMPLE = ru.XT_SAMPLE
xt_sample_index = ru.xt_sample_index


def case_patch(name):
    return 1024 if "p1024" in name else 256


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    cfg = lcfg.preset(CASES[name][1])
    if CASES[name][0] != "mp_ada":
        cfg.action_config.txt_reduce = "mean"
    return cfg


def case_batch(name):
    """The synth batch of the case, built as rpe_util.case_batch builds it."""
    saved = ru.CASES.get(name)
    ru.CASES[name] = CASES[name]
    try:
        return ru.case_batch(name)
    finally:
        if saved is None:
            del ru.CASES[name]
        else:
            ru.CASES[name] = saved


def level_facts(batch, n_levels, perms, patch_size):
    """Per level, from the oracle's integer front end (CPU): the clouds' point counts, the tile lengths at `patch_size` and how
    many rows the clouds borrow."""
    counts = [int(c) for c in batch["npoints_in_batch"]]
    levels = fe.build_all_levels(batch["pc_fts"][:, :3].numpy(), counts, n_levels, perms=perms)
    out = []
    for lv in levels[:n_levels]:
        cnt = np.bincount(lv["batch"], minlength=len(counts)).tolist()
        t = ru.patch_tables(cnt, patch_size)
        out.append(dict(counts=cnt, tile_lens=t["tiles"][:, 1].tolist(), borrowed=t["n_extra"]))
    return out


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
