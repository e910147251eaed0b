"""Restatements of the sub-block autograd nodes of robot-3dlotus_amd/ops.py in plain torch under torch autograd (test
infrastructure, not collected): one function per node, written from the reference's module definitions the node docstrings cite
(MLP model.py:577-583, Block :659-672, SerializedPooling :760-790, SerializedUnpooling :817-828, Embedding :844-861, CrossAttention
and CABlock model_ca.py:46-101, :135-140).  No import of the reference tree (the GPU tests use this module too).

Every function computes in the dtype of the tensors it is given: float64 is the reference, float32 (on the CPU, same masks) the
floor of the comparison (node_rows.floor).  The dropout masks enter as tensors computed HERE in numpy integer arithmetic from
(seed, element index), never read from the node under test:
    dense / elementwise  head_run.keep_scale(seed, row * N + col, p): 0 or float32(1 / (1 - t16 / 65536)), t16 = floor(p 65536)
    DropPath             head_run.keep_scale(seed, row, p), one draw per row (head_run._run_droppath)
    attention            idx = ((tile H + h) 128 + q) 128 + key (csrc/attention.hip:67), the hash of longattn_util.keep_mask,
                         keep scale 1 / (1 - p)
and the seed streams are restated from ops.py / ptv3.py as constants: the output projection's dropout on `seed`, the
probabilities on mix(seed, 1); fc1's activation dropout on `seed`, fc2's on mix(seed, 1); DropPath on mix(seed, 5); inside a
Block the MLP gets mix(seed, 2); the CABlock gets mix(si, 8).

`Variant` states one deliberate fault at a time (tests/test_nodes_host.py measures that each moves a compared quantity far above
the row's bar): the node's two seed streams swapped, fc1's mask applied to the pre-activation (before GELU and GELU') instead of
to the activation, the keep scale 1 / (1 - p) instead of the quantised one, a Block's MLP on `seed` instead of mix(seed, 2)."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

import head_run
import longattn_util as lu
from oracle import model as om

LN_EPS, QK_EPS, BN_EPS, BN_MOMENTUM = 1e-5, 1e-6, 1e-3, 0.01
_M64 = (1 << 64) - 1

Variant = collections.namedtuple("Variant", "swap pre_gelu plain_scale mlp_on_seed", defaults=(False, False, False, False))
EXACT = Variant()


def mix_seed(seed, k=0):
    """The splitmix64 finaliser of (seed, k) every dropout site draws its sub-seed from (restated from ops.mix_seed)."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


# ------------------------------------------------------------------------------------------------ masks
def _kept(mask, p):
    """Every mask of at least 4096 elements keeps 1 - p of them to within 0.02 (asserted wherever a mask is made)."""
    if mask.size >= 4096:
        frac = float((mask != 0).mean())
        assert abs(frac - (1.0 - p)) < 0.02, (mask.shape, p, frac)
    return mask


def dense_scale(seed, M, N, p, v=EXACT):
    """float64 numpy [M][N]: 0 or the keep scale of element (m, n) of a dense layer's [M, N] output."""
    if p <= 0.0:
        return np.ones((M, N))
    s = head_run.keep_scale(seed, np.arange(M * N, dtype=np.uint64), p).astype(np.float64).reshape(M, N)
    if v.plain_scale:
        s = (s != 0) * (1.0 / (1.0 - p))
    return _kept(s, p)


def droppath_scale(seed, M, p):
    """float64 numpy [M][1]: DropPath's per-row 0 or keep scale."""
    if p <= 0.0:
        return np.ones((M, 1))
    return _kept(head_run.keep_scale(seed, np.arange(M, dtype=np.uint64), p).astype(np.float64).reshape(M, 1), p)


def attn_keep(tile, H, Lq, Lk, seed, p):
    """0 / 1 float64 numpy [H][Lq][Lk] of one tile of the 128-row attention kernels: longattn_util.keep_mask at row stride 128."""
    M = np.uint64(0xFFFFFFFF)
    h = np.arange(H, dtype=np.uint64)[:, None, None]
    i = np.arange(Lq, dtype=np.uint64)[None, :, None]
    j = np.arange(Lk, dtype=np.uint64)[None, None, :]
    idx = ((np.uint64(tile) * np.uint64(H) + h) * np.uint64(128) + i) * np.uint64(128) + j
    lo, hi = idx & M, idx >> np.uint64(32)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    x = (lo * np.uint64(0x9E3779B1) + s_lo) & M
    x ^= (hi * np.uint64(0x7FEB352D) + s_hi) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    return _kept((x >= np.uint64(lu.drop_threshold(p))).astype(np.float64), p)


def _t(a, like):
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype)


def _streams(seed, v):
    """(first, second) seed stream of a node: (seed, mix(seed, 1)), swapped by the fault `swap`."""
    a, b = int(seed), mix_seed(seed, 1)
    return (b, a) if v.swap else (a, b)


# ------------------------------------------------------------------------------------------------ tables
def self_tables(level):
    """Oracle level (oracle.front_end.build_all_levels) -> the gather tables of curve slot 0 and the tile list of the patch
    attention at patch size 128: gidx [npad], owner_pos [n], tiles [nt][4] = q_start, q_len, k_start, k_len."""
    cu = np.asarray(level["cu_seqlens"], dtype=np.int64)
    tiles = np.stack([cu[:-1], np.diff(cu), cu[:-1], np.diff(cu)], 1)
    return dict(gidx=level["order"][0][level["pad"]], owner_pos=level["unpad"][level["inverse"][0]], tiles=tiles)


def cross_tiles(counts, txt):
    """[nt][4] = q_start, q_len, k_start, k_len: every cloud's rows in runs of 128 against the cloud's own context tokens."""
    off, coff = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(txt)])
    out = []
    for b, (n, l) in enumerate(zip(counts, txt)):
        out += [(off[b] + s, min(128, n - s), coff[b], l) for s in range(0, n, 128)]
    return np.asarray(out, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ attention
def cross_attention(q, kv, tiles, H, qn, kn, keep=None, p=0.0):
    """oracle.model.cross_attention (model_ca.py:46-67) over a tile list, with a keep mask on the probabilities: keep = one 0 / 1
    array [H][q_len][k_len] per tile, scaled 1 / (1 - p)."""
    N, C = q.shape
    d = C // H
    qh = F.layer_norm(q.view(-1, H, d), (d,), qn[0], qn[1], QK_EPS)
    kvh = kv.reshape(-1, 2, H, d)
    k = F.layer_norm(kvh[:, 0], (d,), kn[0], kn[1], QK_EPS)
    val = kvh[:, 1]
    outs, end = [], 0
    for t, (qs, ql, ks, kl) in enumerate(np.asarray(tiles).tolist()):
        assert qs == end, "the tiles cover the rows in order"
        end = qs + ql
        s = torch.einsum("qhd,khd->hqk", qh[qs:qs + ql], k[ks:ks + kl]) * d ** -0.5
        pr = torch.softmax(s, -1)
        if keep is not None:
            pr = pr * _t(keep[t], q) / (1.0 - float(np.float32(p)))
        outs.append(torch.einsum("hqk,khd->qhd", pr, val[ks:ks + kl]).reshape(ql, C))
    assert end == N
    return torch.cat(outs, 0)


def _branch_out(x, br, p, seed, dpath, v):
    """x + DropPath(drop(br)): the output projection's dropout on `seed`, DropPath on mix(seed', 5) of the node's seed."""
    M, C = br.shape
    br = br * _t(dense_scale(seed[0], M, C, p, v), x)
    if dpath > 0.0:
        br = br * _t(droppath_scale(mix_seed(seed[1], 5), M, dpath), x)
    return x + br


# ------------------------------------------------------------------------------------------------ the nodes
def ffn(x, g, b, w1, b1, w2, b2, p, seed, dpath=0.0, v=EXACT):
    """FfnFn: x + DropPath(drop(fc2(drop(GELU(fc1(LN(x)))))))."""
    M, C = x.shape
    s1, s2 = _streams(seed, v)
    h = F.linear(F.layer_norm(x, (C,), g, b, LN_EPS), w1, b1)
    m1 = _t(dense_scale(s1, M, w1.shape[0], p, v), x)
    a = F.gelu(h * m1) if v.pre_gelu else F.gelu(h) * m1
    return _branch_out(x, F.linear(a, w2, b2), p, (s2, seed), dpath, v)


def selfattn(x, g, b, wqkv, bqkv, qn, kn, wp, bp, tabs, H, p, seed, attn_p, dpath=0.0, v=EXACT):
    """SelfAttnFn: x + DropPath(drop(proj(PatchAttention(qkv(LN(x)))))); qn = kn = None: no q/k norm."""
    C = x.shape[1]
    s_proj, s_att = _streams(seed, v)
    qkv = F.linear(F.layer_norm(x, (C,), g, b, LN_EPS), wqkv, bqkv)
    keep = None
    if attn_p > 0.0:
        npdt = np.float64 if x.dtype == torch.float64 else np.float32  # (attention_ref multiplies by the array as it is)
        keep = [attn_keep(t, H, int(ql), int(kl), s_att, attn_p).astype(npdt) for t, (_, ql, _, kl) in enumerate(tabs["tiles"])]
    att, _ = lu.attention_ref(qkv, tabs["gidx"], tabs["owner_pos"], tabs["tiles"], H, qn, kn, keep, attn_p)
    return _branch_out(x, F.linear(att, wp, bp), p, (s_proj, seed), dpath, v)


def crossattn(x, kv, g, b, wq, bq, qn, kn, wp, bp, tiles, H, p, seed, attn_p, v=EXACT):
    """CrossAttnKvFn (and CrossAttnFn with kv = Linear(context)): x + drop(proj(CrossAttention(q(LN(x)), kv)))."""
    C = x.shape[1]
    s_proj, s_att = _streams(seed, v)
    q = F.linear(F.layer_norm(x, (C,), g, b, LN_EPS), wq, bq)
    keep = [attn_keep(t, H, int(ql), int(kl), s_att, attn_p) for t, (_, ql, _, kl) in enumerate(tiles)] if attn_p > 0.0 else None
    att = cross_attention(q, kv, tiles, H, qn, kn, keep, attn_p)
    return _branch_out(x, F.linear(att, wp, bp), p, (s_proj, seed), 0.0, v)


def cpe(x, xs, cw, cb, lw, lb, g, b, nbr27):
    """CpeFn: x + LN(Linear(SubMConv3d_3(xs))); nbr27 [n][27] long, -1 = no neighbour (a duplicate voxel: its lowest row)."""
    C = x.shape[1]
    return x + F.layer_norm(F.linear(om.subm_conv(xs, nbr27, cw, cb), lw, lb), (C,), g, b, LN_EPS)


def batch_norm(x, g, b, rmean, rvar, training):
    """nn.BatchNorm1d(eps 1e-3, momentum 0.01) written out -> (y, new running mean, new running var): batch statistics with the
    biased variance in the normalisation and the unbiased one in the running average; eval: the running statistics."""
    if not training:
        return (x - rmean) / torch.sqrt(rvar + BN_EPS) * g + b, rmean, rvar
    M = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    y = (x - mean) / torch.sqrt(var + BN_EPS) * g + b
    unbiased = var * (M / (M - 1.0)) if M > 1 else var
    return (y, (1 - BN_MOMENTUM) * rmean + BN_MOMENTUM * mean.detach(), (1 - BN_MOMENTUM) * rvar + BN_MOMENTUM * unbiased.detach())


def stem(x, cw, g, b, rmean, rvar, nbr125, training):
    """StemFn: GELU(BN(SubMConv3d_5(x))), no convolution bias -> (y, running mean, running var)."""
    y, rm, rv = batch_norm(om.subm_conv(x, nbr125, cw, None), g, b, rmean, rvar, training)
    return F.gelu(y), rm, rv


def pool(x, w, bias, g, b, rmean, rvar, cluster, n_child, training):
    """PoolFn: GELU(BN(segment_max(Linear(x)))) -> (y, running mean, running var, the projection)."""
    proj = F.linear(x, w, bias)
    idx = cluster.view(-1, 1).expand(-1, proj.shape[1])
    pooled = proj.new_zeros(n_child, proj.shape[1]).scatter_reduce(0, idx, proj, "amax", include_self=False)
    y, rm, rv = batch_norm(pooled, g, b, rmean, rvar, training)
    return F.gelu(y), rm, rv, proj


def unpool(xc, xp, wu, bu, gu, betau, rmu, rvu, ws, bs, gs, betas, rms, rvs, cluster, training):
    """UnpoolFn: up = GELU(BN(Linear(xc))), skip = GELU(BN(Linear_skip(xp))) -> (skip + up[cluster], skip, the four statistics)."""
    up, rmu2, rvu2 = batch_norm(F.linear(xc, wu, bu), gu, betau, rmu, rvu, training)
    skip, rms2, rvs2 = batch_norm(F.linear(xp, ws, bs), gs, betas, rms, rvs, training)
    up, skip = F.gelu(up), F.gelu(skip)
    return skip + up[cluster], skip, (rmu2, rvu2, rms2, rvs2)


def chain(x, P, ctx, tabs, tiles, nbr27, H, p, attn_p, si, v=EXACT):
    """ptv3.Block.run followed by CABlock.run as the composition of the five restatements above.  P: dict of the modules' parameters
    by state-dict name; si: the seed of the block position.  The Block's attention runs on si and its MLP on mix(si, 2); the
    CABlock gets sc = mix(si, 8): its attention on sc, its MLP on mix(sc, 2); its keys / values are Linear(context)."""
    B, Cb = "blk.", "cab."
    x = cpe(x, x, P[B + "cpe.0.weight"], P[B + "cpe.0.bias"], P[B + "cpe.1.weight"], P[B + "cpe.1.bias"], P[B + "cpe.2.weight"],
            P[B + "cpe.2.bias"], nbr27)
    x = selfattn(x, P[B + "norm1.0.weight"], P[B + "norm1.0.bias"], P[B + "attn.qkv.weight"], P[B + "attn.qkv.bias"],
                 (P[B + "attn.q_norm.weight"], P[B + "attn.q_norm.bias"]), (P[B + "attn.k_norm.weight"], P[B + "attn.k_norm.bias"]),
                 P[B + "attn.proj.weight"], P[B + "attn.proj.bias"], tabs, H, p, si, attn_p, 0.0, v)
    mlp = lambda t, pre, seed: ffn(t, P[pre + "norm2.0.weight"], P[pre + "norm2.0.bias"], P[pre + "mlp.0.fc1.weight"],  # noqa: E731
                                   P[pre + "mlp.0.fc1.bias"], P[pre + "mlp.0.fc2.weight"], P[pre + "mlp.0.fc2.bias"], p, seed, 0.0, v)
    x = mlp(x, B, si if v.mlp_on_seed else mix_seed(si, 2))
    sc = mix_seed(si, 8)
    kv = F.linear(ctx, P[Cb + "attn.kv.weight"], P[Cb + "attn.kv.bias"])
    x = crossattn(x, kv, P[Cb + "norm1.0.weight"], P[Cb + "norm1.0.bias"], P[Cb + "attn.q.weight"], P[Cb + "attn.q.bias"],
                  (P[Cb + "attn.q_norm.weight"], P[Cb + "attn.q_norm.bias"]), (P[Cb + "attn.k_norm.weight"], P[Cb + "attn.k_norm.bias"]),
                  P[Cb + "attn.proj.weight"], P[Cb + "attn.proj.bias"], tiles, H, p, sc, attn_p, v)
    return mlp(x, Cb, sc if v.mlp_on_seed else mix_seed(sc, 2))
