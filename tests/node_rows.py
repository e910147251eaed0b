"""The rows of the sub-block node tests (test infrastructure, not collected): Row(id, node, layout, shape, opts, why) — `why` names
the branch the row enters —, their inputs (CPU, float32, seeded by the row id), their evaluation through the restatements of
tests/node_ref.py in float64 (the reference) and in float32 (the floor), the bars, and `self_check()`, which asserts on the CPU
that every row is what it says.  Layouts come from tests/edge_layouts.py; the integer tables are the oracle front end's
(tests/test_gpu_nodes.py compares them with FrontEnd's before any float is compared).

Bars.  floor(row, quantity) = |float32 restatement - float64 restatement|max relative to max(1, |float64|max), same masks, on the
CPU (one thread); bar = max(coordattn_util.KERNEL_TOL, factor x floor), factor = 4 — the kernels sum in another order than torch's
CPU code, a second float32 rounding of the same size — except for the one quantity `factor()` names, with its reason (never above
16).  BARS records per node and quantity the largest floor, the factor and the largest error measured on the MI355X."""
import collections
import functools
import os
import re
import zlib

import numpy as np
import torch

import edge_layouts as el
import node_ref as nr
from coordattn_util import KERNEL_TOL
from frontend_util import fe

Row = collections.namedtuple("Row", "id node layout shape opts why")

SEED = 0x5EED0000C0FFEE       # the seed every node is given
HAND_P, HAND_SEED = 0.1, 777  # what the previous sub-block armed the outgoing hand-over with
FFN_WS_ROWS, FUSED_LN_ROWS = 8192, 16384  # the row thresholds of FfnFn's routes (csrc/blocks.cpp, csrc/gemm.hip), see self_check
CC = 256                      # context width
P = 0.1

# node -> {quantity: (largest floor over the node's rows and modes, factor, largest error measured on the MI355X)}, from the ledger
# of a full run of tests/test_gpu_nodes.py (177 tests; profiles/r10_nodes_parity.json has the figures per row, mode and quantity).  Quantities are named
# as node_rows.evaluate names them; the chain's 40 parameter gradients are one line, its two k_norm.bias gradients another.  The
# largest share of a bar any quantity used: 0.39 (pool d_bias, mathematically zero under batch statistics); everything that is not
# a mathematically zero gradient stays below 0.2 of its bar.  A record, not a limit: the bars come from floor() and factor().
BARS = {
    "ffn": {"d_b": (3.6e-06, 4, 5.6e-07), "d_b1": (3.9e-07, 4, 5.6e-07), "d_b2": (1.7e-07, 4, 3.0e-07), "d_g": (3.4e-06, 4,
            5.8e-07), "d_w1": (5.9e-07, 4, 7.4e-07), "d_w2": (6.4e-07, 4, 7.2e-07), "d_x": (3.7e-07, 4, 8.0e-07), "dz":
            (3.8e-07, 4, 8.2e-07), "y": (3.7e-07, 4, 6.1e-07)},
    "self": {"d_b": (1.5e-06, 4, 5.8e-07), "d_bp": (1.8e-07, 4, 4.6e-07), "d_bqkv": (2.8e-07, 4, 6.4e-07), "d_g": (1.2e-06, 4,
             9.2e-07), "d_knb": (4.6e-05, 16, 2.8e-05), "d_knw": (2.7e-06, 4, 1.5e-06), "d_qnb": (4.8e-06, 4, 7.0e-07), "d_qnw":
             (3.2e-06, 4, 1.6e-06), "d_wp": (4.9e-07, 4, 9.1e-07), "d_wqkv": (6.8e-07, 4, 9.5e-07), "d_x": (4.4e-07, 4,
             7.9e-07), "y": (3.0e-07, 4, 3.9e-07)},
    "cross": {"d_b": (1.3e-06, 4, 1.2e-06), "d_bkv": (2.4e-07, 4, 7.4e-07), "d_bp": (1.4e-07, 4, 2.8e-07), "d_bq": (6.5e-07, 4,
              9.1e-07), "d_ctx": (5.5e-07, 4, 7.4e-07), "d_g": (8.9e-07, 4, 1.1e-06), "d_knb": (2.0e-05, 16, 2.8e-05), "d_knw":
              (2.1e-06, 4, 1.5e-06), "d_qnb": (2.2e-06, 4, 8.0e-07), "d_qnw": (1.5e-06, 4, 1.3e-06), "d_wkv": (8.4e-07, 4,
              1.1e-06), "d_wp": (6.0e-07, 4, 6.8e-07), "d_wq": (7.1e-07, 4, 8.9e-07), "d_x": (4.0e-07, 4, 6.4e-07), "dz":
              (3.9e-07, 4, 6.3e-07), "y": (3.0e-07, 4, 5.6e-07)},
    "crosskv": {"d_b": (1.6e-06, 4, 1.1e-06), "d_bkv": (2.4e-07, 4, 5.2e-07), "d_bkv0": (0.0e+00, 4, 0.0e+00), "d_bp": (1.4e-07,
                4, 2.6e-07), "d_bq": (7.4e-07, 4, 9.9e-07), "d_ctx": (5.3e-07, 4, 7.9e-07), "d_g": (9.2e-07, 4, 1.1e-06),
                "d_knb": (2.1e-05, 16, 4.5e-05), "d_knw": (1.7e-06, 4, 1.1e-06), "d_qnb": (2.1e-06, 4, 1.4e-06), "d_qnw":
                (2.5e-06, 4, 1.7e-06), "d_wkv": (7.5e-07, 4, 8.5e-07), "d_wkv0": (0.0e+00, 4, 0.0e+00), "d_wp": (4.0e-07, 4,
                5.7e-07), "d_wq": (7.1e-07, 4, 9.8e-07), "d_x": (3.0e-07, 4, 5.5e-07), "dkv": (5.3e-07, 4, 8.7e-07), "dz":
                (3.0e-07, 4, 5.7e-07), "y": (2.9e-07, 4, 5.2e-07)},
    "cpe": {"d_b": (1.6e-06, 4, 3.9e-07), "d_cb": (3.8e-07, 4, 9.5e-07), "d_cw": (4.4e-07, 4, 1.2e-06), "d_g": (1.7e-06, 4,
            7.4e-07), "d_lb": (2.8e-07, 4, 3.3e-07), "d_lw": (4.5e-07, 4, 8.2e-07), "d_x": (4.3e-07, 4, 1.5e-06), "d_xs":
            (4.1e-07, 4, 4.3e-07), "y": (3.9e-07, 4, 7.5e-07)},
    "stem": {"d_b": (3.2e-07, 4, 7.9e-07), "d_cw": (4.7e-07, 4, 7.7e-07), "d_g": (3.1e-07, 4, 9.2e-07), "d_x": (4.2e-07, 4,
             3.5e-06), "rmean": (5.4e-08, 4, 5.4e-08), "rvar": (7.8e-08, 4, 7.8e-08), "y": (6.3e-07, 4, 1.2e-06)},
    "pool": {"d_b": (5.4e-07, 4, 5.4e-07), "d_bias": (5.7e-05, 4, 4.2e-05), "d_g": (5.6e-07, 4, 8.5e-07), "d_w": (5.0e-07, 4,
             4.3e-07), "d_x": (9.1e-07, 4, 8.1e-07), "rmean": (5.6e-08, 4, 5.6e-08), "rvar": (8.7e-08, 4, 8.7e-08), "y":
             (7.8e-07, 4, 7.7e-07)},
    "unpool": {"d_betas": (2.6e-07, 4, 1.6e-07), "d_betau": (2.5e-07, 4, 1.8e-07), "d_bs": (9.8e-05, 4, 4.6e-05), "d_bu":
               (5.8e-05, 4, 3.4e-05), "d_gs": (4.6e-07, 4, 3.5e-07), "d_gu": (3.3e-07, 4, 3.0e-07), "d_ws": (5.1e-07, 4,
               3.7e-07), "d_wu": (4.7e-07, 4, 4.6e-07), "d_xc": (5.8e-07, 4, 6.0e-07), "d_xp": (5.3e-07, 4, 5.3e-07), "rms":
               (4.8e-08, 4, 4.8e-08), "rmu": (4.8e-08, 4, 4.8e-08), "rvs": (8.1e-08, 4, 8.1e-08), "rvu": (8.3e-08, 4, 7.4e-08),
               "skip": (5.5e-07, 4, 6.0e-07), "y": (4.9e-07, 4, 4.3e-07)},
    "chain": {"d_ctx": (5.1e-07, 4, 7.4e-07), "d_k_norm.bias": (6.9e-06, 16, 1.4e-05), "d_params": (1.3e-06, 4, 1.3e-06), "d_x":
              (3.4e-07, 4, 4.1e-07), "y": (2.8e-07, 4, 4.2e-07)},
}
# Factors above 4, by quantity.  d k_norm.bias is mathematically ZERO (a constant added to every normalised key shifts all scores
# of a query by the same amount, which the softmax does not see): what any float32 evaluation returns is the cancellation noise
# of a sum over every (query, key, head), and the floor itself is one draw of it (4.9e-6 .. 7.4e-6 for one row, by the number of
# CPU threads alone).  Measured on the MI355X: up to 3.8 x the floor (2.8e-5 at cross_short_64_2), i.e. over 4 x the smaller
# draws -> 16, the most a factor may be.  (The per-kernel tests give this gradient 5e-4 for the same reason.)
ZERO_GRAD_FACTOR = 16


def factor(row, q):
    return ZERO_GRAD_FACTOR if row.node in ("self", "cross", "crosskv", "chain") and (q == "d_knb" or q.endswith("k_norm.bias")) else 4


def _ffn(M, C, why, **o):
    o = dict(dict(p=P, dpath=0.0), **o)
    tag = "".join(f"_{k}{v}" for k, v in sorted(o.items()) if (k, v) not in (("p", P), ("dpath", 0.0)))
    return Row(f"ffn_{M}x{C}{tag}", "ffn", None, (M, C), o, why)


def _self(kind, name, C, H, why, **o):
    o = dict(dict(p=P, attn_p=P, dpath=0.0, qk=True), **o)
    tag = "".join(f"_{k}{v}" for k, v in sorted(o.items()) if (k, v) not in (("p", P), ("attn_p", P), ("dpath", 0.0), ("qk", True)))
    return Row(f"self_{name or kind}_{C}_{H}{tag}", "self", (kind, name, 1), (C, H), o, why)


ROWS = [
    # ---- FfnFn (M, C), Hd = 4 C
    _ffn(1, 64, "one row: every tile ragged, a LayerNorm of one row"),
    _ffn(63, 96, "C = 96: no multiple of 64, one short row tile"),
    _ffn(65, 128, "one row past a 64-row tile"),
    _ffn(300, 768, "the widest level: Hd = 3072, split-K products"),
    _ffn(FFN_WS_ROWS, 64, "the last row count that is offered the main workspace"),
    _ffn(FFN_WS_ROWS + 1, 64, "the first row count without the main workspace"),
    _ffn(FUSED_LN_ROWS - 1, 64, "the last row count whose LayerNorm backward is a launch of its own"),
    _ffn(FUSED_LN_ROWS, 64, "LayerNorm backward as the epilogue of the fc1 input gradient (composite), C = 64"),
    _ffn(FUSED_LN_ROWS, 128, "LayerNorm backward as the epilogue of the fc1 input gradient (composite), C = 128: the widest it takes"),
    _ffn(65, 128, "dropout off: every mask is the identity, no mask launch in backward", p=0.0),
    _ffn(63, 96, "DropPath 0.3 on the branch: per launch, no incoming hand-over", dpath=0.3),
    # ---- SelfAttnFn
    _self("patch", "", 64, 2, "patches of 1 .. 128 rows, 127 and 1 borrowed rows; head width 32"),
    _self("patch", "", 96, 4, "head width 24"),
    _self("patch", "", 128, 4, "head width 32, four heads"),
    _self("conv", "n1", 64, 2, "one point: a softmax over one key"),
    _self("conv", "many_tiny", 64, 2, "100 clouds of 3: 100 tiles of 3 rows"),
    _self("ctx", "short", 768, 32, "the widest level: 32 heads of 24"),
    _self("patch", "", 64, 2, "no q/k norm: per launch, the kernels without the norm", qk=False),
    _self("patch", "", 64, 2, "all dropout off", p=0.0, attn_p=0.0),
    _self("patch", "", 64, 2, "DropPath 0.3 on the branch: per launch", dpath=0.3),
]
for _node in ("cross", "crosskv"):
    for _layout in ("short", "long", "full"):
        for _C, _H in ((64, 2), (256, 8)):
            ROWS.append(Row(f"{_node}_{_layout}_{_C}_{_H}", _node, ("ctx", _layout, 1), (_C, _H), dict(p=P, attn_p=P),
                            {"short": "contexts of 1 .. 32 tokens: the short-key kernels", "long": "contexts of 1 .. 78 tokens: the tile kernels",
                             "full": "128 tokens, the most a key image holds, and a single token"}[_layout]
                            + ("; own kv projection, d context" if _node == "cross" else "; kv a slice of a ProjAllFn bank, d kv into its gradient slice")))
for _scene in ("dups", "line", "solid", "n1", "many_tiny"):
    for _C in (64, 128):
        ROWS.append(Row(f"cpe_{_scene}_{_C}", "cpe", ("conv", _scene, 2 if _scene == "dups" else 1), (_C,), dict(same=True),
                        f"composite; scene {_scene}" + (": duplicate voxels, the fold / mask passes" if _scene == "dups" else "")))
ROWS += [
    Row("cpe_dups_96", "cpe", ("conv", "dups", 2), (96,), dict(same=True), "C = 96: the eligibility rule sends it per launch"),
    Row("cpe_dups_64_skip", "cpe", ("conv", "dups", 2), (64,), dict(same=False), "xs a second tensor (the decoder's stale skip branch), duplicates"),
    Row("cpe_solid_128_skip", "cpe", ("conv", "solid", 1), (128,), dict(same=False), "xs a second tensor, every tap full"),
    Row("cpe_many_tiny_96_skip", "cpe", ("conv", "many_tiny", 1), (96,), dict(same=False), "xs a second tensor, per launch"),
]
for _scene in ("solid", "dups", "many_tiny"):
    for _xg in (False, True):
        for _tr in (True, False):
            ROWS.append(Row(f"stem_{_scene}_{'xgrad' if _xg else 'nox'}_{'train' if _tr else 'eval'}", "stem",
                            ("conv", _scene, 2 if _scene == "dups" else 1), (7, 64), dict(xgrad=_xg, training=_tr),
                            ("planner: conv_dgrad runs, the weight gradient goes to the side stream" if _xg
                             else "policy: no input gradient, the weight gradient on the main stream") + ("" if _tr else "; running statistics")))
for _scene in el.POOL_SCENES:
    for _ci, _co in ((64, 128), (128, 64)):
        for _tr in (True, False):
            ROWS.append(Row(f"pool_{_scene}_{_ci}_{_co}_{'train' if _tr else 'eval'}", "pool", ("pool", _scene, 2), (_ci, _co),
                            dict(training=_tr), f"cells of scene {_scene}"))
            ROWS.append(Row(f"unpool_{_scene}_{_ci}_{_co}_{'train' if _tr else 'eval'}", "unpool", ("pool", _scene, 2), (_ci, _co),
                            dict(training=_tr), f"coarse width {_ci}, skip and output width {_co}; scene {_scene}"))
ROWS.append(Row("chain_long_64_2", "chain", ("ctx", "long", 1), (64, 2), dict(p=P, attn_p=P),
                "Block.run then CABlock.run on module instances: hand-overs and seed wiring of the product; PairFn when the pair is on"))
ROW = {r.id: r for r in ROWS}
NODES = ("ffn", "self", "cross", "crosskv", "cpe", "stem", "pool", "unpool", "chain")
END_JOIN_ROWS = ("ffn_65x128", "self_patch_96_4", "cross_long_64_2", "crosskv_long_256_8", "cpe_dups_64_skip", "stem_dups_xgrad_train",
                 "pool_all_eight_64_128_train", "unpool_100_clouds_of_3_128_64_train", "chain_long_64_2")


# ------------------------------------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def tables(layout):
    """(kind, name, n_levels) -> dict(pc, counts, txt, levels): the scene and the oracle front end's integer tables."""
    kind, name, n_levels = layout
    pc, counts, txt = {"patch": lambda: el.patch_edges(), "ctx": lambda: el.ctx_edges(name), "conv": lambda: el.conv_scenes(name),
                       "pool": lambda: el.pool_scenes(name)}[kind]()
    levels = fe.build_all_levels(pc[:, :3].numpy(), counts, n_levels, perms=[[0, 1, 2, 3]] * n_levels)
    return dict(pc=pc, counts=counts, txt=txt, levels=levels)


def _long(a):
    return torch.from_numpy(np.ascontiguousarray(a)).long()


# ------------------------------------------------------------------------------------------------ inputs
def _w(g, o, i):
    return torch.randn(o, i, generator=g) / i ** 0.5


def _v(g, n, base=0.0):
    return base + 0.1 * torch.randn(n, generator=g)


def _qk(g, d):
    return [torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2, torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2]


def _bn(g, C):
    """gamma, beta, running mean, running var (positive)."""
    return [_v(g, C, 1.0), _v(g, C), 0.3 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5]


CHAIN_SHAPES = lambda C, Hd, d: {  # noqa: E731  (state-dict names of ptv3.Block / ptv3.CABlock under "blk." / "cab.")
    "blk.cpe.0.weight": (C, 3, 3, 3, C), "blk.cpe.0.bias": (C,), "blk.cpe.1.weight": (C, C), "blk.cpe.1.bias": (C,),
    "blk.cpe.2.weight": (C,), "blk.cpe.2.bias": (C,), "blk.norm1.0.weight": (C,), "blk.norm1.0.bias": (C,),
    "blk.attn.qkv.weight": (3 * C, C), "blk.attn.qkv.bias": (3 * C,), "blk.attn.proj.weight": (C, C), "blk.attn.proj.bias": (C,),
    "blk.attn.q_norm.weight": (d,), "blk.attn.q_norm.bias": (d,), "blk.attn.k_norm.weight": (d,), "blk.attn.k_norm.bias": (d,),
    "blk.norm2.0.weight": (C,), "blk.norm2.0.bias": (C,), "blk.mlp.0.fc1.weight": (Hd, C), "blk.mlp.0.fc1.bias": (Hd,),
    "blk.mlp.0.fc2.weight": (C, Hd), "blk.mlp.0.fc2.bias": (C,),
    "cab.norm1.0.weight": (C,), "cab.norm1.0.bias": (C,), "cab.attn.q.weight": (C, C), "cab.attn.q.bias": (C,),
    "cab.attn.kv.weight": (2 * C, CC), "cab.attn.kv.bias": (2 * C,), "cab.attn.proj.weight": (C, C), "cab.attn.proj.bias": (C,),
    "cab.attn.q_norm.weight": (d,), "cab.attn.q_norm.bias": (d,), "cab.attn.k_norm.weight": (d,), "cab.attn.k_norm.bias": (d,),
    "cab.norm2.0.weight": (C,), "cab.norm2.0.bias": (C,), "cab.mlp.0.fc1.weight": (Hd, C), "cab.mlp.0.fc1.bias": (Hd,),
    "cab.mlp.0.fc2.weight": (C, Hd), "cab.mlp.0.fc2.bias": (C,)}

POOL_MARGIN = 1e-4  # x max |proj|: the least gap between the best and the second-best member of a (cell, column)


def pool_gaps(proj, cluster, n_child):
    """float64 proj [n][C], cluster [n] -> (gap [n_child][C] between the largest and the second-largest member, inf for cells of
    one point; row [n_child][C] of the second-largest member)."""
    n, C = proj.shape
    idx = cluster.view(-1, 1).expand(-1, C)
    best = proj.new_full((n_child, C), -np.inf).scatter_reduce(0, idx, proj, "amax")
    is_best = proj == best[cluster]
    rest = torch.where(is_best, torch.full_like(proj, -np.inf), proj)
    second = proj.new_full((n_child, C), -np.inf).scatter_reduce(0, idx, rest, "amax")
    rows = torch.arange(n).view(-1, 1).expand(-1, C)
    cand = torch.where((rest == second[cluster]) & ~is_best, rows, torch.full_like(rows, n))
    arg2 = torch.full((n_child, C), n, dtype=torch.long).scatter_reduce(0, idx, cand, "amin")
    ties = torch.zeros(n_child, C).scatter_reduce(0, idx, is_best.float(), "sum") > 1
    gap = torch.where(ties, torch.zeros_like(best), best - second)
    return gap, arg2


def _pool_x(x, w, bias, cluster, n_child):
    """Move the few rows whose projection is a near-tie for a (cell, column) maximum away from it (the smallest change of the
    row along that column's weight vector), until every gap is above twice POOL_MARGIN: a float32 rounding then cannot move an
    arg-max and no (cell, column) has to be excluded from the comparison."""
    x = x.double().clone()
    wd, bd = w.double(), bias.double()
    for _ in range(50):
        proj = x @ wd.t() + bd
        gap, arg2 = pool_gaps(proj, cluster, n_child)
        want = 2 * POOL_MARGIN * float(proj.abs().max())
        bad = torch.nonzero(gap < want)
        if not len(bad):
            return x.float()
        for cell, col in bad.tolist()[:1 + len(bad) // 4]:
            r = int(arg2[cell, col])
            if r < x.shape[0]:
                x[r] -= (4 * want) * wd[col] / float(wd[col] @ wd[col])
    raise AssertionError("the pooling rows keep near-ties")


@functools.lru_cache(maxsize=None)
def inputs(rid):
    """Row id -> dict of float32 CPU tensors: the node's tensor inputs by name, and `up_<output>` = the gradient it is given."""
    row = ROW[rid]
    g = torch.Generator().manual_seed(zlib.crc32(rid.encode()))
    node = row.node
    R = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if node == "ffn":
        M, C = row.shape
        return dict(x=R(M, C), g=_v(g, C, 1.0), b=_v(g, C), w1=_w(g, 4 * C, C), b1=_v(g, 4 * C), w2=_w(g, C, 4 * C), b2=_v(g, C), up_y=R(M, C))
    T = tables(row.layout)
    n = len(T["pc"])
    if node == "self":
        C, H = row.shape
        qk = dict(zip(("qnw", "qnb", "knw", "knb"), _qk(g, C // H)))
        I = dict(x=R(n, C), g=_v(g, C, 1.0), b=_v(g, C), wqkv=_w(g, 3 * C, C), bqkv=_v(g, 3 * C), **qk, wp=_w(g, C, C), bp=_v(g, C), up_y=R(n, C))
        if not row.opts["qk"]:
            for k in qk:
                del I[k]
        return I
    if node in ("cross", "crosskv"):
        C, H = row.shape
        L = sum(T["txt"])
        I = dict(x=R(n, C), ctx=R(L, CC), g=_v(g, C, 1.0), b=_v(g, C), wq=_w(g, C, C), bq=_v(g, C), wkv=_w(g, 2 * C, CC), bkv=_v(g, 2 * C),
                 **dict(zip(("qnw", "qnb", "knw", "knb"), _qk(g, C // H))), wp=_w(g, C, C), bp=_v(g, C), up_y=R(n, C))
        if node == "crosskv":  # a first consumer of the bank, so that the slice under test starts at column 96
            I.update(wkv0=_w(g, 96, CC), bkv0=_v(g, 96))
        return I
    if node == "cpe":
        (C,) = row.shape
        I = dict(x=R(n, C), cw=R(C, 3, 3, 3, C) / (C * 9) ** 0.5, cb=_v(g, C), lw=_w(g, C, C), lb=_v(g, C), g=_v(g, C, 1.0), b=_v(g, C), up_y=R(n, C))
        if not row.opts["same"]:
            I["xs"] = R(n, C)
        return I
    if node == "stem":
        cin, C = row.shape
        return dict(x=R(n, cin), cw=R(C, 5, 5, 5, cin) / (cin * 9) ** 0.5, **dict(zip(("g", "b", "rmean", "rvar"), _bn(g, C))), up_y=R(n, C))
    if node == "pool":
        ci, co = row.shape
        lv = T["levels"][1]
        nc = lv["grid"].shape[0]
        w, bias = _w(g, co, ci), _v(g, co)
        x = _pool_x(R(n, ci), w, bias, _long(lv["cluster"]), nc)
        return dict(x=x, w=w, bias=bias, **dict(zip(("g", "b", "rmean", "rvar"), _bn(g, co))), up_y=R(nc, co))
    if node == "unpool":
        ci, co = row.shape
        nc = T["levels"][1]["grid"].shape[0]
        return dict(xc=R(nc, ci), xp=R(n, co), wu=_w(g, co, ci), bu=_v(g, co), **dict(zip(("gu", "betau", "rmu", "rvu"), _bn(g, co))),
                    ws=_w(g, co, co), bs=_v(g, co), **dict(zip(("gs", "betas", "rms", "rvs"), _bn(g, co))), up_y=R(n, co), up_skip=R(n, co))
    if node == "chain":
        C, H = row.shape
        I = dict(x=R(n, C), ctx=R(sum(T["txt"]), CC), up_y=R(n, C))
        for name, s in CHAIN_SHAPES(C, 4 * C, C // H).items():
            if name.endswith("_norm.weight"):
                I[name] = torch.rand(*s, generator=g) + 0.5
            elif len(s) == 1:
                I[name] = _v(g, s[0], 1.0 if "norm" in name and name.endswith("weight") or name.endswith("cpe.2.weight") else 0.0)
            else:
                I[name] = R(*s) / (int(np.prod(s[1:])) / (3 if len(s) == 5 else 1)) ** 0.5
        return I
    raise KeyError(node)


NO_GRAD = ("rmean", "rvar", "rmu", "rvu", "rms", "rvs")


def grad_names(row):
    """The inputs whose gradients are compared (every float input except the running statistics; the stem's x by option)."""
    return [k for k in inputs(row.id) if not k.startswith("up_") and k not in NO_GRAD and not (row.node == "stem" and k == "x" and not row.opts["xgrad"])]


# ------------------------------------------------------------------------------------------------ evaluation
def _eval(row, T, v):
    """-> (outputs {name: tensor} in the order of the `up_` gradients, extras {name: tensor without gradient}, retained {name: tensor})."""
    node, o = row.node, row.opts
    if node == "ffn":
        return dict(y=nr.ffn(T["x"], T["g"], T["b"], T["w1"], T["b1"], T["w2"], T["b2"], o["p"], SEED, o["dpath"], v)), {}, {}
    tb = tables(row.layout)
    lv0 = tb["levels"][0]
    if node == "self":
        C, H = row.shape
        qn, kn = ((T["qnw"], T["qnb"]), (T["knw"], T["knb"])) if o["qk"] else (None, None)
        y = nr.selfattn(T["x"], T["g"], T["b"], T["wqkv"], T["bqkv"], qn, kn, T["wp"], T["bp"], nr.self_tables(lv0), H, o["p"], SEED,
                        o["attn_p"], o["dpath"], v)
        return dict(y=y), {}, {}
    if node in ("cross", "crosskv"):
        C, H = row.shape
        kv = torch.nn.functional.linear(T["ctx"], T["wkv"], T["bkv"])
        y = nr.crossattn(T["x"], kv, T["g"], T["b"], T["wq"], T["bq"], (T["qnw"], T["qnb"]), (T["knw"], T["knb"]), T["wp"], T["bp"],
                         nr.cross_tiles(tb["counts"], tb["txt"]), H, o["p"], SEED, o["attn_p"], v)
        return dict(y=y), {}, (dict(kv=kv) if node == "crosskv" else {})
    if node == "cpe":
        return dict(y=nr.cpe(T["x"], T["x"] if o["same"] else T["xs"], T["cw"], T["cb"], T["lw"], T["lb"], T["g"], T["b"], _long(lv0["nbr27"]))), {}, {}
    if node == "stem":
        y, rm, rv = nr.stem(T["x"], T["cw"], T["g"], T["b"], T["rmean"], T["rvar"], _long(lv0["nbr125"]), o["training"])
        return dict(y=y), dict(rmean=rm, rvar=rv), {}
    lv1 = tb["levels"][1] if len(tb["levels"]) > 1 else None
    if node == "pool":
        y, rm, rv, _ = nr.pool(T["x"], T["w"], T["bias"], T["g"], T["b"], T["rmean"], T["rvar"], _long(lv1["cluster"]), lv1["grid"].shape[0], o["training"])
        return dict(y=y), dict(rmean=rm, rvar=rv), {}
    if node == "unpool":
        y, skip, st = nr.unpool(T["xc"], T["xp"], T["wu"], T["bu"], T["gu"], T["betau"], T["rmu"], T["rvu"], T["ws"], T["bs"], T["gs"], T["betas"],
                                T["rms"], T["rvs"], _long(lv1["cluster"]), o["training"])
        return dict(y=y, skip=skip), dict(zip(("rmu", "rvu", "rms", "rvs"), st)), {}
    if node == "chain":
        C, H = row.shape
        y = nr.chain(T["x"], T, T["ctx"], nr.self_tables(lv0), nr.cross_tiles(tb["counts"], tb["txt"]), _long(lv0["nbr27"]), H, o["p"], o["attn_p"], SEED, v)
        return dict(y=y), {}, {}
    raise KeyError(node)


def evaluate(row, dtype=torch.float64, v=nr.EXACT):
    """The row through its restatement in `dtype` -> {quantity: tensor}: the outputs by name, `d_<input>` for every compared
    gradient, the new running statistics of a BatchNorm row, `dkv` (the gradient of the bank slice) and `dz` (the parked
    hand-over: d x times the mask the previous sub-block armed) where the node has them."""
    I = inputs(row.id)
    need = set(grad_names(row))
    T = {k: t.detach().clone().to(dtype).requires_grad_(k in need) for k, t in I.items() if not k.startswith("up_")}
    outs, extras, kept = _eval(row, T, v)
    for t in kept.values():
        t.retain_grad()
    torch.autograd.backward(list(outs.values()), [I["up_" + k].to(dtype) for k in outs])
    res = {k: t.detach() for k, t in outs.items()}
    # (an input nothing reads — the bank's other consumer — has the gradient zero)
    res.update({"d_" + k: (T[k].grad if T[k].grad is not None else torch.zeros_like(T[k])) for k in I if k in need})
    res.update({k: t.detach() for k, t in extras.items()})
    res.update({"d" + k: t.grad for k, t in kept.items()})
    if row.node in ("ffn", "cross", "crosskv"):
        M, C = T["x"].shape
        res["dz"] = res["d_x"] * torch.from_numpy(nr.dense_scale(HAND_SEED, M, C, HAND_P, v)).to(dtype)
    return res


@functools.lru_cache(maxsize=None)
def reference(rid):
    return evaluate(ROW[rid])


def rel_err(got, ref):
    """|got - ref|max relative to max(1, |ref|max), in float64."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@functools.lru_cache(maxsize=None)
def floor(rid):
    """{quantity: error of the float32 restatement (CPU, same masks) against the float64 one}."""
    ref = reference(rid)
    threads = torch.get_num_threads()
    try:  # (one thread: the float32 sums, hence the floor, do not depend on how many CPUs the machine has)
        torch.set_num_threads(1)
        f32 = evaluate(ROW[rid], torch.float32)
    finally:
        torch.set_num_threads(threads)
    return {k: rel_err(f32[k], ref[k]) for k in ref}


def bars(rid):
    row = ROW[rid]
    return {q: max(KERNEL_TOL, factor(row, q) * f) for q, f in floor(rid).items()}


# ------------------------------------------------------------------------------------------------ faults
FAULTS = {"swap": nr.Variant(swap=True), "pre_gelu": nr.Variant(pre_gelu=True), "plain_scale": nr.Variant(plain_scale=True),
          "mlp_on_seed": nr.Variant(mlp_on_seed=True)}


def faults_of(row):
    """The deliberate faults that can show on the row: none without dropout, (b) where there is an fc1, (d) on the chain."""
    o = row.opts
    if not (o.get("p", 0.0) > 0.0 or o.get("attn_p", 0.0) > 0.0):
        return []
    return {"ffn": ["swap", "pre_gelu", "plain_scale"], "self": ["swap", "plain_scale"], "cross": ["swap", "plain_scale"],
            "crosskv": ["swap", "plain_scale"], "chain": ["swap", "pre_gelu", "plain_scale", "mlp_on_seed"]}[row.node]


def fault_power(rid, fault):
    """max over the quantities of (movement under the fault) / (the quantity's bar)."""
    ref, b = reference(rid), bars(rid)
    bad = evaluate(ROW[rid], torch.float64, FAULTS[fault])
    return max(rel_err(bad[k], ref[k]) / b[k] for k in ref)


# ------------------------------------------------------------------------------------------------ self check
def _src(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "robot-3dlotus_amd", "csrc", name)) as f:
        return f.read()


def self_check():
    """Every row is what it says (CPU).  -> number of rows."""
    assert len(ROW) == len(ROWS) and {r.node for r in ROWS} == set(NODES) and set(END_JOIN_ROWS) <= set(ROW)
    assert sorted(ROW[r].node for r in END_JOIN_ROWS) == sorted(NODES), "one row per node under the deferred join"
    # the thresholds the FfnFn rows straddle are the ones the sources state today
    assert int(re.search(r"rows > (\d+) \? Ws\{nullptr", _src("blocks.cpp")).group(1)) == FFN_WS_ROWS
    assert int(re.search(r'"LOTUS_GEMM_DMA_MINROWS", (\d+)', _src("gemm.hip")).group(1)) == FUSED_LN_ROWS
    shapes = {r.shape for r in ROWS if r.node == "ffn"}
    assert {(1, 64), (63, 96), (65, 128), (300, 768), (FFN_WS_ROWS, 64), (FFN_WS_ROWS + 1, 64), (FUSED_LN_ROWS - 1, 64), (FUSED_LN_ROWS, 64),
            (FUSED_LN_ROWS, 128)} == shapes
    assert any(r.node == "ffn" and r.opts["p"] == 0.0 for r in ROWS) and any(r.node == "ffn" and r.opts["dpath"] == 0.3 for r in ROWS)
    # masks: kept fraction wherever there are at least 4096 elements; streams differ
    for M, N, seed in ((64, 64, SEED), (300, 3072, nr.mix_seed(SEED, 1)), (FUSED_LN_ROWS, 128, nr.mix_seed(SEED, 2)), (756, 64, HAND_SEED)):
        s = nr.dense_scale(seed, M, N, P)
        assert abs((s != 0).mean() - (1 - P)) < 0.02, (M, N, (s != 0).mean())
        assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1.0 / (1.0 - int(float(np.float32(P)) * 65536) / 65536.0)))}
    assert (nr.dense_scale(SEED, 64, 64, P) != nr.dense_scale(nr.mix_seed(SEED, 1), 64, 64, P)).mean() > 0.1
    dp = nr.droppath_scale(nr.mix_seed(SEED, 5), FFN_WS_ROWS, 0.3)
    assert abs((dp != 0).mean() - 0.7) < 0.02
    k0, k1 = nr.attn_keep(0, 2, 128, 128, SEED, P), nr.attn_keep(1, 2, 128, 128, SEED, P)
    assert abs(k0.mean() - (1 - P)) < 0.02 and abs(k1.mean() - (1 - P)) < 0.02 and (k0 != k1).mean() > 0.1 and (k0[0] != k0[1]).mean() > 0.1
    # the dropout rows of the 63-row DropPath case drop some rows and keep some
    d63 = nr.droppath_scale(nr.mix_seed(SEED, 5), 63, 0.3)
    assert 0 < (d63 == 0).sum() < 63
    # layouts
    t = tables(("patch", "", 1))
    st = nr.self_tables(t["levels"][0])
    assert len(t["pc"]) == 1828 and set(st["tiles"][:, 1].tolist()) == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128}
    assert nr.self_tables(tables(("conv", "n1", 1))["levels"][0])["tiles"].tolist() == [[0, 1, 0, 1]]
    assert nr.self_tables(tables(("conv", "many_tiny", 1))["levels"][0])["tiles"][:, 1].tolist() == [3] * 100
    for layout, kmax in (("short", 32), ("long", 78), ("full", 128)):
        c = tables(("ctx", layout, 1))
        ct = nr.cross_tiles(c["counts"], c["txt"])
        assert ct[:, 3].max() == kmax and ct[:, 3].min() == 1 and ct[:, 1].max() == 128 and ct[:, 1].sum() == len(c["pc"])
    assert (tables(("conv", "dups", 2))["levels"][0]["nbr27"][:, 13] != np.arange(1900)).sum() == 172, "the duplicates of the dups scene"
    for r in ROWS:
        if r.node in ("stem", "pool", "unpool"):  # at least two rows per BatchNorm statistic
            tb = tables(r.layout)
            assert len(tb["pc"]) >= 2 and (r.node == "stem" or tb["levels"][1]["grid"].shape[0] >= 2), r.id
        if r.node == "pool":  # no (cell, column) whose arg-max a float32 rounding could move: nothing is excluded
            I, lv = inputs(r.id), tables(r.layout)["levels"][1]
            proj = I["x"].double() @ I["w"].double().t() + I["bias"].double()
            gap, _ = pool_gaps(proj, _long(lv["cluster"]), lv["grid"].shape[0])
            excluded = float((gap <= POOL_MARGIN * float(proj.abs().max())).float().mean())
            assert excluded == 0.0, (r.id, excluded)
    return len(ROWS)
