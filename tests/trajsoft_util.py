"""Shared helpers of the soft trajectory head's tests (test infrastructure, not collected): the float64 restatement of the head
(motion_planner_ptv3.py:89-109, pos_pred_type 'heatmap_mlp') and of the masked losses (:338-397) in plain torch, with autograd
for the gradients; the case table of tests/test_gpu_trajsoft.py; the runners of one row through the raw C-ABI (fused:
lotus_mp_softpos_fwd / _bwd into guarded caller-owned buffers, twice) and through the composition of the entry points that were
there before it (lotus_step_act_fwd -> lotus_softpos_fwd per step, then lotus_softpos_bwd -> linear_dgrad / linear_wgrad ->
lotus_step_act_bwd).  The dropout mask is the uint32 numpy restatement of tests/head_run.py.  No reference import here.

One row per shape: `Row(id, counts, C, T, ld, temp, p, opts, why)`; `why` names the branch the row is there to enter.  The
geometry the rows are built around (csrc/reg_head.hip): 32 row chunks per cloud and 16 lanes per row in the forward pass, 64 rows
per block in the backward pass, whose per-block column partials lotus_reduce_parts sums 16 at a time."""
import collections

import numpy as np
import torch

SLOPE = float(np.float32(0.02))
SP_SPLITS, SP_LPR, MPB_ROWS, MP_TMAX = 32, 16, 64, 8
KERNEL_TOL = 2e-5   # x max(1, |ref|max): the per-kernel bar (tests/test_gpu_reghead.py)
LOSS_TOL = 1e-4
SEED = 0x5EED0BADC0FFEE11

Row = collections.namedtuple("Row", "id counts C T ld temp p opts why")

ROWS = [
    Row("one-point-c4-t1", (1,), 4, 1, 3, 1.0, 0.0, {},
        "one row, one quad, one step: 31 empty chunks, 15 idle lanes, p_i = 1: xt = coord + e[1:4] and de_0 = 0 exactly"),
    Row("one-point-c64-t5", (1,), 64, 5, 6, 0.1, 0.1, {}, "the same cloud at the YAML's width, steps and temperature, dropout on"),
    Row("sizes-c64-t5", (1, 2, 31, 33, 257), 64, 5, 6, 0.1, 0.1, {"zero_steps": 1},
        "B = 5, mixed sizes: chunks empty below 32 rows, 5 backward blocks over 324 rows that straddle clouds; a zero step, a zero cloud"),
    Row("ragged-c132-t8", (4099,), 132, 8, 7, 0.1, 0.1, {},
        "33 quads: the 16-lane loop runs ragged (3 trips, 1 lane in the last); T = 8 fills every accumulator; 65 blocks, ld 7"),
    Row("hot-c64-t5", (300, 40), 64, 5, 3, 0.1, 0.0, {"hot": 100.0},
        "|e0| up to 100 at temp 0.1: exponents ~1e3 stay finite with the maximum subtracted; one row dominates its cloud"),
    Row("rows63-c64-t5", (63,), 64, 5, 3, 1.0, 0.1, {}, "one row below the backward block: 1 block, its last row group short"),
    Row("rows64-c64-t5", (64,), 64, 5, 3, 1.0, 0.1, {}, "exactly one backward block: 1 partial"),
    Row("rows65-c64-t5", (65,), 64, 5, 3, 1.0, 0.1, {}, "one row above: 2 partials, the second block holds one row"),
    Row("big-c64-t5", (70001,), 64, 5, 3, 1.0, 0.0, {},
        "1094 backward blocks: more than 256 partials, 69 per reduction lane; 2188 rows per forward chunk"),
    Row("wide-c2048-t8", (40,), 2048, 8, 3, 1.0, 0.0, {},
        "the widest admitted C with T = 8: 96 KiB of W3 and bias rows in LDS, 32 quads per lane"),
    Row("t1-c64-zero-g", (33, 31), 64, 1, 3, 0.1, 0.0, {"zero_steps": 1}, "T = 1 with B = 2: the zero cloud's rows get exact zeros"),
]
ROW_IDS = [r.id for r in ROWS]


def self_check():
    """The rows enter the branches they name (a retuned geometry makes this fail: move the row)."""
    by = {r.id: r for r in ROWS}
    assert {r.C for r in ROWS} >= {4, 64, 132} and {r.T for r in ROWS} >= {1, 5, 8} and {r.ld for r in ROWS} >= {3, 6, 7}
    assert {n for r in ROWS for n in r.counts} >= {1, 2, 31, 33, 257, 4099}
    assert (by["ragged-c132-t8"].C // 4) % SP_LPR != 0 and by["ragged-c132-t8"].T == MP_TMAX
    assert [sum(by[f"rows{n}-c64-t5"].counts) for n in (63, 64, 65)] == [MPB_ROWS - 1, MPB_ROWS, MPB_ROWS + 1]
    assert -(-sum(by["big-c64-t5"].counts) // MPB_ROWS) > 256
    assert (4 + by["wide-c2048-t8"].T) * by["wide-c2048-t8"].C * 4 > 65536
    assert any(r.p > 0 for r in ROWS) and any(r.p == 0 for r in ROWS) and any(len(r.counts) == 1 for r in ROWS)
    assert all(min(r.counts) < SP_SPLITS for r in ROWS if r.id.startswith(("one-point", "sizes")))


def mix_seed(seed, k):
    from robot_3dlotus_amd import ops

    return ops.mix_seed(seed, k)


def drop_scales(row, n):
    """[T, n, C] float32 keep scales: step t's mask is lotus_step_act_fwd's with seed mix_seed(SEED, t), index row * C + column."""
    import head_run as hr

    if row.p == 0:
        return torch.ones(row.T, n, row.C)
    idx = np.arange(n * row.C, dtype=np.uint64)
    return torch.stack([torch.from_numpy(hr.keep_scale(mix_seed(SEED, t), idx, row.p)).view(n, row.C) for t in range(row.T)])


# ================================================================================================= float64 restatement
def head_ref(base, bias, w3, b3, coord, counts, temp, scales, e_hook=None, slope=SLOPE):
    """ActionHead.forward, heatmap_mlp branch (motion_planner_ptv3.py:89-109), from the shared product `base` = x Wx^T and the
    step rows `bias` = te Wt^T + b: -> (e [T, n, 4], xt [B, T, 3]).  scales [T, n, C]: the dropout keep scales.  Differentiable.
    e_hook (optional) maps e before the softmax stage (see reference()); slope: the fp32 constant the kernels and torch's fp32
    LeakyReLU carry, float32(0.02), unless the caller compares against a float64 module (0.02)."""
    pre = base.unsqueeze(0) + bias.unsqueeze(1)                                  # [T, n, C]
    h = torch.where(pre > 0, pre, pre * slope) * scales
    e = h @ w3.t() + b3                                                          # [T, n, 4]
    if e_hook is not None:
        e = e_hook(e)
    xt, o = [], 0
    for nn in counts:
        w = torch.softmax(e[:, o:o + nn, 0] / temp, dim=1)                       # [T, nn]
        q = coord[o:o + nn].unsqueeze(0) + e[:, o:o + nn, 1:]                    # [T, nn, 3]
        xt.append(torch.einsum("tp,tpc->tc", w, q))
        o += nn
    return e, torch.stack(xt, 0)


def loss_ref(ae, xt, gt, stop, mask, nrot, pos_w, rot_w):
    """compute_loss (motion_planner_ptv3.py:338-397; heatmap_mlp, euler_disc): ae [B, T, nrot*3 + 2], xt [B, T, 3], gt [B, T, ga],
    stop / mask [B, T] -> losses [5] = pos, rot, open, stop, total.  Differentiable."""
    import torch.nn.functional as F

    B, T = mask.shape
    msum = mask.sum()
    pos = (((xt - gt[..., :3]) ** 2) * mask.unsqueeze(-1)).sum() / msum / 3
    rl = F.cross_entropy(ae[..., :nrot * 3].reshape(B, T, nrot, 3).permute(0, 1, 3, 2).reshape(-1, nrot),
                         gt[..., 3:6].long().reshape(-1), reduction="none").view(B, T, 3)
    rot = (rl * mask.unsqueeze(-1)).sum() / msum / 3
    opn = (F.binary_cross_entropy_with_logits(ae[..., -2], gt[..., -1], reduction="none") * mask).sum() / msum
    stp = (F.binary_cross_entropy_with_logits(ae[..., -1], stop, reduction="none") * mask).sum() / msum
    return torch.stack([pos, rot, opn, stp, pos_w * pos + rot_w * rot + opn + stp])


# ================================================================================================= inputs of a row
def inputs(row):
    """-> dict of float32 CPU tensors; the row alone seeds them.  No float64 pre-activation lies within 1e-5 of zero (an offending
    draw is redrawn from the next seed: LeakyReLU' of a float32 and a float64 evaluation then agree everywhere)."""
    n, B, C, T = sum(row.counts), len(row.counts), row.C, row.T
    seed = 7 + 131 * n + 17 * C + T
    g = torch.Generator().manual_seed(seed)
    base, bias = torch.randn(n, C, generator=g), 0.5 * torch.randn(T, C, generator=g)
    w3 = torch.randn(4, C, generator=g) * (0.2 * (64.0 / C) ** 0.5)
    b3 = 0.1 * torch.randn(4, generator=g)
    pc = torch.randn(n, row.ld, generator=g)
    gx = torch.randn(B, T, 3, generator=g)
    for k in range(1, 100):
        bad = ((base.double()[None] + bias.double()[:, None]).abs() < 1e-5).any(0)
        if not bool(bad.any()):
            break
        base[bad] = torch.randn(int(bad.sum()), generator=torch.Generator().manual_seed(seed + 7919 * k))
    assert not bool(((base.double()[None] + bias.double()[:, None]).abs() < 1e-5).any())
    if row.opts.get("zero_steps"):
        if T > 1:
            gx[:, T // 2] = 0.0      # a whole step (of every cloud) ...
        gx[B - 1] = 0.0              # ... and a whole cloud
    scales = drop_scales(row, n)
    if row.opts.get("hot"):
        e, _ = head_ref(base.double(), bias.double(), w3.double(), b3.double(), pc.double()[:, :3], row.counts, row.temp, scales.double())
        s = row.opts["hot"] / float(e[..., 0].abs().max())
        w3[0] *= s
        b3[0] *= s
    return dict(base=base, bias=bias, w3=w3, b3=b3, pc=pc, g=gx, scales=scales)


def reference(row, v, e_stored=None):
    """float64 from the inputs: e, xt, stats = (max, log-sum-exp) of e0 / temp per (cloud, step), and the gradients of
    sum(g * xt).  e_stored [T, n, 4] (the 'hot' row): the softmax stage is evaluated AT the logits the kernel stored, the
    gradients still flow to the inputs through the float64 e.  The interface stores e in fp32; at |e0| = 100 and temp 0.1 its
    rounding alone (2^-24 x 100 = 6e-6) moves the exponent by 6e-5, i.e. every softmax weight — and every gradient, which is
    proportional to one — by 6e-5 relative: three times the bar before the kernel has computed anything.  e itself is still
    compared against float64 from the inputs.  tests/test_gpu_reghead.py treats the policy's large-logit rows the same way."""
    leaf = {k: v[k].double().requires_grad_(True) for k in ("base", "bias", "w3", "b3")}
    hook = None if e_stored is None else (lambda e: e + (e_stored.double() - e).detach())
    e, xt = head_ref(leaf["base"], leaf["bias"], leaf["w3"], leaf["b3"], v["pc"].double()[:, :3], row.counts, row.temp, v["scales"].double(),
                     hook)
    (xt * v["g"].double()).sum().backward()
    z = torch.split(e.detach()[..., 0] / row.temp, list(row.counts), dim=1)
    stats = torch.stack([torch.stack([s.max(1).values, torch.logsumexp(s, 1)], -1) for s in z], 0)      # [B, T, 2]
    return dict(e=e.detach(), xt=xt.detach(), stats=stats, dbase=leaf["base"].grad, dbias=leaf["bias"].grad, dw3=leaf["w3"].grad,
                db3=leaf["b3"].grad)


def offsets(counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    batch = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return torch.from_numpy(off), torch.from_numpy(batch)


# ================================================================================================= the fused entry points
def run_fused(row, v, chk):
    """lotus_mp_softpos_fwd / _bwd through the raw C-ABI into guarded buffers, workspaces of exactly the queried size, twice."""
    from dense_run import FILL
    from head_run import _ws
    from norm_run import _Bufs, _capi, _twice

    capi = _capi()
    n, B, C, T = sum(row.counts), len(row.counts), row.C, row.T
    off, batch = (t.cuda() for t in offsets(row.counts))
    Bf = _Bufs()
    pb, pbias, pw3, pb3 = Bf.inp("base", v["base"]), Bf.inp("bias", v["bias"]), Bf.inp("w3", v["w3"]), Bf.inp("b3", v["b3"].view(4, 1))
    ppc, pg = Bf.inp("pc", v["pc"]), Bf.inp("g", v["g"].view(B * T, 3))
    e, xt = Bf.out("e", T * n, 4), Bf.out("xt", B * T, 3)
    stats = Bf.out("stats", B * T, 2, torch.float64)
    dbase, dbias, dw3, db3 = Bf.out("dbase", n, C), Bf.out("dbias", T, C), Bf.out("dw3", 4, C), Bf.out("db3", 4, 1)
    nf, nb = capi.query("lotus_mp_softpos_workspace", B, T), capi.query("lotus_mp_softpos_bwd_workspace", n, C, T)
    wf, wb = _ws(Bf, nf, "workspace_fwd"), _ws(Bf, nb, "workspace_bwd")

    def body():
        Bf.b["workspace_fwd"].view.fill_(FILL)
        Bf.b["workspace_bwd"].view.fill_(FILL)
        capi.call("lotus_mp_softpos_fwd", pb, pbias, pw3, pb3, ppc, row.ld, off, B, n, C, T, row.temp, row.p, SEED, e, xt, stats, wf, nf)
        capi.call("lotus_mp_softpos_bwd", pg, pb, pbias, pw3, e, ppc, row.ld, batch, stats, xt, B, n, C, T, row.temp, row.p, SEED,
                  dbase, dbias, dw3, db3, wb, nb)

    got = _twice(Bf, chk, body)
    got["e"], got["xt"], got["stats"] = got["e"].view(T, n, 4), got["xt"].view(B, T, 3), got["stats"].view(B, T, 2)
    got["db3"] = got["db3"].view(4)
    return got


# ================================================================================================= the composition
class _Lvl:
    def __init__(self, counts):
        self.counts = list(counts)
        self.off, self.batch = (t.cuda() for t in offsets(counts))


def run_composed(row, v):
    """The same head from the entry points that were there before the fused pass, step by step: lotus_step_act_fwd ->
    lotus_softpos_fwd, then lotus_softpos_bwd -> linear_wgrad / linear_dgrad -> lotus_step_act_bwd (accumulating dbase over the
    steps).  lotus_step_act_bwd takes the widths whose quads divide 256; at the other widths of the table (132, 2048) its map
    dpre = dh * LeakyReLU'(base + bias_t) * mask is formed in fp32 torch arithmetic from the numpy mask instead."""
    from robot_3dlotus_amd import _capi, ops

    n, B, C, T = sum(row.counts), len(row.counts), row.C, row.T
    lvl = _Lvl(row.counts)
    base, bias, w3, b3, pc, gx = (v[k].cuda() for k in ("base", "bias", "w3", "b3", "pc", "g"))
    es, xts, sts = [], [], []
    dbase, dbias = torch.empty_like(base), torch.empty_like(bias)
    dw3, db3 = torch.zeros_like(w3), torch.zeros(4, device="cuda")
    sa_bwd = 256 % (C // 4) == 0
    ws = ops._ws(_capi.query("lotus_step_act_bwd_workspace", n, C), base.device) if sa_bwd else None
    for t in range(T):
        h = torch.empty_like(base)
        _capi.call("lotus_step_act_fwd", base, bias[t], h, n, C, ops.ACT_LEAKY, row.p, mix_seed(SEED, t))
        e, xt, st = ops.softpos_fwd(h, w3, b3, pc, lvl, row.temp)
        de = ops.softpos_bwd(gx[:, t].contiguous(), e, pc, lvl, st, xt, row.temp)
        dw, db = ops.linear_wgrad(de, h)
        ops.sync_side_stream()
        dw3, db3 = dw3 + dw, db3 + db
        dh = ops.linear_dgrad(de, w3)
        if sa_bwd:
            _capi.call("lotus_step_act_bwd", dh, base, bias[t], dbase, dbias[t], n, C, ops.ACT_LEAKY, row.p, mix_seed(SEED, t),
                       1 if t else 0, ws, ws.numel())
        else:
            pre = base + bias[t]
            dpre = dh * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE)) * v["scales"][t].cuda()
            dbase = dpre if t == 0 else dbase + dpre
            dbias[t] = dpre.sum(0)
        es.append(e); xts.append(xt); sts.append(st)
    torch.cuda.synchronize()
    return dict(e=torch.stack(es, 0), xt=torch.stack(xts, 1), stats=torch.stack(sts, 1), dbase=dbase, dbias=dbias, dw3=dw3, db3=db3)


# ================================================================================================= the losses
LOSS_CASES = {"1x1": (1, 1, 72, "full"), "2x5-prefix": (2, 5, 72, "prefix"), "7x5-holes": (7, 5, 72, "holes"),
              "86x1": (86, 1, 72, "full"), "300x8-prefix": (300, 8, 5, "prefix")}
POS_W, ROT_W = 1.5, 0.7
G5 = [0.3, -1.1, 0.9, 2.0, 0.6]


def loss_inputs(name):
    B, T, nrot, kind = LOSS_CASES[name]
    g = torch.Generator().manual_seed(3 + 1009 * B + 31 * T + nrot)
    ae = torch.randn(B, T, nrot * 3 + 2, generator=g)
    xt = 0.3 * torch.randn(B, T, 3, generator=g)
    gt = torch.cat([0.3 * torch.randn(B, T, 3, generator=g), torch.randint(0, nrot, (B, T, 3), generator=g).float(),
                    torch.randint(0, 2, (B, T, 1), generator=g).float()], -1)
    stop = torch.randint(0, 2, (B, T), generator=g).float()
    steps = torch.arange(T)[None]
    if kind == "prefix":
        lens = 1 + (torch.arange(B) * 3) % T
        mask = (steps < lens[:, None]).float()
    elif kind == "holes":
        mask = (torch.rand(B, T, generator=g) < 0.5).float()
        mask[torch.arange(B), torch.arange(B) % T] = 1.0
        mask[0] = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])[:T]
    else:
        mask = torch.ones(B, T)
    return dict(ae=ae, xt=xt, gt=gt, stop=stop, mask=mask.contiguous())


def loss_reference(name, v):
    nrot = LOSS_CASES[name][2]
    ae, xt = v["ae"].double().requires_grad_(True), v["xt"].double().requires_grad_(True)
    L = loss_ref(ae, xt, v["gt"].double(), v["stop"].double(), v["mask"].double(), nrot, POS_W, ROT_W)
    dae, dxt = torch.autograd.grad((L * torch.tensor(G5, dtype=torch.float64)).sum(), [ae, xt])
    return dict(losses=L.detach(), dae_out=dae, dxt_out=dxt)


def run_loss(name, v, chk):
    from norm_run import _Bufs, _capi, _twice

    capi = _capi()
    B, T, nrot, _ = LOSS_CASES[name]
    R, W = B * T, nrot * 3 + 2
    Bf = _Bufs()
    ae, xt, gt = Bf.inp("ae", v["ae"].view(R, W)), Bf.inp("xt", v["xt"].view(R, 3)), Bf.inp("gt", v["gt"].view(R, 7))
    stop, mask, g = Bf.inp("stop", v["stop"].view(R, 1)), Bf.inp("mask", v["mask"].view(R, 1)), Bf.inp("g", torch.tensor(G5).view(5, 1))
    losses, dae, dxt = Bf.out("losses", 5, 1), Bf.out("dae", R, W), Bf.out("dxt", R, 3)
    dae_out, dxt_out = Bf.out("dae_out", R, W), Bf.out("dxt_out", R, 3)

    def body():
        capi.call("lotus_mp_reg_loss_fwd", ae, gt, stop, mask, xt, B, T, nrot, 7, POS_W, ROT_W, losses, dae, dxt)
        capi.call("lotus_mp_reg_loss_bwd", dae, dxt, g, POS_W, ROT_W, B, T, nrot, dae_out, dxt_out)

    return _twice(Bf, chk, body)
