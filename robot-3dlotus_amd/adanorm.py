"""Adaptive PDNorm backbone of SimplePolicyPTV3AdaNorm (genrobo3d/models/simple_policy_ptv3.py:160-373) over the HIP operators.

The point backbone is the Block-only PointTransformerV3 (PointTransformerV3/model.py:864-1100) with every norm wrapped in
PDNorm(adaptive=True, decouple=False) (model.py:257-303): BatchNorm at the stem, every pooling and both unpooling branches,
LayerNorm at `cpe.2`, `norm1` and `norm2` of every Block.  Norm j of width C is modulated by one vector per cloud,
[shift_j | scale_j] = Linear_j(SiLU(c_b)), c_b the instruction (+ pose, + step) context of cloud b.

PointTransformerV3AdaNorm is ptv3.PointTransformerV3CA's skeleton (constructor, forward prologue, encoder / decoder walk) with the
PDNorm modules and steps overridden; the Block sub-block nodes run ops.{cpe,selfattn,ffn}_branch_{fwd,bwd} — the bodies they share
with ops.CpeFn / SelfAttnFn / FfnFn — between adaln_fwd and adaln_bwd.
The autograd nodes below are composed of the library's existing per-launch primitives (sparse convolution, dense layers,
patch attention, BatchNorm statistics) and the modulated-norm entry points of csrc/adanorm.hip.  Under data parallel
(parallel.GradReducer + parallel.enable_sync_batchnorm) the 13 BatchNorm sites of a five-stage model run split — statistics ->
one fp64 message per site and direction (the two unpooling branches share theirs: 9 forward + 9 backward) -> apply.  All modulation projections
of a forward pass are one product (ModAllFn; the same idea as ops.KvAllFn for the CABlocks): SiLU(c) [B, 256] against the
concatenated weights of every PDNorm, and one weight-gradient / one input-gradient product in backward over the d mod slab
that the norms' backward passes fill in place.  fp32 activation storage only.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._capi import call, query, WS
from .ops import ACT_GELU, BN_EPS, BN_MOMENTUM, _fwd, _joined, mix_seed
from .ptv3 import PointTransformerV3CA, SubMConv3d, _Attn, _MLP, _bn

_WS_SLOT = 6  # workspace slot of the (P, Q) partials (main stream)


# ------------------------------------------------------------------------------------ primitives
def _n_clouds(lvl):
    return len(lvl.counts)


def adaln_fwd(x, g, b, mod, lvl, res=None, eps=1e-5):
    """(LN(x) g + b) (1 + scale_b) + shift_b (+ res); mod = [B, 2C] (row stride free) of [shift | scale]."""
    M, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    call("lotus_adaln_fwd", x, res, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), y, mean, rstd, M, C, float(eps))
    return y, mean, rstd


def adaln_bwd(dy, x, mean, rstd, g, b, mod, dmod, lvl, add=None):
    """-> dx (+ add), dgamma, dbeta; d mod written into `dmod` ([B, 2C] view)."""
    M, C = x.shape
    B = _n_clouds(lvl)
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = WS.get(query("lotus_adanorm_workspace", M, B, C), x.device, slot=_WS_SLOT)
    call("lotus_adaln_bwd", dy, x, mean, rstd, g, b, mod, mod.stride(0), lvl.off, B, add, dx, dg, db, dmod, dmod.stride(0), M, C,
         ws, ws.numel())
    return dx, dg, db


def _split():
    """SyncBatchNorm route (statistics -> ops.BnState.reduce -> apply) of the BatchNorm sites: a training pass while a statistics
    hook is installed (parallel.enable_sync_batchnorm)."""
    return ops.BnState.reduce is not None


def _adabn_apply_sums(x, sums, g, b, rmean, rvar, mod, lvl, act):
    """Second half of the split forward: mean / invstd / running averages from the all-reduced sums and the modulated apply pass."""
    M, C = x.shape
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    call("lotus_adabn_apply_sums", x, sums, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), y, mean, invstd, rmean, rvar, M, C, act,
         float(BN_EPS), float(BN_MOMENTUM))
    return y, mean, invstd


def adabn_fwd(x, g, b, rmean, rvar, mod, lvl, training, act=ACT_GELU):
    """act((BN(x) g + b) (1 + scale_b) + shift_b): batch statistics (+ running-average update) in training, running ones in eval.
    With a statistics hook (SyncBatchNorm) the training pass is statistics -> one fp64 message (sum x, sum x^2, rows) -> apply."""
    M, C = x.shape
    if training and _split():
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
        ops._bn_stats(x, sums)
        ops.BnState.reduce(sums)
        return _adabn_apply_sums(x, sums, g, b, rmean, rvar, mod, lvl, act)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    if training:
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
        ws = ops._ws(query("lotus_batchnorm_workspace", M, C), x.device)
        call("lotus_batchnorm_stats_fused", x, sums, mean, invstd, rmean, rvar, M, C, float(BN_EPS), float(BN_MOMENTUM), ws,
             ws.numel(), ops._bn_counter(x.device))
    else:
        call("lotus_batchnorm_eval_stats", rmean, rvar, mean, invstd, C, float(BN_EPS))
    y = torch.empty_like(x)
    call("lotus_adabn_apply", x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), y, M, C, act)
    return y, mean, invstd


def adabn_fwd_pair(xa, pa, xb, pb, training, act=ACT_GELU):
    """Two independent sites (the branches of SerializedUnpooling) with ONE statistics message when SyncBatchNorm is on — the
    adaptive ops.bn_fwd_pair.  pa / pb = (g, b, rmean, rvar, mod, lvl)."""
    if not training or not _split():
        return adabn_fwd(xa, *pa, training, act), adabn_fwd(xb, *pb, training, act)
    na = 2 * xa.shape[1] + 1
    sums = torch.empty(na + 2 * xb.shape[1] + 1, dtype=torch.float64, device=xa.device)
    ops._bn_stats(xa, sums[:na])
    ops._bn_stats(xb, sums[na:])
    ops.BnState.reduce(sums)
    return _adabn_apply_sums(xa, sums[:na], *pa, act), _adabn_apply_sums(xb, sums[na:], *pb, act)


def _adabn_bwd_stats(dy, x, mean, invstd, g, b, mod, dmod, lvl, act, sums):
    """First half of the split backward: dgamma, dbeta (LOCAL sums: averaging them is the reducer's job), d mod into `dmod`, and the
    local message sums = (gamma dbeta, gamma dgamma, rows) in fp64."""
    M, C = x.shape
    B = _n_clouds(lvl)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = WS.get(query("lotus_adanorm_workspace", M, B, C), x.device, slot=_WS_SLOT)
    call("lotus_adabn_bwd_stats", dy, x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, B, dg, db, dmod, dmod.stride(0), sums, M, C,
         act, ws, ws.numel())
    return dg, db


def _adabn_bwd_apply_sums(dy, x, mean, invstd, g, b, mod, lvl, act, sums):
    M, C = x.shape
    dx = torch.empty_like(x)
    call("lotus_adabn_bwd_apply_sums", dy, x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), sums, dx, M, C, act)
    return dx


def adabn_bwd(dy, x, mean, invstd, g, b, mod, dmod, lvl, training, act=ACT_GELU):
    M, C = x.shape
    if training and _split():  # partials + fixed-order reduce -> message (sum dxhat, sum dxhat xhat, rows) -> apply
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
        dg, db = _adabn_bwd_stats(dy, x, mean, invstd, g, b, mod, dmod, lvl, act, sums)
        ops.BnState.reduce(sums)
        return _adabn_bwd_apply_sums(dy, x, mean, invstd, g, b, mod, lvl, act, sums), dg, db
    B = _n_clouds(lvl)
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = WS.get(query("lotus_adanorm_workspace", M, B, C), x.device, slot=_WS_SLOT)
    call("lotus_adabn_bwd", dy, x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, B, dx, dg, db, dmod, dmod.stride(0), M, C, act,
         1 if training else 0, ws, ws.numel())
    return dx, dg, db


def adabn_bwd_pair(a, bb, training, act=ACT_GELU):
    """Backward of adabn_fwd_pair: a / bb = (dy, x, mean, invstd, g, b, mod, dmod, lvl); one statistics message for both."""
    if not training or not _split():
        return adabn_bwd(*a, training, act), adabn_bwd(*bb, training, act)
    na = 2 * a[1].shape[1] + 1
    sums = torch.empty(na + 2 * bb[1].shape[1] + 1, dtype=torch.float64, device=a[1].device)
    sa, sb = sums[:na], sums[na:]
    ga = _adabn_bwd_stats(*a, act, sa)
    gb = _adabn_bwd_stats(*bb, act, sb)
    ops.BnState.reduce(sums)
    da = _adabn_bwd_apply_sums(*a[:7], a[8], act, sa)
    db_ = _adabn_bwd_apply_sums(*bb[:7], bb[8], act, sb)
    return (da,) + ga, (db_,) + gb


def silu(x, dy=None):
    y = torch.empty_like(x)
    call("lotus_ada_silu", x, dy, y, x.numel())
    return y


# ------------------------------------------------------------------------------------ modulation bank
class ModBank:
    """[shift | scale] of every PDNorm of one forward pass: `mod` [B, sum 2C_j], norm j in columns offs[j] : offs[j] + 2C_j.
    `dmod` (same shape) collects d mod, each norm's backward writing its own column slice."""
    __slots__ = ("mod", "dmod", "offs", "widths", "slices")

    def slice(self, j):
        return self.slices[j]

    def grad_slice(self, j):
        if self.dmod is None:
            self.dmod = torch.empty_like(self.mod)
        return self.dmod[:, self.offs[j]:self.offs[j] + self.widths[j]]


class ModAllFn(torch.autograd.Function):
    """mod_j = Linear_j(SiLU(c)) for every PDNorm j in ONE product: SiLU(c) [B, Cc] x cat(W_j) [sum 2C_j, Cc] (v1: 40 norms,
    24 064 columns).  The weights stay the modules' own parameters; their concatenation is one copy per step."""

    @_fwd
    def forward(ctx, context, bank, *wb):
        ws, bs = wb[0::2], wb[1::2]
        W = torch.cat(ws, 0)
        bias = torch.cat(bs, 0)
        s = silu(context)
        mod, _ = ops.linear_fwd(s, W, bias)
        bank.mod, bank.dmod = mod, None
        bank.widths = [w.shape[0] for w in ws]
        bank.offs = [0]
        for w_ in bank.widths[:-1]:
            bank.offs.append(bank.offs[-1] + w_)
        bank.slices = tuple(mod[:, o:o + w_] for o, w_ in zip(bank.offs, bank.widths))
        ctx.bank = bank
        ctx.save_for_backward(context, s, W)
        return bank.slices

    @_joined
    def backward(ctx, *gs):
        context, s, W = ctx.saved_tensors
        bank = ctx.bank
        if bank.dmod is None:
            bank.dmod = torch.empty_like(bank.mod)
        dmod = bank.dmod
        for j, g in enumerate(gs):  # normally every g IS its slice of the slab (written in place by the norm's backward)
            sl = dmod[:, bank.offs[j]:bank.offs[j] + bank.widths[j]]
            if g is None:
                sl.zero_()
            elif g.data_ptr() != sl.data_ptr() or g.stride() != sl.stride():
                sl.copy_(g)
        dW, db = ops.linear_wgrad(dmod, s)
        dctx = silu(context, ops.linear_dgrad(dmod, W)) if ctx.needs_input_grad[0] else None
        out = [dctx, None]
        for o, w_ in zip(bank.offs, bank.widths):
            out += [dW[o:o + w_], db[o:o + w_]]
        bank.dmod = None
        return tuple(out)


# ------------------------------------------------------------------------------------ sub-blocks
class AdaCpeFn(torch.autograd.Function):
    """x1 = x + PDNorm_LN(Linear(SubMConv3d_3(xs)))   (model.py:615-625, 661-663)."""

    @_fwd
    def forward(ctx, x, xs, mod, cw, cb, lw, lb, g, b, lvl, wt, bank, j):
        same = xs is x
        if wt is None:
            wt = ops.conv_weight_t(cw)
        c, l = ops.cpe_branch_fwd(xs, cw, cb, lw, lb, lvl, wt)
        y, mean, rstd = adaln_fwd(l, g, b, mod, lvl, res=x)
        ctx.meta = (lvl, same, bank, j)
        ctx.save_for_backward(xs, cw, lw, g, b, mod, c, l, mean, rstd, wt)
        return y

    @_joined
    def backward(ctx, dy):
        xs, cw, lw, g, b, mod, c, l, mean, rstd, wt = ctx.saved_tensors
        lvl, same, bank, j = ctx.meta
        dy = dy.contiguous()
        dmod = bank.grad_slice(j)
        dl, dg, db = adaln_bwd(dy, l, mean, rstd, g, b, mod, dmod, lvl)
        dx, dxs, dcw, dcb, dlw, dlb = ops.cpe_branch_bwd(dl, dy, xs, cw, lw, c, lvl, wt, same)
        return dx, dxs, dmod, dcw, dcb, dlw, dlb, dg, db, None, None, None, None


class AdaSelfAttnFn(torch.autograd.Function):
    """y = x + DropPath(drop(proj(PatchAttention(qkv(PDNorm_LN(x))))))   (model.py:664-668)."""

    @_fwd
    def forward(ctx, x, mod, g, b, wqkv, bqkv, qnw, qnb, knw, knb, wp, bp, lvl, H, drop_p, seed, attn_p, dpath, bank, j):
        """qnw = qnb = knw = knb = None: a block without q_norm / k_norm (qk_norm False)."""
        n, mean, rstd = adaln_fwd(x, g, b, mod, lvl)
        qn, kn = ((qnw, qnb), (knw, knb)) if qnw is not None else (None, None)
        y, qkv, att, lse = ops.selfattn_branch_fwd(n, x, wqkv, bqkv, qn, kn, wp, bp, lvl, H, drop_p, seed, attn_p, dpath)
        ctx.meta = (lvl, H, drop_p, seed, attn_p, float(dpath), bank, j)
        ctx.save_for_backward(x, g, b, mod, wqkv, qnw, qnb, knw, knb, wp, n, qkv, att, lse, mean, rstd)
        return y

    @_joined
    def backward(ctx, dy):
        x, g, b, mod, wqkv, qnw, qnb, knw, knb, wp, n, qkv, att, lse, mean, rstd = ctx.saved_tensors
        lvl, H, p, seed, attn_p, dpath, bank, j = ctx.meta
        dy = dy.contiguous()
        qn, kn = ((qnw, qnb), (knw, knb)) if qnw is not None else (None, None)
        dn, dwqkv, dbqkv, gq, bq, gk, bk, dwp, dbp = ops.selfattn_branch_bwd(dy, n, qkv, att, lse, wqkv, qn, kn, wp,
                                                                             lvl, H, p, seed, attn_p, dpath, None)
        dmod = bank.grad_slice(j)
        dx, dg, db = adaln_bwd(dn, x, mean, rstd, g, b, mod, dmod, lvl, add=dy)
        return (dx, dmod, dg, db, dwqkv, dbqkv, gq, bq, gk, bk, dwp, dbp) + (None,) * 8


class AdaFfnFn(torch.autograd.Function):
    """y = x + DropPath(drop(fc2(drop(GELU(fc1(PDNorm_LN(x)))))))   (model.py:671-675, MLP :577-583)."""

    @_fwd
    def forward(ctx, x, mod, g, b, w1, b1, w2, b2, lvl, drop_p, seed, dpath, bank, j):
        n, mean, rstd = adaln_fwd(x, g, b, mod, lvl)
        y, a, hpre = ops.ffn_branch_fwd(n, x, w1, b1, w2, b2, drop_p, seed, dpath)
        ctx.meta = (lvl, drop_p, seed, float(dpath), bank, j)
        ctx.save_for_backward(x, g, b, mod, w1, w2, n, hpre, a, mean, rstd)
        return y

    @_joined
    def backward(ctx, dy):
        x, g, b, mod, w1, w2, n, hpre, a, mean, rstd = ctx.saved_tensors
        lvl, p, seed, dpath, bank, j = ctx.meta
        dy = dy.contiguous()
        dn, dw1, db1, dw2, db2 = ops.ffn_branch_bwd(dy, n, hpre, a, w1, w2, p, seed, dpath, None)
        dmod = bank.grad_slice(j)
        dx, dg, db = adaln_bwd(dn, x, mean, rstd, g, b, mod, dmod, lvl, add=dy)
        return (dx, dmod, dg, db, dw1, db1, dw2, db2) + (None,) * 6


class AdaStemFn(torch.autograd.Function):
    """Embedding: GELU(PDNorm_BN(SubMConv3d_5(x)))   (model.py:844-861)."""

    @_fwd
    def forward(ctx, x, mod, cw, g, b, rmean, rvar, lvl, training, bank, j):
        c = ops.conv_fwd(x, cw, None, lvl.nbr125, lvl.order[0])
        y, mean, invstd = adabn_fwd(c, g, b, rmean, rvar, mod, lvl, training)
        ctx.meta = (lvl, training, bank, j)
        ctx.save_for_backward(x, mod, cw, g, b, c, mean, invstd)
        return y

    @_joined
    def backward(ctx, dy):
        x, mod, cw, g, b, c, mean, invstd = ctx.saved_tensors
        lvl, training, bank, j = ctx.meta
        dmod = bank.grad_slice(j)
        dc, dg, db = adabn_bwd(dy.contiguous(), c, mean, invstd, g, b, mod, dmod, lvl, training)
        dcw, _ = ops.conv_wgrad(dc, x, cw.shape, lvl.nbr125, need_bias=False, side=ctx.needs_input_grad[0])
        dx = ops.conv_dgrad(dc, cw, lvl.nbr125, lvl.order[0], lvl=lvl) if ctx.needs_input_grad[0] else None
        return dx, dmod, dcw, dg, db, None, None, None, None, None, None


class AdaStemGroupsFn(torch.autograd.Function):
    """AdaStemFn for an input given as two column groups with a weight each: SubMConv3d_5 is linear in its input columns, so
    conv(W, [xa | xb]) = conv(Wa, xa) + conv(Wb, xb) — two thin convolutions, the second adding onto the first, and one weight
    gradient per group.  The groups are never concatenated (the motion planner: point features | one-hot label, <= 8 columns each,
    where the concatenation would be wider than the thin-input kernels take)."""

    @_fwd
    def forward(ctx, xa, xb, mod, wa, wb, g, b, rmean, rvar, lvl, training, bank, j):
        ca = ops.conv_fwd(xa, wa, None, lvl.nbr125, lvl.order[0])
        c = ops.conv_fwd(xb, wb, None, lvl.nbr125, lvl.order[0], add=ca)
        y, mean, invstd = adabn_fwd(c, g, b, rmean, rvar, mod, lvl, training)
        ctx.meta = (lvl, training, bank, j, wa.shape, wb.shape)
        ctx.save_for_backward(xa, xb, mod, g, b, c, mean, invstd)
        return y

    @_joined
    def backward(ctx, dy):
        xa, xb, mod, g, b, c, mean, invstd = ctx.saved_tensors
        lvl, training, bank, j, wa_shape, wb_shape = ctx.meta
        dmod = bank.grad_slice(j)
        dc, dg, db = adabn_bwd(dy.contiguous(), c, mean, invstd, g, b, mod, dmod, lvl, training)
        dwa, _ = ops.conv_wgrad(dc, xa, wa_shape, lvl.nbr125, need_bias=False)
        dwb, _ = ops.conv_wgrad(dc, xb, wb_shape, lvl.nbr125, need_bias=False)
        return None, None, dmod, dwa, dwb, dg, db, None, None, None, None, None, None


class AdaPoolFn(torch.autograd.Function):
    """SerializedPooling: GELU(PDNorm_BN(segment_max(Linear(x))))   (model.py:760-790); the norm sees the pooled level's clouds."""

    @_fwd
    def forward(ctx, x, mod, w, bias, g, b, rmean, rvar, child, training, bank, j):
        proj, _ = ops.linear_fwd(x, w, bias)
        C = w.shape[0]
        pooled = torch.empty(child.n, C, dtype=x.dtype, device=x.device)
        arg = torch.empty(child.n, C, dtype=torch.int32, device=x.device)
        call("lotus_pool_max_fwd", proj, child.members, child.seg_start, child.n, C, pooled, arg)
        y, mean, invstd = adabn_fwd(pooled, g, b, rmean, rvar, mod, child, training)
        ctx.meta = (child, training, bank, j)
        ctx.save_for_backward(x, mod, w, g, b, pooled, arg, mean, invstd)
        return y

    @_joined
    def backward(ctx, dy):
        x, mod, w, g, b, pooled, arg, mean, invstd = ctx.saved_tensors
        child, training, bank, j = ctx.meta
        C = w.shape[0]
        dmod = bank.grad_slice(j)
        dpool, dg, db = adabn_bwd(dy.contiguous(), pooled, mean, invstd, g, b, mod, dmod, child, training)
        dproj = torch.empty(x.shape[0], C, dtype=x.dtype, device=x.device)
        call("lotus_pool_max_bwd", dpool, arg, child.cluster, x.shape[0], C, dproj)
        dw, dbias = ops.linear_wgrad(dproj, x)
        dx = ops.linear_dgrad(dproj, w)
        return dx, dmod, dw, dbias, dg, db, None, None, None, None, None, None


class AdaUnpoolFn(torch.autograd.Function):
    """SerializedUnpooling: skip = GELU(PDNorm_BN(Linear_skip(parent))), up = GELU(PDNorm_BN(Linear(point)));
    returns (skip + up[cluster], skip)   (model.py:817-828).  `up` is modulated per cloud of the coarse level, `skip` per
    cloud of the fine one."""

    @_fwd
    def forward(ctx, xc, xp, modu, mods, wu, bu, gu, betau, rmu, rvu, ws_, bs, gs, betas, rms, rvs, child, lvl, training, bank,
                ju, js):
        lu, _ = ops.linear_fwd(xc, wu, bu)
        ls, _ = ops.linear_fwd(xp, ws_, bs)
        (up, mu, iu), (skip, ms, is_) = adabn_fwd_pair(lu, (gu, betau, rmu, rvu, modu, child), ls, (gs, betas, rms, rvs, mods, lvl),
                                                       training)
        x = torch.empty_like(skip)
        call("lotus_unpool_fwd", skip, up, child.cluster, skip.shape[0], skip.shape[1], x)
        ctx.meta = (child, lvl, training, bank, ju, js)
        ctx.save_for_backward(xc, xp, modu, mods, wu, gu, betau, ws_, gs, betas, lu, ls, mu, iu, ms, is_)
        return x, skip

    @_joined
    def backward(ctx, dx, dskip):
        xc, xp, modu, mods, wu, gu, betau, ws_, gs, betas, lu, ls, mu, iu, ms, is_ = ctx.saved_tensors
        child, lvl, training, bank, ju, js = ctx.meta
        C = wu.shape[0]
        dx = dx.contiguous()
        dup = torch.empty(child.n, C, dtype=dx.dtype, device=dx.device)
        call("lotus_unpool_bwd", dx, child.members, child.seg_start, child.n, C, dup)
        dsk = ops.add(dx, dskip.contiguous()) if dskip is not None else dx
        dmu, dms = bank.grad_slice(ju), bank.grad_slice(js)
        (dlu, dgu, dbetau), (dls, dgs, dbetas) = adabn_bwd_pair((dup, lu, mu, iu, gu, betau, modu, dmu, child),
                                                                (dsk, ls, ms, is_, gs, betas, mods, dms, lvl), training)
        dwu, dbu = ops.linear_wgrad(dlu, xc)
        dxc = ops.linear_dgrad(dlu, wu)
        dws, dbs = ops.linear_wgrad(dls, xp)
        dxp = ops.linear_dgrad(dls, ws_)
        return (dxc, dxp, dmu, dms, dwu, dbu, dgu, dbetau, None, None, dws, dbs, dgs, dbetas) + (None,) * 8


# ------------------------------------------------------------------------------------ modules
class PDNorm(nn.Module):
    """Parameter container with the layout of model.py:257-278 (decouple = False, adaptive = True):
    `norm` (nn.LayerNorm / nn.BatchNorm1d) and `modulation` = Sequential(SiLU, Linear(context, 2C))."""

    def __init__(self, norm, c, context_channels=256):
        super().__init__()
        self.norm = norm
        self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(context_channels, 2 * c))

    @property
    def num_batches_tracked(self):
        return self.norm.num_batches_tracked


def _pd_ln(c, ctx):
    return PDNorm(nn.LayerNorm(c), c, ctx)


def _pd_bn(c, ctx):
    return PDNorm(_bn(c), c, ctx)


class AdaBlock(nn.Module):
    """model.py:586-680 with PDNorm LayerNorms (cpe.2, norm1, norm2); attn.q_norm / k_norm stay plain (nn.Identity when
    qk_norm is False: the patch attention then runs without them)."""

    def __init__(self, c, h, mlp_ratio, ctx, qk_norm=True):
        super().__init__()
        self.num_heads = h
        self.cpe = nn.Sequential(SubMConv3d(c, c, 3, bias=True), nn.Linear(c, c), _pd_ln(c, ctx))
        self.norm1 = nn.Sequential(_pd_ln(c, ctx))
        self.attn = _Attn(c, h, qk_norm)
        self.norm2 = nn.Sequential(_pd_ln(c, ctx))
        self.mlp = nn.Sequential(_MLP(c, int(c * mlp_ratio)))


class _AdaDown(nn.Module):
    def __init__(self, cin, cout, ctx):
        super().__init__()
        self.proj = nn.Linear(cin, cout)
        self.norm = nn.Sequential(_pd_bn(cout, ctx))


class _AdaUp(nn.Module):
    def __init__(self, cin, cskip, cout, ctx):
        super().__init__()
        self.proj = nn.Sequential(nn.Linear(cin, cout), _pd_bn(cout, ctx))
        self.proj_skip = nn.Sequential(nn.Linear(cskip, cout), _pd_bn(cout, ctx))


class _AdaStem(nn.Module):
    def __init__(self, cin, cout, ctx):
        super().__init__()
        self.conv = SubMConv3d(cin, cout, 5, bias=False)
        self.norm = _pd_bn(cout, ctx)


class _AdaEmbedding(nn.Module):
    def __init__(self, cin, cout, ctx):
        super().__init__()
        self.stem = _AdaStem(cin, cout, ctx)


def check_pdnorm_options(pdnorm_bn, pdnorm_ln, pdnorm_decouple, pdnorm_adaptive, pdnorm_affine, pdnorm_only_decoder):
    """The one PDNorm combination built here: the reference YAML's (simple_policy_ptv3.yaml:93 ff.)."""
    want = dict(pdnorm_bn=True, pdnorm_ln=True, pdnorm_decouple=False, pdnorm_adaptive=True, pdnorm_affine=True,
                pdnorm_only_decoder=False)
    got = dict(pdnorm_bn=pdnorm_bn, pdnorm_ln=pdnorm_ln, pdnorm_decouple=pdnorm_decouple, pdnorm_adaptive=pdnorm_adaptive,
               pdnorm_affine=pdnorm_affine, pdnorm_only_decoder=pdnorm_only_decoder)
    bad = [f"{k}={got[k]}" for k in want if bool(got[k]) != want[k]]
    if bad:
        raise NotImplementedError(f"SimplePolicyPTV3AdaNorm builds pdnorm_bn = pdnorm_ln = pdnorm_adaptive = pdnorm_affine = True, "
                                  f"pdnorm_decouple = pdnorm_only_decoder = False only; unsupported: {bad}")


class PointTransformerV3AdaNorm(PointTransformerV3CA):
    """PointTransformerV3(pdnorm_bn = pdnorm_ln = pdnorm_adaptive = True), model.py:864-1100: every stage a chain of Blocks.
    forward(data_dict) takes data_dict["context"] = [B, pdnorm_context_channels], one vector per cloud.  The constructor, the
    forward prologue and the encoder / decoder walk, the front end, its prefetch, seeds and pack helpers are
    PointTransformerV3CA's; this class supplies the PDNorm modules and the steps of a pass that run them."""
    block_cls = AdaBlock
    plain_attention = True

    def __init__(self, *args, pdnorm_bn=True, pdnorm_ln=True, pdnorm_decouple=False, pdnorm_adaptive=True, **kw):
        super().__init__(*args, pdnorm_bn=pdnorm_bn, pdnorm_ln=pdnorm_ln, pdnorm_decouple=pdnorm_decouple,
                         pdnorm_adaptive=pdnorm_adaptive, **kw)

    # -- construction
    @staticmethod
    def _pdnorm_unsupported(*flags):
        check_pdnorm_options(*flags)
        return {}

    @staticmethod
    def _context_width(ctx_channels, pdnorm_context_channels):
        return pdnorm_context_channels

    def _make_embedding(self, cin, cout):
        return _AdaEmbedding(cin, cout, self.context_channels)

    def _make_down(self, cin, cout):
        return _AdaDown(cin, cout, self.context_channels)

    def _make_up(self, cin, cskip, cout):
        return _AdaUp(cin, cskip, cout, self.context_channels)

    def _add_depth(self, stage, i, c, h, mlp_ratio):
        stage.add_module(f"block{i}", AdaBlock(c, h, mlp_ratio, self.context_channels, self.qk_norm))

    def _index_sites(self):
        self._pdnorms = [m for m in self.modules() if isinstance(m, PDNorm)]  # slice j of the modulation bank = norm j
        self._pd_index = {id(m): j for j, m in enumerate(self._pdnorms)}

    def _drop_param_caches(self):
        self._nbt = None

    def _check_sync_bn(self):
        """Data parallel (train_simple_policy.py:116-117,177): BatchNorm containers converted by
        `nn.SyncBatchNorm.convert_sync_batchnorm` switch the statistics messages on (parallel.enable_sync_batchnorm — collective:
        every rank enters its first forward), as PointTransformerV3CA does.  A process group of more than one rank with neither
        converted containers nor a statistics hook would normalise per rank, which is not what the reference trains: refused."""
        import torch.distributed as dist
        if ops.BnState.reduce is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if not any(isinstance(m, nn.SyncBatchNorm) for m in self.modules()):
                raise NotImplementedError(
                    f"SimplePolicyPTV3AdaNorm in a process group with world size {dist.get_world_size()} > 1 needs SyncBatchNorm "
                    "statistics: convert the model with nn.SyncBatchNorm.convert_sync_batchnorm(model) or call "
                    "parallel.enable_sync_batchnorm() before the first forward (BatchNorm per rank is not built)")
            from . import parallel
            parallel.enable_sync_batchnorm()
        self._sync_bn_checked = True

    def _mod_params(self):
        wb = []
        for m in self._pdnorms:
            lin = m.modulation[1]
            wb += [lin.weight, lin.bias]
        return wb

    # -- the steps of a pass
    def _check_inputs(self, feat, counts, context):
        if context is None or context.dim() != 2 or context.shape[0] != len(counts) or context.shape[1] != self.context_channels:
            raise ValueError(f"PointTransformerV3AdaNorm needs one context vector per cloud: [{len(counts)}, "
                             f"{self.context_channels}], got {None if context is None else tuple(context.shape)}")
        if context.dtype != torch.float32 or feat.dtype != torch.float32:
            raise NotImplementedError("SimplePolicyPTV3AdaNorm stores activations in fp32 only")

    def _begin(self, fw, data_dict, feat):
        """Top of a pass -> stem output: the modulation bank of every PDNorm, the stem, then the join of the packed weights."""
        fw.bank = ModBank()
        fw.mods = ModAllFn.apply(fw.context, fw.bank, *self._mod_params())
        st = self.embedding.stem
        nb, j = st.norm.norm, self._pd_index[id(st.norm)]
        groups = data_dict.get("stem_groups")
        if groups is not None:
            # (xa, xb, wa, wb): the input as two column groups, each with its weight [cout, 5, 5, 5, columns of the group] — a
            # differentiable function of st.conv.weight (the motion planner: point features | one-hot point label)
            xa, xb, wa, wb = groups
            if xa.shape[1] > 8 or xb.shape[1] > 8:
                raise NotImplementedError(f"stem_groups of {xa.shape[1]} and {xb.shape[1]} columns: the thin-input stem "
                                          "convolution takes at most 8 columns per group")
            x = AdaStemGroupsFn.apply(xa, xb, fw.mods[j], wa, wb, nb.weight, nb.bias, nb.running_mean, nb.running_var,
                                      fw.levels[0], fw.training, fw.bank, j)
        else:
            x = AdaStemFn.apply(feat, fw.mods[j], st.conv.weight, nb.weight, nb.bias, nb.running_mean, nb.running_var,
                                fw.levels[0], fw.training, fw.bank, j)
        ops.sync_side_stream()  # the packed convolution weights
        return x

    def _enter_stage(self, fw, lvl):
        pass

    def _pool(self, fw, d, x, lvl):
        pn = d.norm[0]
        j = self._pd_index[id(pn)]
        return AdaPoolFn.apply(x, fw.mods[j], d.proj.weight, d.proj.bias, pn.norm.weight, pn.norm.bias, pn.norm.running_mean,
                               pn.norm.running_var, lvl, fw.training, fw.bank, j)

    def _unpool(self, fw, up, x, skip, child, lvl):
        u, us = up.proj, up.proj_skip
        nu, ns = u[1], us[1]
        ju, js = self._pd_index[id(nu)], self._pd_index[id(ns)]
        return AdaUnpoolFn.apply(x, skip, fw.mods[ju], fw.mods[js], u[0].weight, u[0].bias, nu.norm.weight, nu.norm.bias,
                                 nu.norm.running_mean, nu.norm.running_var, us[0].weight, us[0].bias, ns.norm.weight,
                                 ns.norm.bias, ns.norm.running_mean, ns.norm.running_var, child, lvl, fw.training, fw.bank, ju, js)

    def _run_depth(self, fw, stage, i, x, xs, lvl_o, lvl, si, dpath):
        blk, mods, bank, pid, p = getattr(stage, f"block{i}"), fw.mods, fw.bank, self._pd_index, fw.p
        c0, c1, pc = blk.cpe[0], blk.cpe[1], blk.cpe[2]
        x = AdaCpeFn.apply(x, xs, mods[pid[id(pc)]], c0.weight, c0.bias, c1.weight, c1.bias, pc.norm.weight, pc.norm.bias,
                           lvl_o, fw.packs[blk], bank, pid[id(pc)])
        a, n1 = blk.attn, blk.norm1[0]
        qk = (a.q_norm.weight, a.q_norm.bias, a.k_norm.weight, a.k_norm.bias) if self.qk_norm else (None,) * 4
        x = AdaSelfAttnFn.apply(x, mods[pid[id(n1)]], n1.norm.weight, n1.norm.bias, a.qkv.weight, a.qkv.bias, *qk,
                                a.proj.weight, a.proj.bias, lvl_o, blk.num_heads, p, si, fw.pa, dpath, bank, pid[id(n1)])
        m, n2 = blk.mlp[0], blk.norm2[0]
        return AdaFfnFn.apply(x, mods[pid[id(n2)]], n2.norm.weight, n2.norm.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight,
                              m.fc2.bias, lvl_o, p, mix_seed(si, 2), dpath, bank, pid[id(n2)])


def cloud_context(txt_ctx, txt_w, lens):
    """txt_reduce == 'attn' (simple_policy_ptv3.py:204-211): per cloud, softmax over its tokens of txt_attn_fc, weighting the
    projected tokens.  txt_ctx [T, C], txt_w [T, 1], lens: tokens per cloud -> [B, C].  Padded to the longest instruction:
    every index but the padding one is gathered once, so the backward pass has no colliding accumulation."""
    B, L = len(lens), max(lens)
    T = txt_ctx.shape[0]
    idx = np.full((B, L), T, dtype=np.int64)
    st = 0
    for b, n in enumerate(lens):
        idx[b, :n] = np.arange(st, st + n)
        st += n
    idx_t = torch.from_numpy(idx).to(txt_ctx.device)
    w = torch.cat([txt_w[:, 0], txt_w.new_full((1,), float("-inf"))])[idx_t]          # [B, L]
    p = torch.softmax(w, 1)
    tok = torch.cat([txt_ctx, txt_ctx.new_zeros(1, txt_ctx.shape[1])])[idx_t]          # [B, L, C]
    return (p.unsqueeze(-1) * tok).sum(1)
