"""Adaptive PDNorm backbone of SimplePolicyPTV3AdaNorm (genrobo3d/models/simple_policy_ptv3.py:160-373) over the HIP operators.

The point backbone is the Block-only PointTransformerV3 (PointTransformerV3/model.py:864-1100) with every norm wrapped in
PDNorm(adaptive=True, decouple=False) (model.py:257-303): BatchNorm at the stem, every pooling and both unpooling branches,
LayerNorm at `cpe.2`, `norm1` and `norm2` of every Block.  Norm j of width C is modulated by one vector per cloud,
[shift_j | scale_j] = Linear_j(SiLU(c_b)), c_b the instruction (+ pose, + step) context of cloud b.

PointTransformerV3AdaNorm is ptv3.PointTransformerV3CA's skeleton (constructor, forward prologue, encoder / decoder walk) with the
PDNorm modules and steps overridden.  Every site runs the node of the plain backbones — ops.StemFn / PoolFn / UnpoolFn / CpeFn /
SelfAttnFn / FfnFn, per launch — handed the site's modulation slice: the norm primitives of ops.py (ln_fwd / ln_bwd, bn_fwd /
bn_bwd and their pair forms) then call the modulated-norm entry points of csrc/adanorm.hip.  Under data parallel
(parallel.GradReducer + parallel.enable_sync_batchnorm) the 13 BatchNorm sites of a five-stage model run split — statistics ->
one fp64 message per site and direction (the two unpooling branches share theirs: 9 forward + 9 backward) -> apply.  All modulation projections
of a forward pass are one product (ops.ProjAllFn with pre = "silu", the node that projects the keys / values of the CABlocks):
SiLU(c) [B, 256] against the concatenated weights of every PDNorm, and one weight-gradient / one input-gradient product in
backward over the gradient slab of the ops.ProjBank that the norms' backward passes fill in place.  fp32 activation storage only.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .ops import ACT_GELU, _fwd, _joined
from .ptv3 import Block, PointTransformerV3CA, SubMConv3d, _Attn, _MLP, _bn


# ------------------------------------------------------------------------------------ primitives
# The adaptive norms are ops.ln_* / bn_* given `mod`; these are their names and argument orders for direct callers (tests/).
def adaln_fwd(x, g, b, mod, lvl, res=None, eps=1e-5):
    """(LN(x) g + b) (1 + scale_b) + shift_b (+ res); mod = [B, 2C] (row stride free) of [shift | scale]."""
    return ops.ln_fwd(x, g, b, res, eps, True, mod, lvl)


def adaln_bwd(dy, x, mean, rstd, g, b, mod, dmod, lvl, add=None):
    """-> dx (+ add), dgamma, dbeta; d mod written into `dmod` ([B, 2C] view)."""
    return ops.ln_bwd(dy, x, mean, rstd, g, add, None, b, mod, dmod, lvl)


def adabn_fwd(x, g, b, rmean, rvar, mod, lvl, training, act=ACT_GELU):
    """act((BN(x) g + b) (1 + scale_b) + shift_b), see ops.bn_fwd."""
    return ops.bn_fwd(x, g, b, rmean, rvar, training, act, mod=mod, lvl=lvl)


def adabn_bwd(dy, x, mean, invstd, g, b, mod, dmod, lvl, training, act=ACT_GELU):
    return ops.bn_bwd(dy, x, mean, invstd, g, b, training, act, mod, dmod, lvl)


def _adabn_apply_sums(x, sums, g, b, rmean, rvar, mod, lvl, act):
    """Second half of the split forward: mean / invstd / running averages from the all-reduced sums and the modulated apply pass."""
    return ops._bn_apply_sums(x, sums, g, b, rmean, rvar, act, mod=mod, lvl=lvl)


def _adabn_bwd_stats(dy, x, mean, invstd, g, b, mod, dmod, lvl, act, sums):
    """First half of the split backward -> (dgamma, dbeta), d mod into `dmod`, the local fp64 message into `sums`."""
    return ops._bn_bwd_stats(dy, x, mean, invstd, g, b, act, sums, True, mod, dmod, lvl)


def _adabn_bwd_apply_sums(dy, x, mean, invstd, g, b, mod, lvl, act, sums):
    return ops._bn_bwd_apply(dy, x, mean, invstd, g, b, True, act, sums, (None, None), mod, None, lvl)[0]


# ------------------------------------------------------------------------------------ the two-group stem
class StemGroupsFn(torch.autograd.Function):
    """ops.StemFn for an input given as two column groups with a weight each: SubMConv3d_5 is linear in its input columns, so
    conv(W, [xa | xb]) = conv(Wa, xa) + conv(Wb, xb) — two thin convolutions, the second adding onto the first, and one weight
    gradient per group.  The groups are never concatenated (the motion planner: point features | one-hot label, <= 8 columns each,
    where the concatenation would be wider than the thin-input kernels take)."""

    @_fwd
    def forward(ctx, xa, xb, mod, wa, wb, g, b, rmean, rvar, lvl, training, bank, j):
        ca = ops.conv_fwd(xa, wa, None, lvl.nbr125, lvl.order[0])
        c = ops.conv_fwd(xb, wb, None, lvl.nbr125, lvl.order[0], add=ca)
        y, mean, invstd = ops.bn_fwd(c, g, b, rmean, rvar, training, ACT_GELU, mod=mod, lvl=lvl)
        ctx.meta = (lvl, training, bank, j, wa.shape, wb.shape)
        ctx.save_for_backward(xa, xb, mod, g, b, c, mean, invstd)
        return y

    @_joined
    def backward(ctx, dy):
        xa, xb, mod, g, b, c, mean, invstd = ctx.saved_tensors
        lvl, training, bank, j, wa_shape, wb_shape = ctx.meta
        dmod = ops._dmod(mod, (bank, j))
        dc, dg, db = ops.bn_bwd(dy.contiguous(), c, mean, invstd, g, b, training, ACT_GELU, mod, dmod, lvl)
        dwa, _ = ops.conv_wgrad(dc, xa, wa_shape, lvl.nbr125, need_bias=False)
        dwb, _ = ops.conv_wgrad(dc, xb, wb_shape, lvl.nbr125, need_bias=False)
        return None, None, dmod, dwa, dwb, dg, db, None, None, None, None, None, None


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
    qk_norm is False: the patch attention then runs without them).  Not a ptv3.Block (whose constructor builds the plain norms),
    but run by its walker."""

    def __init__(self, c, h, mlp_ratio, ctx, qk_norm=True, coords=False, rpe_patch=None):
        super().__init__()
        self.num_heads = h
        self.cpe = nn.Sequential(SubMConv3d(c, c, 3, bias=True), nn.Linear(c, c), _pd_ln(c, ctx))
        self.norm1 = nn.Sequential(_pd_ln(c, ctx))
        self.attn = _Attn(c, h, qk_norm, coords, rpe_patch)
        self.norm2 = nn.Sequential(_pd_ln(c, ctx))
        self.mlp = nn.Sequential(_MLP(c, int(c * mlp_ratio)))

    run = Block.run


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
    coord_attention = True
    dense_attention = True
    long_patches = True

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
        stage.add_module(f"block{i}", AdaBlock(c, h, mlp_ratio, self.context_channels, self.qk_norm, self.add_coords,
                                                   self.rpe_patch))

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
        fw.bank = ops.ProjBank()
        fw.mods = ops.ProjAllFn.apply(fw.context, fw.bank, "silu", *self._mod_params())
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
            x = StemGroupsFn.apply(xa, xb, fw.mods[j], wa, wb, nb.weight, nb.bias, nb.running_mean, nb.running_var,
                                   fw.levels[0], fw.training, fw.bank, j)
        else:
            x = ops.StemFn.apply(feat, st.conv.weight, nb.weight, nb.bias, nb.running_mean, nb.running_var, fw.levels[0], fw.training,
                                 fw.mods[j], fw.bank, j)
        ops.sync_side_stream()  # the packed convolution weights
        return x

    def _enter_stage(self, fw, lvl):
        pass

    def _pool(self, fw, d, x, lvl):
        pn = d.norm[0]
        j = self._pd_index[id(pn)]
        return ops.PoolFn.apply(x, d.proj.weight, d.proj.bias, pn.norm.weight, pn.norm.bias, pn.norm.running_mean,
                                pn.norm.running_var, lvl, fw.training, fw.mods[j], fw.bank, j)

    def _unpool(self, fw, up, x, skip, child, lvl):
        u, us = up.proj, up.proj_skip
        nu, ns = u[1], us[1]
        ju, js = self._pd_index[id(nu)], self._pd_index[id(ns)]
        return ops.UnpoolFn.apply(x, skip, u[0].weight, u[0].bias, nu.norm.weight, nu.norm.bias, nu.norm.running_mean,
                                  nu.norm.running_var, us[0].weight, us[0].bias, ns.norm.weight, ns.norm.bias, ns.norm.running_mean,
                                  ns.norm.running_var, child, fw.training, fw.mods[ju], fw.mods[js], fw.bank, ju, js, lvl)

    def _run_depth(self, fw, stage, i, x, xs, lvl_o, lvl, si, dpath):
        blk = getattr(stage, f"block{i}")
        return blk.run(x, xs, lvl_o, fw.p, si, fw.pa, fw.packs[blk], dpath, fw.mods, fw.bank, self._pd_index)[0]


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
