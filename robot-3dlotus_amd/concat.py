"""Backbone of SimplePolicyPTV3Concat (genrobo3d/models/simple_policy_ptv3.py:434-463) over the HIP operators.

The reference repeats the context vector of a cloud — txt_fc(txt) (+ pose) (+ step) — over the cloud's points and concatenates it
to pc_fts (:457-461); the backbone is then a plain PointTransformerV3 (PointTransformerV3/model.py:864-1100, no cross attention,
no adaptive norm) whose 5^3 stem convolution (:844-853) has `c_pc + context_channels` input columns.  All but c_pc of them are
constant over a cloud, and SubMConv3d is linear in its input columns (as adanorm.StemGroupsFn already uses), so with
P_b[t] = W_ctx[:, t, :] ctx_b for the 125 taps t

    conv(W, [pc | ctx_b(i)])_i = conv(W_pc, pc)_i + sum over the taps t with nbr125[t][i] >= 0 of P_b(i)[t]

(a neighbour is always in the same cloud: the batch index is part of the voxel key).  The wide part needs the presence bits of the
neighbour table and a [B, 125, cout] table that one small dense product makes: cout additions per present pair instead of
(c_pc + 256) x cout multiply-adds, and the [N, c_pc + 256] input never exists (csrc/ctx_stem.hip: lotus_ctx_taps_fwd / _bwd).

PointTransformerV3Plain is ptv3.PointTransformerV3CA's skeleton with the hooks overridden: every stage a chain of Blocks, the stem
above, plain BatchNorm pooling / unpooling.  Either way the blocks run ptv3.Block.run: with qk_norm True the composites as they
are; with qk_norm False ops.SelfAttnFn runs per launch — LayerNorm, qkv, patch attention without q/k LayerNorm, proj — and no
hand-over is made.  fp32 activation storage only.
"""
import torch
import torch.nn as nn

from . import ops
from ._capi import call, query, WS
from .ops import ACT_GELU, _fwd, _joined
from .ptv3 import Block, PointTransformerV3CA, _Attn

_WS_SLOT = 6  # workspace slot of the dP chunk partials (main stream)
MAX_PC_COLUMNS = 8  # the thin-input stem convolution of csrc/conv.hip


def _taps_dims(P, lvl):
    T = lvl.nbr125.shape[0]
    return len(lvl.counts), lvl.n, T, P.shape[1] // T


def ctx_taps_fwd(P, lvl, add=None):
    """y_i = add_i + sum_{t ascending, nbr125[t][i] >= 0} P[b(i)][t];  P [B, T * C] (tap-major rows of C)."""
    B, n, T, C = _taps_dims(P, lvl)
    y = torch.empty(n, C, dtype=torch.float32, device=P.device)
    call("lotus_ctx_taps_fwd", P, lvl.nbr125, lvl.off, add, y, B, n, T, C)
    return y


def ctx_taps_bwd(dy, lvl, T):
    """dP[b][t] = sum_{i in cloud b, nbr125[t][i] >= 0} dy_i -> [B, T * C]."""
    n, C = dy.shape
    B = len(lvl.counts)
    dP = torch.empty(B, T * C, dtype=torch.float32, device=dy.device)
    ws = WS.get(query("lotus_ctx_taps_workspace", B, T, C), dy.device, slot=_WS_SLOT)
    call("lotus_ctx_taps_bwd", dy, lvl.nbr125, lvl.off, dP, B, n, T, C, ws, ws.numel())
    return dP


def split_stem_weight(w, c_pc):
    """stem.conv.weight [cout, 5, 5, 5, c_pc + Cc] -> (W_pc [cout, 5, 5, 5, c_pc], W_ctx [T * cout, Cc] tap-major), contiguous
    differentiable: ops.SplitStemWeightFn carries both gradients back into the one parameter, assembled in one gradient slab."""
    return ops.SplitStemWeightFn.apply(w, c_pc)


def ctx_stem_pre(pc, cvec, w_pc, w_ctx, lvl):
    """The stem convolution of [pc | repeat(cvec)] before its norm: conv(W_pc, pc) + taps(P), P = cvec W_ctx^T."""
    P, _ = ops.linear_fwd(cvec, w_ctx, None)
    ca = ops.conv_fwd(pc, w_pc, None, lvl.nbr125, lvl.order[0])
    return ctx_taps_fwd(P, lvl, add=ca)


class CtxStemFn(torch.autograd.Function):
    """Embedding of the Concat policy: GELU(BN(SubMConv3d_5([pc | repeat(cvec)])))   (model.py:844-861; conv has no bias) with the
    context columns folded into per-cloud tap sums.  pc [N, <= 8 columns] gets no gradient; cvec [B, Cc]."""

    @_fwd
    def forward(ctx, pc, cvec, w_pc, w_ctx, g, b, rmean, rvar, lvl, training):
        c = ctx_stem_pre(pc, cvec, w_pc, w_ctx, lvl)
        y, mean, invstd = ops.bn_fwd(c, g, b, rmean, rvar, training, ACT_GELU)
        ctx.meta = (lvl, training, w_pc.shape)
        ctx.save_for_backward(pc, cvec, w_ctx, g, b, c, mean, invstd)
        return y

    @_joined
    def backward(ctx, dy):
        pc, cvec, w_ctx, g, b, c, mean, invstd = ctx.saved_tensors
        lvl, training, wpc_shape = ctx.meta
        dc, dg, db = ops.bn_bwd(dy.contiguous(), c, mean, invstd, g, b, training, ACT_GELU)
        dw_pc, _ = ops.conv_wgrad(dc, pc, wpc_shape, lvl.nbr125, need_bias=False)
        dP = ctx_taps_bwd(dc, lvl, lvl.nbr125.shape[0])
        dw_ctx, _ = ops.linear_wgrad(dP, cvec, need_bias=False)
        dcvec = ops.linear_dgrad(dP, w_ctx) if ctx.needs_input_grad[1] else None
        return None, dcvec, dw_pc, dw_ctx, dg, db, None, None, None, None


class PlainBlock(Block):
    """model.py:586-680; qk_norm False registers attn.q_norm / k_norm as nn.Identity (model.py:393-394): no state entries."""

    def __init__(self, c, h, mlp_ratio, qk_norm=True, coords=False, rpe_patch=None):
        super().__init__(c, h, mlp_ratio)
        if not qk_norm or coords or rpe_patch:
            self.attn = _Attn(c, h, qk_norm, coords, rpe_patch)


class PointTransformerV3Plain(PointTransformerV3CA):
    """PointTransformerV3 without PDNorm (model.py:864-1100) whose input is [pc | one context vector per cloud]: forward(data_dict)
    takes data_dict["feat"] = pc [N, c_pc <= 8] and data_dict["stem_context"] = [B, pdnorm_context_channels];
    in_channels = c_pc + pdnorm_context_channels is the width of embedding.stem.conv.weight, as in the reference."""
    plain_attention = True
    coord_attention = True
    dense_attention = True
    long_patches = True

    def __init__(self, in_channels=6, *args, **kw):
        super().__init__(in_channels, *args, **kw)
        self.in_channels = int(in_channels)
        self.pc_channels = self.in_channels - self.context_channels
        if self.pc_channels < 3:
            raise ValueError(f"SimplePolicyPTV3Concat: in_channels={self.in_channels} leaves {self.pc_channels} point columns beside "
                             f"the {self.context_channels} context channels (in_channels = columns of pc_fts + context_channels)")

    # -- construction
    @staticmethod
    def _pdnorm_unsupported(pdnorm_bn, pdnorm_ln, pdnorm_decouple, pdnorm_adaptive, pdnorm_affine, pdnorm_only_decoder):
        if (pdnorm_bn or pdnorm_ln) and pdnorm_adaptive:
            raise NotImplementedError("SimplePolicyPTV3Concat with pdnorm_adaptive=True: the Concat policy passes no context to the "
                                      "backbone (the reference asserts at PointTransformerV3/model.py:296); set pdnorm_bn = pdnorm_ln "
                                      "= pdnorm_adaptive = False")
        if pdnorm_bn or pdnorm_ln:
            raise NotImplementedError(f"SimplePolicyPTV3Concat with the non-adaptive PDNorm wrapper (pdnorm_bn={pdnorm_bn}, "
                                      f"pdnorm_ln={pdnorm_ln}) is not built: switch both off — the same arithmetic under other "
                                      "state_dict key names ('<site>.norm.*')")
        return {}

    @staticmethod
    def _context_width(ctx_channels, pdnorm_context_channels):
        return pdnorm_context_channels

    def _add_depth(self, stage, i, c, h, mlp_ratio):
        stage.add_module(f"block{i}", PlainBlock(c, h, mlp_ratio, self.qk_norm, self.add_coords, self.rpe_patch))

    def _index_sites(self):
        pass

    # -- the steps of a pass
    def _check_inputs(self, feat, counts, context):
        if feat.dtype != torch.float32:
            raise NotImplementedError("SimplePolicyPTV3Concat stores activations in fp32 only")
        if feat.shape[1] > MAX_PC_COLUMNS:
            raise NotImplementedError(f"pc_fts of {feat.shape[1]} columns: the thin-input stem convolution of SimplePolicyPTV3Concat "
                                      f"takes at most {MAX_PC_COLUMNS}")
        if feat.shape[1] != self.pc_channels:
            raise ValueError(f"SimplePolicyPTV3Concat: in_channels={self.in_channels} != {feat.shape[1]} columns of pc_fts + "
                             f"{self.context_channels} context_channels")

    def _begin(self, fw, data_dict, feat):
        """Top of a pass -> stem output: the context stem, then the join of the packed convolution weights."""
        cvec = data_dict.get("stem_context")
        B = len(fw.levels[0].counts)
        if cvec is None or cvec.dim() != 2 or tuple(cvec.shape) != (B, self.context_channels) or cvec.dtype != torch.float32:
            raise ValueError(f"PointTransformerV3Plain needs one fp32 context vector per cloud: stem_context [{B}, "
                             f"{self.context_channels}], got {None if cvec is None else (tuple(cvec.shape), cvec.dtype)}")
        st = self.embedding.stem
        w_pc, w_ctx = split_stem_weight(st.conv.weight, self.pc_channels)
        x = CtxStemFn.apply(feat, cvec.contiguous(), w_pc, w_ctx, st.norm.weight, st.norm.bias, st.norm.running_mean,
                            st.norm.running_var, fw.levels[0], fw.training)
        ops.sync_side_stream()  # the packed convolution weights
        fw.bank = None
        return x

    def _enter_stage(self, fw, lvl):
        pass

    def _run_depth(self, fw, stage, i, x, xs, lvl_o, lvl, si, dpath):
        blk = getattr(stage, f"block{i}")
        return blk.run(x, xs, lvl_o, fw.p, si, fw.pa, fw.packs[blk], dpath)[0]
