"""MotionPlannerPTV3CA — the 3D-LOTUS++ motion planner (BASELINE configs[3]) on the lotus-hip kernels; drop-in for
`genrobo3d/models/motion_planner_ptv3.py:400-463` (+ forward / compute_loss of its base class, :222-397).

Same backbone as the policy (68 input channels: xyz + height + a 64-d embedding of the 4 point labels), a trajectory
head that scores `max_traj_len` future steps at once, and five losses (pos, rot, open, stop, total) masked by the
per-sample trajectory length.  Module surface kept: `cls(config.MODEL)`, `forward(batch, compute_loss=False,
**kwargs)` -> `final_pred_actions [B, T, 3+4+2]` or `(final_pred_actions, losses)`, kwarg `compute_final_action`,
the reference's state_dict keys (incl. the unused `txt_attn_fc` the CA variant builds for txt_reduce == 'attn').

What runs where: every matrix product over points, the sparse convolutions, attention, norms, the per-cloud max and the
heatmap cross entropy are lotus-hip kernels (ops.*Fn); the [B, T]-sized rotation / openness / stop losses, the
trajectory-embedding bias (5 x 64 floats) and the effective stem weight (see prepare_ptv3_batch) are a few ATen
launches on small tensors.

MotionPlannerPTV3AdaNorm (:151-397, the class motion_planner_ptv3.yaml names) is the same planner on the adaptive-PDNorm
backbone with the soft trajectory head (pos_pred_type 'heatmap_mlp'): see the class.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .config import to_cfg
from .policy import BaseModel, RobotPoseEmbedding, _PTV3_KEYS
from .ptv3 import PointTransformerV3CA


class TrajectoryActionHead(nn.Module):
    """Parameter layout of motion_planner_ptv3.py:20-75 for (max, heatmap_disc, euler_disc) and, with `soft_pos` (set by
    MotionPlannerPTV3AdaNorm only), for (max, heatmap_mlp, euler_disc): heatmap_mlp.3 then has 1 + 3 outputs (:55-62)."""

    def __init__(self, reduce, pos_pred_type, rot_pred_type, hidden_size, dim_actions, max_traj_len, dropout=0,
                 voxel_size=0.01, euler_resolution=5, ptv3_config=None, pos_bins=50, traj_embed_size=64, soft_pos=False):
        super().__init__()
        if not soft_pos:
            if (reduce, pos_pred_type, rot_pred_type) != ("max", "heatmap_disc", "euler_disc"):
                raise NotImplementedError("lotus-hip builds the published head: reduce=max, heatmap_disc, euler_disc")
        else:
            if reduce != "max":
                raise NotImplementedError(f"reduce={reduce!r}: lotus-hip builds the trajectory head with reduce='max' only")
            if pos_pred_type not in ("heatmap_disc", "heatmap_mlp"):
                raise NotImplementedError(f"pos_pred_type={pos_pred_type!r}: lotus-hip builds the trajectory head with "
                                          "'heatmap_mlp' (MotionPlannerPTV3AdaNorm) and 'heatmap_disc'")
            if rot_pred_type != "euler_disc":
                raise NotImplementedError(f"rot_pred_type={rot_pred_type!r}: lotus-hip builds the trajectory head with 'euler_disc' only")
        if traj_embed_size <= 0:
            raise NotImplementedError("traj_embed_size == 0 (single-step head) is the SimplePolicy head; use that")
        self.pos_pred_type = pos_pred_type
        self.euler_resolution, self.euler_bins, self.pos_bins = euler_resolution, 360 // euler_resolution, pos_bins
        self.max_traj_len, self.hidden_size, self.dropout = max_traj_len, hidden_size, float(dropout)
        self.traj_embedding = nn.Embedding(max_traj_len, traj_embed_size)
        self.heatmap_mlp = nn.Sequential(nn.Linear(hidden_size + traj_embed_size, hidden_size), nn.LeakyReLU(0.02),
                                         nn.Dropout(dropout),
                                         nn.Linear(hidden_size, 3 * pos_bins * 2 if pos_pred_type == "heatmap_disc" else 4))
        self.action_mlp = nn.Sequential(nn.Linear(hidden_size + traj_embed_size, hidden_size), nn.LeakyReLU(0.02),
                                        nn.Dropout(dropout), nn.Linear(hidden_size, self.euler_bins * 3 + 1 + 1))


class _Prefetched:
    """What prefetch() built ahead of forward(): entries (pc_fts, pc_labels, built), matched by the identity of the batch's two
    tensors.  At most two are kept (the batch about to run and the one after it); a consumed entry is forgotten."""

    def __init__(self):
        self.entries = []

    def remember(self, batch, built):
        self.entries = (self.entries + [(batch["pc_fts"], batch["pc_labels"], built)])[-2:]

    def take(self, batch):
        """-> what remember() was given for this very batch, or None."""
        hit = next((q for q in self.entries if q[0] is batch["pc_fts"] and q[1] is batch["pc_labels"]), None)
        self.entries = [q for q in self.entries if q is not hit][-1:]  # (at most one more: the batch after this one)
        return None if hit is None else hit[2]


class MotionPlannerPTV3CA(BaseModel):
    def __init__(self, config):
        super().__init__()
        self._pre = _Prefetched()
        config = to_cfg(config)
        self.config = config
        act = config.action_config
        p3 = {k: v for k, v in config.ptv3_config.items() if k in _PTV3_KEYS}
        # the reference adds pc_label_channels into config.ptv3_config.in_channels in place
        # (motion_planner_ptv3.py:405-408); the caller's config is left untouched here
        p3["in_channels"] = config.ptv3_config.in_channels + act.pc_label_channels
        self.ptv3_model = self._make_backbone(p3, act)
        self.pc_label_embedding = nn.Embedding(4, act.pc_label_channels)   # 0 obstacle, 1 robot, 2 object, 3 target
        self.txt_fc = nn.Linear(act.txt_ft_size, act.context_channels)
        if act.txt_reduce == "attn":
            self.txt_attn_fc = nn.Linear(act.txt_ft_size, 1)               # built, never used by the CA variant
        if act.use_ee_pose:
            self.pose_embedding = RobotPoseEmbedding(act.context_channels)   # one extra context token per cloud (:421-422)
        self.act_proj_head = TrajectoryActionHead(
            act.reduce, act.pos_pred_type, act.rot_pred_type, config.ptv3_config.dec_channels[0], act.dim_actions,
            act.max_traj_len, dropout=act.dropout, voxel_size=act.voxel_size, pos_bins=act.pos_bins,
            traj_embed_size=act.traj_embed_size, soft_pos=self.soft_pos)
        self.apply(self._init_weights)

    soft_pos = False  # the trajectory head's 'heatmap_mlp' option: MotionPlannerPTV3AdaNorm only

    def _make_backbone(self, p3, act):
        return PointTransformerV3CA(**p3)

    def prepare_ptv3_batch(self, batch):
        """motion_planner_ptv3.py:433-463: feat = [pc_fts | label embedding], context = txt_fc(txt_embeds)."""
        # The 64 embedding channels take only 4 distinct values per point, and the stem convolution is linear:
        #   conv(W, [pc | E[label]]) == conv([W_pc | W_emb E^T], [pc | onehot(label)])
        # so the 68-channel 5^3 convolution (81 % of whose gathered rows are absent neighbours) becomes the 8-channel
        # stem the policy already has a kernel for, with an effective weight that autograd differentiates back into
        # the stem weight and the embedding table (two products of a few hundred kFLOP); no input gradient is needed.
        W, E = self.ptv3_model.embedding.stem.conv.weight, self.pc_label_embedding.weight
        c_pc = batch["pc_fts"].shape[1]
        w_eff = torch.cat([W[..., :c_pc], torch.matmul(W[..., c_pc:], E.t())], -1)                  # [64,5,5,5,c_pc+4]
        feat = self._pre.take(batch)   # prefetch() built it (and started the front-end on exactly this tensor)
        feat = self._point_input(batch) if feat is None else feat
        txt, extra = batch["txt_embeds"].contiguous(), {}
        if getattr(self, "act_storage", None) == "bf16":
            # bf16 activation storage (as SimplePolicyPTV3CA.prepare_ptv3_batch): the network inputs are rounded once here;
            # the integer front end keeps reading the fp32 coordinates — the first three columns of the fp32 `feat`
            extra["coord_src"] = feat
            txt, feat_in = txt.to(torch.bfloat16), feat.to(torch.bfloat16)
        else:
            feat_in = feat
        ctx = ops.LinearFn.apply(txt, self.txt_fc.weight, self.txt_fc.bias)
        ctx_counts = list(batch["txt_lens"])
        if self.config.action_config.use_ee_pose:   # motion_planner_ptv3.py:451-457
            ctx, ctx_counts = self.append_context_tokens(ctx, ctx_counts, [self.pose_embedding(batch["ee_poses"].float())])
        return {"coord": feat[:, :3], "grid_size": self.config.action_config.voxel_size, "offset": batch["offset"],
                "feat": feat_in, "stem_weight": w_eff.contiguous(), "context": ctx, "counts": list(batch["npoints_in_batch"]),
                "context_counts": ctx_counts, **extra}

    @staticmethod
    def _point_input(batch):
        """-> [pc | one-hot label] [N, c_pc + 4] fp32."""
        return torch.cat([batch["pc_fts"].float(), F.one_hot(batch["pc_labels"].long(), 4).float()], -1)

    @torch.no_grad()
    def prefetch(self, batch):
        """Input-pipeline hook, as SimplePolicyPTV3CA.prefetch: build the network input of `batch` ([pc | one-hot label]) and
        start its integer front-end on the side stream; the following forward(batch) must get the same (device) batch."""
        batch = self.prepare_batch(batch)
        feat = self._point_input(batch)
        self._pre.remember(batch, feat)
        self.ptv3_model.prefetch({"coord": feat[:, :3], "grid_size": self.config.action_config.voxel_size, "offset": batch["offset"],
                                  "feat": feat, "counts": list(batch["npoints_in_batch"]),
                                  "context_counts": [c + int(bool(self.config.action_config.use_ee_pose)) for c in batch["txt_lens"]]})

    gemm_precision = None  # as SimplePolicyPTV3CA.gemm_precision
    act_storage = None     # None / 'fp32' | 'bf16': as SimplePolicyPTV3CA.act_storage (bf16 activations in HBM, fp32 masters)

    def forward(self, batch, compute_loss=False, **kwargs):
        if self.act_storage == "bf16":
            with ops.storage(torch.bfloat16):
                return self._forward(batch, compute_loss, **kwargs)
        with ops.precision(self.gemm_precision):
            return self._forward(batch, compute_loss, **kwargs)

    def _forward(self, batch, compute_loss=False, **kwargs):
        """The planner's one forward; what differs between the heat-map head and the soft head ('heatmap_mlp',
        MotionPlannerPTV3AdaNorm) are its three steps _positions, _pos_loss_term and _final_positions."""
        batch = self.prepare_batch(batch)
        dev = self.hip_device(batch)
        head = self.act_proj_head
        d = self.prepare_ptv3_batch(batch)
        last = self.ptv3_model(d, return_dec_layers=True)[-1]
        x, lvl = last.feat, last.level
        B, T, C = len(lvl.counts), head.max_traj_len, head.hidden_size
        eb = head.euler_bins
        p = head.dropout if self.training else 0.0
        hm, am = head.heatmap_mlp, head.action_mlp
        te = head.traj_embedding.weight                                         # [T, E]

        # heatmap branch, motion_planner_ptv3.py:88-97,113-114.  Linear([x | te_t]) = x Wx^T + (te_t Wt^T + b): the
        # point-feature product is shared by all T steps and the step only shifts the bias.
        base = ops.LinearFn.apply(x, hm[0].weight[:, :C].contiguous(), None)                       # [N, C]
        step_bias = F.linear(te, hm[0].weight[:, C:], hm[0].bias)                                  # [T, C]
        pos = self._positions(base, step_bias.contiguous(), hm[3], d, lvl, p, ops.mix_seed(self.ptv3_model.last_seed, 2000))
        # action branch, :116-120,139-146: max over points commutes with the concatenated step embedding
        pc = ops.CloudMaxFn.apply(x, lvl)                                                         # [B, C]
        pcs = torch.cat([pc.unsqueeze(1).expand(-1, T, -1), te.to(pc.dtype).unsqueeze(0).expand(B, -1, -1)], -1).reshape(B * T, -1)
        a = F.dropout(F.leaky_relu(ops.LinearFn.apply(pcs, am[0].weight, am[0].bias), 0.02), p, self.training)
        ae = ops.LinearFn.apply(a, am[3].weight, am[3].bias).view(B, T, -1)
        pred_rot = ae[..., :eb * 3].reshape(B, T, eb, 3)
        pred_open, pred_stop = ae[..., -2], ae[..., -1]
        self.last_pred = (pos, pred_rot, pred_open, pred_stop)

        losses = self._traj_losses(pos, ae, batch, lvl) if compute_loss else None
        decode = kwargs.get("compute_final_action", True)
        if compute_loss and self.training and not decode and not kwargs.get("decode_actions", False):
            return None, losses                                  # trainer discards the actions (see policy.py)
        final_pos = self._final_positions(pos, batch, lvl, decode)
        quat = self.decode_euler_disc(pred_rot.reshape(B * T, eb, 3), head.euler_resolution, dev).reshape(B, T, 4)
        final = torch.cat([final_pos, quat, pred_open.detach().unsqueeze(-1), pred_stop.detach().unsqueeze(-1)], -1)
        return (final, losses) if compute_loss else final

    def _positions(self, base, step_bias, out, d, lvl, p, seed):
        """-> last_pred[0]: the T heat maps xts[t] [N, 3*nb] (reference layout: pred_pos()); out = heatmap_mlp.3, d = the backbone's input."""
        return list(ops.StepHeadFn.apply(base, step_bias, out.weight, out.bias, p, seed))

    def _final_positions(self, xts, batch, lvl, decode):
        """:238-267, best_disc_pos == 'max'; one launch pair per step instead of B*T host round trips."""
        if not decode:
            return batch["gt_trajs"][..., :3].float()
        act, nb = self.config.action_config, 2 * self.act_proj_head.pos_bins
        pcf = batch["pc_fts"] if batch["pc_fts"].stride(1) == 1 else batch["pc_fts"].contiguous()
        best = act.get("best_disc_pos", "max")
        pos = torch.stack([self.decode_disc_pos(best, xt.detach(), pcf, batch["npoints_in_batch"], lvl, nb, act.pos_bin_size)
                           for xt in xts], 1)
        return pos.float()                                       # reference: .float() at :266

    def pred_pos(self):
        """Last forward's position logits in the reference layout (T, 3, N, 2*pos_bins)."""
        nb = 2 * self.act_proj_head.pos_bins
        return torch.stack([xt.view(-1, 3, nb).permute(1, 0, 2) for xt in self.last_pred[0]], 0)

    def compute_loss(self, xts, pred_rot, pred_open, pred_stop, batch, lvl):
        """motion_planner_ptv3.py:307-397 (heatmap_disc / euler_disc), reference argument list."""
        B, T = pred_rot.shape[:2]
        ae = torch.cat([pred_rot.reshape(B, T, -1), pred_open.unsqueeze(-1), pred_stop.unsqueeze(-1)], -1)
        return self._traj_losses(xts, ae, batch, lvl)

    def _traj_losses(self, pos, ae, batch, lvl):
        """pos = last_pred[0]; ae [B, T, euler_bins * 3 + 2]: rotation logits (bin, axis) at bin * 3 + axis | openness | stop."""
        B, T = ae.shape[:2]
        gt = batch["gt_trajs"].float()
        m = batch["traj_masks"].float()                                                  # [B, T]
        node, term = self._pos_loss_term(pos, batch, lvl, T)
        # the position term's masked mean (:327-336), masked rotation CE, openness and stop BCE (:338-383): one launch for the
        # lot (the same arithmetic as ~40 small ATen kernels cost 2 ms per step)
        lc = self.config.loss_config
        L = node.apply(ae.reshape(B * T, -1), term.reshape(B * T, 3), gt.reshape(B * T, -1).contiguous(),
                       batch["gt_trajs_stop"].float().reshape(-1).contiguous(), m.reshape(B, T).contiguous(),
                       (ae.shape[-1] - 2) // 3, lc.pos_weight, lc.rot_weight)
        return {"pos": L[0], "rot": L[1], "open": L[2], "stop": L[3], "total": L[4]}

    def _pos_loss_term(self, xts, batch, lvl, T):
        """-> (the loss node, its position input [B, T, 3]): ops.TrajLossFn over the heat-map cross entropies per (cloud, step,
        axis) — sum_tc CE * mask / (3 * sum_t mask) per cloud, mean over clouds."""
        dev = xts[0].device
        dp = batch["gt_trajs_disc_pos_probs"]
        # per step t the targets in the layout the CE kernel reads: cloud-major, [3][n_b * nb] per cloud
        if isinstance(dp, torch.Tensor):
            tgts = dp.float().to(dev)                                                    # pre-packed [T, sum 3*n_b*nb]
        else:
            tgts = torch.cat([d.to(dev).float().reshape(T, -1) for d in dp], 1)
        tgts = tgts.contiguous()
        return ops.TrajLossFn, torch.stack([ops.PosCEFn.apply(xts[t], tgts[t], lvl) for t in range(T)], 1)


class MotionPlannerPTV3AdaNorm(MotionPlannerPTV3CA):
    """motion_planner_ptv3.py:151-397, the model class of genrobo3d/configs/rlbench/motion_planner_ptv3.yaml: the instruction
    (+ pose) enters the point backbone through adaptive PDNorm (adanorm.PointTransformerV3AdaNorm), one context vector per
    cloud, and the trajectory head predicts soft positions (pos_pred_type 'heatmap_mlp': ops.TrajSoftPosFn, ops.TrajRegLossFn)
    or the published heat maps ('heatmap_disc').  Forward contract, kwargs and `last_pred` are MotionPlannerPTV3CA's; with
    'heatmap_mlp' last_pred[0] is xt [B, T, 3] and the final position is xt whatever compute_final_action says (:243).
    fp32 activation storage; data parallel through parallel.GradReducer + SyncBatchNorm statistics like the AdaNorm policy."""
    soft_pos = True

    def _make_backbone(self, p3, act):
        from .adanorm import PointTransformerV3AdaNorm

        p3.setdefault("pdnorm_only_decoder", False)  # (motion_planner_ptv3.py:157-160)
        p3["pdnorm_context_channels"] = act.context_channels
        if act.txt_reduce not in ("mean", "attn"):
            raise NotImplementedError(f"txt_reduce={act.txt_reduce!r}: MotionPlannerPTV3AdaNorm builds 'mean' and 'attn'")
        return PointTransformerV3AdaNorm(**p3)

    @staticmethod
    def _point_input(batch):
        """-> (pc [N, c_pc] fp32 contiguous, one-hot label [N, 4]): the two column groups, never concatenated."""
        return batch["pc_fts"].float().contiguous(), F.one_hot(batch["pc_labels"].long(), 4).float()

    def prepare_ptv3_batch(self, batch):
        """motion_planner_ptv3.py:190-222: feat = [pc_fts | label embedding], context = one vector per cloud (txt_fc reduced by
        'mean' — one token per cloud — or 'attn', plus the pose embedding).  The stem convolution is linear in its input
        columns, so its two column groups are convolved separately (adanorm.StemGroupsFn): the point features with
        W[..., :c_pc], the one-hot label with W[..., c_pc:] E^T (the embedding folded into the weight as MotionPlannerPTV3CA
        does); autograd carries both weight gradients back into stem.conv.weight and the embedding table."""
        from .adanorm import cloud_context

        act = self.config.action_config
        pc, onehot = self._pre.take(batch) or self._point_input(batch)   # (prefetch() may have built them already)
        c_pc = pc.shape[1]
        if c_pc > 8:
            raise NotImplementedError(f"MotionPlannerPTV3AdaNorm: pc_fts with {c_pc} > 8 columns (the thin-input stem convolution "
                                      "takes at most 8 per column group)")
        W, E = self.ptv3_model.embedding.stem.conv.weight, self.pc_label_embedding.weight
        if W.shape[-1] != c_pc + E.shape[1]:
            raise ValueError(f"pc_fts has {c_pc} columns, ptv3_config.in_channels is {W.shape[-1] - E.shape[1]}")
        w_pc, w_lab = W[..., :c_pc].contiguous(), torch.matmul(W[..., c_pc:], E.t()).contiguous()
        txt = batch["txt_embeds"].contiguous()
        lens = [int(v) for v in batch["txt_lens"]]
        if act.txt_reduce == "mean" and any(n != 1 for n in lens):
            raise ValueError(f"txt_reduce='mean' takes one instruction token per cloud (instr_embed_type='last'); txt_lens={lens}")
        ctx = ops.LinearFn.apply(txt, self.txt_fc.weight, self.txt_fc.bias)
        if act.txt_reduce == "attn":
            ctx = cloud_context(ctx, ops.LinearFn.apply(txt, self.txt_attn_fc.weight, self.txt_attn_fc.bias), lens)
        if act.use_ee_pose:
            ctx = ctx + self.pose_embedding(batch["ee_poses"].float())
        B = len(batch["npoints_in_batch"])
        return {"coord": pc[:, :3], "grid_size": act.voxel_size, "offset": batch["offset"], "feat": pc,
                "stem_groups": (pc, onehot, w_pc, w_lab), "context": ctx.contiguous(),
                "counts": list(batch["npoints_in_batch"]), "context_counts": [1] * B}

    @torch.no_grad()
    def prefetch(self, batch):
        """Input-pipeline hook, as MotionPlannerPTV3CA.prefetch: build the network input of `batch` and start its integer
        front-end on the side stream; the following forward(batch) must get the same (device) batch."""
        batch = self.prepare_batch(batch)
        pc, onehot = self._point_input(batch)
        self._pre.remember(batch, (pc, onehot))
        self.ptv3_model.prefetch({"coord": pc[:, :3], "grid_size": self.config.action_config.voxel_size, "offset": batch["offset"],
                                  "feat": pc, "counts": list(batch["npoints_in_batch"]),
                                  "context_counts": [1] * len(batch["npoints_in_batch"])})

    def forward(self, batch, compute_loss=False, **kwargs):
        if self.act_storage == "bf16":
            raise NotImplementedError("MotionPlannerPTV3AdaNorm: act_storage='bf16' is not built (fp32 activations only)")
        if not self.ptv3_model.qk_norm:
            mode = self.gemm_precision or ops.get_gemm_precision()
            if mode != "fp32":  # the patch attention without q/k LayerNorm exists as exact-fp32 kernels only
                raise NotImplementedError(f"MotionPlannerPTV3AdaNorm with qk_norm=False is built for gemm_precision None / 'fp32' "
                                          f"only, got {mode!r}")
        if self.ptv3_model.enable_rpe:
            mode = self.gemm_precision or ops.get_gemm_precision()
            if mode != "fp32":  # the patch attention with the relative-position term exists as exact-fp32 kernels only
                raise NotImplementedError(f"MotionPlannerPTV3AdaNorm with enable_rpe=True is built for gemm_precision None / 'fp32' "
                                          f"only, got {mode!r}")
        if self.ptv3_model.patch_size > 128:
            mode = self.gemm_precision or ops.get_gemm_precision()
            if mode != "fp32":  # the patch attention above 128 rows per patch exists as exact-fp32 kernels only
                raise NotImplementedError(f"MotionPlannerPTV3AdaNorm with patch sizes above 128 is built for gemm_precision None / 'fp32' "
                                          f"only, got {mode!r}")
        return super().forward(batch, compute_loss, **kwargs)

    @property
    def _soft(self):
        return self.act_proj_head.pos_pred_type == "heatmap_mlp"

    def _positions(self, base, step_bias, out, d, lvl, p, seed):
        """'heatmap_mlp', motion_planner_ptv3.py:89-109 -> xt [B, T, 3]: the T hidden layers, the 4-column product, the per-cloud
        softmax and the weighted coordinates are one pass over `base`."""
        if not self._soft:
            return super()._positions(base, step_bias, out, d, lvl, p, seed)
        temp = float(self.config.action_config.get("pos_heatmap_temp", 1))
        return ops.TrajSoftPosFn.apply(base, step_bias, out.weight, out.bias, d["feat"], lvl, temp, p, seed)

    def _pos_loss_term(self, xt, batch, lvl, T):
        """'heatmap_mlp': ops.TrajRegLossFn, the masked MSE of xt with one global normalisation (:338-397)."""
        return (ops.TrajRegLossFn, xt) if self._soft else super()._pos_loss_term(xt, batch, lvl, T)

    def _final_positions(self, xt, batch, lvl, decode):
        """:243,276-294: the continuous position is final as it is (the float64 quaternions promote the whole action)."""
        return xt.detach() if self._soft else super()._final_positions(xt, batch, lvl, decode)

    def pred_pos(self):
        """Last forward's position: xt [B, T, 3] ('heatmap_mlp'), or the logits in the reference layout ('heatmap_disc')."""
        return self.last_pred[0] if self._soft else super().pred_pos()
