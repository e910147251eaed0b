"""Shared helpers of the regression action head's tests (pos_pred_type 'heatmap_mlp', rot_pred_type 'euler' / 'quat'): the
float64 restatement of the head and its losses (simple_policy_ptv3.py:83-103,117-157,322-368 — plain torch, differentiable),
the fixture case table of tests/golden/make_golden_reghead.py and the batch / label derivation.  No reference import here
(the GPU tests use this module too)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (policy, reference variant, base preset, pos_pred_type, rot_pred_type, dim_actions, temp, clouds, points, ragged,
#        data seed, weight seed, train, the reference's own forward)
CASES = {
    "reghead_tiny_mlp_euler_train": ("ca", "tiny", "tiny", "heatmap_mlp", "euler", 7, 0.1, 2, 512, False, 41, 51, True, False),
    "reghead_tiny_mlp_quat_train": ("ca", "tiny", "tiny", "heatmap_mlp", "quat", 8, 1.0, 2, 600, True, 45, 52, True, False),
    "reghead_adanorm_tiny_mlp_eulerdisc_train": ("adanorm", "tiny", "adanorm_tiny", "heatmap_mlp", "euler_disc", 7, 0.1, 2, 512,
                                                 False, 43, 53, True, False),
    "reghead_v1_disc_euler_eval": ("ca", "v1", "v1", "heatmap_disc", "euler", 7, 0.1, 2, 1024, True, 44, 54, False, True),
}
SELECT_MARGIN = 1e-3   # the two candidate losses of every stored min-selection differ by more than this
MIN_QUAT_NORM = 1e-2   # ... and no quaternion is normalised from a shorter vector


def head_overrides(pos, rot, dim_actions, temp):
    return ["action_config.pos_pred_type", pos, "action_config.rot_pred_type", rot, "action_config.dim_actions", str(dim_actions),
            "action_config.pos_heatmap_temp", str(temp)]


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    _, _, preset, pos, rot, da, temp = CASES[name][:7]
    base = lcfg.ADANORM_OVERRIDES[preset] if preset in lcfg.ADANORM_OVERRIDES else {"tiny": lcfg.TINY_OVERRIDES, "v1": lcfg.V1_OVERRIDES}[preset]
    return lcfg.load_model_config(None, base + head_overrides(pos, rot, da, temp))


def rot_labels(rot, B, seed):
    """Rotation labels that reach both branches of the closest-of-two selections: 'euler' targets near +-1 (the wrapped
    candidate wins whenever the prediction lies on the other side of 0) mixed with small ones, 'quat' unit quaternions."""
    rng = np.random.default_rng([seed, 0x52])
    if rot == "euler":
        near = rng.uniform(0.8, 0.98, size=(B, 3)) * rng.choice([-1.0, 1.0], size=(B, 3))
        small = rng.uniform(-0.4, 0.4, size=(B, 3))
        return np.where(rng.random((B, 3)) < 0.67, near, small).astype(np.float32)
    q = rng.standard_normal((B, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def case_batch(name):
    from robot_3dlotus_amd import synth
    import adanorm_util as au

    policy, _, _, _, rot, _, _, B, n, ragged, dseed = CASES[name][:11]
    batch = synth.synth_batch(B, n, ragged=ragged, seed=dseed)
    if rot != "euler_disc":
        gt = batch["gt_actions"]
        batch["gt_actions"] = torch.cat([gt[:, :3], torch.from_numpy(rot_labels(rot, B, dseed)), gt[:, -1:]], 1)
    return au.last_token_batch(batch) if policy == "adanorm" else batch


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))


# ------------------------------------------------------------------------------------------ float64 restatement
def softpos(e, coord, counts, temp):
    """xt [B, 3] = sum_i softmax_i(e_i0 / temp) (coord_i + e_i[1:4]) per cloud (simple_policy_ptv3.py:89-103)."""
    out = []
    for eb, cb in zip(torch.split(e, list(counts)), torch.split(coord, list(counts))):
        p = torch.softmax(eb[:, 0] / temp, 0)
        out.append((p[:, None] * (cb + eb[:, 1:4])).sum(0))
    return torch.stack(out, 0)


def _mlp(x, w0, b0, w3, b3):
    return F.linear(F.leaky_relu(F.linear(x, w0, b0), 0.02), w3, b3)


def head(feat, p, counts, coord, pos, rot, temp=1.0, euler_bins=72):
    """ActionHead.forward (reduce = max, no dropout).  p: {'hw0','hb0','hw3','hb3','aw0','ab0','aw3','ab3'}.
    -> (xt, xr, xo): xt [B, 3] ('heatmap_mlp') or logits [3, N, 2 pos_bins]; xr [B, 3] / normalised [B, 4] / [B, bins, 3]."""
    hm = _mlp(feat, p["hw0"], p["hb0"], p["hw3"], p["hb3"])
    xt = softpos(hm, coord, counts, temp) if pos == "heatmap_mlp" else hm.view(hm.shape[0], 3, -1).permute(1, 0, 2)
    pc = torch.stack([x.max(0)[0] for x in torch.split(feat, list(counts))], 0)
    ae = _mlp(pc, p["aw0"], p["ab0"], p["aw3"], p["ab3"])
    if rot == "quat":
        xr = ae[:, :4] / ae[:, :4].square().sum(-1, keepdim=True).sqrt()
    elif rot == "euler":
        xr = ae[:, :3]
    else:
        xr = ae[:, :euler_bins * 3].view(-1, euler_bins, 3)
    return xt, xr, ae[:, -1]


def rot_candidates(xr, tgt, rot):
    """The two candidate losses of the closest-of-two selection: per element ('euler') or per row ('quat')."""
    if rot == "euler":
        alt = torch.where(tgt < 0, tgt + 2, torch.where(tgt > 0, tgt - 2, tgt))
        return (xr - tgt) ** 2, (xr - alt) ** 2
    return ((xr - tgt) ** 2).mean(-1), ((xr + tgt) ** 2).mean(-1)


def losses(xt, xr, xo, gt, pos, rot, counts=None, disc_pos_probs=None, pos_w=1.0, rot_w=1.0):
    """compute_loss (simple_policy_ptv3.py:308-373) -> dict(pos, rot, open, total)."""
    tgt_rot, tgt_open = gt[:, 3:-1], gt[:, -1]
    if pos == "heatmap_mlp":
        lp = ((xt - gt[:, :3]) ** 2).mean()
    else:
        lp = 0
        for x, t in zip(torch.split(xt, list(counts), 1), disc_pos_probs):
            lp = lp + F.cross_entropy(x.reshape(3, -1), t.to(x.dtype))
        lp = lp / len(counts)
    if rot == "euler_disc":
        lr = F.cross_entropy(xr, tgt_rot.long())
    else:
        la, lb = rot_candidates(xr, tgt_rot, rot)
        sel = (la < lb).detach()      # strictly smaller keeps the target itself; a constant in backward
        lr = torch.where(sel, la, lb).mean()
    lo = F.binary_cross_entropy_with_logits(xo, tgt_open)
    return {"pos": lp, "rot": lr, "open": lo, "total": pos_w * lp + rot_w * lr + lo}

