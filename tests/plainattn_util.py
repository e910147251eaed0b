"""Shared helpers of the tests of attention without q/k LayerNorm (qk_norm False): the float64 restatement of the patch
attention with the norm optional, the inputs of the kernel tests, and the case table / batch / configuration of the fixtures
of tests/golden/make_golden_plainattn.py.  No reference import here (the GPU tests use this module too)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------ float64 restatement
def patch_attention(qkv, lvl, slot, H, qn=None, kn=None):
    """SerializedAttention's flash branch (PointTransformerV3/model.py:478-551) over the oracle's level tables, one patch at
    a time: rows qkv[order[slot][pad]] are cut at cu_seqlens, every patch attends to itself per head, and the result goes
    back through unpad[inverse[slot]].  qn / kn = (weight, bias) of q_norm / k_norm (LayerNorm over the head width,
    eps 1e-6), or None: q and k enter the scores as they are (nn.Identity, model.py:393-394).  Differentiable; computes in
    the dtype of qkv."""
    N, C3 = qkv.shape
    C = C3 // 3
    d = C // H
    rows = lvl["order_t"][slot][lvl["pad_t"]]
    back = lvl["unpad_t"][lvl["inverse_t"][slot]]
    x = qkv[rows]
    q, k, v = (x[:, i * C:(i + 1) * C].reshape(-1, H, d) for i in range(3))
    if qn is not None:
        q = F.layer_norm(q, (d,), qn[0], qn[1], 1e-6)
    if kn is not None:
        k = F.layer_norm(k, (d,), kn[0], kn[1], 1e-6)
    cu = [int(c) for c in lvl["cu_seqlens"]]
    out = []
    for a, b in zip(cu[:-1], cu[1:]):
        s = torch.einsum("qhd,khd->hqk", q[a:b], k[a:b]) * d ** -0.5
        p = torch.softmax(s, dim=-1)
        out.append(torch.einsum("hqk,khd->qhd", p, v[a:b]).reshape(b - a, C))
    return torch.cat(out, 0)[back]


def plain_inputs(C, n, seed):
    """qkv [n, 3C] with the q and k columns drawn as randn of scale 1.0 (logits of spread ~1, as normalised operands give) and
    the v columns and dout as test_gpu_edge_layouts._patch_inputs draws them (randn * 1.5, randn)."""
    g = torch.Generator().manual_seed(seed)
    qk = torch.randn(n, 2 * C, generator=g)
    v = torch.randn(n, C, generator=g) * 1.5
    dout = torch.randn(n, C, generator=g)
    return torch.cat([qk, v], 1).contiguous(), dout


# ------------------------------------------------------------------------------------------ fixtures
# name: (configuration, clouds, points, ragged, data seed, weight seed, train, the reference's own forward)
#   'tiny_plain': adanorm_tiny plus qk_norm False, published head (two stages: the head is called as forward does);
#   'yaml_dp0': simple_policy_ptv3.yaml with drop_path 0 (DropPath draws cannot be shared between implementations);
#   'yaml': the YAML untouched (drop_path 0.1 is the identity in eval mode)
CASES = {
    "plain_adanorm_tiny_train": ("tiny_plain", 2, 512, False, 61, 71, True, False),
    "plain_adanorm_yaml_train": ("yaml_dp0", 2, 1024, True, 62, 72, True, True),
    "plain_adanorm_yaml_eval": ("yaml", 2, 1024, True, 63, 72, False, True),
}


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    kind = CASES[name][0]
    if kind == "tiny_plain":
        return lcfg.preset("adanorm_tiny_plain")
    return lcfg.load_model_config(None, ["ptv3_config.drop_path", "0.0"] if kind == "yaml_dp0" else [])


def case_batch(name):
    """The synth batch of the case with one instruction token per cloud (txt_reduce 'mean'); the YAML cases keep 6 input
    channels (xyz, rgb) and take 'euler' labels that reach both branches of the closest-of-two selection."""
    from robot_3dlotus_amd import synth
    import adanorm_util as au
    import reghead_util as ru

    kind, B, n, ragged, dseed = CASES[name][:5]
    batch = au.last_token_batch(synth.synth_batch(B, n, ragged=ragged, seed=dseed))
    if kind != "tiny_plain":
        batch["pc_fts"] = batch["pc_fts"][:, :6].contiguous()
        gt = batch["gt_actions"]
        batch["gt_actions"] = torch.cat([gt[:, :3], torch.from_numpy(ru.rot_labels("euler", B, dseed)), gt[:, -1:]], 1)
    return batch


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
