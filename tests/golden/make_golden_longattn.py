"""Generate the fixtures of patch sizes above 128 from the *imported reference* (build container only).

    python tests/golden/make_golden_longattn.py [case ...]      # writes tests/golden/long_*.npz

The reference's own SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat and MotionPlannerPTV3AdaNorm are built through
tests/golden/ref_harness.py with every entry of ptv3_config.enc_patch_size / dec_patch_size at 256 (the tiny cases, with the
configurations of make_golden_plainattn / make_golden_concat / make_golden_mp_ada: two stages, the policies' head is called as
forward does, the planner runs its own forward) or at 1024 (the MODEL section of simple_policy_ptv3.yaml, in eval mode through the
reference's own forward); SerializedAttention.forward, PointTransformerV3/model.py:529-551.  Dropouts are zeroed and the run is
single-threaded, so a fixture can be regenerated bit for bit.  The files hold DATA only, laid out as make_golden_rpe.py lays them
out, plus the tile lengths of every level, `level_tiles`.

A case is stored only if it is worth storing (asserted here, on the CPU): at level 0 a cloud is longer than the patch size and its
tail patch borrows rows, a cloud of some level holds between 129 and patch size - 1 points (one tile longer than 128 rows), and —
in the five-stage YAML case — a deeper level has tiles of at most 128 rows only, so both kernel routes run in one model.  (The
tiny networks have two stages, and the second level of a synth cloud keeps about nine points in ten of the first: a cloud longer
than 256 points cannot fall under 129 there.  Their level 1 runs on the long kernels too.)
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import ref_harness as rh  # noqa: E402
from make_golden import zero_dropouts  # noqa: E402
from make_golden_adanorm import PDNORM  # noqa: E402
from make_golden_concat import NO_PDNORM  # noqa: E402
from make_golden_plainattn import reference_yaml_config  # noqa: E402
from make_golden_reghead import check_selections, reference_step  # noqa: E402
import robot_3dlotus_amd  # noqa: E402,F401
import adanorm_util as au  # noqa: E402
import longattn_util as lu  # noqa: E402
from weights_util import seeded_state_dict  # noqa: E402


def reference_model(name):
    """-> (the reference's model of the case, its configuration)."""
    rh.install_shims()
    family, preset = lu.CASES[name][:2]
    K = lu.case_patch(name)
    ours = lu.case_config(name)
    if family == "mp_ada":
        import einops  # noqa: F401
        from genrobo3d.models.motion_planner_ptv3 import MotionPlannerPTV3AdaNorm

        cfg = rh.to_cfg(json.loads(json.dumps(ours)))   # (the reference adds the label channels into it in place)
        assert cfg["model_class"] == "MotionPlannerPTV3AdaNorm"
    else:
        from genrobo3d.models.simple_policy_ptv3 import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat

        if preset == "adanorm_yaml_p1024":
            cfg = reference_yaml_config()
            assert cfg["model_class"] == "SimplePolicyPTV3AdaNorm"
        elif family == "adanorm":
            cfg = rh.reference_model_config("tiny")
            cfg["model_class"] = "SimplePolicyPTV3AdaNorm"
            cfg["ptv3_config"].update(PDNORM)
            cfg["ptv3_config"]["qk_norm"] = "plain" not in preset
            cfg["action_config"]["txt_reduce"] = "mean"
        else:
            cfg = rh.reference_model_config("tinyctx")
            cfg["action_config"]["txt_reduce"] = "mean"
            cfg["model_class"] = "SimplePolicyPTV3Concat"
            cfg["ptv3_config"].update(NO_PDNORM)
            cfg["ptv3_config"]["in_channels"] = 7 + cfg["action_config"]["context_channels"]
        cfg["ptv3_config"]["enc_patch_size"] = [K] * len(cfg["ptv3_config"]["enc_depths"])
        cfg["ptv3_config"]["dec_patch_size"] = [K] * len(cfg["ptv3_config"]["dec_depths"])
    p3 = cfg["ptv3_config"]
    assert list(p3["enc_patch_size"]) + list(p3["dec_patch_size"]) == [K] * (len(p3["enc_depths"]) + len(p3["dec_depths"]))
    assert list(ours.ptv3_config.enc_patch_size) == list(p3["enc_patch_size"]) and ours.ptv3_config.qk_norm == p3["qk_norm"]
    assert p3["enable_flash"] is True and p3["enable_rpe"] is False
    if family == "mp_ada":
        return MotionPlannerPTV3AdaNorm(cfg), cfg
    return (SimplePolicyPTV3AdaNorm if family == "adanorm" else SimplePolicyPTV3Concat)(cfg), cfg


def run_case(name, out_dir=HERE):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run_case(name, out_dir)
    finally:
        torch.set_num_threads(threads)


def worth_storing(facts, K):
    """The conditions of the module docstring -> list of what is missing."""
    missing = []
    if not (any(c > K for c in facts[0]["counts"]) and facts[0]["borrowed"] > 0):
        missing.append("no cloud of level 0 is longer than the patch size with a borrowing tail patch")
    if not any(128 < c < K for f in facts for c in f["counts"]):
        missing.append("no cloud holds between 129 and patch size - 1 points")
    if len(facts) > 2 and not any(max(f["tile_lens"]) <= 128 for f in facts[1:]):
        missing.append("no deeper level has tiles of at most 128 rows only")
    return missing


def _run_case(name, out_dir):
    family, preset, B, n, ragged, dseed, wseed, train, full = lu.CASES[name]
    planner = family == "mp_ada"
    K = lu.case_patch(name)
    torch.manual_seed(0)
    ref, cfg = reference_model(name)
    sd = seeded_state_dict(ref.state_dict(), wseed, "scaled")
    ref.load_state_dict(sd, strict=True)
    zero_dropouts(ref)
    ref.train(train)
    batch = lu.case_batch(name)
    head = {}
    if planner:
        hooks = [ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2], xstop=o[3]))]
    else:
        hooks = [ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2])),
                 ref.act_proj_head.action_mlp.register_forward_hook(lambda mod, i, o: head.update(ae=o))]
    for mname, mod in ref.named_modules():   # every SerializedAttention of the reference is configured at K
        if type(mod).__name__ == "SerializedAttention":
            assert int(mod.patch_size) == K, (mname, mod.patch_size)
    perms = []
    with rh.neutralise_half(), rh.record_randperm(perms):
        torch.manual_seed(100 + dseed)
        if planner:
            final, losses = ref(copy.deepcopy(batch), compute_loss=True, compute_final_action=not train)
        else:
            final, losses = reference_step(ref, cfg, copy.deepcopy(batch), full, decode=not train)
    for h in hooks:
        h.remove()
    if not planner:
        check_selections(name, cfg["action_config"]["rot_pred_type"], head["ae"], head["xr"], batch["gt_actions"])
    for p in ref.parameters():
        p.grad = None
    # ---- is the case worth storing?
    n_levels = len(cfg["ptv3_config"]["enc_depths"])
    facts = lu.level_facts(batch, n_levels, [p.tolist() for p in perms], K)
    missing = worth_storing(facts, K)
    assert not missing, (missing, facts)
    labels = "gt_trajs" if planner else "gt_actions"
    checksum = batch["pc_fts"].double().sum().item() + (batch["pc_labels"].double().sum().item() if planner else 0.0)
    tl = [f["tile_lens"] for f in facts]
    level_tiles = np.full((len(tl), max(len(t) for t in tl)), -1, np.int64)
    for i, t in enumerate(tl):
        level_tiles[i, :len(t)] = t
    out = {"meta_wseed": wseed, "meta_train": train,
           "perms": torch.stack(perms).numpy().astype(np.int64),
           "npoints_in_batch": np.array(batch["npoints_in_batch"]),
           "level_tiles": level_tiles,
           labels: batch[labels].numpy(),
           "input_checksum": np.float64(checksum),
           "weight_checksum": np.float64(sum(v.double().sum().item() for v in sd.values())),
           "state_layout": np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))}
    for k in ("xt", "xr", "xo") + (("xstop",) if planner else ()):
        out[k] = head[k].detach().numpy()
    if out["xt"].size > lu.XT_SAMPLE:  # heat-map logits [3, N, 2 pos_bins]: a fixed sample of them
        xt = out.pop("xt")
        out["xt_shape"] = np.array(xt.shape, np.int64)
        out["xt_absmax"] = np.float32(np.abs(xt).max())
        out["xt_sample"] = xt.reshape(-1)[lu.xt_sample_index(xt.size)]
    for k, v in losses.items():
        out["loss_" + k] = np.float32(v.item())
    if train:
        losses["total"].backward()
        named = list(ref.named_parameters())
        assert all(p.grad is not None for _, p in named), "a parameter of the reference got no gradient"
        out.update(au.pack_grads([(nme, p.grad.detach().numpy()) for nme, p in named]))
        for nme, b in ref.named_buffers():
            if "running" in nme:
                out["buf/" + nme] = b.detach().numpy()
    else:
        out["final_actions"] = final.detach().numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    peer = os.path.join(HERE, lu.SIZE_PEER[name] + ".npz")
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB (peer {os.path.getsize(peer) / 1e6:.2f})  "
          f"losses={ {k: round(float(v), 5) for k, v in losses.items()} }  perms={out['perms'].tolist()}  facts={facts}")
    assert os.path.getsize(path) <= 1.1 * os.path.getsize(peer) and os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    return path


if __name__ == "__main__":
    for nme in sys.argv[1:] or list(lu.CASES):
        run_case(nme)
