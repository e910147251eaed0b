"""Generate the fixtures of enable_flash False / enable_rpe True from the *imported reference* (build container only).

    python tests/golden/make_golden_rpe.py [case ...]      # writes tests/golden/rpe_*.npz

The reference's own SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat and MotionPlannerPTV3AdaNorm are built through
tests/golden/ref_harness.py with ptv3_config.enable_flash False (the non-flash branch of SerializedAttention,
PointTransformerV3/model.py:469-472, :499-527: every level is patched at min(patch size, fewest points of a cloud)) and, but for
the `dense` case, enable_rpe True (:307-326): the tiny cases with the configurations of make_golden_plainattn /
make_golden_concat / make_golden_mp_ada (two stages: the policies' head is called as forward does, the planner runs its own
forward), the YAML case with the MODEL section of simple_policy_ptv3.yaml and those two keys flipped, in eval mode through the
reference's own forward.  Dropouts are zeroed and the run is single-threaded, so a fixture can be regenerated bit for bit.  The
files hold DATA only, laid out as make_golden_coordattn.py lays them out, plus the per-level patch sizes `level_K`.

A case is stored only if it is worth storing (asserted here, on the CPU): a level runs at K = 128 and a level below it, a cloud
borrows rows at a level of either kind, the clamp of the relative offsets is hit on both sides at level 0, and every rpe_table
gradient has a norm above the fixture's gradient floor.
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
import rpe_util as ru  # noqa: E402


def reference_model(name):
    """-> (the reference's model of the case, its configuration)."""
    rh.install_shims()
    family, preset = ru.CASES[name][:2]
    rpe = ru.case_has_rpe(name)
    ours = ru.case_config(name)
    if family == "mp_ada":
        import einops  # noqa: F401
        from genrobo3d.models.motion_planner_ptv3 import MotionPlannerPTV3AdaNorm

        cfg = rh.to_cfg(json.loads(json.dumps(ours)))   # (the reference adds the label channels into it in place)
        assert cfg["model_class"] == "MotionPlannerPTV3AdaNorm"
        assert cfg["ptv3_config"]["enable_flash"] is False and cfg["ptv3_config"]["enable_rpe"] is rpe
        return MotionPlannerPTV3AdaNorm(cfg), cfg
    from genrobo3d.models.simple_policy_ptv3 import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat

    if preset == "adanorm_yaml_rpe":
        cfg = reference_yaml_config()
        assert cfg["model_class"] == "SimplePolicyPTV3AdaNorm" and cfg["ptv3_config"]["enable_flash"] is True
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
    cfg["ptv3_config"]["enable_flash"] = False
    cfg["ptv3_config"]["enable_rpe"] = rpe
    assert ours.ptv3_config.qk_norm == cfg["ptv3_config"]["qk_norm"]
    assert ours.ptv3_config.enable_flash is False and ours.ptv3_config.enable_rpe is rpe
    return (SimplePolicyPTV3AdaNorm if family == "adanorm" else SimplePolicyPTV3Concat)(cfg), cfg


def run_case(name, out_dir=HERE):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run_case(name, out_dir)
    finally:
        torch.set_num_threads(threads)


def _run_case(name, out_dir):
    family, preset, B, n, ragged, dseed, wseed, train, full = ru.CASES[name]
    planner = family == "mp_ada"
    rpe = ru.case_has_rpe(name)
    torch.manual_seed(0)
    ref, cfg = reference_model(name)
    sd = ru.case_state_dict(ref.state_dict(), wseed, boost=train)
    ref.load_state_dict(sd, strict=True)
    tables = [k for k in sd if k.endswith("rpe.rpe_table")]
    assert bool(tables) == rpe and all(tuple(sd[k].shape)[0] == 93 for k in tables)
    zero_dropouts(ref)
    ref.train(train)
    batch = ru.case_batch(name)
    head = {}
    if planner:
        hooks = [ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2], xstop=o[3]))]
    else:
        hooks = [ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2])),
                 ref.act_proj_head.action_mlp.register_forward_hook(lambda mod, i, o: head.update(ae=o))]
    # the patch size every SerializedAttention ran at (it sets self.patch_size per forward, model.py:469-472), per level
    stage_K = {}
    for mname, mod in ref.named_modules():
        if type(mod).__name__ == "SerializedAttention":
            hooks.append(mod.register_forward_hook(
                lambda mod, i, o, mname=mname: stage_K.setdefault((i[0].feat.shape[0]), set()).add(int(mod.patch_size))))
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
    facts = ru.level_facts(batch, n_levels, [p.tolist() for p in perms])
    level_K = [f["K"] for f in facts]
    by_n = {sum(f["counts"]): f["K"] for f in facts}
    assert all(stage_K[nrows] == {by_n[nrows]} for nrows in stage_K), (stage_K, by_n)   # the reference ran at the restated sizes
    assert any(k == 128 for k in level_K) and any(k < 128 for k in level_K), level_K
    assert any(f["borrowed"] > 0 for f in facts if f["K"] == 128) and any(f["borrowed"] > 0 for f in facts if f["K"] < 128), facts
    assert facts[0]["clamp_both"], "the clamp is not hit on both sides at level 0"
    labels = "gt_trajs" if planner else "gt_actions"
    checksum = batch["pc_fts"].double().sum().item() + (batch["pc_labels"].double().sum().item() if planner else 0.0)
    out = {"meta_wseed": wseed, "meta_train": train,
           "perms": torch.stack(perms).numpy().astype(np.int64),
           "npoints_in_batch": np.array(batch["npoints_in_batch"]),
           "level_K": np.array(level_K, np.int64),
           labels: batch[labels].numpy(),
           "input_checksum": np.float64(checksum),
           "weight_checksum": np.float64(sum(v.double().sum().item() for v in sd.values())),
           "state_layout": np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))}
    for k in ("xt", "xr", "xo") + (("xstop",) if planner else ()):
        out[k] = head[k].detach().numpy()
    if out["xt"].size > ru.XT_SAMPLE:  # heat-map logits [3, N, 2 pos_bins]: a fixed sample of them
        xt = out.pop("xt")
        out["xt_shape"] = np.array(xt.shape, np.int64)
        out["xt_absmax"] = np.float32(np.abs(xt).max())
        out["xt_sample"] = xt.reshape(-1)[ru.xt_sample_index(xt.size)]
    for k, v in losses.items():
        out["loss_" + k] = np.float32(v.item())
    if train:
        losses["total"].backward()
        named = list(ref.named_parameters())
        assert all(p.grad is not None for _, p in named), "a parameter of the reference got no gradient"
        gmax = max(float(p.grad.double().norm()) for _, p in named)
        for nme, p in named:
            if nme.endswith("rpe.rpe_table"):
                print(f"    {nme}: |g| {float(p.grad.double().norm()):.3e}  of the largest {gmax:.3e}")
                assert float(p.grad.double().norm()) > ru.GRAD_FLOOR * gmax, ("an rpe_table gradient under the floor", nme)
        out.update(au.pack_grads([(nme, p.grad.detach().numpy()) for nme, p in named]))
        for nme, b in ref.named_buffers():
            if "running" in nme:
                out["buf/" + nme] = b.detach().numpy()
    else:
        out["final_actions"] = final.detach().numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    peer = os.path.join(HERE, ru.SIZE_PEER[name] + ".npz")
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB (peer {os.path.getsize(peer) / 1e6:.2f})  "
          f"losses={ {k: round(float(v), 5) for k, v in losses.items()} }  perms={out['perms'].tolist()}  facts={facts}")
    assert os.path.getsize(path) <= 1.1 * os.path.getsize(peer) and os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    return path


if __name__ == "__main__":
    for nme in sys.argv[1:] or list(ru.CASES):
        run_case(nme)
