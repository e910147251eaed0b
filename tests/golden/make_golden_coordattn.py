"""Generate the fixtures of add_coords_in_attn 'qk' / 'qkv' from the *imported reference* (build container only).

    python tests/golden/make_golden_coordattn.py [case ...]      # writes tests/golden/coord_*.npz

The reference's own SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat and MotionPlannerPTV3AdaNorm are built through
tests/golden/ref_harness.py with ptv3_config.add_coords_in_attn set (PointTransformerV3/model.py:396-398, 484-495): the tiny cases
with the configurations of make_golden_plainattn / make_golden_concat / make_golden_mp_ada (two stages: the policies' head is called
as forward does, the planner runs its own forward), the YAML case with the MODEL section of simple_policy_ptv3.yaml and that one
key flipped, in eval mode through the reference's own forward.  Dropouts are zeroed and the run is single-threaded, so a fixture
can be regenerated bit for bit.  The files hold DATA only, laid out as make_golden_plainattn.py / make_golden_mp_ada.py lay them
out: seeds, sizes, labels, the recorded shuffle permutations, the state_dict layout, the head outputs, losses, gradient norms,
leading entries, whole vectors and sketches (tests/adanorm_util.py), BatchNorm buffers after a train step, the final actions of
the eval case.
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
from weights_util import seeded_state_dict  # noqa: E402
import robot_3dlotus_amd  # noqa: E402,F401
import adanorm_util as au  # noqa: E402
import coordattn_util as cu  # noqa: E402


def reference_model(name):
    """-> (the reference's model of the case, its configuration)."""
    rh.install_shims()
    family, preset = cu.CASES[name][:2]
    mode = cu.case_mode(name)
    if family == "mp_ada":
        import einops  # noqa: F401
        from genrobo3d.models.motion_planner_ptv3 import MotionPlannerPTV3AdaNorm

        cfg = rh.to_cfg(json.loads(json.dumps(cu.case_config(name))))   # (the reference adds the label channels into it in place)
        assert cfg["model_class"] == "MotionPlannerPTV3AdaNorm" and cfg["ptv3_config"]["add_coords_in_attn"] == mode
        return MotionPlannerPTV3AdaNorm(cfg), cfg
    from genrobo3d.models.simple_policy_ptv3 import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat

    if preset == "adanorm_yaml_qk":
        cfg = reference_yaml_config()
        assert cfg["model_class"] == "SimplePolicyPTV3AdaNorm" and cfg["ptv3_config"]["add_coords_in_attn"] == "none"
    elif family == "adanorm":
        cfg = rh.reference_model_config("tiny")
        cfg["model_class"] = "SimplePolicyPTV3AdaNorm"
        cfg["ptv3_config"].update(PDNORM)
        cfg["ptv3_config"]["qk_norm"] = mode == "qkv"   # 'qk' on attention without q/k LayerNorm, 'qkv' with it
        cfg["action_config"]["txt_reduce"] = "mean"
    else:
        cfg = rh.reference_model_config("tinyctx")
        cfg["action_config"]["txt_reduce"] = "mean"
        cfg["model_class"] = "SimplePolicyPTV3Concat"
        cfg["ptv3_config"].update(NO_PDNORM)
        cfg["ptv3_config"]["in_channels"] = 7 + cfg["action_config"]["context_channels"]
    cfg["ptv3_config"]["add_coords_in_attn"] = mode
    ours = cu.case_config(name)
    assert ours.ptv3_config.qk_norm == cfg["ptv3_config"]["qk_norm"] and ours.ptv3_config.add_coords_in_attn == mode
    return (SimplePolicyPTV3AdaNorm if family == "adanorm" else SimplePolicyPTV3Concat)(cfg), cfg


def run_case(name, out_dir=HERE):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run_case(name, out_dir)
    finally:
        torch.set_num_threads(threads)


def _run_case(name, out_dir):
    family, preset, B, n, ragged, dseed, wseed, train, full = cu.CASES[name]
    planner = family == "mp_ada"
    torch.manual_seed(0)
    ref, cfg = reference_model(name)
    sd = seeded_state_dict(ref.state_dict(), wseed, "scaled")
    ref.load_state_dict(sd, strict=True)
    assert any("coords_proj" in k for k in sd)
    zero_dropouts(ref)
    ref.train(train)
    batch = cu.case_batch(name)
    head = {}
    if planner:
        hooks = [ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2], xstop=o[3]))]
    else:
        hooks = [ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2])),
                 ref.act_proj_head.action_mlp.register_forward_hook(lambda mod, i, o: head.update(ae=o))]
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
    labels = "gt_trajs" if planner else "gt_actions"
    checksum = batch["pc_fts"].double().sum().item() + (batch["pc_labels"].double().sum().item() if planner else 0.0)
    # (the case table holds the other settings: a zip member per scalar costs more than the state layout's extra keys leave room for)
    out = {"meta_wseed": wseed, "meta_train": train,
           "perms": torch.stack(perms).numpy().astype(np.int64),
           "npoints_in_batch": np.array(batch["npoints_in_batch"]),
           labels: batch[labels].numpy(),
           "input_checksum": np.float64(checksum),
           "weight_checksum": np.float64(sum(v.double().sum().item() for v in sd.values())),
           "state_layout": np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))}
    for k in ("xt", "xr", "xo") + (("xstop",) if planner else ()):
        out[k] = head[k].detach().numpy()
    if out["xt"].size > cu.XT_SAMPLE:  # heat-map logits [3, N, 2 pos_bins]: a fixed sample of them
        xt = out.pop("xt")
        out["xt_shape"] = np.array(xt.shape, np.int64)
        out["xt_absmax"] = np.float32(np.abs(xt).max())
        out["xt_sample"] = xt.reshape(-1)[cu.xt_sample_index(xt.size)]
    for k, v in losses.items():
        out["loss_" + k] = np.float32(v.item())
    if train:
        losses["total"].backward()
        named = list(ref.named_parameters())
        assert all(p.grad is not None for _, p in named), "a parameter of the reference got no gradient"
        assert all(float(p.grad.abs().max()) > 0 for nme, p in named if "coords_proj" in nme), "a coords_proj gradient is zero"
        out.update(au.pack_grads([(nme, p.grad.detach().numpy()) for nme, p in named]))
        for nme, b in ref.named_buffers():
            if "running" in nme:
                out["buf/" + nme] = b.detach().numpy()
    else:
        out["final_actions"] = final.detach().numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    peer = os.path.join(HERE, cu.SIZE_PEER[name] + ".npz")
    assert os.path.getsize(path) <= os.path.getsize(peer), (os.path.getsize(path), os.path.getsize(peer))
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB  losses={ {k: round(float(v), 5) for k, v in losses.items()} }  "
          f"perms={out['perms'].tolist()}")
    return path


if __name__ == "__main__":
    for nme in sys.argv[1:] or list(cu.CASES):
        run_case(nme)
