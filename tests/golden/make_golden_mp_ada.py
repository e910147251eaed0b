"""Generate the fixtures of MotionPlannerPTV3AdaNorm from the *imported reference* (build container only).

    python tests/golden/make_golden_mp_ada.py [case ...]      # writes tests/golden/mp_ada_*.npz

The reference's MotionPlannerPTV3AdaNorm (genrobo3d/models/motion_planner_ptv3.py:151-397) is built through
tests/golden/ref_harness.py: for 'mp_ada_tiny_train' with the configuration of preset mp_ada_tiny, for the 'yaml' cases with the
MODEL section of motion_planner_ptv3.yaml itself (train: drop_path 0, since DropPath draws cannot be shared between
implementations; eval: untouched), always through the reference's own forward.  Dropouts are zeroed and the run is
single-threaded, so a fixture can be regenerated bit for bit.  The files hold DATA only, laid out as make_golden_plainattn.py
lays them out: seeds, sizes, the recorded shuffle permutations, the state_dict layout, the head outputs xt [B, T, 3] / xr / xo /
xstop, the five losses, gradient norms, leading entries, whole vectors and sketches (tests/adanorm_util.py), BatchNorm buffers
after a train step, the final actions of the eval case.
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
from weights_util import seeded_state_dict  # noqa: E402
import robot_3dlotus_amd  # noqa: E402,F401
import adanorm_util as au  # noqa: E402
import mp_ada_util as mu  # noqa: E402


def reference_planner(name):
    rh.install_shims()
    import einops  # noqa: F401
    from genrobo3d.models.motion_planner_ptv3 import MotionPlannerPTV3AdaNorm

    kind = mu.CASES[name][0]
    if kind == "tiny":
        cfg = rh.to_cfg(json.loads(json.dumps(mu.case_config(name))))   # (the reference adds the label channels into it in place)
    else:
        import yaml

        with open(f"{rh.REFERENCE_ROOT}/genrobo3d/configs/rlbench/motion_planner_ptv3.yaml") as f:
            cfg = rh.to_cfg(yaml.safe_load(f)["MODEL"])
        if kind == "yaml_dp0":
            cfg["ptv3_config"]["drop_path"] = 0.0
        assert cfg == mu.case_config(name), "preset mp_yaml is not the YAML's MODEL section"
    assert cfg["model_class"] == "MotionPlannerPTV3AdaNorm" and cfg["ptv3_config"]["qk_norm"] is False
    return MotionPlannerPTV3AdaNorm(cfg), cfg


def run_case(name, out_dir=HERE):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run_case(name, out_dir)
    finally:
        torch.set_num_threads(threads)


def _run_case(name, out_dir):
    kind, B, n, ragged, dseed, wseed, train = mu.CASES[name]
    torch.manual_seed(0)
    ref, cfg = reference_planner(name)
    sd = seeded_state_dict(ref.state_dict(), wseed, "scaled")
    ref.load_state_dict(sd, strict=True)
    zero_dropouts(ref)
    ref.train(train)
    batch = mu.case_batch(name)
    head = {}
    hh = ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2], xstop=o[3]))
    perms = []
    with rh.neutralise_half(), rh.record_randperm(perms):
        torch.manual_seed(100 + dseed)
        final, losses = ref(copy.deepcopy(batch), compute_loss=True, compute_final_action=not train)
    hh.remove()
    for p in ref.parameters():
        p.grad = None
    out = {"meta_kind": kind, "meta_B": B, "meta_n": n, "meta_ragged": ragged, "meta_dseed": dseed, "meta_wseed": wseed,
           "meta_train": train,
           "perms": torch.stack(perms).numpy().astype(np.int64),
           "npoints_in_batch": np.array(batch["npoints_in_batch"]),
           "gt_trajs": batch["gt_trajs"].numpy(),
           "input_checksum": np.float64(batch["pc_fts"].double().sum().item() + batch["pc_labels"].double().sum().item()),
           "weight_checksum": np.float64(sum(v.double().sum().item() for v in sd.values())),
           "state_layout": np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))}
    for k in ("xt", "xr", "xo", "xstop"):
        out[k] = head[k].detach().numpy()
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
    assert os.path.getsize(path) < 500_000, os.path.getsize(path)
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB  losses={ {k: round(float(v), 5) for k, v in losses.items()} }  "
          f"perms={out['perms'].tolist()}")
    return path


if __name__ == "__main__":
    for nme in sys.argv[1:] or list(mu.CASES):
        run_case(nme)
