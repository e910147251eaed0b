"""Generate the fixtures of the regression action head from the *imported reference* (build container only).

    python tests/golden/make_golden_reghead.py [case ...]      # writes tests/golden/reghead_*.npz

The reference's SimplePolicyPTV3CA / SimplePolicyPTV3AdaNorm are built through tests/golden/ref_harness.py with the configuration
of `reference_model_config(variant)` plus the head options of tests/reghead_util.CASES (pos_pred_type, rot_pred_type, dim_actions,
pos_heatmap_temp).  Two-stage variants cannot run the reference's own forward (simple_policy_ptv3.py:243 indexes five stages):
their head is called as forward does (:238-244), with the CONFIGURED temperature.  Dropouts are zeroed and the run is
single-threaded, so a fixture can be regenerated bit for bit.  The files hold DATA only: seeds, sizes, the labels, the recorded
shuffle permutations, the state_dict layout, xt / xr / xo, losses, gradient norms, leading entries, whole vectors and sketches
(tests/adanorm_util.py), BatchNorm buffers after a train step, the final actions of an eval case.

The closest-of-two selections of the rotation losses are discrete routing: a case is stored only if the two candidate losses of
every element ('euler') or row ('quat') differ by more than reghead_util.SELECT_MARGIN, both branches occur, and no quaternion is
normalised from a vector shorter than MIN_QUAT_NORM (conditions of the fixture: the seeds are chosen so that they hold).
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
from weights_util import seeded_state_dict  # noqa: E402
import robot_3dlotus_amd  # noqa: E402,F401
import adanorm_util as au  # noqa: E402
from adanorm_util import pack_grads  # noqa: E402
import reghead_util as ru  # noqa: E402


def reference_policy(name):
    rh.install_shims()
    from genrobo3d.models.simple_policy_ptv3 import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA

    policy, variant, _, pos, rot, da, temp = ru.CASES[name][:7]
    cfg = rh.reference_model_config(variant)
    cfg["action_config"].update(pos_pred_type=pos, rot_pred_type=rot, dim_actions=da, pos_heatmap_temp=temp)
    if policy == "adanorm":
        cfg["model_class"] = "SimplePolicyPTV3AdaNorm"
        cfg["ptv3_config"].update(PDNORM)
        cfg["action_config"]["txt_reduce"] = "mean"
        return SimplePolicyPTV3AdaNorm(cfg), cfg
    return SimplePolicyPTV3CA(cfg), cfg


def reference_step(ref, cfg, batch, full, decode):
    """-> (final actions | None, losses); the head's outputs are taken by a forward hook."""
    if full:
        return ref(batch, compute_loss=True, compute_final_action=decode)
    batch = ref.prepare_batch(batch)
    outs = ref.ptv3_model(ref.prepare_ptv3_batch(batch), return_dec_layers=True)
    pred = ref.act_proj_head(outs[-1].feat, batch["npoints_in_batch"], coords=outs[-1].coord,
                             temp=cfg["action_config"].get("pos_heatmap_temp", 1), gt_pos=batch["gt_actions"][..., :3],
                             dec_layers_embed=None)
    return None, ref.compute_loss(pred, batch["gt_actions"], disc_pos_probs=batch.get("disc_pos_probs"),
                                  npoints_in_batch=batch["npoints_in_batch"])


def check_selections(name, rot, ae, xr, gt):
    """The conditions of the fixture (module docstring), on the reference's own fp32 head outputs."""
    if rot == "euler_disc":
        return
    la, lb = ru.rot_candidates(xr.detach(), gt[:, 3:-1], rot)
    gap = float((la - lb).abs().min())
    assert gap > ru.SELECT_MARGIN, f"{name}: candidate losses within {gap:.2e}: choose another seed"
    sel = la < lb
    assert bool(sel.any()) and bool((~sel).any()), f"{name}: one branch of the selection only: choose another seed"
    if rot == "quat":
        nrm = float(ae[:, :4].detach().norm(dim=1).min())
        assert nrm > ru.MIN_QUAT_NORM, f"{name}: quaternion normalised from a vector of length {nrm:.2e}"


def run_case(name, out_dir=HERE):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run_case(name, out_dir)
    finally:
        torch.set_num_threads(threads)


def _run_case(name, out_dir):
    policy, variant, _, pos, rot, da, temp, B, n, ragged, dseed, wseed, train, full = ru.CASES[name]
    torch.manual_seed(0)
    ref, cfg = reference_policy(name)
    sd = seeded_state_dict(ref.state_dict(), wseed, "scaled")
    ref.load_state_dict(sd, strict=True)
    zero_dropouts(ref)
    ref.train(train)
    batch = ru.case_batch(name)
    head = {}
    hh = ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2]))
    ha = ref.act_proj_head.action_mlp.register_forward_hook(lambda mod, i, o: head.update(ae=o))
    perms = []
    with rh.neutralise_half(), rh.record_randperm(perms):
        torch.manual_seed(100 + dseed)
        final, losses = reference_step(ref, cfg, copy.deepcopy(batch), full, decode=not train)
    hh.remove(); ha.remove()
    check_selections(name, rot, head["ae"], head["xr"], batch["gt_actions"])
    for p in ref.parameters():
        p.grad = None
    out = {"meta_policy": policy, "meta_variant": variant, "meta_pos": pos, "meta_rot": rot, "meta_dim_actions": da, "meta_temp": temp,
           "meta_B": B, "meta_n": n, "meta_ragged": ragged, "meta_dseed": dseed, "meta_wseed": wseed, "meta_train": train,
           "perms": torch.stack(perms).numpy().astype(np.int64),
           "npoints_in_batch": np.array(batch["npoints_in_batch"]),
           "gt_actions": batch["gt_actions"].numpy(),
           "input_checksum": np.float64(batch["pc_fts"].double().sum().item()),
           "weight_checksum": np.float64(sum(v.double().sum().item() for v in sd.values())),
           "state_layout": np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))}
    for k in ("xt", "xr", "xo"):
        out[k] = head[k].detach().numpy()
    if out["xt"].size > au.XT_SAMPLE:  # heat-map logits [3, N, 2 pos_bins]: a fixed sample of them
        xt = out.pop("xt")
        out["xt_shape"] = np.array(xt.shape, np.int64)
        out["xt_absmax"] = np.float32(np.abs(xt).max())
        out["xt_sample"] = xt.reshape(-1)[au.xt_sample_index(xt.size)]
    for k, v in losses.items():
        out["loss_" + k] = np.float32(v.item())
    if train:
        losses["total"].backward()
        out.update(pack_grads([(nme, p.grad.detach().numpy()) for nme, p in ref.named_parameters()]))
        for nme, b in ref.named_buffers():
            if "running" in nme:
                out["buf/" + nme] = b.detach().numpy()
    else:
        out["final_actions"] = final.detach().numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB  losses={ {k: round(float(v), 5) for k, v in losses.items()} }  "
          f"perms={out['perms'].tolist()}")
    return path


if __name__ == "__main__":
    for nme in sys.argv[1:] or list(ru.CASES):
        run_case(nme)
