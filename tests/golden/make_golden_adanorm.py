"""Generate the SimplePolicyPTV3AdaNorm fixtures from the *imported reference* (build container only).

    python tests/golden/make_golden_adanorm.py [case ...]      # writes tests/golden/adanorm_*.npz

The reference's SimplePolicyPTV3AdaNorm (simple_policy_ptv3.py:160-373) is built through tests/golden/ref_harness.py with the
configuration of `reference_model_config(variant)` plus model_class and the PDNorm switches of simple_policy_ptv3.yaml
(pdnorm_bn / pdnorm_ln / pdnorm_adaptive True, decouple False).  Dropouts are zeroed and the run is single-threaded, as in
make_golden.run_case, so a fixture can be regenerated bit for bit.  The files hold DATA only: seeds, sizes, the recorded
shuffle permutations, the state_dict layout, losses, logits (a fixed sample of the position logits in train mode), gradient norms and leading entries, whole vector gradients and
sketches of the matrices (tests/adanorm_util.py) and the BatchNorm buffers after a train step.
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

PDNORM = dict(pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=True, pdnorm_decouple=False, pdnorm_affine=True,
              pdnorm_only_decoder=False)


def reference_adanorm(variant, reduce):
    rh.install_shims()
    from genrobo3d.models.simple_policy_ptv3 import SimplePolicyPTV3AdaNorm

    cfg = rh.reference_model_config(variant)
    cfg["model_class"] = "SimplePolicyPTV3AdaNorm"
    cfg["ptv3_config"].update(PDNORM)
    cfg["action_config"]["txt_reduce"] = reduce
    return SimplePolicyPTV3AdaNorm(cfg)


def run_case(name, out_dir=HERE):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _run_case(name, out_dir)
    finally:
        torch.set_num_threads(threads)


def _run_case(name, out_dir):
    variant, _, reduce, B, n, ragged, dseed, wseed, train, full = au.CASES[name]
    torch.manual_seed(0)
    ref = reference_adanorm(variant, reduce)
    sd = seeded_state_dict(ref.state_dict(), wseed, "scaled")
    ref.load_state_dict(sd, strict=True)
    zero_dropouts(ref)
    ref.train(train)
    batch = au.case_batch(name)
    head = {}
    hh = ref.act_proj_head.register_forward_hook(lambda mod, i, o: head.update(xt=o[0], xr=o[1], xo=o[2]))
    perms = []
    with rh.neutralise_half(), rh.record_randperm(perms):
        torch.manual_seed(100 + dseed)
        losses = rh.reference_forward(ref, copy.deepcopy(batch), full=full)
    hh.remove()
    for p in ref.parameters():
        p.grad = None
    out = {"meta_variant": variant, "meta_B": B, "meta_n": n, "meta_ragged": ragged, "meta_dseed": dseed, "meta_wseed": wseed,
           "meta_train": train, "meta_reduce": reduce,
           "perms": torch.stack(perms).numpy().astype(np.int64),
           "npoints_in_batch": np.array(batch["npoints_in_batch"]),
           "input_checksum": np.float64(batch["pc_fts"].double().sum().item()),
           "weight_checksum": np.float64(sum(v.double().sum().item() for v in sd.values())),
           "state_layout": np.array(json.dumps([[k, list(v.shape)] for k, v in ref.state_dict().items()]))}
    for k in ("xt", "xr", "xo"):
        out[k] = head[k].detach().numpy()
    if train:  # the [3, N, 2 pos_bins] position logits: a fixed sample of them (eval-mode fixtures keep every one)
        xt = out.pop("xt")
        out["xt_shape"] = np.array(xt.shape, np.int64)
        out["xt_absmax"] = np.float32(np.abs(xt).max())
        out["xt_sample"] = xt.reshape(-1)[au.xt_sample_index(xt.size)]
    for k, v in losses.items():
        out["loss_" + k] = np.float32(v.item())
    if train:
        losses["total"].backward()
        out.update(au.pack_grads([(nme, p.grad.detach().numpy()) for nme, p in ref.named_parameters()]))
        for nme, b in ref.named_buffers():
            if "running" in nme:
                out["buf/" + nme] = b.detach().numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1e6:.2f} MB  losses={ {k: round(float(v), 5) for k, v in losses.items()} }  "
          f"perms={out['perms'].tolist()}")
    return path


if __name__ == "__main__":
    for nme in sys.argv[1:] or list(au.CASES):
        run_case(nme)
