"""Shared helpers of the MotionPlannerPTV3AdaNorm tests: the case table, configuration and batch of the fixtures of
tests/golden/make_golden_mp_ada.py.  No reference import here (the GPU tests use this module too)."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (configuration, clouds, points, ragged, data seed, weight seed, train)
#   'tiny': preset mp_ada_tiny (two stages, 4 input columns, pose context);
#   'yaml_dp0': the MODEL section of motion_planner_ptv3.yaml with drop_path 0 (DropPath draws cannot be shared between
#               implementations); 6 input columns, hence the two-group stem;
#   'yaml': the YAML untouched (drop_path 0.1 is the identity in eval mode)
CASES = {
    "mp_ada_tiny_train": ("tiny", 2, 512, True, 81, 91, True),
    "mp_ada_yaml_train": ("yaml_dp0", 2, 512, False, 82, 92, True),
    "mp_ada_yaml_eval": ("yaml", 2, 512, False, 83, 92, False),
}


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    kind = CASES[name][0]
    cfg = lcfg.preset("mp_ada_tiny" if kind == "tiny" else "mp_yaml")
    if kind == "yaml_dp0":
        cfg.ptv3_config.drop_path = 0.0
    return cfg


def mp_batch(B, n, ragged, seed, columns):
    """synth.synth_batch_mp with one instruction token per cloud (txt_reduce 'mean'), float masks, and `columns` point-feature
    columns: xyz, height and, beyond 4, colour-like columns in [0, 1) from a generator of their own."""
    from robot_3dlotus_amd import synth
    import adanorm_util as au

    batch = au.last_token_batch(synth.synth_batch_mp(B, n, ragged=ragged, seed=seed))
    del batch["gt_trajs_disc_pos_probs"]
    if columns > 4:
        extra = np.random.default_rng([seed, 0xC0]).random((batch["pc_fts"].shape[0], columns - 4)).astype(np.float32)
        batch["pc_fts"] = torch.cat([batch["pc_fts"], torch.from_numpy(extra)], 1).contiguous()
    batch["traj_masks"] = batch["traj_masks"].float()
    return batch


def case_batch(name):
    kind, B, n, ragged, dseed = CASES[name][:5]
    return mp_batch(B, n, ragged, dseed, 4 if kind == "tiny" else 6)


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
