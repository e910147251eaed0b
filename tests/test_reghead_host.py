"""Host-side checks of the regression action head (pos_pred_type 'heatmap_mlp', rot_pred_type 'euler' / 'quat'): parameter
layout against the reference-derived fixtures, refused options, presets and YAML round trip, the synthetic label layouts, the
dataset's continuous rotation targets; where the reference tree exists (build container) the float64 restatement of
tests/reghead_util.py against the live reference head and losses, and the regeneration of a fixture."""
import json
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import config as lcfg, dataset as ds, synth
from robot_3dlotus_amd.policy import MODEL_FACTORY, ActionHead, SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA

import golden_util as gu
import reghead_util as ru

HAVE_REF = os.path.isdir("/root/reference/genrobo3d")
HERE = os.path.dirname(os.path.abspath(__file__))
COMBOS = [(p, r) for p in ("heatmap_disc", "heatmap_mlp") for r in ("euler_disc", "euler", "quat")]


def _layout(name):
    return {k: tuple(s) for k, s in json.loads(str(ru.load(name)["state_layout"]))}


def _tiny(pos, rot, da):
    return SimplePolicyPTV3CA(lcfg.load_model_config(None, lcfg.TINY_OVERRIDES + ru.head_overrides(pos, rot, da, 0.1)))


@pytest.mark.parametrize("case", list(ru.CASES))
def test_state_dict_matches_the_reference_layout(case):
    cls = {"ca": SimplePolicyPTV3CA, "adanorm": SimplePolicyPTV3AdaNorm}[ru.CASES[case][0]]
    sd = cls(ru.case_config(case)).state_dict()
    want = _layout(case)
    assert list(sd) == list(want) and all(tuple(sd[k].shape) == want[k] for k in want)


@pytest.mark.parametrize("pos,rot", COMBOS)
def test_six_combinations_build_the_reference_head(pos, rot):
    """The head's last layers per option, taken from the fixture of the reference that has the option; everything else is the
    tiny policy's layout."""
    da = 8 if rot == "quat" else 7
    sd = {k: tuple(v.shape) for k, v in _tiny(pos, rot, da).state_dict().items()}
    tiny = _layout("reghead_tiny_mlp_euler_train")
    assert set(sd) == set(tiny)
    hm, am = "act_proj_head.heatmap_mlp.3.", "act_proj_head.action_mlp.3."
    assert all(sd[k] == tiny[k] for k in tiny if not k.startswith((hm, am)))
    if pos == "heatmap_mlp":
        assert sd[hm + "weight"] == tiny[hm + "weight"] == (4, 64) and sd[hm + "bias"] == (4,)
    else:
        v1 = _layout("reghead_v1_disc_euler_eval")
        assert sd[hm + "weight"] == (v1[hm + "weight"][0], 64) == (90, 64) and sd[hm + "bias"] == v1[hm + "bias"]
    src = {"euler": "reghead_tiny_mlp_euler_train", "quat": "reghead_tiny_mlp_quat_train",
           "euler_disc": "reghead_adanorm_tiny_mlp_eulerdisc_train"}[rot]
    assert sd[am + "weight"] == _layout(src)[am + "weight"] == ({"euler": 4, "quat": 5, "euler_disc": 217}[rot], 64)
    assert sd[am + "bias"] == _layout(src)[am + "bias"]


def test_unused_column_exists_at_dim_actions_8_with_euler():
    """simple_policy_ptv3.yaml: dim_actions 8 with rot_pred_type 'euler' -> action_mlp.3 has 5 outputs, xo is the last."""
    sd = _tiny("heatmap_mlp", "euler", 8).state_dict()
    assert sd["act_proj_head.action_mlp.3.weight"].shape == (5, 64) and sd["act_proj_head.action_mlp.3.bias"].shape == (5,)
    y = lcfg.load_model_config(None)
    assert (y.action_config.pos_pred_type, y.action_config.rot_pred_type, y.action_config.dim_actions) == ("heatmap_mlp", "euler", 8)
    assert ActionHead("max", "heatmap_mlp", "euler", 64, 8).action_mlp[3].out_features == 5


@pytest.mark.parametrize("key,value", [("pos_pred_type", v) for v in ("heatmap_mlp3", "heatmap_mlp_topk", "heatmap_mlp_clf", "heatmap_normmax")]
                         + [("rot_pred_type", v) for v in ("rot6d", "euler_delta")]
                         + [("reduce", v) for v in ("mean", "attn", "multiscale_max", "multiscale_max_large")])
def test_refused_options_name_themselves(key, value):
    for base in ("tiny", "adanorm_tiny"):
        cfg = lcfg.preset(base)
        cfg.action_config[key] = value
        with pytest.raises(NotImplementedError, match=f"{key}='{value}'"):
            MODEL_FACTORY[cfg.model_class](cfg)


def test_quaternion_needs_its_own_columns():
    with pytest.raises(ValueError, match="dim_actions"):
        _tiny("heatmap_mlp", "quat", 7)


def test_motion_planner_head_stays_refused():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3CA

    cfg = lcfg.preset("mp_tiny")
    cfg.action_config.pos_pred_type = "heatmap_mlp"
    with pytest.raises(NotImplementedError):
        MotionPlannerPTV3CA(cfg)


@pytest.mark.parametrize("cls,base", [(SimplePolicyPTV3CA, "tiny_reg"), (SimplePolicyPTV3AdaNorm, "adanorm_tiny_reg")])
def test_bf16_storage_raises_with_a_new_head_option(cls, base):
    m = cls(lcfg.preset(base))
    m.act_storage = "bf16"
    with pytest.raises(NotImplementedError, match="act_storage"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


@pytest.mark.parametrize("name,base", [("tiny_reg", "tiny"), ("v1_reg", "v1"), ("adanorm_tiny_reg", "adanorm_tiny")])
def test_reg_presets_factory_and_yaml_round_trip(name, base, tmp_path):
    import yaml

    cfg, b = lcfg.preset(name), lcfg.preset(base)
    a = cfg.action_config
    assert (a.pos_pred_type, a.rot_pred_type, a.dim_actions) == ("heatmap_mlp", "euler", 7)
    b.action_config.update(pos_pred_type="heatmap_mlp", rot_pred_type="euler")
    assert json.loads(json.dumps(cfg)) == json.loads(json.dumps(b))       # the base preset plus the two switches, nothing else
    path = tmp_path / (name + ".yaml")
    path.write_text(yaml.safe_dump({"MODEL": json.loads(json.dumps(cfg))}))
    loaded = lcfg.load_model_config(str(path))
    m = MODEL_FACTORY[loaded.model_class](loaded)
    assert type(m).__name__ == cfg.model_class
    sd = m.state_dict()
    assert sd["act_proj_head.heatmap_mlp.3.weight"].shape[0] == 4 and sd["act_proj_head.action_mlp.3.weight"].shape[0] == 4
    m2 = MODEL_FACTORY[cfg.model_class](lcfg.preset(name))
    m2.load_state_dict(sd, strict=True)
    assert m2.num_parameters == m.num_parameters


def test_existing_presets_are_unchanged():
    for name in ("v1", "tiny", "peract", "tinydeep", "tinyctx", "adanorm_v1", "adanorm_tiny", "adanorm_tinyctx"):
        a = lcfg.preset(name).action_config
        assert (a.pos_pred_type, a.rot_pred_type, a.reduce) == ("heatmap_disc", "euler_disc", "max"), name


def test_synth_batch_default_is_unchanged_and_new_layouts():
    fx = dict(np.load(os.path.join(gu.GOLDEN_DIR, "v1_scaled_train.npz")))
    args = (int(fx["meta_B"]), int(fx["meta_n"]))
    kw = dict(ragged=bool(fx["meta_ragged"]), seed=int(fx["meta_dseed"]))
    base = synth.synth_batch(*args, **kw)
    assert abs(base["pc_fts"].double().sum().item() - float(fx["input_checksum"])) < 1e-9
    assert base["npoints_in_batch"] == fx["npoints_in_batch"].tolist()
    same = synth.synth_batch(*args, rot_type="euler_disc", **kw)
    B = args[0]
    for rot, width in (("euler", 7), ("quat", 8)):
        b = synth.synth_batch(*args, rot_type=rot, **kw)
        assert b["gt_actions"].shape == (B, width) and b["gt_actions"].dtype == torch.float32
        r = b["gt_actions"][:, 3:-1]
        if rot == "euler":
            assert (r.abs() < 1).all()
        else:
            assert torch.allclose(r.norm(dim=1), torch.ones(B), atol=1e-6)
        assert torch.equal(b["gt_actions"][:, :3], base["gt_actions"][:, :3]) and torch.equal(b["gt_actions"][:, -1], base["gt_actions"][:, -1])
        for other in (same, b):   # every other field is the default batch, bit for bit
            for k, v in base.items():
                if k == "gt_actions" and other is b:
                    continue
                if isinstance(v, torch.Tensor):
                    assert torch.equal(v, other[k]), k
                elif k == "disc_pos_probs":
                    assert all(torch.equal(x, y) for x, y in zip(v, other[k]))
                else:
                    assert v == other[k], k
    with pytest.raises(ValueError, match="rot_type"):
        synth.synth_batch(1, 64, rot_type="rot6d")


def test_fixture_labels_reach_both_branches():
    """Conditions the generator asserts on the reference's outputs, re-checked on the stored data."""
    for case, spec in ru.CASES.items():
        rot = spec[4]
        if rot == "euler_disc":
            continue
        fx = ru.load(case)
        assert np.array_equal(ru.case_batch(case)["gt_actions"].numpy(), fx["gt_actions"])
        la, lb = ru.rot_candidates(torch.from_numpy(fx["xr"]), torch.from_numpy(fx["gt_actions"])[:, 3:-1], rot)
        assert float((la - lb).abs().min()) > ru.SELECT_MARGIN and bool((la < lb).any()) and bool((la >= lb).any()), case
        assert os.path.getsize(os.path.join(ru.GOLDEN_DIR, case + ".npz")) < 1 << 20


# ------------------------------------------------------------------------------------ dataset
def _fixture_store(fx, tmp_path):
    taskvar = str(fx["taskvar"])
    root = tmp_path / "eps" / taskvar
    root.mkdir(parents=True)
    for k in fx.files:
        if k.startswith("rec/"):
            (root / (k[4:] + ".msgpack")).write_bytes(fx[k].tobytes())
    (tmp_path / "instr.json").write_text(str(fx["instrs"]))
    np.save(tmp_path / "embeds.npy", {k[6:]: fx[k] for k in fx.files if k.startswith("embed/")}, allow_pickle=True)
    return str(tmp_path / "eps"), str(tmp_path / "embeds.npy"), str(tmp_path / "instr.json")


def test_dataset_items_match_the_golden_fixture(tmp_path):
    """tests/golden/reghead_dataset_items.npz (make_golden_reghead_dataset.py, from the imported reference dataset): rot_type
    'quat' and 'euler', pos_type 'cont' and 'disc', read back through KeystepDataset with the recorded seeds."""
    fx = np.load(os.path.join(ru.GOLDEN_DIR, "reghead_dataset_items.npz"), allow_pickle=False)
    paths = _fixture_store(fx, tmp_path)
    seen = set()
    for si, opts in enumerate(json.loads(str(fx["opts"]))):
        d = ds.KeystepDataset(*paths, host_labels=True, **opts)
        assert len(d) == int(fx[f"set{si}/len"])
        seen.add(opts["rot_type"])
        for idx in range(min(len(d), 2)):
            random.seed(17 + idx); np.random.seed(17 + idx)
            item = d[idx]
            keys = {k.split("/")[2] for k in fx.files if k.startswith(f"set{si}/item{idx}/")}
            assert keys == set(item), (si, keys ^ set(item))
            for k in keys:
                assert len(item[k]) == int(fx[f"set{si}/item{idx}/{k}/n"]) > 0, k
                for j, v in enumerate(item[k]):
                    want = fx[f"set{si}/item{idx}/{k}/{j}"]
                    have = np.asarray(v.numpy() if hasattr(v, "numpy") else v)
                    assert have.shape == want.shape, (si, k)
                    if want.dtype.kind in "fc":
                        np.testing.assert_allclose(have, want, rtol=0, atol=1e-6, err_msg=f"set{si}/{k}")
                    else:
                        assert np.array_equal(have, want), k
            width = 8 if opts["rot_type"] == "quat" else 7
            assert all(t.shape == (width,) and t.dtype == torch.float32 for t in item["gt_actions"])
    assert seen == {"quat", "euler"}


@pytest.mark.parametrize("rot_type", ["rot6d", "euler_delta"])
def test_dataset_refuses_the_other_rotation_types(rot_type, tmp_path):
    with pytest.raises(NotImplementedError, match=rot_type):
        ds.KeystepDataset(str(tmp_path), "none.npy", "none.json", rot_type=rot_type)


@pytest.mark.reference
@pytest.mark.skipif(not HAVE_REF, reason="reference tree is only present in the build container")
@pytest.mark.parametrize("opts", [
    dict(rot_type="quat", pos_type="cont", rm_robot="box_keep_gripper", augment_pc=True, aug_max_rot=180, xyz_shift="center",
         xyz_norm=False, use_height=True, instr_embed_type="all", num_points=500),
    dict(rot_type="euler", pos_type="cont", rm_robot="box", augment_pc=False, xyz_shift="gripper", xyz_norm=True, use_height=False,
         instr_embed_type="last", num_points=4096, all_step_in_batch=False, include_last_step=True),
    dict(rot_type="euler", pos_type="disc", pos_bins=15, pos_bin_size=0.01, rm_robot="none", augment_pc=True, aug_max_rot=45,
         xyz_shift="none", xyz_norm=False, use_height=True, instr_embed_type="all", num_points=300),
    dict(rot_type="quat", pos_type="cont", rm_robot="none", augment_pc=False, xyz_shift="center", xyz_norm=True, use_height=True,
         instr_embed_type="last", num_points=300),
])
def test_dataset_items_match_the_reference_dataset(tmp_path, opts):
    import test_host_dataset as th

    store, instr_file, embed_file = th._make_store(tmp_path, seed=12)
    th._install_reference_standins()
    from genrobo3d.train.datasets.simple_policy_dataset import SimplePolicyDataset

    ref = SimplePolicyDataset(store.root, embed_file, instr_file, **opts)
    got = ds.KeystepDataset(store.root, embed_file, instr_file, host_labels=True, **opts)
    assert len(ref) == len(got) > 0
    for idx in range(0, len(ref), max(1, len(ref) // 5)):
        random.seed(200 + idx); np.random.seed(200 + idx)
        want = ref[idx]
        random.seed(200 + idx); np.random.seed(200 + idx)
        have = got[idx]
        assert set(want) == set(have) and len(want["pc_fts"]) > 0
        for k in want:
            assert len(want[k]) == len(have[k]), k
            for a, b in zip(want[k], have[k]):
                if isinstance(a, torch.Tensor):
                    assert a.dtype == b.dtype and a.shape == b.shape, k
                    assert torch.allclose(a.double(), b.double(), rtol=0, atol=1e-6 if k != "disc_pos_probs" else 1e-9), k
                elif isinstance(a, np.ndarray):
                    np.testing.assert_allclose(a, b, rtol=0, atol=1e-9, err_msg=k)
                else:
                    assert a == pytest.approx(b) if isinstance(a, float) else a == b, k


# ------------------------------------------------------------------------------------ restatement vs the live reference
def _golden_path():
    p = os.path.join(HERE, "golden")
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.mark.reference
@pytest.mark.skipif(not HAVE_REF, reason="reference tree is only present in the build container")
@pytest.mark.parametrize("temp", [1.0, 0.1])
@pytest.mark.parametrize("pos,rot,da", [(p, r, 8 if r == "quat" else 7) for p, r in COMBOS] + [("heatmap_mlp", "euler", 8)])
def test_restatement_agrees_with_the_live_reference(pos, rot, da, temp):
    """tests/reghead_util.head / losses against the reference's ActionHead.forward and compute_loss, both in float64, on random
    weights and a ragged batch with labels on both sides of every selection."""
    _golden_path()
    import ref_harness as rh

    rh.install_shims()
    from genrobo3d.models.simple_policy_ptv3 import ActionHead as RefHead, SimplePolicyPTV3CA as RefPolicy

    torch.manual_seed(11)
    hs, bins, counts = 32, 6, [17, 1, 40]
    B, N = len(counts), sum(counts)
    ref = RefHead("max", pos, rot, hs, da, dropout=0, pos_bins=bins).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn_like(p) * (0.5 if p.ndim == 2 else 0.1))
    feat, coord = torch.randn(N, hs, dtype=torch.float64), torch.randn(N, 3, dtype=torch.float64)
    sd = ref.state_dict()
    par = {a + b + c: sd[f"{m}.{i}.{t}"] for a, m in (("h", "heatmap_mlp"), ("a", "action_mlp"))
           for b, t in (("w", "weight"), ("b", "bias")) for c, i in (("0", 0), ("3", 3))}
    want = ref(feat, counts, coords=coord, temp=temp)
    have = ru.head(feat, par, counts, coord, pos, rot, temp=temp)
    for a, b in zip(want, have):
        assert a.shape == b.shape and (a - b).abs().max() < 1e-6
    if rot == "euler":
        r = torch.where(torch.rand(B, 3) < 0.5, 0.9, -0.9).double() * torch.sign(torch.randn(B, 3)).double()
        r[0, 0] = 0.0
    elif rot == "quat":
        r = have[1].detach() * torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)[:, None] + 0.1 * torch.randn(B, 4, dtype=torch.float64)
    else:
        r = torch.randint(0, 72, (B, 3)).double()
    gt = torch.cat([0.1 * torch.randn(B, 3, dtype=torch.float64), r, torch.randint(0, 2, (B, 1)).double()], 1)
    probs = [torch.softmax(torch.randn(3, n * 2 * bins, dtype=torch.float64), 1) for n in counts]
    stub = types.SimpleNamespace(config=rh.to_cfg({"action_config": {"pos_pred_type": pos, "rot_pred_type": rot},
                                                   "loss_config": {"pos_weight": 1.5, "rot_weight": 0.75}}))
    lw = RefPolicy.compute_loss(stub, want, gt, disc_pos_probs=probs, npoints_in_batch=counts)
    lh = ru.losses(*have, gt, pos, rot, counts=counts, disc_pos_probs=probs, pos_w=1.5, rot_w=0.75)
    for k in ("pos", "rot", "open", "total"):
        assert abs(float(lw[k].detach()) - float(lh[k].detach())) < 1e-6, k
    if rot != "euler_disc":
        la, lb = ru.rot_candidates(have[1].detach(), r, rot)
        assert bool((la < lb).any()) and bool((la >= lb).any())


@pytest.mark.reference
@pytest.mark.skipif(not HAVE_REF, reason="reference tree is only present in the build container")
def test_fixture_regenerates_bit_for_bit(tmp_path):
    _golden_path()
    import make_golden_reghead as mg

    name = "reghead_tiny_mlp_quat_train"
    new = dict(np.load(mg.run_case(name, str(tmp_path))))
    old = ru.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k], equal_nan=old[k].dtype.kind == "f"), k
