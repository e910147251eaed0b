"""Model configuration for the 3D-LOTUS hot path.

Mirrors the reference's config contract: `genrobo3d/configs/rlbench/simple_policy_ptv3.yaml`
(section MODEL) merged with `KEY VALUE` overrides (genrobo3d/configs/default.py:60-92).  yacs is
not available, so the YAML is read with PyYAML into an attribute dict with no-op
defrost()/freeze().  The published v1 model is defined by the CLI overrides of
job_scripts/train_3dlotus_policy.sh:61-87; they ship here as the preset `v1`.
"""
import ast
import copy


class Cfg(dict):
    """Attribute dict standing in for yacs.CfgNode (attribute access, .get, defrost/freeze)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def defrost(self):
        pass

    def freeze(self):
        pass


def to_cfg(d):
    if isinstance(d, dict):
        return Cfg({k: to_cfg(v) for k, v in d.items()})
    return d


# YAML defaults of MODEL (simple_policy_ptv3.yaml:92-158), restated as data.
_YAML_MODEL = dict(
    model_class="SimplePolicyPTV3AdaNorm",
    ptv3_config=dict(
        in_channels=6, order=["z", "z-trans", "hilbert", "hilbert-trans"], stride=[2, 2, 2, 2],
        enc_depths=[2, 2, 2, 6, 2], enc_channels=[32, 64, 128, 256, 512], enc_num_head=[2, 4, 8, 16, 32],
        enc_patch_size=[128] * 5, dec_depths=[2, 2, 2, 2], dec_channels=[64, 64, 128, 256],
        dec_num_head=[4, 4, 8, 16], dec_patch_size=[128] * 4, mlp_ratio=4, qkv_bias=True, qk_scale=None,
        qk_norm=False, scaled_cosine_attn=False, attn_drop=0.1, proj_drop=0.1, drop_path=0.1,
        pre_norm=True, shuffle_orders=True, enable_rpe=False, enable_flash=True, upcast_attention=False,
        upcast_softmax=False, cls_mode=False, pdnorm_bn=True, pdnorm_ln=True, pdnorm_decouple=False,
        pdnorm_adaptive=True, pdnorm_affine=True, pdnorm_conditions=None, pdnorm_only_decoder=False,
        add_coords_in_attn="none"),
    action_config=dict(
        voxel_size=0.01, context_channels=256, txt_ft_size=512, max_txt_len=77, txt_reduce="mean",
        use_ee_pose=True, use_step_id=False, max_steps=30, reduce="max", max_traj_len=1, dim_actions=8,
        pos_pred_type="heatmap_mlp", pos_heatmap_temp=0.1, rot_pred_type="euler", dropout=0.1,
        pos_bins=40, pos_bin_size=0.01, best_disc_pos="max"),
    loss_config=dict(pos_weight=1, rot_weight=1),
)

# job_scripts/train_3dlotus_policy.sh:61-87 (MODEL.* overrides only)
V1_OVERRIDES = [
    "ptv3_config.drop_path", "0.0", "ptv3_config.attn_drop", "0.1", "ptv3_config.proj_drop", "0.1",
    "action_config.dropout", "0.2", "action_config.voxel_size", "0.01", "action_config.reduce", "max",
    "action_config.dim_actions", "7", "action_config.rot_pred_type", "euler_disc",
    "action_config.pos_heatmap_temp", "0.1", "ptv3_config.in_channels", "7",
    "ptv3_config.pdnorm_only_decoder", "False", "ptv3_config.qk_norm", "True",
    "ptv3_config.scaled_cosine_attn", "False", "ptv3_config.enable_flash", "True",
    "action_config.max_steps", "30", "ptv3_config.enc_depths", "[1, 1, 1, 1, 1]",
    "ptv3_config.dec_depths", "[1, 1, 1, 1]", "ptv3_config.enc_channels", "[64, 128, 256, 512, 768]",
    "ptv3_config.dec_channels", "[128, 128, 256, 512]", "action_config.use_step_id", "False",
    "action_config.use_ee_pose", "False", "loss_config.pos_weight", "1", "loss_config.rot_weight", "1",
    "action_config.pos_pred_type", "heatmap_disc", "action_config.pos_bins", "15",
    "model_class", "SimplePolicyPTV3CA", "ptv3_config.pdnorm_bn", "False",
    "ptv3_config.pdnorm_ln", "False", "ptv3_config.pdnorm_adaptive", "False",
]

# BASELINE.json configs[0]: "3D-LOTUS tiny (2 layers, 64-dim, 512 pts/scene)"
TINY_OVERRIDES = V1_OVERRIDES + [
    "ptv3_config.enc_depths", "[1, 1]", "ptv3_config.enc_channels", "[64, 64]",
    "ptv3_config.enc_num_head", "[2, 2]", "ptv3_config.enc_patch_size", "[128, 128]",
    "ptv3_config.stride", "[2]", "ptv3_config.dec_depths", "[1]", "ptv3_config.dec_channels", "[64]",
    "ptv3_config.dec_num_head", "[2]", "ptv3_config.dec_patch_size", "[128]",
]


# the tiny width with stages deeper than one Block (the reference YAML default is enc_depths [2, 2, 2, 6, 2]): Block i of a
# stage attends along curve slot i % 4, so depth 5 wraps around the four curves
TINYDEEP_OVERRIDES = TINY_OVERRIDES + ["ptv3_config.enc_depths", "[2, 5]", "ptv3_config.dec_depths", "[2]"]


# tiny width with the two optional context tokens of SimplePolicyPTV3CA (simple_policy_ptv3.py:386-389,419-427): the current
# end-effector pose and the key-step index are appended to every cloud's instruction tokens
TINYCTX_OVERRIDES = TINY_OVERRIDES + ["action_config.use_ee_pose", "True", "action_config.use_step_id", "True"]


def _parse(v):
    if not isinstance(v, str):
        return v
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return {"null": None, "true": True, "false": False}.get(v.lower(), v)


def merge_overrides(cfg, overrides):
    """yacs merge_from_list semantics: [KEY, VALUE, KEY, VALUE, ...] with dotted keys."""
    assert len(overrides) % 2 == 0
    for k, v in zip(overrides[0::2], overrides[1::2]):
        node = cfg
        parts = k.split(".")
        if parts[0] == "MODEL":
            parts = parts[1:]
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = _parse(v)
    return cfg


def load_model_config(yaml_path=None, overrides=()):
    """Read the MODEL section of a reference-format YAML (or the built-in defaults) and apply
    overrides.  Returns an attribute dict usable as `config.MODEL` of the reference trainer."""
    if yaml_path is not None:
        import yaml

        with open(yaml_path) as f:
            model = yaml.safe_load(f)["MODEL"]
    else:
        model = copy.deepcopy(_YAML_MODEL)
    return to_cfg(merge_overrides(model, list(overrides)))


# genrobo3d/configs/rlbench/motion_planner_ptv3.yaml:103-164 differs from the simple-policy YAML in these MODEL keys
_YAML_MP_DELTA = dict(model_class="MotionPlannerPTV3AdaNorm",
                      action_config=dict(pc_label_channels=64, traj_embed_size=64, max_traj_len=5,
                                         rot_pred_type="euler_disc"))

# job_scripts/train_3dlotusplus_motion_planner.sh:71-98 (MODEL.* overrides; pos_bin_size=15, max_traj_len=5)
MP_OVERRIDES = [
    "ptv3_config.drop_path", "0.0", "ptv3_config.attn_drop", "0.1", "ptv3_config.proj_drop", "0.1",
    "action_config.dropout", "0.2", "action_config.voxel_size", "0.01", "action_config.reduce", "max",
    "action_config.dim_actions", "7", "action_config.rot_pred_type", "euler_disc",
    "action_config.pos_pred_type", "heatmap_disc", "action_config.pos_heatmap_temp", "0.1",
    "ptv3_config.in_channels", "4", "ptv3_config.pdnorm_only_decoder", "False", "ptv3_config.qk_norm", "True",
    "ptv3_config.scaled_cosine_attn", "False", "ptv3_config.enable_flash", "True",
    "action_config.max_steps", "30", "ptv3_config.enc_depths", "[1, 1, 1, 1, 1]",
    "ptv3_config.dec_depths", "[1, 1, 1, 1]", "ptv3_config.enc_channels", "[64, 128, 256, 512, 768]",
    "ptv3_config.dec_channels", "[128, 128, 256, 512]", "loss_config.pos_weight", "1",
    "loss_config.rot_weight", "1", "action_config.max_traj_len", "5", "action_config.pos_bins", "15",
    "action_config.txt_reduce", "attn", "action_config.use_ee_pose", "False",
    "model_class", "MotionPlannerPTV3CA", "ptv3_config.pdnorm_bn", "False",
    "ptv3_config.pdnorm_ln", "False", "ptv3_config.pdnorm_adaptive", "False",
]
MP_TINY_OVERRIDES = MP_OVERRIDES + TINY_OVERRIDES[len(V1_OVERRIDES):]
# the YAML's own use_ee_pose = True (motion_planner_ptv3.yaml:151; the published job script switches it off)
MP_TINYCTX_OVERRIDES = MP_TINY_OVERRIDES + ["action_config.use_ee_pose", "True"]


# job_scripts/train_3dlotus_policy_peract.sh:55-75: the v1 model; `txt_reduce attn` is set but SimplePolicyPTV3CA ignores it
PERACT_OVERRIDES = V1_OVERRIDES + ["action_config.txt_reduce", "attn"]


# SimplePolicyPTV3AdaNorm (simple_policy_ptv3.py:160-373): the same networks with the YAML's adaptive PDNorm switches
# (simple_policy_ptv3.yaml:93 ff.) instead of cross attention
ADANORM_SWITCHES = ["model_class", "SimplePolicyPTV3AdaNorm", "ptv3_config.pdnorm_bn", "True", "ptv3_config.pdnorm_ln", "True",
                    "ptv3_config.pdnorm_adaptive", "True", "ptv3_config.pdnorm_decouple", "False",
                    "ptv3_config.pdnorm_affine", "True", "ptv3_config.pdnorm_only_decoder", "False"]
ADANORM_OVERRIDES = {"adanorm_v1": V1_OVERRIDES + ADANORM_SWITCHES, "adanorm_tiny": TINY_OVERRIDES + ADANORM_SWITCHES,
                     "adanorm_tinyctx": TINYCTX_OVERRIDES + ADANORM_SWITCHES}
# ... with the YAML's own qk_norm False (attention without q/k LayerNorm); 'adanorm_yaml' is the YAML as shipped, no override
PLAIN_ATTN = ["ptv3_config.qk_norm", "False"]
ADANORM_OVERRIDES.update({"adanorm_yaml": [], "adanorm_tiny_plain": ADANORM_OVERRIDES["adanorm_tiny"] + PLAIN_ATTN,
                          "adanorm_v1_plain": ADANORM_OVERRIDES["adanorm_v1"] + PLAIN_ATTN})


# The regression head of the YAML's own defaults (simple_policy_ptv3.yaml: pos_pred_type 'heatmap_mlp', rot_pred_type 'euler')
# on the published networks; dim_actions stays 7 (3 angles + openness from action_mlp)
REG_SWITCHES = ["action_config.pos_pred_type", "heatmap_mlp", "action_config.rot_pred_type", "euler"]
REG_OVERRIDES = {"tiny_reg": TINY_OVERRIDES + REG_SWITCHES, "v1_reg": V1_OVERRIDES + REG_SWITCHES,
                 "adanorm_tiny_reg": ADANORM_OVERRIDES["adanorm_tiny"] + REG_SWITCHES}


# MotionPlannerPTV3AdaNorm (motion_planner_ptv3.py:151-397).  'mp_yaml' is the MODEL section of motion_planner_ptv3.yaml as
# shipped: _YAML_MODEL + _YAML_MP_DELTA without the keys that YAML does not have (use_step_id is commented out there, :152).
# 'mp_ada_tiny': the tiny widths of BASELINE configs[0] under the YAML's own switches (adaptive PDNorm, qk_norm False, heatmap_mlp
# positions, pose context); the job-script overrides it keeps are the ones about the networks' size and the 4-column input.
_YAML_MP_ABSENT = ("use_step_id",)
MP_ADA_OVERRIDES = {"mp_yaml": [], "mp_ada_tiny": [
    "ptv3_config.in_channels", "4", "ptv3_config.drop_path", "0.0", "action_config.dropout", "0.2", "action_config.dim_actions", "7",
    "action_config.pos_bins", "15"] + TINY_OVERRIDES[len(V1_OVERRIDES):]}


# SimplePolicyPTV3Concat (simple_policy_ptv3.py:434-463): the context vector of a cloud is concatenated to every point's features, so
# in_channels = columns of pc_fts + context_channels and the backbone is a plain PointTransformerV3 (no PDNorm).  'concat_yaml' is
# the YAML's MODEL section with the class, the input width and the three PDNorm flags changed; 'concat_tiny' the tiny family
# (7 point columns + 256) with the two optional context terms on.
CONCAT_SWITCHES = ["model_class", "SimplePolicyPTV3Concat", "ptv3_config.pdnorm_bn", "False", "ptv3_config.pdnorm_ln", "False",
                   "ptv3_config.pdnorm_adaptive", "False"]
CONCAT_OVERRIDES = {"concat_yaml": CONCAT_SWITCHES + ["ptv3_config.in_channels", "262"],
                    "concat_tiny": TINYCTX_OVERRIDES + CONCAT_SWITCHES + ["ptv3_config.in_channels", "263"]}


# add_coords_in_attn 'qk' / 'qkv' (simple_policy_ptv3.yaml:129, motion_planner_ptv3.yaml:139: "none, qk, qkv"; PointTransformerV3/
# model.py:484-495) on the AdaNorm and the Concat backbone.  'adanorm_yaml_qk' is the shipped YAML with that one key flipped; the
# tiny ones cover both modes with and without q/k LayerNorm (adanorm_tiny_plain and mp_ada_tiny have qk_norm False, adanorm_tiny
# and concat_tiny qk_norm True).
def _coords(mode):
    return ["ptv3_config.add_coords_in_attn", mode]


ADANORM_OVERRIDES.update({"adanorm_tiny_qk": ADANORM_OVERRIDES["adanorm_tiny_plain"] + _coords("qk"),
                          "adanorm_tiny_qkv": ADANORM_OVERRIDES["adanorm_tiny"] + _coords("qkv"),
                          "adanorm_yaml_qk": _coords("qk")})
CONCAT_OVERRIDES.update({"concat_tiny_qk": CONCAT_OVERRIDES["concat_tiny"] + _coords("qk"),
                         "concat_tiny_qkv": CONCAT_OVERRIDES["concat_tiny"] + _coords("qkv")})
MP_ADA_OVERRIDES["mp_ada_tiny_qkv"] = MP_ADA_OVERRIDES["mp_ada_tiny"] + _coords("qkv")


# enable_flash False / enable_rpe True (simple_policy_ptv3.yaml:117-120, motion_planner_ptv3.yaml:127-130; PointTransformerV3/
# model.py:307-326, :469-472, :499-527) on the AdaNorm and the Concat backbone: the non-flash patching (per-level patch size =
# min(patch size, fewest points of a cloud)) alone ('adanorm_tiny_dense') and with the relative-position term.  'adanorm_yaml_rpe'
# is the shipped YAML with those two keys flipped (qk_norm False); adanorm_tiny_plain_rpe and mp_ada_tiny_rpe have qk_norm False too,
# adanorm_tiny_rpe and concat_tiny_rpe qk_norm True.
DENSE_ATTN = ["ptv3_config.enable_flash", "False"]
RPE_ATTN = DENSE_ATTN + ["ptv3_config.enable_rpe", "True"]
ADANORM_OVERRIDES.update({"adanorm_tiny_dense": ADANORM_OVERRIDES["adanorm_tiny"] + DENSE_ATTN,
                          "adanorm_tiny_rpe": ADANORM_OVERRIDES["adanorm_tiny"] + RPE_ATTN,
                          "adanorm_tiny_plain_rpe": ADANORM_OVERRIDES["adanorm_tiny_plain"] + RPE_ATTN,
                          "adanorm_yaml_rpe": RPE_ATTN})
CONCAT_OVERRIDES["concat_tiny_rpe"] = CONCAT_OVERRIDES["concat_tiny"] + RPE_ATTN
MP_ADA_OVERRIDES["mp_ada_tiny_rpe"] = MP_ADA_OVERRIDES["mp_ada_tiny"] + RPE_ATTN


# patch sizes above 128 (PointTransformerV3/model.py:529-551; the reference's constructors default to 1024) on the AdaNorm and the
# Concat backbone: the tiny networks at 256 — with (adanorm_tiny, concat_tiny) and without (adanorm_tiny_plain, mp_ada_tiny) q/k
# LayerNorm — and the shipped YAML with both patch-size lists at 1024.
def _patches(k, n_enc, n_dec):
    return ["ptv3_config.enc_patch_size", str([k] * n_enc), "ptv3_config.dec_patch_size", str([k] * n_dec)]


ADANORM_OVERRIDES.update({"adanorm_tiny_p256": ADANORM_OVERRIDES["adanorm_tiny"] + _patches(256, 2, 1),
                          "adanorm_tiny_plain_p256": ADANORM_OVERRIDES["adanorm_tiny_plain"] + _patches(256, 2, 1),
                          "adanorm_yaml_p1024": _patches(1024, 5, 4)})
CONCAT_OVERRIDES["concat_tiny_p256"] = CONCAT_OVERRIDES["concat_tiny"] + _patches(256, 2, 1)
MP_ADA_OVERRIDES["mp_ada_tiny_p256"] = MP_ADA_OVERRIDES["mp_ada_tiny"] + _patches(256, 2, 1)


def preset(name="v1"):
    """'v1' / 'tiny': 3D-LOTUS policy; 'peract': the RLBench-18task (PerAct) variant of BASELINE configs[4] (same network;
    its bf16 compute mode is ops.set_gemm_precision("bf16")); 'mp' / 'mp_tiny': 3D-LOTUS++ motion planner (configs[3]);
    'adanorm_v1' / 'adanorm_tiny' / 'adanorm_tinyctx': the policy networks as SimplePolicyPTV3AdaNorm (adaptive PDNorm);
    'adanorm_yaml': simple_policy_ptv3.yaml as shipped (= load_model_config(None)); 'adanorm_tiny_plain' / 'adanorm_v1_plain':
    adanorm_tiny / adanorm_v1 with qk_norm False;
    'tiny_reg' / 'v1_reg' / 'adanorm_tiny_reg': their base preset with the regression head (heatmap_mlp positions, euler);
    'mp_yaml': motion_planner_ptv3.yaml as shipped (MotionPlannerPTV3AdaNorm, soft trajectory head); 'mp_ada_tiny': its tiny width;
    'concat_yaml' / 'concat_tiny': SimplePolicyPTV3Concat on the YAML's networks (in_channels 262) / the tiny ones (263);
    'adanorm_tiny_qk' / 'adanorm_tiny_qkv' / 'adanorm_yaml_qk' / 'concat_tiny_qk' / 'concat_tiny_qkv' / 'mp_ada_tiny_qkv': their
    base preset with add_coords_in_attn 'qk' / 'qkv' (adanorm_tiny_qk on adanorm_tiny_plain: qk_norm False);
    'adanorm_tiny_dense': adanorm_tiny with enable_flash False; 'adanorm_tiny_rpe' / 'adanorm_tiny_plain_rpe' / 'concat_tiny_rpe' /
    'mp_ada_tiny_rpe' / 'adanorm_yaml_rpe': their base preset with enable_flash False and enable_rpe True;
    'adanorm_tiny_p256' / 'adanorm_tiny_plain_p256' / 'concat_tiny_p256' / 'mp_ada_tiny_p256': their base preset with every patch
    size 256; 'adanorm_yaml_p1024': the shipped YAML with every patch size 1024."""
    if name in ("mp", "mp_tiny", "mp_tinyctx"):
        model = copy.deepcopy(_YAML_MODEL)
        model["model_class"] = _YAML_MP_DELTA["model_class"]
        model["action_config"].update(_YAML_MP_DELTA["action_config"])
        return to_cfg(merge_overrides(model, {"mp": MP_OVERRIDES, "mp_tiny": MP_TINY_OVERRIDES, "mp_tinyctx": MP_TINYCTX_OVERRIDES}[name]))
    if name in MP_ADA_OVERRIDES:
        model = copy.deepcopy(_YAML_MODEL)
        model["model_class"] = _YAML_MP_DELTA["model_class"]
        model["action_config"].update(_YAML_MP_DELTA["action_config"])
        for k in _YAML_MP_ABSENT:
            del model["action_config"][k]
        return to_cfg(merge_overrides(model, MP_ADA_OVERRIDES[name]))
    if name in ADANORM_OVERRIDES:
        return load_model_config(None, ADANORM_OVERRIDES[name])
    if name in REG_OVERRIDES:
        return load_model_config(None, REG_OVERRIDES[name])
    if name in CONCAT_OVERRIDES:  # 'concat_yaml' / 'concat_tiny': SimplePolicyPTV3Concat
        return load_model_config(None, CONCAT_OVERRIDES[name])
    return load_model_config(None, {"v1": V1_OVERRIDES, "tiny": TINY_OVERRIDES, "peract": PERACT_OVERRIDES,
                                    "tinydeep": TINYDEEP_OVERRIDES, "tinyctx": TINYCTX_OVERRIDES}[name])


def plain(cfg):
    """dict(ptv3=..., action=..., loss=...) view used by the oracle and the kernels' host code."""
    return dict(ptv3=dict(cfg["ptv3_config"]), action=dict(cfg["action_config"]), loss=dict(cfg["loss_config"]))
