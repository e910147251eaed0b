"""Host-side checks of the soft trajectory head and MotionPlannerPTV3AdaNorm (no device): the float64 restatement of
tests/trajsoft_util.py against the reference's own ActionHead + compute_loss, the state_dict layout of the new presets against
the fixtures, a YAML round trip through the factory, every refusal by name, the argument checks of the four entry points (they
return before any launch) and the workspace queries."""
import json
import types

import numpy as np
import pytest
import torch

import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg
from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm, MotionPlannerPTV3CA, TrajectoryActionHead
from robot_3dlotus_amd.policy import MODEL_FACTORY

import mp_ada_util as mu
import trajsoft_util as tu

REF_YAML = "/root/reference/genrobo3d/configs/rlbench/motion_planner_ptv3.yaml"


def test_rows_enter_the_branches_they_name():
    tu.self_check()
    assert len(set(tu.ROW_IDS)) == len(tu.ROWS)


# ------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.reference
def test_restatement_equals_the_reference_head_and_losses():
    from golden import ref_harness as rh

    rh.install_shims()
    import einops  # noqa: F401
    from genrobo3d.models.motion_planner_ptv3 import ActionHead, MotionPlannerPTV3AdaNorm as RefPlanner

    torch.manual_seed(3)
    C, T, E, temp, counts = 64, 5, 64, 0.1, [40, 1, 129]
    n, B = sum(counts), len(counts)
    head = ActionHead("max", "heatmap_mlp", "euler_disc", C, 7, T, dropout=0, traj_embed_size=E).double()
    for p in head.parameters():
        torch.nn.init.normal_(p, std=0.3)
    x, coords = torch.randn(n, C, dtype=torch.float64), torch.randn(n, 3, dtype=torch.float64)
    xt, xr, xo, xstop = head(x, counts, coords=coords, temp=temp)
    hm, te = head.heatmap_mlp, head.traj_embedding.weight
    base = x @ hm[0].weight[:, :C].t()
    bias = te @ hm[0].weight[:, C:].t() + hm[0].bias
    e, mine = tu.head_ref(base, bias, hm[3].weight, hm[3].bias, coords, counts, temp, torch.ones(T, n, C, dtype=torch.float64),
                          slope=0.02)
    assert mine.shape == xt.shape == (B, T, 3)
    assert float((mine - xt).abs().max()) <= 1e-12 * max(1.0, float(xt.abs().max()))
    gt = torch.cat([torch.randn(B, T, 3, dtype=torch.float64), torch.randint(0, 72, (B, T, 3)).double(),
                    torch.randint(0, 2, (B, T, 1)).double()], -1)
    stop = torch.randint(0, 2, (B, T)).double()
    mask = torch.tensor([[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.float64)
    cfg = rh.to_cfg(dict(action_config=dict(pos_pred_type="heatmap_mlp", rot_pred_type="euler_disc"),
                         loss_config=dict(pos_weight=1.5, rot_weight=0.7)))
    ref = RefPlanner.compute_loss(types.SimpleNamespace(config=cfg), (xt, xr, xo, xstop), gt, stop, npoints_in_batch=counts,
                                  tgt_traj_masks=mask)
    ae = torch.cat([xr.reshape(B, T, -1), xo.unsqueeze(-1), xstop.unsqueeze(-1)], -1)
    L = tu.loss_ref(ae, mine, gt, stop, mask, 72, 1.5, 0.7)
    # the reference casts the stop targets with .float() (motion_planner_ptv3.py:386), which takes its stop term — and the total
    # that contains it — through float32 whatever the dtype of the predictions: those two agree to fp32 rounding, the rest to 1e-12
    for k, name in enumerate(("pos", "rot", "open", "stop", "total")):
        bar = 1e-12 if name in ("pos", "rot", "open") else 4 * 2.0 ** -24
        assert abs(float(L[k]) - float(ref[name])) <= bar * max(1.0, abs(float(ref[name]))), name
    assert abs(float(L[4] - L[3]) - float(ref["total"] - ref["stop"])) <= 1e-12 * max(1.0, abs(float(ref["total"])))


# ------------------------------------------------------------------------------------ configuration, layout, factory
@pytest.mark.reference
def test_preset_mp_yaml_is_the_shipped_yaml_key_for_key():
    import yaml

    with open(REF_YAML) as f:
        model = yaml.safe_load(f)["MODEL"]
    got = lcfg.preset("mp_yaml")
    assert got == model
    for sec in ("ptv3_config", "action_config", "loss_config"):
        assert set(got[sec]) == set(model[sec]), sec


def test_new_presets():
    y, t = lcfg.preset("mp_yaml"), lcfg.preset("mp_ada_tiny")
    for cfg in (y, t):
        assert cfg.model_class == "MotionPlannerPTV3AdaNorm" and cfg.ptv3_config.qk_norm is False
        assert cfg.action_config.pos_pred_type == "heatmap_mlp" and cfg.action_config.rot_pred_type == "euler_disc"
        assert cfg.ptv3_config.pdnorm_adaptive and cfg.ptv3_config.pdnorm_bn and cfg.ptv3_config.pdnorm_ln
    assert y.ptv3_config.in_channels == 6 and y.ptv3_config.enc_depths == [2, 2, 2, 6, 2] and "use_step_id" not in y.action_config
    assert t.ptv3_config.in_channels == 4 and t.ptv3_config.enc_channels == [64, 64]
    # the published presets are what they were
    assert lcfg.preset("mp").model_class == "MotionPlannerPTV3CA" and lcfg.preset("mp").action_config.use_step_id is False


@pytest.mark.parametrize("case", ["mp_ada_tiny_train", "mp_ada_yaml_train"])
def test_state_dict_layout_equals_the_reference_layout(case):
    cfg = mu.case_config(case)
    before = json.dumps(cfg, sort_keys=True)
    m = MODEL_FACTORY[cfg.model_class](cfg)
    assert type(m) is MotionPlannerPTV3AdaNorm
    assert json.dumps(cfg, sort_keys=True) == before, "the caller's configuration was modified"
    want = json.loads(str(mu.load(case)["state_layout"]))
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == want
    assert m.act_proj_head.heatmap_mlp[3].out_features == 4
    assert m.ptv3_model.embedding.stem.conv.weight.shape[-1] == cfg.ptv3_config.in_channels + 64


def test_yaml_round_trip_through_the_factory(tmp_path):
    import yaml

    path = tmp_path / "motion_planner.yaml"
    model = json.loads(json.dumps(lcfg.preset("mp_ada_tiny")))
    path.write_text(yaml.safe_dump({"SEED": 1, "MODEL": model}))
    cfg = lcfg.load_model_config(str(path))
    assert cfg == lcfg.preset("mp_ada_tiny")
    m = MODEL_FACTORY[cfg.model_class](cfg)
    assert type(m) is MotionPlannerPTV3AdaNorm and m.soft_pos and not MotionPlannerPTV3CA.soft_pos
    cfg2 = lcfg.load_model_config(str(path), ["action_config.txt_reduce", "attn"])
    assert "txt_attn_fc.weight" in MODEL_FACTORY[cfg2.model_class](cfg2).state_dict() and "txt_attn_fc.weight" not in m.state_dict()


# ------------------------------------------------------------------------------------ refusals, by name
def _head(soft, reduce="max", pos="heatmap_mlp", rot="euler_disc", emb=64):
    return TrajectoryActionHead(reduce, pos, rot, 64, 7, 5, traj_embed_size=emb, soft_pos=soft)


def test_head_options():
    assert _head(True).heatmap_mlp[3].out_features == 4
    assert _head(True, pos="heatmap_disc").heatmap_mlp[3].out_features == 3 * 50 * 2
    assert _head(False, pos="heatmap_disc").heatmap_mlp[3].out_features == 3 * 50 * 2
    with pytest.raises(NotImplementedError, match="published head"):
        _head(False)
    for kw, word in ((dict(reduce="mean"), "reduce='mean'"), (dict(reduce="attn"), "reduce='attn'"),
                     (dict(pos="heatmap_mlp3"), "heatmap_mlp3"), (dict(pos="regression"), "regression"),
                     (dict(rot="euler"), "rot_pred_type='euler'"), (dict(rot="quat"), "quat"), (dict(rot="rot6d"), "rot6d"),
                     (dict(emb=0), "traj_embed_size")):
        with pytest.raises(NotImplementedError, match=word):
            _head(True, **kw)


def test_the_ca_planner_still_refuses_the_soft_head():
    cfg = lcfg.preset("mp_tiny")
    cfg.action_config.pos_pred_type = "heatmap_mlp"
    with pytest.raises(NotImplementedError):
        MotionPlannerPTV3CA(cfg)


def test_planner_refusals():
    cfg = lcfg.preset("mp_ada_tiny")
    m = MotionPlannerPTV3AdaNorm(cfg)
    batch = mu.mp_batch(1, 64, False, 5, 4)
    m.act_storage = "bf16"
    with pytest.raises(NotImplementedError, match="MotionPlannerPTV3AdaNorm: act_storage='bf16'"):
        m(dict(batch))
    m.act_storage = None
    for prec in ("bf16", "bf16x3"):
        m.gemm_precision = prec
        with pytest.raises(NotImplementedError, match="MotionPlannerPTV3AdaNorm with qk_norm=False"):
            m(dict(batch))
    m.gemm_precision = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(dict(batch))
    wide = dict(batch, pc_fts=torch.zeros(64, 9))
    with pytest.raises(NotImplementedError, match="9 > 8 columns"):
        m.prepare_ptv3_batch(wide)
    with pytest.raises(ValueError, match="in_channels is 4"):
        m.prepare_ptv3_batch(dict(batch, pc_fts=torch.zeros(64, 6)))
    with pytest.raises(ValueError, match="one instruction token per cloud"):
        m.prepare_ptv3_batch(dict(batch, txt_lens=[2]))
    for key, val in (("txt_reduce", "max"),):
        bad = lcfg.preset("mp_ada_tiny")
        bad.action_config[key] = val
        with pytest.raises(NotImplementedError, match="txt_reduce='max'"):
            MotionPlannerPTV3AdaNorm(bad)
    bad = lcfg.preset("mp_ada_tiny")
    bad.ptv3_config.pdnorm_decouple = True
    with pytest.raises(NotImplementedError, match="pdnorm_decouple"):
        MotionPlannerPTV3AdaNorm(bad)


# ------------------------------------------------------------------------------------ one forward, one prefetch memory
def test_one_planner_forward():
    """The AdaNorm planner runs MotionPlannerPTV3CA's _forward; the soft head lives in the three steps it overrides."""
    assert MotionPlannerPTV3AdaNorm._forward is MotionPlannerPTV3CA._forward
    for step in ("_positions", "_pos_loss_term", "_final_positions"):
        assert getattr(MotionPlannerPTV3AdaNorm, step) is not getattr(MotionPlannerPTV3CA, step), step
    assert MotionPlannerPTV3AdaNorm._traj_losses is MotionPlannerPTV3CA._traj_losses


def test_prefetch_memory_matches_by_identity_keeps_two_and_forgets_what_it_handed_out():
    from robot_3dlotus_amd.motion_planner import _Prefetched

    def batch(i):
        return {"pc_fts": torch.full((3, 4), float(i)), "pc_labels": torch.zeros(3, dtype=torch.long)}

    pre, b = _Prefetched(), [batch(i) for i in range(4)]
    assert pre.take(b[0]) is None and pre.entries == []
    built = [object() for _ in b]
    pre.remember(b[0], built[0])
    # an equal batch that is not the same tensors is another batch; so is one that shares only one of the two tensors
    assert pre.take({k: v.clone() for k, v in b[0].items()}) is None
    assert pre.take(dict(b[0], pc_labels=b[0]["pc_labels"].clone())) is None
    assert pre.take(dict(b[0], pc_fts=b[0]["pc_fts"].clone())) is None
    assert pre.take(b[0]) is built[0]
    assert pre.take(b[0]) is None and pre.entries == []                     # consumed: forgotten
    for i in range(3):
        pre.remember(b[i], built[i])
    assert len(pre.entries) == 2 and pre.take(b[0]) is None                 # at most two: the oldest is gone
    assert len(pre.entries) == 1 and pre.entries[0][2] is built[2]          # a miss keeps the latest entry only
    pre.remember(b[3], built[3])
    assert pre.take(b[2]) is built[2] and len(pre.entries) == 1
    assert pre.take(b[3]) is built[3] and pre.entries == []
    # both planners use it, for what each of them builds: [pc | one-hot] as one tensor, or the two column groups
    for cls, preset in ((MotionPlannerPTV3CA, "mp_tiny"), (MotionPlannerPTV3AdaNorm, "mp_ada_tiny")):
        m = cls(lcfg.preset(preset))
        assert isinstance(m._pre, _Prefetched)
        got = m._point_input(b[1])
        if cls is MotionPlannerPTV3CA:
            assert got.shape == (3, 8) and got.dtype == torch.float32
        else:
            assert [tuple(t.shape) for t in got] == [(3, 4), (3, 4)]
        m._pre.remember(b[1], got)
        assert m._pre.take(b[1]) is got


# ------------------------------------------------------------------------------------ the C-ABI: refusals and workspace sizes
def _buf(nfloat, dtype=np.float32):
    a = np.zeros(nfloat + 8, dtype=dtype)
    assert a.ctypes.data % 16 == 0
    return a


def _softpos_args(which):
    """Valid arguments of lotus_mp_softpos_fwd / _bwd on host memory (n = 10 rows, B = 2, C = 8, T = 3), keyed by name."""
    B, n, C, T = 2, 10, 8, 3
    keep = {k: _buf(sz) for k, sz in dict(base=n * C, bias=T * C, w3=4 * C, b3=4, pc=n * 3, e=T * n * 4, xt=B * T * 3, g=B * T * 3,
                                         dbase=n * C, dbias=T * C, dw3=4 * C, db3=4).items()}
    keep["stats"] = _buf(B * T * 2, np.float64)
    keep["off"], keep["batch"] = np.array([0, 4, 10], np.int32), np.repeat(np.arange(2, dtype=np.int32), [4, 6])
    nbytes = _capi.query("lotus_mp_softpos_workspace" if which == "fwd" else "lotus_mp_softpos_bwd_workspace",
                         *((B, T) if which == "fwd" else (n, C, T)))
    keep["workspace"] = _buf(nbytes // 4)
    a = {k: v.ctypes.data for k, v in keep.items()}
    a.update(ld=3, B=B, n=n, C=C, T=T, temp=0.1, drop_p=0.1, seed=7, workspace_bytes=nbytes, stream=None)
    return a, keep


def _call(name, a):
    L = _capi.lib()
    names = L.protos[name][2]
    rc = L.fn[name](*[a[k] for k in names])
    return rc, L.last_error()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_softpos_entry_points_refuse_bad_arguments(which):
    name = "lotus_mp_softpos_" + which
    a, keep = _softpos_args(which)
    names = _capi.lib().protos[name][2]
    assert set(names) <= set(a), set(names) - set(a)
    rc, msg = _call(name, a)
    assert rc == -2 and name in msg and "launch failed" in msg      # every check passes; no device to launch on
    ptrs = [k for k in names if k in keep and k != "workspace"]
    cases = [({k: None}, f"null {k}") for k in ptrs]
    cases += [(dict(B=0), "B"), (dict(n=0), "n"), (dict(T=0), "T"), (dict(B=-1), "B"), (dict(T=9), "T > 8"), (dict(C=0), "C"),
              (dict(C=6), "C % 4"), (dict(C=2052), "C > 2048"), (dict(ld=2), "ld"), (dict(temp=0.0), "temp"), (dict(temp=-1.0), "temp"),
              (dict(drop_p=1.0), "drop_p"), (dict(drop_p=-0.1), "drop_p"), (dict(workspace=None), "workspace"),
              (dict(workspace_bytes=a["workspace_bytes"] - 1), "workspace too small"), (dict(base=a["base"] + 4), "misaligned base"),
              (dict(e=a["e"] + 4), "misaligned e")]
    if which == "bwd":
        cases.append((dict(dbase=a["dbase"] + 4), "misaligned dbase"))
    for change, what in cases:
        rc, msg = _call(name, dict(a, **change))
        assert rc == -1 and msg.startswith(name + ":"), (what, rc, msg)
    del keep


def test_reg_loss_entry_points_refuse_bad_arguments():
    B, T, nrot = 2, 3, 4
    R, W = B * T, nrot * 3 + 2
    keep = {k: _buf(sz) for k, sz in dict(ae=R * W, gt=R * 7, stop=R, mask=R, xt=R * 3, losses=5, dae=R * W, dxt=R * 3, gl=5,
                                         dae_out=R * W, dxt_out=R * 3).items()}
    a = {k: v.ctypes.data for k, v in keep.items()}
    a.update(B=B, T=T, nrot=nrot, ga=7, pos_w=1.0, rot_w=1.0, stream=None)
    for name in ("lotus_mp_reg_loss_fwd", "lotus_mp_reg_loss_bwd"):
        names = _capi.lib().protos[name][2]
        rc, msg = _call(name, a)
        assert rc == -2 and name in msg
        cases = [{k: None} for k in names if k in keep] + [dict(B=0), dict(T=0), dict(nrot=0)]
        if name.endswith("fwd"):
            cases.append(dict(ga=6))
        for change in cases:
            rc, msg = _call(name, dict(a, **change))
            assert rc == -1 and msg.startswith(name + ":"), (change, rc, msg)
    del keep


def test_workspace_queries():
    assert _capi.query("lotus_mp_softpos_workspace", 5, 8) == 5 * 8 * tu.SP_SPLITS * 5 * 8
    assert _capi.query("lotus_mp_softpos_workspace", 1, 1) == _capi.query("lotus_softpos_workspace", 1)
    for n, C, T in ((1, 4, 1), (64, 64, 5), (65, 64, 5), (70001, 64, 5), (40, 2048, 8)):
        blocks = -(-n // tu.MPB_ROWS)
        assert _capi.query("lotus_mp_softpos_bwd_workspace", n, C, T) == blocks * ((T + 4) * C + 4) * 4
    assert _capi.lib().fn["lotus_abi_version"]() == 3
