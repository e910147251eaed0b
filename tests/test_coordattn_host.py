"""CPU checks of add_coords_in_attn 'qk' / 'qkv' (PointTransformerV3/model.py:396-398, 484-495): the self-check of the kernel
rows (tests/coordattn_util.py), the plan and workspace queries and the argument refusals of csrc/coord_attn.hip (answered before
any launch), the three model classes built with the option — parameter names, shapes and registration order against the
state layouts the reference's own models recorded in the fixtures —, what keeps refusing, the presets and their YAML round trip,
checkpoints both ways, and the float64 restatement of the two modes against autograd."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import coordattn_util as cu
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg
from robot_3dlotus_amd.policy import MODEL_FACTORY, SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA, SimplePolicyPTV3Concat

E_ARG = -1
COORD_PRESETS = ("adanorm_tiny_qk", "adanorm_tiny_qkv", "concat_tiny_qk", "concat_tiny_qkv", "mp_ada_tiny_qkv", "adanorm_yaml_qk")
BASE = {"adanorm_tiny_qk": "adanorm_tiny_plain", "adanorm_tiny_qkv": "adanorm_tiny", "concat_tiny_qk": "concat_tiny",
        "concat_tiny_qkv": "concat_tiny", "mp_ada_tiny_qkv": "mp_ada_tiny", "adanorm_yaml_qk": "adanorm_yaml"}


def _layout(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def _build(cfg):
    return MODEL_FACTORY[cfg.model_class](cfg)


# ------------------------------------------------------------------------------------------------- the kernel rows
def test_rows_self_check():
    rows, worst = cu.self_check()
    assert rows == len(cu.ROWS) >= 20
    print(f"    {rows} rows; the plan's float32 summation order alone: {worst:.3e} of max(1, |ref|max) (a quarter of the bar: "
          f"{0.25 * cu.KERNEL_TOL:.1e})")


def test_restatement_of_the_two_modes_against_autograd():
    """attn_input / coord_add_fwd / coord_add_wgrad against torch float64 autograd on the reference's own expressions
    (model.py:484-495)."""
    g = torch.Generator().manual_seed(3)
    n, C = 37, 8
    x, c = torch.randn(n, C, generator=g).double(), torch.randn(n, 3, generator=g).double()
    w, b = torch.randn(3 * C, C, generator=g).double(), torch.randn(3 * C, generator=g).double()
    dq = torch.randn(n, 3 * C, generator=g).double()
    for mode in ("qk", "qkv", "none"):
        P = torch.randn(C, 3, generator=g).double().requires_grad_(True)
        if mode == "qkv":
            qkv = torch.nn.functional.linear(x + torch.nn.functional.linear(c, P), w, b)
        elif mode == "qk":
            qkv = torch.nn.functional.linear(x, w, b)
            qk = torch.nn.functional.linear(c, P).repeat(1, 2)
            qkv = qkv + torch.cat([qk, torch.zeros(n, C, dtype=qkv.dtype)], dim=-1)
        else:
            qkv = torch.nn.functional.linear(x, w, b) + 0.0 * P.sum()
        qkv.backward(dq)
        got = cu.attn_input(mode, x.numpy(), c.numpy(), P.detach().numpy(), w.numpy(), b.numpy())
        assert np.abs(got - qkv.detach().numpy()).max() < 1e-12
        if mode == "qk":
            dP = cu.coord_add_wgrad(dq.numpy(), 2 * C, C, c.numpy())
            y = cu.coord_add_fwd(torch.nn.functional.linear(x, w, b).numpy(), 2 * C, C, c.numpy(), P.detach().numpy())
            assert np.abs(y - got).max() < 1e-12
        elif mode == "qkv":
            dP = cu.coord_add_wgrad((dq @ w).numpy(), C, C, c.numpy())
        else:
            continue
        assert np.abs(dP - P.grad.numpy()).max() < 1e-10


# ------------------------------------------------------------------------------------------------- plan, workspace, refusals
def _plan(n, W, Cw):
    out = np.full(6, -7, np.int32)
    _capi.call_raw("lotus_coord_add_plan", n, W, Cw, int(out.ctypes.data))
    return out.tolist()


def test_plan_and_workspace_queries():
    for r in cu.ROWS:
        _, W = cu.dims(r)
        p = _plan(r.n, W, r.Cw)
        assert p == cu.plan(r.n, W, r.Cw), (r.id, p)
        assert (p[1], p[2]) == r.branch[:2], r.id
        assert _capi.query("lotus_coord_add_workspace", r.n, W, r.Cw) == p[2] * r.Cw * 3 * 8, r.id
    assert _plan(0, 64, 64) == [64, 0, 1, 16, 16, 16]
    for Cw, qx in ((4, 1), (8, 2), (16, 4), (32, 8), (36, 16), (64, 16), (128, 32), (132, 64), (256, 64), (2048, 64)):
        assert _plan(1000, Cw, Cw)[4:] == [qx, 256 // qx], Cw
    # the ranges stop growing at 256, from where a thread folds more than one fp32 chunk
    assert _plan(10 ** 6, 128, 64)[2] == 256 and cu.chunks_per_thread(10 ** 6, 128, 64) == 16


BAD_SHAPES = [(10, 8, 0, "positive multiple of 4"), (10, 6, 6, "positive multiple of 4"), (10, -4, -4, "positive multiple of 4"),
              (10, 12, 4, "Cw or 2 Cw"), (10, 0, 4, "Cw or 2 Cw"), (10, 2052, 2052, "> 2048"), (-1, 8, 4, "must not be negative")]


def test_refusals_before_any_launch():
    """Every refusal is answered by the argument checks (LOTUS_E_ARG with the entry point named), so no pointer is ever read:
    the buffers here are host memory."""
    F = _capi.lib().fn
    y = np.zeros(64, np.float32)
    buf = ctypes.c_void_p(y.ctypes.data)
    odd = ctypes.c_void_p(y.ctypes.data + 4)
    out = np.zeros(6, np.int32)

    def fwd(**kw):
        a = dict(y=buf, ld=12, W=8, Cw=4, coord=buf, coord_ld=3, P=buf, n=2)
        a.update(kw)
        return F["lotus_coord_add_fwd"](a["y"], a["ld"], a["W"], a["Cw"], a["coord"], a["coord_ld"], a["P"], a["n"], None)

    def wgrad(**kw):
        a = dict(dy=buf, ld=12, W=8, Cw=4, coord=buf, coord_ld=3, n=2, dP=buf, ws=buf, ws_bytes=1 << 20)
        a.update(kw)
        return F["lotus_coord_add_wgrad"](a["dy"], a["ld"], a["W"], a["Cw"], a["coord"], a["coord_ld"], a["n"], a["dP"], a["ws"],
                                          a["ws_bytes"], None)

    def refused(rc, who, text):
        assert rc == E_ARG and who in _capi.lib().last_error() and text in _capi.lib().last_error(), (rc, _capi.lib().last_error())

    for n, W, Cw, text in BAD_SHAPES:
        refused(fwd(n=n, W=W, Cw=Cw, ld=max(W, 4) * 2), "lotus_coord_add_fwd", text)
        refused(wgrad(n=n, W=W, Cw=Cw, ld=max(W, 4) * 2), "lotus_coord_add_wgrad", text)
        refused(F["lotus_coord_add_plan"](n, W, Cw, out.ctypes.data), "lotus_coord_add_plan", text)
    refused(F["lotus_coord_add_plan"](10, 8, 4, None), "lotus_coord_add_plan", "null pointer")
    for k in ("y", "coord", "P"):
        refused(fwd(**{k: None}), "lotus_coord_add_fwd", "null pointer")
    for k in ("dy", "coord", "dP"):
        refused(wgrad(**{k: None}), "lotus_coord_add_wgrad", "null pointer")
    for f, who in ((fwd, "lotus_coord_add_fwd"), (wgrad, "lotus_coord_add_wgrad")):
        refused(f(ld=4), who, "ld = 4")            # ld < W
        refused(f(ld=10), who, "ld = 10")          # ld % 4 != 0
        refused(f(coord_ld=2), who, "coord_ld = 2")
    refused(fwd(y=odd), "lotus_coord_add_fwd", "16-byte aligned")
    refused(wgrad(dy=odd), "lotus_coord_add_wgrad", "16-byte aligned")
    refused(wgrad(ws=None), "lotus_coord_add_wgrad", "workspace")
    refused(wgrad(ws_bytes=_capi.query("lotus_coord_add_workspace", 2, 8, 4) - 1), "lotus_coord_add_wgrad", "workspace")
    # n == 0 forward: nothing to do, no launch
    assert fwd(n=0) == 0


def test_kernels_are_fp32_only_and_outside_the_twin_build():
    protos = _capi.parse_header()
    for name in ("lotus_coord_add_fwd", "lotus_coord_add_wgrad", "lotus_coord_add_workspace", "lotus_coord_add_plan"):
        assert name in protos and "lotus_b16_" + name[6:] not in protos, name
    from robot_3dlotus_amd import ops
    _capi.BF16 = True
    try:
        with pytest.raises(AssertionError, match="fp32 activation storage"):
            ops.coord_add_fwd(torch.zeros(4, 4), 4, 4, torch.zeros(4, 3), torch.zeros(4, 3))
    finally:
        _capi.BF16 = False


# ------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("case", list(cu.CASES))
def test_state_dict_layout_equals_the_fixtures(case):
    """Names, shapes and registration order of the reference's own model (coords_proj sits behind k_norm in every attention)."""
    layout = json.loads(str(cu.load(case)["state_layout"]))
    cfg = cu.case_config(case)
    m = _build(cfg)
    assert _layout(m) == layout
    cp = [k for k, _ in layout if k.endswith(".attn.coords_proj.weight")]
    blocks = sum(cfg.ptv3_config.enc_depths) + sum(cfg.ptv3_config.dec_depths)
    assert len(cp) == blocks == sum("coords_proj" in k for k, _ in layout)
    for k, shape in layout:
        if "coords_proj" in k:
            assert shape == [m.state_dict()[k.replace("coords_proj.weight", "proj.weight")].shape[0], 3]
    keys = [k for k, _ in layout]
    for k in cp:  # registered after k_norm (or, without q/k LayerNorm, after proj), before norm2
        prev = keys[keys.index(k) - 1]
        assert prev.endswith(".attn.k_norm.bias" if cfg.ptv3_config.qk_norm else ".attn.proj.bias"), (k, prev)
    names = [n for n, _ in m.named_parameters()]
    assert [n for n in names if "coords_proj" in n] == cp
    if case == "coord_adanorm_yaml_qk_eval":
        assert len(layout) == 661 + 22


@pytest.mark.parametrize("name", COORD_PRESETS)
def test_presets_and_none_has_no_coords_proj(name):
    cfg, base = lcfg.preset(name), lcfg.preset(BASE[name])
    mode = "qkv" if name.endswith("qkv") else "qk"
    assert cfg.ptv3_config.add_coords_in_attn == mode and base.ptv3_config.add_coords_in_attn == "none"
    cfg2 = lcfg.preset(name)
    cfg2.ptv3_config.add_coords_in_attn = "none"
    assert cfg2 == base
    if name == "adanorm_yaml_qk":
        assert cfg == lcfg.load_model_config(None, ["ptv3_config.add_coords_in_attn", "qk"])
        return
    with_c, without = _layout(_build(cfg)), _layout(_build(base))
    assert not any("coords_proj" in k for k, _ in without)
    assert [e for e in with_c if "coords_proj" not in e[0]] == without
    for off in (False, None, "none"):
        cfg2.ptv3_config.add_coords_in_attn = off
        assert _layout(_build(cfg2)) == without


@pytest.mark.parametrize("name", COORD_PRESETS)
def test_yaml_round_trip(name, tmp_path):
    import yaml

    cfg = lcfg.preset(name)
    path = tmp_path / (name + ".yaml")
    path.write_text(yaml.safe_dump({"MODEL": json.loads(json.dumps(cfg))}))
    loaded = lcfg.load_model_config(str(path))
    assert loaded == cfg and loaded.ptv3_config.add_coords_in_attn in ("qk", "qkv")
    if name != "adanorm_yaml_qk":
        assert _layout(_build(loaded)) == _layout(_build(cfg))


def test_classes_hand_the_mode_to_their_blocks():
    from robot_3dlotus_amd import adanorm, concat, ptv3
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm

    assert ptv3.PointTransformerV3CA.coord_attention is False
    assert adanorm.PointTransformerV3AdaNorm.coord_attention is True and concat.PointTransformerV3Plain.coord_attention is True
    for name, cls, blk in (("adanorm_tiny_qk", SimplePolicyPTV3AdaNorm, adanorm.AdaBlock),
                           ("concat_tiny_qkv", SimplePolicyPTV3Concat, concat.PlainBlock),
                           ("mp_ada_tiny_qkv", MotionPlannerPTV3AdaNorm, adanorm.AdaBlock)):
        m = _build(lcfg.preset(name))
        assert isinstance(m, cls)
        mode = "qkv" if name.endswith("qkv") else "qk"
        blocks = [b for b in m.ptv3_model.modules() if isinstance(b, blk)]
        assert len(blocks) == 3
        for b in blocks:
            assert b.attn.coords_mode == mode and isinstance(b.attn.coords_proj, torch.nn.Linear)
            assert b.attn.coords_proj.bias is None and b.attn.coords_proj.weight.shape == (b.attn.proj.weight.shape[0], 3)
    m = _build(lcfg.preset("adanorm_tiny_plain"))
    assert all(b.attn.coords_mode is None and not hasattr(b.attn, "coords_proj")
               for b in m.ptv3_model.modules() if isinstance(b, adanorm.AdaBlock))


def test_cross_attention_family_refuses_by_name_and_a_bad_value_is_a_value_error():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3CA

    for cls, name in ((SimplePolicyPTV3CA, "tiny"), (MotionPlannerPTV3CA, "mp_tiny")):
        for mode in ("qk", "qkv"):
            cfg = lcfg.preset(name)
            cls(cfg)
            cfg.ptv3_config.add_coords_in_attn = mode
            with pytest.raises(NotImplementedError) as e:
                cls(cfg)
            assert str(e.value) == ("lotus-hip builds the published 3D-LOTUS configuration family only; unsupported: "
                                    "['add_coords']")
    for name in ("tiny", "adanorm_tiny", "concat_tiny", "mp_ada_tiny"):
        for bad in ("qv", "QK", True, 1, "all"):
            cfg = lcfg.preset(name)
            cfg.ptv3_config.add_coords_in_attn = bad
            with pytest.raises(ValueError, match="add_coords_in_attn"):
                _build(cfg)


def test_bf16_storage_keeps_refusing():
    m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny_qk"))
    m.act_storage = "bf16"
    with pytest.raises(NotImplementedError, match="act_storage"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


@pytest.mark.parametrize("name", ["adanorm_tiny_qk", "concat_tiny_qkv", "mp_ada_tiny_qkv"])
def test_checkpoints_load_strictly_both_ways(name):
    """The reference's key layout (the fixture's state_layout) -> load_state_dict(strict=True) into our model, and our
    state_dict() back into a module tree with exactly those keys."""
    from weights_util import seeded_state_dict

    case = {"adanorm_tiny_qk": "coord_adanorm_tiny_qk_train", "concat_tiny_qkv": "coord_concat_tiny_qkv_train",
            "mp_ada_tiny_qkv": "coord_mp_ada_tiny_qkv_train"}[name]
    layout = json.loads(str(cu.load(case)["state_layout"]))
    ref_sd = {k: (torch.zeros(shape, dtype=torch.long) if k.endswith("num_batches_tracked") else torch.full(shape, 0.25))
              for k, shape in layout}
    m = _build(lcfg.preset(name))
    m.load_state_dict(ref_sd, strict=True)
    assert all(float(v.float().mean()) == 0.25 for k, v in m.state_dict().items() if "coords_proj" in k)
    sd = seeded_state_dict(m.state_dict(), 5, "scaled")
    assert sorted([k, list(v.shape)] for k, v in sd.items()) == sorted(layout)   # (seeded_state_dict walks the keys sorted)
    m2 = _build(lcfg.preset(name))
    m2.load_state_dict(sd, strict=True)
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    # a checkpoint of the model without the term is refused by name, and the other way round
    base = _build(lcfg.preset(BASE[name]))
    with pytest.raises(RuntimeError, match="coords_proj"):
        m.load_state_dict(base.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="coords_proj"):
        base.load_state_dict(sd, strict=True)


def test_node_refuses_half_given_coordinates():
    """SelfAttnFn with coord but without cproj / with another mode: refused before anything is launched."""
    from robot_3dlotus_amd import ops

    x = torch.zeros(4, 8)
    w = torch.zeros(8)
    args = (x, w, w, torch.zeros(24, 8), torch.zeros(24), None, None, None, None, torch.zeros(8, 8), w, None, 2, 0.0, 0, 0.0, None,
            0.0, None, None, 0)
    with pytest.raises(ValueError, match="cmode"):
        ops.SelfAttnFn.apply(*args, torch.zeros(4, 3), torch.zeros(8, 3), "all")
    with pytest.raises(ValueError, match="cmode"):
        ops.SelfAttnFn.apply(*args, torch.zeros(4, 3), None, "qk")


@pytest.mark.reference
@pytest.mark.parametrize("name", ["coord_adanorm_tiny_qk_train", "coord_concat_tiny_qkv_train", "coord_mp_ada_tiny_qkv_train"])
def test_fixture_regenerates_bit_for_bit(name, tmp_path):
    """One fixture per class, from the imported reference's own model (the files hold data only)."""
    import sys

    sys.path.insert(0, cu.GOLDEN_DIR)
    import make_golden_coordattn as mk

    new = dict(np.load(mk.run_case(name, str(tmp_path))))
    old = cu.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f"), k   # (NaN = padding of short gradient heads)


def test_fixture_sizes():
    for name, peer in cu.SIZE_PEER.items():
        a, b = (os.path.getsize(os.path.join(cu.GOLDEN_DIR, n + ".npz")) for n in (name, peer))
        assert a <= b, (name, a, peer, b)
