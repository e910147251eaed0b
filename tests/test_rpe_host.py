"""CPU checks of enable_flash False / enable_rpe True (PointTransformerV3/model.py:307-326, :400-408, :469-472, :499-527): the
three model classes built with the new presets — parameter names, shapes and registration order against the state layouts the
reference's own models recorded in the fixtures —, the option rule (what is a ValueError, what keeps refusing by name), the
presets, the per-level patch size and the host plan of the patch tables against the restatement on oracle/front_end.py, the
float64 restatement of the term and of its table gradient against torch autograd on the reference's own expressions, and the
argument refusals, the route record and the workspace query of csrc/attention_rpe.hip (answered before any launch)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import rpe_util as ru
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg
from robot_3dlotus_amd.policy import MODEL_FACTORY, SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA, SimplePolicyPTV3Concat

E_ARG = -1
NEW_PRESETS = ("adanorm_tiny_dense", "adanorm_tiny_rpe", "adanorm_tiny_plain_rpe", "concat_tiny_rpe", "mp_ada_tiny_rpe",
               "adanorm_yaml_rpe")
BASE = {"adanorm_tiny_dense": "adanorm_tiny", "adanorm_tiny_rpe": "adanorm_tiny", "adanorm_tiny_plain_rpe": "adanorm_tiny_plain",
        "concat_tiny_rpe": "concat_tiny", "mp_ada_tiny_rpe": "mp_ada_tiny", "adanorm_yaml_rpe": "adanorm_yaml"}
# ptv3_config of every preset that existed before the switches were read: the four keys as shipped
OLD_PRESETS = ("v1", "tiny", "peract", "tinydeep", "tinyctx", "mp", "mp_tiny", "mp_tinyctx", "adanorm_v1", "adanorm_tiny",
               "adanorm_tinyctx", "adanorm_yaml", "adanorm_tiny_plain", "adanorm_v1_plain", "tiny_reg", "v1_reg", "adanorm_tiny_reg",
               "mp_yaml", "mp_ada_tiny", "concat_yaml", "concat_tiny", "adanorm_tiny_qk", "adanorm_tiny_qkv", "adanorm_yaml_qk",
               "concat_tiny_qk", "concat_tiny_qkv", "mp_ada_tiny_qkv")
SHIPPED = {"enable_flash": True, "enable_rpe": False, "upcast_attention": False, "upcast_softmax": False}


def _layout(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def _build(cfg):
    return MODEL_FACTORY[cfg.model_class](cfg)


def test_rows_self_check():
    assert ru.self_check() == len(ru.ROWS) >= 9


# ------------------------------------------------------------------------------------------------- modules and the option rule
@pytest.mark.parametrize("case", list(ru.CASES))
def test_state_dict_layout_equals_the_fixtures(case):
    """Names, shapes and registration order of the reference's own model: rpe.rpe_table [93, H] sits behind proj in every
    attention (model.py:386-394), and only with enable_rpe."""
    layout = json.loads(str(ru.load(case)["state_layout"]))
    cfg = ru.case_config(case)
    m = _build(cfg)
    assert _layout(m) == layout
    tabs = [k for k, _ in layout if k.endswith(".attn.rpe.rpe_table")]
    blocks = sum(cfg.ptv3_config.enc_depths) + sum(cfg.ptv3_config.dec_depths)
    assert len(tabs) == (blocks if ru.case_has_rpe(case) else 0) == sum("rpe" in k for k, _ in layout)
    keys = [k for k, _ in layout]
    sd = m.state_dict()
    for k in tabs:
        H = sd[k.replace("rpe.rpe_table", "proj.weight")].shape[0] // (sd[k.replace("rpe.rpe_table", "q_norm.weight")].shape[0]
                                                                         if cfg.ptv3_config.qk_norm else 1)
        assert list(sd[k].shape)[0] == 93 == 3 * (2 * ru.pos_bnd(128) + 1)
        if cfg.ptv3_config.qk_norm:
            assert sd[k].shape[1] == H
        assert keys[keys.index(k) - 1].endswith(".attn.proj.bias"), k
    assert [n for n, _ in m.named_parameters() if "rpe" in n] == tabs
    if case == "rpe_adanorm_yaml_rpe_eval":
        assert len(layout) == 661 + 22


@pytest.mark.parametrize("name", NEW_PRESETS)
def test_presets_build_and_differ_from_their_base_by_the_switches_only(name):
    from robot_3dlotus_amd import adanorm, concat
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm

    cfg, base = lcfg.preset(name), lcfg.preset(BASE[name])
    rpe = not name.endswith("dense")
    assert cfg.ptv3_config.enable_flash is False and cfg.ptv3_config.enable_rpe is rpe
    cfg2 = lcfg.preset(name)
    cfg2.ptv3_config.enable_flash, cfg2.ptv3_config.enable_rpe = True, False
    assert cfg2 == base
    if name == "adanorm_yaml_rpe":
        assert cfg == lcfg.load_model_config(None, ["ptv3_config.enable_flash", "False", "ptv3_config.enable_rpe", "True"])
        assert cfg.ptv3_config.qk_norm is False
        return
    m = _build(cfg)
    assert isinstance(m, {"a": SimplePolicyPTV3AdaNorm, "c": SimplePolicyPTV3Concat, "m": MotionPlannerPTV3AdaNorm}[name[0]])
    bb = m.ptv3_model
    assert bb.dense_attention and bb.enable_flash is False and bb.enable_rpe is rpe and bb.frontend.min_count_patches is True
    blocks = [b for b in bb.modules() if isinstance(b, (adanorm.AdaBlock, concat.PlainBlock))]
    assert len(blocks) == 3
    for b in blocks:
        if rpe:
            t = b.attn.rpe.rpe_table
            assert isinstance(t, torch.nn.Parameter) and t.dtype == torch.float32 and t.requires_grad
            assert tuple(t.shape) == (93, b.num_heads) and b.attn.rpe.pos_bnd == 15
            assert 0.01 < float(t.detach().std()) < 0.03   # trunc_normal_(std=0.02) of RPE.__init__: _init_weights leaves it
        else:
            assert b.attn.rpe is None
    with_t, without = _layout(m), _layout(_build(base))
    assert [e for e in with_t if "rpe" not in e[0]] == without
    assert _build(base).ptv3_model.frontend.min_count_patches is False
    # the two upcast switches are no-ops with enable_flash False
    cfg.ptv3_config.upcast_attention = cfg.ptv3_config.upcast_softmax = True
    assert _layout(_build(cfg)) == with_t


def test_table_rows_follow_the_configured_patch_size():
    from robot_3dlotus_amd import ops, ptv3

    assert [ops.rpe_bound(p) for p in (128, 64, 100, 16)] == [ru.pos_bnd(p) for p in (128, 64, 100, 16)] == [15, 12, 14, 7]
    a = ptv3._Attn(32, 4, True, False, 64)
    assert tuple(a.rpe.rpe_table.shape) == (3 * 25, 4)
    assert list(dict(a.named_parameters())) == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "rpe.rpe_table",
                                                "q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias"]


@pytest.mark.parametrize("name", OLD_PRESETS)
def test_existing_presets_keep_the_shipped_switches(name):
    p3 = lcfg.preset(name).ptv3_config
    assert {k: p3[k] for k in SHIPPED} == SHIPPED


@pytest.mark.parametrize("name", ["adanorm_tiny", "concat_tiny", "mp_ada_tiny"])
def test_value_errors_of_the_reference_rules(name):
    """enable_rpe / upcast_* True with enable_flash True: the reference's asserts (model.py:365-374), here ValueErrors."""
    cfg = lcfg.preset(name)
    cfg.ptv3_config.enable_rpe = True
    with pytest.raises(ValueError, match="Set enable_rpe to False when enable Flash Attention"):
        _build(cfg)
    for k in ("upcast_attention", "upcast_softmax"):
        cfg = lcfg.preset(name)
        cfg.ptv3_config[k] = True
        with pytest.raises(ValueError, match=f"Set {k} to False when enable Flash Attention"):
            _build(cfg)
        cfg.ptv3_config.enable_flash = False   # accepted, a no-op
        _build(cfg)


def test_cross_attention_family_and_scaled_cosine_keep_refusing_by_name():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3CA

    msg = "lotus-hip builds the published 3D-LOTUS configuration family only; unsupported: "
    for cls, name in ((SimplePolicyPTV3CA, "tiny"), (MotionPlannerPTV3CA, "mp_tiny")):
        for keys, bad in (({"enable_flash": False}, "['not_flash']"), ({"enable_rpe": True}, "['enable_rpe']"),
                          ({"enable_flash": False, "enable_rpe": True}, "['enable_rpe', 'not_flash']")):
            cfg = lcfg.preset(name)
            cls(cfg)
            cfg.ptv3_config.update(keys)
            with pytest.raises(NotImplementedError) as e:
                cls(cfg)
            assert str(e.value) == msg + bad
    for name in ("adanorm_tiny", "adanorm_tiny_rpe", "concat_tiny_rpe", "mp_ada_tiny_rpe", "tiny"):
        cfg = lcfg.preset(name)
        cfg.ptv3_config.scaled_cosine_attn = True
        with pytest.raises(NotImplementedError) as e:
            _build(cfg)
        assert str(e.value) == msg + "['scaled_cosine_attn']"


def test_storage_and_precision_refusals_at_forward():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm

    for name in ("adanorm_tiny_dense", "adanorm_tiny_rpe", "concat_tiny_rpe", "mp_ada_tiny_rpe"):
        m = _build(lcfg.preset(name))
        m.act_storage = "bf16"
        with pytest.raises(NotImplementedError, match="act_storage"):
            m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    for name, cls in (("adanorm_tiny_rpe", SimplePolicyPTV3AdaNorm), ("concat_tiny_rpe", SimplePolicyPTV3Concat),
                      ("mp_ada_tiny_rpe", MotionPlannerPTV3AdaNorm)):
        for mode in ("bf16", "bf16x3"):
            m = _build(lcfg.preset(name))
            assert isinstance(m, cls)
            m.gemm_precision = mode
            with pytest.raises(NotImplementedError, match="gemm_precision None / 'fp32'"):
                m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    m = _build(lcfg.preset("adanorm_tiny_rpe"))   # (qk_norm True: it is the term that refuses)
    m.gemm_precision = "bf16"
    with pytest.raises(NotImplementedError, match="enable_rpe=True"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


@pytest.mark.parametrize("name", ["adanorm_tiny_rpe", "concat_tiny_rpe", "mp_ada_tiny_rpe"])
def test_checkpoints_load_strictly_both_ways(name):
    case = "rpe_" + name + "_train"
    layout = json.loads(str(ru.load(case)["state_layout"]))
    ref_sd = {k: (torch.zeros(shape, dtype=torch.long) if k.endswith("num_batches_tracked") else torch.full(shape, 0.25))
              for k, shape in layout}
    m = _build(lcfg.preset(name))
    m.load_state_dict(ref_sd, strict=True)
    assert all(float(v.float().mean()) == 0.25 for k, v in m.state_dict().items() if "rpe" in k)
    sd = ru.case_state_dict(m.state_dict(), 5)
    assert sorted([k, list(v.shape)] for k, v in sd.items()) == sorted(layout)
    base = _build(lcfg.preset(BASE[name]))
    with pytest.raises(RuntimeError, match="rpe_table"):
        m.load_state_dict(base.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="rpe_table"):
        base.load_state_dict(sd, strict=True)


def test_node_refuses_a_table_of_the_wrong_shape():
    from robot_3dlotus_amd import ops

    x = torch.zeros(4, 8)
    w = torch.zeros(8)
    args = (x, w, w, torch.zeros(24, 8), torch.zeros(24), None, None, None, None, torch.zeros(8, 8), w, None, 2, 0.0, 0, 0.0, None,
            0.0, None, None, 0, None, None, None)
    with pytest.raises(ValueError, match="rpe_table"):
        ops.SelfAttnFn.apply(*args, torch.zeros(93, 4), 15)
    with pytest.raises(ValueError, match="rpe_table"):
        ops.SelfAttnFn.apply(*args, torch.zeros(93, 2), 14)


# ------------------------------------------------------------------------------------------------- per-level K and the patch tables
@pytest.mark.parametrize("counts", ru.PLAN_COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_host_plan_against_the_restatement(counts):
    from robot_3dlotus_amd.frontend import FrontEnd

    dense, flash = FrontEnd(1, min_count_patches=True), FrontEnd(1)
    K, off, offp, tiles, blocks = dense.patch_plan(counts)
    assert K == ru.dense_patch_size(counts, 128) == dense.level_patch_size(counts) and 1 <= K <= 128
    t = ru.patch_tables(counts, K)
    for got, want in ((off, t["off"]), (offp, t["offp"]), (tiles, t["tiles"]), (blocks, t["blocks"])):
        np.testing.assert_array_equal(got, want)
    assert (tiles[:, 1] == K).all() and int(offp[-1]) == t["npad"] and t["npad"] % K == 0   # every patch has exactly K rows
    want_K = {(128,): 128, (300, 131): 128, (77, 80): 77, (5, 9, 5): 5, (1, 3): 1, (4096, 200): 128}[tuple(counts)]
    assert K == want_K
    # borrowed rows: the tail patch of a cloud longer than K repeats the rows before it (position - K)
    pad = t["pad"]
    for e in t["ext_pos"]:
        assert pad[e] == pad[e - K]
    # with the mode off the plan is today's: the patch size is the configured one whatever the counts
    K0, off0, offp0, tiles0, blocks0 = flash.patch_plan(counts)
    t0 = ru.patch_tables(counts, 128)
    assert K0 == 128 == flash.level_patch_size(counts)
    for got, want in ((off0, t0["off"]), (offp0, t0["offp"]), (tiles0, t0["tiles"]), (blocks0, t0["blocks"])):
        np.testing.assert_array_equal(got, want)
    if K == 128:
        for a, b in zip((off, offp, tiles, blocks), (off0, offp0, tiles0, blocks0)):
            np.testing.assert_array_equal(a, b)


def test_level_carries_its_patch_size():
    from robot_3dlotus_amd.frontend import FrontEnd, Level

    assert "K" in Level.__slots__
    assert FrontEnd(2, patch_size=64, min_count_patches=True).level_patch_size([70, 65]) == 64
    assert FrontEnd(2, patch_size=64, min_count_patches=True).level_patch_size([70, 3]) == 3
    assert FrontEnd(2, patch_size=64).level_patch_size([70, 3]) == 64


# ------------------------------------------------------------------------------------------------- the restatement against autograd
def test_restatement_of_the_term_and_of_its_gradient_against_autograd():
    """position_term / table_grad / attention_ref against torch float64 autograd on the reference's own expressions: the table
    lookup of RPE.forward (model.py:317-326: clamp, shift, per-axis stride, index_select, sum over the axes) on get_rel_pos
    (:400-408), added to (q * scale) @ k^T before the softmax (:518-527)."""
    g = torch.Generator().manual_seed(7)
    K, H, d, bnd, P = 9, 3, 4, 2, 2
    num = 2 * bnd + 1
    grid = torch.randint(0, 7, (P * K, 3), generator=g)
    q, k, v = (torch.randn(P, H, K, d, generator=g).double() for _ in range(3))
    dout = torch.randn(P, H, K, d, generator=g).double()
    table = torch.randn(3 * num, H, generator=g).double().requires_grad_(True)
    # the reference's expressions
    gc = grid.reshape(-1, K, 3)
    rel = gc.unsqueeze(2) - gc.unsqueeze(1)
    idx = rel.clamp(-bnd, bnd) + bnd + torch.arange(3) * num
    term = table.index_select(0, idx.reshape(-1)).view(idx.shape + (-1,)).sum(3).permute(0, 3, 1, 2)   # (P, H, K, K)
    attn = (q * d ** -0.5) @ k.transpose(-2, -1) + term
    attn.retain_grad()
    out = torch.softmax(attn, -1) @ v
    out.backward(dout)
    for p in range(P):
        gp = grid[p * K:(p + 1) * K].numpy()
        assert np.abs(ru.position_term(gp, gp, table.detach().numpy(), bnd) - term[p].detach().numpy()).max() < 1e-14
    dt = sum(ru.table_grad(attn.grad[p].numpy(), grid[p * K:(p + 1) * K].numpy(), grid[p * K:(p + 1) * K].numpy(), bnd)
             for p in range(P))
    assert np.abs(dt - table.grad.numpy()).max() < 1e-12 and np.abs(table.grad.numpy()).max() > 1e-3
    # rows no pair selects stay exact zeros
    sel = np.zeros(3 * num, bool)
    sel[np.unique(idx.numpy())] = True
    assert (dt[~sel] == 0).all()
    # attention_ref (what the GPU rows are compared with) is the same function
    qkv = torch.cat([t.permute(0, 2, 1, 3).reshape(P * K, H * d) for t in (q, k, v)], 1).requires_grad_(True)
    t2 = table.detach().clone().requires_grad_(True)
    o2, lse = ru.attention_ref(qkv, np.arange(P * K), np.arange(P * K), np.arange(0, P * K + 1, K), grid.numpy(), t2, bnd, H)
    assert float((o2 - out.permute(0, 2, 1, 3).reshape(P * K, H * d)).detach().abs().max()) < 1e-12
    o2.backward(dout.permute(0, 2, 1, 3).reshape(P * K, H * d))
    assert float((t2.grad - table.grad).abs().max()) < 1e-12
    assert float((lse.reshape(P, K, H).permute(0, 2, 1) - torch.logsumexp(attn, -1)).detach().abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------- the entry points on the host
def _route():
    out = (ctypes.c_int * 8)()
    _capi.call_raw("lotus_attention_last_route", ctypes.addressof(out))
    return list(out)


def test_refusals_before_any_launch_and_the_route_record():
    """Every refusal is answered by the argument checks (LOTUS_E_ARG with the entry point named), so no pointer is ever read: the
    buffers here are host memory.  A refused call leaves the route record as it was."""
    F = _capi.lib().fn
    y = np.zeros(4096, np.float32)
    buf = ctypes.c_void_p(y.ctypes.data)
    odd = ctypes.c_void_p(y.ctypes.data + 4)
    before = _route()

    def fwd(**kw):
        a = dict(q=buf, kv=buf, tiles=buf, ntiles=1, qn=(None,) * 4, out=buf, H=2, d=16, drop=0.0, grid=buf, table=buf, bnd=15)
        a.update(kw)
        return F["lotus_attention_rpe_fwd"](a["q"], 96, 0, a["kv"], 96, 32, 64, None, None, None, a["tiles"], a["ntiles"], *a["qn"],
                                            a["out"], 32, buf, a["H"], a["d"], 0.25, 1e-6, a["drop"], 1, a["grid"], a["table"],
                                            a["bnd"], None)

    def bwd(**kw):
        a = dict(q=buf, kv=buf, tiles=buf, blocks=buf, nblocks=1, qn=(None,) * 4, out=buf, dout=buf, lse=buf, dq=buf, dkv=buf,
                 dv_off=64, kext=None, ext_pos=None, n_extra=0, extra=None, dn=(None,) * 4, H=2, d=16, drop=0.0, grid=buf, table=buf,
                 bnd=15, dtable=buf, ws=buf, ws_bytes=1 << 14)
        a.update(kw)
        return F["lotus_attention_rpe_bwd"](a["q"], 96, 0, a["kv"], 96, 32, 64, None, buf, None, a["tiles"], a["blocks"],
                                            a["nblocks"], *a["qn"], a["out"], a["dout"], 32, a["lse"], a["dq"], 96, 0, a["dkv"], 96,
                                            32, a["dv_off"], 0, a["kext"], a["ext_pos"], a["n_extra"], a["extra"], *a["dn"], 0, a["H"],
                                            a["d"], 0.25, 1e-6, a["drop"], 1, a["grid"], a["table"], a["bnd"], a["dtable"], a["ws"],
                                            a["ws_bytes"], None)

    def refused(rc, who, text):
        err = _capi.lib().last_error()
        assert rc == E_ARG and who in err and text in err, (rc, err)
        assert _route() == before

    for f, who, ptrs in ((fwd, "lotus_attention_rpe_fwd", ("q", "kv", "tiles", "out")),
                         (bwd, "lotus_attention_rpe_bwd", ("q", "kv", "tiles", "blocks", "out", "dout", "lse", "dq", "dkv", "dtable"))):
        for k in ptrs:
            refused(f(**{k: None}), who, "null pointer")
        refused(f(grid=None), who, "a table without grid")
        refused(f(table=None), who, "null pointer (table, grid)")
        refused(f(bnd=-1), who, "bnd = -1")
        refused(f(bnd=16), who, "bnd = 16 > 15")
        for H, d in ((0, 16), (2, 0), (2, 6), (2, 36), (2, -4)):
            refused(f(H=H, d=d), who, f"H = {H}, d = {d}")
        refused(f(drop=1.0), who, "drop_p")
        refused(f(drop=-0.1), who, "drop_p")
        refused(f(qn=(buf, buf, buf, None)), who, "all given or all null")
        refused(f(qn=(buf, None, None, None)), who, "all given or all null")
    refused(fwd(ntiles=-1), "lotus_attention_rpe_fwd", "ntiles = -1")
    refused(bwd(nblocks=-1), "lotus_attention_rpe_bwd", "nblocks = -1")
    refused(bwd(qn=(buf,) * 4), "lotus_attention_rpe_bwd", "null norm gradient")
    refused(bwd(qn=(buf,) * 4, dn=(buf, buf, buf, None)), "lotus_attention_rpe_bwd", "null norm gradient")
    refused(bwd(ws=None), "lotus_attention_rpe_bwd", "workspace")
    refused(bwd(ws=odd), "lotus_attention_rpe_bwd", "workspace")
    refused(bwd(ws_bytes=_capi.query("lotus_attention_rpe_bwd_workspace", 1, 2, 15) - 1), "lotus_attention_rpe_bwd", "workspace")
    refused(bwd(kext=buf, n_extra=3), "lotus_attention_rpe_bwd", "borrowed-row buffer")
    refused(bwd(kext=buf, n_extra=3, extra=buf), "lotus_attention_rpe_bwd", "borrowed-row buffer")
    refused(bwd(kext=buf, n_extra=3, extra=buf, ext_pos=buf, dv_off=60), "lotus_attention_rpe_bwd", "adjacent k|v column blocks")
    # nothing to do: no launch, no error, the record stays
    assert fwd(ntiles=0) == 0 and _route() == before


def test_workspace_query():
    q = lambda nb, H, bnd: _capi.query("lotus_attention_rpe_bwd_workspace", nb, H, bnd)   # noqa: E731
    for nb, H, bnd in ((1, 1, 0), (3, 2, 15), (7, 32, 15), (100, 4, 2), (0, 4, 15)):
        assert q(nb, H, bnd) == nb * H * (4 * 32 * 4 + 3 * (2 * bnd + 1) * 8)
    assert q(-1, 2, 15) == 0 and q(2, 0, 15) == 0 and q(2, 2, -1) == 0
    assert q(3, 2, 15) % 8 == 0


def test_kernels_are_fp32_only_and_outside_the_twin_build():
    from robot_3dlotus_amd import ops

    protos = _capi.parse_header()
    for name in ("lotus_attention_rpe_fwd", "lotus_attention_rpe_bwd", "lotus_attention_rpe_bwd_workspace"):
        assert name in protos and "lotus_b16_" + name[6:] not in protos, name
    assert (ops.ATTN_RPE_FWD, ops.ATTN_RPE_BWD) == (6, 7)
    hdr = open(_capi.HEADER_PATH.replace("include/lotus_hip.h", "robot-3dlotus_amd/csrc/attn_route.h")).read()
    assert "#define LOTUS_ATTN_RPE_FWD 6" in hdr and "#define LOTUS_ATTN_RPE_BWD 7" in hdr
    _capi.BF16 = True
    try:
        with pytest.raises(AssertionError, match="fp32 activation storage"):
            ops.attention_rpe_fwd(*([None] * 21))
    finally:
        _capi.BF16 = False


@pytest.mark.reference
@pytest.mark.parametrize("name", ["rpe_adanorm_tiny_rpe_train", "rpe_concat_tiny_rpe_train", "rpe_mp_ada_tiny_rpe_train"])
def test_fixture_regenerates_bit_for_bit(name, tmp_path):
    """One fixture per class, from the imported reference's own model (the files hold data only)."""
    import sys

    sys.path.insert(0, ru.GOLDEN_DIR)
    import make_golden_rpe as mk

    new = dict(np.load(mk.run_case(name, str(tmp_path))))
    old = ru.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f"), k
