"""CPU checks of patch sizes above 128 (PointTransformerV3/model.py:529-551; csrc/attention_long.hip): the rows' self-check and the
float64 restatement against torch autograd, every argument refusal of lotus_attention_long_fwd / _bwd without a device and the
route record, the workspace query, the constructor rules by exact message, FrontEnd.patch_plan at K = 256 against the restatement
of get_padding_and_inverse, the presets, and the state_dict keys against the K = 128 presets."""
import ctypes

import numpy as np
import pytest
import torch

import longattn_util as lu
import rpe_util as ru
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg, ops
from robot_3dlotus_amd.policy import MODEL_FACTORY, SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA, SimplePolicyPTV3Concat

E_ARG, E_LAUNCH = -1, -2
NEW_PRESETS = ("adanorm_tiny_p256", "adanorm_tiny_plain_p256", "concat_tiny_p256", "mp_ada_tiny_p256", "adanorm_yaml_p1024")
BASE = {"adanorm_tiny_p256": "adanorm_tiny", "adanorm_tiny_plain_p256": "adanorm_tiny_plain", "concat_tiny_p256": "concat_tiny",
        "mp_ada_tiny_p256": "mp_ada_tiny", "adanorm_yaml_p1024": "adanorm_yaml"}
MSG = "lotus-hip builds the published 3D-LOTUS configuration family only; unsupported: "


def _build(cfg):
    return MODEL_FACTORY[cfg.model_class](cfg)


def test_rows_self_check():
    assert lu.self_check() == len(lu.ROWS) >= 8


# ------------------------------------------------------------------------------------------------- the constructor rules
def test_tiny_preset_at_256_builds():
    """Fails without the feature: NotImplementedError ... unsupported: ['patch_ne_128']."""
    m = _build(lcfg.preset("adanorm_tiny_p256"))
    assert isinstance(m, SimplePolicyPTV3AdaNorm) and m.ptv3_model.frontend.K == 256 and m.ptv3_model.patch_size == 256


@pytest.mark.parametrize("name", NEW_PRESETS)
def test_presets_build_with_the_keys_of_their_base(name):
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm

    cfg, base = lcfg.preset(name), lcfg.preset(BASE[name])
    K = 1024 if name.endswith("p1024") else 256
    p3 = cfg.ptv3_config
    assert list(p3.enc_patch_size) == [K] * len(p3.enc_depths) and list(p3.dec_patch_size) == [K] * len(p3.dec_depths)
    assert all(p <= 128 for p in list(base.ptv3_config.enc_patch_size) + list(base.ptv3_config.dec_patch_size))
    assert {k: v for k, v in p3.items() if "patch_size" not in k} == {k: v for k, v in base.ptv3_config.items() if "patch_size" not in k}
    m, mb = _build(cfg), _build(base)
    want = {"adanorm": SimplePolicyPTV3AdaNorm, "concat_": SimplePolicyPTV3Concat, "mp_ada_": MotionPlannerPTV3AdaNorm}[name[:7]]
    assert type(m) is want and type(mb) is want
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in mb.state_dict().items()]
    assert m.ptv3_model.frontend.K == K and m.ptv3_model.long_patches


def test_cross_attention_family_keeps_refusing_exactly():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3CA

    for cls, name in ((SimplePolicyPTV3CA, "tiny"), (MotionPlannerPTV3CA, "mp_tiny")):
        for K in (256, 512, 1024, 129):
            cfg = lcfg.preset(name)
            cls(cfg)
            cfg.ptv3_config.enc_patch_size = [K] * len(cfg.ptv3_config.enc_depths)
            cfg.ptv3_config.dec_patch_size = [K] * len(cfg.ptv3_config.dec_depths)
            with pytest.raises(NotImplementedError) as e:
                cls(cfg)
            assert str(e.value) == MSG + "['patch_ne_128']"
    from robot_3dlotus_amd import ptv3
    assert ptv3.PointTransformerV3CA.long_patches is False


@pytest.mark.parametrize("name", ["adanorm_tiny", "concat_tiny", "mp_ada_tiny"])
def test_option_rules_by_message(name):
    def with_patches(enc, dec, **keys):
        cfg = lcfg.preset(name)
        cfg.ptv3_config.enc_patch_size, cfg.ptv3_config.dec_patch_size = enc, dec
        cfg.ptv3_config.update(keys)
        return cfg

    for K in (256, 512, 1024):
        m = _build(with_patches([K, K], [K]))
        assert m.ptv3_model.frontend.K == K and not m.ptv3_model.frontend.min_count_patches
        m = _build(with_patches([K, K], [K], enable_flash=False))    # only the patching changes
        assert m.ptv3_model.frontend.K == K and m.ptv3_model.frontend.min_count_patches
        m = _build(with_patches([K, K], [K], add_coords_in_attn="qk"))
        assert m.ptv3_model.add_coords == "qk"
        with pytest.raises(NotImplementedError) as e:                # the table lookups are not in the long kernels
            _build(with_patches([K, K], [K], enable_flash=False, enable_rpe=True))
        assert str(e.value) == MSG + "['rpe_long_patch']"
    with pytest.raises(NotImplementedError) as e:
        _build(with_patches([256, 128], [256]))
    assert str(e.value) == "all patch sizes must be equal"
    with pytest.raises(NotImplementedError) as e:
        _build(with_patches([256, 256], [128]))
    assert str(e.value) == "all patch sizes must be equal"
    for K in (129, 200, 384, 768, 2048):   # above 128: 256, 512, 1024 and nothing else
        with pytest.raises(ValueError) as e:
            _build(with_patches([K, K], [K]))
        assert str(e.value) == f"patch_size={K}: above 128 the patch attention is built for (256, 512, 1024) (csrc/attention_long.hip)"
    _build(with_patches([128, 128], [128], enable_flash=False, enable_rpe=True))   # at 128 the term is built as before
    _build(with_patches([64, 64], [64]))


def test_frontend_patch_sizes():
    from robot_3dlotus_amd.frontend import FrontEnd, LONG_PATCH_SIZES

    assert LONG_PATCH_SIZES == (256, 512, 1024)
    for K in (1, 5, 77, 128, 256, 512, 1024):
        assert FrontEnd(1, patch_size=K).K == K
    for K in (129, 255, 257, 384, 1023, 1025, 2048, 4096):
        with pytest.raises(ValueError, match=f"patch_size={K}: above 128"):
            FrontEnd(1, patch_size=K)
    # enable_flash False: K_s = min(K, fewest points)
    fe = FrontEnd(1, patch_size=256, min_count_patches=True)
    assert fe.level_patch_size([700, 300]) == 256 and fe.level_patch_size([700, 200]) == 200 and fe.level_patch_size([700, 90]) == 90
    assert FrontEnd(1, patch_size=1024, min_count_patches=True).level_patch_size([5000, 1500]) == 1024


def test_storage_and_precision_refusals_at_forward():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm

    for name in ("adanorm_tiny_p256", "concat_tiny_p256", "mp_ada_tiny_p256"):
        m = _build(lcfg.preset(name))
        m.act_storage = "bf16"
        with pytest.raises(NotImplementedError, match="act_storage='bf16' is not built"):
            m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    for name, cls in (("adanorm_tiny_p256", SimplePolicyPTV3AdaNorm), ("concat_tiny_p256", SimplePolicyPTV3Concat),
                      ("mp_ada_tiny_p256", MotionPlannerPTV3AdaNorm)):
        for mode in ("bf16", "bf16x3"):
            m = _build(lcfg.preset(name))
            assert isinstance(m, cls)
            m.gemm_precision = mode
            with pytest.raises(NotImplementedError, match="gemm_precision None / 'fp32'"):
                m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    m = _build(lcfg.preset("adanorm_tiny_p256"))   # (qk_norm True, no RPE: it is the patch size that refuses)
    m.gemm_precision = "bf16"
    with pytest.raises(NotImplementedError) as e:
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    assert str(e.value) == ("SimplePolicyPTV3AdaNorm with patch sizes above 128 is built for gemm_precision None / 'fp32' only, "
                            "got 'bf16'")
    m = _build(lcfg.preset("mp_ada_tiny"))         # (at 128 the planner keeps its own rule: qk_norm False)
    m.gemm_precision = "bf16"
    with pytest.raises(NotImplementedError, match="qk_norm=False"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


# ------------------------------------------------------------------------------------------------- the host plan
@pytest.mark.parametrize("counts", lu.PLAN_COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_host_plan_at_256_against_the_restatement(counts):
    from robot_3dlotus_amd.frontend import FrontEnd

    K, off, offp, tiles, blocks = FrontEnd(1, patch_size=256).patch_plan(counts)
    assert K == 256
    for got, want in zip((off, offp, tiles, blocks), lu.plan_ref(counts, 256)):
        np.testing.assert_array_equal(got, want)
    want_lens = {(256,): [256], (300, 131): [256, 256, 131], (700, 200): [256, 256, 256, 200], (1, 513): [1, 256, 256, 256]}[tuple(counts)]
    assert tiles[:, 1].tolist() == want_lens and (tiles[:, 0] == tiles[:, 2]).all() and (tiles[:, 1] == tiles[:, 3]).all()
    # a cloud longer than K is padded to a multiple of K and its tail patch borrows from the patch before it
    t = ru.patch_tables(counts, 256)
    c = np.asarray(counts)
    assert int(offp[-1]) == int(np.where(c > 256, (c + 255) // 256 * 256, c).sum()) == t["npad"]
    assert t["n_extra"] == int(offp[-1] - off[-1]) == {(256,): 0, (300, 131): 212, (700, 200): 68, (1, 513): 255}[tuple(counts)]
    for e in t["ext_pos"]:
        assert t["pad"][e] == t["pad"][e - 256]
    # at K <= 128 the plan is what it was
    K0, *plan0 = FrontEnd(1).patch_plan(counts)
    assert K0 == 128
    for got, want in zip(plan0, lu.plan_ref(counts, 128)):
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------- the entry points on the host
def _route():
    out = (ctypes.c_int * 8)()
    _capi.call_raw("lotus_attention_last_route", ctypes.addressof(out))
    return list(out)


def _calls():
    F = _capi.lib().fn
    y = np.zeros(1 << 16, np.float32)
    buf = ctypes.c_void_p(y.ctypes.data + (-y.ctypes.data) % 16)
    odd = ctypes.c_void_p(buf.value + 4)

    def fwd(**kw):
        a = dict(q=buf, kv=buf, tiles=buf, ntiles=1, qn=(None,) * 4, out=buf, H=2, d=16, drop=0.0, len_max=256)
        a.update(kw)
        return F["lotus_attention_long_fwd"](a["q"], 96, 0, a["kv"], 96, 32, 64, None, None, None, a["tiles"], a["ntiles"], *a["qn"],
                                             a["out"], 32, buf, a["H"], a["d"], 0.25, 1e-6, a["drop"], 1, a["len_max"], None)

    def bwd(**kw):
        a = dict(q=buf, kv=buf, tiles=buf, blocks=buf, nblocks=1, qn=(None,) * 4, out=buf, dout=buf, lse=buf, dq=buf, dkv=buf,
                 dv_off=64, kext=None, ext_pos=None, n_extra=0, extra=None, dn=(None,) * 4, H=2, d=16, drop=0.0, len_max=256, npos=256,
                 ws=buf, ws_bytes=1 << 17)
        a.update(kw)
        return F["lotus_attention_long_bwd"](a["q"], 96, 0, a["kv"], 96, 32, 64, None, buf, None, a["tiles"], a["blocks"],
                                             a["nblocks"], *a["qn"], a["out"], a["dout"], 32, a["lse"], a["dq"], 96, 0, a["dkv"], 96,
                                             32, a["dv_off"], 0, a["kext"], a["ext_pos"], a["n_extra"], a["extra"], *a["dn"], 0, a["H"],
                                             a["d"], 0.25, 1e-6, a["drop"], 1, a["len_max"], a["npos"], a["ws"], a["ws_bytes"], None)
    return fwd, bwd, buf, odd


def test_refusals_before_any_launch_and_the_route_record():
    """Every refusal is answered by the argument checks (LOTUS_E_ARG with the entry point named), so no pointer is ever read: the
    buffers here are host memory.  A refused call leaves the route record as it was."""
    fwd, bwd, buf, odd = _calls()
    before = _route()

    def refused(rc, who, text):
        err = _capi.lib().last_error()
        assert rc == E_ARG and who in err and text in err, (rc, err)
        assert _route() == before

    for f, who, ptrs in ((fwd, "lotus_attention_long_fwd", ("q", "kv", "tiles", "out")),
                         (bwd, "lotus_attention_long_bwd", ("q", "kv", "tiles", "blocks", "out", "dout", "lse", "dq", "dkv"))):
        for k in ptrs:
            refused(f(**{k: None}), who, "null pointer")
        for H, d in ((0, 16), (2, 0), (2, 6), (2, 36), (2, -4)):
            refused(f(H=H, d=d), who, f"H = {H}, d = {d}")
        refused(f(len_max=1025), who, "len_max = 1025 > 1024")     # a tile above LOTUS_ATTN_LONG_MAX
        refused(f(len_max=4096), who, "len_max = 4096 > 1024")
        refused(f(len_max=0), who, "len_max = 0")
        refused(f(drop=1.0), who, "drop_p")
        refused(f(drop=-0.1), who, "drop_p")
        refused(f(qn=(buf, buf, buf, None)), who, "all given or all null")
        refused(f(qn=(buf, None, None, None)), who, "all given or all null")
    refused(fwd(ntiles=-1), "lotus_attention_long_fwd", "ntiles = -1")
    refused(bwd(nblocks=-1), "lotus_attention_long_bwd", "nblocks = -1")
    refused(bwd(npos=-1), "lotus_attention_long_bwd", "npos = -1")
    refused(bwd(qn=(buf,) * 4), "lotus_attention_long_bwd", "null norm gradient")
    refused(bwd(qn=(buf,) * 4, dn=(buf, buf, buf, None)), "lotus_attention_long_bwd", "null norm gradient")
    refused(bwd(ws=None), "lotus_attention_long_bwd", "workspace")
    refused(bwd(ws=odd), "lotus_attention_long_bwd", "workspace")
    refused(bwd(ws_bytes=_capi.query("lotus_attention_long_bwd_workspace", 1, 2, 256, 256) - 1), "lotus_attention_long_bwd", "workspace")
    refused(bwd(kext=buf, n_extra=3), "lotus_attention_long_bwd", "borrowed-row buffer")
    refused(bwd(kext=buf, n_extra=3, extra=buf), "lotus_attention_long_bwd", "borrowed-row buffer")
    refused(bwd(kext=buf, n_extra=3, extra=buf, ext_pos=buf, dv_off=60), "lotus_attention_long_bwd", "adjacent k|v column blocks")
    # nothing to do: no launch, no error, the record stays
    assert fwd(ntiles=0) == 0 and bwd(nblocks=0) == 0 and _route() == before


@pytest.mark.skipif(torch.cuda.is_available(), reason="launches with host pointers: only meaningful (and safe) without a device")
def test_route_record_of_a_launch_that_fails_without_a_device():
    fwd, bwd, buf, _ = _calls()
    assert fwd() == E_LAUNCH and _route() == [8, 0, 0, 0, 0, 256, 57344, 0]
    assert fwd(qn=(buf,) * 4, len_max=1024) == E_LAUNCH and _route() == [8, 0, 0, 0, 1, 256, 57344, 0]
    assert bwd() == E_LAUNCH and _route() == [9, 1, 0, 0, 0, 256, 75264, 0]
    assert bwd(qn=(buf,) * 4, dn=(buf,) * 4) == E_LAUNCH and _route() == [9, 1, 0, 0, 1, 256, 75264, 2]
    assert bwd(kext=buf, n_extra=3, extra=buf, ext_pos=buf) == E_LAUNCH and _route() == [9, 1, 0, 0, 0, 256, 75264, 1]
    assert ops.last_attn_route() == ops.AttnRoute(ops.ATTN_LONG_BWD, 1, 0, 0, 0, 256, lu.BWD_LDS, 1)
    assert (lu.FWD_LDS, lu.BWD_LDS) == (57344, 75264)


def test_workspace_query():
    q = lambda nb, H, lm, npos: _capi.query("lotus_attention_long_bwd_workspace", nb, H, lm, npos)   # noqa: E731
    for nb, H, lm, npos in ((1, 1, 129, 129), (3, 2, 256, 700), (7, 32, 1024, 7000), (100, 4, 512, 3), (0, 4, 256, 10)):
        slabs = (lm + 127) // 128
        assert q(nb, H, lm, npos) == 4 * ((npos * H + 3) // 4 * 4 + nb * slabs * H * 128)
    assert q(-1, 2, 256, 1) == 0 and q(2, 0, 256, 1) == 0 and q(2, 2, 0, 1) == 0 and q(2, 2, 1025, 1) == 0 and q(2, 2, 256, -1) == 0
    assert q(3, 2, 256, 5) % 8 == 0


def test_kernels_are_fp32_only_and_outside_the_twin_build():
    protos = _capi.parse_header()
    for name in ("lotus_attention_long_fwd", "lotus_attention_long_bwd", "lotus_attention_long_bwd_workspace"):
        assert name in protos and "lotus_b16_" + name[6:] not in protos, name
    assert (ops.ATTN_LONG_FWD, ops.ATTN_LONG_BWD, ops.ATTN_LONG_MAX) == (8, 9, 1024)
    hdr = open(_capi.HEADER_PATH.replace("include/lotus_hip.h", "robot-3dlotus_amd/csrc/attn_route.h")).read()
    assert "#define LOTUS_ATTN_LONG_FWD 8" in hdr and "#define LOTUS_ATTN_LONG_BWD 9" in hdr
    assert "#define LOTUS_ATTN_LONG_MAX 1024" in open(_capi.HEADER_PATH).read()
    _capi.BF16 = True
    try:
        with pytest.raises(AssertionError, match="fp32 activation storage"):
            ops.attention_long_fwd(*([None] * 19))
    finally:
        _capi.BF16 = False
