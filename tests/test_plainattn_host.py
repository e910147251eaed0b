"""CPU checks of attention without q/k LayerNorm (qk_norm False): the state layout of the plain presets against their
with-norm twins and against the reference's layout, the presets and their YAML round trip, what keeps refusing, the argument
checks of lotus_attention_fwd / _bwd (answered before any launch), the float64 restatement of the patch attention that the GPU
tests use as their reference, and the reproducibility of the fixtures."""
import ctypes
import json

import numpy as np
import pytest
import torch

import adanorm_util as au
import plainattn_util as pu
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg
from robot_3dlotus_amd.policy import MODEL_FACTORY, SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA

E_ARG, E_LAUNCH = -1, -2
PLAIN_PRESETS = ("adanorm_yaml", "adanorm_tiny_plain", "adanorm_v1_plain")


def _layout(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def _is_qk(name):
    return ".attn.q_norm." in name or ".attn.k_norm." in name


# ------------------------------------------------------------------------------------------------- presets and layouts
def test_presets():
    assert lcfg.preset("adanorm_yaml") == lcfg.load_model_config(None)
    for name in ("adanorm_tiny", "adanorm_v1"):
        cfg, plain = lcfg.preset(name), lcfg.preset(name + "_plain")
        assert cfg.ptv3_config.qk_norm is True and plain.ptv3_config.qk_norm is False
        plain.ptv3_config.qk_norm = True
        assert plain == cfg
    y = lcfg.preset("adanorm_yaml")
    assert y.model_class == "SimplePolicyPTV3AdaNorm" and y.ptv3_config.qk_norm is False and y.ptv3_config.in_channels == 6
    assert y.ptv3_config.enc_depths == [2, 2, 2, 6, 2] and y.ptv3_config.enc_channels[0] == 32 and y.ptv3_config.drop_path == 0.1
    assert (y.action_config.pos_pred_type, y.action_config.rot_pred_type, y.action_config.dim_actions) == ("heatmap_mlp", "euler", 8)


def test_plain_layout_is_the_with_norm_layout_minus_the_qk_norms():
    m, p = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny")), SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny_plain"))
    full = _layout(m)
    assert sum(_is_qk(k) for k, _ in full) == 4 * 3                      # three Blocks, q_norm / k_norm weight and bias
    assert _layout(p) == [e for e in full if not _is_qk(e[0])]
    names = [(n, list(v.shape)) for n, v in m.named_parameters()]
    assert [(n, list(v.shape)) for n, v in p.named_parameters()] == [e for e in names if not _is_qk(e[0])]
    # the modules keep their names (nn.Identity, as the reference registers them)
    assert [n for n, _ in p.named_modules()] == [n for n, _ in m.named_modules()]
    a = p.ptv3_model.enc.enc0.block0.attn
    assert isinstance(a.q_norm, torch.nn.Identity) and isinstance(a.k_norm, torch.nn.Identity)


@pytest.mark.parametrize("case", list(pu.CASES))
def test_state_dict_layout_equals_the_fixtures(case):
    layout = json.loads(str(pu.load(case)["state_layout"]))
    assert _layout(SimplePolicyPTV3AdaNorm(pu.case_config(case))) == layout
    assert not any(_is_qk(k) for k, _ in layout)
    if case != "plain_adanorm_tiny_train":
        assert len(layout) == 661
        assert _layout(MODEL_FACTORY["SimplePolicyPTV3AdaNorm"](lcfg.preset("adanorm_yaml"))) == layout


@pytest.mark.parametrize("name", PLAIN_PRESETS)
def test_yaml_round_trip(name, tmp_path):
    import yaml

    cfg = lcfg.preset(name)
    path = tmp_path / (name + ".yaml")
    path.write_text(yaml.safe_dump({"MODEL": json.loads(json.dumps(cfg))}))
    loaded = lcfg.load_model_config(str(path))
    assert loaded == cfg
    if name != "adanorm_v1_plain":  # (the v1 width is built on the GPU; its layout rule is the tiny one's)
        m = MODEL_FACTORY[loaded.model_class](loaded)
        assert isinstance(m, SimplePolicyPTV3AdaNorm) and m.ptv3_model.qk_norm is False
        assert _layout(m) == _layout(SimplePolicyPTV3AdaNorm(cfg))


# ------------------------------------------------------------------------------------------------- what keeps refusing
def test_cross_attention_family_still_refuses():
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3CA

    for cls, name in ((SimplePolicyPTV3CA, "tiny"), (MotionPlannerPTV3CA, "mp_tiny")):
        cfg = lcfg.preset(name)
        cls(cfg)
        cfg.ptv3_config.qk_norm = False
        with pytest.raises(NotImplementedError) as e:
            cls(cfg)
        assert str(e.value) == ("lotus-hip builds the published 3D-LOTUS configuration family only; unsupported: "
                                "['not_qk_norm']")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_other_gemm_precisions_raise_at_forward(mode):
    from robot_3dlotus_amd import ops

    m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny_plain"))
    m.gemm_precision = mode
    with pytest.raises(NotImplementedError, match="gemm_precision"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    m.gemm_precision = None
    prev = ops.get_gemm_precision()
    ops.set_gemm_precision(mode)          # ... and as the process default
    try:
        with pytest.raises(NotImplementedError, match="gemm_precision"):
            m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)
    finally:
        ops.set_gemm_precision(prev)
    m.act_storage = "bf16"
    with pytest.raises(NotImplementedError, match="act_storage"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


def test_norms_come_in_pairs():
    from robot_3dlotus_amd import ops

    w = torch.ones(32)
    with pytest.raises(ValueError, match="together"):
        ops._qk_norms((w, w), None)
    assert ops._qk_norms(None, None) == ((None, None), (None, None))


# ------------------------------------------------------------------------------------------------- argument checks
needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="calls entry points with host pointers: only safe without a device")
NORMS = ("qn_w", "qn_b", "kn_w", "kn_b")
DNORMS = ("dqn_w", "dqn_b", "dkn_w", "dkn_b")
_INTS = dict(q_ld=192, q_off=0, kv_ld=192, k_off=64, v_off=128, ntiles=1, nblocks=1, out_ld=64, H=2, d=32, scale=0.17, eps=1e-6,
             drop_p=0.0, drop_seed=1, precision=0, k_max=0, dq_ld=192, dq_off=0, dkv_ld=192, dk_off=64, dv_off=128,
             dkv_part_stride=0, atomic_out=0, n_extra=0, accumulate=0)
_NULL = ("qidx", "kidx", "owner", "kext", "ext_pos", "dkv_extra", "stream")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib()


def _call(L, name, host, **over):
    restype, argtypes, names = L.protos[name]
    args = []
    for ty, nm in zip(argtypes, names):
        if nm in over:
            args.append(over[nm])
        elif ty is ctypes.c_void_p:
            args.append(None if nm in _NULL else host.ctypes.data)
        elif ty is ctypes.c_size_t:
            args.append(1 << 20)
        else:
            args.append(_INTS[nm])
    return L.fn[name](*args)


@needs_no_device
@pytest.mark.parametrize("base", ["lotus_attention_fwd", "lotus_attention_bwd"])
def test_attention_entry_points_refuse_bad_norm_arguments(lib, base):
    host = np.zeros(1 << 16, dtype=np.float64)
    null4 = dict.fromkeys(NORMS)
    twin = base.replace("lotus_", "lotus_b16_", 1)
    assert base in lib.protos and twin in lib.protos
    # all four given, and all four null in fp32: every check passes and the call gets as far as the launch (no device here)
    assert _call(lib, base, host) == E_LAUNCH, lib.last_error()
    assert _call(lib, twin, host) == E_LAUNCH, lib.last_error()
    assert _call(lib, base, host, **null4) == E_LAUNCH, lib.last_error()
    if base.endswith("bwd"):  # without the norm neither its gradient outputs nor a workspace are needed ...
        assert _call(lib, base, host, **null4, **dict.fromkeys(DNORMS), workspace=None, workspace_bytes=0) == E_LAUNCH, lib.last_error()
        # ... with it they are
        assert _call(lib, base, host, workspace=None, workspace_bytes=0) == E_ARG
        assert _call(lib, base, host, dqn_b=None) == E_ARG
    # some but not all of the four
    for k in range(1, 15):
        some = {n: None for i, n in enumerate(NORMS) if k >> i & 1}
        for name in (base, twin):
            assert _call(lib, name, host, **some) == E_ARG, (name, sorted(some))
            assert "all given or all null" in lib.last_error()
    # no norm: fp32 operands and fp32 storage only, refused by name
    for prec in (1, 3):
        assert _call(lib, base, host, **null4, precision=prec) == E_ARG
        assert "without q/k norm" in lib.last_error() and f"precision {prec}" in lib.last_error()
    for prec in (0, 1, 3):
        assert _call(lib, twin, host, **null4, precision=prec) == E_ARG
        assert "without q/k norm" in lib.last_error() and "bf16 activation storage" in lib.last_error()
    assert lib.fn["lotus_abi_version"]() == _capi.ABI_VERSION == 3
    assert not host.any()


# ------------------------------------------------------------------------------------------------- float64 restatement
def _edge_level():
    import edge_layouts as el
    from frontend_util import fe

    pc, counts, txt = el.patch_edges()
    r = fe.build_all_levels(pc[:, :3].numpy(), counts, 1, perms=[[0, 1, 2, 3]])[0]
    lvl = dict(order_t=torch.from_numpy(r["order"]), inverse_t=torch.from_numpy(r["inverse"]), pad_t=torch.from_numpy(r["pad"]),
               unpad_t=torch.from_numpy(r["unpad"]), cu_seqlens=r["cu_seqlens"])
    return lvl, sum(counts)


@pytest.mark.parametrize("C,H,slot", [(64, 2, 0), (96, 4, 0), (64, 4, 0), (64, 2, 1), (64, 2, 2), (64, 2, 3)])
def test_restatement_equals_the_oracle_with_the_norm(C, H, slot):
    from oracle import model as om

    lvl, n = _edge_level()
    d = C // H
    g = torch.Generator().manual_seed(C + H + slot)
    qkv = (torch.randn(n, 3 * C, generator=g, dtype=torch.float64) * 1.5)
    nrm = [torch.rand(d, generator=g, dtype=torch.float64) + 0.5, torch.randn(d, generator=g, dtype=torch.float64) * 0.2,
           torch.rand(d, generator=g, dtype=torch.float64) + 0.5, torch.randn(d, generator=g, dtype=torch.float64) * 0.2]
    dout = torch.randn(n, C, generator=g, dtype=torch.float64)
    grads = []
    for fn in (lambda x, p: om.patch_attention(x, lvl, slot, H, p[0], p[1], p[2], p[3], 128),
               lambda x, p: pu.patch_attention(x, lvl, slot, H, (p[0], p[1]), (p[2], p[3]))):
        x = qkv.clone().requires_grad_(True)
        p = [t.clone().requires_grad_(True) for t in nrm]
        out = fn(x, p)
        out.backward(dout)
        grads.append([out.detach(), x.grad] + [t.grad for t in p])
    for a, b in zip(*grads):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


def test_restatement_without_the_norm_is_not_the_identity_affine():
    """LayerNorm with weight 1 and bias 0 still centres and scales: the two references differ, so a kernel that ran the norm
    with an identity affine cannot pass the GPU tests."""
    lvl, n = _edge_level()
    qkv, _ = pu.plain_inputs(64, n, 3)
    one, zero = torch.ones(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
    a = pu.patch_attention(qkv.double(), lvl, 0, 2)
    b = pu.patch_attention(qkv.double(), lvl, 0, 2, (one, zero), (one, zero))
    assert float((a - b).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.reference
def test_fixture_regenerates_bit_for_bit(tmp_path):
    import sys

    sys.path.insert(0, au.GOLDEN_DIR)
    import make_golden_plainattn as mk

    name = "plain_adanorm_tiny_train"
    new = dict(np.load(mk.run_case(name, str(tmp_path))))
    old = pu.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f"), k   # (NaN = padding of short gradient heads)


@pytest.mark.reference
def test_reference_runs_the_shipped_yaml_and_matches_the_fixture():
    """A full forward + backward of the shipped YAML (drop_path 0) by the reference on the CPU: the stored losses are not stale,
    and every parameter receives a gradient."""
    import copy
    import sys

    sys.path.insert(0, au.GOLDEN_DIR)
    import make_golden_plainattn as mk
    import ref_harness as rh
    from make_golden import zero_dropouts
    from weights_util import seeded_state_dict

    name = "plain_adanorm_yaml_train"
    fx = pu.load(name)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.manual_seed(0)
        ref, cfg = mk.reference_policy("yaml_dp0")
        assert _layout(ref) == json.loads(str(fx["state_layout"])) and len(ref.state_dict()) == 661
        ref.load_state_dict(seeded_state_dict(ref.state_dict(), int(fx["meta_wseed"]), "scaled"), strict=True)
        zero_dropouts(ref)
        ref.train(True)
        with rh.neutralise_half():
            torch.manual_seed(100 + int(fx["meta_dseed"]))
            _, losses = ref(copy.deepcopy(pu.case_batch(name)), compute_loss=True, compute_final_action=False)
        losses["total"].backward()
    finally:
        torch.set_num_threads(threads)
    for k in ("pos", "rot", "open", "total"):
        assert np.float32(losses[k].item()) == fx["loss_" + k], k
    params = list(ref.named_parameters())
    assert len(params) == 622 and all(p.grad is not None for _, p in params)
