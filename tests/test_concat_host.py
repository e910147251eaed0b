"""CPU checks of SimplePolicyPTV3Concat: the identity that folds the per-cloud context columns of the stem convolution into tap sums
(float64, forward and both gradients), the rows of the kernel tests, the state layout against the reference-derived fixtures, every
refusal by name, the argument checks of lotus_ctx_taps_fwd / _bwd (answered before any launch), the presets and their YAML round
trip, the factory entry, and — where the reference is present — the restatement against the reference's own stem and the
reproducibility of a fixture."""
import ctypes
import json

import numpy as np
import pytest
import torch

import adanorm_util as au
import concat_util as cu
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg
from robot_3dlotus_amd.policy import MODEL_FACTORY, SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA

E_ARG, E_LAUNCH = -1, -2


def _layout(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def _concat():
    return MODEL_FACTORY["SimplePolicyPTV3Concat"]


# ------------------------------------------------------------------------------------------------- the identity
@pytest.mark.parametrize("name", ["cube", "dups", "isolated"])
def test_context_columns_fold_into_tap_sums(name):
    """conv(W, [pc | repeat(ctx)]) through the table = conv(W_pc, pc) + taps(P), and the same for dW_ctx, dW_pc and d ctx."""
    pc, counts, nbr = cu.scene_table(name)
    c_pc, Cc, cout, T = 6, 16, 8, 125
    rng = np.random.default_rng(3)
    n, B = sum(counts), len(counts)
    W = rng.standard_normal((cout, T, c_pc + Cc))
    x_pc, ctx = pc[:, :c_pc].double().numpy(), rng.standard_normal((B, Cc))
    dy = rng.standard_normal((n, cout))
    W_pc, W_ctx = W[..., :c_pc], W[..., c_pc:]
    x = np.concatenate([x_pc, cu.repeat_context(ctx, counts)], 1)
    full = cu.dense_conv(W, x, nbr)
    P = cu.tap_table(ctx, W_ctx)
    got = cu.taps_fwd(P, nbr, counts, add=cu.dense_conv(W_pc, x_pc, nbr))
    assert np.abs(got - full).max() <= 1e-12 * max(1.0, np.abs(full).max())
    dW, dx = cu.dense_conv_grads(W, x, nbr, dy)
    dP = cu.taps_bwd(dy, nbr, counts)
    dW_ctx = np.einsum("bto,bc->otc", dP, ctx)
    dctx = np.einsum("bto,otc->bc", dP, W_ctx)
    off = np.concatenate([[0], np.cumsum(counts)])
    dctx_ref = np.stack([dx[s:e, c_pc:].sum(0) for s, e in zip(off[:-1], off[1:])])
    dW_pc, _ = cu.dense_conv_grads(W_pc, x_pc, nbr, dy)
    for a, b in ((dW_ctx, dW[..., c_pc:]), (dW_pc, dW[..., :c_pc]), (dctx, dctx_ref)):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    if name == "isolated":   # the centre tap only: every other dP row is an exact zero
        assert not dP[:, np.arange(T) != 62].any() and dP[:, 62].any()


def test_restatement_reads_the_sign_only_and_the_rows_enter_their_branches():
    assert cu.self_check() == len(cu.ROWS) >= 14
    row = cu.ROWS[2]
    counts, nbr = cu.row_table(row)
    P, add, dy = cu.row_inputs(row, counts)
    sign = np.where(nbr >= 0, 0, -1).astype(np.int32)
    assert np.array_equal(cu.taps_fwd(P, nbr, counts, add), cu.taps_fwd(P, sign, counts, add))
    dP = cu.taps_bwd(dy, nbr, counts)
    for b in range(len(counts)):
        assert not dP[b, cu.absent_tap(b, row.T)].any()
    # <dy, taps(P)> = <dP, P>: the two restatements are adjoint
    lhs = float((dy.astype(np.float64) * cu.taps_fwd(P, nbr, counts)).sum())
    assert abs(lhs - float((dP * P).sum())) <= 1e-9 * max(1.0, abs(lhs))


# ------------------------------------------------------------------------------------------------- presets, layouts, factory
def test_factory_resolves_and_presets():
    cls = _concat()
    assert cls.__name__ == "SimplePolicyPTV3Concat" and issubclass(cls, SimplePolicyPTV3AdaNorm) and issubclass(cls, SimplePolicyPTV3CA)
    y, a = lcfg.preset("concat_yaml"), lcfg.preset("adanorm_yaml")
    assert y.model_class == "SimplePolicyPTV3Concat" and y.ptv3_config.in_channels == 262 and y.ptv3_config.qk_norm is False
    assert (y.ptv3_config.pdnorm_bn, y.ptv3_config.pdnorm_ln, y.ptv3_config.pdnorm_adaptive) == (False, False, False)
    y.model_class = a.model_class
    y.ptv3_config.update(in_channels=6, pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=True)
    assert y == a                                   # the shipped YAML with the class, the width and three flags changed
    t = lcfg.preset("concat_tiny")
    assert t.ptv3_config.in_channels == 263 and t.ptv3_config.qk_norm is True and t.ptv3_config.enc_channels == [64, 64]
    assert t.action_config.use_ee_pose is True and t.action_config.use_step_id is True


@pytest.mark.parametrize("name", ["concat_tiny", "concat_yaml"])
def test_yaml_round_trip(name, tmp_path):
    import yaml

    cfg = lcfg.preset(name)
    path = tmp_path / (name + ".yaml")
    path.write_text(yaml.safe_dump({"MODEL": json.loads(json.dumps(cfg))}))
    loaded = lcfg.load_model_config(str(path))
    assert loaded == cfg
    m = MODEL_FACTORY[loaded.model_class](loaded)
    assert type(m) is _concat() and _layout(m) == _layout(_concat()(cfg))
    w = m.state_dict()["ptv3_model.embedding.stem.conv.weight"]
    assert tuple(w.shape) == (cfg.ptv3_config.enc_channels[0], 5, 5, 5, cfg.ptv3_config.in_channels)


@pytest.mark.parametrize("case", list(cu.CASES))
def test_state_dict_layout_equals_the_fixtures(case):
    layout = json.loads(str(cu.load(case)["state_layout"]))
    m = _concat()(cu.case_config(case))
    assert _layout(m) == layout
    names = [k for k, _ in layout]
    assert not any(".modulation." in k or ".norm.norm." in k or "ca_block" in k for k in names)
    if case != "concat_tiny_train":
        assert not any(".attn.q_norm." in k or ".attn.k_norm." in k for k in names)     # nn.Identity, as the reference registers
        assert dict(map(tuple, map(lambda e: (e[0], tuple(e[1])), layout)))["ptv3_model.embedding.stem.conv.weight"] == (32, 5, 5, 5, 262)
    else:
        assert "stepid_embedding.weight" in names and "pose_embedding.layer_norm.weight" in names


def test_txt_attn_fc_is_built_for_txt_reduce_attn():
    cfg = lcfg.preset("concat_tiny")
    plain = [k for k, _ in _layout(_concat()(cfg))]
    cfg.action_config.txt_reduce = "attn"
    attn = [k for k, _ in _layout(_concat()(cfg))]
    assert [k for k in attn if k not in plain] == ["txt_attn_fc.weight", "txt_attn_fc.bias"]
    assert attn.index("txt_attn_fc.weight") == attn.index("txt_fc.bias") + 1


def test_backbone_has_blocks_only():
    from robot_3dlotus_amd.concat import PlainBlock, PointTransformerV3Plain

    m = _concat()(lcfg.preset("concat_yaml")).ptv3_model
    assert isinstance(m, PointTransformerV3Plain) and m.plain_attention and m.pc_channels == 6 and m.context_channels == 256
    kids = [n for s in list(m.enc) + list(m.dec) for n, _ in s.named_children()]
    assert all(n in ("down", "up") or n.startswith("block") for n in kids)
    assert sum(isinstance(b, PlainBlock) for b in m.modules()) == sum([2, 2, 2, 6, 2]) + sum([2, 2, 2, 2])
    assert isinstance(m.enc.enc0.block0.attn.q_norm, torch.nn.Identity)
    assert isinstance(_concat()(lcfg.preset("concat_tiny")).ptv3_model.enc.enc0.block0.attn.q_norm, torch.nn.LayerNorm)


# ------------------------------------------------------------------------------------------------- refusals
def test_adaptive_pdnorm_is_refused_by_name():
    cfg = lcfg.preset("concat_yaml")
    cfg.ptv3_config.update(pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=True)     # the YAML's own flags
    with pytest.raises(NotImplementedError, match="pdnorm_adaptive=True.*passes no context"):
        _concat()(cfg)


@pytest.mark.parametrize("bn,ln", [(True, True), (True, False), (False, True)])
def test_non_adaptive_pdnorm_is_refused_with_the_hint(bn, ln):
    cfg = lcfg.preset("concat_tiny")
    cfg.ptv3_config.update(pdnorm_bn=bn, pdnorm_ln=ln, pdnorm_adaptive=False)
    with pytest.raises(NotImplementedError, match=f"pdnorm_bn={bn}, pdnorm_ln={ln}.*switch both off"):
        _concat()(cfg)


def _host_batch(c_pc=7, lens=(1, 1)):
    return {"pc_fts": torch.zeros(8, c_pc), "txt_embeds": torch.zeros(sum(lens), 512), "txt_lens": list(lens),
            "npoints_in_batch": [4, 4], "offset": torch.tensor([4, 8])}


def test_prepare_batch_refusals():
    m = _concat()(lcfg.preset("concat_tiny"))
    with pytest.raises(ValueError, match=r"one instruction token per cloud.*txt_lens=\[1, 3\]"):
        m.prepare_ptv3_batch(_host_batch(lens=(1, 3)))
    with pytest.raises(NotImplementedError, match="pc_fts of 9 columns.*at most 8"):
        m.prepare_ptv3_batch(_host_batch(c_pc=9))
    with pytest.raises(ValueError, match=r"in_channels=263 != 6 columns of pc_fts \+ 256 context_channels"):
        m.prepare_ptv3_batch(_host_batch(c_pc=6))
    cfg = lcfg.preset("concat_tiny")
    cfg.ptv3_config.in_channels = 200
    with pytest.raises(ValueError, match="in_channels=200"):
        _concat()(cfg)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_other_precisions_and_bf16_storage_raise_at_forward(mode):
    from robot_3dlotus_amd import ops

    m = _concat()(lcfg.preset("concat_tiny"))
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
    with pytest.raises(NotImplementedError, match="SimplePolicyPTV3Concat: act_storage='bf16'"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


def test_head_options_refuse_as_in_the_other_policies():
    cfg = lcfg.preset("concat_tiny")
    cfg.action_config.reduce = "mean"
    with pytest.raises(NotImplementedError, match="reduce='mean'"):
        _concat()(cfg)


# ------------------------------------------------------------------------------------------------- argument checks
needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="calls entry points with host pointers: only safe without a device")
_INTS = dict(B=2, n=10, T=27, C=8)
_NULL = ("stream",)


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
            args.append(host.nbytes)
        else:
            args.append(_INTS[nm])
    return L.fn[name](*args)


def test_entry_points_exist_without_twins(lib):
    for name in ("lotus_ctx_taps_fwd", "lotus_ctx_taps_bwd", "lotus_ctx_taps_workspace", "lotus_ctx_taps_plan"):
        assert name in lib.protos and name.replace("lotus_", "lotus_b16_", 1) not in lib.protos
    assert lib.fn["lotus_ctx_taps_workspace"](2, 125, 32) == cu.CT_SPLITS * 2 * 125 * 32 * 4
    out = (ctypes.c_int * 6)()
    assert lib.fn["lotus_ctx_taps_plan"](70001, 1, 125, 32, ctypes.addressof(out)) == 0
    assert list(out) == [cu.CT_ROWS, -(-70001 // cu.CT_ROWS), cu.CT_SPLITS, cu.CT_TILE, cu.CT_BTILE, cu.max_width(125)]
    assert lib.fn["lotus_ctx_taps_plan"](1, 1, 128, 4, ctypes.addressof(out)) == 0 and out[5] == cu.max_width(128) == 256


@needs_no_device
@pytest.mark.parametrize("name", ["lotus_ctx_taps_fwd", "lotus_ctx_taps_bwd"])
def test_entry_points_refuse_bad_arguments_before_any_launch(lib, name):
    host = np.zeros(1 << 20, dtype=np.float64)
    # valid arguments: every check passes and the call gets as far as the launch (no device here)
    assert _call(lib, name, host) == E_LAUNCH, lib.last_error()
    assert _call(lib, name, host, n=0) == 0                                   # no rows: 0 without a launch
    bad = [dict(C=0), dict(C=-4), dict(C=6), dict(T=0), dict(T=-1), dict(T=129), dict(B=0), dict(B=-1), dict(n=-1),
           dict(T=125, C=cu.max_width(125) + 4), dict(T=128, C=260), dict(T=1, C=cu.CT_MAX_TC + 4)]
    for o in bad:
        assert _call(lib, name, host, **o) == E_ARG, o
        assert name in lib.last_error()
    assert _call(lib, name, host, T=125, C=cu.max_width(125), n=0) == 0       # the widest admitted shape
    ptrs = [nm for ty, nm in zip(*lib.protos[name][1:]) if ty is ctypes.c_void_p and nm not in _NULL + ("add", "workspace")]
    assert sorted(ptrs) == sorted({"lotus_ctx_taps_fwd": ["P", "nbr", "off", "y"], "lotus_ctx_taps_bwd": ["dy", "nbr", "off", "dP"]}[name])
    for p in ptrs:
        assert _call(lib, name, host, **{p: None}) == E_ARG, p
        assert "null pointer" in lib.last_error()
    if name.endswith("fwd"):
        assert _call(lib, name, host, add=None) == E_LAUNCH                   # add is optional
        assert _call(lib, name, host, y=host.ctypes.data + 4) == E_ARG and "aligned" in lib.last_error()
    else:
        need = lib.fn["lotus_ctx_taps_workspace"](_INTS["B"], _INTS["T"], _INTS["C"])
        assert _call(lib, name, host, workspace_bytes=need) == E_LAUNCH
        assert _call(lib, name, host, workspace_bytes=need - 1) == E_ARG and "workspace" in lib.last_error()
        assert _call(lib, name, host, workspace=None) == E_ARG and "workspace" in lib.last_error()
    assert lib.fn["lotus_abi_version"]() == _capi.ABI_VERSION
    assert not host.any()


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.reference
def test_restatement_equals_the_reference_stem():
    """The reference's Embedding stem convolution (its SubMConv3d through tests/golden/ref_harness.py) on the reference's own
    concatenation, simple_policy_ptv3.py:457-461, against conv(W_pc, pc) + taps(P) of the restatement."""
    import sys

    sys.path.insert(0, au.GOLDEN_DIR)
    import ref_harness as rh
    from frontend_util import fe

    rh.install_shims()
    import spconv.pytorch as spconv

    pc, counts, nbr = cu.scene_table("cube")
    _, _, _, rel = cu.scene("cube")
    c_pc, Cc, cout = 7, 256, 32
    g = torch.Generator().manual_seed(4)
    ctx = torch.randn(len(counts), Cc, generator=g, dtype=torch.float64)
    conv = spconv.SubMConv3d(c_pc + Cc, cout, 5, bias=False).double()
    feat = torch.cat([pc.double(), torch.repeat_interleave(ctx, torch.tensor(counts), 0)], -1)
    idx = torch.cat([torch.from_numpy(cu.cloud_of(counts))[:, None], torch.from_numpy(rel.astype(np.int64))], 1).int()
    ref = conv(spconv.SparseConvTensor(feat, idx, (rel.max(0) + 1).tolist(), len(counts))).features.detach().numpy()
    W = conv.weight.detach().numpy().reshape(cout, 125, c_pc + Cc)
    got = cu.taps_fwd(cu.tap_table(ctx.numpy(), W[..., c_pc:]), nbr, counts, add=cu.dense_conv(W[..., :c_pc], pc.double().numpy(), nbr))
    assert np.abs(got - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max())
    np.testing.assert_array_equal(fe.neighbour_table(rel, cu.cloud_of(counts).astype(np.int32), 5).T, nbr)


@pytest.mark.reference
def test_fixture_regenerates_bit_for_bit(tmp_path):
    import sys

    sys.path.insert(0, au.GOLDEN_DIR)
    import make_golden_concat as mk

    name = "concat_tiny_train"
    new = dict(np.load(mk.run_case(name, str(tmp_path))))
    old = cu.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f"), k   # (NaN = padding of short gradient heads)
