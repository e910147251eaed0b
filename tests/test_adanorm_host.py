"""CPU checks of SimplePolicyPTV3AdaNorm: the reference's state_dict layout, the option set it builds (everything else
raises), the YAML / factory route, and the reproducibility of its fixtures."""
import json
import os

import numpy as np
import pytest
import torch

import adanorm_util as au
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import config as lcfg
from robot_3dlotus_amd.policy import MODEL_FACTORY, SimplePolicyPTV3AdaNorm


def _layout(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


@pytest.mark.parametrize("case", list(au.CASES))
def test_state_dict_layout_equals_the_fixtures(case):
    fx = au.load(case)
    m = SimplePolicyPTV3AdaNorm(au.case_config(case))
    assert _layout(m) == json.loads(str(fx["state_layout"]))


def test_state_dict_sizes_and_sites():
    tiny = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny")).state_dict()
    assert len(tiny) == 129
    cfg = lcfg.preset("adanorm_v1")
    cfg.action_config.txt_reduce = "attn"
    v1 = SimplePolicyPTV3AdaNorm(cfg).state_dict()
    assert len(v1) == 380 and "txt_attn_fc.weight" in v1
    assert not any("ca_block" in k for k in v1)
    assert sum(k.endswith("modulation.1.weight") for k in v1) == 40
    assert sum(v1[k].shape[0] for k in v1 if k.endswith("modulation.1.weight")) == 24064
    assert v1["ptv3_model.embedding.stem.norm.norm.running_var"].shape == (64,)
    assert "ptv3_model.dec.dec0.up.proj_skip.1.modulation.1.bias" in v1
    assert "ptv3_model.enc.enc0.block0.attn.q_norm.weight" in v1        # q_norm / k_norm stay plain LayerNorms
    assert "txt_attn_fc.weight" not in SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).state_dict()


@pytest.mark.reference
def test_state_dict_layout_equals_the_live_reference():
    import sys

    sys.path.insert(0, au.GOLDEN_DIR)
    import make_golden_adanorm as mk

    for variant, preset in (("tiny", "adanorm_tiny"), ("tinyctx", "adanorm_tinyctx"), ("v1", "adanorm_v1")):
        for reduce in ("mean", "attn"):
            ref = mk.reference_adanorm(variant, reduce)
            cfg = lcfg.preset(preset)
            cfg.action_config.txt_reduce = reduce
            assert _layout(SimplePolicyPTV3AdaNorm(cfg)) == _layout(ref), (variant, reduce)


@pytest.mark.reference
def test_fixture_regenerates_bit_for_bit(tmp_path):
    import sys

    sys.path.insert(0, au.GOLDEN_DIR)
    import make_golden_adanorm as mk

    name = "adanorm_tiny_scaled_train"
    new = dict(np.load(mk.run_case(name, str(tmp_path))))
    old = au.load(name)
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f"), k   # (NaN = padding of short gradient heads)


def test_presets_are_additive():
    for name in ("adanorm_tiny", "adanorm_v1", "adanorm_tinyctx"):
        cfg, base = lcfg.preset(name), lcfg.preset(name[len("adanorm_"):])
        assert cfg.model_class == "SimplePolicyPTV3AdaNorm" and base.model_class == "SimplePolicyPTV3CA"
        p = cfg.ptv3_config
        assert p.pdnorm_bn and p.pdnorm_ln and p.pdnorm_adaptive and not p.pdnorm_decouple and not p.pdnorm_only_decoder
        for k in ("enc_channels", "enc_depths", "dec_channels", "qk_norm", "enc_patch_size"):
            assert p[k] == base.ptv3_config[k]
        assert cfg.action_config == base.action_config


def test_factory_and_yaml_build(tmp_path):
    import yaml

    cfg = lcfg.preset("adanorm_tiny")
    path = tmp_path / "adanorm.yaml"
    path.write_text(yaml.safe_dump({"MODEL": json.loads(json.dumps(cfg))}))
    loaded = lcfg.load_model_config(str(path))
    m = MODEL_FACTORY[loaded.model_class](loaded)
    assert isinstance(m, SimplePolicyPTV3AdaNorm)
    sd = m.state_dict()
    m2 = MODEL_FACTORY["SimplePolicyPTV3AdaNorm"](lcfg.preset("adanorm_tiny"))
    m2.load_state_dict(sd, strict=True)
    assert m2.num_parameters == m.num_parameters


@pytest.mark.parametrize("opt,value", [("pdnorm_decouple", True), ("pdnorm_adaptive", False), ("pdnorm_bn", False),
                                       ("pdnorm_ln", False), ("pdnorm_affine", False), ("pdnorm_only_decoder", True)])
def test_other_pdnorm_combinations_raise(opt, value):
    cfg = lcfg.preset("adanorm_tiny")
    cfg.ptv3_config[opt] = value
    with pytest.raises(NotImplementedError, match=opt):
        SimplePolicyPTV3AdaNorm(cfg)


def test_bf16_storage_raises():
    m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny"))
    m.act_storage = "bf16"
    with pytest.raises(NotImplementedError, match="act_storage"):
        m({"pc_fts": torch.zeros(4, 7)}, compute_loss=True)


def test_data_parallel_raises(monkeypatch):
    import torch.distributed as dist

    m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny"))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        m.ptv3_model._check_sync_bn()


def test_mean_reduce_needs_one_token_per_cloud():
    from robot_3dlotus_amd import synth

    m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny"))
    with pytest.raises(ValueError, match="one instruction token"):
        m.prepare_ptv3_batch(synth.synth_batch(2, 64, seed=0))


def test_one_set_of_norm_site_nodes():
    """The CA, AdaNorm and Concat backbones reach their stem, pooling, unpooling and Block sub-blocks through the six nodes of
    ops.py and one block walker: adanorm.py and concat.py define no autograd node besides the two stems with a pre-norm convolution
    of their own — the modulation product is ops.ProjAllFn over an ops.ProjBank, the node and bank of the CABlocks' keys / values,
    under no other name — and ops.py (which holds both norm families) does not import adanorm.py."""
    from robot_3dlotus_amd import adanorm, concat, ops, ptv3

    def nodes(mod):
        return {n for n, c in vars(mod).items()
                if isinstance(c, type) and issubclass(c, torch.autograd.Function) and c.__module__ == mod.__name__}

    assert nodes(adanorm) == {"StemGroupsFn"}
    assert issubclass(ops.ProjAllFn, torch.autograd.Function) and isinstance(ops.ProjBank, type)
    for old in ("KvBank", "KvAllFn", "ModBank", "ModAllFn"):
        assert not hasattr(ops, old) and not hasattr(adanorm, old), old
    assert nodes(concat) == {"CtxStemFn"}
    assert {"StemFn", "PoolFn", "UnpoolFn", "CpeFn", "SelfAttnFn", "FfnFn"} <= nodes(ops)
    assert adanorm.AdaBlock.run is ptv3.Block.run and concat.PlainBlock.run is ptv3.Block.run
    assert not hasattr(concat.PlainBlock, "run_plain")
    for cls in (adanorm.PointTransformerV3AdaNorm, concat.PointTransformerV3Plain):
        assert cls.forward is ptv3.PointTransformerV3CA.forward and cls._run_stage is ptv3.PointTransformerV3CA._run_stage
    assert concat.PointTransformerV3Plain._pool is ptv3.PointTransformerV3CA._pool
    assert not any(v is adanorm for v in vars(ops).values())
