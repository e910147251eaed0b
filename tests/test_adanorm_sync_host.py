"""CPU checks of the data-parallel route of SimplePolicyPTV3AdaNorm: when `_check_sync_bn()` refuses, passes or switches the
SyncBatchNorm statistics on, what `nn.SyncBatchNorm.convert_sync_batchnorm` does to the state_dict, and the C-ABI of the split
(statistics -> message -> apply) adaptive BatchNorm passes."""
import re

import pytest
import torch.nn as nn

import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi, config as lcfg, ops, parallel
from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm

NEW_ENTRIES = ("lotus_adabn_apply_sums", "lotus_adabn_bwd_stats", "lotus_adabn_bwd_apply_sums")


@pytest.fixture
def world(monkeypatch):
    """-> set(n): torch.distributed reports an initialised process group of n ranks; parallel.enable_sync_batchnorm records."""
    import torch.distributed as dist

    calls = []
    monkeypatch.setattr(parallel, "enable_sync_batchnorm", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(ops.BnState, "reduce", None)

    def set_world(n):
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a: n)
        return calls

    return set_world


def _model():
    return SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_tiny"))


def test_statistics_hook_lifts_the_refusal(world, monkeypatch):
    calls = world(2)
    m = _model()
    monkeypatch.setattr(ops.BnState, "reduce", staticmethod(lambda sums: None))
    m.ptv3_model._check_sync_bn()          # must not raise: the statistics are already reduced across ranks
    assert m.ptv3_model._sync_bn_checked and calls == []


def test_converted_containers_switch_the_statistics_on(world):
    calls = world(2)
    m = nn.SyncBatchNorm.convert_sync_batchnorm(_model())
    assert sum(isinstance(x, nn.SyncBatchNorm) for x in m.modules()) == 4  # stem, one pooling, two unpooling branches
    m.ptv3_model._check_sync_bn()
    assert len(calls) == 1 and m.ptv3_model._sync_bn_checked


def test_unconverted_world_of_two_is_refused_and_says_what_to_call(world):
    world(2)
    m = _model()
    with pytest.raises(NotImplementedError, match="world size") as e:
        m.ptv3_model._check_sync_bn()
    assert "convert_sync_batchnorm" in str(e.value) and "enable_sync_batchnorm" in str(e.value)
    assert not m.ptv3_model._sync_bn_checked


@pytest.mark.parametrize("converted", [False, True])
def test_world_of_one_never_raises(world, converted):
    calls = world(1)
    m = _model()
    if converted:
        m = nn.SyncBatchNorm.convert_sync_batchnorm(m)
    m.ptv3_model._check_sync_bn()
    assert calls == [] and m.ptv3_model._sync_bn_checked


def test_conversion_keeps_the_state_dict_layout():
    m = _model()
    before = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    conv = nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert [(k, tuple(v.shape)) for k, v in conv.state_dict().items()] == before
    # the counters the forward pass advances still cover every (converted) BatchNorm, and the seed source is still there
    assert len(conv.ptv3_model._bn_counters()) == 4
    assert conv.ptv3_model.embedding.stem.norm.num_batches_tracked is conv.ptv3_model.embedding.stem.norm.norm.num_batches_tracked


def test_split_entry_points_are_declared_with_a_reference_citation():
    protos = _capi.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos, name
        args = protos[name][2]
        assert args[-1] == "stream" and "sums" in args and "mod_ld" in args and "off" in args, (name, args)
    assert protos["lotus_adabn_apply_sums"][2][-3:-1] == ["eps", "momentum"]
    assert {"dgamma", "dbeta", "dmod", "workspace", "workspace_bytes"} <= set(protos["lotus_adabn_bwd_stats"][2])
    src = open(_capi.HEADER_PATH).read()
    # the comment block in front of the three prototypes cites the reference lines they implement
    at = src.index("int " + NEW_ENTRIES[0])
    block = src[src.rindex("/*", 0, at):at]
    assert re.search(r"train_simple_policy\.py:\d+", block) and re.search(r"model\.py:\d+", block), block
    assert "convert_sync_batchnorm" in block
    assert _capi.ABI_VERSION == 3
