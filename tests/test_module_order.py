"""Registration ORDER of modules, parameters and state_dict entries of every preset, pinned against a fixture.

The gradient reducer's buckets, the optimizer's parameter groups, the slice order of the PDNorms' ops.ProjBank, ops.WeightShadows and
checkpoints all depend on the order in which sub-modules are registered, not only on the set of their names.  The fixture
tests/golden/module_order.json was written at the commit BEFORE the backbone constructors were split into overridable steps, by

    import json, test_module_order as t
    json.dump({name: t.record(name) for name in t.PRESETS}, open(t.FIXTURE, "w"), indent=0, sort_keys=True)

and the test asserts equality with it.  Tiny presets store the full lists (a failure names the first differing entry), the
v1-size presets a sha256 of each list joined by newlines.  The AdaNorm presets also store the PDNorm site order (slice j of the
modulation bank is norm j).  CPU only; the models are built, never run."""
import hashlib
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "module_order.json")
PRESETS = ("v1", "tiny", "tinydeep", "tinyctx", "peract", "mp", "mp_tiny", "mp_tinyctx", "adanorm_v1", "adanorm_tiny",
           "adanorm_tinyctx", "tiny_reg", "v1_reg", "adanorm_tiny_reg")


def record(name):
    from robot_3dlotus_amd import config as lcfg
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    cfg = lcfg.preset(name)
    m = MODEL_FACTORY[cfg.model_class](cfg)
    lists = {"state_dict": list(m.state_dict()), "parameters": [n for n, _ in m.named_parameters()],
             "modules": [n for n, _ in m.named_modules()]}
    pd = getattr(m.ptv3_model, "_pdnorms", None)
    if pd is not None:
        names = {id(mod): n for n, mod in m.ptv3_model.named_modules()}
        lists["pdnorm_sites"] = [names[id(mod)] for mod in pd]
    if "tiny" in name:
        return lists
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in lists.items()}


with open(FIXTURE) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_preset():
    assert sorted(GOLDEN) == sorted(PRESETS)
    for name in PRESETS:
        want = {"state_dict", "parameters", "modules"} | ({"pdnorm_sites"} if name.startswith("adanorm") else set())
        assert set(GOLDEN[name]) == want, name


@pytest.mark.parametrize("name", PRESETS)
def test_registration_order(name):
    got, want = record(name), GOLDEN[name]
    assert set(got) == set(want)
    for kind in sorted(want):
        if isinstance(want[kind], list):
            assert len(got[kind]) == len(want[kind]), (name, kind)
            first = next((i for i, (a, b) in enumerate(zip(got[kind], want[kind])) if a != b), None)
            assert first is None, f"{name}.{kind}[{first}]: {got[kind][first]!r} != {want[kind][first]!r}"
        else:
            assert got[kind] == want[kind], f"{name}.{kind}: order or names changed (sha256 of the joined list)"
