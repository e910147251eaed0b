"""The oracle against the reference: live against the imported reference (tests marked `reference`: build container only,
skipped where /root/reference does not exist), and against the reference's outputs stored in
tests/golden/serialization_layout.npz (tests/golden/make_golden_serialization.py) everywhere."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _harness():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import ref_harness as rh

    rh.install_shims()
    return rh


@pytest.mark.reference
@pytest.mark.parametrize("variant,wvar,B,n,train", [("tiny", "scaled", 3, 700, True), ("tiny", "init", 2, 300, False),
                                                    ("v1", "scaled", 2, 640, True)])
def test_losses_and_grads_match_reference(variant, wvar, B, n, train):
    rh = _harness()
    from weights_util import seeded_state_dict
    from robot_3dlotus_amd import config as lcfg, synth
    from oracle.model import Oracle
    from make_golden import zero_dropouts

    ref, _ = rh.build_reference_policy(variant)
    sd = seeded_state_dict(ref.state_dict(), 7, wvar)
    ref.load_state_dict(sd, strict=True)
    zero_dropouts(ref)
    ref.train(train)
    batch = synth.synth_batch(B, n, ragged=True, seed=21)
    perms = []
    with rh.neutralise_half(), rh.record_randperm(perms):
        torch.manual_seed(3)
        losses = rh.reference_forward(ref, copy.deepcopy(batch), full=(variant == "v1"))
    losses["total"].backward()
    sdg = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    out = Oracle(sdg, lcfg.plain(lcfg.preset(variant)), training=train).forward(batch, [p.numpy() for p in perms])
    for k in losses:
        assert abs(losses[k].item() - out["losses"][k].item()) < 1e-5 * max(1, abs(losses[k].item()))
    out["losses"]["total"].backward()
    gmax = max(p.grad.norm().item() for p in ref.parameters())
    for name, p in ref.named_parameters():
        assert (p.grad - sdg[name].grad).norm().item() <= 1e-4 * p.grad.norm().item() + 1e-6 * gmax, name


@pytest.mark.reference
@pytest.mark.parametrize("variant,B,n,train", [("tiny", 3, 1024, True), ("tinydeep", 2, 1024, True), ("tinyctx", 2, 900, False)])
def test_oracle_matches_the_reference_own_attention_arithmetic(variant, B, n, train):
    """flash_attn is not installed here, so everywhere else the reference runs over the harness' stand-in for it.  With
    `enable_flash=False` the reference computes both attentions ITSELF — the padded-patch softmax of SerializedAttention
    (PointTransformerV3/model.py:499-527) and the padded einsum of the cross attention (model_ca.py:68-95; absent words masked
    with -1e4) — over the same patches and the same key sets as its flash calls.  The oracle (and the HIP kernels checked
    against it) must agree with THAT code: losses 1e-5, every parameter gradient 1e-4; and the stand-in must agree with it too,
    which pins the fixtures generated over the stand-in.  (Two-stage configurations with >= 128 points per cloud at both levels:
    the non-flash branch shrinks the patch size to the smallest cloud of a level, model.py:469-472 — a different function as soon
    as a cloud is shorter than one patch, as at the deep levels of v1.)"""
    rh = _harness()
    from weights_util import seeded_state_dict
    from robot_3dlotus_amd import config as lcfg, synth
    from oracle.model import Oracle
    from make_golden import zero_dropouts

    batch = synth.synth_batch(B, n, ragged=False, seed=33)
    runs = {}
    for flash in (False, True):
        ref, _ = rh.build_reference_policy(variant, enable_flash=flash)
        if flash:
            ref.load_state_dict(sd, strict=True)
        else:
            sd = seeded_state_dict(ref.state_dict(), 9, "scaled")
            ref.load_state_dict(sd, strict=True)
        zero_dropouts(ref)
        ref.train(train)
        perms = []
        with rh.neutralise_half(), rh.record_randperm(perms):
            torch.manual_seed(4)
            losses = rh.reference_forward(ref, copy.deepcopy(batch), full=(variant == "v1"))
        losses["total"].backward()
        runs[flash] = (ref, losses, perms)
    ref, losses, perms = runs[False]
    sdg = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    out = Oracle(sdg, lcfg.plain(lcfg.preset(variant)), training=train).forward(batch, [p.numpy() for p in perms])
    out["losses"]["total"].backward()
    gmax = max(p.grad.norm().item() for p in ref.parameters())
    stand_in = dict(runs[True][0].named_parameters())
    for k in losses:
        assert abs(losses[k].item() - out["losses"][k].item()) < 1e-5 * max(1, abs(losses[k].item())), k
        assert abs(losses[k].item() - runs[True][1][k].item()) < 1e-5 * max(1, abs(losses[k].item())), k
    for name, p in ref.named_parameters():
        assert (p.grad - sdg[name].grad).norm().item() <= 1e-4 * p.grad.norm().item() + 1e-6 * gmax, name
        assert (p.grad - stand_in[name].grad).norm().item() <= 1e-4 * p.grad.norm().item() + 1e-6 * gmax, name


@pytest.mark.reference
@pytest.mark.parametrize("variant", ["mp_tiny", "mp_tinyctx"])
def test_motion_planner_fixtures_stand_on_the_reference_own_attention_arithmetic(variant):
    """The 3D-LOTUS++ motion planner (motion_planner_ptv3.py) over the same backbone: with `enable_flash=False` the reference runs
    its own attention arithmetic; the run over the harness' flash stand-in — what tests/golden/mp_*.npz were generated with — must
    agree with it (losses 1e-5, every parameter gradient 1e-4).  Two-stage variants, >= 128 points per cloud at both levels."""
    rh = _harness()
    from weights_util import seeded_state_dict
    from robot_3dlotus_amd import synth
    from make_golden import zero_dropouts

    batch = synth.synth_batch_mp(2, 1024, ragged=False, seed=35)
    runs = {}
    sd = None
    for flash in (False, True):
        ref, _ = rh.build_reference_mp(variant, enable_flash=flash)
        if sd is None:
            sd = seeded_state_dict(ref.state_dict(), 10, "scaled")
        ref.load_state_dict(sd, strict=True)
        zero_dropouts(ref)
        ref.train(True)
        with rh.neutralise_half():
            torch.manual_seed(5)
            losses = rh.reference_forward_mp(ref, copy.deepcopy(batch))
        losses["total"].backward()
        runs[flash] = (ref, losses)
    own, stand_in = runs[False], runs[True]
    for k in own[1]:
        assert abs(own[1][k].item() - stand_in[1][k].item()) < 1e-5 * max(1, abs(own[1][k].item())), k
    gmax = max(p.grad.norm().item() for p in own[0].parameters() if p.grad is not None)
    other = dict(stand_in[0].named_parameters())
    for name, p in own[0].named_parameters():
        if p.grad is None:
            assert other[name].grad is None, name
            continue
        assert (p.grad - other[name].grad).norm().item() <= 1e-4 * p.grad.norm().item() + 1e-6 * gmax, name


def _golden_serialization():
    sys.path.insert(0, GOLDEN)
    import make_golden_serialization as mgs

    return mgs, np.load(os.path.join(GOLDEN, "serialization_layout.npz"))


def test_encode_matches_reference_all_depths():
    """The reference's serialization codes of seeded grids, every depth and order (captured by make_golden_serialization.py)."""
    from oracle import front_end as fe

    mgs, gold = _golden_serialization()
    assert tuple(fe.ORDERS) == mgs.ORDERS
    for depth, g, b in mgs.encode_inputs():
        for o in fe.ORDERS:
            np.testing.assert_array_equal(fe.encode(g, b, depth, o), gold[f"encode_{depth}_{o}"])


def test_hilbert_roundtrip_through_reference_decoder():
    """Hilbert codes decode back to coordinates with the reference's own decoder (its output on the codes
    below, captured by make_golden_serialization.py)."""
    from oracle import front_end as fe

    mgs, gold = _golden_serialization()
    g, b = mgs.hilbert_inputs()
    np.testing.assert_array_equal(fe.encode(g, b, 9, "hilbert"), gold["hilbert_code"])
    np.testing.assert_array_equal(gold["hilbert_decoded_grid"], g)
    np.testing.assert_array_equal(gold["hilbert_decoded_batch"], b)


def test_state_template_matches_reference_layout():
    """Checkpoint-format contract: 460 entries, same names and shapes as the reference policy's
    state_dict (captured by make_golden_serialization.py)."""
    import golden_util as gu
    from robot_3dlotus_amd import config as lcfg

    _, gold = _golden_serialization()
    for variant in ("v1", "tiny"):
        rsd = {k: tuple(int(x) for x in s.split(",") if x) for k, s in zip(gold[f"layout_{variant}_names"], gold[f"layout_{variant}_shapes"])}
        t = gu.state_template(lcfg.preset(variant))
        assert set(t) == set(rsd)
        for k in t:
            assert tuple(t[k].shape) == rsd[k], k
        if variant == "v1":
            assert len(t) == 460


@pytest.mark.reference
def test_committed_fixture_equals_what_the_generator_writes(tmp_path):
    """The committed fixtures ARE the generator's output: regenerate one case from the imported reference
    and compare every key bit for bit (the generator runs the reference on one thread: with several, its CPU backward is not
    reproducible from run to run)."""
    import os
    import sys

    import numpy as np

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg

    mg.run_case("tiny_scaled_train", mg.CASES["tiny_scaled_train"], out_dir=str(tmp_path))
    new = np.load(os.path.join(str(tmp_path), "tiny_scaled_train.npz"))
    old = np.load(os.path.join(mg.HERE, "tiny_scaled_train.npz"))
    assert set(new.files) == set(old.files)
    diff = [k for k in new.files if not np.array_equal(new[k], old[k])]
    assert not diff, diff[:10]
