"""Patch sizes above 128 on the GPU, model level: SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat and MotionPlannerPTV3AdaNorm
against the fixtures of the imported reference's own models (tests/golden/long_*.npz, made by tests/golden/
make_golden_longattn.py) with the comparisons and bars of tests/test_gpu_rpe_model.py: head outputs and losses 1e-4, every
gradient 1e-4 with its floor, running statistics 2e-3, final actions 1e-5; the tile lengths of every level equal the fixture's;
the long kernels (route family 8) ran at level 0, the 128-row kernels at the levels whose tiles fit them; a second training step
gives the same bits; a K = 128 preset still records the family it recorded before."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402
import longattn_util as lu  # noqa: E402
from weights_util import seeded_state_dict  # noqa: E402

LOGIT_TOL = 1e-4    # the bars of tests/test_gpu_rpe_model.py
GRAD_TOL = 1e-4
GRAD_FLOOR = lu.GRAD_FLOOR
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _no_dropout(m):
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0


def _level_tiles(m, batch, perms):
    pc = batch["pc_fts"].cuda()
    counts = list(batch["npoints_in_batch"])
    levels = m.ptv3_model.frontend.build(pc, counts, [1] * len(counts), perms, need_coord=True)
    out = []
    for lv in levels:
        lens = lv.self_tiles[:, 1].cpu().tolist()
        assert lv.for_order(1).tile_max == lv.tile_max == max(lens) and lv.K == m.ptv3_model.patch_size
        out.append(lens)
    return out


class _Routes:
    """Records (rows of the level, route family) of every patch-attention forward of a pass."""

    def __init__(self, ops, monkeypatch):
        self.seen = []
        for name in ("attention_fwd", "attention_long_fwd"):
            inner = getattr(ops, name)

            def outer(*a, _inner=inner, **kw):
                _inner(*a, **kw)
                self.seen.append((int(a[0].shape[0]), ops.last_attn_route()))
            monkeypatch.setattr(ops, name, outer)


@pytest.mark.parametrize("case", list(lu.CASES))
def test_long_fixture_parity(case, monkeypatch):
    from robot_3dlotus_amd import ops
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    family = lu.CASES[case][0]
    planner = family == "mp_ada"
    K = lu.case_patch(case)
    fx = lu.load(case)
    cfg = lu.case_config(case)
    assert set(cfg.ptv3_config.enc_patch_size) | set(cfg.ptv3_config.dec_patch_size) == {K} and cfg.ptv3_config.enable_flash is True
    train = bool(fx["meta_train"])
    assert train == lu.CASES[case][7]
    batch = lu.case_batch(case)
    checksum = batch["pc_fts"].double().sum().item() + (batch["pc_labels"].double().sum().item() if planner else 0.0)
    assert abs(checksum - float(fx["input_checksum"])) < 1e-9
    labels = "gt_trajs" if planner else "gt_actions"
    assert np.array_equal(batch[labels].numpy(), fx[labels])
    m = MODEL_FACTORY[cfg.model_class](cfg)
    sd = seeded_state_dict(m.state_dict(), int(fx["meta_wseed"]), "scaled")
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(fx["weight_checksum"])) < 1e-6 * abs(float(fx["weight_checksum"]))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train(train)
    _no_dropout(m)
    perms = [p.tolist() for p in fx["perms"]]
    m.ptv3_model.order_perms = perms
    routes = _Routes(ops, monkeypatch)
    final, losses = m(_dev(batch), compute_loss=True, compute_final_action=not train)
    fwd_route = ops.last_attn_route()
    for name, got in zip(("xt", "xr", "xo") + (("xstop",) if planner else ()), m.last_pred):
        got = got.detach().cpu().numpy()
        if name == "xt" and "xt" not in fx:   # heat-map logits: a fixed sample of them
            assert list(got.shape) == fx["xt_shape"].tolist()
            ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
            got = got.reshape(-1)[lu.xt_sample_index(got.size)]
        else:
            ref = fx[name]
            amax = float(np.abs(ref).max())
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = float(np.abs(got - ref).max())
        print(f"    {name}: err {err:.3e}  bar {LOGIT_TOL * max(1.0, amax):.3e}")
        assert err <= LOGIT_TOL * max(1.0, amax), (case, name, err)
    for k in ("pos", "rot", "open") + (("stop",) if planner else ()) + ("total",):
        ref = float(fx["loss_" + k])
        print(f"    loss {k}: {losses[k].item():.7f}  ref {ref:.7f}")
        assert abs(losses[k].item() - ref) <= 1e-4 * max(1.0, abs(ref)), (k, losses[k].item(), ref)
    # which kernels ran: the pass ends at level 0, on the long kernels; every level by the rows of its longest tile
    qk = int(bool(cfg.ptv3_config.qk_norm))
    R = ops.AttnRoute
    assert fwd_route == R(ops.ATTN_LONG_FWD, 0, 0, 0, qk, 256, 57344, 0) == R(8, 0, 0, 0, qk, 256, 57344, 0), fwd_route
    tiles = [[t for t in row if t >= 0] for row in fx["level_tiles"].tolist()]
    n0 = int(sum(fx["npoints_in_batch"]))   # rows of level 0
    assert max(tiles[0]) > 128
    at_level0 = {r.family for n, r in routes.seen if n == n0}
    assert at_level0 == {ops.ATTN_LONG_FWD}, routes.seen
    families = {r.family for _, r in routes.seen}
    if any(max(t) <= 128 for t in tiles):   # a level whose tiles fit the 128-row kernels keeps them: both routes in one model
        assert families == {ops.ATTN_LONG_FWD, ops.ATTN_FWD}, families
        assert all(r.family == ops.ATTN_FWD for n, r in routes.seen if n < 129)
    else:
        assert families == {ops.ATTN_LONG_FWD}, families
    print(f"    forward: {fwd_route}; attention launches by level rows: {sorted({(n, r.family) for n, r in routes.seen})}")
    if not train:
        assert any(max(t) <= 128 for t in tiles)
        ref = fx["final_actions"]
        assert final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
        err = float(np.abs(final.cpu().numpy() - ref).max())
        print(f"    final actions: err {err:.3e}")
        assert final.shape == ref.shape and err <= ACTION_TOL
        assert _level_tiles(m, batch, perms) == tiles
        return
    assert final is None
    losses["total"].backward()
    # (the backward kernels run on autograd's thread, whose route record this thread does not see: tests/test_gpu_longattn.py
    # names them)
    refs = au.unpack_grads(fx)
    assert sorted(refs) == sorted(n for n, _ in m.named_parameters())
    gmax = max(r[0] for r in refs.values())
    worst, worst_name = 0.0, ""
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        g = p.grad.detach().cpu()
        rnorm, head, whole, sketch = refs[name]
        assert abs(g.double().norm().item() - rnorm) / (rnorm + GRAD_FLOOR * gmax) < GRAD_TOL, ("norm", name)
        assert float(np.abs(g.flatten()[:head.size].numpy() - head).max()) / (float(np.abs(head).max()) + GRAD_FLOOR * gmax) < 1e-3, name
        if whole is not None:
            got, ref, floor = g.double().numpy().reshape(-1), whole.astype(np.float64), GRAD_FLOOR * gmax
        else:
            got, ref, floor = au.grad_sketch(g.numpy()), sketch, GRAD_FLOOR * gmax * np.sqrt(au.SKETCH_K)
        rel = float(np.linalg.norm(got - ref)) / (float(np.linalg.norm(ref)) + floor)
        if rel > worst:
            worst, worst_name = rel, name
        assert rel < GRAD_TOL, ("whole gradient" if whole is not None else "gradient sketch", name, rel)
    print(f"    worst gradient error {worst:.3e} ({worst_name})")
    sdn = m.state_dict()
    for k in fx:
        if k.startswith("buf/"):
            np.testing.assert_allclose(sdn[k[4:]].cpu().numpy(), fx[k], atol=2e-3, rtol=2e-3, err_msg=k)
    assert _level_tiles(m, batch, perms) == tiles


def test_a_second_step_gives_the_same_bits():
    """One training step of concat_tiny_p256 (q/k norm, borrowed rows) twice from the same seed: losses and every gradient bit
    for bit (the long backward has no atomics)."""
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    case = "long_concat_tiny_p256_train"
    cfg = lu.case_config(case)
    batch = _dev(lu.case_batch(case))

    def step():
        torch.manual_seed(5)
        m = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
        m.ptv3_model.order_perms = [[2, 0, 1, 3], [1, 3, 0, 2]]
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        named = list(m.named_parameters())
        for n, p in named:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        return [losses["total"].detach().clone()] + [p.grad.clone() for _, p in named]

    a, b = step(), step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("preset", ["adanorm_tiny", "concat_tiny", "mp_ada_tiny"])
def test_a_128_preset_records_the_family_it_recorded_before(preset):
    """K = 128: no level has a tile above 128 rows, the forward ends on attn_fwd_kernel (family 1, 53 760 bytes of LDS) as before."""
    from robot_3dlotus_amd import ops
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    case = {"adanorm_tiny": "long_adanorm_tiny_p256_train", "concat_tiny": "long_concat_tiny_p256_train",
            "mp_ada_tiny": "long_mp_ada_tiny_p256_train"}[preset]
    cfg = lu.case_config(case)
    K = 128
    cfg.ptv3_config.enc_patch_size = [K] * len(cfg.ptv3_config.enc_depths)
    cfg.ptv3_config.dec_patch_size = [K] * len(cfg.ptv3_config.dec_depths)
    batch = lu.case_batch(case)
    torch.manual_seed(3)
    m = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
    _no_dropout(m)
    m.ptv3_model.order_perms = [[2, 0, 1, 3], [1, 3, 0, 2]]
    _, losses = m(_dev(batch), compute_loss=True, compute_final_action=False)
    qk = int(bool(cfg.ptv3_config.qk_norm))
    assert ops.last_attn_route() == ops.AttnRoute(ops.ATTN_FWD, 0, 0, 0, qk, 256, 53760, 0)
    losses["total"].backward()
    torch.cuda.synchronize()
    levels = m.ptv3_model.frontend.build(batch["pc_fts"].cuda(), list(batch["npoints_in_batch"]), [1] * len(batch["npoints_in_batch"]),
                                         m.ptv3_model.order_perms)
    assert [lv.K for lv in levels] == [128] * len(levels) and all(lv.tile_max <= 128 and not ops.long_tiles(lv) for lv in levels)
