"""enable_flash False / enable_rpe True on the GPU, model level: SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat and
MotionPlannerPTV3AdaNorm against the fixtures of the imported reference's own models (tests/golden/rpe_*.npz, made by
tests/golden/make_golden_rpe.py) with the comparisons and bars of tests/test_gpu_coordattn.py: head outputs and losses 1e-4,
every gradient 1e-4 with its floor (the rpe_table ones named), running statistics 2e-3, final actions 1e-5; the patch size every
level ran at equals the fixture's.  A second training step gives the same bits; with both switches at their shipped values the
models are the ones they were (bit for bit between the spellings, and the existing fixtures still hold); every new preset names
the attention kernels that ran."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402
import concat_util as ccu  # noqa: E402
import mp_ada_util as mu  # noqa: E402
import rpe_util as ru  # noqa: E402

LOGIT_TOL = 1e-4    # the bars of tests/test_gpu_coordattn.py
GRAD_TOL = 1e-4
GRAD_FLOOR = ru.GRAD_FLOOR
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _no_dropout(m):
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0


def _level_K(m, batch, perms):
    pc = batch["pc_fts"].cuda()
    counts = list(batch["npoints_in_batch"])
    levels = m.ptv3_model.frontend.build(pc, counts, [1] * len(counts), perms, need_coord=True)
    for lv in levels:
        assert lv.for_order(1).K == lv.K and int(lv.self_tiles[:, 1].max()) == lv.K == int(lv.self_tiles[:, 1].min())
    return [lv.K for lv in levels]


@pytest.mark.parametrize("case", list(ru.CASES))
def test_rpe_fixture_parity(case):
    from robot_3dlotus_amd import ops
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    family = ru.CASES[case][0]
    planner = family == "mp_ada"
    rpe = ru.case_has_rpe(case)
    fx = ru.load(case)
    cfg = ru.case_config(case)
    assert cfg.ptv3_config.enable_flash is False and cfg.ptv3_config.enable_rpe is rpe
    train = bool(fx["meta_train"])
    assert train == ru.CASES[case][7]
    batch = ru.case_batch(case)
    checksum = batch["pc_fts"].double().sum().item() + (batch["pc_labels"].double().sum().item() if planner else 0.0)
    assert abs(checksum - float(fx["input_checksum"])) < 1e-9
    labels = "gt_trajs" if planner else "gt_actions"
    assert np.array_equal(batch[labels].numpy(), fx[labels])
    m = MODEL_FACTORY[cfg.model_class](cfg)
    sd = ru.case_state_dict(m.state_dict(), int(fx["meta_wseed"]), boost=train)
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(fx["weight_checksum"])) < 1e-6 * abs(float(fx["weight_checksum"]))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train(train)
    _no_dropout(m)
    perms = [p.tolist() for p in fx["perms"]]
    m.ptv3_model.order_perms = perms
    final, losses = m(_dev(batch), compute_loss=True, compute_final_action=not train)
    fwd_route = ops.last_attn_route()
    for name, got in zip(("xt", "xr", "xo") + (("xstop",) if planner else ()), m.last_pred):
        got = got.detach().cpu().numpy()
        if name == "xt" and "xt" not in fx:   # heat-map logits: a fixed sample of them
            assert list(got.shape) == fx["xt_shape"].tolist()
            ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
            got = got.reshape(-1)[ru.xt_sample_index(got.size)]
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
    # which kernels ran: the new family with the term, the existing exact-fp32 tile family for the non-flash patching alone
    qk = int(bool(cfg.ptv3_config.qk_norm))
    R = ops.AttnRoute
    assert fwd_route == (R(ops.ATTN_RPE_FWD, 0, 0, 0, qk, 256, 57216, 0) if rpe else R(ops.ATTN_FWD, 0, 0, 0, qk, 256, 53760, 0)), fwd_route
    print(f"    forward: {fwd_route}; last dense product: {ops.last_dense_route()}")
    if not train:
        ref = fx["final_actions"]
        assert final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
        err = float(np.abs(final.cpu().numpy() - ref).max())
        print(f"    final actions: err {err:.3e}")
        assert final.shape == ref.shape and err <= ACTION_TOL
        assert _level_K(m, batch, perms) == fx["level_K"].tolist()
        return
    assert final is None
    losses["total"].backward()
    # (the backward kernels run on autograd's thread, whose route record this thread does not see: tests/test_gpu_rpe_attn.py
    # names them)
    refs = au.unpack_grads(fx)
    assert sorted(refs) == sorted(n for n, _ in m.named_parameters())
    tabs = [n for n in refs if n.endswith("rpe.rpe_table")]
    gmax = max(r[0] for r in refs.values())
    assert len(tabs) == (3 if rpe else 0) and all(refs[n][0] > GRAD_FLOOR * gmax for n in tabs)
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
        if name in tabs:
            print(f"    {name}: |g| {g.double().norm().item():.4e}  ref {rnorm:.4e}  sketch err {rel:.3e}")
        if rel > worst:
            worst, worst_name = rel, name
        assert rel < GRAD_TOL, ("whole gradient" if whole is not None else "gradient sketch", name, rel)
    print(f"    worst gradient error {worst:.3e} ({worst_name})")
    sdn = m.state_dict()
    for k in fx:
        if k.startswith("buf/"):
            np.testing.assert_allclose(sdn[k[4:]].cpu().numpy(), fx[k], atol=2e-3, rtol=2e-3, err_msg=k)
    assert _level_K(m, batch, perms) == fx["level_K"].tolist()


def test_a_second_step_gives_the_same_bits():
    """One training step of adanorm_tiny_rpe twice from the same seed: losses and every gradient bit for bit (the gradient of
    rpe_table has no atomics)."""
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    case = "rpe_adanorm_tiny_rpe_train"
    cfg = ru.case_config(case)
    batch = _dev(ru.case_batch(case))

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
        assert all(float(p.grad.abs().max()) > 0 for n, p in named if n.endswith("rpe.rpe_table"))
        return [losses["total"].detach().clone()] + [p.grad.clone() for _, p in named]

    a, b = step(), step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


SHIPPED = {"enable_flash": True, "enable_rpe": False, "upcast_attention": False, "upcast_softmax": False}


@pytest.mark.parametrize("util,case", [(au, "adanorm_tiny_scaled_train"), (ccu, "concat_tiny_train"), (mu, "mp_ada_tiny_train")],
                         ids=["adanorm_tiny", "concat_tiny", "mp_ada_tiny"])
def test_shipped_switches_are_the_model_it_was(util, case):
    """adanorm_tiny, concat_tiny and mp_ada_tiny with the four switches at their shipped values against the same preset with the
    keys absent (a configuration written before they were read): the same state dict, logits, loss and gradients bit for bit,
    the flash patching (K = 128 at every level), the kernels of before — and the existing fixture still holds."""
    from robot_3dlotus_amd import ops
    from robot_3dlotus_amd.policy import MODEL_FACTORY
    from weights_util import seeded_state_dict

    fx = util.load(case)
    batch = _dev(util.case_batch(case))
    outs = []
    for variant in ("absent", "shipped"):
        cfg = util.case_config(case)
        for k, v in SHIPPED.items():
            assert cfg.ptv3_config[k] is v, k
            if variant == "absent":
                del cfg.ptv3_config[k]
        torch.manual_seed(9)
        m = MODEL_FACTORY[cfg.model_class](cfg)
        fresh = {k: v.clone() for k, v in m.state_dict().items()}
        assert not any("rpe" in k for k in fresh) and m.ptv3_model.frontend.min_count_patches is False
        m.load_state_dict(seeded_state_dict(m.state_dict(), int(fx["meta_wseed"]), "scaled"), strict=True)
        m = m.cuda().train(True)
        _no_dropout(m)
        m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        assert ops.last_attn_route().family == ops.ATTN_FWD
        losses["total"].backward()
        outs.append((fresh, [t.detach().clone() for t in m.last_pred], losses["total"].detach().clone(),
                     [p.grad.clone() for p in m.parameters()]))
    (f0, pred0, loss0, g0), (f1, pred1, loss1, g1) = outs
    assert list(f0) == list(f1) and all(torch.equal(f0[k], f1[k]) for k in f0)
    assert all(torch.equal(a, b) for a, b in zip(pred0, pred1)) and torch.equal(loss0, loss1)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    xt = pred0[0].cpu().numpy()
    if "xt" in fx:
        ref, got, amax = fx["xt"], xt, float(np.abs(fx["xt"]).max())
    else:
        ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
        got = xt.reshape(-1)[au.xt_sample_index(xt.size)]
    err = float(np.abs(got - ref).max())
    print(f"    xt against the existing fixture: err {err:.3e}  bar {LOGIT_TOL * max(1.0, amax):.3e}")
    assert err <= LOGIT_TOL * max(1.0, amax)
    assert abs(loss0.item() - float(fx["loss_total"])) <= 1e-4 * max(1.0, abs(float(fx["loss_total"])))
    levels = m.ptv3_model.frontend.build(batch["pc_fts"], list(batch["npoints_in_batch"]), [1] * len(batch["npoints_in_batch"]),
                                         m.ptv3_model.order_perms)
    assert [lv.K for lv in levels] == [128] * len(levels)
