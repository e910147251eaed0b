"""add_coords_in_attn 'qk' / 'qkv' on the GPU, model level: SimplePolicyPTV3AdaNorm, SimplePolicyPTV3Concat and
MotionPlannerPTV3AdaNorm against the fixtures of the imported reference's own models (tests/golden/coord_*.npz, made by
tests/golden/make_golden_coordattn.py) with the comparisons and bars of tests/test_gpu_plainattn.py / test_gpu_mp_adanorm.py:
head outputs and losses 1e-4, every gradient 1e-4 with its floor (the coords_proj ones named), running statistics 2e-3, final
actions 1e-5.  The tiny cases have two stages, so the mean-pooled coordinates of level 1 enter the term; every level's
coordinates are also compared with a float64 per-voxel mean.  With the option off the model is the one it was: state dict and
logits bit for bit, and the existing fixture of adanorm_tiny_plain still holds through the new argument path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402
import coordattn_util as cu  # noqa: E402
import plainattn_util as pu  # noqa: E402

LOGIT_TOL = 1e-4    # the bars of tests/test_gpu_plainattn.py / test_gpu_adanorm.py / test_gpu_mp_adanorm.py
GRAD_TOL = 1e-4
GRAD_FLOOR = 1e-3
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _no_dropout(m):
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0


def _check_level_coords(m, batch, perms):
    """The coordinates the term reads at every level: level 0 is pc_fts[:, :3] itself, level s > 0 the mean of the coordinates
    of each voxel's members one level up (model.py:763-765), here in float64."""
    pc = batch["pc_fts"].cuda()
    counts = list(batch["npoints_in_batch"])
    levels = m.ptv3_model.frontend.build(pc, counts, [1] * len(counts), perms, need_coord=True)
    assert len(levels) >= 2
    assert levels[0].coord.data_ptr() == pc.data_ptr() and levels[0].coord.stride(0) == pc.shape[1]
    prev = pc[:, :3].double()
    for s, lv in enumerate(levels[1:], 1):
        cl = lv.cluster.long()
        assert cl.numel() == prev.shape[0] and int(cl.max()) == lv.n - 1
        ref = torch.zeros(lv.n, 3, dtype=torch.float64, device="cuda").index_add_(0, cl, prev)
        ref /= torch.bincount(cl, minlength=lv.n).double().unsqueeze(1)
        err = float((lv.coord.double() - ref).abs().max())
        print(f"    level {s}: {lv.n} voxels, pooled coordinates err {err:.3e}")
        assert lv.coord.shape == (lv.n, 3) and err <= cu.KERNEL_TOL * max(1.0, float(ref.abs().max()))
        assert lv.for_order(1).coord is lv.coord
        prev = ref


@pytest.mark.parametrize("case", list(cu.CASES))
def test_coord_fixture_parity(case):
    from robot_3dlotus_amd.policy import MODEL_FACTORY
    from weights_util import seeded_state_dict

    family = cu.CASES[case][0]
    planner = family == "mp_ada"
    fx = cu.load(case)
    cfg = cu.case_config(case)
    assert cfg.ptv3_config.add_coords_in_attn == cu.case_mode(case)
    train = bool(fx["meta_train"])
    batch = cu.case_batch(case)
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
    final, losses = m(_dev(batch), compute_loss=True, compute_final_action=not train)
    for name, got in zip(("xt", "xr", "xo") + (("xstop",) if planner else ()), m.last_pred):
        got = got.detach().cpu().numpy()
        if name == "xt" and "xt" not in fx:   # heat-map logits: a fixed sample of them
            assert list(got.shape) == fx["xt_shape"].tolist()
            ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
            got = got.reshape(-1)[cu.xt_sample_index(got.size)]
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
    if not train:
        ref = fx["final_actions"]
        assert final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
        err = float(np.abs(final.cpu().numpy() - ref).max())
        print(f"    final actions: err {err:.3e}")
        assert final.shape == ref.shape and err <= ACTION_TOL
        _check_level_coords(m, batch, perms)
        return
    assert final is None
    losses["total"].backward()
    refs = au.unpack_grads(fx)
    assert sorted(refs) == sorted(n for n, _ in m.named_parameters())
    cps = [n for n in refs if "coords_proj" in n]
    assert len(cps) == 3 and all(refs[n][0] > 0 for n in cps)
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
        if "coords_proj" in name:
            print(f"    {name}: |g| {g.double().norm().item():.4e}  ref {rnorm:.4e}  sketch err {rel:.3e}")
        if rel > worst:
            worst, worst_name = rel, name
        assert rel < GRAD_TOL, ("whole gradient" if whole is not None else "gradient sketch", name, rel)
    print(f"    worst gradient error {worst:.3e} ({worst_name})")
    sdn = m.state_dict()
    for k in fx:
        if k.startswith("buf/"):
            np.testing.assert_allclose(sdn[k[4:]].cpu().numpy(), fx[k], atol=2e-3, rtol=2e-3, err_msg=k)
    _check_level_coords(m, batch, perms)


def test_a_second_step_gives_the_same_bits():
    """One training step of adanorm_tiny_qk twice from the same seed: losses and every gradient bit for bit (the weight gradient
    of coords_proj has no atomics)."""
    from robot_3dlotus_amd import config as lcfg
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    cfg = lcfg.preset("adanorm_tiny_qk")
    cfg.action_config.txt_reduce = "mean"
    batch = _dev(cu.case_batch("coord_adanorm_tiny_qk_train"))

    def step():
        torch.manual_seed(5)
        m = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        named = list(m.named_parameters())
        for n, p in named:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert all(float(p.grad.abs().max()) > 0 for n, p in named if "coords_proj" in n)
        return [losses["total"].detach().clone()] + [p.grad.clone() for _, p in named]

    a, b = step(), step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_option_off_is_the_model_it_was():
    """adanorm_tiny_plain with add_coords_in_attn 'none' against the same preset with the key absent (a configuration written
    before the option was read): the same state dict and the same logits bit for bit, no coords_proj key, and the existing
    fixture plain_adanorm_tiny_train still holds."""
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm
    from weights_util import seeded_state_dict

    case = "plain_adanorm_tiny_train"
    fx = pu.load(case)
    batch = _dev(pu.case_batch(case))
    outs = []
    for variant in ("absent", "none", False):
        cfg = pu.case_config(case)
        if variant == "absent":
            del cfg.ptv3_config["add_coords_in_attn"]
        else:
            cfg.ptv3_config.add_coords_in_attn = variant
        torch.manual_seed(9)
        m = SimplePolicyPTV3AdaNorm(cfg)
        fresh = {k: v.clone() for k, v in m.state_dict().items()}
        assert not any("coords_proj" in k for k in fresh)
        m.load_state_dict(seeded_state_dict(m.state_dict(), int(fx["meta_wseed"]), "scaled"), strict=True)
        m = m.cuda().train(True)
        _no_dropout(m)
        m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        outs.append((fresh, [t.detach().clone() for t in m.last_pred], losses["total"].detach().clone(),
                     [p.grad.clone() for p in m.parameters()]))
    base = outs[0]
    for fresh, pred, loss, grads in outs[1:]:
        assert list(fresh) == list(base[0]) and all(torch.equal(fresh[k], base[0][k]) for k in fresh)
        assert all(torch.equal(a, b) for a, b in zip(pred, base[1])) and torch.equal(loss, base[2])
        assert all(torch.equal(a, b) for a, b in zip(grads, base[3]))
    xt = base[1][0].cpu().numpy()
    ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
    err = float(np.abs(xt.reshape(-1)[au.xt_sample_index(xt.size)] - ref).max())
    print(f"    xt against the existing fixture: err {err:.3e}  bar {LOGIT_TOL * max(1.0, amax):.3e}")
    assert err <= LOGIT_TOL * max(1.0, amax)
    assert abs(base[2].item() - float(fx["loss_total"])) <= 1e-4 * max(1.0, abs(float(fx["loss_total"])))
