"""MotionPlannerPTV3AdaNorm on the GPU: against the fixtures of the imported reference's own MotionPlannerPTV3AdaNorm
(tests/golden/mp_ada_*.npz; bars of tests/test_gpu_plainattn.py / test_gpu_adanorm.py: head outputs and losses 1e-4, gradients
1e-4 with their floor, running statistics 2e-3, final actions 1e-5); one training step of the shipped YAML with every dropout
and DropPath on; prefetch(); the two-group stem against the single 8-column stem; the published heat-map head on this
backbone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402
import mp_ada_util as mu  # noqa: E402

KERNEL_TOL = 2e-5
LOGIT_TOL = 1e-4
GRAD_TOL = 1e-4
GRAD_FLOOR = 1e-3
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _model(cfg, wseed=None, train=True):
    from robot_3dlotus_amd.policy import MODEL_FACTORY
    from weights_util import seeded_state_dict

    m = MODEL_FACTORY[cfg.model_class](cfg)
    sd = None
    if wseed is not None:
        sd = seeded_state_dict(m.state_dict(), wseed, "scaled")
        m.load_state_dict(sd, strict=True)
    return m.cuda().train(train), sd


def _no_dropout(m):
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0


@pytest.mark.parametrize("case", list(mu.CASES))
def test_fixture_parity(case):
    fx = mu.load(case)
    cfg = mu.case_config(case)
    train = bool(fx["meta_train"])
    batch = mu.case_batch(case)
    assert abs(batch["pc_fts"].double().sum().item() + batch["pc_labels"].double().sum().item() - float(fx["input_checksum"])) < 1e-9
    assert np.array_equal(batch["gt_trajs"].numpy(), fx["gt_trajs"])
    m, sd = _model(cfg, int(fx["meta_wseed"]), train)
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(fx["weight_checksum"])) < 1e-6 * abs(float(fx["weight_checksum"]))
    _no_dropout(m)
    m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
    final, losses = m(_dev(batch), compute_loss=True, compute_final_action=not train)
    for name, got in zip(("xt", "xr", "xo", "xstop"), m.last_pred):
        got, ref = got.detach().cpu().numpy(), fx[name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err, amax = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print(f"    {name}: err {err:.3e}  bar {LOGIT_TOL * max(1.0, amax):.3e}")
        assert err <= LOGIT_TOL * max(1.0, amax), (case, name, err)
    for k in ("pos", "rot", "open", "stop", "total"):
        ref = float(fx["loss_" + k])
        print(f"    loss {k}: {losses[k].item():.7f}  ref {ref:.7f}")
        assert abs(losses[k].item() - ref) <= 1e-4 * max(1.0, abs(ref)), (k, losses[k].item(), ref)
    if not train:
        ref = fx["final_actions"]
        assert final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
        err = float(np.abs(final.cpu().numpy() - ref).max())
        print(f"    final actions: err {err:.3e}  dtype {final.dtype}")
        assert final.shape == ref.shape and err <= ACTION_TOL
        assert torch.equal(final[..., :3].float(), m.last_pred[0].detach())      # the position is xt as it is
        return
    assert final is None
    losses["total"].backward()
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


def test_shipped_yaml_trains_as_it_is():
    """preset mp_yaml — qk_norm False, dropouts 0.1, DropPath 0.1, depths [2, 2, 2, 6, 2], 6 + 64 input channels, T = 5 — in train
    mode: one forward + backward, finite, a gradient for every parameter, and the same step seed again gives the same bits."""
    from robot_3dlotus_amd import config as lcfg

    cfg = lcfg.preset("mp_yaml")
    batch = _dev(mu.case_batch("mp_ada_yaml_train"))

    def step(dropout=True):
        torch.manual_seed(5)
        m, _ = _model(cfg)
        if not dropout:
            _no_dropout(m)
        acts, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        named = list(m.named_parameters())
        for n, p in named:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert acts is None and all(torch.isfinite(v).all() for v in losses.values())
        return [losses[k].detach().clone() for k in ("pos", "rot", "open", "stop", "total")] + [p.grad.clone() for _, p in named]

    a, b = step(), step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(step(dropout=False)[4], a[4])     # dropouts and DropPath are on: without them the loss is another one


def test_prefetch_is_bit_identical():
    cfg = mu.case_config("mp_ada_tiny_train")
    host = mu.case_batch("mp_ada_tiny_train")
    perms = [[2, 0, 1, 3], [1, 3, 0, 2]]

    def run(prefetch):
        torch.manual_seed(7)
        m, _ = _model(cfg, 91)
        m.ptv3_model.order_perms = perms
        batch = _dev(host)
        if prefetch:
            m.prefetch(batch)
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        return [losses["total"].detach().clone()] + [t.detach().clone() for t in m.last_pred] + [p.grad.clone() for p in m.parameters()]

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_final_actions_and_loss_dict_contract():
    cfg = mu.case_config("mp_ada_tiny_train")
    m, _ = _model(cfg, 91, train=False)
    m.ptv3_model.order_perms = [[2, 0, 1, 3], [1, 3, 0, 2]]   # (the serialisation orders are drawn per forward otherwise)
    batch = _dev(mu.case_batch("mp_ada_tiny_train"))
    B, T = len(batch["npoints_in_batch"]), cfg.action_config.max_traj_len
    with torch.no_grad():
        final = m(batch)
        final2, losses = m(batch, compute_loss=True, compute_final_action=False)
    assert final.shape == (B, T, 3 + 4 + 2) and final.dtype == torch.float64 and torch.equal(final, final2)
    assert sorted(losses) == ["open", "pos", "rot", "stop", "total"]
    assert torch.equal(m.pred_pos(), m.last_pred[0]) and m.last_pred[0].shape == (B, T, 3)
    m.train()
    out = m(batch, compute_loss=True, compute_final_action=False, decode_actions=True)
    assert out[0] is not None and out[0].shape == (B, T, 9)


def test_published_heatmap_head_on_the_adanorm_backbone():
    """pos_pred_type 'heatmap_disc' with this class: MotionPlannerPTV3CA's head path on the AdaNorm backbone and two-group stem."""
    from robot_3dlotus_amd import synth

    cfg = mu.case_config("mp_ada_tiny_train")
    cfg.action_config.pos_pred_type = "heatmap_disc"
    m, _ = _model(cfg, 91)
    batch = au.last_token_batch(synth.synth_batch_mp(2, 300, ragged=True, seed=3))
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "gt_trajs_disc_pos_probs" else v))
           for k, v in batch.items()}
    final, losses = m(dev, compute_loss=True, decode_actions=True)
    losses["total"].backward()
    assert final.shape == (2, 5, 9) and all(torch.isfinite(v).all() for v in losses.values())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ------------------------------------------------------------------------------------ the stem in two column groups
def test_two_group_stem_equals_the_single_stem():
    """c_pc = 4: [pc | one-hot] is 8 columns wide, which the thin-input stem takes in one call (ops.StemFn, as the policy
    calls it).  The two-group route — conv(W_pc, pc) then conv(W_lab, one-hot) added onto it, a weight gradient per group — must
    give the same output and the same two weight gradients within the per-kernel bar."""
    from robot_3dlotus_amd import adanorm, ops
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm

    cfg = mu.case_config("mp_ada_tiny_train")
    m, _ = _model(cfg, 91)
    m.ptv3_model.order_perms = [[2, 0, 1, 3], [1, 3, 0, 2]]
    batch = _dev(mu.case_batch("mp_ada_tiny_train"))
    seen = {}
    orig = adanorm.StemGroupsFn.apply

    def spy(xa, xb, mod, wa, wb, g, b, rmean, rvar, lvl, training, bank, j):
        seen.update(xa=xa, xb=xb, mod=mod.detach(), g=g.detach(), b=b.detach(), lvl=lvl)
        return orig(xa, xb, mod, wa, wb, g, b, rmean, rvar, lvl, training, bank, j)

    adanorm.StemGroupsFn.apply = spy
    try:
        m(batch, compute_loss=True, compute_final_action=False)
    finally:
        adanorm.StemGroupsFn.apply = orig
    assert seen["xa"].shape[1] == 4 and seen["xb"].shape[1] == 4
    lvl, mod, g, b = seen["lvl"], seen["mod"], seen["g"], seen["b"]
    C = g.shape[0]
    gen = torch.Generator().manual_seed(11)
    w = (0.05 * torch.randn(C, 5, 5, 5, 8, generator=gen)).cuda()
    dy = torch.randn(lvl.n, C, generator=gen).cuda()

    class _Bank:
        def __init__(self):
            self.g = torch.zeros(mod.shape, device="cuda")

        def grad_slice(self, j):
            return self.g

    def run(groups):
        wl = w.clone().requires_grad_(True)
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        if groups:
            y = adanorm.StemGroupsFn.apply(seen["xa"], seen["xb"], mod, wl[..., :4].contiguous(), wl[..., 4:].contiguous(), g, b,
                                           rm, rv, lvl, True, _Bank(), 0)
        else:
            y = ops.StemFn.apply(torch.cat([seen["xa"], seen["xb"]], 1).contiguous(), wl, g, b, rm, rv, lvl, True, mod, _Bank(), 0)
        y.backward(dy)
        ops.sync_side_stream()
        torch.cuda.synchronize()
        return y.detach(), wl.grad.detach(), rm, rv

    (y1, dw1, rm1, rv1), (y2, dw2, rm2, rv2) = run(True), run(False)
    for name, a, r in (("y", y1, y2), ("dW_pc", dw1[..., :4], dw2[..., :4]), ("dW_lab", dw1[..., 4:], dw2[..., 4:]),
                       ("running_mean", rm1, rm2), ("running_var", rv1, rv2)):
        err = float((a.double() - r.double()).abs().max())
        bar = KERNEL_TOL * max(1.0, float(r.abs().max()))
        print(f"    {name}: err {err:.3e}  bar {bar:.3e}")
        assert err <= bar, name
    assert float(dw2.abs().max()) > 0 and isinstance(m, MotionPlannerPTV3AdaNorm)
