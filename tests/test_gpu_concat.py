"""SimplePolicyPTV3Concat on the GPU against the fixtures of the imported reference (tests/golden/concat_*.npz, made by
tests/golden/make_golden_concat.py; bars of tests/test_gpu_reghead.py: head outputs and losses 1e-4, gradients 1e-4 with floor
1e-3, running statistics 2e-3, final actions 1e-5), one training step of the preset concat_yaml with every dropout and DropPath
on, prefetch(), and the published path before and after a Concat step in the same process."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402
import concat_util as cu  # noqa: E402
import ledger  # noqa: E402

TAG = "concat/"
LOGIT_TOL = 1e-4
GRAD_TOL = 1e-4
GRAD_FLOOR = 1e-3
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _concat():
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    return MODEL_FACTORY["SimplePolicyPTV3Concat"]


@pytest.mark.parametrize("case", list(cu.CASES))
def test_concat_fixture_parity(case):
    from weights_util import seeded_state_dict

    fx = cu.load(case)
    cfg = cu.case_config(case)
    assert cfg.model_class == "SimplePolicyPTV3Concat" and cfg.ptv3_config.qk_norm is (case == "concat_tiny_train")
    train = bool(fx["meta_train"])
    batch = cu.case_batch(case)
    assert abs(batch["pc_fts"].double().sum().item() - float(fx["input_checksum"])) < 1e-9
    assert np.array_equal(batch["gt_actions"].numpy(), fx["gt_actions"])
    m = _concat()(cfg)
    sd = seeded_state_dict(m.state_dict(), int(fx["meta_wseed"]), "scaled")
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(fx["weight_checksum"])) < 1e-6 * abs(float(fx["weight_checksum"]))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train(train)
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0
    m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
    final, losses = m(_dev(batch), compute_loss=True, compute_final_action=not train)
    rec = {}
    for name, got in zip(("xt", "xr", "xo"), m.last_pred):
        got = got.detach().cpu().numpy()
        if name == "xt" and "xt" not in fx:   # heat-map logits: a fixed sample of them
            assert list(got.shape) == fx["xt_shape"].tolist()
            ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
            got = got.reshape(-1)[au.xt_sample_index(got.size)]
        else:
            ref = fx[name]
            amax = float(np.abs(ref).max())
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = float(np.abs(got - ref).max())
        rec[name] = err / max(1.0, amax)
        print(f"    {name}: err {err:.3e}  bar {LOGIT_TOL * max(1.0, amax):.3e}")
        assert err <= LOGIT_TOL * max(1.0, amax), (case, name, err)
    for k in ("pos", "rot", "open", "total"):
        ref = float(fx["loss_" + k])
        rec["loss_" + k] = abs(losses[k].item() - ref) / max(1.0, abs(ref))
        print(f"    loss {k}: {losses[k].item():.7f}  ref {ref:.7f}")
        assert abs(losses[k].item() - ref) <= 1e-4 * max(1.0, abs(ref)), (k, losses[k].item(), ref)
    if not train:
        ref = fx["final_actions"]
        assert final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
        err = float(np.abs(final.cpu().numpy() - ref).max())
        rec["final_actions"] = err
        print(f"    final actions: err {err:.3e}")
        ledger.record(TAG + case, **rec)
        assert final.shape == ref.shape and err <= ACTION_TOL
        return
    assert final is None
    losses["total"].backward()
    refs = au.unpack_grads(fx)
    assert sorted(refs) == sorted(n for n, _ in m.named_parameters())
    gmax = max(r[0] for r in refs.values())
    worst, worst_name, fails = 0.0, "", []
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        g = p.grad.detach().cpu()
        rnorm, head, whole, sketch = refs[name]
        if not abs(g.double().norm().item() - rnorm) / (rnorm + GRAD_FLOOR * gmax) < GRAD_TOL:
            fails.append(("norm", name))
        if not float(np.abs(g.flatten()[:head.size].numpy() - head).max()) / (float(np.abs(head).max()) + GRAD_FLOOR * gmax) < 1e-3:
            fails.append(("head", name))
        if whole is not None:
            got, ref, floor = g.double().numpy().reshape(-1), whole.astype(np.float64), GRAD_FLOOR * gmax
        else:
            got, ref, floor = au.grad_sketch(g.numpy()), sketch, GRAD_FLOOR * gmax * np.sqrt(au.SKETCH_K)
        rel = float(np.linalg.norm(got - ref)) / (float(np.linalg.norm(ref)) + floor)
        if rel > worst:
            worst, worst_name = rel, name
        if not rel < GRAD_TOL:
            fails.append(("whole gradient" if whole is not None else "gradient sketch", name, rel))
    stem = "ptv3_model.embedding.stem.conv.weight"
    gs = m.get_parameter(stem).grad
    rec.update(worst_gradient=worst, worst_gradient_name=worst_name,
               stem_grad_norm_rel=abs(gs.double().norm().item() - refs[stem][0]) / (refs[stem][0] + GRAD_FLOOR * gmax))
    print(f"    worst gradient error {worst:.3e} ({worst_name})")
    sdn = m.state_dict()
    worst_buf = 0.0
    for k in fx:
        if k.startswith("buf/"):
            worst_buf = max(worst_buf, float(np.abs(sdn[k[4:]].cpu().numpy() - fx[k]).max()))
    rec["worst_running_stat_abs"] = worst_buf
    ledger.record(TAG + case, **rec)
    assert not fails, fails
    for k in fx:
        if k.startswith("buf/"):
            np.testing.assert_allclose(sdn[k[4:]].cpu().numpy(), fx[k], atol=2e-3, rtol=2e-3, err_msg=k)


def test_concat_yaml_trains_with_every_dropout_on():
    """preset concat_yaml — qk_norm False, dropouts 0.1, DropPath 0.1, depths [2, 2, 2, 6, 2], 6 + 256 input channels — with
    txt_reduce 'attn' (the reference then builds txt_attn_fc and never uses it) in train mode: finite losses and gradients, a
    gradient for every parameter but txt_attn_fc's, the same seed again gives the same bits, and the dropouts do act."""
    from robot_3dlotus_amd import config as lcfg

    cfg = lcfg.preset("concat_yaml")
    cfg.action_config.txt_reduce = "attn"
    batch = _dev(cu.case_batch("concat_yaml_train"))

    def step(drop=True):
        torch.manual_seed(5)
        m = _concat()(cfg).cuda().train()
        assert m.ptv3_model.qk_norm is False
        if not drop:
            m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
            m.act_proj_head.dropout = 0.0
        acts, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        named = list(m.named_parameters())
        for n, p in named:
            if n.startswith("txt_attn_fc."):
                assert p.grad is None, n
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert sum(n.startswith("txt_attn_fc.") for n, _ in named) == 2
        assert acts is None and all(torch.isfinite(v).all() for v in losses.values())
        return [losses[k].detach().clone() for k in ("pos", "rot", "open", "total")] + [p.grad.clone() for _, p in named if p.grad is not None]

    a, b = step(), step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(step(drop=False)[3], a[3])


def test_concat_prefetch_is_bit_identical():
    from robot_3dlotus_amd import config as lcfg
    from weights_util import seeded_state_dict

    cfg = lcfg.preset("concat_tiny")
    host = cu.case_batch("concat_tiny_train")
    perms = [[2, 0, 3, 1], [1, 3, 0, 2]]

    def run(prefetch):
        torch.manual_seed(7)
        m = _concat()(cfg)
        m.load_state_dict(seeded_state_dict(m.state_dict(), 91, "scaled"), strict=True)
        m = m.cuda().train()
        m.ptv3_model.order_perms = perms
        batch = _dev(host)
        if prefetch:
            m.prefetch(batch)
            assert m.ptv3_model._pending is not None
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        assert m.ptv3_model._pending is None
        losses["total"].backward()
        torch.cuda.synchronize()
        return [losses["total"].detach().clone()] + [t.detach().clone() for t in m.last_pred] + [p.grad.clone() for p in m.parameters()]

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_published_path_is_unchanged_by_a_concat_step():
    """preset v1 on v1_scaled_train: bit-identical losses and gradients before and after a Concat step has run in the process
    (new autograd functions and kernels, shared workspaces)."""
    import golden_util as gu
    from robot_3dlotus_amd import config as lcfg
    from robot_3dlotus_amd.policy import SimplePolicyPTV3CA

    fx, cfg, batch, sd = gu.load_case("v1_scaled_train", gu.state_template(lcfg.preset("v1")))
    batch = _dev(batch)

    def step():
        m = SimplePolicyPTV3CA(cfg)
        m.load_state_dict(sd)
        m = m.cuda().train()
        m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
        m.act_proj_head.dropout = 0.0
        m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        return [losses[k].detach().clone() for k in ("pos", "rot", "open", "total")] + [p.grad.clone() for p in m.parameters()]

    before = step()
    assert abs(before[3].item() - float(fx["loss_total"])) <= 1e-4 * max(1.0, abs(float(fx["loss_total"])))
    torch.manual_seed(0)
    r = _concat()(lcfg.preset("concat_tiny")).cuda().train()
    _, lr = r(_dev(cu.case_batch("concat_tiny_train")), compute_loss=True, compute_final_action=False)
    lr["total"].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(lr["total"])
    after = step()
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
