"""GPU checks of the regression action head (pos_pred_type 'heatmap_mlp', rot_pred_type 'euler' / 'quat'): the entry points of
csrc/reg_head.hip and the 4-column dense gradients against float64 torch expressions, the policies against the fixtures of the
imported reference (tests/golden/reghead_*.npz), the three `*_reg` presets as drop-ins and the unchanged published path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402
import reghead_util as ru  # noqa: E402

KERNEL_TOL = 2e-5   # x max(1, |ref|max): the per-kernel bar
LOGIT_TOL = 1e-4    # the bars of tests/test_gpu_adanorm.py for head outputs, losses, gradients and running statistics
GRAD_TOL = 1e-4
GRAD_FLOOR = 1e-3
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _close(got, ref, tol=KERNEL_TOL):
    ref = ref.double()
    err = (got.double() - ref).abs().max().item()
    bar = tol * max(1.0, ref.abs().max().item())
    print(f"    err {err:.3e}  bar {bar:.3e}")
    return err <= bar


class _Lvl:
    def __init__(self, counts):
        self.counts = list(counts)
        self.off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
        self.batch = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts)).cuda()


# ------------------------------------------------------------------------------------ soft position
LAYOUTS = {"sizes": [1, 63, 64, 65, 257], "b1": [300], "ragged": [40, 1, 4099, 1, 129], "big": [70001]}


def _softpos_case(counts, C, seed, scale0=1.0):
    g = torch.Generator().manual_seed(seed)
    N, B = sum(counts), len(counts)
    h = torch.randn(N, C, generator=g)
    w3 = 0.2 * torch.randn(4, C, generator=g)
    w3[0] *= scale0
    b3 = 0.1 * torch.randn(4, generator=g)
    pc = torch.randn(N, 7, generator=g)       # xyz in the leading columns of a wider row (stride 7)
    gx = torch.randn(B, 3, generator=g)
    return [t.cuda() for t in (h, w3, b3, pc, gx)]


def _softpos_run(h, w3, b3, pc, gx, lvl, temp):
    from robot_3dlotus_amd import ops

    e, xt, stats = ops.softpos_fwd(h, w3, b3, pc, lvl, temp)
    de = ops.softpos_bwd(gx, e, pc, lvl, stats, xt, temp)
    torch.cuda.synchronize()
    return e, xt, stats, de


def _softpos_ref(e64, pc, gx, counts, temp):
    """float64 restatement from given logits e: (xt, (max, lse) per cloud, de = d sum(gx * xt) / de)."""
    e64 = e64.detach().clone().requires_grad_()
    xt = ru.softpos(e64, pc.double()[:, :3], counts, temp)
    (xt * gx.double()).sum().backward()
    z = torch.split(e64.detach()[:, 0] / temp, list(counts))
    stats = torch.stack([torch.stack([v.max(), torch.logsumexp(v, 0)]) for v in z], 0)
    return xt.detach(), stats, e64.grad


@pytest.mark.parametrize("temp", [1.0, 0.1])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_softpos_kernels_against_float64(layout, C, temp):
    counts = LAYOUTS[layout]
    lvl = _Lvl(counts)
    h, w3, b3, pc, gx = _softpos_case(counts, C, 7 * C + len(counts))
    e, xt, stats, de = _softpos_run(h, w3, b3, pc, gx, lvl, temp)
    e_ref = h.double() @ w3.double().t() + b3.double()
    assert _close(e, e_ref)
    # the whole pass against float64 from the inputs, and the softmax stage alone from the logits the kernel stored
    for src in (e_ref, e.double()):
        xt_ref, st_ref, de_ref = _softpos_ref(src, pc, gx, counts, temp)
        assert _close(xt, xt_ref) and _close(stats, st_ref) and _close(de, de_ref)
    # a directional finite difference of the restatement (float64 on the host, no autograd) against the kernel's de: the
    # direction has unit L1 norm on the eight largest entries of de, so |<de - de_ref, d>| <= max |de - de_ref| (Hoelder) and the
    # bar is the kernel's
    de_c, e_c, xyz_c, gx_c = de_ref.cpu(), e.double().cpu(), pc.double()[:, :3].cpu(), gx.double().cpu()
    top = de_c.abs().flatten().topk(min(8, de_c.numel())).indices
    d = torch.zeros_like(de_c).flatten()
    d[top] = torch.sign(de_c.flatten()[top]) / len(top)
    d = d.view_as(de_c)
    eps = 1e-5

    def loss(ee):
        return (ru.softpos(ee, xyz_c, counts, temp) * gx_c).sum().item()

    fd = (loss(e_c + eps * d) - loss(e_c - eps * d)) / (2 * eps)
    got = (de.double().cpu() * d).sum().item()
    bar = KERNEL_TOL * max(1.0, de_c.abs().max().item()) + 1e-8   # (+ the truncation / rounding of the difference quotient)
    print(f"    fd {fd:.9e}  <de, d> {got:.9e}  bar {bar:.3e}")
    assert abs(fd - got) <= bar
    again = _softpos_run(h, w3, b3, pc, gx, lvl, temp)
    assert all(torch.equal(a, b) for a, b in zip((e, xt, stats, de), again))


@pytest.mark.parametrize("layout", ["sizes", "ragged"])
def test_softpos_stays_finite_at_large_logits(layout):
    """|e_0| / temp ~ 1e3: exp() of the raw logits overflows in every format; with the maximum subtracted nothing does."""
    counts, temp = LAYOUTS[layout], 0.1
    lvl = _Lvl(counts)
    h, w3, b3, pc, gx = _softpos_case(counts, 128, 5, scale0=12.0)
    e, xt, stats, de = _softpos_run(h, w3, b3, pc, gx, lvl, temp)
    zmax = (e[:, 0].abs().max() / temp).item()
    print(f"    max |e0| / temp = {zmax:.1f}")
    assert 500 < zmax < 5000
    assert all(torch.isfinite(t).all() for t in (e, xt, stats, de))
    assert _close(e, h.double() @ w3.double().t() + b3.double())
    xt_ref, st_ref, de_ref = _softpos_ref(e.double(), pc, gx, counts, temp)
    assert _close(xt, xt_ref) and _close(stats, st_ref) and _close(de, de_ref)


# ------------------------------------------------------------------------------------ dense gradients, 4 output columns
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("M", [1, 5, 4096, 70001])
def test_linear_gradients_at_four_columns(M, K):
    """lotus_linear_wgrad / lotus_linear_dgrad with N = 4 (heatmap_mlp.3 of the regression head), the dgrad with the fused
    LeakyReLU' and dropout mask of HeadLossFn.backward."""
    from robot_3dlotus_amd import ops

    g = torch.Generator().manual_seed(M + K)
    dy, x = torch.randn(M, 4, generator=g).cuda(), torch.randn(M, K, generator=g).cuda()
    w, pre = torch.randn(4, K, generator=g).cuda(), torch.randn(M, K, generator=g).cuda()
    dw, db = ops.linear_wgrad(dy, x)
    ops.sync_side_stream()
    dx = ops.linear_dgrad(dy, w)
    dxa = ops.linear_dgrad(dy, w, pre=pre, act=ops.ACT_LEAKY)
    seed = ops.mix_seed(3, M)
    dxd = ops.linear_dgrad(dy, w, pre=pre, act=ops.ACT_LEAKY, drop_p=0.25, seed=seed)
    mask = ops.dropout(torch.ones_like(pre), 0.25, seed)    # the same counter-hash mask, scaled by 1 / keep
    torch.cuda.synchronize()
    ref = dy.double() @ w.double()
    slope = torch.where(pre > 0, 1.0, 0.02).double()
    assert _close(dw, dy.double().t() @ x.double()) and _close(db, dy.double().sum(0))
    assert _close(dx, ref) and _close(dxa, ref * slope) and _close(dxd, ref * slope * mask.double())


# ------------------------------------------------------------------------------------ [B]-sized losses
def _reg_loss_case(B, rot, W, seed, flip0=False):
    """ae [B, W], gt, with both branches of the rotation's selection in the batch and a zero euler target."""
    g = torch.Generator().manual_seed(seed)
    ae = torch.randn(B, W, generator=g)
    pos = 0.1 * torch.randn(B, 3, generator=g)
    opn = torch.randint(0, 2, (B, 1), generator=g).float()
    if rot == "euler":
        ae[:, :3] = torch.rand(B, 3, generator=g) * 1.6 - 0.8
        r = torch.from_numpy(ru.rot_labels("euler", B, seed))
        ae[0, :3] = torch.tensor([-0.5, 0.1, 0.3])
        r[0] = torch.tensor([0.9, 0.3, 0.0])       # wrapped candidate (-1.1), the target itself, a zero target
    elif rot == "quat":
        x = ae[:, :4] / ae[:, :4].norm(dim=1, keepdim=True)
        r = x + 0.3 * torch.randn(B, 4, generator=g)
        r = r / r.norm(dim=1, keepdim=True)
        sign = torch.where(torch.arange(B) % 2 == (1 if flip0 else 0), 1.0, -1.0)   # every other target negated
        r = r * sign[:, None]
    else:
        r = torch.randint(0, (W - 1) // 3, (B, 3), generator=g).float()
    return ae.cuda(), torch.cat([pos, r, opn], 1).cuda()


def _reg_loss_run(ae, gt, xt, ce, rot, gl, pos_w, rot_w):
    from robot_3dlotus_amd import ops
    from robot_3dlotus_amd._capi import call

    B, W = ae.shape
    kind = ops.ROT_KINDS[rot]
    losses = torch.zeros(4, device="cuda")
    dae, dpos = torch.full((B, W), 7.0, device="cuda"), torch.full((B, 3), 7.0, device="cuda")
    xr = torch.empty(B, 4, device="cuda") if kind == 2 else None
    call("lotus_reg_loss_fwd", ae, gt, xt, ce, 4, B, W, gt.shape[1], kind, (W - 1) // 3 if kind == 0 else 0, pos_w, rot_w, losses,
         dae, dpos, xr)
    outs = []
    for gg in (gl, 2 * gl):
        dae_o, dpos_o = torch.empty_like(dae), torch.empty_like(dpos)
        call("lotus_reg_loss_bwd", dae, dpos, gg, pos_w, rot_w, B, W, dae_o, dpos_o)
        outs.append((dae_o, dpos_o))
    torch.cuda.synchronize()
    return losses, xr, outs


@pytest.mark.parametrize("pos", ["heatmap_mlp", "heatmap_disc"])
@pytest.mark.parametrize("rot,W", [("euler", 4), ("euler", 5), ("quat", 5), ("quat", 6), ("euler_disc", 217)])
@pytest.mark.parametrize("B", [1, 2, 16, 129])
def test_reg_loss_kernels_against_float64(B, rot, W, pos):
    pos_w, rot_w = 1.5, 0.75
    for flip0 in ((False, True) if (rot == "quat" and B == 1) else (False,)):
        ae, gt = _reg_loss_case(B, rot, W, 100 * B + W, flip0)
        g = torch.Generator().manual_seed(B)
        gl = (0.5 + torch.rand(4, generator=g)).cuda()
        xt = (0.1 * torch.randn(B, 3, generator=g)).cuda()
        ce = (3 + torch.randn(B * 3, 4, generator=g)).cuda()     # column 0: cross entropy per (cloud, axis), stride 4
        mlp = pos == "heatmap_mlp"
        losses, xr, ((dae, dpos), (dae2, dpos2)) = _reg_loss_run(ae, gt, xt if mlp else None, None if mlp else ce, rot, gl, pos_w, rot_w)
        # float64 restatement
        a64 = ae.double().requires_grad_()
        x64 = xt.double().requires_grad_()
        c64 = ce[:, 0].double().requires_grad_()
        g64 = gt.double()
        if rot == "quat":
            xr64 = a64[:, :4] / a64[:, :4].square().sum(-1, keepdim=True).sqrt()
        elif rot == "euler":
            xr64 = a64[:, :3]
        else:
            xr64 = a64[:, :W - 1].view(B, -1, 3)
        ref = ru.losses(x64, xr64, a64[:, -1], g64, "heatmap_mlp", rot, pos_w=pos_w, rot_w=rot_w)
        if not mlp:
            ref["pos"] = c64.mean()
            ref["total"] = pos_w * ref["pos"] + rot_w * ref["rot"] + ref["open"]
        if rot != "euler_disc":
            la, lb = ru.rot_candidates(xr64.detach(), g64[:, 3:-1], rot)
            sel = la < lb
            if rot == "euler":
                assert bool(sel.any()) and bool((~sel).any()) and bool((g64[:, 3:-1] == 0).any())
            else:
                assert bool(sel[0]) != flip0 and (B == 1 or (bool(sel.any()) and bool((~sel).any())))
        lvec = torch.stack([ref[k] for k in ("pos", "rot", "open", "total")])
        (lvec * gl.double()).sum().backward()
        assert _close(losses, lvec.detach())
        assert _close(dae, a64.grad) and _close(dpos, x64.grad if mlp else c64.grad.view(B, 3))
        if rot == "quat":
            assert _close(xr, xr64.detach())
        # columns of neither loss get an exact zero; the upstream gradient scales the result (a factor of two: exactly)
        nrot = {"euler": 3, "quat": 4, "euler_disc": W - 1}[rot]
        assert (dae[:, nrot:W - 1] == 0).all() and (a64.grad[:, nrot:W - 1] == 0).all()
        assert torch.equal(dae2, 2 * dae) and torch.equal(dpos2, 2 * dpos)


# ------------------------------------------------------------------------------------ models against the fixtures
def _policy(name):
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA

    return {"ca": SimplePolicyPTV3CA, "adanorm": SimplePolicyPTV3AdaNorm}[ru.CASES[name][0]]


@pytest.mark.parametrize("case", list(ru.CASES))
def test_reghead_fixture_parity(case):
    from weights_util import seeded_state_dict

    fx = ru.load(case)
    cfg = ru.case_config(case)
    train = bool(fx["meta_train"])
    batch = ru.case_batch(case)
    assert abs(batch["pc_fts"].double().sum().item() - float(fx["input_checksum"])) < 1e-9
    assert np.array_equal(batch["gt_actions"].numpy(), fx["gt_actions"])
    m = _policy(case)(cfg)
    sd = seeded_state_dict(m.state_dict(), int(fx["meta_wseed"]), "scaled")
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(fx["weight_checksum"])) < 1e-6 * abs(float(fx["weight_checksum"]))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train(train)
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0
    m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
    final, losses = m(_dev(batch), compute_loss=True, compute_final_action=not train)
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
        print(f"    {name}: err {err:.3e}  bar {LOGIT_TOL * max(1.0, amax):.3e}")
        assert err <= LOGIT_TOL * max(1.0, amax), (case, name, err)
    for k in ("pos", "rot", "open", "total"):
        ref = float(fx["loss_" + k])
        print(f"    loss {k}: {losses[k].item():.7f}  ref {ref:.7f}")
        assert abs(losses[k].item() - ref) <= 1e-4 * max(1.0, abs(ref)), (k, losses[k].item(), ref)
    if not train:
        ref = fx["final_actions"]
        assert train is False and final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
        err = float(np.abs(final.cpu().numpy() - ref).max())
        print(f"    final actions: err {err:.3e}")
        assert final.shape == ref.shape and err <= ACTION_TOL
        return
    assert final is None
    losses["total"].backward()
    refs = au.unpack_grads(fx)
    assert sorted(refs) == sorted(n for n, _ in m.named_parameters())
    gmax = max(r[0] for r in refs.values())
    worst = 0.0
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
        worst = max(worst, rel)
        assert rel < GRAD_TOL, ("whole gradient" if whole is not None else "gradient sketch", name, rel)
    print(f"    worst gradient error {worst:.3e}")
    sdn = m.state_dict()
    for k in fx:
        if k.startswith("buf/"):
            np.testing.assert_allclose(sdn[k[4:]].cpu().numpy(), fx[k], atol=2e-3, rtol=2e-3, err_msg=k)


def test_unused_action_column_gets_a_zero_gradient():
    """dim_actions = 8 with 'euler' (the YAML's own values): action_mlp.3 has 5 rows, row 3 enters no loss."""
    from robot_3dlotus_amd import config as lcfg, synth
    from robot_3dlotus_amd.policy import SimplePolicyPTV3CA

    torch.manual_seed(1)
    cfg = lcfg.load_model_config(None, lcfg.TINY_OVERRIDES + ru.head_overrides("heatmap_mlp", "euler", 8, 0.1))
    m = SimplePolicyPTV3CA(cfg).cuda().train()
    _, losses = m(_dev(synth.synth_batch(2, 512, seed=3, rot_type="euler")), compute_loss=True, compute_final_action=False)
    losses["total"].backward()
    w, b = m.act_proj_head.action_mlp[3].weight.grad, m.act_proj_head.action_mlp[3].bias.grad
    assert w.shape == (5, 64) and (w[3] == 0).all() and b[3] == 0
    assert all((w[i] != 0).any() for i in (0, 1, 2, 4))


# ------------------------------------------------------------------------------------ drop-in, unchanged path
@pytest.mark.parametrize("preset", ["tiny_reg", "v1_reg", "adanorm_tiny_reg"])
def test_reg_presets_train_step(preset):
    from robot_3dlotus_amd import config as lcfg, synth
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    torch.manual_seed(0)
    cfg = lcfg.preset(preset)
    m = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
    batch = synth.synth_batch(2, 1024, ragged=True, seed=9, rot_type="euler")
    if preset.startswith("adanorm"):
        batch = au.last_token_batch(batch)
    acts, losses = m(_dev(batch), compute_loss=True, compute_final_action=False)
    assert acts is None and all(torch.isfinite(v).all() for v in losses.values())
    losses["total"].backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    m.eval()
    with torch.no_grad():
        acts = m(_dev(batch))
    assert acts.shape == (2, 8) and acts.dtype == torch.float32 and torch.isfinite(acts).all()
    assert torch.equal(acts[:, :3], m.last_pred[0])   # pred_pos of the final action is xt itself


@pytest.mark.parametrize("pos,rot,da,dtype", [("heatmap_disc", "quat", 8, torch.float32), ("heatmap_mlp", "euler_disc", 7, torch.float64),
                                              ("heatmap_disc", "euler", 7, torch.float32)])
def test_other_combinations_decode(pos, rot, da, dtype):
    from robot_3dlotus_amd import config as lcfg, synth
    from robot_3dlotus_amd.policy import SimplePolicyPTV3CA

    torch.manual_seed(2)
    m = SimplePolicyPTV3CA(lcfg.load_model_config(None, lcfg.TINY_OVERRIDES + ru.head_overrides(pos, rot, da, 0.1))).cuda().train()
    batch = _dev(synth.synth_batch(2, 512, ragged=True, seed=4, rot_type=rot))
    acts, losses = m(batch, compute_loss=True, compute_final_action=False, decode_actions=True)
    losses["total"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert acts.shape == (2, 8) and acts.dtype == dtype and torch.isfinite(acts).all()
    if pos == "heatmap_disc":
        assert torch.equal(acts[:, :3].float(), batch["gt_actions"][:, :3])    # compute_final_action=False: the ground truth
    if rot == "quat":
        assert torch.allclose(acts[:, 3:7].norm(dim=1), torch.ones(2, device="cuda"), atol=1e-6)


def test_published_path_is_unchanged_by_the_new_module():
    """preset v1 on v1_scaled_train: bit-identical losses and gradients before and after the regression head has run in the
    process (separate autograd function, separate kernels, shared workspace)."""
    import golden_util as gu
    from robot_3dlotus_amd import config as lcfg, synth
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
    r = SimplePolicyPTV3CA(lcfg.preset("tiny_reg")).cuda().train()
    _, lr = r(_dev(synth.synth_batch(2, 512, seed=9, rot_type="euler")), compute_loss=True, compute_final_action=False)
    lr["total"].backward()
    torch.cuda.synchronize()
    after = step()
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
