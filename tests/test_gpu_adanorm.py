"""GPU checks of SimplePolicyPTV3AdaNorm: parity with the fixtures of the imported reference (tests/golden/adanorm_*.npz),
the modulated-norm entry points of csrc/adanorm.hip against float64 torch, and the full-size v1 model."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adanorm_util as au  # noqa: E402

LOGIT_TOL = 1e-4
GRAD_TOL = 1e-4
GRAD_FLOOR = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


@pytest.mark.parametrize("case", list(au.CASES))
def test_adanorm_fixture_parity(case):
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm
    from weights_util import seeded_state_dict

    fx = au.load(case)
    cfg = au.case_config(case)
    train = bool(fx["meta_train"])
    batch = au.case_batch(case)
    assert abs(batch["pc_fts"].double().sum().item() - float(fx["input_checksum"])) < 1e-9
    m = SimplePolicyPTV3AdaNorm(cfg)
    sd = seeded_state_dict(m.state_dict(), int(fx["meta_wseed"]), "scaled")
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(fx["weight_checksum"])) < 1e-6 * abs(float(fx["weight_checksum"]))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train(train)
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0
    m.ptv3_model.order_perms = [p.tolist() for p in fx["perms"]]
    _, losses = m(_dev(batch), compute_loss=True, compute_final_action=False)
    for name, got in zip(("xt", "xr", "xo"), m.last_pred):
        got = got.detach().cpu().numpy()
        if name == "xt" and "xt" not in fx:  # train-mode fixtures keep a fixed sample of the position logits
            assert list(got.shape) == fx["xt_shape"].tolist()
            ref, amax = fx["xt_sample"], float(fx["xt_absmax"])
            got = got.reshape(-1)[au.xt_sample_index(got.size)]
        else:
            ref = fx[name]
            amax = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max())
        assert err <= LOGIT_TOL * max(1.0, amax), (case, name, err)
    for k in ("pos", "rot", "open", "total"):
        ref = float(fx["loss_" + k])
        assert abs(losses[k].item() - ref) <= 1e-4 * max(1.0, abs(ref)), (k, losses[k].item(), ref)
    if not train:
        return
    losses["total"].backward()
    refs = au.unpack_grads(fx)
    assert sorted(refs) == sorted(n for n, _ in m.named_parameters())
    gmax = max(r[0] for r in refs.values())
    n_whole = n_sketch = 0
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        g = p.grad.detach().cpu()
        rnorm, head, whole, sketch = refs[name]
        assert abs(g.double().norm().item() - rnorm) / (rnorm + GRAD_FLOOR * gmax) < GRAD_TOL, ("norm", name)
        assert float(np.abs(g.flatten()[:head.size].numpy() - head).max()) / (float(np.abs(head).max()) + GRAD_FLOOR * gmax) < 1e-3, name
        if whole is not None:
            got, ref, floor = g.double().numpy().reshape(-1), whole.astype(np.float64), GRAD_FLOOR * gmax
            n_whole += 1
        else:
            # E ||sketch(E)||^2 = K ||E||_F^2: the floor scales by sqrt(K) like the sketch itself
            got, ref, floor = au.grad_sketch(g.numpy()), sketch, GRAD_FLOOR * gmax * np.sqrt(au.SKETCH_K)
            n_sketch += 1
        rel = float(np.linalg.norm(got - ref)) / (float(np.linalg.norm(ref)) + floor)
        assert rel < GRAD_TOL, ("whole gradient" if whole is not None else "gradient sketch", name, rel)
    assert n_whole > 0 and n_sketch > 0
    sdn = m.state_dict()
    for k in fx:
        if k.startswith("buf/"):
            np.testing.assert_allclose(sdn[k[4:]].cpu().numpy(), fx[k], atol=2e-3, rtol=2e-3, err_msg=k)


# ------------------------------------------------------------------------------------ kernels vs float64
class _Lvl:
    def __init__(self, counts):
        self.counts = list(counts)
        self.off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")


def _mods(B, C, width, seed):
    g = torch.Generator().manual_seed(seed)
    slab = (0.5 * torch.randn(B, width, generator=g)).cuda()
    return slab, slab[:, 3 * 4:3 * 4 + 2 * C]   # a column slice of a wider slab (row stride = width)


def _ref_mod(counts, mod):
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).cuda()
    m = mod.double()[idx]
    C = mod.shape[1] // 2
    return m[:, :C], m[:, C:], idx


COUNTS = {"ragged": [37, 1, 300, 5, 129], "b1": [411], "b16": [int(v) for v in np.random.default_rng(3).integers(1, 90, 16)]}


@pytest.mark.parametrize("C", [64, 128, 256, 512, 768])
@pytest.mark.parametrize("layout", list(COUNTS))
def test_adaln_kernels_against_float64(C, layout):
    from robot_3dlotus_amd import adanorm as an

    counts = COUNTS[layout]
    M, B = sum(counts), len(counts)
    lvl = _Lvl(counts)
    torch.manual_seed(C + M)
    x = (torch.randn(M, C) * 2 + 0.5).cuda()
    res = torch.randn(M, C).cuda()
    g, b = (1 + 0.2 * torch.randn(C)).cuda(), (0.2 * torch.randn(C)).cuda()
    slab, mod = _mods(B, C, 2 * C + 20, C)
    dy, add = torch.randn(M, C).cuda(), torch.randn(M, C).cuda()
    dslab = torch.full_like(slab, 7.0)
    dmod = dslab[:, 12:12 + 2 * C]

    def run():
        y, mean, rstd = an.adaln_fwd(x, g, b, mod, lvl, res=res)
        dx, dg, db = an.adaln_bwd(dy, x, mean, rstd, g, b, mod, dmod, lvl, add=add)
        return [t.clone() for t in (y, dx, dg, db, dslab)]

    y, dx, dg, db, ds = run()
    xd = x.double().requires_grad_()
    gd, bd = g.double().requires_grad_(), b.double().requires_grad_()
    md = mod.double().requires_grad_()
    sh, sc, idx = _ref_mod(counts, md)
    yr = torch.nn.functional.layer_norm(xd, (C,), gd, bd, 1e-5) * (1 + sc) + sh + res.double()
    yr.backward(dy.double())
    tol = 2e-5
    assert (y.double() - yr.detach()).abs().max() < tol * yr.abs().max()
    assert (dx.double() - add.double() - xd.grad).abs().max() < tol * max(1.0, xd.grad.abs().max().item())
    for got, ref in ((dg, gd.grad), (db, bd.grad), (ds[:, 12:12 + 2 * C], md.grad)):
        assert (got.double() - ref).abs().max() < tol * max(1.0, ref.abs().max().item())
    assert (ds[:, :12] == 7.0).all() and (ds[:, 12 + 2 * C:] == 7.0).all()   # nothing outside the norm's slice is written
    again = run()
    assert all(torch.equal(a, b_) for a, b_ in zip((y, dx, dg, db, ds), again))


@pytest.mark.parametrize("C", [64, 128, 256, 512, 768])
@pytest.mark.parametrize("layout", list(COUNTS))
@pytest.mark.parametrize("training", [True, False])
def test_adabn_kernels_against_float64(C, layout, training):
    from robot_3dlotus_amd import adanorm as an

    counts = COUNTS[layout]
    M, B = sum(counts), len(counts)
    lvl = _Lvl(counts)
    torch.manual_seed(C + M + training)
    x = (torch.randn(M, C) * 1.5 + 0.3).cuda()
    g, b = (1 + 0.2 * torch.randn(C)).cuda(), (0.2 * torch.randn(C)).cuda()
    rm0, rv0 = (0.1 * torch.randn(C)).cuda(), (0.5 + torch.rand(C)).cuda()
    slab, mod = _mods(B, C, 2 * C + 20, C + 1)
    dy = torch.randn(M, C).cuda()
    dslab = torch.zeros_like(slab)
    dmod = dslab[:, 12:12 + 2 * C]

    def run():
        rm, rv = rm0.clone(), rv0.clone()
        y, mean, invstd = an.adabn_fwd(x, g, b, rm, rv, mod, lvl, training)
        dx, dg, db = an.adabn_bwd(dy, x, mean, invstd, g, b, mod, dmod, lvl, training)
        return [t.clone() for t in (y, dx, dg, db, dslab, rm, rv)]

    y, dx, dg, db, ds, rm, rv = run()
    xd = x.double().requires_grad_()
    gd, bd = g.double().requires_grad_(), b.double().requires_grad_()
    md = mod.double().requires_grad_()
    sh, sc, _ = _ref_mod(counts, md)
    rmd, rvd = rm0.double().clone(), rv0.double().clone()
    n = torch.nn.functional.batch_norm(xd, rmd, rvd, gd, bd, training, 0.01, 1e-3)
    yr = torch.nn.functional.gelu(n * (1 + sc) + sh)
    yr.backward(dy.double())
    tol = 3e-5
    assert (y.double() - yr.detach()).abs().max() < tol * max(1.0, yr.abs().max().item())
    for got, ref in ((dx, xd.grad), (dg, gd.grad), (db, bd.grad), (ds[:, 12:12 + 2 * C], md.grad)):
        assert (got.double() - ref).abs().max() < tol * max(1.0, ref.abs().max().item())
    if training:
        assert (rm.double() - rmd).abs().max() < 1e-5 and (rv.double() - rvd).abs().max() < 1e-5
    again = run()
    assert all(torch.equal(a, b_) for a, b_ in zip((y, dx, dg, db, ds, rm, rv), again))


def test_silu_and_modulation_product():
    from robot_3dlotus_amd import ops

    c = torch.randn(5, 256, device="cuda", requires_grad=True)
    ws = [torch.randn(2 * C, 256, device="cuda", requires_grad=True) * 0.05 for C in (64, 128)]
    ws = [w.detach().requires_grad_() for w in ws]
    bs = [torch.randn(w.shape[0], device="cuda", requires_grad=True) for w in ws]
    bank = ops.ProjBank()
    outs = ops.ProjAllFn.apply(c, bank, "silu", ws[0], bs[0], ws[1], bs[1])
    cd = c.detach().double().requires_grad_()
    wd = [w.detach().double().requires_grad_() for w in ws]
    bd = [b.detach().double().requires_grad_() for b in bs]
    refs = [torch.nn.functional.linear(torch.nn.functional.silu(cd), w, b) for w, b in zip(wd, bd)]
    gs = [torch.randn_like(o) for o in outs]
    for o, r in zip(outs, refs):
        assert (o.double() - r).abs().max() < 1e-5 * max(1.0, r.abs().max().item())
    torch.autograd.backward(list(outs), gs)
    torch.autograd.backward(refs, [g.double() for g in gs])
    for got, ref in [(c.grad, cd.grad)] + [(w.grad, r.grad) for w, r in zip(ws, wd)] + [(b.grad, r.grad) for b, r in zip(bs, bd)]:
        assert (got.double() - ref).abs().max() < 1e-4 * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------ full size
_STEP = r"""
import sys, torch, numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import robot_3dlotus_amd
from robot_3dlotus_amd import config as lcfg, synth
from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm
import adanorm_util as au
torch.manual_seed(5)
m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).cuda().train()
b = au.last_token_batch(synth.augment_clouds(synth.synth_batch(16, 4096, seed=1), seed=2))
b = {{k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v)) for k, v in b.items()}}
_, losses = m(b, compute_loss=True, compute_final_action=False)
losses["total"].backward()
torch.cuda.synchronize()
out = {{"loss_" + k: v.detach().cpu().numpy() for k, v in losses.items()}}
for n, p in m.named_parameters():
    out["g/" + n] = p.grad.cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def test_full_size_two_processes_bit_identical(tmp_path):
    script = tmp_path / "step.py"
    script.write_text(_STEP.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    outs = []
    for i in range(2):
        path = str(tmp_path / f"r{i}.npz")
        subprocess.run([sys.executable, str(script), path], check=True, timeout=600)
        outs.append(dict(np.load(path)))
    a, b = outs
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


def test_full_size_train_eval_optimise_and_checkpoint(tmp_path):
    from robot_3dlotus_amd import checkpoint, config as lcfg, synth
    from robot_3dlotus_amd.optim import AdamW
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm

    torch.manual_seed(0)
    m = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).cuda().train()
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0
    batch = _dev(au.last_token_batch(synth.augment_clouds(synth.synth_batch(16, 4096, seed=3), seed=4)))
    m.ptv3_model.order_perms = [[0, 1, 2, 3]] * 5
    opt = AdamW(m.parameters(), lr=1e-4)
    first = None
    for step in range(4):
        opt.zero_grad()
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        assert all(torch.isfinite(v).all() for v in losses.values())
        for n_, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n_
        opt.step()
        first = losses["total"].item() if first is None else first
    last = losses["total"].item()
    assert last < first, (first, last)
    # eval at B = 1 (running statistics)
    m.eval()
    one = _dev(au.last_token_batch(synth.synth_batch(1, 4096, seed=5)))
    with torch.no_grad():
        acts = m(one, compute_loss=False)
    assert acts.shape == (1, 8) and torch.isfinite(acts).all()
    # checkpoint round trip (reference file format, strict load)
    path = checkpoint.ModelSaver(str(tmp_path)).save(m, 4)
    m2 = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1"))
    kept, _ = checkpoint.load_model_checkpoint(m2, path, strict=True)
    assert kept == len(m.state_dict())
    m2 = m2.cuda().eval()
    m2.ptv3_model.order_perms = m.ptv3_model.order_perms
    with torch.no_grad():
        m(one, compute_loss=False)
        a = [t.clone() for t in m.last_pred]
        m2(one, compute_loss=False)
    assert all(torch.equal(x, y) for x, y in zip(a, m2.last_pred))
