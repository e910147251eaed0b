"""Attention without q/k LayerNorm (qk_norm False) on the GPU.

Kernel level: the NORM = false tile kernels through the raw entry points (qn = kn = None) on tests/edge_layouts.patch_edges()
— patches of 1, 2, 31 .. 33, 63 .. 65, 127 and 128 rows, 0 / 1 / 127 borrowed rows — at head widths 32, 24 and 16 and on the
four curve slots, against the float64 restatement of tests/plainattn_util.py (pinned to oracle.model.patch_attention by
tests/test_plainattn_host.py).  The bars are those of the same kernels with the norm (tests/test_gpu_edge_layouts.py): forward
5e-6, dqkv 2e-5, relative to max(1, |ref|max); they were measured on normalised operands, whose logits have a spread of about 1,
so q and k are drawn as randn of scale 1.0 here.  Guarded caller-owned buffers, errors per cloud into the ledger, every case run
twice bit for bit, and once more in a child interpreter under LOTUS_XQ=2, where a with-norm call would move to the
query-per-lane kernels and a no-norm call must not.

Model level: SimplePolicyPTV3AdaNorm with qk_norm False against the fixtures of the imported reference
(tests/golden/plain_adanorm_*.npz, bars of tests/test_gpu_adanorm.py / test_gpu_reghead.py), and the shipped YAML as it is —
dropouts and DropPath on — for one training step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child interpreter of test_plain_attention_stays_on_the_tile_kernels_under_xq2
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import adanorm_util as au  # noqa: E402
import ledger  # noqa: E402
import plainattn_util as pu  # noqa: E402
import test_gpu_edge_layouts as ge  # noqa: E402  (helpers only: guarded buffers, per-cloud bars, the level cache, _patch_run)

TAG = "plain_attention/"
FWD_TOL, DQKV_TOL = 5e-6, 2e-5
LOGIT_TOL = 1e-4    # the bars of tests/test_gpu_adanorm.py / test_gpu_reghead.py
GRAD_TOL = 1e-4
GRAD_FLOOR = 1e-3
ACTION_TOL = 1e-5


def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


# ------------------------------------------------------------------------------------------------ kernels
def _plain_run(C, H, slot):
    """The case on the device, qn = kn = None -> (buffers, level, oracle level tables, counts, inputs)."""
    ops = ge._ops()
    pc, counts, txt, ref, got = ge._levels("patch", "", 1)
    r, lv = ref[0], got[0].for_order(slot)
    qkv, dout = pu.plain_inputs(C, lv.n, seed=1000 + C + H + slot)
    routes = []
    b, gr = ge._patch_run(ops, lv, qkv.cuda(), None, None, dout.cuda(), C, H, routes=routes)
    ge._guards_intact(**b)
    assert gr == [None] * 4
    # the NORM = false tile pair whatever LOTUS_XQ says (this runs in the LOTUS_XQ=2 child too): norm 0, no norm-gradient
    # reduction (tail bit 1 clear); the fix-up of the borrowed rows is the only launch after the backward kernel
    assert lv.n_extra > 0
    R = ops.AttnRoute
    assert routes == [R(1, 0, 0, 0, 0, 256, 53760, 0), R(3, 1, 0, 0, 0, 256, 72192, 1)], routes
    return b, lv, r, counts, qkv, dout


@pytest.mark.parametrize("C,H,slot", ge.PATCH_CASES)
def test_plain_patch_attention_edges_fwd_bwd(C, H, slot):
    assert ge.PATCH_CASES == [(64, 2, 0), (96, 4, 0), (64, 4, 0), (64, 2, 1), (64, 2, 2), (64, 2, 3)]
    b, lv, r, counts, qkv, dout = _plain_run(C, H, slot)
    qd = qkv.double().requires_grad_(True)
    oref = pu.patch_attention(qd, ge._oracle_level(r), slot, H)
    oref.backward(dout.double())
    rec, fails = {}, []
    fails.append(ge._per_cloud(rec, "fwd", b["att"][1], oref, counts, FWD_TOL))
    fails.append(ge._per_cloud(rec, "dqkv", b["dqkv"][1], qd.grad, counts, DQKV_TOL))
    for part, cols in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):   # (recorded only)
        e, scale = ge._err(b["dqkv"][1][:, cols], qd.grad[:, cols])
        rec[part] = e / scale
    print(f"    C {C} H {H} slot {slot}: fwd {rec['fwd']:.3e} (bar {FWD_TOL:.0e})  dqkv {rec['dqkv']:.3e} (bar {DQKV_TOL:.0e})  "
          f"dq {rec['dq']:.3e} dk {rec['dk']:.3e} dv {rec['dv']:.3e}")
    lse = b["lse"][1]
    assert torch.isfinite(lse).all()
    b2, *_ = _plain_run(C, H, slot)
    for k in ("att", "lse", "dqkv", "extra"):
        assert torch.equal(b[k][0], b2[k][0]), f"{k}: a second run differs (no atomics, fixed order: must be bit-equal)"
    ledger.record(TAG + f"C{C}_H{H}_slot{slot}", **rec)
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)


def test_plain_patch_attention_edges_dropout():
    """test_gpu_edge_layouts.test_patch_attention_edges_dropout with qn = kn = None, its four checks and its tolerances: E[sum_k
    P~] = 1, the mask replays, the adjoint identity in V, a central difference in q / k."""
    ops = ge._ops()
    pc, counts, txt, ref, got = ge._levels("patch", "", 1)
    lv = got[0]
    C, H, p_drop, seed = 64, 2, 0.25, 99
    n, d = lv.n, C // H
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(n, 3 * C, generator=g).cuda()

    def fwd(t):
        b = dict(att=ge._guarded(n, C), lse=ge._guarded(lv.npad, H))
        ops.attention_fwd(t, 3 * C, 0, t, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.n_self_tiles,
                          None, None, b["att"][1], b["lse"][1], H, d, p_drop, seed)
        ge._guards_intact(**b)
        return b["att"][1], b["lse"][1]

    ones = qkv.clone()
    ones[:, 2 * C:] = 1.0
    att1, _ = fwd(ones)
    assert abs(att1.mean().item() - 1.0) < 0.02 and att1.std().item() > 0.01
    att, lse = fwd(qkv)
    att_b, _ = fwd(qkv)
    assert torch.equal(att, att_b)
    dout = torch.randn(n, C, generator=g).cuda()
    b = dict(dqkv=ge._guarded(n, 3 * C), extra=ge._guarded(max(lv.n_extra, 1), 2 * C))
    dqkv = b["dqkv"][1]
    gr = ops.attention_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.self_blocks,
                           lv.n_self_tiles, None, None, att, dout, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, 0, H, d, p_drop,
                           seed, lv.kext, lv.ext_pos, lv.n_extra, b["extra"][1])
    ge._guards_intact(**b)
    assert gr == [None] * 4
    u = torch.randn(n, 3 * C, generator=g).cuda()
    uv = torch.zeros_like(u)
    uv[:, 2 * C:] = u[:, 2 * C:]
    lhs = ((fwd(qkv + uv)[0] - att) * dout).double().sum().item()
    rhs = (dqkv * uv).double().sum().item()
    uq = torch.zeros_like(u)
    uq[:, :2 * C] = u[:, :2 * C]
    eps = 1e-2
    num = (((fwd(qkv + eps * uq)[0] - fwd(qkv - eps * uq)[0]) / (2 * eps)) * dout).double().sum().item()
    ana = (dqkv * uq).double().sum().item()
    ledger.record(TAG + "dropout_0.25", v_adjoint_rel=abs(lhs - rhs) / max(1.0, abs(rhs)),
                  central_difference_rel=abs(num - ana) / max(1.0, abs(ana)))
    print(f"    adjoint {lhs:.6f} / {rhs:.6f}   central difference {num:.6f} / {ana:.6f}")
    assert abs(lhs - rhs) <= 2e-4 * max(1.0, abs(rhs)), (lhs, rhs)
    assert abs(num - ana) <= 3e-2 * max(1.0, abs(ana)), (num, ana)


XQ_CASES = [(64, 2, 0), (96, 4, 0), (64, 4, 0)]   # the three head widths the query-per-lane kernels exist for


def _xq_results():
    out = {}
    for C, H, slot in XQ_CASES:
        b, *_ = _plain_run(C, H, slot)
        for k in ("att", "lse", "dqkv"):
            out[f"{k}_{C}_{H}"] = b[k][1].cpu()
    return out


def test_plain_attention_stays_on_the_tile_kernels_under_xq2(tmp_path):
    """LOTUS_XQ=2 moves the fp32 patch attention WITH the norm to the query-per-lane kernels, which have no variant without
    it: a no-norm call must stay on the tile kernels, so a fresh interpreter under LOTUS_XQ=2 reproduces this process's
    forward and backward bit for bit."""
    assert os.environ.get("LOTUS_XQ") in (None, "", "0", "1"), "run from a process with the default kernel selection"
    path = str(tmp_path / "default_process.pt")
    torch.save(_xq_results(), path)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, LOTUS_XQ="2"), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "bit-identical under LOTUS_XQ=2: 9 tensors" in r.stdout, r.stdout[-500:]


def _child_main(path):
    assert os.environ.get("LOTUS_XQ") == "2"
    want = torch.load(path)
    got = _xq_results()
    assert sorted(want) == sorted(got)
    bad = [k for k in want if not torch.equal(want[k], got[k])]
    if bad:
        print("differs from the default process:", bad)
        return 1
    print(f"bit-identical under LOTUS_XQ=2: {len(want)} tensors")
    return 0


# ------------------------------------------------------------------------------------------------ models against the fixtures
@pytest.mark.parametrize("case", list(pu.CASES))
def test_plain_adanorm_fixture_parity(case):
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm
    from weights_util import seeded_state_dict

    fx = pu.load(case)
    cfg = pu.case_config(case)
    assert cfg.ptv3_config.qk_norm is False
    train = bool(fx["meta_train"])
    batch = pu.case_batch(case)
    assert abs(batch["pc_fts"].double().sum().item() - float(fx["input_checksum"])) < 1e-9
    assert np.array_equal(batch["gt_actions"].numpy(), fx["gt_actions"])
    m = SimplePolicyPTV3AdaNorm(cfg)
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
        assert final.dtype == {"float32": torch.float32, "float64": torch.float64}[str(ref.dtype)]
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


def test_shipped_yaml_trains_as_it_is():
    """load_model_config(None) — qk_norm False, dropouts 0.1, DropPath 0.1, depths [2, 2, 2, 6, 2], 6 input channels — in train
    mode: one forward + backward, finite loss and gradients, a gradient for every parameter, and the same step seed again
    gives the same bits."""
    from robot_3dlotus_amd import config as lcfg
    from robot_3dlotus_amd.policy import MODEL_FACTORY

    cfg = lcfg.load_model_config(None)
    batch = _dev(pu.case_batch("plain_adanorm_yaml_train"))

    def step():
        torch.manual_seed(5)
        m = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
        assert m.ptv3_model.qk_norm is False and len(m.state_dict()) == 661
        acts, losses = m(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        torch.cuda.synchronize()
        named = list(m.named_parameters())
        assert len(named) == 622
        for n, p in named:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert acts is None and all(torch.isfinite(v).all() for v in losses.values())
        return [losses[k].detach().clone() for k in ("pos", "rot", "open", "total")] + [p.grad.clone() for _, p in named]

    a, b = step(), step()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    # dropouts and DropPath are on: without them the loss is another one
    torch.manual_seed(5)
    m = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
    m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
    m.act_proj_head.dropout = 0.0
    _, l0 = m(batch, compute_loss=True, compute_final_action=False)
    assert not torch.equal(l0["total"], a[3])


if __name__ == "__main__":
    sys.exit(_child_main(sys.argv[1]))
