"""The infrastructure of tests/test_gpu_nodes.py on the CPU: the rows are what they say (node_rows.self_check), every restatement
of tests/node_ref.py with dropout off is the plain torch.nn composition (float64, under autograd, to 1e-10), every row's float32
floor is finite and small, and every row can tell the faults this work is after: each deliberate change (node_rows.FAULTS) moves
at least one compared quantity by more than 100 x that quantity's bar."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import node_ref as nr
import node_rows as rows

TIGHT = 1e-10


def test_rows_are_what_they_say():
    assert rows.self_check() == len(rows.ROWS)


# ------------------------------------------------------------------------------------------------ restatements against torch.nn
def _off(rid):
    """The row with every dropout off."""
    r = rows.ROW[rid]
    return r._replace(opts=dict(r.opts, **{k: 0.0 for k in ("p", "attn_p", "dpath") if k in r.opts}))


def _mod(m, **tensors):
    """A torch.nn module in float64 with its parameters / buffers set -> the module."""
    m = m.double()
    with torch.no_grad():
        for k, t in tensors.items():
            getattr(m, k).copy_(t.double())
    return m


def _against(res, outs, ups, grads, extras=()):
    """Backward through the torch.nn composition, then every quantity against the restatement's."""
    torch.autograd.backward(list(outs.values()), ups)
    worst = 0.0
    for k, t in outs.items():
        worst = max(worst, float((t.detach() - res[k]).abs().max()))
    for k, t in grads.items():
        worst = max(worst, float((t.grad - res["d_" + k]).abs().max()))
    for k, t in extras:
        worst = max(worst, float((t.detach() - res[k]).abs().max()))
    assert worst <= TIGHT, worst


def _ln(g, b, eps=1e-5):
    return _mod(nn.LayerNorm(g.shape[0], eps=eps), weight=g, bias=b)


def _lin(w, b):
    return _mod(nn.Linear(w.shape[1], w.shape[0]), weight=w, bias=b)


def _bnm(g, b, rm, rv, training):
    m = _mod(nn.BatchNorm1d(g.shape[0], eps=1e-3, momentum=0.01), weight=g, bias=b, running_mean=rm, running_var=rv)
    return m.train(training)


def test_ffn_restatement_is_the_torch_mlp():
    r = _off("ffn_65x128")
    I, res = rows.inputs(r.id), rows.evaluate(r)
    x = I["x"].double().requires_grad_(True)
    ln, fc1, fc2 = _ln(I["g"], I["b"]), _lin(I["w1"], I["b1"]), _lin(I["w2"], I["b2"])
    y = x + fc2(F.gelu(fc1(ln(x))))
    _against(res, dict(y=y), [I["up_y"].double()],
             dict(x=x, g=ln.weight, b=ln.bias, w1=fc1.weight, b1=fc1.bias, w2=fc2.weight, b2=fc2.bias))


def _sdpa_tiles(q, k, v, tiles):
    """q [nq][H][d], k / v [nk][H][d]: torch's own attention per tile -> [nq][H d]."""
    outs = []
    for qs, ql, ks, kl in np.asarray(tiles).tolist():
        o = F.scaled_dot_product_attention(q[qs:qs + ql].transpose(0, 1)[None], k[ks:ks + kl].transpose(0, 1)[None], v[ks:ks + kl].transpose(0, 1)[None])
        outs.append(o[0].transpose(0, 1).reshape(ql, -1))
    return torch.cat(outs, 0)


@pytest.mark.parametrize("rid", ["self_patch_96_4", "self_patch_64_2_qkFalse"])
def test_selfattn_restatement_is_torch_attention_per_patch(rid):
    r = _off(rid)
    (C, H), I, res = r.shape, rows.inputs(r.id), rows.evaluate(r)
    d = C // H
    tabs = nr.self_tables(rows.tables(r.layout)["levels"][0])
    x = I["x"].double().requires_grad_(True)
    ln, qkv, proj = _ln(I["g"], I["b"]), _lin(I["wqkv"], I["bqkv"]), _lin(I["wp"], I["bp"])
    grads = dict(x=x, g=ln.weight, b=ln.bias, wqkv=qkv.weight, bqkv=qkv.bias, wp=proj.weight, bp=proj.bias)
    t = qkv(ln(x))[torch.as_tensor(tabs["gidx"], dtype=torch.long)].reshape(-1, 3, H, d)
    q, k, v = t.unbind(1)
    if r.opts["qk"]:
        qn, kn = _ln(I["qnw"], I["qnb"], 1e-6), _ln(I["knw"], I["knb"], 1e-6)
        q, k = qn(q), kn(k)
        grads.update(qnw=qn.weight, qnb=qn.bias, knw=kn.weight, knb=kn.bias)
    att = _sdpa_tiles(q, k, v, tabs["tiles"])[torch.as_tensor(tabs["owner_pos"], dtype=torch.long)]
    _against(res, dict(y=x + proj(att)), [I["up_y"].double()], grads)


@pytest.mark.parametrize("rid", ["cross_long_64_2", "crosskv_full_256_8"])
def test_crossattn_restatement_is_torch_attention_per_cloud(rid):
    r = _off(rid)
    (C, H), I, res = r.shape, rows.inputs(r.id), rows.evaluate(r)
    d = C // H
    tb = rows.tables(r.layout)
    x, ctx = I["x"].double().requires_grad_(True), I["ctx"].double().requires_grad_(True)
    ln, ql, kvl, proj = _ln(I["g"], I["b"]), _lin(I["wq"], I["bq"]), _lin(I["wkv"], I["bkv"]), _lin(I["wp"], I["bp"])
    qn, kn = _ln(I["qnw"], I["qnb"], 1e-6), _ln(I["knw"], I["knb"], 1e-6)
    kv = kvl(ctx)
    kv.retain_grad()
    kvh = kv.view(-1, 2, H, d)
    off, coff = np.concatenate([[0], np.cumsum(tb["counts"])]), np.concatenate([[0], np.cumsum(tb["txt"])])
    clouds = [(off[i], tb["counts"][i], coff[i], tb["txt"][i]) for i in range(len(tb["counts"]))]   # whole clouds, not 128-row tiles
    att = _sdpa_tiles(qn(ql(ln(x)).view(-1, H, d)), kn(kvh[:, 0]), kvh[:, 1], clouds)
    _against(res, dict(y=x + proj(att)), [I["up_y"].double()],
             dict(x=x, ctx=ctx, g=ln.weight, b=ln.bias, wq=ql.weight, bq=ql.bias, wkv=kvl.weight, bkv=kvl.bias, qnw=qn.weight, qnb=qn.bias,
                  knw=kn.weight, knb=kn.bias, wp=proj.weight, bp=proj.bias))
    if r.node == "crosskv":
        assert float((kv.grad - res["dkv"]).abs().max()) <= TIGHT
        assert not res["d_wkv0"].any() and not res["d_bkv0"].any()


def _dense_conv(x, grid, w):
    """The submanifold convolution of a FULL box as torch's dense conv3d: x [n][cin] at integer `grid` [n][3] covering a box
    exactly once, w [cout][k][k][k][cin] -> [n][cout] (zero padding = the taps that leave the box have no neighbour)."""
    ext = grid.max(0) + 1
    assert len(grid) == int(np.prod(ext))
    k = w.shape[1]
    g = torch.as_tensor(grid, dtype=torch.long)
    vol = x.new_zeros(*ext.tolist(), x.shape[1]).index_put((g[:, 0], g[:, 1], g[:, 2]), x).permute(3, 0, 1, 2)
    out = F.conv3d(vol[None], w.permute(0, 4, 1, 2, 3), padding=k // 2)[0]
    return out[:, g[:, 0], g[:, 1], g[:, 2]].t()


def test_cpe_restatement_is_dense_conv_linear_layernorm_on_the_solid_block():
    r = rows.ROW["cpe_solid_128_skip"]
    I, res = rows.inputs(r.id), rows.evaluate(r)
    grid = rows.tables(r.layout)["levels"][0]["grid"]
    x, xs = I["x"].double().requires_grad_(True), I["xs"].double().requires_grad_(True)
    cw, cb = I["cw"].double().requires_grad_(True), I["cb"].double().requires_grad_(True)
    lin, ln = _lin(I["lw"], I["lb"]), _ln(I["g"], I["b"])
    y = x + ln(lin(_dense_conv(xs, grid, cw) + cb))
    _against(res, dict(y=y), [I["up_y"].double()], dict(x=x, xs=xs, cw=cw, cb=cb, lw=lin.weight, lb=lin.bias, g=ln.weight, b=ln.bias))


@pytest.mark.parametrize("training", [True, False])
def test_stem_restatement_is_dense_conv_batchnorm_gelu(training):
    r = rows.ROW[f"stem_solid_xgrad_{'train' if training else 'eval'}"]
    I, res = rows.inputs(r.id), rows.evaluate(r)
    grid = rows.tables(r.layout)["levels"][0]["grid"]
    x, cw = I["x"].double().requires_grad_(True), I["cw"].double().requires_grad_(True)
    bn = _bnm(I["g"], I["b"], I["rmean"], I["rvar"], training)
    y = F.gelu(bn(_dense_conv(x, grid, cw)))
    _against(res, dict(y=y), [I["up_y"].double()], dict(x=x, cw=cw, g=bn.weight, b=bn.bias), [("rmean", bn.running_mean), ("rvar", bn.running_var)])
    assert training or (torch.equal(res["rmean"], I["rmean"].double()) and torch.equal(res["rvar"], I["rvar"].double()))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("scene", ["all_eight", "100_clouds_of_3"])
def test_pool_and_unpool_restatements_are_torch_modules(scene, training):
    tag = "train" if training else "eval"
    r = rows.ROW[f"pool_{scene}_64_128_{tag}"]
    I, res = rows.inputs(r.id), rows.evaluate(r)
    lv = rows.tables(r.layout)["levels"][1]
    cl, nc = torch.from_numpy(lv["cluster"]).long(), lv["grid"].shape[0]
    x = I["x"].double().requires_grad_(True)
    lin, bn = _lin(I["w"], I["bias"]), _bnm(I["g"], I["b"], I["rmean"], I["rvar"], training)
    proj = lin(x)
    pooled = torch.stack([proj[cl == c].max(0)[0] for c in range(nc)], 0)   # torch.max per cell: gradient to the arg-max row
    _against(res, dict(y=F.gelu(bn(pooled))), [I["up_y"].double()], dict(x=x, w=lin.weight, bias=lin.bias, g=bn.weight, b=bn.bias),
             [("rmean", bn.running_mean), ("rvar", bn.running_var)])
    r = rows.ROW[f"unpool_{scene}_128_64_{tag}"]
    I, res = rows.inputs(r.id), rows.evaluate(r)
    xc, xp = I["xc"].double().requires_grad_(True), I["xp"].double().requires_grad_(True)
    lu_, ls_ = _lin(I["wu"], I["bu"]), _lin(I["ws"], I["bs"])
    bu, bs = _bnm(I["gu"], I["betau"], I["rmu"], I["rvu"], training), _bnm(I["gs"], I["betas"], I["rms"], I["rvs"], training)
    up, skip = F.gelu(bu(lu_(xc))), F.gelu(bs(ls_(xp)))
    _against(res, dict(y=skip + up[cl], skip=skip), [I["up_y"].double(), I["up_skip"].double()],
             dict(xc=xc, xp=xp, wu=lu_.weight, bu=lu_.bias, gu=bu.weight, betau=bu.bias, ws=ls_.weight, bs=ls_.bias, gs=bs.weight, betas=bs.bias),
             [("rmu", bu.running_mean), ("rvu", bu.running_var), ("rms", bs.running_mean), ("rvs", bs.running_var)])


def test_chain_restatement_without_dropout_is_the_oracle_block_pair():
    """The composition against oracle.model.Oracle.block / ca_block (the restatement the model fixtures are pinned with)."""
    from oracle import model as om
    r = _off("chain_long_64_2")
    (C, H), I, res = r.shape, rows.inputs(r.id), rows.evaluate(r)
    tb = rows.tables(r.layout)
    lv = dict(tb["levels"][0])
    for k in ("order", "inverse"):
        lv[k + "_t"] = torch.from_numpy(lv[k]).long()
    lv["pad_t"], lv["unpad_t"], lv["nbr27_t"] = (torch.from_numpy(np.ascontiguousarray(lv[k])).long() for k in ("pad", "unpad", "nbr27"))
    sd = {k: t.double().requires_grad_(True) for k, t in I.items() if k[:4] in ("blk.", "cab.")}
    x, ctx = I["x"].double().requires_grad_(True), I["ctx"].double().requires_grad_(True)
    o = om.Oracle(sd, None, training=True, dtype=torch.float64)
    y = o.ca_block(o.block(x, x, lv, "blk", H, 128, 0), lv, ctx, list(tb["txt"]), "cab", H)
    _against(res, dict(y=y), [I["up_y"].double()], dict(x=x, ctx=ctx, **sd))


# ------------------------------------------------------------------------------------------------ floors and discriminating power
@pytest.mark.parametrize("rid", [r.id for r in rows.ROWS])
def test_float32_floor_of_every_row(rid):
    """The floor every bar is stated from: finite, and far below the faults the rows are there to tell (a restatement that is
    ill-conditioned in float32 at a row's shape would show here, before any GPU is involved)."""
    fl = rows.floor(rid)
    print(rid, {k: f"{v:.2e}" for k, v in fl.items()})
    ref = rows.reference(rid)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    # (1e-3: the gradients that are mathematically zero — a bias in front of a BatchNorm, k_norm.bias — are pure cancellation noise
    # of up to 1e-4 at these shapes; everything else is below 5e-6)
    assert all(np.isfinite(v) and v < 1e-3 for v in fl.values()), fl
    assert all(rows.KERNEL_TOL <= b <= 16 * max(rows.KERNEL_TOL, f) for b, f in zip(rows.bars(rid).values(), fl.values()))


C_BLIND = "plain_scale"  # see test_every_row_tells_the_faults


@pytest.mark.parametrize("rid", [r.id for r in rows.ROWS if rows.faults_of(r)])
def test_every_row_tells_the_faults(rid):
    """Each deliberate change moves at least one compared quantity by more than 100 x that quantity's bar.  The keep scale
    1 / (1 - p) against the quantised 1 / (1 - 6553 / 65536) differs by 1.0e-5 relative at p = 0.1: it moves every quantity by about
    half the per-kernel bar of 2e-5 whatever the row, so NO row tells it (the power is printed and recorded, 0.1 .. 1 bar); such
    rows do not count for that fault, and a float32 comparison at this bar cannot be made to.  Every other fault must show."""
    row = rows.ROW[rid]
    for fault in rows.faults_of(row):
        power = rows.fault_power(rid, fault)
        print(rid, fault, f"{power:.3g} bars")
        if fault == C_BLIND and power <= 100:
            continue  # recorded above; the row does not count for this fault
        assert power > 100, (rid, fault, power)
