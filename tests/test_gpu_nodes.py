"""The sub-block autograd nodes of ops.py — FfnFn, SelfAttnFn, CrossAttnFn, CrossAttnKvFn (with ProjAllFn), CpeFn, StemFn, PoolFn,
UnpoolFn, and Block.run + CABlock.run as the five nodes or as PairFn — against their float64 restatements under torch autograd
(tests/node_ref.py), with dropout ON: the masks are numpy tensors computed from (seed, element index), the seed streams are
restated constants.  Every row of tests/node_rows.py runs with the composites on and off (and one row per node under the deferred
weight-gradient join), and each run is compared with float64: the output, d x (d xs, d context, d kv), every parameter gradient in
full, the q/k-norm gradients, the BatchNorm running statistics, the parked hand-over tensor.  All values finite, a second run
gives the same bits, the errors go to the ledger next to the float32 floor and the bar (node_rows: bar = max(2e-5, 4 x floor)).

The integer tables of every layout are compared with the oracle front end's first, and the attention mask of the numpy
restatement is proven once against the mask read back through lotus_attention_fwd."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ledger  # noqa: E402
import node_ref as nr  # noqa: E402
import node_rows as rows  # noqa: E402
from frontend_util import assert_levels_equal  # noqa: E402

GUARD, FILL = 64, 12345.0
MODES = {"launch": (False, "node", False), "comp": (True, "node", False), "comp_end": (True, "end", False), "pair": (True, "node", True)}
CASES = [(r.id, m) for r in rows.ROWS for m in ("launch", "comp")] + [(rid, "comp_end") for rid in rows.END_JOIN_ROWS] + \
        [(r.id, "pair") for r in rows.ROWS if r.node == "chain"]


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _levels(layout, width=None):
    """The FrontEnd levels of a layout, their integer tables compared with the oracle's and with the restated tile lists."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    tb = rows.tables(layout)
    n_levels = layout[2]
    perms = [[0, 1, 2, 3]] * n_levels
    got = FrontEnd(n_levels, conv_widths=[width] * n_levels if width else None).build(tb["pc"].cuda(), tb["counts"], tb["txt"], perms)
    assert_levels_equal(tb["levels"], got, n_levels, ctx_counts=tb["txt"])
    st = nr.self_tables(tb["levels"][0])
    lv = got[0]
    np.testing.assert_array_equal(lv.self_tiles.cpu().numpy()[:lv.n_self_tiles], st["tiles"])
    np.testing.assert_array_equal(lv.gidx.cpu().numpy(), st["gidx"])
    np.testing.assert_array_equal(lv.ca_tiles.cpu().numpy()[:lv.n_ca_tiles], nr.cross_tiles(tb["counts"], tb["txt"]))
    return got


# ------------------------------------------------------------------------------------------------ the nodes on the device
def _run(ops, row, pair):
    """One forward and backward of the row's node -> {quantity: tensor} with the names of node_rows.evaluate."""
    I = rows.inputs(row.id)
    need = set(rows.grad_names(row))
    T = {k: t.cuda().requires_grad_(k in need) for k, t in I.items() if not k.startswith("up_")}
    up = {k[3:]: t.cuda() for k, t in I.items() if k.startswith("up_")}
    node, o = row.node, row.opts
    extra, outs = {}, None
    if node == "ffn":
        h_in, h_out = ops.Handoff(), ops.Handoff()
        h_out.arm(rows.HAND_P, rows.HAND_SEED)
        y = ops.FfnFn.apply(T["x"], T["g"], T["b"], T["w1"], T["b1"], T["w2"], T["b2"], o["p"], rows.SEED, h_in, h_out, o["dpath"])
        extra = dict(dz=lambda: h_out.dz)
    elif node == "self":
        C, H = row.shape
        lvl = _levels(row.layout)[0]
        qk = [T[k] for k in ("qnw", "qnb", "knw", "knb")] if o["qk"] else [None] * 4
        y = ops.SelfAttnFn.apply(T["x"], T["g"], T["b"], T["wqkv"], T["bqkv"], *qk, T["wp"], T["bp"], lvl, H, o["p"], rows.SEED, o["attn_p"],
                                 ops.Handoff(), o["dpath"])
    elif node in ("cross", "crosskv"):
        C, H = row.shape
        lvl = _levels(row.layout)[0]
        h_in, h_out = ops.Handoff(), ops.Handoff()
        h_out.arm(rows.HAND_P, rows.HAND_SEED)
        extra = dict(dz=lambda: h_out.dz)
        norms = [T[k] for k in ("qnw", "qnb", "knw", "knb")]
        if node == "cross":
            y = ops.CrossAttnFn.apply(T["x"], T["ctx"], T["g"], T["b"], T["wq"], T["bq"], T["wkv"], T["bkv"], *norms, T["wp"], T["bp"], lvl, H,
                                      o["p"], rows.SEED, o["attn_p"], h_in, h_out)
        else:
            bank = ops.ProjBank()
            slices = ops.ProjAllFn.apply(T["ctx"], bank, None, T["wkv0"], T["bkv0"], T["wkv"], T["bkv"])
            L, W = bank.slab.shape
            # the bank's gradient slab with GUARD poisoned rows behind it: the consumer writes its column slice of the first L rows
            buf = torch.full((L + GUARD, W), FILL, device="cuda")
            bank.dslab = buf[:L]
            y = ops.CrossAttnKvFn.apply(T["x"], slices[1], T["g"], T["b"], T["wq"], T["bq"], *norms, T["wp"], T["bp"], lvl, H, o["p"], rows.SEED,
                                        o["attn_p"], h_in, h_out, bank, 1)
            extra.update(dkv=lambda: buf[:L, 96:], _guard=lambda: buf[L:], _other=lambda: buf[:L, :96])
    elif node == "cpe":
        lvl = _levels(row.layout, row.shape[0])[0]
        y = ops.CpeFn.apply(T["x"], T["x"] if o["same"] else T["xs"], T["cw"], T["cb"], T["lw"], T["lb"], T["g"], T["b"], lvl, None)
    elif node == "stem":
        lvl = _levels(row.layout)[0]
        y = ops.StemFn.apply(T["x"], T["cw"], T["g"], T["b"], T["rmean"], T["rvar"], lvl, o["training"])
        extra = dict(rmean=lambda: T["rmean"], rvar=lambda: T["rvar"])
    elif node == "pool":
        child = _levels(row.layout)[1]
        y = ops.PoolFn.apply(T["x"], T["w"], T["bias"], T["g"], T["b"], T["rmean"], T["rvar"], child, o["training"])
        extra = dict(rmean=lambda: T["rmean"], rvar=lambda: T["rvar"])
    elif node == "unpool":
        child = _levels(row.layout)[1]
        y, skip = ops.UnpoolFn.apply(T["xc"], T["xp"], T["wu"], T["bu"], T["gu"], T["betau"], T["rmu"], T["rvu"], T["ws"], T["bs"], T["gs"],
                                     T["betas"], T["rms"], T["rvs"], child, o["training"])
        outs = dict(y=y, skip=skip)
        extra = {k: (lambda k=k: T[k]) for k in ("rmu", "rvu", "rms", "rvs")}
    elif node == "chain":
        y, named = _run_chain(ops, row, T, pair)
    outs = outs or dict(y=y)
    torch.autograd.backward(list(outs.values()), [up[k] for k in outs])
    torch.cuda.synchronize()
    res = {k: t.detach().clone() for k, t in outs.items()}
    if node == "chain":
        res.update({"d_" + k: p.grad.clone() for k, p in named.items()})
    else:
        res.update({"d_" + k: T[k].grad.clone() for k in I if k in need})
    res.update({k: f().detach().clone() for k, f in extra.items()})
    return res


def _run_chain(ops, row, T, pair):
    """ptv3.Block.run then CABlock.run on module instances, through the model's own walker (_run_depth: PairFn where the pair is
    on), the CABlock's keys / values slice 1 of a two-consumer bank."""
    from robot_3dlotus_amd import ptv3

    C, H = row.shape
    M = ptv3.PointTransformerV3CA
    blk, cab = ptv3.Block(C, H, 4).cuda(), ptv3.CABlock(C, H, rows.CC, 4).cuda()
    blk.load_state_dict({k[4:]: t.detach() for k, t in T.items() if k.startswith("blk.")})
    cab.load_state_dict({k[4:]: t.detach() for k, t in T.items() if k.startswith("cab.")})
    lvl = _levels(row.layout, C)[0]

    class Walker:
        _run_depth, _pair, _pair_ok = M._run_depth, M._pair, M._pair_ok
        _pair_on, _pair_params, _cab_index = ops.pair_enabled(lvl.n), {}, {id(cab): 1}

    assert Walker._pair_on == pair
    bank = ops.ProjBank()
    ops.ProjAllFn.apply(T["ctx"], bank, None, torch.zeros(96, rows.CC, device="cuda"), torch.zeros(96, device="cuda"), cab.attn.kv.weight,
                        cab.attn.kv.bias)
    fw = SimpleNamespace(p=row.opts["p"], pa=row.opts["attn_p"], packs={blk: ops.conv_weight_t(blk.cpe[0].weight.detach())}, context=T["ctx"],
                         bank=bank)
    y = Walker()._run_depth(fw, SimpleNamespace(block0=blk, ca_block0=cab), 0, T["x"], T["x"], lvl.for_order(0), lvl, rows.SEED, 0.0)
    assert (type(y.grad_fn).__name__ == "PairFnBackward") == pair, type(y.grad_fn).__name__
    named = dict(x=T["x"], ctx=T["ctx"])
    named.update({"blk." + k: p for k, p in blk.named_parameters()})
    named.update({"cab." + k: p for k, p in cab.named_parameters()})
    return y, named


@pytest.mark.parametrize("rid,mode", CASES)
def test_node_against_float64(rid, mode):
    ops = _ops()
    row = rows.ROW[rid]
    comp, join, pair = MODES[mode]
    ref, fl, bar = rows.reference(rid), rows.floor(rid), rows.bars(rid)
    try:
        ops.set_composites(comp)
        ops.set_wgrad_join(join)
        ops.set_pair(pair)
        got = _run(ops, row, pair)
        again = _run(ops, row, pair)
    finally:
        ops.set_composites(True)
        ops.set_wgrad_join("node")
        ops.set_pair("auto")
    if "_guard" in got:
        assert bool((got.pop("_guard") == FILL).all()), "rows past the end of the bank's gradient slab were written"
        assert not got.pop("_other").any(), "the gradient slice of the bank's other consumer is not zero"
        again.pop("_guard"), again.pop("_other")
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    rec, fails = dict(rows=int(ref["y"].shape[0]), why=row.why), []
    for q in ref:
        e = rows.rel_err(got[q], ref[q])
        rec[q], rec[q + "_floor"], rec[q + "_bar"] = e, fl[q], bar[q]
        print(f"{rid} {mode} {q}: err {e:.3e} floor {fl[q]:.3e} bar {bar[q]:.3e}")
        if not bool(torch.isfinite(got[q]).all()):
            fails.append(f"{q} is not finite")
        if not e <= bar[q]:
            fails.append(f"{q}: err {e:.3e} > bar {bar[q]:.3e} (floor {fl[q]:.3e})")
        if not torch.equal(got[q], again[q]):
            fails.append(f"{q}: a second run differs by {float((got[q] - again[q]).abs().max()):.3e}")
    if row.node in ("stem", "pool", "unpool") and not row.opts["training"]:
        I = rows.inputs(rid)
        assert all(torch.equal(got[k].cpu(), I[k]) for k in I if k in rows.NO_GRAD), "eval mode moved the running statistics"
    ledger.record(f"nodes/{rid}/{mode}", **rec)
    assert not fails, "\n".join(fails)


def test_numpy_attention_mask_is_the_kernels():
    """The keep mask of node_ref.attn_keep against the one read back through lotus_attention_fwd, for every tile of the patch
    layout (lengths 1 .. 128, borrowed rows): with q = k = 0 the probabilities of a tile of k_len keys are uniform, and an indicator
    column in V returns keep / (k_len (1 - p)) of one key per head column; 128 / d launches read every key."""
    ops = _ops()
    C, H, p, seed = 64, 2, rows.P, nr.mix_seed(rows.SEED, 1)
    d = C // H
    layout = ("patch", "", 1)
    lv = _levels(layout)[0]
    st = nr.self_tables(rows.tables(layout)["levels"][0])
    tiles, n = st["tiles"], lv.n
    cu = np.concatenate([tiles[:, 0], [tiles[-1, 0] + tiles[-1, 1]]])
    pos = np.arange(lv.npad)
    tile_of = np.searchsorted(cu, pos, side="right") - 1
    local = pos - cu[tile_of]
    own = st["owner_pos"]
    np.testing.assert_array_equal(local, local[own][st["gidx"]])   # a borrowed copy sits at the row its point has in its own tile
    ones, zeros = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    keep = np.zeros((n, H, 128))
    for l in range(128 // d):
        v = torch.zeros(n, H, d)
        for c in range(d):
            v[torch.from_numpy(local[own] == l * d + c), :, c] = 1.0
        qkv = torch.zeros(n, 3 * C)
        qkv[:, 2 * C:] = v.reshape(n, C)
        att = torch.full((n + GUARD, C), FILL, device="cuda")
        lse = torch.empty(lv.npad, H, device="cuda")
        qc = qkv.cuda()
        ops.attention_fwd(qc, 3 * C, 0, qc, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.n_self_tiles, (ones, zeros),
                          (ones, zeros), att[:n], lse, H, d, p, seed)
        torch.cuda.synchronize()
        assert bool((att[n:] == FILL).all())
        klen = tiles[tile_of[own], 3].astype(np.float64)
        keep[:, :, l * d:(l + 1) * d] = att[:n].cpu().double().numpy().reshape(n, H, d) * klen[:, None, None] * (1.0 - float(np.float32(p)))
    assert np.abs(keep - keep.round()).max() < 1e-4, "the read-back is not a 0 / 1 mask"
    keep = keep.round()
    checked = 0
    for t, (_, ql, _, kl) in enumerate(tiles.tolist()):
        want = nr.attn_keep(t, H, ql, kl, seed, p)          # [H][ql][kl]
        mine = np.nonzero(tile_of[own] == t)[0]            # the rows whose query position lies in tile t
        got = keep[mine][:, :, :kl].transpose(1, 0, 2)     # [H][rows][kl]
        np.testing.assert_array_equal(got, want[:, local[own][mine], :], err_msg=f"tile {t} ({ql} x {kl})")
        assert not keep[mine][:, :, kl:].any()
        checked += got.size
    assert checked > 100000 and abs(keep.sum() / checked - (1 - p)) < 0.02
    ledger.record("nodes/attention_mask_proof", elements=int(checked), kept=float(keep.sum() / checked))
