"""GPU checks of the context tap sums of the Concat stem (csrc/ctx_stem.hip: lotus_ctx_taps_fwd / _bwd).

The rows of tests/concat_util.ROWS — each names the branch it enters — through the raw C-ABI into guarded caller-owned buffers and
a workspace of exactly the queried size, twice (no atomics, fixed order: bit-equal), against the float64 restatement of
tests/concat_util.py (pinned to the dense convolution and to the reference's stem by tests/test_concat_host.py) at the project's
per-kernel bar, 2e-5 x max(1, |ref|max).  The 'cube' / 'isolated' / 'dups' rows read the device front end's own neighbour table.
Cross-check: ops through concat.CtxStemFn against ops.StemFn on the materialised [pc | repeat(ctx)] at a width the existing
convolution kernels take, at the same bar."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import concat_util as cu  # noqa: E402
import ledger  # noqa: E402
import test_gpu_edge_layouts as ge  # noqa: E402  (helpers only: guarded buffers, error bars)

TAG = "ctx_stem/"
TOL = cu.KERNEL_TOL


@functools.lru_cache(maxsize=None)
def _scene_level(name):
    """Scene -> (pc_fts, counts, host table, FrontEnd level 0); the device table is the oracle's, bit for bit."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    pc, counts, nbr = cu.scene_table(name)
    # (two levels: the duplicate count of level 0 comes with the pooling of level 1)
    lvl = FrontEnd(2).build(pc.cuda(), counts, [1] * len(counts), [[0, 1, 2, 3]] * 2)[0]
    assert lvl.n == sum(counts) and list(lvl.counts) == list(counts) and (lvl.n_dup > 0) == (name == "dups")
    assert np.array_equal(lvl.nbr125.cpu().numpy(), nbr), "the front end's table is not the oracle's"
    return pc, counts, nbr, lvl


def _run(row, counts, nbr_dev, P, add, dy):
    from robot_3dlotus_amd import _capi

    B, n, T, C = len(counts), sum(counts), row.T, row.C
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
    nws = _capi.query("lotus_ctx_taps_workspace", B, T, C)
    assert nws % 4 == 0
    b = dict(y=ge._guarded(n, C), dP=ge._guarded(B * T, C), ws=ge._guarded(nws // 4))
    _capi.call("lotus_ctx_taps_fwd", P, nbr_dev, off, add, b["y"][1], B, n, T, C)
    _capi.call("lotus_ctx_taps_bwd", dy, nbr_dev, off, b["dP"][1], B, n, T, C, b["ws"][1], nws)
    ge._guards_intact(**b)
    return b


@pytest.mark.parametrize("row", cu.ROWS, ids=[r.id for r in cu.ROWS])
def test_ctx_taps_rows(row):
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi

    if row.table == "random":
        counts, nbr = cu.row_table(row)
        nbr_dev = torch.from_numpy(nbr).cuda()
    else:
        _, counts, nbr, lvl = _scene_level(row.table)
        nbr_dev = lvl.nbr125
    B, n = len(counts), sum(counts)
    plan = np.zeros(6, np.int32)
    _capi.call_raw("lotus_ctx_taps_plan", n, B, row.T, row.C, int(plan.ctypes.data))
    assert plan.tolist() == [cu.CT_ROWS, -(-n // cu.CT_ROWS), cu.CT_SPLITS, cu.CT_TILE, cu.CT_BTILE, cu.max_width(row.T)]
    P, add, dy = cu.row_inputs(row, counts)
    dev = [torch.from_numpy(P).cuda(), None if add is None else torch.from_numpy(add).cuda(), torch.from_numpy(dy).cuda()]
    b = _run(row, counts, nbr_dev, *dev)
    b2 = _run(row, counts, nbr_dev, *dev)
    for k in ("y", "dP"):
        assert torch.equal(b[k][0], b2[k][0]), f"{k}: a second run differs (no atomics, fixed order: must be bit-equal)"
    y_ref = torch.from_numpy(cu.taps_fwd(P, nbr, counts, add))
    dP_ref = cu.taps_bwd(dy, nbr, counts)
    rec, fails = {}, []
    fails.append(ge._per_cloud(rec, "fwd", b["y"][1], y_ref, counts, TOL))
    fails.append(ge._bar(rec, "dP", b["dP"][1], torch.from_numpy(dP_ref).reshape(B * row.T, row.C), TOL))
    print(f"    {row.id}: fwd {rec['fwd']:.3e}  dP {rec['dP']:.3e}  (bar {TOL:.0e})   [{row.why}]")
    # a tap that occurs nowhere in a cloud: an exact zero, not a small number
    dP = b["dP"][1].view(B, row.T, row.C).cpu().numpy()
    absent = ~(np.add.reduceat((nbr >= 0).astype(np.int64), np.concatenate([[0], np.cumsum(counts)])[:-1], axis=1) > 0).T  # [B][T]
    assert absent.shape == (B, row.T)
    assert not dP[absent].any(), "dP of a tap that is absent from its cloud is not exactly 0"
    if row.table == "random":
        assert all(absent[bi, cu.absent_tap(bi, row.T)] for bi in range(B) if cu.absent_tap(bi, row.T) is not None)
    if row.table in ("random", "isolated") and row.T > 1:
        assert absent.any()
    rec["why"] = row.why
    ledger.record(TAG + row.id, **rec)
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cout,c_pc,Cc", [(32, 6, 16), (64, 8, 24)])
def test_ctx_stem_equals_the_convolution_of_the_concatenation(cout, c_pc, Cc):
    """concat.CtxStemFn (thin convolution + tap sums + BatchNorm + GELU) against ops.StemFn on the materialised [N, c_pc + Cc]
    input through the existing convolution kernels: pre-norm output, output, and the gradients of the stem weight, the norm's
    affine and the context vectors (there: the per-cloud sums of the input gradient's context columns)."""
    from robot_3dlotus_amd import concat, ops

    pc, counts, nbr, lvl = _scene_level("cube")
    B, n = len(counts), sum(counts)
    g = torch.Generator().manual_seed(cout + Cc)
    W0 = (torch.randn(cout, 5, 5, 5, c_pc + Cc, generator=g) * 0.05).cuda()
    c0 = torch.randn(B, Cc, generator=g).cuda()
    gam, bet = (torch.rand(cout, generator=g) + 0.5).cuda(), (torch.randn(cout, generator=g) * 0.2).cuda()
    dout = torch.randn(n, cout, generator=g).cuda()
    x_pc = torch.cat([pc, pc[:, 3:4] * 0.5], 1)[:, :c_pc].contiguous().cuda()   # (the scene has 7 columns)
    rep = torch.repeat_interleave(torch.arange(B), torch.tensor(counts)).cuda()

    def stats():
        return torch.zeros(cout, device="cuda"), torch.ones(cout, device="cuda")

    with ops.precision("fp32"):
        W, cv, ga, be = (t.clone().requires_grad_(True) for t in (W0, c0, gam, bet))
        w_pc, w_ctx = concat.split_stem_weight(W, c_pc)
        pre = concat.ctx_stem_pre(x_pc, cv.detach(), w_pc.detach(), w_ctx.detach(), lvl)
        y = concat.CtxStemFn.apply(x_pc, cv, w_pc, w_ctx, ga, be, *stats(), lvl, True)
        y.backward(dout)
        W2, ga2, be2 = (t.clone().requires_grad_(True) for t in (W0, gam, bet))
        xcat = torch.cat([x_pc, c0[rep]], 1).contiguous().requires_grad_(True)
        pre_ref = ops.conv_fwd(xcat.detach(), W2.detach(), None, lvl.nbr125, lvl.order[0])
        y_ref = ops.StemFn.apply(xcat, W2, ga2, be2, *stats(), lvl, True)
        y_ref.backward(dout)
    torch.cuda.synchronize()
    dctx_ref = torch.zeros(B, Cc, dtype=torch.float64, device="cuda").index_add_(0, rep, xcat.grad[:, c_pc:].double())
    rec, fails = {}, []
    for name, a, r in (("pre", pre, pre_ref), ("y", y, y_ref), ("dW_pc", W.grad[..., :c_pc], W2.grad[..., :c_pc]),
                       ("dW_ctx", W.grad[..., c_pc:], W2.grad[..., c_pc:]), ("dgamma", ga.grad, ga2.grad),
                       ("dbeta", be.grad, be2.grad), ("dctx", cv.grad, dctx_ref)):
        fails.append(ge._bar(rec, name, a, r, TOL))
    # ... and the pre-norm output against the float64 dense convolution of the concatenation
    Wn = W0.double().cpu().numpy().reshape(cout, 125, c_pc + Cc)
    dense = cu.dense_conv(Wn, xcat.detach().double().cpu().numpy(), nbr)
    fails.append(ge._bar(rec, "pre_vs_fp64", pre, torch.from_numpy(dense), TOL))
    print("    " + "  ".join(f"{k} {v:.3e}" for k, v in rec.items()))
    ledger.record(TAG + f"cross_check_cout{cout}_cpc{c_pc}_cc{Cc}", **rec)
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)
