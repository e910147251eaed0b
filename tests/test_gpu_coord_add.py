"""GPU checks of the coordinate term of the patch attention (csrc/coord_attn.hip: lotus_coord_add_fwd / _wgrad).

The rows of tests/coordattn_util.ROWS — each names the branch of the launch plan it lands in, which is compared with the plan the
library reports — through the raw C-ABI on guarded caller-owned buffers and a workspace of exactly the queried size, against the
float64 restatements of tests/coordattn_util.py at the project's per-kernel bar, 2e-5 x max(1, |ref|max).  Forward runs in
place: the columns it may not touch (the v third of [q | k | v]) and the guard rows are compared bit for bit with what was there.
The weight gradient runs twice (no atomics, fixed order: bit-equal), into a dP poisoned beforehand (written, not accumulated)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import coordattn_util as cu  # noqa: E402
import ledger  # noqa: E402
import test_gpu_edge_layouts as ge  # noqa: E402  (helpers only: guarded buffers, error bars)

TAG = "coord_add/"
TOL = cu.KERNEL_TOL


def _run(row, y, buf, P, dy):
    from robot_3dlotus_amd import _capi

    ld, W = cu.dims(row)
    n, Cw = row.n, row.Cw
    nws = _capi.query("lotus_coord_add_workspace", n, W, Cw)
    assert nws % 8 == 0
    b = dict(y=ge._guarded(n, ld), dP=ge._guarded(Cw, 3), ws=ge._guarded(nws // 4))
    b["y"][1].copy_(y)
    coord = buf[:, :3]                               # (a view: row stride coord_ld)
    assert coord.stride(0) == row.coord_ld
    _capi.call("lotus_coord_add_fwd", b["y"][1], ld, W, Cw, coord, row.coord_ld, P, n)
    _capi.call("lotus_coord_add_wgrad", dy, ld, W, Cw, coord, row.coord_ld, n, b["dP"][1], b["ws"][1], nws)
    ge._guards_intact(**b)
    return b


@pytest.mark.parametrize("row", cu.ROWS, ids=[r.id for r in cu.ROWS])
def test_coord_add_rows(row):
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi

    ld, W = cu.dims(row)
    plan = np.zeros(6, np.int32)
    _capi.call_raw("lotus_coord_add_plan", row.n, W, row.Cw, int(plan.ctypes.data))
    assert plan.tolist() == cu.plan(row.n, W, row.Cw)
    assert (int(plan[1]), int(plan[2]), cu.chunks_per_thread(row.n, W, row.Cw)) == row.branch
    y, buf, P, dy = cu.row_inputs(row)
    dev = [torch.from_numpy(t).cuda() for t in (y, buf, P, dy)]
    b = _run(row, *dev)
    b2 = _run(row, *dev)
    for k in ("y", "dP"):
        assert torch.equal(b[k][0], b2[k][0]), f"{k}: a second run differs (no atomics, fixed order: must be bit-equal)"
    coord = buf[:, :3]
    y_ref = cu.coord_add_fwd(y, W, row.Cw, coord, P)
    dP_ref = cu.coord_add_wgrad(dy, W, row.Cw, coord)
    rec, fails = {}, []
    got = b["y"][1]
    fails.append(ge._bar(rec, "fwd", got[:, :W], torch.from_numpy(y_ref[:, :W]), TOL))
    fails.append(ge._bar(rec, "dP", b["dP"][1], torch.from_numpy(dP_ref), TOL))
    print(f"    {row.id}: fwd {rec['fwd']:.3e}  dP {rec['dP']:.3e}  (bar {TOL:.0e})   plan {plan.tolist()}   [{row.why}]")
    if ld > W:   # the v columns: never read, never written
        assert torch.equal(got[:, W:], dev[0][:, W:]), "columns past W of y were written"
    assert torch.equal(dev[1], torch.from_numpy(buf).cuda()) and torch.equal(dev[3], torch.from_numpy(dy).cuda())
    if row.coords == "zero":
        assert torch.equal(got, dev[0]), "zero coordinates: y must come back bit for bit"
        assert not b["dP"][1].any(), "zero coordinates: dP must be an exact 0"
    rec["why"], rec["plan"] = row.why, plan.tolist()
    ledger.record(TAG + row.id, **rec)
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", ["qk", "qkv"])
def test_ops_wrappers_on_a_pc_fts_view(mode):
    """ops.coord_add_fwd / coord_add_wgrad (what the attention node calls) with the coordinates as the [:, :3] view of a
    7-column pc_fts, against the float64 restatement of the mode's attention input and its adjoint."""
    from robot_3dlotus_amd import ops

    n, C = 1000, 64
    g = torch.Generator().manual_seed(11)
    pc = torch.randn(n, 7, generator=g).cuda()
    x, w, bq = torch.randn(n, C, generator=g).cuda(), (torch.randn(3 * C, C, generator=g) * 0.1).cuda(), torch.randn(3 * C, generator=g).cuda()
    P = (torch.randn(C, 3, generator=g) * 0.5).cuda()
    dqkv = torch.randn(n, 3 * C, generator=g).cuda()
    coord = pc[:, :3]
    ref = cu.attn_input(mode, *(t.cpu().numpy() for t in (x, coord, P, w, bq)))
    with ops.precision("fp32"):
        if mode == "qkv":
            nrm = x.clone()
            ops.coord_add_fwd(nrm, C, C, coord, P)
            qkv, _ = ops.linear_fwd(nrm, w, bq)
            dn = ops.linear_dgrad(dqkv, w)
            dP = ops.coord_add_wgrad(dn, C, C, coord)
            dP_ref = cu.coord_add_wgrad(dqkv.double().cpu().numpy() @ w.double().cpu().numpy(), C, C, coord.cpu().numpy())
        else:
            qkv, _ = ops.linear_fwd(x, w, bq)
            ops.coord_add_fwd(qkv, 2 * C, C, coord, P)
            dP = ops.coord_add_wgrad(dqkv, 2 * C, C, coord)
            dP_ref = cu.coord_add_wgrad(dqkv.cpu().numpy(), 2 * C, C, coord.cpu().numpy())
    rec, fails = {}, []
    fails.append(ge._bar(rec, "qkv", qkv, torch.from_numpy(ref), TOL))
    fails.append(ge._bar(rec, "dP", dP, torch.from_numpy(dP_ref), TOL))
    print("    " + "  ".join(f"{k} {v:.3e}" for k, v in rec.items()))
    ledger.record(TAG + "ops_" + mode, **rec)
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)
