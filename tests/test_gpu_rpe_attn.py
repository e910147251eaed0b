"""lotus_attention_rpe_fwd / _bwd (csrc/attention_rpe.hip: the patch attention with the relative-position term of
PointTransformerV3/model.py:307-326, :518-527) on the rows of tests/rpe_util.py against float64, into guarded, poisoned
caller-owned buffers: forward, lse, dq / dk / dv, the q/k-norm gradients and the table gradient at the project's bars of the
exact-fp32 tile kernels; with a table of zeros the entry points agree with lotus_attention_fwd / _bwd on the same inputs and seed
(which pins the numbering of the dropout mask); the dropout row's mask is read back through the kernel itself and enters the
float64 reference; a second backward gives the same bits; rows of the table that no pair selects come back as exact zeros."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ledger  # noqa: E402
import rpe_util as ru  # noqa: E402

GUARD = 64
FILL = 12345.0
SENT = -7

ru.self_check()  # the rows' CPU assertions: a row that is not what it says fails the collection


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops
    return ops


def _guarded(rows, cols=None):
    shape = (rows + GUARD,) if cols is None else (rows + GUARD, cols)
    buf = torch.full(shape, FILL, dtype=torch.float32, device="cuda")
    return buf, buf[:rows]


def _guards_intact(bufs):
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        tail = buf[view.shape[0]:]
        assert torch.equal(tail, torch.full_like(tail, FILL)), f"{name}: rows past the end were written"


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0, max(1.0, float(b.abs().max()) if b.numel() else 0.0)


def _bar(rec, name, a, b, tol):
    e, scale = _err(a, b)
    rec[name] = e / scale
    return None if e <= tol * scale else f"{name}: max err {e:.3e} > {tol:.1e} * {scale:.3g}"


def _finish(test, rec, fails):
    ledger.record("rpe_attn/" + test, **rec)
    print("   ", test, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in rec.items()})
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)


class Dev:
    """The device tensors of a row."""

    def __init__(self, row):
        v = ru.row_inputs(row)
        t = v["tabs"]
        i32 = dict(dtype=torch.int32, device="cuda")
        self.row, self.v, self.t = row, v, t
        self.n, self.C, self.H, self.d = sum(row.counts), row.H * row.d, row.H, row.d
        self.qkv, self.dout, self.table = v["qkv"].cuda(), v["dout"].cuda(), v["table"].cuda()
        self.qn = tuple(x.cuda() for x in v["qn"]) if row.norm else None
        self.kn = tuple(x.cuda() for x in v["kn"]) if row.norm else None
        self.grid = torch.as_tensor(v["grid"], **i32)
        self.gidx = torch.as_tensor(v["gidx"], **i32)
        self.owner, self.kext = torch.as_tensor(t["owner"], **i32), torch.as_tensor(t["kext"], **i32)
        self.ext_pos = torch.as_tensor(t["ext_pos"] if t["n_extra"] else np.zeros(1, np.int32), **i32)
        self.tiles, self.blocks = torch.as_tensor(t["tiles"], **i32), torch.as_tensor(t["blocks"], **i32)
        self.ntiles, self.npad, self.n_extra = len(t["tiles"]), t["npad"], t["n_extra"]
        self.seed = 4242 + self.n


def _fwd(ops, D, qkv, table, drop=0.0, rpe=True, routes=None):
    C, H, d = D.C, D.H, D.d
    b = dict(att=_guarded(D.n, C), lse=_guarded(D.npad, H))
    if rpe:
        ops.attention_rpe_fwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.ntiles, D.qn, D.kn,
                              b["att"][1], b["lse"][1], H, d, D.grid, table, D.row.bnd, drop, D.seed)
    else:
        ops.attention_fwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.ntiles, D.qn, D.kn,
                          b["att"][1], b["lse"][1], H, d, drop, D.seed)
    if routes is not None:
        routes.append(ops.last_attn_route())
    _guards_intact(b)
    return b["att"][1], b["lse"][1]


def _bwd(ops, D, qkv, table, att, lse, drop=0.0, rpe=True, routes=None):
    """-> (dqkv, norm gradients, dtable or None)"""
    C, H, d = D.C, D.H, D.d
    b = dict(dqkv=_guarded(D.n, 3 * C), extra=_guarded(max(D.n_extra, 1), 2 * C))
    dqkv = b["dqkv"][1]
    if rpe:
        gr, dtable = ops.attention_rpe_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.blocks, D.ntiles,
                                           D.qn, D.kn, att, D.dout, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, H, d, D.grid,
                                           table, D.row.bnd, drop, D.seed, D.kext, D.ext_pos, D.n_extra, b["extra"][1])
    else:
        gr = ops.attention_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.blocks, D.ntiles, D.qn,
                               D.kn, att, D.dout, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, 0, H, d, drop, D.seed, D.kext,
                               D.ext_pos, D.n_extra, b["extra"][1])
        dtable = None
    if routes is not None:
        routes.append(ops.last_attn_route())
    _guards_intact(b)
    return dqkv, gr, dtable


def _mask(ops, D):
    """The dropout row's keep mask [npad][H][K], read back through the forward kernel: with q = k = 0 and a table of zeros the
    probabilities are uniform, and an indicator column in V returns (1 / K) keep / (1 - p) of one key per head column: K / d
    launches.  Positions that own no output row (borrowed copies as queries) have dout = 0: their mask cannot matter, it is 1."""
    row, C, H, d, K = D.row, D.C, D.H, D.d, D.row.K
    assert K % d == 0
    cu = D.t["cu"]
    local = torch.as_tensor(np.arange(D.npad) - np.repeat(cu[:-1], np.diff(cu)), dtype=torch.long)   # position -> row of its patch
    own = torch.as_tensor(D.t["owner"], dtype=torch.bool)
    gidx = torch.as_tensor(D.v["gidx"], dtype=torch.long)
    pos_of = torch.as_tensor(D.v["owner_pos"], dtype=torch.long)          # output row i <- position
    # a borrowed copy sits at the row its point has in its own patch (position - K), so one V row per point serves both patches
    assert torch.equal(local[~own], local[pos_of][gidx[~own]])
    row_of_point = local[pos_of]
    keep = torch.ones(D.npad, H, K, dtype=torch.float64)
    zero_table = torch.zeros_like(D.table)
    for l in range(K // d):
        vv = torch.zeros(D.n, H, d)
        for c in range(d):
            vv[row_of_point == l * d + c, :, c] = 1.0
        qkv = torch.zeros(D.n, 3 * C)
        qkv[:, 2 * C:] = vv.reshape(D.n, C)
        att, _ = _fwd(ops, D, qkv.cuda(), zero_table, drop=row.drop)
        keep[pos_of, :, l * d:(l + 1) * d] = (att.cpu().double() * K * (1.0 - row.drop)).reshape(D.n, H, d)
    assert bool(((keep - keep.round()).abs() < 1e-4).all()), "the read-back is not a 0 / 1 mask"
    keep = keep.round()
    frac = float(keep[own].mean())
    assert abs(frac - (1.0 - row.drop)) < 0.02, frac
    return keep


@functools.lru_cache(maxsize=None)
def _case(rid):
    """Reference (float64, once per row) and the device run of the row: shared by the tests below, not modified."""
    ops = _ops()
    row = ru.ROW[rid]
    D = Dev(row)
    v = D.v
    keep = _mask(ops, D) if row.drop > 0 else None
    qd = v["qkv"].double().requires_grad_(True)
    td = v["table"].double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (*v["qn"], *v["kn"])] if row.norm else []
    qn, kn = ((pr[0], pr[1]), (pr[2], pr[3])) if row.norm else (None, None)
    oref, lse_ref = ru.attention_ref(qd, v["gidx"], v["owner_pos"], D.t["cu"], v["grid"], td, row.bnd, row.H, qn, kn, keep, row.drop)
    oref.backward(v["dout"].double())
    routes = []
    att, lse = _fwd(ops, D, D.qkv, D.table, row.drop, routes=routes)
    dqkv, gr, dtable = _bwd(ops, D, D.qkv, D.table, att, lse, row.drop, routes=routes)
    return dict(D=D, oref=oref.detach(), lse_ref=lse_ref.detach(), dqkv_ref=qd.grad, dtable_ref=td.grad, norm_ref=[p.grad for p in pr],
                att=att, lse=lse, dqkv=dqkv, gr=gr, dtable=dtable, routes=routes)


@pytest.mark.parametrize("rid", [r.id for r in ru.ROWS])
def test_rows_against_float64(rid):
    ops = _ops()
    c = _case(rid)
    row, D = ru.ROW[rid], c["D"]
    rec, fails = {"why": row.why}, []
    fails.append(_bar(rec, "fwd", c["att"], c["oref"], ru.TOL_FWD))
    fails.append(_bar(rec, "lse", c["lse"], c["lse_ref"], ru.TOL_FWD))
    fails.append(_bar(rec, "dqkv", c["dqkv"], c["dqkv_ref"], ru.TOL_DQKV))
    if row.norm:
        for name, a, b in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), c["gr"], c["norm_ref"]):
            fails.append(_bar(rec, name, a, b, ru.TOL_DKN_B if name == "dkn_b" else ru.TOL_NORM))
    else:
        assert c["gr"] == [None] * 4
    if rid == "k1":  # mathematically zero: the bound is absolute, 1e-6 of max |dout|
        e = float(c["dtable"].abs().max())
        rec["dtable_abs"] = e
        assert float(c["dtable_ref"].abs().max()) < 1e-12
        fails.append(None if e <= 1e-6 * float(D.dout.abs().max()) else f"dtable: |.|max {e:.3e} of a gradient that is zero")
    else:
        fails.append(_bar(rec, "dtable", c["dtable"], c["dtable_ref"], ru.TOL_DTABLE))
        assert float(c["dtable_ref"].abs().max()) > 1e-2, "the row does not exercise the table gradient"
    # rows no pair selects: exact zeros (and the reference agrees that they are not selected)
    untouched = (c["dtable_ref"] == 0).all(1)
    if rid == "near":
        assert int(untouched.sum()) == 3 * (2 * row.bnd + 1 - 5)
    if rid != "k1":
        assert bool((c["dtable"].cpu()[untouched] == 0).all()), "a table row that no pair selects is not an exact zero"
    # the kernels that ran
    R = ops.AttnRoute
    norm = int(row.norm)
    tail = 4 | (2 if row.norm else 0) | (1 if D.n_extra else 0)
    want = [R(ops.ATTN_RPE_FWD, 0, 0, 0, norm, 256, 57216, 0),
            R(ops.ATTN_RPE_BWD, 1, 0, 0, norm, 256, 74112 + 1536 * (2 * row.bnd + 1), tail)]
    assert c["routes"] == want, (c["routes"], want)
    _finish(rid, rec, fails)


@pytest.mark.parametrize("rid", [r.id for r in ru.ROWS])
def test_zero_table_is_the_existing_attention(rid):
    """With a table of zeros the new entry points agree with lotus_attention_fwd / _bwd on the same inputs and seed — on the
    dropout row too, which pins the mask function and its element numbering — and the table gradient is still the sum of G."""
    ops = _ops()
    row = ru.ROW[rid]
    D = _case(rid)["D"]
    zero = torch.zeros_like(D.table)
    att0, lse0 = _fwd(ops, D, D.qkv, None, row.drop, rpe=False)
    dqkv0, gr0, _ = _bwd(ops, D, D.qkv, None, att0, lse0, row.drop, rpe=False)
    att, lse = _fwd(ops, D, D.qkv, zero, row.drop)
    dqkv, gr, dtable = _bwd(ops, D, D.qkv, zero, att, lse, row.drop)
    rec, fails = {}, []
    fails.append(_bar(rec, "fwd", att, att0, ru.TOL_FWD))
    fails.append(_bar(rec, "lse", lse, lse0, ru.TOL_FWD))
    fails.append(_bar(rec, "dqkv", dqkv, dqkv0, ru.TOL_DQKV))
    if row.norm:
        for name, a, b in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), gr, gr0):
            fails.append(_bar(rec, name, a, b, ru.TOL_DKN_B if name == "dkn_b" else ru.TOL_NORM))
    if row.drop > 0:  # the same mask: the kept entries of a row are the same ones (a different mask moves the output by O(1))
        assert float((att - att0).abs().max()) < 1e-4
    assert bool(torch.isfinite(dtable).all())
    _finish("zero_table/" + rid, rec, fails)


@pytest.mark.parametrize("rid", ru.DETERMINISM_ROWS)
def test_second_backward_gives_the_same_bits(rid):
    ops = _ops()
    c = _case(rid)
    D, row = c["D"], ru.ROW[rid]
    dqkv, gr, dtable = _bwd(ops, D, D.qkv, D.table, c["att"], c["lse"], row.drop)
    assert torch.equal(dqkv, c["dqkv"]) and torch.equal(dtable, c["dtable"])
    for a, b in zip(gr, c["gr"]):
        assert (a is None and b is None) or torch.equal(a, b)
    att, lse = _fwd(ops, D, D.qkv, D.table, row.drop)
    assert torch.equal(att, c["att"]) and torch.equal(lse, c["lse"])


def test_no_blocks_writes_a_zero_table_gradient_and_keeps_the_route_record():
    ops = _ops()
    c = _case("k5")
    D = c["D"]
    before = ops.last_attn_route()
    C, H, d = D.C, D.H, D.d
    dq = torch.full((D.n, 3 * C), FILL, device="cuda")
    gr, dtable = ops.attention_rpe_bwd(D.qkv, 3 * C, 0, D.qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.blocks, 0, None,
                                       None, c["att"], D.dout, c["lse"], dq, 3 * C, 0, dq, 3 * C, C, 2 * C, 0, H, d, D.grid, D.table,
                                       D.row.bnd)
    torch.cuda.synchronize()
    assert bool((dtable == 0).all()) and bool((dq == FILL).all()) and ops.last_attn_route() == before
