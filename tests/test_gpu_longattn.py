"""lotus_attention_long_fwd / _bwd (csrc/attention_long.hip: the patch attention over tiles of up to 1024 rows, PointTransformerV3/
model.py:529-551) on the rows of tests/longattn_util.py against float64, into guarded, poisoned caller-owned buffers: forward, lse,
dq / dk / dv and the q/k-norm gradients at the project's per-kernel bar, coordattn_util.KERNEL_TOL = 2e-5 x max(1, |ref|max); the
route record of every call; a second backward gives the same bits; tiles of at most 128 rows given to the new entry points agree
with the 128-row exact-fp32 kernels within the same bar; ntiles == 0 / nblocks == 0 write nothing and keep the record."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import coordattn_util as cu  # noqa: E402
import ledger  # noqa: E402
import longattn_util as lu  # noqa: E402

GUARD = 64
FILL = 12345.0
TOL = cu.KERNEL_TOL


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops
    return ops


def _guarded(rows, cols):
    buf = torch.full((rows + GUARD, cols), FILL, dtype=torch.float32, device="cuda")
    return buf, buf[:rows]


def _guards_intact(bufs):
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        tail = buf[view.shape[0]:]
        assert torch.equal(tail, torch.full_like(tail, FILL)), f"{name}: rows past the end were written"


def _bar(rec, name, a, b, tol=TOL):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    e = float((a - b).abs().max()) if a.numel() else 0.0
    scale = max(1.0, float(b.abs().max()) if b.numel() else 0.0)
    rec[name] = e / scale
    return None if e <= tol * scale else f"{name}: max err {e:.3e} > {tol:.1e} * {scale:.3g}"


def _finish(test, rec, fails):
    ledger.record("longattn/" + test, **rec)
    print("   ", test, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in rec.items()})
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)


class Dev:
    """The device tensors of a row."""

    def __init__(self, row):
        v = lu.row_inputs(row)
        t = v["tabs"]
        i32 = dict(dtype=torch.int32, device="cuda")
        self.row, self.v, self.t = row, v, t
        self.n, self.C, self.H, self.d = sum(row.counts), row.H * row.d, row.H, row.d
        self.qkv, self.dout = v["qkv"].cuda(), v["dout"].cuda()
        self.qn = tuple(x.cuda() for x in v["qn"]) if row.norm else None
        self.kn = tuple(x.cuda() for x in v["kn"]) if row.norm else None
        self.gidx = torch.as_tensor(v["gidx"], **i32)
        self.owner, self.kext = torch.as_tensor(t["owner"], **i32), torch.as_tensor(t["kext"], **i32)
        self.ext_pos = torch.as_tensor(t["ext_pos"] if t["n_extra"] else np.zeros(1, np.int32), **i32)
        self.tiles, self.blocks = torch.as_tensor(t["tiles"], **i32), torch.as_tensor(t["blocks"], **i32)
        self.ntiles, self.npad, self.n_extra = len(t["tiles"]), t["npad"], t["n_extra"]
        self.len_max = int(t["tiles"][:, 1].max())
        self.seed = v["seed"]


def _fwd(ops, D, long=True, routes=None, ntiles=None, len_max=None):
    C, H, d = D.C, D.H, D.d
    b = dict(att=_guarded(D.n, C), lse=_guarded(D.npad, H))
    nt = D.ntiles if ntiles is None else ntiles
    if long:
        ops.attention_long_fwd(D.qkv, 3 * C, 0, D.qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, nt, D.qn, D.kn,
                               b["att"][1], b["lse"][1], H, d, len_max or D.len_max, D.row.drop, D.seed)
    else:
        ops.attention_fwd(D.qkv, 3 * C, 0, D.qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, nt, D.qn, D.kn,
                          b["att"][1], b["lse"][1], H, d, D.row.drop, D.seed)
    if routes is not None:
        routes.append(ops.last_attn_route())
    _guards_intact(b)
    return b["att"][1], b["lse"][1]


def _bwd(ops, D, att, lse, long=True, routes=None, nblocks=None, len_max=None):
    """-> (dqkv, norm gradients)"""
    C, H, d = D.C, D.H, D.d
    b = dict(dqkv=_guarded(D.n, 3 * C), extra=_guarded(max(D.n_extra, 1), 2 * C))
    dqkv = b["dqkv"][1]
    nb = D.ntiles if nblocks is None else nblocks
    if long:
        gr = ops.attention_long_bwd(D.qkv, 3 * C, 0, D.qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.blocks, nb, D.qn,
                                    D.kn, att, D.dout, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, H, d, len_max or D.len_max,
                                    D.row.drop, D.seed, D.kext, D.ext_pos, D.n_extra, b["extra"][1])
    else:
        gr = ops.attention_bwd(D.qkv, 3 * C, 0, D.qkv, 3 * C, C, 2 * C, D.gidx, D.gidx, D.owner, D.tiles, D.blocks, nb, D.qn,
                               D.kn, att, D.dout, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, 0, H, d, D.row.drop, D.seed, D.kext,
                               D.ext_pos, D.n_extra, b["extra"][1])
    if routes is not None:
        routes.append(ops.last_attn_route())
    _guards_intact(b)
    return dqkv, gr


@functools.lru_cache(maxsize=None)
def _case(rid):
    """Reference (float64, once per row) and the device run of the row: shared by the tests below, not modified."""
    ops = _ops()
    row = lu.ROW[rid]
    D = Dev(row)
    ref = lu.reference(row, D.v)
    routes = []
    att, lse = _fwd(ops, D, routes=routes)
    dqkv, gr = _bwd(ops, D, att, lse, routes=routes)
    return dict(D=D, ref=ref, att=att, lse=lse, dqkv=dqkv, gr=gr, routes=routes)


def test_rows_are_what_they_say():
    assert lu.self_check() == len(lu.ROWS)


@pytest.mark.parametrize("rid", [r.id for r in lu.ROWS])
def test_rows_against_float64(rid):
    ops = _ops()
    c = _case(rid)
    row, D, ref = lu.ROW[rid], c["D"], c["ref"]
    rec, fails = {"why": row.why}, []
    fails.append(_bar(rec, "fwd", c["att"], ref["out"]))
    fails.append(_bar(rec, "lse", c["lse"], ref["lse"]))
    C = D.C
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        fails.append(_bar(rec, name, c["dqkv"][:, sl], ref["dqkv"][:, sl]))
    if row.norm:
        for name, a, b in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), c["gr"], ref["norm"]):
            fails.append(_bar(rec, name, a, b))
    else:
        assert c["gr"] == [None] * 4
    assert float(ref["dqkv"][:, :C].abs().max()) > 1e-3 and float(ref["dqkv"][:, C:2 * C].abs().max()) > 1e-3
    # the kernels that ran
    R = ops.AttnRoute
    norm = int(row.norm)
    tail = (2 if row.norm else 0) | (1 if D.n_extra else 0)
    want = [R(ops.ATTN_LONG_FWD, 0, 0, 0, norm, 256, 57344, 0), R(ops.ATTN_LONG_BWD, 1, 0, 0, norm, 256, 75264, tail)]
    assert c["routes"] == want, (c["routes"], want)
    assert (R(8, 0, 0, 0, norm, 256, 57344, 0), R(9, 1, 0, 0, norm, 256, 75264, tail)) == tuple(want)
    _finish(rid, rec, fails)


@pytest.mark.parametrize("rid", lu.DETERMINISM_ROWS)
def test_second_backward_gives_the_same_bits(rid):
    ops = _ops()
    c = _case(rid)
    D = c["D"]
    dqkv, gr = _bwd(ops, D, c["att"], c["lse"])
    assert torch.equal(dqkv, c["dqkv"])
    for a, b in zip(gr, c["gr"]):
        assert (a is None and b is None) or torch.equal(a, b)
    att, lse = _fwd(ops, D)
    assert torch.equal(att, c["att"]) and torch.equal(lse, c["lse"])


@pytest.mark.parametrize("rid", [r.id for r in lu.SHORT_ROWS])
def test_short_tiles_agree_with_the_128_row_kernels(rid):
    """k_len <= 128: the new entry points compute what the exact-fp32 tile kernels compute (families 1 / 3), and what float64
    computes."""
    ops = _ops()
    row = lu.SHORT_ROW[rid]
    D = Dev(row)
    ref = lu.reference(row, D.v)
    r0, r1 = [], []
    att0, lse0 = _fwd(ops, D, long=False, routes=r0)
    dqkv0, gr0 = _bwd(ops, D, att0, lse0, long=False, routes=r0)
    att, lse = _fwd(ops, D, routes=r1)
    dqkv, gr = _bwd(ops, D, att, lse, routes=r1)
    assert [r.family for r in r0] == [ops.ATTN_FWD, ops.ATTN_BWD2] and [r.family for r in r1] == [ops.ATTN_LONG_FWD, ops.ATTN_LONG_BWD]
    rec, fails = {}, []
    for name, a, b, f in (("fwd", att, att0, ref["out"]), ("lse", lse, lse0, ref["lse"]), ("dqkv", dqkv, dqkv0, ref["dqkv"])):
        fails.append(_bar(rec, name, a, b))
        fails.append(_bar(rec, name + "_f64", a, f))
    if row.norm:
        for name, a, b, f in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), gr, gr0, ref["norm"]):
            fails.append(_bar(rec, name, a, b))
            fails.append(_bar(rec, name + "_f64", a, f))
    _finish("short/" + rid, rec, fails)


def test_a_longer_declared_length_changes_nothing():
    """len_max sizes the grid: slabs and images past a tile's rows do nothing (the 129-row tile declared as 1024)."""
    ops = _ops()
    c = _case("k129")
    D = c["D"]
    att, lse = _fwd(ops, D, len_max=1024)
    dqkv, gr = _bwd(ops, D, att, lse, len_max=1024)
    assert torch.equal(att, c["att"]) and torch.equal(lse, c["lse"]) and torch.equal(dqkv, c["dqkv"])


def test_nothing_to_do_writes_nothing_and_keeps_the_route_record():
    ops = _ops()
    c = _case("k129")
    D = c["D"]
    before = ops.last_attn_route()
    att, lse = _fwd(ops, D, ntiles=0)
    dqkv, gr = _bwd(ops, D, c["att"], c["lse"], nblocks=0)
    torch.cuda.synchronize()
    assert bool((att == FILL).all()) and bool((lse == FILL).all()) and bool((dqkv == FILL).all())
    assert ops.last_attn_route() == before
