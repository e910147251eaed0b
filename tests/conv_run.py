"""Run one row of tests/conv_edges.py on the GPU (test infrastructure, not collected): the raw C-ABI call into caller-owned
buffers with guard rows and a sentinel fill, twice; the float64 restatement of the gather; the recorded route.

Bars (none of them new):
  fp32 fwd / dgrad      3e-6 * max(1, |ref|max)                      (test_subm_conv_fwd_dgrad_wgrad)
  fp32 wgrad / bgrad    5e-6 * max(1, |ref|max)
  precision 1           2e-6 against the float64 product of the bf16-rounded operands, per element relative to the
                        convolution of the absolute values (at least 1)   (test_subm_conv_bf16_operand_paths)
  precision 3           2^-16 against the exact operands, same scale; the bias gradient 2e-6 of sum |dy| in both modes
  bf16-storage twin     R_STORE = 6e-3 of |ref|max on stored activations, 1e-5 on the fp32 dw / db (tests/test_gpu_bf16_ops.py),
                        on bf16-exact inputs
A launch or device error ends the whole session (pytest.exit): nothing more is started on the device."""
import pytest
import torch

import conv_edges as ce

GUARD = ce.GUARD
FILL = 12345.0
R_STORE, R_B16_WGRAD = 6e-3, 1e-5


def _mods():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi, ops

    return _capi, ops


class Buf:
    """rows x cols elements inside a flat buffer with GUARD extra rows (at least GUARD elements) of FILL behind them."""

    def __init__(self, rows, cols, dtype=torch.float32):
        n = rows * cols
        self.flat = torch.full((n + GUARD * max(cols, 1),), FILL, dtype=dtype, device="cuda")
        self.view = self.flat[:n].view(rows, cols)
        self.tail = self.flat[n:]
        assert self.view.data_ptr() % 16 == 0

    def guard_intact(self):
        return torch.equal(self.tail, torch.full_like(self.tail, FILL))


def device(what, fn, *args):
    """A call that touches the device: any failure is the end of the session."""
    _capi, _ = _mods()
    try:
        return fn(*args)
    except (_capi.LotusError, RuntimeError) as e:
        pytest.exit(f"{what}: {e} — nothing more is started on the device", returncode=3)


def gather_ref(x, w, nbr, mode):
    """sum_t x[nbr[t][i]] w[:, t, :]^T (mode 0) or x[nbr[t][i]] w[:, T-1-t, :] (mode 1) in the dtype of x.  w [cout][T][cin]."""
    T, n = nbr.shape
    y = torch.zeros(n, w.shape[0] if mode == 0 else w.shape[2], dtype=x.dtype)
    for t in range(T):
        m = nbr[t] >= 0
        if bool(m.any()):
            wt = w[:, t, :].t() if mode == 0 else w[:, T - 1 - t, :]
            y[m] += x[nbr[t][m]] @ wt
    return y


def scatter_ref(dy, w, nbr):
    """The gradient of mode 0 with respect to x on the table as it stands: dx[nbr[t][p]] += dy[p] w[:, t, :]."""
    T, n = nbr.shape
    dx = torch.zeros(n, w.shape[2], dtype=dy.dtype)
    for t in range(T):
        m = nbr[t] >= 0
        if bool(m.any()):
            dx.index_add_(0, nbr[t][m], dy[m] @ w[:, t, :])
    return dx


def wgrad_ref(dy, x, nbr):
    T, n = nbr.shape
    dw = torch.zeros(dy.shape[1], T, x.shape[1], dtype=dy.dtype)
    for t in range(T):
        m = nbr[t] >= 0
        if bool(m.any()):
            dw[:, t, :] = dy[m].t() @ x[nbr[t][m]]
    return dw


def _inputs(row):
    sc, o = ce.scene(row.scene), row.opts
    n = sc.n
    g = torch.Generator().manual_seed(7 * n + 3 * row.cin + row.cout + row.T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    v = {}
    for name, (rows, cols, written, kind) in ce.buffers(row).items():
        if name == "w_t":
            continue
        if written:
            v[name] = r(rows, cols) * 3.0 if o.get("accumulate") else None
        elif name == "w":
            v[name] = r(rows, cols) / (row.cin * 9) ** 0.5
        else:
            v[name] = r(rows, cols)
        if o.get("b16") and v[name] is not None and not written and name != "bias":
            v[name] = v[name].bfloat16().float()       # bf16-exact activations and weights
    return v


def reference(row, v):
    """-> {output: (float64 reference, per-element scale or None, bar)}."""
    sc, o = ce.scene(row.scene), row.opts
    prec = o.get("prec", 0) if row.route.prec else 0     # (a kernel that always multiplies in fp32 is held to the fp32 bar)
    nbr = torch.from_numpy(sc.nbr).long()
    rnd = (lambda t: t.bfloat16().double()) if prec == 1 else (lambda t: t.double())
    tol = {0: None, 1: 2e-6, 3: 2.0 ** -16}[prec]
    if row.call == "wgrad":
        dy, x = v["dy"], v["x"]
        dw = wgrad_ref(rnd(dy), rnd(x), nbr).reshape(-1, 1)
        db = dy.double().sum(0).reshape(-1, 1)
        pw = pb = 0.0
        if o.get("accumulate"):
            wsz = dw.numel()
            pw = v["dwdb"][:wsz].double() if "dwdb" in v else v["dw"].double()
            pb = v["dwdb"][wsz:].double() if "dwdb" in v else (v["db"].double() if "db" in v else 0.0)
        out = {"dw": (dw + pw, None, 5e-6)}
        if prec:
            sw = wgrad_ref(dy.abs().double(), x.abs().double(), nbr).reshape(-1, 1)
            out["dw"] = (dw + pw, (sw + (pw.abs() if o.get("accumulate") else 0.0)).clamp_min(1.0), tol)
        if o["db"] != "none":
            sb = (dy.abs().double().sum(0).reshape(-1, 1) + (pb.abs() if o.get("accumulate") else 0.0)).clamp_min(1.0)
            out["db"] = (db + pb, sb, 2e-6) if prec else (db + pb, None, 5e-6)
        return out
    mode = ce.MODE[row.call]
    w = v["w"].view(row.cout, row.T, row.cin)
    if o.get("fold"):
        y = scatter_ref(v["x"].double(), w.double(), nbr)
    else:
        y = gather_ref(rnd(v["x"]), rnd(w), nbr, mode)
    rest = torch.zeros_like(y)
    if "bias" in v:
        rest = rest + v["bias"].double()
    if "add" in v:
        rest = rest + v["add"].double()
    scale = None
    if prec:
        scale = (gather_ref(v["x"].abs().double(), w.abs().double(), nbr, mode) + rest.abs()).clamp_min(1.0)
    return {"y": (y + rest, scale, tol if prec else 3e-6)}


def _setup(row):
    """Device buffers of the row.  -> (v, bufs, ptr, ws Buf or None, ws_bytes, keep-alive list)."""
    _capi, ops = _mods()
    sc, o = ce.scene(row.scene), row.opts
    b16 = bool(o.get("b16"))
    v = _inputs(row)
    bufs = {name: Buf(rows, cols, torch.bfloat16 if (b16 and kind == "act") else torch.float32)
            for name, (rows, cols, _, kind) in ce.buffers(row).items()}
    for name, t in v.items():
        if t is not None and not ce.buffers(row)[name][2]:
            bufs[name].view.copy_(t)
    ptr = {name: b.view for name, b in bufs.items()}
    keep = []
    nbr = torch.from_numpy(sc.nbr).cuda()
    ptr["nbr"] = nbr
    ri = ce.rowidx_of(row)
    if ri is not None:
        ptr["rowidx"] = torch.from_numpy(ri).cuda()
    if "dwdb" in ptr:
        ptr["dwdb_db"] = bufs["dwdb"].view.data_ptr() + 4 * row.cout * row.T * row.cin
    if "w_t" in bufs and row.call != "transpose" and o.get("prec", 0) in (0, 1, 3):
        device(row.id, _capi.call, "lotus_conv_weight_transpose", bufs["w"].view, bufs["w_t"].view, row.cout, row.T, row.cin, o.get("prec", 0))
    if o.get("tap_plan"):
        plan = torch.zeros(_capi.query("lotus_fe_tap_plan_ints", sc.n), dtype=torch.int32, device="cuda")
        device(row.id, _capi.call, "lotus_fe_tap_plan", nbr, ptr.get("rowidx"), sc.n, plan)
        ptr["tap_plan"] = plan
    if o.get("fold"):
        C = row.cout
        code0, order0 = torch.from_numpy(sc.extra["code0"]).cuda(), torch.from_numpy(sc.extra["order0"]).cuda()
        dyr = Buf(sc.n, C, bufs["x"].view.dtype)
        device(row.id, _capi.call, "lotus_conv_dup_fold", bufs["x"].view, code0, order0, sc.n, C, dyr.view)
        bufs["dyr"], ptr["x"] = dyr, dyr.view
        keep += [code0, order0]
    nbytes = ce.workspace_bytes(row, _capi.query)
    assert nbytes % 4 == 0
    ws = Buf(nbytes // 4, 1) if nbytes else None     # exactly the size handed over; the guard starts at its last byte
    return v, bufs, ptr, ws, nbytes, keep


def run(row, expect=None):
    """Run `row` twice into guarded buffers.  -> (record {name: error}, failures [text])."""
    _capi, _ = _mods()
    prev, _capi.BF16 = _capi.BF16, bool(row.opts.get("b16"))   # (twin rows: every call and query goes to lotus_b16_*)
    try:
        return _run(row, expect)
    finally:
        _capi.BF16 = prev


def _run(row, expect):
    _capi, ops = _mods()
    sc, o = ce.scene(row.scene), row.opts
    v, bufs, ptr, ws, nbytes, keep = _setup(row)
    written = [name for name, spec in ce.buffers(row).items() if spec[2]]
    args = ce.arguments(row, ptr, ws.view if ws is not None else None, nbytes)
    name = "lotus_subm_conv_wgrad" if row.call == "wgrad" else "lotus_subm_conv"
    fails, runs, want = [], [], tuple(row.route if expect is None else expect)
    for _ in range(2):
        for w in written:
            if v[w] is not None:
                bufs[w].view.copy_(v[w])
            else:
                bufs[w].view.fill_(FILL)
        device(row.id, _capi.call, name, *args)
        route = tuple(ops.last_conv_route())
        if route != want:
            fails.append(f"{row.id}: route {route} instead of {want}")
        if o.get("fold"):
            device(row.id, _capi.call, "lotus_conv_dup_mask", bufs["y"].view, ptr.get("add"), ptr["nbr"][row.T // 2], sc.n, row.cin)
        device(row.id, torch.cuda.synchronize)
        runs.append({w: bufs[w].view.clone() for w in written})
    for w in written:
        if not torch.equal(runs[0][w], runs[1][w]):
            fails.append(f"{row.id}: {w} differs between two runs")
    for bname, b in list(bufs.items()) + [("workspace", ws)]:
        if b is not None and not b.guard_intact():
            fails.append(f"{row.id}: {bname}: rows past the end were written")
    rec = {}
    for oname, (ref, scale, bar) in reference(row, v).items():
        got = _output(row, runs[0], oname).double().cpu().reshape(ref.shape)
        left = int((got == FILL).sum())
        if left:
            fails.append(f"{row.id}: {oname}: {left} elements still hold the sentinel")
        if o.get("b16"):
            e, bar = float((got - ref).abs().max()) / float(ref.abs().max()), (R_B16_WGRAD if oname in ("dw", "db") else R_STORE)
        elif scale is None:
            e = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        else:
            e = float(((got - ref).abs() / scale).max())
        rec[oname] = e
        if not e <= bar:
            fails.append(f"{row.id}: {oname} error {e:.3e} > {bar:.3e}")
    return rec, fails


def _output(row, outs, name):
    if "dwdb" in outs and name in ("dw", "db"):
        wsz = row.cout * row.T * row.cin
        return outs["dwdb"][:wsz] if name == "dw" else outs["dwdb"][wsz:]
    return outs[name]


def run_refusal(row):
    """The call must return row.opts['refuse'] before any launch: no route recorded, the outputs untouched.  -> failures."""
    _capi, ops = _mods()
    L = _capi.lib()
    sc, o = ce.scene(row.scene), row.opts
    fails = []
    before = tuple(ops.last_conv_route())
    if row.call == "transpose":
        w, wt = Buf(row.cout * row.T * row.cin, 1), Buf(2 * row.cout * row.T * row.cin, 1)
        rc = L.fn["lotus_conv_weight_transpose"](w.view.data_ptr(), wt.view.data_ptr(), row.cout, row.T, row.cin, 0, _capi.stream_ptr())
        outs = {"w_t": wt}
    else:
        v, bufs, ptr, ws, nbytes, keep = _setup(row)
        args = ce.arguments(row, ptr, ws.view if ws is not None else None, nbytes)
        rc = L.fn["lotus_subm_conv"](*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _capi.stream_ptr())
        outs = {"y": bufs["y"], "workspace": ws}
    device(row.id, torch.cuda.synchronize)
    if rc != o["refuse"]:
        fails.append(f"{row.id}: returned {rc} instead of {o['refuse']} ({L.last_error()})")
    if tuple(ops.last_conv_route()) != before:
        fails.append(f"{row.id}: a route was recorded: {tuple(ops.last_conv_route())}")
    for name, b in outs.items():
        if b is not None and not torch.equal(b.flat, torch.full_like(b.flat, FILL)):
            fails.append(f"{row.id}: {name} was written")
    return fails


__all__ = ["run", "run_refusal", "gather_ref", "scatter_ref", "wgrad_ref", "reference"]
