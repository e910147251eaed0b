"""Run one row of tests/dense_edges.py on the GPU (test infrastructure, not collected): the raw C-ABI call into caller-owned
buffers with guard rows, twice; the float64 reference; the route; the arrival counters.

Bars (the project's own for these kernels, tests/test_gpu_gemm_dma.py and test_linear_dgrad_wgrad), relative to
max(1, |ref|max):  4e-7 * sqrt(reduction length) + 1e-6, x 1.4 with a dropout mask (the mask comes from ops.dropout on ones
with the same seed).  bf16 operands (precision 1): the same bar against the float64 product of the bf16-rounded operands,
relative to sum |a||b| per element; bf16x3 (precision 3): 2^-16 relative to sum |a||b| (test_linear_bf16_operand_paths).
The LayerNorm epilogue keeps the bars of test_input_gradient_with_layernorm_backward_epilogue.
The bf16-storage twin (rows with b16) keeps the bars of tests/test_gpu_bf16_ops.py on bf16-exact inputs, relative to the
largest magnitude of the reference: R_STORE = 6e-3 for the bf16 outputs (one rounding of a stored value), 1e-5 for the fp32
dw / db (the same fp32 arithmetic as the fp32 entry point)."""
import numpy as np
import torch
import torch.nn.functional as F

import dense_edges as de

GUARD = de.GUARD
FILL = 12345.0
R_STORE, R_B16_WGRAD = 6e-3, 1e-5


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops

    return ops


class Buf:
    """rows x cols floats inside a flat buffer with GUARD extra rows (at least GUARD floats) of FILL behind them."""

    def __init__(self, rows, cols, off4=False, dtype=torch.float32):
        n, lead = rows * cols, 1 if off4 else 0
        self.flat = torch.full((lead + n + GUARD * max(cols, 1),), FILL, dtype=dtype, device="cuda")
        self.view = self.flat[lead:lead + n].view(rows, cols)
        self.tail = self.flat[lead + n:]
        assert self.view.data_ptr() % 16 == (4 if off4 else 0)

    def guard_intact(self):
        return torch.equal(self.tail, torch.full_like(self.tail, FILL))


def _act(v, act):
    return F.gelu(v) if act == de.ACT_GELU else (F.leaky_relu(v, 0.02) if act == de.ACT_LEAKY else v)


def _act_grad(pre, act):
    if act == de.ACT_NONE:
        return torch.ones_like(pre)
    p = pre.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_act(p, act).sum(), p)
    return g


def _inputs(case, g):
    """-> {name: float32 CPU tensor} of every buffer the call reads (and the prior contents of an accumulating one)."""
    M, N, K = case.M, case.N, case.K
    red = K if case.call == "fwd" else N
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    v = {}
    for name, (rows, cols, written) in de.buffers(case).items():
        if written:
            v[name] = r(rows, cols) * 3.0 if case.opts.get("accumulate") else None
        elif name == "w":
            v[name] = r(rows, cols) / red ** 0.5
        elif name == "x" and case.call == "dgrad_ln":
            v[name] = r(rows, cols) * 1.5 + 0.3
        elif name == "gamma":
            v[name] = torch.rand(rows, cols, generator=g) + 0.5
        elif name in ("mean", "rstd"):
            v[name] = None   # from the LayerNorm forward
        else:
            v[name] = r(rows, cols)
        if case.opts.get("b16") and v[name] is not None and not written and name != "bias":
            v[name] = v[name].bfloat16().float()      # bf16-exact activations and weights: the products are then exact too
    return v


def _mask(ops, rows, cols, p, seed):
    from robot_3dlotus_amd import _capi

    prev, _capi.BF16 = _capi.BF16, False      # (an fp32 tensor of ones: the fp32 mask kernel, whichever row is running)
    try:
        return ops.dropout(torch.ones(rows, cols, device="cuda"), p, seed).double().cpu()
    finally:
        _capi.BF16 = prev


def reference(case, v, ops):
    """-> {output name: (float64 reference, scale tensor or None, bar)}."""
    M, N, K, o = case.M, case.N, case.K, case.opts
    prec = o.get("prec", 0)
    rnd = (lambda t: t.bfloat16().double()) if prec == 1 else (lambda t: t.double())
    red = K if case.call == "fwd" else (M if case.call == "wgrad" else N)
    bar = 2.0 ** -16 if prec == 3 else 4e-7 * red ** 0.5 + 1e-6
    if case.call == "fwd":
        pre = rnd(v["x"]) @ rnd(v["w"]).t()
        scale = (v["x"].abs().double() @ v["w"].abs().double().t()).clamp_min(1.0) if prec else None
        if "bias" in v:
            pre = pre + v["bias"].double()
        y = _act(pre, o.get("act", 0))
        if o.get("drop"):
            y = y * _mask(ops, M, N, o["drop"], de.drop_seed(case))
        if "residual" in v:
            y = y + v["residual"].double()
        out = {"y": (y, scale, bar * (1.4 if o.get("drop") else 1.0))}
        if o.get("pre"):
            out["pre"] = (pre, scale, bar)
        return out
    if case.call == "dgrad":
        dx = rnd(v["dy"]) @ rnd(v["w"])
        scale = (v["dy"].abs().double() @ v["w"].abs().double()).clamp_min(1.0) if prec else None
        if "pre" in v:
            dx = dx * _act_grad(v["pre"].double(), o.get("act", 0))
        if o.get("drop"):
            dx = dx * _mask(ops, M, K, o["drop"], de.drop_seed(case))
        if "add" in v:
            dx = dx + v["add"].double()
        return {"dx": (dx, scale, bar * (1.4 if o.get("drop") else 1.0))}
    if case.call == "wgrad":
        dw = (rnd(v["dy"]).t() @ rnd(v["x"])).reshape(-1, 1)
        db = v["dy"].double().sum(0).reshape(-1, 1)
        sw = (v["dy"].abs().double().t() @ v["x"].abs().double()).clamp_min(1.0).reshape(-1, 1) if prec else None
        sb = v["dy"].abs().double().sum(0).clamp_min(1.0).reshape(-1, 1) if prec else None
        bar_b = 4e-7 * M ** 0.5 + 1e-6
        prior_w = prior_b = 0.0
        if o.get("accumulate"):
            prior = v["dwdb"].double() if "dwdb" in v else None
            prior_w = prior[:N * K] if prior is not None else v["dw"].double()
            prior_b = prior[N * K:] if prior is not None else (v["db"].double() if "db" in v else 0.0)
        out = {"dw": (dw + prior_w, sw, bar)}
        if o.get("bias"):
            out["db"] = (db + prior_b, sb, bar_b)
        return out
    raise KeyError(case.call)


def run(case, counters, expect=None):
    """Run `case` twice into guarded buffers.  -> (record {name: relative error}, failures [text])."""
    from robot_3dlotus_amd import _capi

    prev, _capi.BF16 = _capi.BF16, bool(case.opts.get("b16"))   # (twin rows: every call and query below goes to lotus_b16_*)
    try:
        return _run(case, counters, expect)
    finally:
        _capi.BF16 = prev


def _run(case, counters, expect):
    ops = _ops()
    from robot_3dlotus_amd import _capi

    M, N, K, o = case.M, case.N, case.K, case.opts
    g = torch.Generator().manual_seed(7 * M + 3 * N + K)   # (the shape alone: variants of one shape are compared bit for bit)
    v = _inputs(case, g)
    bufs = {name: Buf(rows, cols, off4=(name == de.misaligned(case)), dtype=torch.bfloat16 if de.is_bf16(case, name) else torch.float32)
            for name, (rows, cols, _) in de.buffers(case).items()}
    written = [name for name, (_, _, w) in de.buffers(case).items() if w]
    for name, t in v.items():
        if t is not None and name not in written:
            bufs[name].view.copy_(t)
    ptr = {name: b.view for name, b in bufs.items()}
    if "dwdb" in ptr:
        ptr["dwdb_db"] = bufs["dwdb"].view.data_ptr() + 4 * N * K
    ws = ws_bytes = None
    q = de.workspace_query(case)
    if q:
        ws_bytes = _capi.query(q[0], *q[1])
        assert ws_bytes % 4 == 0
        if ws_bytes:
            ws = Buf(ws_bytes // 4, 1)        # exactly the queried size; the guard starts at its last byte
    ln_ws = ln_bytes = nparts = None
    if case.call == "dgrad_ln":
        _, mean, rstd = ops.ln_fwd(bufs["x"].view, bufs["gamma"].view.view(-1), torch.zeros(K, device="cuda"))
        bufs["mean"].view.copy_(mean.view(1, -1))
        bufs["rstd"].view.copy_(rstd.view(1, -1))
        ln_bytes = _capi.query("lotus_layernorm_bwd_workspace", M, K)
        ln_ws = Buf(ln_bytes // 4, 1)
        nparts = np.zeros(1, dtype=np.int32)
    args = de.arguments(case, ptr, ws.view if ws is not None else None, ws_bytes or 0, counters, ln_ws.view if ln_ws else None,
                        ln_bytes or 0, None if nparts is None else int(nparts.ctypes.data))
    fails, runs, want = [], [], tuple(case.route if expect is None else expect)
    for _ in range(2):
        for name in written:
            if v[name] is not None:
                bufs[name].view.copy_(v[name])
            else:
                bufs[name].view.fill_(FILL)
        _capi.call(de.ENTRY[case.call], *args)
        route = tuple(ops.last_dense_route())
        if route[:7] != want or route[7] != o.get("depth", route[7]):
            fails.append(f"{case.id}: route {route} instead of {want} (depth {o.get('depth', 'any')})")
        torch.cuda.synchronize()
        runs.append({name: bufs[name].view.clone() for name in written})
    for name in written:
        if not torch.equal(runs[0][name], runs[1][name]):
            fails.append(f"{case.id}: {name} differs between two runs")
    for name, b in list(bufs.items()) + [("workspace", ws), ("ln_workspace", ln_ws)]:
        if b is not None and not b.guard_intact():
            fails.append(f"{case.id}: {name}: rows past the end were written")
    if not bool((counters == 0).all()):
        fails.append(f"{case.id}: arrival counters left non-zero")
        counters.zero_()
    rec = {}
    if case.call == "dgrad_ln":
        _check_ln(case, v, bufs, runs[0], ln_ws, int(nparts[0]), ops, rec, fails)
    else:
        for name, (ref, scale, bar) in reference(case, v, ops).items():
            got = _output(case, runs[0], name).double().cpu()
            if o.get("b16"):
                e, bar = float((got - ref).abs().max()) / float(ref.abs().max()), (R_B16_WGRAD if name in ("dw", "db") else R_STORE)
            elif scale is None:
                e = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
            else:
                e = float(((got - ref).abs() / scale).max())
            rec[name] = e
            if not e <= bar:
                fails.append(f"{case.id}: {name} error {e:.3e} > {bar:.3e}")
    return rec, fails, runs[0]


def _output(case, outs, name):
    """dw / db of a weight gradient whether or not they share one slab."""
    if "dwdb" in outs and name in ("dw", "db"):
        nk = case.N * case.K
        return outs["dwdb"][:nk] if name == "dw" else outs["dwdb"][nk:]
    return outs[name]


def _check_ln(case, v, bufs, got, ln_ws, nparts, ops, rec, fails):
    """dx = LN'(dy w) + add, dz = dx * mask, dgamma / dbeta from the column partials: against float64 autograd."""
    from robot_3dlotus_amd import _capi

    M, N, K = case.M, case.N, case.K
    if case.opts.get("ln_fused"):
        if nparts != (M + 127) // 128:
            fails.append(f"{case.id}: nparts {nparts} instead of {(M + 127) // 128}")
        if not bool((got["dn"] == FILL).all()):
            fails.append(f"{case.id}: dn was written: the product reached memory, the LayerNorm epilogue did not run")
    else:   # the two-launch path: dn = dy w in memory, then lotus_layernorm_bwd on its own grid
        want = _capi.query("lotus_layernorm_bwd_parts", M, K)
        if nparts != want:
            fails.append(f"{case.id}: nparts {nparts} instead of lotus_layernorm_bwd_parts = {want}")
        ref_dn = v["dy"].double() @ v["w"].double()
        rec["dn"] = float((got["dn"].double().cpu() - ref_dn).abs().max()) / max(1.0, float(ref_dn.abs().max()))
        if not rec["dn"] <= 4e-7 * N ** 0.5 + 1e-6:
            fails.append(f"{case.id}: dn error {rec['dn']:.3e} > {4e-7 * N ** 0.5 + 1e-6:.3e}")
    dg, db = torch.empty(K, device="cuda"), torch.empty(K, device="cuda")
    _capi.call("lotus_layernorm_bwd_params_n", ln_ws.view, nparts, K, dg, db, 0)
    x64 = v["x"].double().requires_grad_(True)
    g64 = v["gamma"].view(-1).double().requires_grad_(True)
    b64 = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (K,), g64, b64, 1e-5).backward(v["dy"].double() @ v["w"].double())
    ref_dx = x64.grad + (v["add"].double() if "add" in v else 0.0)

    def err(a, b):
        return float((a.double().cpu() - b).abs().max()) / max(1.0, float(b.abs().max()))

    for name, e, bar in (("dx", err(got["dx"], ref_dx), 4e-7 * N ** 0.5 + 4e-6), ("dgamma", err(dg, g64.grad), 4e-7 * M ** 0.5 + 1e-5),
                         ("dbeta", err(db, b64.grad), 4e-7 * M ** 0.5 + 1e-5)):
        rec[name] = e
        if not e <= bar:
            fails.append(f"{case.id}: {name} error {e:.3e} > {bar:.3e}")
    if case.opts.get("dz"):
        mask = ops.dropout(torch.ones(M, K, device="cuda"), 0.1, de.drop_seed(case))
        if not torch.equal(got["dz"], got["dx"] * mask):
            fails.append(f"{case.id}: dz is not dx times the dropout mask")
