"""Run one row of tests/norm_edges.py on the GPU (test infrastructure, not collected): the raw C-ABI calls into caller-owned
buffers with guard rows (dense_run.Buf), twice; the float64 reference; the arrival counters.

Every buffer a call writes is a Buf — y, dx, dz, mean, rstd / invstd, dgamma, dbeta, the fp64 sums, the running averages, the
dmod slab — and the workspace has exactly the queried size, so its guard starts at its last byte.  Two runs must be bit-equal,
every guard intact, the counter buffer of the stream zero after every fused call.  No element of any output is skipped.

Bars (the project's own for these kernels), relative to max(1, |ref|max) of the float64 reference:
  LayerNorm   3e-6 forward (y, mean, rstd), 5e-6 backward (dx, dgamma, dbeta)                  tests/test_gpu_ops.py test_layernorm
  BatchNorm   3e-6 forward (y, mean, invstd), 1e-5 backward (dx, dgamma, dbeta, the backward sums: their terms go through the
              fp32 GELU fit), 1e-6 running averages                                             test_batchnorm_gelu
  AdaNorm     2e-5 LayerNorm sites, 3e-5 BatchNorm sites (incl. the fp64 message of lotus_adabn_bwd_stats, whose terms are fp32
              partial sums)                                                                     tests/test_gpu_adanorm.py
  bf16 twin   R_STORE = 6e-3 for stored bf16 outputs (y, dx, dz) against the fp32 entry point on the same bf16-exact inputs, 1e-5
              for the fp32 parameter gradients, relative to |ref|max; mean / rstd / invstd bit-equal   tests/test_gpu_bf16_ops.py
Derived bars:
  forward fp64 sums of both BatchNorm statistics paths: every term (x, or x x formed in double) is exact, and any fixed-order
  double sum of M terms errs by at most (M - 1) 2^-53 sum |term|: bar M 2^-52 sum |term| per column against a float64 sum.
  lotus_ada_silu: __expf(-v) = 2^(-v log2 e): the fp32 product errs by |v| 1.44 2^-24 in the exponent, i.e. <= 6 2^-24 = 3.6e-7
  relative for |v| <= 6, plus one ulp of the exponential and three roundings: the sigmoid is good to 7e-7 relative, and
  d sigmoid = sigmoid (1 - sigmoid) (relative error) <= 1.8e-7 absolute, so y = v sigmoid and dy sigmoid (1 + v (1 - sigmoid)) stay
  under 1e-6 of the largest output: bar 2e-6 (inputs are clamped to |v| <= 6).

Input conditions (asserted; offending rows / columns are redrawn from the next seed, no bar is loosened): LayerNorm rows with
C < 64 have variance >= 0.05; BatchNorm columns over M >= 2 rows have batch variance >= 0.01 (eps = 1e-3 then bounds invstd at
31.6 either way); with LeakyReLU no float64 pre-activation lies within 1e-5 of zero (a sign flipped by rounding is a change of
route, slope 1 against 0.02, not an error)."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import dense_run
import norm_edges as ne
from dense_run import FILL, R_STORE, Buf

R_B16_PARAM = 1e-5
LN_FWD, LN_BWD = 3e-6, 5e-6
BN_FWD, BN_BWD, BN_RUN = 3e-6, 1e-5, 1e-6
ADA_LN, ADA_BN = 2e-5, 3e-5
SILU_BAR = 2e-6
SLAB_OFF, SLAB_EXTRA = 12, 20     # the norm's [shift | scale] slice starts at column 12 of a slab 20 columns wider


def _capi():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi

    return _capi


def _act(v, act):
    return F.gelu(v) if act == ne.ACT_GELU else (F.leaky_relu(v, 0.02) if act == ne.ACT_LEAKY else v)


def _rel(got, ref):
    """|got - ref|max relative to max(1, |ref|max)."""
    if ref.numel() == 0:
        return 0.0
    return float((got.double().cpu().reshape(ref.shape) - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _rel_twin(got, ref):
    """|got - ref|max relative to |ref|max (absolute where the reference is identically zero)."""
    if ref.numel() == 0:
        return 0.0
    d, s = float((got.double() - ref.double()).abs().max()), float(ref.double().abs().max())
    return d / s if s > 0 else d


class _Check:
    def __init__(self, row):
        self.id, self.rec, self.fails = row.id, {}, []

    def bar(self, name, e, bar):
        self.rec[name] = e
        if not e <= bar:
            self.fails.append(f"{self.id}: {name} error {e:.3e} > {bar:.3e}")

    def same(self, what, a, b):
        if not torch.equal(a, b):
            self.fails.append(f"{self.id}: {what} not bit-equal")

    def true(self, cond, what):
        if not cond:
            self.fails.append(f"{self.id}: {what}")


class _Bufs:
    """Named guarded buffers; `prior` holds what an accumulating output starts from (otherwise FILL)."""

    def __init__(self):
        self.b, self.written, self.prior = {}, [], {}

    def inp(self, name, t, dtype=torch.float32):
        b = Buf(t.shape[0], t.shape[1], dtype=dtype)
        b.view.copy_(t)
        self.b[name] = b
        return b.flat.data_ptr()

    def out(self, name, rows, cols, dtype=torch.float32, prior=None):
        self.b[name] = Buf(rows, cols, dtype=dtype)
        self.written.append(name)
        if prior is not None:
            self.prior[name] = prior.reshape(rows, cols)
        return self.b[name].flat.data_ptr()

    def reset(self):
        for name in self.written:
            if name in self.prior:
                self.b[name].view.copy_(self.prior[name])
            else:
                self.b[name].view.fill_(FILL)

    def snapshot(self):
        return {name: self.b[name].view.clone() for name in self.written}

    def guards(self, chk):
        for name, b in self.b.items():
            chk.true(b.guard_intact(), f"{name}: rows past the end were written")


def _twice(bufs, chk, body):
    """Run `body` twice from reset outputs; -> the outputs of the first run (CPU copies are taken by the caller)."""
    runs = []
    for _ in range(2):
        bufs.reset()
        body()
        torch.cuda.synchronize()
        runs.append(bufs.snapshot())
    for name in bufs.written:
        chk.same(f"{name} between two runs", runs[0][name], runs[1][name])
    bufs.guards(chk)
    return runs[0]


def _workspace(bufs, capi, query, *args):
    nbytes = capi.query(query, *args)
    assert nbytes % 4 == 0 and nbytes > 0
    bufs.b["workspace"] = Buf(nbytes // 4, 1)       # exactly the queried size: the guard starts at its last byte
    return bufs.b["workspace"].flat.data_ptr(), nbytes


def _counters_zero(counters, chk, after):
    torch.cuda.synchronize()
    if not bool((counters == 0).all()):
        chk.fails.append(f"{chk.id}: arrival counters left non-zero after {after}")
        counters.zero_()


# ================================================================================================= LayerNorm
def ln_inputs(M, C, opts):
    """-> {name: float32 CPU tensor}.  The shape alone seeds them: variants of one shape are compared bit for bit."""
    seed = 100003 * C + M
    g = torch.Generator().manual_seed(seed)
    rnd = (lambda t: t.bfloat16().float()) if opts.get("b16") else (lambda t: t)
    r = lambda *s: rnd(torch.randn(*s, generator=g))  # noqa: E731
    v = {"x": rnd(torch.randn(M, C, generator=g) * 2 + 0.5), "res": r(M, C), "dy": r(M, C), "add": r(M, C),
         "gamma": torch.rand(1, C, generator=g) + 0.5, "beta": torch.randn(1, C, generator=g),
         "prior_g": torch.randn(1, C, generator=g) * 3, "prior_b": torch.randn(1, C, generator=g) * 3}
    if C < 64 and M:
        for k in itertools.count(1):
            bad = v["x"].double().var(1, unbiased=False) < 0.05
            if not bool(bad.any()):
                break
            g2 = torch.Generator().manual_seed(seed + 7919 * k)
            v["x"][bad] = rnd(torch.randn(int(bad.sum()), C, generator=g2) * 2 + 0.5)
        assert bool((v["x"].double().var(1, unbiased=False) >= 0.05).all())
    for k in ("res", "add"):
        if not opts.get(k):
            del v[k]
    return v


def _ln_pass(row, v, b16, chk):
    capi = _capi()
    M, C, o = row.shape, row.C, row.opts
    adt = torch.bfloat16 if b16 else torch.float32
    acc = 1 if o.get("accumulate") else 0
    pg, pb = (v["prior_g"], v["prior_b"]) if acc else (None, None)
    B = _Bufs()
    x, dy = B.inp("x", v["x"], adt), B.inp("dy", v["dy"], adt)
    res = B.inp("res", v["res"], adt) if "res" in v else None
    add = B.inp("add", v["add"], adt) if "add" in v else None
    gam, bet = B.inp("gamma", v["gamma"]), B.inp("beta", v["beta"])
    y, mean, rstd = B.out("y", M, C, adt), B.out("mean", M, 1), B.out("rstd", M, 1)
    dx, dg, db = B.out("dx", M, C, adt), B.out("dgamma", 1, C, prior=pg), B.out("dbeta", 1, C, prior=pb)
    ws, ws_bytes = _workspace(B, capi, "lotus_layernorm_bwd_workspace", M, C)
    seed = 0x5EED0000 + 131 * M + C
    extra = []
    if o.get("nostat"):
        y2 = B.out("y_nostat", M, C, adt)
        extra.append(lambda: capi.call("lotus_layernorm_fwd", x, res, gam, bet, y2, None, None, M, C, ne.LN_EPS))
    if o.get("dz"):
        dz, dx2 = B.out("dz", M, C, adt), B.out("dx_nodz", M, C, adt)
    if o.get("deferred"):
        dx3 = B.out("dx_def", M, C, adt)
        d = {n: B.out(n, 1, C, prior=(pg if "gamma" in n else pb)) for n in ("dgamma_def", "dbeta_def", "dgamma_n", "dbeta_n", "dgamma_n0", "dbeta_n0")}
        parts = capi.query("lotus_layernorm_bwd_parts", M, C)

    def body():
        B.b["workspace"].view.fill_(FILL)
        capi.call("lotus_layernorm_fwd", x, res, gam, bet, y, mean, rstd, M, C, ne.LN_EPS)
        for f in extra:
            f()
        if o.get("dz"):
            capi.call("lotus_layernorm_bwd", dy, x, mean, rstd, gam, add, dx2, None, None, M, C, 0, None, 0.0, 0, ws, ws_bytes)
            capi.call("lotus_layernorm_bwd", dy, x, mean, rstd, gam, add, dx, dg, db, M, C, acc, dz, ne.DROP_P, seed, ws, ws_bytes)
        else:
            capi.call("lotus_layernorm_bwd", dy, x, mean, rstd, gam, add, dx, dg, db, M, C, acc, None, 0.0, 0, ws, ws_bytes)
        if o.get("deferred"):
            capi.call("lotus_layernorm_bwd", dy, x, mean, rstd, gam, add, dx3, None, None, M, C, 0, None, 0.0, 0, ws, ws_bytes)
            capi.call("lotus_layernorm_bwd_params", ws, M, C, d["dgamma_def"], d["dbeta_def"], acc)
            capi.call("lotus_layernorm_bwd_params_n", ws, parts, C, d["dgamma_n"], d["dbeta_n"], acc)
            capi.call("lotus_layernorm_bwd_params_n", ws, 0, C, d["dgamma_n0"], d["dbeta_n0"], acc)

    got = _twice(B, chk, body)
    if o.get("nostat"):
        chk.same("y with mean = rstd = NULL", got["y_nostat"], got["y"])
    if o.get("dz"):
        chk.same("dx with and without the dz output", got["dx_nodz"], got["dx"])
        if not b16:
            mask = dense_run._mask(dense_run._ops(), M, C, ne.DROP_P, seed).float().cuda()
            chk.same("dz and dx times the dropout mask", got["dz"], got["dx"] * mask)
            chk.true(0.02 < float((mask == 0).float().mean()) < 0.25, "the dropout mask of dz drops about a tenth")
    if o.get("deferred"):
        chk.same("dx of the deferred path", got["dx_def"], got["dx"])
        for n in ("dgamma", "dbeta"):
            chk.same(f"{n}: lotus_layernorm_bwd_params against the one-call result", got[n + "_def"], got[n])
            chk.same(f"{n}: _params_n against _params", got[n + "_n"], got[n + "_def"])
            want = (pg if n == "dgamma" else pb).cuda() if acc else torch.zeros(1, C, device="cuda")
            chk.same(f"{n}: _params_n over no partial rows", got[n + "_n0"], want)
    return got


def _ln_reference(row, v):
    M, C = row.shape, row.C
    x64 = v["x"].double().requires_grad_(True)
    g64, b64 = v["gamma"].view(-1).double().requires_grad_(True), v["beta"].view(-1).double().requires_grad_(True)
    yr = F.layer_norm(x64, (C,), g64, b64, ne.LN_EPS)
    if M:
        yr.backward(v["dy"].double())
    dxr = x64.grad if M else torch.zeros(0, C, dtype=torch.float64)
    dgr, dbr = (g64.grad, b64.grad) if M else (torch.zeros(C, dtype=torch.float64),) * 2
    mu = v["x"].double().mean(1, keepdim=True) if M else torch.zeros(0, 1, dtype=torch.float64)
    var = v["x"].double().var(1, unbiased=False, keepdim=True) if M else mu
    if row.opts.get("accumulate"):
        dgr, dbr = dgr + v["prior_g"].view(-1).double(), dbr + v["prior_b"].view(-1).double()
    return {"y": yr.detach() + (v["res"].double() if "res" in v else 0.0), "mean": mu, "rstd": (var + ne.LN_EPS).rsqrt() if M else mu,
            "dx": dxr + (v["add"].double() if "add" in v else 0.0), "dgamma": dgr.view(1, C), "dbeta": dbr.view(1, C)}


def _run_ln(row, counters, chk):
    v = ln_inputs(row.shape, row.C, row.opts)
    got = _ln_pass(row, v, False, chk)
    ref = _ln_reference(row, v)
    for name in ("y", "mean", "rstd"):
        chk.bar(name, _rel(got[name], ref[name]), LN_FWD)
    for name in ("dx", "dgamma", "dbeta"):
        chk.bar(name, _rel(got[name], ref[name]), LN_BWD)
    if row.opts.get("b16"):
        capi = _capi()
        prev, capi.BF16 = capi.BF16, True      # every call and query of the pass goes to lotus_b16_*
        try:
            twin = _ln_pass(row, v, True, chk)
        finally:
            capi.BF16 = prev
        chk.true(twin["y"].dtype == torch.bfloat16 and twin["dx"].dtype == torch.bfloat16, "the twin's activations are bf16")
        for name in ("y", "dx") + (("dz",) if row.opts.get("dz") else ()):
            chk.bar("b16/" + name, _rel_twin(twin[name], got[name]), R_STORE)
        for name in ("dgamma", "dbeta"):
            chk.bar("b16/" + name, _rel_twin(twin[name], got[name]), R_B16_PARAM)
        for name in ("mean", "rstd"):
            chk.same(f"{name} of the bf16 twin and the fp32 entry point", twin[name], got[name])


# ================================================================================================= BatchNorm
def _bn_pre64(x, gamma, beta):
    """float64 pre-activation of the training forward: (x - mean) / sqrt(var + eps) gamma + beta."""
    x = x.double()
    mu, var = x.mean(0, keepdim=True), x.var(0, unbiased=False, keepdim=True)
    return (x - mu) / (var + ne.BN_EPS).sqrt() * gamma.double() + beta.double()


def bn_inputs(M, C, opts, scale=1.7, shift=0.3):
    seed = 100003 * C + M + 17
    g = torch.Generator().manual_seed(seed)
    rnd = (lambda t: t.bfloat16().float()) if opts.get("b16") else (lambda t: t)
    v = {"x": rnd(torch.randn(M, C, generator=g) * scale + shift), "dy": rnd(torch.randn(M, C, generator=g)),
         "gamma": torch.rand(1, C, generator=g) + 0.5, "beta": torch.randn(1, C, generator=g) * 0.1,
         "rm": torch.randn(1, C, generator=g) * 0.1, "rv": torch.rand(1, C, generator=g) + 0.5,
         "prior_g": torch.randn(1, C, generator=g) * 3, "prior_b": torch.randn(1, C, generator=g) * 3}

    def bad_columns():
        bad = torch.zeros(C, dtype=torch.bool)
        if M >= 2:
            bad |= v["x"].double().var(0, unbiased=False) < 0.01
        if opts.get("act") == ne.ACT_LEAKY and M:
            bad |= (_bn_pre64(v["x"], v["gamma"], v["beta"]).abs() < 1e-5).any(0)
            rm, rv = v["rm"].double(), v["rv"].double()
            bad |= (((v["x"].double() - rm) / (rv + ne.BN_EPS).sqrt() * v["gamma"].double() + v["beta"].double()).abs() < 1e-5).any(0)
        return bad

    for k in itertools.count(1):
        bad = bad_columns()
        if not bool(bad.any()):
            break
        g2 = torch.Generator().manual_seed(seed + 7919 * k)
        v["x"][:, bad] = rnd(torch.randn(M, int(bad.sum()), generator=g2) * scale + shift)
    assert not bool(bad_columns().any())
    return v


def _bn_pass(row, v, b16, chk, counters):
    capi = _capi()
    M, C, act = row.shape, row.C, row.opts["act"]
    adt = torch.bfloat16 if b16 else torch.float32
    f64 = torch.float64
    cnt = counters.data_ptr() + capi.query("lotus_bn_counters_offset")
    eps, mom = ne.BN_EPS, ne.BN_MOMENTUM
    B = _Bufs()
    x, dy = B.inp("x", v["x"], adt), B.inp("dy", v["dy"], adt)
    gam, bet = B.inp("gamma", v["gamma"]), B.inp("beta", v["beta"])
    rm0, rv0 = B.inp("rm0", v["rm"]), B.inp("rv0", v["rv"])
    ws, ws_bytes = _workspace(B, capi, "lotus_batchnorm_workspace", M, C)
    S = lambda n: B.out(n, 2 * C + 1, 1, f64)  # noqa: E731
    V = lambda n, prior=None: B.out(n, 1, C, prior=prior)  # noqa: E731
    A = lambda n: B.out(n, M, C, adt)  # noqa: E731
    st = {k: (V("mean_" + k), V("invstd_" + k), V("rm_" + k, v["rm"]), V("rv_" + k, v["rv"])) for k in "abcde"}
    sums = {k: S("sums_" + k) for k in "abcefgv"}
    y_b, y_d, y_v = A("y_b"), A("y_d"), A("y_v")
    dg_f, db_f = V("dgamma_f"), V("dbeta_f")
    dx_h, dg_h, db_h = A("dx_h"), V("dgamma_h"), V("dbeta_h")
    dx_i, dg_i, db_i = A("dx_i"), V("dgamma_i", v["prior_g"]), V("dbeta_i", v["prior_b"])
    dx_j = A("dx_j")
    mean_v, invstd_v = V("mean_v"), V("invstd_v")
    dx_v, dg_v, db_v = A("dx_v"), V("dgamma_v"), V("dbeta_v")
    dx_w, dg_w, db_w = A("dx_w"), V("dgamma_w", v["prior_g"]), V("dbeta_w", v["prior_b"])

    def fused(name, *args):
        capi.call(name, *args, ws, ws_bytes, cnt)
        _counters_zero(counters, chk, name)

    def body():
        B.b["workspace"].view.fill_(FILL)
        m, i, rm, rv = st["a"]      # one launch: sums, statistics, running averages
        fused("lotus_batchnorm_stats_fused", x, sums["a"], m, i, rm, rv, M, C, eps, mom)
        m, i, rm, rv = st["b"]      # the sums alone, then the finalisation
        fused("lotus_batchnorm_stats_fused", x, sums["b"], None, None, None, None, M, C, 0.0, 0.0)
        capi.call("lotus_batchnorm_finalize", sums["b"], m, i, rm, rv, C, eps, mom)
        capi.call("lotus_batchnorm_apply", x, m, i, gam, bet, y_b, M, C, act)
        m, i, rm, rv = st["c"]      # statistics in two launches, then the finalisation
        capi.call("lotus_batchnorm_stats", x, sums["c"], M, C, ws, ws_bytes)
        capi.call("lotus_batchnorm_finalize", sums["c"], m, i, rm, rv, C, eps, mom)
        m, i, rm, rv = st["d"]      # the apply pass finishes the statistics itself
        capi.call("lotus_batchnorm_apply_sums", x, sums["a"], gam, bet, y_d, m, i, rm, rv, M, C, act, eps, mom)
        m, i, rm, rv = st["e"]      # ... and with no local rows: the statistics alone (the count comes with the sums)
        capi.call("lotus_batchnorm_apply_sums", None, sums["a"], gam, bet, None, m, i, rm, rv, 0, C, act, eps, mom)
        m, i = st["a"][:2]
        fused("lotus_batchnorm_bwd_stats_fused", dy, x, m, i, gam, bet, sums["e"], M, C, act)
        fused("lotus_batchnorm_bwd_stats_fused_params", dy, x, m, i, gam, bet, sums["f"], dg_f, db_f, M, C, act)
        capi.call("lotus_batchnorm_bwd_stats", dy, x, m, i, gam, bet, sums["g"], M, C, act, ws, ws_bytes)
        capi.call("lotus_batchnorm_bwd_apply", dy, x, m, i, gam, bet, sums["e"], dx_h, dg_h, db_h, M, C, act, 1, 0)
        capi.call("lotus_batchnorm_bwd_apply", dy, x, m, i, gam, bet, sums["e"], dx_i, dg_i, db_i, M, C, act, 1, 1)
        capi.call("lotus_batchnorm_bwd_apply", dy, x, m, i, gam, bet, sums["e"], dx_j, None, None, M, C, act, 1, 0)
        # eval mode: the running statistics as constants
        capi.call("lotus_batchnorm_eval_stats", rm0, rv0, mean_v, invstd_v, C, eps)
        capi.call("lotus_batchnorm_apply", x, mean_v, invstd_v, gam, bet, y_v, M, C, act)
        fused("lotus_batchnorm_bwd_stats_fused", dy, x, mean_v, invstd_v, gam, bet, sums["v"], M, C, act)
        capi.call("lotus_batchnorm_bwd_apply", dy, x, mean_v, invstd_v, gam, bet, sums["v"], dx_v, dg_v, db_v, M, C, act, 0, 0)
        capi.call("lotus_batchnorm_bwd_apply", dy, x, mean_v, invstd_v, gam, bet, sums["v"], dx_w, dg_w, db_w, M, C, act, 0, 1)

    got = _twice(B, chk, body)
    four = ("mean", "invstd", "rm", "rv")
    for k, what in (("b", "stats_fused(sums) + finalize"), ("c", "stats + finalize"), ("d", "apply_sums"), ("e", "apply_sums with M = 0")):
        for n in four:
            chk.same(f"{n}: {what} against stats_fused", got[f"{n}_{k}"], got[f"{n}_a"])
    chk.same("sums: stats_fused with and without the statistics", got["sums_b"], got["sums_a"])
    chk.same("y: apply_sums against finalize + apply", got["y_d"], got["y_b"])
    chk.same("sums: bwd_stats_fused_params against bwd_stats_fused", got["sums_f"], got["sums_e"])
    chk.same("dbeta of bwd_stats_fused_params and float(sums[:C])", got["dbeta_f"].view(-1), got["sums_e"].view(-1)[:C].float())
    chk.same("dgamma of bwd_stats_fused_params and float(sums[C:2C])", got["dgamma_f"].view(-1), got["sums_e"].view(-1)[C:2 * C].float())
    for mode, plain, accd in (("train", "h", "i"), ("eval", "v", "w")):
        chk.same(f"dx ({mode}) with accumulate", got["dx_" + accd], got["dx_" + plain])
        chk.same(f"dgamma ({mode}): prior + plain", got["dgamma_" + accd], v["prior_g"].cuda() + got["dgamma_" + plain])
        chk.same(f"dbeta ({mode}): prior + plain", got["dbeta_" + accd], v["prior_b"].cuda() + got["dbeta_" + plain])
    chk.same("dx with dgamma = NULL", got["dx_j"], got["dx_h"])
    for k in "abcefgv":
        chk.true(float(got["sums_" + k].view(-1)[2 * C]) == float(M), f"sums_{k}[2C] is the row count")
    return got


def _bn_reference(row, v):
    """float64: F.batch_norm + autograd; M = 1 in training (which PyTorch refuses) by hand: variance 0, the unbiased variance equal
    to it, xhat = 0, dx = 0.  (The kernel's dx of one row is not exactly zero: dz - mean(dz) keeps the rounding error of the product
    dy act'(z), a few 1e-8, times gamma invstd <= 1.5 x 31.6: 2.5e-6 measured, inside the backward bar.)"""
    M, C, act = row.shape, row.C, row.opts["act"]
    x, dy = v["x"].double(), v["dy"].double()
    ref = {"sum_x": x.sum(0), "sum_xx": (x * x).sum(0), "abs_x": x.abs().sum(0)}
    for mode in ("train", "eval"):
        xd = x.clone().requires_grad_(True)
        gd, bd = v["gamma"].view(-1).double().requires_grad_(True), v["beta"].view(-1).double().requires_grad_(True)
        rm, rv = v["rm"].view(-1).double().clone(), v["rv"].view(-1).double().clone()
        if mode == "train" and M == 1:
            n = (xd - xd.detach()) * (0.0 + ne.BN_EPS) ** -0.5 * gd + bd     # xhat = 0; d xhat / dx cancels against the batch mean
            mean, var = x[0].clone(), torch.zeros(C, dtype=torch.float64)
            rm, rv = (1 - ne.BN_MOMENTUM) * rm + ne.BN_MOMENTUM * mean, (1 - ne.BN_MOMENTUM) * rv
        else:
            n = F.batch_norm(xd, rm, rv, gd, bd, mode == "train", ne.BN_MOMENTUM, ne.BN_EPS)
            mean, var = (x.mean(0), x.var(0, unbiased=False)) if mode == "train" else (v["rm"].view(-1).double(), v["rv"].view(-1).double())
        invstd = (var + ne.BN_EPS).rsqrt()
        y = _act(n, act)
        y.backward(dy)
        pre = n.detach().clone().requires_grad_(True)
        (dz,) = torch.autograd.grad(_act(pre, act).sum(), pre)
        dz = dz * dy
        xhat = (x - mean) * invstd
        dxr = torch.zeros_like(x) if (mode == "train" and M == 1) else xd.grad
        ref[mode] = dict(y=y.detach(), mean=mean, invstd=invstd, rm=rm, rv=rv, dx=dxr, dgamma=gd.grad, dbeta=bd.grad,
                         sum_dz=dz.sum(0), sum_dzx=(dz * xhat).sum(0))
    return ref


def _bn_check(row, got, ref, chk, tag=""):
    M, C = row.shape, row.C
    t, e = ref["train"], ref["eval"]
    for k in "ac":        # both orders of summation against the derived fp64 bar, per column
        s = got["sums_" + k].view(-1).cpu()
        for name, r, mag in (("sum_x", ref["sum_x"], ref["abs_x"]), ("sum_xx", ref["sum_xx"], ref["sum_xx"])):
            part = s[:C] if name == "sum_x" else s[C:2 * C]
            excess = float(((part - r).abs() - M * 2.0 ** -52 * mag).max())
            chk.rec[f"{tag}{name}_{k}/rel"] = float(((part - r).abs() / mag.clamp_min(1e-300)).max())
            chk.true(excess <= 0.0, f"{tag}{name} of sums_{k} is off by more than M 2^-52 sum |term| (excess {excess:.3e})")
    for n, bar in (("mean", BN_FWD), ("invstd", BN_FWD), ("rm", BN_RUN), ("rv", BN_RUN)):
        chk.bar(f"{tag}{n}", _rel(got[n + "_a"], t[n].view(1, C)), bar)
    chk.bar(f"{tag}y", _rel(got["y_b"], t["y"]), BN_FWD)
    chk.bar(f"{tag}y_eval", _rel(got["y_v"], e["y"]), BN_FWD)
    chk.bar(f"{tag}mean_eval", _rel(got["mean_v"], e["mean"].view(1, C)), BN_FWD)
    chk.bar(f"{tag}invstd_eval", _rel(got["invstd_v"], e["invstd"].view(1, C)), BN_FWD)
    for k, r in (("e", t), ("g", t), ("v", e)):
        s = got["sums_" + k].view(-1).cpu()
        chk.bar(f"{tag}sums_{k}/dz", _rel(s[:C], r["sum_dz"]), BN_BWD)
        chk.bar(f"{tag}sums_{k}/dz_xhat", _rel(s[C:2 * C], r["sum_dzx"]), BN_BWD)
    for k, r, mode in (("h", t, ""), ("v", e, "_eval")):
        for n in ("dx", "dgamma", "dbeta"):
            chk.bar(f"{tag}{n}{mode}", _rel(got[f"{n}_{k}"], r[n].view(got[f"{n}_{k}"].shape)), BN_BWD)


def _run_bn(row, counters, chk):
    v = bn_inputs(row.shape, row.C, row.opts)
    got = _bn_pass(row, v, False, chk, counters)
    _bn_check(row, got, _bn_reference(row, v), chk)
    if row.opts.get("b16"):
        capi = _capi()
        prev, capi.BF16 = capi.BF16, True
        try:
            twin = _bn_pass(row, v, True, chk, counters)
        finally:
            capi.BF16 = prev
        chk.true(twin["y_b"].dtype == torch.bfloat16 and twin["dx_h"].dtype == torch.bfloat16, "the twin's activations are bf16")
        for name in ("y_b", "y_d", "y_v", "dx_h", "dx_j", "dx_v"):
            chk.bar("b16/" + name, _rel_twin(twin[name], got[name]), R_STORE)
        for name in ("dgamma_h", "dbeta_h", "dgamma_f", "dbeta_f", "dgamma_v", "dbeta_v"):
            chk.bar("b16/" + name, _rel_twin(twin[name], got[name]), R_B16_PARAM)
        for name in ("mean_a", "invstd_a", "mean_d", "invstd_d", "rm_a", "rv_a"):
            chk.same(f"{name} of the bf16 twin and the fp32 entry point", twin[name], got[name])


def _run_bn0(row, counters, chk):
    """No rows on the two-launch path: the sums are zero and carry a count of zero (a SyncBatchNorm shard without points)."""
    capi = _capi()
    C = row.C
    B = _Bufs()
    z = torch.zeros(0, C)
    x, dy = B.inp("x", z), B.inp("dy", z)
    one = torch.ones(1, C)
    m, i, gam, bet = B.inp("mean", one * 0.3), B.inp("invstd", one), B.inp("gamma", one), B.inp("beta", one * 0.1)
    s_f, s_b = B.out("sums_fwd", 2 * C + 1, 1, torch.float64), B.out("sums_bwd", 2 * C + 1, 1, torch.float64)
    ws, ws_bytes = _workspace(B, capi, "lotus_batchnorm_workspace", 0, C)

    def body():
        capi.call("lotus_batchnorm_stats", x, s_f, 0, C, ws, ws_bytes)
        capi.call("lotus_batchnorm_bwd_stats", dy, x, m, i, gam, bet, s_b, 0, C, row.opts["act"], ws, ws_bytes)

    got = _twice(B, chk, body)
    for n in ("sums_fwd", "sums_bwd"):
        chk.true(not bool(got[n].any()), f"{n} of no rows is all zero")
        chk.rec[n] = float(got[n].abs().max())


# ================================================================================================= AdaNorm
def ada_inputs(counts, C):
    M, Bn = sum(counts), len(counts)
    v = bn_inputs(M, C, dict(act=ne.ACT_GELU), scale=1.5)
    g = torch.Generator().manual_seed(100003 * C + M + 29)
    v["res"], v["add"] = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    v["gamma"], v["beta"] = 1 + 0.2 * torch.randn(1, C, generator=g), 0.2 * torch.randn(1, C, generator=g)
    v["slab"] = 0.5 * torch.randn(Bn, 2 * C + SLAB_EXTRA, generator=g)
    v["x_ln"] = torch.randn(M, C, generator=g) * 2 + 0.5
    if C < 64:
        for k in itertools.count(1):
            bad = v["x_ln"].double().var(1, unbiased=False) < 0.05
            if not bool(bad.any()):
                break
            g2 = torch.Generator().manual_seed(100003 * C + M + 29 + 7919 * k)
            v["x_ln"][bad] = torch.randn(int(bad.sum()), C, generator=g2) * 2 + 0.5
    return v


def _ada_reference(counts, C, v, site):
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    md = v["slab"][:, SLAB_OFF:SLAB_OFF + 2 * C].double().requires_grad_(True)
    gd, bd = v["gamma"].view(-1).double().requires_grad_(True), v["beta"].view(-1).double().requires_grad_(True)
    sh, sc = md[idx][:, :C], md[idx][:, C:]
    if site == "ln":
        xd = v["x_ln"].double().requires_grad_(True)
        y = F.layer_norm(xd, (C,), gd, bd, ne.LN_EPS) * (1 + sc) + sh
        y.backward(v["dy"].double())
        x = v["x_ln"].double()
        return dict(y=y.detach() + v["res"].double(), dx=xd.grad + v["add"].double(), dgamma=gd.grad, dbeta=bd.grad, dmod=md.grad,
                    mean=x.mean(1, keepdim=True), rstd=(x.var(1, unbiased=False, keepdim=True) + ne.LN_EPS).rsqrt())
    xd = v["x"].double().requires_grad_(True)
    rm, rv = v["rm"].view(-1).double().clone(), v["rv"].view(-1).double().clone()
    y = F.gelu(F.batch_norm(xd, rm, rv, gd, bd, True, ne.BN_MOMENTUM, ne.BN_EPS) * (1 + sc) + sh)
    y.backward(v["dy"].double())
    x = v["x"].double()
    gcol = v["gamma"].view(-1).double()
    return dict(y=y.detach(), dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad, dmod=md.grad, mean=x.mean(0), rm=rm, rv=rv,
                invstd=(x.var(0, unbiased=False) + ne.BN_EPS).rsqrt(),
                msg=torch.cat([gcol * bd.grad, gcol * gd.grad, torch.tensor([float(sum(counts))], dtype=torch.float64)]))


def _slab_checks(chk, name, slab, C, counts):
    """Only the norm's slice of the dmod slab is written; the rows of empty clouds are exactly zero."""
    chk.true(bool((slab[:, :SLAB_OFF] == FILL).all()) and bool((slab[:, SLAB_OFF + 2 * C:] == FILL).all()), f"{name}: columns outside the norm's slice were written")
    empty = [b for b, n in enumerate(counts) if n == 0]
    if empty:
        chk.true(not bool(slab[empty, SLAB_OFF:SLAB_OFF + 2 * C].any()), f"{name}: dmod of an empty cloud is not exactly zero")


def _run_ada(row, counters, chk):
    capi = _capi()
    counts, C = list(row.shape), row.C
    M, Bn = sum(counts), len(counts)
    v = ada_inputs(counts, C)
    W = 2 * C + SLAB_EXTRA
    cnt = counters.data_ptr() + capi.query("lotus_bn_counters_offset")
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
    eps, mom, act = ne.BN_EPS, ne.BN_MOMENTUM, ne.ACT_GELU
    B = _Bufs()
    x, xl, dy = B.inp("x", v["x"]), B.inp("x_ln", v["x_ln"]), B.inp("dy", v["dy"])
    res, add = B.inp("res", v["res"]), B.inp("add", v["add"])
    gam, bet = B.inp("gamma", v["gamma"]), B.inp("beta", v["beta"])
    mod = B.inp("slab", v["slab"]) + 4 * SLAB_OFF
    ws, ws_bytes = _workspace(B, capi, "lotus_adanorm_workspace", M, Bn, C)
    bws, bws_bytes = capi.query("lotus_batchnorm_workspace", M, C), None
    B.b["bn_workspace"] = Buf(bws // 4, 1)
    bws, bws_bytes = B.b["bn_workspace"].flat.data_ptr(), bws
    V = lambda n, prior=None: B.out(n, 1, C, prior=prior)  # noqa: E731
    A = lambda n: B.out(n, M, C)  # noqa: E731
    D = lambda n: B.out(n, Bn, W) + 4 * SLAB_OFF  # noqa: E731
    ln_ok = C <= 1024
    if ln_ok:
        ly, lmean, lrstd, ldx, ldg, ldb, ldm = A("ln/y"), B.out("ln/mean", M, 1), B.out("ln/rstd", M, 1), A("ln/dx"), V("ln/dgamma"), V("ln/dbeta"), D("ln/dmod")
    # the BatchNorm site on one GPU ...
    s1 = B.out("bn/sums", 2 * C + 1, 1, torch.float64)
    m1, i1, rm1, rv1 = V("bn/mean"), V("bn/invstd"), V("bn/rm", v["rm"]), V("bn/rv", v["rv"])
    y1, dx1, dg1, db1, dm1 = A("bn/y"), A("bn/dx"), V("bn/dgamma"), V("bn/dbeta"), D("bn/dmod")
    # ... and split: statistics -> message (passed through unchanged: one rank) -> apply
    s2, msg = B.out("split/sums", 2 * C + 1, 1, torch.float64), B.out("split/msg", 2 * C + 1, 1, torch.float64)
    m2, i2, rm2, rv2 = V("split/mean"), V("split/invstd"), V("split/rm", v["rm"]), V("split/rv", v["rv"])
    y2, dx2, dg2, db2, dm2 = A("split/y"), A("split/dx"), V("split/dgamma"), V("split/dbeta"), D("split/dmod")

    def body():
        B.b["workspace"].view.fill_(FILL)
        if ln_ok:
            capi.call("lotus_adaln_fwd", xl, res, gam, bet, mod, W, off, Bn, ly, lmean, lrstd, M, C, ne.LN_EPS)
            capi.call("lotus_adaln_bwd", dy, xl, lmean, lrstd, gam, bet, mod, W, off, Bn, add, ldx, ldg, ldb, ldm, W, M, C, ws, ws_bytes)
        capi.call("lotus_batchnorm_stats_fused", x, s1, m1, i1, rm1, rv1, M, C, eps, mom, bws, bws_bytes, cnt)
        _counters_zero(counters, chk, "lotus_batchnorm_stats_fused")
        capi.call("lotus_adabn_apply", x, m1, i1, gam, bet, mod, W, off, Bn, y1, M, C, act)
        capi.call("lotus_adabn_bwd", dy, x, m1, i1, gam, bet, mod, W, off, Bn, dx1, dg1, db1, dm1, W, M, C, act, 1, ws, ws_bytes)
        capi.call("lotus_batchnorm_stats_fused", x, s2, None, None, None, None, M, C, 0.0, 0.0, bws, bws_bytes, cnt)
        _counters_zero(counters, chk, "lotus_batchnorm_stats_fused (sums)")
        capi.call("lotus_adabn_apply_sums", x, s2, gam, bet, mod, W, off, Bn, y2, m2, i2, rm2, rv2, M, C, act, eps, mom)
        capi.call("lotus_adabn_bwd_stats", dy, x, m2, i2, gam, bet, mod, W, off, Bn, dg2, db2, dm2, W, msg, M, C, act, ws, ws_bytes)
        capi.call("lotus_adabn_bwd_apply_sums", dy, x, m2, i2, gam, bet, mod, W, off, Bn, msg, dx2, M, C, act)

    got = _twice(B, chk, body)
    sl = slice(SLAB_OFF, SLAB_OFF + 2 * C)
    if ln_ok:
        r = _ada_reference(counts, C, v, "ln")
        for n in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
            chk.bar("ln/" + n, _rel(got["ln/" + n], r[n]), ADA_LN)
        chk.bar("ln/dmod", _rel(got["ln/dmod"][:, sl], r["dmod"]), ADA_LN)
        _slab_checks(chk, "ln/dmod", got["ln/dmod"], C, counts)
    else:   # the LayerNorm site refuses the width before anything is launched
        L = capi.lib()
        p = B.b["x"].flat.data_ptr()
        chk.true(L.fn["lotus_adaln_fwd"](p, None, p, p, p, W, off.data_ptr(), Bn, p, None, None, M, C, ne.LN_EPS, None) == -1, "lotus_adaln_fwd takes an unsupported width")
        chk.true(L.fn["lotus_adaln_bwd"](p, p, p, p, p, p, p, W, off.data_ptr(), Bn, None, p, p, p, p, W, M, C, p, 1 << 40, None) == -1, "lotus_adaln_bwd takes an unsupported width")
    r = _ada_reference(counts, C, v, "bn")
    for route in ("bn", "split"):
        for n in ("y", "dx", "dgamma", "dbeta", "mean", "invstd", "rm", "rv"):
            chk.bar(f"{route}/{n}", _rel(got[f"{route}/{n}"], r[n]), ADA_BN)
        chk.bar(f"{route}/dmod", _rel(got[f"{route}/dmod"][:, sl], r["dmod"]), ADA_BN)
        _slab_checks(chk, f"{route}/dmod", got[f"{route}/dmod"], C, counts)
    chk.bar("split/msg", _rel(got["split/msg"], r["msg"]), ADA_BN)
    chk.true(float(got["split/msg"].view(-1)[2 * C]) == float(M), "the backward message carries the row count")
    chk.same("the forward sums of the two routes", got["split/sums"], got["bn/sums"])


def _run_silu(row, counters, chk):
    capi = _capi()
    n = row.shape
    g = torch.Generator().manual_seed(n)
    xv, dyv = (torch.randn(n, 1, generator=g) * 2).clamp(-6, 6), torch.randn(n, 1, generator=g)
    B = _Bufs()
    x, dy = B.inp("x", xv), B.inp("dy", dyv)
    y, dx = B.out("y", n, 1), B.out("dx", n, 1)

    def body():
        capi.call("lotus_ada_silu", x, None, y, n)
        capi.call("lotus_ada_silu", x, dy, dx, n)

    got = _twice(B, chk, body)
    xd = xv.double().requires_grad_(True)
    yr = F.silu(xd)
    yr.backward(dyv.double())
    chk.bar("y", _rel(got["y"], yr.detach()), SILU_BAR)
    chk.bar("dx", _rel(got["dx"], xd.grad), SILU_BAR)


_FAMILY = {"ln": _run_ln, "bn": _run_bn, "bn0": _run_bn0, "ada": _run_ada, "silu": _run_silu}


def run(row, counters):
    """Run `row`.  -> (record {name: error}, failures [text])."""
    chk = _Check(row)
    _FAMILY[row.family](row, counters, chk)
    if not bool((counters == 0).all()):
        chk.fails.append(f"{row.id}: arrival counters left non-zero")
        counters.zero_()
    return chk.rec, chk.fails
