"""Run one row of tests/head_edges.py on the GPU (test infrastructure, not collected): the raw C-ABI calls of csrc/pool_head.hip
into caller-owned buffers with guard rows (dense_run.Buf), twice; the float64 reference; the numpy restatement of the dropout
mask.  Every buffer a call writes is a Buf, every workspace has exactly the queried size (its guard starts at its last byte), two
runs must be bit-equal, every guard intact, no element of any output is skipped.  The input generators and the references run on
the CPU (tests/test_head_args_host.py asserts the input conditions there).

The dropout mask (csrc/common.h: lotus_hash32, lotus_drop_setup, dropout_scale) is restated here in uint32 / uint64 numpy
arithmetic: one hash per pair (2k, 2k + 1), its low half for the even and its high half for the odd element against
t16 = floor(float32(p) 65536); keep scale float32(1 / (1 - t16 / 65536)).  Every mask comparison is against it, bit for bit.

Bars.  eps = 2^-24 (half an ulp of fp32, relative).
  STEP forward      three fp32 roundings (add, slope, keep scale): per element |got - ref| <= 4 eps |ref|; dropped elements exactly 0.
                    The reference takes the slope as the fp32 constant the kernel and torch's fp32 LeakyReLU carry, float32(0.02).
       GELU         gelu_f is not homogeneous: the rounding of pre = base + bias (eps |pre|) passes through |gelu'| <= 1.13, and the
                    fit errs by 1.2e-7 max(1, |gelu|) (stated beside gelu_f): bound (4 eps |ref| + 1.13 eps |pre| + 1.2e-7 max(1, |gelu|)) scale
  STEP dbase        after step k (0-based): (k + 3) eps sum_t |term_t| per element.  GELU: + sum_t |dh_t| scale_t (1.3e-7 + 0.8 eps |pre_t|)
                    (the bound beside gelu_grad_f; |gelu''| <= 0.8 times the rounding of pre)
  STEP dbias        fp32 column sum over M rows: the dense bar 4e-7 sqrt(M) + 1e-6 relative to max(1, |ref|max) (tests/dense_run.py);
                    for M < 64 also M eps sum |term| per element (M - 1 additions and the one rounding of the term; those rows have p = 0)
  MPLOSS            losses 3e-6 relative to max(1, |ref|) (the bar of the published head); gradients 1e-5 relative to |ref|max of each
                    tensor (rtol of test_traj_loss_fn_matches_torch_expression; not max(1, .): they are O(1 / sum mask))
  POSCE             CE per (cloud, axis) 3e-6 relative to max(1, |ref|); dxt 1e-5 per cloud relative to that cloud's |ref|max (exactly
                    zero where the reference is); stats[1] == float32(lse_ref), |stats[1] + stats[3] - lse_ref| <= 2^-40 max(1, |lse_ref|);
                    stats[2] = float32 of a double sum of the targets: one fp32 rounding, 2^-23 relative
  LABELS            'plain' targets and decoded coordinates bit-equal, 'dist' targets within 1.2e-7 ref.max() (tests/test_gpu_labels.py)
  CLOUDMAX          values, arg-max, dx exact; dy + add one correctly rounded fp32 addition (formed in fp32 on the CPU)
  ELEMENTWISE       bit-equal to the fp32 expression with the numpy mask (lotus_drop_path: fl(fl(s branch) + x), the two statements of
                    the kernel; a build that contracted them into one fma would show here)
  bf16 twin         R_STORE = 6e-3 for stored bf16 outputs against the fp32 entry point on the same bf16-exact inputs, relative to
                    |ref|max; integer outputs and fp32 statistics bit-equal

Input conditions (asserted; an offending draw is redrawn from the next seed, no bar is loosened): with LeakyReLU or GELU no
float64 pre-activation base + bias lies within 1e-5 of zero; every trajectory has an active step; rotation bins lie in [0, nrot);
tie rows use eighths; upstream gradients are distinct, nonzero (except the masked entries of `g`), one negative; pos_w, rot_w != 1."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import head_edges as he
from dense_run import FILL, R_STORE, Buf
from norm_run import _Bufs, _Check, _capi, _rel_twin, _twice

EPS = 2.0 ** -24
SLOPE = float(np.float32(0.02))
LOSS_BAR, GRAD_BAR, DIST_BAR = 3e-6, 1e-5, 1.2e-7
POS_W, ROT_W = 1.5, 0.7
G5 = [0.3, -1.1, 0.9, 2.0, 0.6]
NSTEPS = 3


# ================================================================================================= the dropout mask in numpy
def hash32(seed, idx):
    """lotus_hash32(seed, idx) for an array of uint64 indices -> uint32."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = np.uint64(seed)
    m32 = np.uint64(0xFFFFFFFF)
    lo, hi = (idx & m32).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = lo * np.uint32(0x9E3779B1) + np.uint32(seed & m32)
        x = x ^ (hi * np.uint32(0x7FEB352D) + np.uint32(seed >> np.uint64(32)))
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13))
        x = x * np.uint32(0xC2B2AE35)
        x = x ^ (x >> np.uint32(16))
    return x


def drop_setup(p):
    """lotus_drop_setup -> (t16, float32 keep scale)."""
    p = np.float32(p)
    if not p > 0:
        return 0, np.float32(1.0)
    t16 = min(max(int(float(p) * 65536.0), 1), 65535)
    return t16, np.float32(1.0 / (1.0 - t16 / 65536.0))


def keep_scale(seed, idx, p):
    """dropout_scale(seed, idx) for an array of element indices -> float32 (0 or the keep scale)."""
    idx = np.asarray(idx, dtype=np.uint64)
    t16, inv = drop_setup(p)
    if t16 == 0:
        return np.ones(idx.shape, np.float32)
    h = hash32(seed, idx >> np.uint64(1))
    half = np.where((idx & np.uint64(1)).astype(bool), h >> np.uint32(16), h & np.uint32(0xFFFF))
    return np.where(half >= np.uint32(t16), inv, np.float32(0.0)).astype(np.float32)


def _scale_t(seed, n, p, shape=None):
    s = torch.from_numpy(keep_scale(seed, np.arange(n, dtype=np.uint64), p))
    return s.view(shape) if shape else s


def step_seed(M, C, t):
    return ((0x01234567 + t) << 32) | ((0xC0FFEE00 + 977 * t + 131 * M + C) & 0xFFFFFFFF)


# ================================================================================================= helpers
def _act64(v, act):
    return F.gelu(v) if act == he.ACT_GELU else (torch.where(v > 0, v, v * SLOPE) if act == he.ACT_LEAKY else v)


def _act_grad64(v, act):
    if act == he.ACT_NONE:
        return torch.ones_like(v)
    if act == he.ACT_LEAKY:
        return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, SLOPE))
    p = v.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(p).sum(), p)
    return g


def _bound(chk, name, got, ref, bound):
    """Every element within its own bound: records max |got - ref| / bound (elements with a zero bound must be equal)."""
    d = (got.double().cpu().reshape(ref.shape) - ref).abs()
    if d.numel() == 0:
        chk.rec[name] = 0.0
        return
    zero = bound == 0
    chk.true(bool((d[zero] == 0).all()), f"{name}: elements whose reference is exactly zero differ")
    ratio = float((d[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    chk.bar(name, ratio, 1.0)


def _relmax(got, ref):
    """|got - ref|max relative to |ref|max (absolute where the reference is identically zero)."""
    if ref.numel() == 0:
        return 0.0
    d, s = float((got.double().cpu().reshape(ref.shape) - ref).abs().max()), float(ref.abs().max())
    return d / s if s > 0 else d


def _ws(bufs, nbytes, name="workspace"):
    assert nbytes % 4 == 0 and nbytes > 0
    bufs.b[name] = Buf(nbytes // 4, 1)            # exactly the queried size: the guard starts at its last byte
    return bufs.b[name].flat.data_ptr()


def _twin(fn):
    capi = _capi()
    prev, capi.BF16 = capi.BF16, True
    try:
        return fn()
    finally:
        capi.BF16 = prev


def _offsets(counts):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    batch = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return off, batch


# ================================================================================================= STEP
def step_inputs(row):
    """-> base [M, C], bias [3, C], dh [3, M, C] (float32, CPU).  The shape alone seeds them."""
    (M, C), act = row.shape, row.opts["act"]
    seed = 100003 * C + M
    g = torch.Generator().manual_seed(seed)
    rnd = (lambda t: t.bfloat16().float()) if row.opts.get("b16") else (lambda t: t)
    base, bias, dh = rnd(torch.randn(M, C, generator=g)), torch.randn(NSTEPS, C, generator=g), rnd(torch.randn(NSTEPS, M, C, generator=g))
    if row.group == "stepid":
        bias.zero_()
    near = lambda: ((base.double()[None] + bias.double()[:, None, :]).abs() < 1e-5).any(0)  # noqa: E731
    if act != he.ACT_NONE and M:
        for k in itertools.count(1):
            bad = near()
            if not bool(bad.any()):
                break
            g2 = torch.Generator().manual_seed(seed + 7919 * k)
            base[bad] = rnd(torch.randn(int(bad.sum()), generator=g2))
        assert not bool(near().any())
    return base, bias, dh


def _step_pass(row, v, b16, chk):
    capi = _capi()
    (M, C), act, p = row.shape, row.opts["act"], row.opts["p"]
    base, bias, dh = v
    adt = torch.bfloat16 if b16 else torch.float32
    B = _Bufs()
    pb = B.inp("base", base, adt)
    pbias = [B.inp(f"bias{t}", bias[t:t + 1]) for t in range(NSTEPS)]
    pdh = [B.inp(f"dh{t}", dh[t], adt) for t in range(NSTEPS)]
    out = [B.out(f"out{t}", M, C, adt) for t in range(NSTEPS)]
    dbase = B.out("dbase", M, C, adt)
    dbias = [B.out(f"dbias{t}", 1, C) for t in range(NSTEPS)]
    for t in range(NSTEPS - 1):
        B.out(f"dbase_after{t}", M, C, adt)
    nbytes = capi.query("lotus_step_act_bwd_workspace", M, C)
    ws = _ws(B, nbytes)

    def body():
        B.b["workspace"].view.fill_(FILL)
        for t in range(NSTEPS):
            capi.call("lotus_step_act_fwd", pb, pbias[t], out[t], M, C, act, p, step_seed(M, C, t))
        for t in range(NSTEPS):
            capi.call("lotus_step_act_bwd", pdh[t], pb, pbias[t], dbase, dbias[t], M, C, act, p, step_seed(M, C, t), 1 if t else 0, ws, nbytes)
            if t < NSTEPS - 1:
                B.b[f"dbase_after{t}"].view.copy_(B.b["dbase"].view)

    got = _twice(B, chk, body)
    got[f"dbase_after{NSTEPS - 1}"] = got["dbase"]
    return got


def _run_step(row, chk):
    (M, C), act, p = row.shape, row.opts["act"], row.opts["p"]
    v = step_inputs(row)
    base, bias, dh = v
    got = _step_pass(row, v, False, chk)
    b64 = base.double()
    acc = torch.zeros(M, C, dtype=torch.float64)
    acc_abs, extra = torch.zeros_like(acc), torch.zeros_like(acc)
    for t in range(NSTEPS):
        pre = b64 + bias[t].double()
        sc = _scale_t(step_seed(M, C, t), M * C, p, (M, C)).double()
        ref = _act64(pre, act) * sc
        bound = 4 * EPS * ref.abs()
        if act == he.ACT_GELU:
            bound = (bound + 1.13 * EPS * pre.abs() + 1.2e-7 * F.gelu(pre).abs().clamp_min(1.0)) * sc
        _bound(chk, f"out{t}", got[f"out{t}"], ref, bound)
        if p > 0:
            chk.true(bool((got[f"out{t}"].cpu()[sc == 0] == 0).all()), f"out{t}: a dropped element is not exactly zero")
            share = float((sc == 0).double().mean())
            chk.true(abs(share - drop_setup(p)[0] / 65536.0) < 5 * (p * (1 - p) / (M * C)) ** 0.5 + 1e-9, f"out{t}: the mask drops {share:.4f} of the elements")
        term = dh[t].double() * _act_grad64(pre, act) * sc
        acc, acc_abs = acc + term, acc_abs + term.abs()
        if act == he.ACT_GELU:
            extra = extra + dh[t].double().abs() * sc * (1.3e-7 + 0.8 * EPS * pre.abs())
        _bound(chk, f"dbase_after{t}", got[f"dbase_after{t}"], acc, (t + 3) * EPS * acc_abs + extra)
        col, col_abs = term.sum(0, keepdim=True), term.abs().sum(0, keepdim=True)
        e = float((got[f"dbias{t}"].double().cpu() - col).abs().max()) / max(1.0, float(col.abs().max()))
        chk.bar(f"dbias{t}", e, 4e-7 * M ** 0.5 + 1e-6)
        if M < he.SA_ROWS:
            _bound(chk, f"dbias{t}/elementwise", got[f"dbias{t}"], col, M * EPS * col_abs)
    if row.opts.get("b16"):
        twin = _twin(lambda: _step_pass(row, v, True, chk))
        chk.true(twin["out0"].dtype == torch.bfloat16 and twin["dbase"].dtype == torch.bfloat16, "the twin's activations are bf16")
        for name in [f"out{t}" for t in range(NSTEPS)] + ["dbase_after0", "dbase"]:
            chk.bar("b16/" + name, _rel_twin(twin[name], got[name]), R_STORE)
        for t in range(NSTEPS):
            chk.same(f"dbias{t} of the bf16 twin and the fp32 entry point", twin[f"dbias{t}"], got[f"dbias{t}"])


def _run_step0(row, chk):
    """No rows: the forward returns at once, the backward zeroes dbias; out and dbase (no rows of their own) stay untouched."""
    capi = _capi()
    (M, C), act = row.shape, row.opts["act"]
    z = torch.zeros(0, C)
    B = _Bufs()
    pb, pdh, pbias = B.inp("base", z), B.inp("dh", z), B.inp("bias", torch.ones(1, C))
    out, dbase, dbias = B.out("out", 0, C), B.out("dbase", 0, C), B.out("dbias", 1, C)
    nbytes = capi.query("lotus_step_act_bwd_workspace", 0, C)
    ws = _ws(B, nbytes)

    def body():
        capi.call("lotus_step_act_fwd", pb, pbias, out, 0, C, act, 0.1, 7)
        capi.call("lotus_step_act_bwd", pdh, pb, pbias, dbase, dbias, 0, C, act, 0.1, 7, 0, ws, nbytes)
        capi.call("lotus_step_act_bwd", pdh, pb, pbias, dbase, dbias, 0, C, act, 0.1, 7, 1, ws, nbytes)

    got = _twice(B, chk, body)
    chk.true(not bool(got["dbias"].any()), "dbias of no rows is not zero")
    chk.true(bool((B.b["workspace"].view == FILL).all()), "the workspace of no rows was written")
    chk.rec["dbias"] = float(got["dbias"].abs().max())


def _run_stepid(row, chk):
    capi = _capi()
    (M, C), p = row.shape, row.opts["p"]
    base, bias, _ = step_inputs(row)
    seed = step_seed(M, C, 0)
    B = _Bufs()
    pb, pbias = B.inp("base", base), B.inp("bias", bias[0:1])
    o1, o2 = B.out("step_act", M, C), B.out("dropout", M, C)

    def body():
        capi.call("lotus_step_act_fwd", pb, pbias, o1, M, C, he.ACT_NONE, p, seed)
        capi.call("lotus_dropout", pb, o2, M * C, p, seed)

    got = _twice(B, chk, body)
    want = base * _scale_t(seed, M * C, p, (M, C))
    chk.same("lotus_step_act_fwd (bias 0, no activation) and lotus_dropout", got["step_act"], got["dropout"])
    chk.same("lotus_dropout and x times the numpy mask", got["dropout"].cpu(), want)
    chk.rec["dropped"] = float((want == 0).float().mean())


# ================================================================================================= MPLOSS
def mp_inputs(row):
    (Bn, T, nrot, ga), o = row.shape, row.opts
    R, W = Bn * T, nrot * 3 + 2
    g = torch.Generator().manual_seed(7 + 1009 * Bn + 31 * T + nrot + ga)
    ae = torch.randn(R, W, generator=g) * o.get("scale", 1.0)
    if o.get("b16"):
        ae = ae.bfloat16().float()
    ce = torch.rand(R, 3, generator=g) * 5
    gt = torch.randn(R, ga, generator=g)
    gt[:, 3:6] = torch.randint(0, nrot, (R, 3), generator=g).float()
    gt[:, ga - 1] = torch.randint(0, 2, (R,), generator=g).float()
    stop = torch.randint(0, 2, (R,), generator=g).float()
    steps = torch.arange(T)[None]
    if o["mask"] == "prefix":
        lens = 1 + (torch.arange(Bn) * 3) % T
        lens[0] = T
        lens[-1] = 1 if Bn > 1 else T
        mask = (steps < lens[:, None]).float()
    elif o["mask"] == "step0":
        mask = (steps == 0).float().expand(Bn, T).contiguous()
    else:
        mask = (torch.rand(Bn, T, generator=g) < 0.5).float()
        mask[torch.arange(Bn), torch.arange(Bn) % T] = 1.0
        mask[0] = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])[:T]
    assert bool((mask.sum(1) >= 1).all()), "every trajectory has an active step"
    assert bool(((gt[:, 3:6] >= 0) & (gt[:, 3:6] < nrot) & (gt[:, 3:6] == gt[:, 3:6].floor())).all())
    return dict(ae=ae, ce=ce, gt=gt, stop=stop.view(R, 1), mask=mask.reshape(R, 1))


def mp_reference(row, v):
    (Bn, T, nrot, ga) = row.shape
    ae, ce = v["ae"].double().requires_grad_(True), v["ce"].double().requires_grad_(True)
    gt, stop, m = v["gt"].double(), v["stop"].double().view(Bn, T), v["mask"].double().view(Bn, T)
    a3 = ae.view(Bn, T, -1)
    rot_logits = a3[..., :nrot * 3].reshape(Bn, T, nrot, 3)
    msum = m.sum()
    pos = ((ce.view(Bn, T, 3).sum(-1) * m).sum(1) / (3.0 * m.sum(1))).sum() / Bn
    rl = F.cross_entropy(rot_logits.permute(0, 1, 3, 2).reshape(-1, nrot), gt[:, 3:6].long().reshape(-1), reduction="none").view(Bn, T, 3)
    rot = (rl * m.unsqueeze(-1)).sum() / msum / 3
    opn = (F.binary_cross_entropy_with_logits(a3[..., -2], gt[:, ga - 1].view(Bn, T), reduction="none") * m).sum() / msum
    stp = (F.binary_cross_entropy_with_logits(a3[..., -1], stop, reduction="none") * m).sum() / msum
    losses = torch.stack([pos, rot, opn, stp, POS_W * pos + ROT_W * rot + opn + stp])
    dae, = torch.autograd.grad(rot + opn + stp, ae, retain_graph=True)       # disjoint columns: each its own loss
    dce, = torch.autograd.grad(pos, ce, retain_graph=True)
    dae_out, dce_out = torch.autograd.grad((losses * torch.tensor(G5, dtype=torch.float64)).sum(), [ae, ce])
    return dict(losses=losses.detach().view(5, 1), dae=dae, dce=dce, dae_out=dae_out, dce_out=dce_out)


def _mp_pass(row, v, b16, chk):
    capi = _capi()
    (Bn, T, nrot, ga) = row.shape
    R, W = Bn * T, nrot * 3 + 2
    adt = torch.bfloat16 if b16 else torch.float32
    B = _Bufs()
    ae, gt, stop, mask, ce = B.inp("ae", v["ae"], adt), B.inp("gt", v["gt"]), B.inp("stop", v["stop"]), B.inp("mask", v["mask"]), B.inp("ce", v["ce"])
    g = B.inp("g", torch.tensor(G5).view(5, 1))
    losses, dae, dce = B.out("losses", 5, 1), B.out("dae", R, W), B.out("dce", R, 3)
    dae_out, dce_out = B.out("dae_out", R, W, adt), B.out("dce_out", R, 3)

    def body():
        capi.call("lotus_mp_loss_fwd", ae, gt, stop, mask, ce, Bn, T, nrot, ga, POS_W, ROT_W, losses, dae, dce)
        capi.call("lotus_mp_loss_bwd", dae, dce, g, POS_W, ROT_W, Bn, T, nrot, dae_out, dce_out)

    return _twice(B, chk, body)


def _run_mploss(row, chk):
    v = mp_inputs(row)
    got = _mp_pass(row, v, False, chk)
    ref = mp_reference(row, v)
    for k, name in enumerate(("pos", "rot", "open", "stop", "total")):
        r = float(ref["losses"][k])
        chk.bar("loss/" + name, abs(float(got["losses"][k]) - r) / max(1.0, abs(r)), LOSS_BAR)
    for name in ("dae", "dce", "dae_out", "dce_out"):
        chk.true(bool(torch.isfinite(got[name]).all()), f"{name} is not finite")
        chk.bar(name, _relmax(got[name], ref[name]), GRAD_BAR)
    chk.true(bool(torch.isfinite(got["losses"]).all()), "a loss is not finite")
    if row.opts.get("b16"):
        twin = _twin(lambda: _mp_pass(row, v, True, chk))
        chk.true(twin["dae_out"].dtype == torch.bfloat16, "the twin's dae_out is bf16")
        chk.bar("b16/dae_out", _rel_twin(twin["dae_out"], got["dae_out"]), R_STORE)
        for name in ("losses", "dae", "dce", "dce_out"):
            chk.same(f"{name} of the bf16 twin and the fp32 entry point", twin[name], got[name])


# ================================================================================================= POSCE
def posce_g(Bn):
    """Upstream weights per (cloud, axis): distinct, both signs; zeros for a masked step (a whole cloud when there are several)."""
    g = torch.tensor([(-1.0) ** i * (0.3 + 0.17 * i) for i in range(Bn * 3)])
    if Bn > 1:
        g[3:6] = 0.0
    g[Bn * 3 - 1] = 0.0
    assert bool((g < 0).any()) and len(set(g[g != 0].tolist())) == int((g != 0).sum())
    return g


def posce_inputs(row):
    counts, nb, o = list(row.shape), row.opts["nb"], row.opts
    n = sum(counts)
    g = torch.Generator().manual_seed(11 + 257 * n + nb)
    xt = torch.randn(n, 3 * nb, generator=g) * o["scale"]
    tg = []
    for b, nn in enumerate(counts):
        if o["tgt"] == "onehot":
            t = torch.zeros(3, nn * nb)
            t[torch.arange(3), torch.randint(0, nn * nb, (3,), generator=g)] = 1.0
        else:
            t = torch.softmax(torch.randn(3, nn * nb, generator=g).double() * 2, -1).float()
        if o["tgt"] == "zero" and b == len(counts) - 2:
            t[1] = 0.0
        tg.append(t.reshape(-1))
    return xt, torch.cat(tg), posce_g(len(counts))


def posce_reference(row, xt, tgt, g):
    counts, nb = list(row.shape), row.opts["nb"]
    x64, o, r0 = xt.double(), 0, 0
    ce, lse, tsum, dxt = [], [], [], torch.zeros_like(x64)
    for b, nn in enumerate(counts):
        t3 = tgt[o:o + 3 * nn * nb].double().view(3, nn * nb)
        for c in range(3):
            x = x64[r0:r0 + nn, c * nb:(c + 1) * nb].reshape(-1)
            l, ts = torch.logsumexp(x, 0), t3[c].sum()
            ce.append(l * ts - (t3[c] * x).sum())
            lse.append(l)
            tsum.append(ts)
            dxt[r0:r0 + nn, c * nb:(c + 1) * nb] = (g[b * 3 + c].double() * (torch.exp(x - l) * ts - t3[c])).view(nn, nb)
        o, r0 = o + 3 * nn * nb, r0 + nn
    return torch.stack(ce), torch.stack(lse), torch.stack(tsum), dxt


def _run_posce(row, chk):
    capi = _capi()
    counts, nb = list(row.shape), row.opts["nb"]
    Bn, n = len(counts), sum(counts)
    xt, tgt, g = posce_inputs(row)
    off, batch = _offsets(counts)
    off_d, batch_d = torch.from_numpy(off).cuda(), torch.from_numpy(batch).cuda()
    B = _Bufs()
    px, pt, pg = B.inp("xt", xt), B.inp("tgt", tgt.view(-1, 1)), B.inp("g", g.view(-1, 1))
    nst = capi.query("lotus_loss_stats_floats", Bn)
    # (held as int32: the slice partials behind the statistics are doubles, whose halves read as floats can be NaN patterns,
    #  and the two runs are compared bit for bit)
    stats, dxt = B.out("stats", nst, 1, torch.int32), B.out("dxt", n, 3 * nb)

    def body():
        capi.call("lotus_pos_ce_fwd", px, pt, off_d, Bn, nb, stats)
        capi.call("lotus_pos_ce_bwd", px, pt, off_d, batch_d, stats, pg, Bn, n, nb, dxt)

    got = _twice(B, chk, body)
    ce, lse, tsum, dref = posce_reference(row, xt, tgt, g)
    st = got["stats"].cpu().view(-1)[:Bn * 12].view(torch.float32).view(Bn * 3, 4).double()
    chk.true(bool(torch.isfinite(st).all()) and bool(torch.isfinite(got["dxt"]).all()), "a statistic or a gradient is not finite")
    chk.bar("ce", float(((st[:, 0] - ce).abs() / ce.abs().clamp_min(1.0)).max()), LOSS_BAR)
    chk.true(bool((st[:, 1] == lse.float().double()).all()), "stats[1] is not float32(lse) of the float64 reference")
    chk.bar("lse_split", float(((st[:, 1] + st[:, 3] - lse).abs() / lse.abs().clamp_min(1.0)).max()), 2.0 ** -40)
    chk.bar("tsum", float(((st[:, 2] - tsum).abs() / torch.where(tsum > 0, tsum, torch.ones_like(tsum))).max()), 2.0 ** -23)
    zero = tsum == 0
    if bool(zero.any()):
        chk.true(bool((st[zero, 0] == 0).all()), "the loss of an axis without target mass is not exactly 0")
    errs, r0 = [], 0
    gd = got["dxt"].double().cpu()
    for b, nn in enumerate(counts):
        r, d = dref[r0:r0 + nn], (gd[r0:r0 + nn] - dref[r0:r0 + nn]).abs()
        s = float(r.abs().max())
        errs.append(float(d.max()) / s if s > 0 else float(d.max()))
        for c in range(3):          # a zero weight or an empty target: exactly zero
            if float(g[b * 3 + c]) == 0.0 or bool(zero[b * 3 + c]):
                chk.true(not bool(gd[r0:r0 + nn, c * nb:(c + 1) * nb].any()), f"dxt of cloud {b} axis {c} is not exactly zero")
        r0 += nn
    chk.rec["dxt_per_cloud"] = [[int(c), e] for c, e in zip(counts, errs)]
    chk.bar("dxt", max(errs), GRAD_BAR)


# ================================================================================================= LABELS
def label_inputs(row):
    """-> pc [n, ld], gt [B, 7], robot (uint8 [n] or None), bin size, xyz per cloud."""
    counts, o = list(row.shape), row.opts
    nb, ld = o["nb"], o["ld"]
    n, Bn = sum(counts), len(counts)
    rng = np.random.default_rng(5 + 131 * n + nb + ld)
    pc = rng.normal(size=(n, ld)).astype(np.float32)
    gt = rng.normal(size=(Bn, 7)).astype(np.float32)
    off, _ = _offsets(counts)
    bin_size = 0.01
    if o.get("ties"):
        bin_size = 0.25
        pc[:, :3] = (64.0 + 0.125 * np.arange(n, dtype=np.float32))[:, None] + np.float32([0.0, 64.0, 128.0])[None]
        pc[off[0]:off[1], :3] = 0.0                                    # the short cloud: ten nearest candidates, in slices that are mostly empty
        for c, sites in enumerate(he.tie_sites(counts[1], nb)):
            for p, _ in sites:
                pc[off[1] + p, c] = 0.0
        gt[:, :3] = 0.125                                              # midway between two candidates of every point at 0
        assert bool((pc[:, :3] * 8 == np.round(pc[:, :3] * 8)).all()) and bool((gt[:, :3] * 8 == np.round(gt[:, :3] * 8)).all())
    else:
        pc[:, :3] = (pc[:, :3] * 0.1).astype(np.float32)
        for b in range(Bn):
            k = off[b] + int(rng.integers(counts[b]))
            gt[b, :3] = pc[k, :3] + rng.uniform(-0.02, 0.02, 3).astype(np.float32)
        if o.get("far"):
            gt[Bn // 2, :3] += 3.0
    robot = None
    if o.get("robot") == "seventh":
        robot = np.zeros(n, np.uint8)
        robot[rng.choice(n, max(n // 7, 1), replace=False)] = 1
    elif o.get("robot") == "cloud":
        robot = np.zeros(n, np.uint8)
        robot[rng.choice(n, n // 7, replace=False)] = 1
        robot[off[3]:off[4]] = 1
    xyz = [np.ascontiguousarray(pc[off[b]:off[b + 1], :3]) for b in range(Bn)]
    return pc, gt, robot, bin_size, xyz


def dec_logits(row):
    """Logits [n, 3 nb] of a decode row (CPU float32)."""
    counts, o = list(row.shape), row.opts
    nb, n = o["nb"], sum(counts)
    off, _ = _offsets(counts)
    g = torch.Generator().manual_seed(3 + 17 * n + nb)
    if o["mode"] == "random":
        xt = torch.randn(n, 3 * nb, generator=g)
        return xt.bfloat16().float() if o.get("b16") else xt
    xt = (torch.randint(-8, 4, (n, 3 * nb), generator=g).float() / 4).view(n, 3, nb)   # quarters, at most 0.75
    for b in range(len(counts)):
        a, e = int(off[b]), int(off[b + 1])
        if o["mode"] == "last":
            xt[e - 1, :, nb - 1] = 1.0
        elif o["mode"] == "first":
            xt[a, :, 0] = 1.0
        elif counts[b] >= 300:
            for c, sites in enumerate(he.tie_sites(counts[b], nb)):
                for p, j in sites:
                    xt[a + p, c, j] = 1.0
        else:
            xt[a:e] = 1.0                                              # a short cloud: every logit ties
    return xt.view(n, 3 * nb).contiguous()


def _run_tgt(row, chk):
    from oracle import labels as ol

    capi = _capi()
    counts, o = list(row.shape), row.opts
    nb, ld, kind = o["nb"], o["ld"], o["kind"]
    n, Bn = sum(counts), len(counts)
    pc, gt, robot, bin_size, xyz = label_inputs(row)
    off, batch = _offsets(counts)
    off_d, batch_d = torch.from_numpy(off).cuda(), torch.from_numpy(batch).cuda()
    rob_d = torch.from_numpy(robot).cuda() if robot is not None else None
    B = _Bufs()
    ppc, pgt = B.inp("pc", torch.from_numpy(pc)), B.inp("gt", torch.from_numpy(gt))
    tgt = B.out("tgt", 3 * nb * n, 1)
    nbytes = capi.query("lotus_pos_workspace", Bn)
    ws = _ws(B, nbytes)

    def body():
        B.b["workspace"].view.fill_(FILL)
        capi.call("lotus_pos_targets", ppc, ld, off_d, batch_d, pgt, 7, rob_d, Bn, n, nb, bin_size, 0 if kind == "plain" else 1, tgt, ws, nbytes)

    got = _twice(B, chk, body)["tgt"].cpu().numpy().reshape(-1)
    worst, pos, onehot = 0.0, 0, 0
    for b, nn in enumerate(counts):
        idx = np.nonzero(robot[off[b]:off[b + 1]])[0] if robot is not None else None
        ref = ol.disc_gt_pos_prob(xyz[b], gt[b, :3], bin_size, nb // 2, kind, idx)
        mine = got[pos:pos + 3 * nn * nb].reshape(3, nn * nb)
        pos += 3 * nn * nb
        onehot += int((ref.max(-1) == 1.0).sum())
        if kind == "plain":
            chk.true(np.array_equal(mine, ref), f"cloud {b}: 'plain' targets differ from the oracle")
        e = float(np.abs(mine.astype(np.float64) - ref).max() / ref.max())
        worst = max(worst, e)
    chk.bar("tgt", worst, DIST_BAR if kind == "dist" else 0.0)
    chk.rec["onehot_axes"] = onehot
    if o.get("far") or o.get("ties") or o.get("robot") == "cloud":
        chk.true(onehot >= 3, "the row has no axis that falls back to the nearest candidate")


def _dec_pass(row, xt, pc, off_d, bin_size, b16, chk):
    capi = _capi()
    counts, nb, ld = list(row.shape), row.opts["nb"], row.opts["ld"]
    Bn = len(counts)
    B = _Bufs()
    px, ppc = B.inp("xt", xt, torch.bfloat16 if b16 else torch.float32), B.inp("pc", torch.from_numpy(pc))
    best = B.out("best", Bn * 3, 1, torch.float64)
    nbytes = capi.query("lotus_pos_workspace", Bn)
    ws = _ws(B, nbytes)

    def body():
        B.b["workspace"].view.fill_(FILL)
        capi.call("lotus_pos_decode_max", px, ppc, ld, off_d, Bn, nb, bin_size, best, ws, nbytes)

    return _twice(B, chk, body)["best"].cpu().numpy().reshape(Bn, 3)


def _run_dec(row, chk):
    from oracle import labels as ol

    counts, nb = list(row.shape), row.opts["nb"]
    pc, _, _, bin_size, xyz = label_inputs(row)
    xt = dec_logits(row)
    off, _ = _offsets(counts)
    off_d = torch.from_numpy(off).cuda()
    got = _dec_pass(row, xt, pc, off_d, bin_size, False, chk)
    for b, nn in enumerate(counts):
        lg = xt[off[b]:off[b + 1]].view(nn, 3, nb).permute(1, 0, 2).reshape(3, -1).numpy()
        ref = ol.best_pos_max(lg, xyz[b], bin_size, nb // 2)
        chk.true(np.array_equal(got[b], ref), f"cloud {b}: decoded {got[b]} for {ref}")
        if row.opts["mode"] in ("ties", "first", "last"):
            chk.true(all(int((lg[c] == lg[c].max()).sum()) >= (2 if row.opts["mode"] == "ties" else 1) for c in range(3)), "the row holds no tie")
    chk.rec["decoded"] = len(counts) * 3
    if row.opts.get("b16"):
        twin = _twin(lambda: _dec_pass(row, xt, pc, off_d, bin_size, True, chk))
        chk.true(np.array_equal(twin, got), "the bf16 twin decodes other coordinates")


# ================================================================================================= CLOUDMAX
def cloudmax_inputs(row):
    """x [n, C] in quarters: column 0 tied over every row, the maximum of column 1 only in the last row of each cloud, column 2
    tied in rows of different splits, column 3 tied in rows of different lanes of one split (where the cloud has such rows)."""
    counts, C = list(row.shape), row.opts["C"]
    n = sum(counts)
    off, _ = _offsets(counts)
    g = torch.Generator().manual_seed(13 + C)
    x = torch.randint(-12, 9, (n, C), generator=g).float() / 4          # at most 2.0, many natural ties
    x[:, 0] = 0.5
    for b, nn in enumerate(counts):
        a = int(off[b])
        x[a + nn - 1, 1] = 3.0
        chunk = -(-nn // he.CM_SPLITS)
        if nn > chunk:                                                  # rows of two different splits
            x[a + nn - 1, 2] = x[a + chunk - 1, 2] = 3.0
            if nn > 2 * chunk:
                x[a + 2 * chunk, 2] = 3.0
        if chunk >= 2:                                                  # two row lanes of split 1 (or 0)
            s = chunk if nn >= 2 * chunk else 0
            x[a + s + 1, 3] = x[a + s, 3] = 3.0
            if chunk > 32:
                x[a + s + 32, 3] = 3.0                                  # ... and the second step of the first lane
    dy, add = torch.randn(len(counts), C, generator=g), torch.randn(n, C, generator=g)
    if row.opts.get("b16"):
        dy, add = dy.bfloat16().float(), add.bfloat16().float()
    return x, dy, add


def _cm_pass(row, v, b16, chk):
    capi = _capi()
    counts, C = list(row.shape), row.opts["C"]
    Bn, n = len(counts), sum(counts)
    x, dy, add = v
    adt = torch.bfloat16 if b16 else torch.float32
    off, batch = _offsets(counts)
    off_d, batch_d = torch.from_numpy(off).cuda(), torch.from_numpy(batch).cuda()
    B = _Bufs()
    px, pdy, padd = B.inp("x", x, adt), B.inp("dy", dy, adt), B.inp("add", add, adt)
    y, arg = B.out("y", Bn, C, adt), B.out("arg", Bn, C, torch.int32)
    dx, dxa = B.out("dx", n, C, adt), B.out("dx_add", n, C, adt)
    nbytes = capi.query("lotus_cloud_max_workspace", Bn, C)
    ws = _ws(B, nbytes)

    def body():
        B.b["workspace"].view.fill_(FILL)
        capi.call("lotus_cloud_max_fwd", px, off_d, Bn, C, y, arg, ws, nbytes)
        capi.call("lotus_cloud_max_bwd", pdy, arg, batch_d, n, C, None, dx)
        capi.call("lotus_cloud_max_bwd", pdy, arg, batch_d, n, C, padd, dxa)

    return _twice(B, chk, body)


def _run_cloudmax(row, chk):
    counts, C = list(row.shape), row.opts["C"]
    v = cloudmax_inputs(row)
    x, dy, add = v
    got = _cm_pass(row, v, False, chk)
    off, _ = _offsets(counts)
    xn = x.numpy().astype(np.float64)
    dx = torch.zeros_like(x)
    ymax, arg = np.zeros((len(counts), C)), np.zeros((len(counts), C), np.int64)
    for b, nn in enumerate(counts):
        seg = xn[off[b]:off[b + 1]]
        arg[b] = seg.argmax(0) + off[b]                                 # numpy: the first row attaining the maximum
        ymax[b] = seg.max(0)
        dx[torch.from_numpy(arg[b]), torch.arange(C)] = dy[b]
    chk.true(np.array_equal(got["y"].cpu().numpy().astype(np.float64), ymax), "the maxima differ")
    chk.true(np.array_equal(got["arg"].cpu().numpy().astype(np.int64), arg), "the arg-max is not the first row attaining the maximum")
    chk.same("dx", got["dx"].cpu(), dx)
    chk.same("dx + add (one fp32 addition)", got["dx_add"].cpu(), dx + add)
    ties = int(sum(((xn[off[b]:off[b + 1]] == ymax[b][None]).sum(0) > 1).sum() for b in range(len(counts))))
    chk.rec["tied_columns"] = ties
    chk.true(ties >= len(counts) - 1, "the row holds too few tied maxima")
    if row.opts.get("b16"):
        twin = _twin(lambda: _cm_pass(row, v, True, chk))
        chk.true(twin["y"].dtype == torch.bfloat16, "the twin's activations are bf16")
        chk.same("y of the bf16 twin (quarters are exact in bf16)", twin["y"].float(), got["y"])
        chk.same("arg of the bf16 twin", twin["arg"], got["arg"])
        chk.same("dx of the bf16 twin (bf16-exact dy)", twin["dx"].float(), got["dx"])
        chk.bar("b16/dx_add", _rel_twin(twin["dx_add"], got["dx_add"]), R_STORE)


# ================================================================================================= ELEMENTWISE
def _run_dropout(row, chk):
    capi = _capi()
    n, p = row.shape, row.opts["p"]
    seed = (0x0BADC0DE << 32) | (n & 0xFFFFFFFF)
    x = torch.randn(n, 1, generator=torch.Generator().manual_seed(n))
    B = _Bufs()
    px, y = B.inp("x", x), B.out("y", n, 1)
    got = _twice(B, chk, lambda: capi.call("lotus_dropout", px, y, n, p, seed))
    sc = _scale_t(seed, n, p, (n, 1))
    chk.same("y and x times the numpy mask", got["y"].cpu(), x * sc)
    chk.rec["dropped"] = float((sc == 0).float().mean())
    if p == 0:
        chk.true(bool((sc == 1).all()), "p = 0 keeps everything with scale 1")


def _run_add(row, chk):
    capi = _capi()
    n = row.shape
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, 1, generator=g), torch.randn(n, 1, generator=g)
    B = _Bufs()
    pa, pb, y = B.inp("a", a), B.inp("b", b), B.out("y", n, 1)
    got = _twice(B, chk, lambda: capi.call("lotus_add", pa, pb, y, n))
    chk.same("y and a + b", got["y"].cpu(), a + b)
    chk.rec["n"] = n


def _run_droppath(row, chk):
    capi = _capi()
    (M, C), p, with_x = row.shape, row.opts["p"], row.opts["x"]
    seed = (0x00C0FFEE << 32) | (M * 4099 + C)
    g = torch.Generator().manual_seed(M + C)
    br, x = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    B = _Bufs()
    pbr, px, y = B.inp("branch", br), (B.inp("x", x) if with_x else None), B.out("y", M, C)
    got = _twice(B, chk, lambda: capi.call("lotus_drop_path", pbr, px, y, M, C, p, seed))["y"].cpu()
    s = _scale_t(seed, M, p, (M, 1))
    rows_kept = (got != 0).any(1) if not with_x else None
    if with_x:
        chk.same("y and x + fl(s branch) with the row's numpy mask", got, br * s + x)      # two roundings, as the kernel states them
        chk.same("dropped rows return x", got[(s == 0).view(-1)], x[(s == 0).view(-1)])
    else:
        chk.same("y and branch times the row's numpy mask", got, br * s)
        chk.true(bool((rows_kept == (s != 0).view(-1)).all()), "the row decisions differ from the numpy mask at index = row")
    chk.rec["rows_dropped"] = float((s == 0).float().mean())
    if p == 0:
        chk.true(bool((s == 1).all()), "p = 0 keeps every row")


_GROUP = {"step": _run_step, "step0": _run_step0, "stepid": _run_stepid, "mploss": _run_mploss, "posce": _run_posce, "tgt": _run_tgt,
          "dec": _run_dec, "cloudmax": _run_cloudmax, "dropout": _run_dropout, "add": _run_add, "droppath": _run_droppath}


def run(row):
    """Run `row`.  -> (record {name: error}, failures [text])."""
    chk = _Check(row)
    _GROUP[row.group](row, chk)
    return chk.rec, chk.fails
