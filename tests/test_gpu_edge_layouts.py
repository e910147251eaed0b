"""The float kernels on the layouts synth scenes never produce (tests/edge_layouts.py): patches of 1 .. 128 rows with 0, 1
and 127 borrowed rows, instructions of 1 .. 78 (and 128) tokens, convolution scenes with 26 empty taps and with 27 full
ones, levels of 1 / 63 / 64 / 65 rows, pooling cells of one and of eight points, a head over 1-point clouds.

References are the float64 formulations tests/test_gpu_ops.py uses for the same kernels, and the bars are its bars (these are
the same kernels on fewer rows), relative to max(1, |ref|max):
    attention forward 5e-6, dqkv / dq / dkv 2e-5, q/k-norm weights 5e-5, dkn_b 5e-4 (mathematically zero: cancellation noise);
    convolution forward and input gradient 3e-6, weight gradient 5e-6; head losses 3e-6, head gradients 1e-5.
The integer tables are compared first (frontend_util.assert_levels_equal), so a float mismatch is never a table mismatch.

Every output buffer the caller owns carries GUARD extra rows filled with a constant; they must come back bit-identical (a
ragged last tile that stores one row too many would otherwise land in the allocator's slack unseen).  The measured errors
go to the ledger (tests/ledger.py), attention errors per cloud so that a failure names the patch length."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import edge_layouts as el  # noqa: E402
import ledger  # noqa: E402
from frontend_util import fe, assert_levels_equal  # noqa: E402
from oracle import model as om  # noqa: E402
from test_gpu_bf16_vs_fp64 import _check_rounded  # noqa: E402

SENT = -7
GUARD = 64
FILL = 12345.0
XQ = os.environ.get("LOTUS_XQ")                # set in the child interpreters only: the kernel family under test
TAG = "edge_layouts/" + (f"xq{XQ}/" if XQ else "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

el.self_check()  # the builders' CPU assertions (no GPU needed): a scene that is not what it says fails the collection


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops
    return ops


def _guarded(rows, cols=None, dtype=torch.float32):
    """-> (buffer with GUARD extra rows, all filled; view of the first `rows` rows)."""
    shape = (rows + GUARD,) if cols is None else (rows + GUARD, cols)
    buf = torch.full(shape, SENT if dtype in (torch.int32, torch.int64) else FILL, dtype=dtype, device="cuda")
    return buf, buf[:rows]


def _guards_intact(**bufs):
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        tail = buf[view.shape[0]:]
        fill = torch.full_like(tail, SENT if buf.dtype in (torch.int32, torch.int64) else FILL)
        assert torch.equal(tail, fill), f"{name}: rows past the end were written"


def _err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0, max(1.0, float(b.abs().max()) if b.numel() else 0.0)


def _bar(rec, name, a, b, tol):
    """Record the error of `a` against `b` relative to max(1, |b|max); -> failure text or None (asserted by the caller after
    everything is recorded)."""
    e, scale = _err(a, b)
    rec[name] = e / scale
    return None if e <= tol * scale else f"{name}: max err {e:.3e} > {tol:.1e} * {scale:.3g}"


def _per_cloud(rec, name, a, b, counts, tol):
    """As _bar, with the error of every cloud (max over its rows) recorded and named in the failure."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(1.0, float(b.abs().max()))
    errs = [float(t.abs().max()) / scale if t.numel() else 0.0 for t in torch.split(a - b, list(counts))]
    rec[name] = max(errs)
    rec[name + "_per_cloud"] = [[int(c), e] for c, e in zip(counts, errs)]
    bad = [(i, int(c), f"{e:.3e}") for i, (c, e) in enumerate(zip(counts, errs)) if not e <= tol]
    return None if not bad else f"{name}: (cloud, rows, err) {bad} over {tol:.1e} (scale {scale:.3g})"


def _finish(test, rec, fails):
    ledger.record(TAG + test, **rec)
    fails = [f for f in fails if f]
    assert not fails, "\n".join(fails)


@functools.lru_cache(maxsize=None)
def _levels(kind, name, n_levels, widths=None):
    """Scene -> (pc_fts, counts, txt_lens, oracle levels, FrontEnd levels), integer tables already compared."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    pc, counts, txt = {"patch": lambda: el.patch_edges(), "ctx": lambda: el.ctx_edges(name),
                       "conv": lambda: el.conv_scenes(name), "pool": lambda: el.pool_scenes(name)}[kind]()
    perms = [[0, 1, 2, 3]] * n_levels
    ref = fe.build_all_levels(pc[:, :3].numpy(), counts, n_levels, perms=perms)
    got = FrontEnd(n_levels, conv_widths=list(widths) if widths else None).build(pc.cuda(), counts, txt, perms)
    assert_levels_equal(ref, got, n_levels, ctx_counts=txt)
    return pc, counts, txt, ref, got


def _child(k_expr, xq, timeout):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", k_expr],
                       capture_output=True, text=True, timeout=timeout, env=dict(os.environ, LOTUS_XQ=xq), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------------------------ patch attention
def _oracle_level(r):
    return dict(order_t=torch.from_numpy(r["order"]), inverse_t=torch.from_numpy(r["inverse"]),
                pad_t=torch.from_numpy(r["pad"]), unpad_t=torch.from_numpy(r["unpad"]), cu_seqlens=r["cu_seqlens"])


def _patch_inputs(C, H, n, seed):
    d = C // H
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * C, generator=g) * 1.5
    qn = (torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2)
    kn = (torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2)
    dout = torch.randn(n, C, generator=g)
    return qkv, qn, kn, dout


def _patch_run(ops, lv, qc, qnc, knc, doutc, C, H, dtype=torch.float32, drop=0.0, seed=0, routes=None):
    """Forward and backward into guarded buffers; -> dict name -> (buffer, view), and the four norm gradients.  `routes` (a
    list) receives the route record after the forward and after the backward call (ops.last_attn_route)."""
    n, d = lv.n, C // H
    b = dict(att=_guarded(n, C, dtype), lse=_guarded(lv.npad, H), dqkv=_guarded(n, 3 * C, dtype),
             extra=_guarded(max(lv.n_extra, 1), 2 * C, dtype))
    att, lse, dqkv, extra = (b[k][1] for k in ("att", "lse", "dqkv", "extra"))
    ops.attention_fwd(qc, 3 * C, 0, qc, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.n_self_tiles,
                      qnc, knc, att, lse, H, d, drop, seed)
    fwd_route = ops.last_attn_route()
    gr = ops.attention_bwd(qc, 3 * C, 0, qc, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.self_blocks,
                           lv.n_self_tiles, qnc, knc, att, doutc, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, 0, H, d, drop, seed,
                           lv.kext, lv.ext_pos, lv.n_extra, extra)
    if routes is not None:
        routes += [fwd_route, ops.last_attn_route()]
    return b, gr


# head widths 32, 24 and 16 along curve slot 0; the other three curve slots (Level.for_order) at 32
PATCH_CASES = [(64, 2, 0), (96, 4, 0), (64, 4, 0), (64, 2, 1), (64, 2, 2), (64, 2, 3)]


@pytest.mark.parametrize("C,H,slot", PATCH_CASES)
def test_patch_attention_edges_fwd_bwd(C, H, slot):
    """Forward and backward of the patch attention on patches of 1, 2, 31 .. 33, 63 .. 65, 127 and 128 rows, clouds of exactly
    128 / 256 rows (nothing borrowed), 129 / 257 (127 borrowed rows) and 255 (one), against om.patch_attention in float64.
    Under LOTUS_XQ=2 (child interpreter, below) the same cases run on the query-per-lane kernels."""
    ops = _ops()
    pc, counts, txt, ref, got = _levels("patch", "", 1)
    r, lv = ref[0], got[0].for_order(slot)
    if slot:  # the gather tables of the other curve slots, against the oracle's
        np.testing.assert_array_equal(lv.gidx.cpu().numpy(), r["order"][slot][r["pad"]])
        owner = np.zeros(len(r["pad"]), np.int32)
        owner[r["unpad"][r["inverse"][slot]]] = 1
        np.testing.assert_array_equal(lv.owner.cpu().numpy(), owner)
    n = lv.n
    qkv, qn, kn, dout = _patch_inputs(C, H, n, seed=C + H + slot)
    qd = qkv.double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (*qn, *kn)]
    oref = om.patch_attention(qd, _oracle_level(r), slot, H, pr[0], pr[1], pr[2], pr[3], 128)
    oref.backward(dout.double())
    routes = []
    b, gr = _patch_run(ops, lv, qkv.cuda(), tuple(t.cuda() for t in qn), tuple(t.cuda() for t in kn), dout.cuda(), C, H, routes=routes)
    _guards_intact(**b)
    # the kernels this case means: the exact-fp32 tile pair, or under LOTUS_XQ=2 the query-per-lane pair of this head width;
    # the edge patches borrow rows, so the fix-up follows the backward kernel, and the norm-gradient reduction always does
    assert lv.n_extra > 0
    R = ops.AttnRoute
    want = ([R(4, 0, C // H, 0, 1, 128, 0, 0), R(4, 1, C // H, 0, 1, 128, 0, 3)] if XQ == "2" else
            [R(1, 0, 0, 0, 1, 256, 53760, 0), R(3, 1, 0, 0, 1, 256, 72192, 3)])
    assert routes == want, (routes, want)
    rec, fails = {}, []
    fails.append(_per_cloud(rec, "fwd", b["att"][1], oref, counts, 5e-6))
    fails.append(_per_cloud(rec, "dqkv", b["dqkv"][1], qd.grad, counts, 2e-5))
    for name, a, p in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), gr, pr):
        fails.append(_bar(rec, name, a, p.grad, 5e-4 if name == "dkn_b" else 5e-5))
    assert torch.isfinite(b["lse"][1]).all()
    _finish(f"patch_attention/C{C}_H{H}_slot{slot}", rec, fails)


def test_patch_attention_edges_query_per_lane():
    """The forward / backward cases and the dropout case on the query-per-lane kernels (LOTUS_XQ=2, read once per process:
    one child interpreter for all of them)."""
    _child("test_patch_attention_edges_fwd_bwd or test_patch_attention_edges_dropout", "2", timeout=300)


def test_patch_attention_edges_bf16_storage():
    """The bf16-storage twin (head width 32) on the same patches.  q / k / v are bf16-exact; the twin feeds bf16 MFMA operands
    (normalised q / k and the probabilities are rounded once more), so its result is not the nearest bf16 of the float64 one
    (exact_min = 0; the fraction is recorded) and the allowance on top of the one output rounding is the bar
    test_patch_attention_twin_against_float64 holds the same kernels to: 1.5e-2 forward, 3e-2 backward, of max |ref|."""
    ops = _ops()
    BF = torch.bfloat16
    C, H = 64, 2
    pc, counts, txt, ref, got = _levels("patch", "", 1)
    r, lv = ref[0], got[0]
    qkv, qn, kn, dout = _patch_inputs(C, H, lv.n, seed=5)
    qkv, dout = qkv.to(BF).float(), dout.to(BF).float()
    qd = qkv.double().requires_grad_(True)
    oref = om.patch_attention(qd, _oracle_level(r), 0, H, qn[0].double(), qn[1].double(), kn[0].double(), kn[1].double(), 128)
    oref.backward(dout.double())
    routes = []
    with ops.storage(BF):
        b, gr = _patch_run(ops, lv, qkv.cuda().to(BF), tuple(t.cuda() for t in qn), tuple(t.cuda() for t in kn),
                           dout.cuda().to(BF), C, H, dtype=BF, routes=routes)
    _guards_intact(**b)
    R = ops.AttnRoute  # (read through the twin's record function inside the storage block: the record is one)
    assert routes == [R(1, 0, 0, 1, 1, 256, 53760, 0), R(2, 1, 0, 1, 1, 256, 72192, 3)], routes
    assert ops.last_attn_route() == routes[1], "the fp32 entry point reads the record the twin wrote"
    rec, fails = {}, []
    fails.append(_per_cloud(rec, "fwd", b["att"][1], oref, counts, 1.5e-2))
    fails.append(_per_cloud(rec, "dqkv", b["dqkv"][1], qd.grad, counts, 3e-2))
    for name, t, r64, slack in (("fwd", b["att"][1], oref.detach(), 1.5e-2), ("dqkv", b["dqkv"][1], qd.grad, 3e-2)):
        try:
            rec[name + "_nearest_bf16"] = _check_rounded(t, r64, slack, f"attention {name} (bf16 storage)", exact_min=0.0)
        except AssertionError as e:
            fails.append(str(e))
    _finish("patch_attention/bf16_storage_C64_H2", rec, fails)


def test_patch_attention_edges_dropout():
    """Attention dropout 0.25 on the edge patches, checked the way test_attention_dropout_mask_is_consistent_between_fwd_and_bwd
    does (same tolerances): E[sum_k P~] = 1, the mask replays, the adjoint identity in V, a central difference in q / k."""
    ops = _ops()
    pc, counts, txt, ref, got = _levels("patch", "", 1)
    lv = got[0]
    C, H, p_drop, seed = 64, 2, 0.25, 99
    n, d = lv.n, C // H
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(n, 3 * C, generator=g).cuda()
    qn = (torch.ones(d).cuda(), torch.zeros(d).cuda())

    def fwd(t):
        b = dict(att=_guarded(n, C), lse=_guarded(lv.npad, H))
        ops.attention_fwd(t, 3 * C, 0, t, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.n_self_tiles,
                          qn, qn, b["att"][1], b["lse"][1], H, d, p_drop, seed)
        _guards_intact(**b)
        return b["att"][1], b["lse"][1]

    ones = qkv.clone()
    ones[:, 2 * C:] = 1.0
    att1, _ = fwd(ones)
    assert abs(att1.mean().item() - 1.0) < 0.02 and att1.std().item() > 0.01
    att, lse = fwd(qkv)
    att_b, _ = fwd(qkv)
    assert torch.equal(att, att_b)
    dout = torch.randn(n, C, generator=g).cuda()
    b = dict(dqkv=_guarded(n, 3 * C), extra=_guarded(max(lv.n_extra, 1), 2 * C))
    dqkv = b["dqkv"][1]
    ops.attention_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lv.gidx, lv.gidx, lv.owner, lv.self_tiles, lv.self_blocks,
                      lv.n_self_tiles, qn, qn, att, dout, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, 0, H, d, p_drop, seed,
                      lv.kext, lv.ext_pos, lv.n_extra, b["extra"][1])
    _guards_intact(**b)
    u = torch.randn(n, 3 * C, generator=g).cuda()
    uv = torch.zeros_like(u)
    uv[:, 2 * C:] = u[:, 2 * C:]
    lhs = ((fwd(qkv + uv)[0] - att) * dout).double().sum().item()
    rhs = (dqkv * uv).double().sum().item()
    uq = torch.zeros_like(u)
    uq[:, :2 * C] = u[:, :2 * C]
    eps = 1e-2
    num = (((fwd(qkv + eps * uq)[0] - fwd(qkv - eps * uq)[0]) / (2 * eps)) * dout).double().sum().item()
    ana = (dqkv * uq).double().sum().item()
    ledger.record(TAG + "patch_attention/dropout_0.25", v_adjoint_rel=abs(lhs - rhs) / max(1.0, abs(rhs)),
                  central_difference_rel=abs(num - ana) / max(1.0, abs(ana)))
    assert abs(lhs - rhs) <= 2e-4 * max(1.0, abs(rhs)), (lhs, rhs)
    assert abs(num - ana) <= 3e-2 * max(1.0, abs(ana)), (num, ana)


# ------------------------------------------------------------------------------------------------ cross attention
def _cross_setup(layout, C, H):
    pc, counts, txt, ref, got = _levels("ctx", layout, 1)
    lv = got[0]
    assert lv.ca_kmax == max(txt)
    n, d, L = lv.n, C // H, sum(txt)
    g = torch.Generator().manual_seed(C + 5)
    q, kv = torch.randn(n, C, generator=g) * 1.5, torch.randn(L, 2 * C, generator=g) * 1.5
    qn = (torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2)
    kn = (torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2)
    dout = torch.randn(n, C, generator=g)
    return lv, counts, txt, q, kv, qn, kn, dout


def _cross_run(ops, lv, qc, kvc, qnc, knc, doutc, C, H, L, k_max, drop=0.0, backward=True, routes=None):
    n, d, G = lv.n, C // H, lv.ca_groups
    routes = [] if routes is None else routes
    b = dict(att=_guarded(n, C), lse=_guarded(n, H))
    att, lse = b["att"][1], b["lse"][1]
    ops.attention_fwd(qc, C, 0, kvc, 2 * C, 0, C, None, None, None, lv.ca_tiles, lv.n_ca_tiles, qnc, knc, att, lse, H, d,
                      drop_p=drop, seed=77, k_max=k_max)
    routes.append(ops.last_attn_route())
    gr = None
    if backward:
        b.update(dq=_guarded(n, C), dkvp=_guarded(G * L * 2 * C))
        dkvp = b["dkvp"][1].view(G, L, 2 * C)
        gr = ops.attention_bwd(qc, C, 0, kvc, 2 * C, 0, C, None, None, None, lv.ca_tiles, lv.ca_blocks, lv.n_ca_blocks, qnc,
                               knc, att, doutc, lse, b["dq"][1], C, 0, dkvp, 2 * C, 0, C, L * 2 * C, 0, H, d, drop_p=drop, seed=77,
                               k_max=k_max)
        routes.append(ops.last_attn_route())
    _guards_intact(**b)
    return b, gr


def _k_max(lv, layout, path):
    """The k_max a path hands the kernels: never smaller than the longest context (the short-key kernels trap on it)."""
    if path == "tile":
        return 0
    if layout == "short":
        assert 0 < lv.ca_kmax <= 32
    else:
        assert lv.ca_kmax > 32, "the dispatcher must see more than 32 keys to route this layout to the tile kernels"
    return lv.ca_kmax


# short: the key-tile-in-registers kernels (k_max = 32; the round-5 kernels under LOTUS_XQ=3) and the tile kernels (k_max = 0);
# long: k_max = 78, which the dispatcher routes to the tile kernels; full: 128 keys, the most their LDS image holds
CROSS_CASES = [(layout, path, C, H) for layout, path in (("short", "short_keys"), ("short", "tile"), ("long", "dispatch"))
               for C, H in ((64, 2), (128, 4), (768, 32))] + [("full", "tile", 64, 2)]


@pytest.mark.parametrize("layout,path,C,H", CROSS_CASES)
def test_cross_attention_edges_fwd_bwd(layout, path, C, H):
    """Cross attention with 1, 2, 31, 32, 33, 64, 77, 78 and 128 keys against clouds of 1 .. 300 points, against
    om.cross_attention in float64; dkv per cloud.  A 1-key cloud has softmax = 1: dK is the LayerNorm backward of zero and
    dV the sum of the cloud's dout rows."""
    ops = _ops()
    lv, counts, txt, q, kv, qn, kn, dout = _cross_setup(layout, C, H)
    L = sum(txt)
    k_max = _k_max(lv, layout, path)
    routes = []
    b, gr = _cross_run(ops, lv, q.cuda(), kv.cuda(), tuple(t.cuda() for t in qn), tuple(t.cuda() for t in kn), dout.cuda(),
                       C, H, L, k_max, routes=routes)
    # the kernels this path means.  short_keys: the key-tile-in-registers pair at head width 32 (the round-5 pair under
    # LOTUS_XQ=3), the keys-in-LDS pair at head width 24; tile (k_max = 0) and dispatch (k_max = 78): the exact-fp32 tile pair
    R, d = ops.AttnRoute, C // H
    if path != "short_keys":
        want = [R(1, 0, 0, 0, 1, 256, 53760, 0), R(3, 1, 0, 0, 1, 256, 72192, 2)]
    elif d == 32 and XQ != "3":
        want = [R(5, 0, 4, 0, 1, 256, 0, 0), R(5, 1, 4, 0, 1, 256, 0, 2)]
    else:
        want = [R(4, 0, d, 0, 1, 128, 0, 0), R(4, 1, d, 0, 1, 128, 0, 2)]
    assert routes == want, (routes, want)
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (*qn, *kn)]
    oref = om.cross_attention(qd, kvd, counts, txt, H, pr[0], pr[1], pr[2], pr[3])
    oref.backward(dout.double())
    dkv = b["dkvp"][1].view(lv.ca_groups, L, 2 * C).sum(0)
    rec, fails = {"k_max": k_max}, []
    fails.append(_per_cloud(rec, "fwd", b["att"][1], oref, counts, 5e-6))
    fails.append(_per_cloud(rec, "dq", b["dq"][1], qd.grad, counts, 2e-5))
    fails.append(_per_cloud(rec, "dkv", dkv, kvd.grad, txt, 2e-5))
    for name, a, p in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), gr, pr):
        fails.append(_bar(rec, name, a, p.grad, 5e-4 if name == "dkn_b" else 5e-5))
    # the 1-key clouds on their own, against closed forms
    scale = max(1.0, float(kvd.grad.abs().max()))
    po, co = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(txt)])
    one = [i for i, t in enumerate(txt) if t == 1]
    assert one
    for i in one:
        row = dkv[co[i]].double().cpu()
        e_k = float(row[:C].abs().max()) / scale
        e_v = float((row[C:] - dout[po[i]:po[i + 1]].double().sum(0)).abs().max()) / scale
        rec[f"one_key_cloud{i}_dk"], rec[f"one_key_cloud{i}_dv"] = e_k, e_v
        if not (e_k <= 2e-5 and e_v <= 2e-5):
            fails.append(f"1-key cloud {i} ({counts[i]} points): |dK| {e_k:.3e}, dV - sum dout {e_v:.3e} over 2e-5")
    _finish(f"cross_attention/{layout}_{path}_C{C}_H{H}", rec, fails)


def test_cross_attention_edges_round5_kernels():
    """`short` with k_max = 32 on the round-5 one-lane-per-query kernels (LOTUS_XQ=3, read once per process: a child)."""
    _child("test_cross_attention_edges_fwd_bwd and short_keys", "3", timeout=300)


@pytest.mark.parametrize("layout", ["short", "long"])
def test_cross_attention_edges_dropout(layout):
    """Dropout 0.25 on the probabilities, as test_cross_attention_fwd_bwd checks it (same tolerances): the hash masks cannot be
    evaluated by the reference, so the backward is checked against central differences of the forward along a random
    direction, and on `short` the two kernel families (k_max = 32 and k_max = 0, which share the mask index) against each
    other.  On `long` both values of k_max reach the tile kernels, so there is no second family to compare with: the
    central difference is the whole check there."""
    ops = _ops()
    C, H, drop = 128, 4, 0.25
    lv, counts, txt, q, kv, qn, kn, dout = _cross_setup(layout, C, H)
    n, L, G = lv.n, sum(txt), lv.ca_groups
    k_max = _k_max(lv, layout, "dispatch" if layout == "long" else "short_keys")
    qc, kvc, doutc = q.cuda(), kv.cuda(), dout.cuda()
    qnc, knc = tuple(t.cuda() for t in qn), tuple(t.cuda() for t in kn)
    run = lambda km, qq=qc, kk=kvc, bw=True: _cross_run(ops, lv, qq, kk, qnc, knc, doutc, C, H, L, km, drop, bw)  # noqa: E731
    b, gr = run(k_max)
    dkv = b["dkvp"][1].view(G, L, 2 * C).sum(0)
    rec, fails = {"k_max": k_max}, []
    if layout == "short":
        b0, gr0 = run(0)
        dkv0 = b0["dkvp"][1].view(G, L, 2 * C).sum(0)
        fails.append(_bar(rec, "fwd_vs_tile", b["att"][1], b0["att"][1], 5e-6))
        fails.append(_bar(rec, "lse_vs_tile", b["lse"][1], b0["lse"][1], 5e-6))
        fails.append(_bar(rec, "dq_vs_tile", b["dq"][1], b0["dq"][1], 2e-5))
        fails.append(_bar(rec, "dkv_vs_tile", dkv, dkv0, 2e-5))
        for name, a, a0 in zip(("dqn_w", "dqn_b", "dkn_w", "dkn_b"), gr, gr0):
            fails.append(_bar(rec, name + "_vs_tile", a, a0, 5e-4 if name == "dkn_b" else 5e-5))
    gdir = torch.Generator(device="cuda").manual_seed(1)
    vq, vk = torch.randn(n, C, device="cuda", generator=gdir), torch.randn(L, 2 * C, device="cuda", generator=gdir)
    want = float((b["dq"][1].double() * vq.double()).sum() + (dkv.double() * vk.double()).sum())
    eps = 1e-2
    fp = float((run(k_max, qc + eps * vq, kvc + eps * vk, False)[0]["att"][1].double() * doutc.double()).sum())
    fm = float((run(k_max, qc - eps * vq, kvc - eps * vk, False)[0]["att"][1].double() * doutc.double()).sum())
    fd = (fp - fm) / (2 * eps)
    rec["central_difference"], rec["analytic"] = fd, want
    if not abs(fd - want) <= 2e-3 * max(abs(want), abs(fd)) + 1e-2:
        fails.append(f"central difference {fd} against {want}")
    _finish(f"cross_attention/dropout_{layout}", rec, fails)


def test_context_longer_than_128_is_refused():
    """The tile kernels hold 128 keys in LDS and index them by tid < 128: FrontEnd.finish refuses a longer context by name,
    on the host, before any cross attention is launched; 128 itself is accepted (test_cross_attention_edges_fwd_bwd[full-tile-64-2]).
    Contexts of length 0 are left as they are: the reference's behaviour there is not pinned."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    pc, counts, txt = el.ctx_edges("full")
    with pytest.raises(ValueError, match=r"129.*128|128.*129"):
        FrontEnd(1).build(pc.cuda(), counts, [129, 5], [[0, 1, 2, 3]])
    lv = FrontEnd(1).build(pc.cuda(), counts, [128, 1], [[0, 1, 2, 3]])[0]
    assert lv.ca_kmax == 128


# ------------------------------------------------------------------------------------------------ sparse convolution
@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 128), (64, 128)])
@pytest.mark.parametrize("scene", el.CONV_SCENES)
def test_subm_conv_edges(scene, cin, cout):
    """The 3^3 convolution — forward, input gradient, weight gradient — on the tap-grouped path (tap plan) and on the
    pair-compacted one (packed weights, no plan), against om.subm_conv in float64 under autograd: a scene whose 26 outer taps
    are empty, three active taps, 27 full taps, levels of 1 / 63 / 64 / 65 rows, 100 clouds of 3, 10 % duplicate voxels (where
    the reference gradient is that of the forward as computed: neighbour = lowest index of the cell)."""
    from robot_3dlotus_amd._capi import query
    ops = _ops()
    n_levels = 2 if scene == "dups" else 1
    pc, counts, txt, ref, got = _levels("conv", scene, n_levels, (64,) * n_levels)
    L, n = got[0], got[0].n
    assert query("lotus_conv_tap_eligible", n, cin, cout) == 1 and L.tap_plan is not None
    lvl = L if scene == "dups" else None
    if scene == "dups":
        assert L.n_dup == 172
    g = torch.Generator().manual_seed(cin * cout + n)
    x, dy = torch.randn(n, cin, generator=g), torch.randn(n, cout, generator=g)
    w = torch.randn(cout, 3, 3, 3, cin, generator=g) / (cin * 9) ** 0.5
    b, add, addd = torch.randn(cout, generator=g), torch.randn(n, cout, generator=g), torch.randn(n, cin, generator=g)
    nbr_ref = torch.from_numpy(ref[0]["nbr27"]).long()
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    yref = om.subm_conv(xd, nbr_ref, wd, bd)
    yref.backward(dy.double())
    xc, dyc, wc, bc, addc, adddc = (t.cuda() for t in (x, dy, w, b, add, addd))
    wt = ops.conv_weight_t(wc)
    rec, fails = {"rows": n}, []
    for path, plan in (("tap_plan", L.tap_plan), ("pairs", None)):
        family = ops.CONV_TAP if plan is not None else ops.CONV_PAIRS
        y = ops.conv_fwd(xc, wc, bc, L.nbr27, L.order[0], add=addc, w_t=wt, tap_plan=plan)
        r = ops.last_conv_route()
        assert (r.family, r.mode, r.nz) == (family, 0, 27 if plan is not None else 9), (path, r)
        fails.append(_bar(rec, f"fwd_{path}", y, yref + add.double(), 3e-6))
        if scene == "isolated":  # only the centre tap: a second, independent reference
            centre = x.double() @ w.double().reshape(cout, 27, cin)[:, 13, :].T + b.double() + add.double()
            fails.append(_bar(rec, f"fwd_{path}_vs_centre_tap", y, centre, 3e-6))
        d = ops.conv_dgrad(dyc, wc, L.nbr27, L.order[0], add=adddc, w_t=wt, lvl=lvl, tap_plan=plan)
        r = ops.last_conv_route()
        assert (r.family, r.mode, r.nz) == (family, 1, 27 if plan is not None else 9), (path, r)
        fails.append(_bar(rec, f"dgrad_{path}", d, xd.grad + addd.double(), 3e-6))
        if scene == "dups":
            naive = ops.conv_dgrad(dyc, wc, L.nbr27, L.order[0], add=adddc, w_t=wt, tap_plan=plan)  # mirrored taps only
            assert float((naive.cpu().double() - xd.grad - addd.double()).abs().max()) > 1e-2, "the case must exercise the fix"
        y2 = ops.conv_fwd(xc, wc, bc, L.nbr27, L.order[0], add=addc, w_t=wt, tap_plan=plan)
        d2 = ops.conv_dgrad(dyc, wc, L.nbr27, L.order[0], add=adddc, w_t=wt, lvl=lvl, tap_plan=plan)
        assert torch.equal(y, y2) and torch.equal(d, d2), f"{path}: two runs must be bit-equal"
    dw, db = ops.conv_wgrad(dyc, xc, w.shape, L.nbr27)
    r = ops.last_conv_route()
    assert (r.family, r.mode, r.nz, r.aux) == (ops.CONV_WGRAD, 2, (n + 1023) // 1024, 1 if n <= 1024 else 0), r
    dw, db = dw.clone(), db.clone()
    fails.append(_bar(rec, "wgrad", dw, wd.grad, 5e-6))
    fails.append(_bar(rec, "bgrad", db, bd.grad, 5e-6))
    dw2, db2 = ops.conv_wgrad(dyc, xc, w.shape, L.nbr27)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "wgrad: two runs must be bit-equal"
    _finish(f"subm_conv/{scene}_{cin}_{cout}", rec, fails)


@pytest.mark.parametrize("scene", el.CONV_SCENES)
def test_stem_conv_edges(scene):
    """The 5^3 stem convolution at 7 input channels (forward and weight gradient: the stem's input has no gradient) on the
    same scenes."""
    ops = _ops()
    n_levels = 2 if scene == "dups" else 1
    pc, counts, txt, ref, got = _levels("conv", scene, n_levels, (64,) * n_levels)
    L, n, cin, cout = got[0], got[0].n, 7, 64
    g = torch.Generator().manual_seed(n)
    x, dy = torch.randn(n, cin, generator=g), torch.randn(n, cout, generator=g)
    w, b = torch.randn(cout, 5, 5, 5, cin, generator=g) / (cin * 9) ** 0.5, torch.randn(cout, generator=g)
    nbr_ref = torch.from_numpy(ref[0]["nbr125"]).long()
    xd, wd, bd = x.double(), w.double().requires_grad_(True), b.double().requires_grad_(True)
    yref = om.subm_conv(xd, nbr_ref, wd, bd)
    yref.backward(dy.double())
    rec, fails = {"rows": n}, []
    y = ops.conv_fwd(x.cuda(), w.cuda(), b.cuda(), L.nbr125, L.order[0])
    fails.append(_bar(rec, "fwd", y, yref, 3e-6))
    assert torch.equal(y, ops.conv_fwd(x.cuda(), w.cuda(), b.cuda(), L.nbr125, L.order[0])), "two runs must be bit-equal"
    dw, db = ops.conv_wgrad(dy.cuda(), x.cuda(), w.shape, L.nbr125)
    fails.append(_bar(rec, "wgrad", dw, wd.grad, 5e-6))
    fails.append(_bar(rec, "bgrad", db, bd.grad, 5e-6))
    dw2, _ = ops.conv_wgrad(dy.cuda(), x.cuda(), w.shape, L.nbr125, need_bias=False)
    fails.append(_bar(rec, "wgrad_no_bias", dw2, wd.grad, 5e-6))
    _finish(f"subm_conv/{scene}_stem_7_64", rec, fails)


# ------------------------------------------------------------------------------------------------ pool / unpool
@pytest.mark.parametrize("C", [64, 128, 768])
@pytest.mark.parametrize("scene", el.POOL_SCENES)
def test_pool_unpool_edges(scene, C):
    """Max pooling and unpooling over cells of one point each, of eight points each and over 100 clouds of 3, at the widths
    the model pools at: values, arg-max and dx exact, unpool_bwd to 2e-6 (as test_pool_unpool)."""
    from robot_3dlotus_amd._capi import call
    pc, counts, txt, ref, got = _levels("pool", scene, 2)
    parent, child = got[0], got[1]
    g = torch.Generator().manual_seed(C)
    x = torch.randn(parent.n, C, generator=g)
    cl = torch.from_numpy(ref[1]["cluster"])
    idx = cl.view(-1, 1).expand(-1, C)
    yref = torch.zeros(child.n, C).scatter_reduce(0, idx, x, "amax", include_self=False)
    b = dict(y=_guarded(child.n, C), arg=_guarded(child.n, C, torch.int32), dx=_guarded(parent.n, C), o=_guarded(parent.n, C),
             dup=_guarded(child.n, C))
    y, arg, dx, o, dup = (b[k][1] for k in ("y", "arg", "dx", "o", "dup"))
    xc = x.cuda()
    call("lotus_pool_max_fwd", xc, child.members, child.seg_start, child.n, C, y, arg)
    assert torch.equal(y.cpu(), yref)
    assert torch.equal(x[arg.cpu().long(), torch.arange(C)], yref)
    dy = torch.randn(child.n, C, generator=g)
    call("lotus_pool_max_bwd", dy.cuda(), arg, child.cluster, parent.n, C, dx)
    xr = x.clone().requires_grad_(True)
    torch.zeros(child.n, C).scatter_reduce(0, idx, xr, "amax", include_self=False).backward(dy)
    assert torch.equal(dx.cpu(), xr.grad)
    if scene == "all_singletons":
        head = torch.from_numpy(ref[1]["head"])
        assert child.n == parent.n and torch.equal(torch.sort(cl)[0], torch.arange(parent.n))
        assert torch.equal(y.cpu(), x[head]) and torch.equal(dx.cpu(), dy[cl]), "singletons: y = x[head], dx a permutation of dy"
    up = torch.randn(child.n, C, generator=g)
    call("lotus_unpool_fwd", xc, up.cuda(), child.cluster, parent.n, C, o)
    assert torch.equal(o.cpu(), x + up[cl])
    call("lotus_unpool_bwd", xc, child.members, child.seg_start, child.n, C, dup)
    _guards_intact(**b)
    rec, fails = {"parents": parent.n, "children": child.n}, []
    fails.append(_bar(rec, "unpool_bwd", dup, torch.zeros(child.n, C, dtype=torch.float64).index_add(0, cl, x.double()), 2e-6))
    _finish(f"pool_unpool/{scene}_C{C}", rec, fails)


# ------------------------------------------------------------------------------------------------ published head
@pytest.mark.parametrize("layout", [0, 1])
def test_head_and_losses_edges(layout):
    """HeadLossFn at the published 30 bins over clouds of 1, 63 .. 65, 129, 257 and 4099 points: a 1-point cloud has 30 logits
    per axis, fewer than the 32 slices its cross entropy is cut into, so some (max, sum) partials are empty.  The four
    losses, ae, dx and all eight parameter gradients against the float64 head of test_head_and_losses; all finite."""
    ops = _ops()
    counts = el.head_counts(layout)
    N, C, B, nb = sum(counts), 128, len(counts), 30
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device="cuda")
    batch = torch.repeat_interleave(torch.arange(B, device="cuda", dtype=torch.int32), torch.tensor(counts, device="cuda"))
    lv = SimpleNamespace(counts=counts, off=off, batch=batch)
    g = torch.Generator().manual_seed(4 + layout)
    x = torch.randn(N, C, generator=g)
    ws = [torch.randn(C, C, generator=g) / 11, torch.randn(C, generator=g) * 0.1, torch.randn(3 * nb, C, generator=g) / 11,
          torch.randn(3 * nb, generator=g) * 0.1, torch.randn(C, C, generator=g) / 11, torch.randn(C, generator=g) * 0.1,
          torch.randn(217, C, generator=g) / 11, torch.randn(217, generator=g) * 0.1]
    gt = torch.cat([torch.randn(B, 3, generator=g) * 0.1, torch.randint(0, 72, (B, 3), generator=g).float(),
                    torch.randint(0, 2, (B, 1), generator=g).float()], 1)
    probs = [torch.softmax(torch.randn(3, c * nb, generator=g), 1) for c in counts]
    tgt = torch.cat([t.reshape(-1) for t in probs])
    xd = x.double().requires_grad_(True)
    wd = [w.double().requires_grad_(True) for w in ws]
    h = F.leaky_relu(F.linear(xd, wd[0], wd[1]), 0.02)
    xt = F.linear(h, wd[2], wd[3]).view(-1, 3, nb).permute(1, 0, 2)
    pcs = torch.stack([t.max(0)[0] for t in torch.split(xd, counts)], 0)
    ae = F.linear(F.leaky_relu(F.linear(pcs, wd[4], wd[5]), 0.02), wd[6], wd[7])
    pos = sum(F.cross_entropy(lg.reshape(3, -1), tg.double()) for lg, tg in zip(torch.split(xt, counts, 1), probs)) / B
    rot = F.cross_entropy(ae[:, :216].reshape(-1, 72, 3), gt[:, 3:6].long())
    opn = F.binary_cross_entropy_with_logits(ae[:, -1], gt[:, -1].double())
    total = pos + rot + opn
    total.backward()
    xc = x.cuda().requires_grad_(True)
    wc = [w.cuda().requires_grad_(True) for w in ws]
    losses, xt_g, ae_g = ops.HeadLossFn.apply(xc, *wc, lv, tgt.cuda(), gt.cuda(), 1.0, 1.0, 0.0, 0, True)
    losses[3].backward()
    torch.cuda.synchronize()
    rec, fails = {}, []
    fails.append(_bar(rec, "losses", losses, torch.stack([pos, rot, opn, total]), 3e-6))
    fails.append(_bar(rec, "ae", ae_g, ae, 3e-6))
    fails.append(_per_cloud(rec, "dx", xc.grad, xd.grad, counts, 1e-5))
    for i, (a, p) in enumerate(zip(wc, wd)):
        fails.append(_bar(rec, f"param{i}", a.grad, p.grad, 1e-5))
    for name, t in (("losses", losses), ("ae", ae_g), ("xt", xt_g), ("dx", xc.grad), *((f"param{i}", a.grad) for i, a in enumerate(wc))):
        if not bool(torch.isfinite(t).all()):
            fails.append(f"{name} is not finite")
    _finish(f"head/counts_{'_'.join(map(str, counts))}", rec, fails)
