"""GPU checks of the soft trajectory head's entry points (csrc/reg_head.hip: lotus_mp_softpos_fwd / _bwd, lotus_mp_reg_loss_fwd /
_bwd) through the raw C-ABI, on the rows of tests/trajsoft_util.py: guarded caller-owned buffers, workspaces of exactly the queried
size, every row run twice bit for bit; against the float64 restatement (bars: KERNEL_TOL = 2e-5 x max(1, |ref|max) per tensor,
losses 1e-4) and against the composition of the per-step entry points that were there before (same masks, same bars); the exact
zeros of masked steps and of a one-point cloud; one directional finite difference.  The row with |e0| = 100 at temp 0.1 checks e
against the inputs and the softmax stage at the logits the kernel stored: trajsoft_util.reference says why."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import trajsoft_util as tu  # noqa: E402
from norm_run import _Check  # noqa: E402

KERNEL_TOL, LOSS_TOL = tu.KERNEL_TOL, tu.LOSS_TOL
_CACHE = {}


def _rel(got, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu().reshape(ref.shape) - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _row(row_id):
    """One row: inputs, float64 reference, the fused run (twice) and the composed run, computed once and shared by the tests."""
    if row_id not in _CACHE:
        row = tu.ROWS[tu.ROW_IDS.index(row_id)]
        chk = _Check(row)
        v = tu.inputs(row)
        _CACHE.clear()   # (one row at a time: the big row holds 70 001 x 64 x 5 scales)
        ref, got = tu.reference(row, v), tu.run_fused(row, v, chk)
        if row.opts.get("hot"):  # e against the inputs; the softmax stage at the stored logits (why: tu.reference)
            ref = dict(tu.reference(row, v, got["e"].cpu()), e=ref["e"])
        _CACHE[row_id] = (row, v, ref, got, chk)
    return _CACHE[row_id]


NAMES = ("e", "xt", "stats", "dbase", "dbias", "dw3", "db3")


@pytest.mark.parametrize("row_id", tu.ROW_IDS)
def test_fused_head_against_float64(row_id):
    row, v, ref, got, chk = _row(row_id)
    print(f"    {row.id}: {row.why}")
    assert not chk.fails, "\n".join(chk.fails)       # bit-equal reruns, guards intact
    for name in NAMES:
        assert bool(torch.isfinite(got[name]).all()), f"{name} is not finite"
        e = _rel(got[name], ref[name])
        print(f"    {name}: err {e:.3e}  (bar {KERNEL_TOL:.0e} x max(1, |ref|max))")
        assert e <= KERNEL_TOL, (row.id, name, e)


@pytest.mark.parametrize("row_id", tu.ROW_IDS)
def test_fused_head_against_the_composed_entry_points(row_id):
    row, v, ref, got, chk = _row(row_id)
    comp = tu.run_composed(row, v)
    for name in NAMES:
        e = _rel(got[name], comp[name])
        print(f"    {name}: fused - composed {e:.3e}  composed - float64 {_rel(comp[name], ref[name]):.3e}")
        assert e <= KERNEL_TOL, (row.id, name, e)


@pytest.mark.parametrize("row_id", ["one-point-c4-t1", "one-point-c64-t5"])
def test_one_point_cloud_is_exact(row_id):
    """p_i = 1: xt is the point's coordinate plus its offsets (one fp32 rounding of their sum), and de_0 — hence db3[0], the only
    row's only contribution — is exactly zero."""
    row, v, ref, got, chk = _row(row_id)
    e = got["e"].cpu()                                                     # [T, 1, 4]
    want = (v["pc"][0, :3].double()[None] + e[:, 0, 1:].double()).float()   # [T, 3]
    assert torch.equal(got["xt"].cpu()[0], want)
    assert float(got["db3"][0]) == 0.0
    assert bool((got["stats"][..., 0] == got["stats"][..., 1]).all())       # log-sum-exp of one logit = the logit


@pytest.mark.parametrize("row_id", ["sizes-c64-t5", "t1-c64-zero-g"])
def test_zero_upstream_steps_give_exact_zeros(row_id):
    row, v, ref, got, chk = _row(row_id)
    B, T = len(row.counts), row.T
    off = torch.from_numpy(tu.offsets(row.counts)[0].numpy())
    assert not bool(got["dbase"][int(off[B - 1]):].any()), "rows of the cloud whose g is zero"
    if T > 1:
        assert not bool(got["dbias"][T // 2].any()), "the bias row of the step whose g is zero"
    assert bool(got["dbase"][:int(off[B - 1])].any())


def test_directional_finite_difference():
    """A central difference of the float64 restatement along a direction in `base` against the kernel's dbase: the direction has
    unit L1 norm on the eight largest entries of the reference gradient, so |<dbase - dbase_ref, d>| <= max |dbase - dbase_ref|
    (Hoelder) and the bar is the kernel's.  No pre-activation is within 1e-5 of zero and the step moves each by at most 1.25e-6."""
    row, v, ref, got, chk = _row("sizes-c64-t5")
    gref = ref["dbase"]
    top = gref.abs().flatten().topk(8).indices
    d = torch.zeros_like(gref).flatten()
    d[top] = torch.sign(gref.flatten()[top]) / 8
    d = d.view_as(gref)
    eps = 1e-5
    f64 = {k: v[k].double() for k in ("base", "bias", "w3", "b3", "pc", "g", "scales")}

    def loss(b):
        return (tu.head_ref(b, f64["bias"], f64["w3"], f64["b3"], f64["pc"][:, :3], row.counts, row.temp, f64["scales"])[1] * f64["g"]).sum().item()

    fd = (loss(f64["base"] + eps * d) - loss(f64["base"] - eps * d)) / (2 * eps)
    mine = (got["dbase"].double().cpu() * d).sum().item()
    bar = KERNEL_TOL * max(1.0, float(gref.abs().max())) + 1e-8   # (+ the truncation / rounding of the difference quotient)
    print(f"    fd {fd:.9e}  <dbase, d> {mine:.9e}  bar {bar:.3e}")
    assert abs(fd - mine) <= bar


def test_hot_logits_stay_finite_and_one_row_dominates():
    row, v, ref, got, chk = _row("hot-c64-t5")
    z = got["e"][..., 0].abs().max().item() / row.temp
    assert 900 < z < 1100, z
    n0 = row.counts[0]
    p = torch.softmax(got["e"].double().cpu()[:, :n0, 0] / row.temp, 1)
    assert float(p.max()) > 0.99, "no (cloud, step) of the row has a dominating point"
    assert all(bool(torch.isfinite(got[k]).all()) for k in NAMES)


@pytest.mark.parametrize("name", list(tu.LOSS_CASES))
def test_reg_losses_against_float64(name):
    B, T, nrot, _ = tu.LOSS_CASES[name]
    v = tu.loss_inputs(name)

    class _R:
        id = "loss-" + name

    chk = _Check(_R)
    got = tu.run_loss(name, v, chk)
    ref = tu.loss_reference(name, v)
    assert not chk.fails, "\n".join(chk.fails)
    for k, nme in enumerate(("pos", "rot", "open", "stop", "total")):
        r = float(ref["losses"][k])
        e = abs(float(got["losses"][k]) - r) / max(1.0, abs(r))
        print(f"    loss {nme}: {float(got['losses'][k]):.7f}  ref {r:.7f}")
        assert e <= LOSS_TOL, (nme, e)
    for nme in ("dae_out", "dxt_out"):
        e = _rel(got[nme], ref[nme])
        print(f"    {nme}: err {e:.3e}")
        assert e <= KERNEL_TOL, (nme, e)
    # the saved partial derivatives scaled by hand are the outputs of the backward entry point
    m0 = (v["mask"].view(-1) == 0)
    if bool(m0.any()):
        for nme in ("dae", "dxt", "dae_out", "dxt_out"):
            assert not bool(got[nme].cpu()[m0].any()), f"{nme}: rows of masked steps are not exactly zero"
