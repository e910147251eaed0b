"""gemm_kernel on the edge shapes of tests/dense_edges.py: 1 .. 257 rows against output widths and reductions that are no
multiple of the tile (68, 36), of 4 (90, 217, 5, 6: the per-element guarded form) or start 4 bytes off a 16-byte boundary;
split-K ranges with a tail and with EMPTY ranges, fused and in two launches; weight gradients over 1 .. 1300 rows with and
without bias, db behind dw and in a buffer of its own, with and without arrival counters, accumulating on each of the three
routes; bf16 / bf16x3 operands.

Every call is the raw C-ABI entry point (tests/dense_run.py): every buffer it writes — y, pre, dx, the dw | db slab, a separate
db, the workspace at exactly the queried size — is the caller's and carries 64 guard rows that must come back bit-identical.
After each call the recorded route (lotus_dense_last_route) must be the table's, two runs must be bit-equal, the arrival
counters zero.  References are float64; bars are in tests/dense_run.py.  Measured errors: ledger, dense_edges/..."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import dense_edges as de  # noqa: E402
import dense_run as dr  # noqa: E402
import ledger  # noqa: E402

CHILD = all(os.environ.get(k) == v for k, v in de.FEW_ENV.items())   # the child interpreter of the few-rows test
TAG = "dense_edges/" + ("few_rows_dma/" if CHILD else "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counters():
    from robot_3dlotus_amd import _capi

    c = torch.zeros(_capi.query("lotus_splitk_counters_bytes"), dtype=torch.uint8, device="cuda")
    yield c
    assert bool((c == 0).all())


def _run_all(test, cases, counters):
    assert cases
    rec, fails, outs = {}, [], {}
    for case in cases:
        r, f, out = dr.run(case, counters, expect=case.route if CHILD else de.default_route(case))
        rec[case.id] = max(r.values())
        fails += f
        outs[case.id] = out
    ledger.record(TAG + test, **rec)
    return fails, outs


def _finish(fails):
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("call", ["fwd", "dgrad"])
@pytest.mark.parametrize("out,red", de.PAIRS)
def test_few_rows_every_epilogue(call, out, red, counters):
    """Rows 1 .. 257 at one (output width, reduction): every epilogue, and (FAST pairs) the activation operand off by 4 bytes."""
    cases = [c for c in de.GRID if c.call == call and (c.N, c.K) == ((out, red) if call == "fwd" else (red, out))]
    assert len(cases) == len(de.ROWS) * (3 if (out, red) not in de.GUARDED_PAIRS else 2)
    fails, _ = _run_all(f"{call}/{out}x{red}", cases, counters)
    _finish(fails)


@pytest.mark.parametrize("call", ["fwd", "dgrad"])
def test_split_reduction_with_tails_and_empty_ranges(call, counters):
    """448 + 324; 3 x 448 + 196; 16 ranges of which the last two are empty; a guarded and an unsplit shape: with the full
    epilogue, fused (counters) and in two launches, bit-identical to each other."""
    cases = [c for c in de.SPLIT if c.call == call]
    fails, outs = _run_all(f"{call}/splitk", cases, counters)
    for c in cases:
        if c.opts["counters"]:
            other = outs[c.id.replace("-cnt", "-nocnt")]
            for name, t in outs[c.id].items():
                if not torch.equal(t, other[name]):
                    fails.append(f"{c.id}: {name} differs between the fused and the two-launch reduction")
    _finish(fails)


@pytest.mark.parametrize("n,k", de.WGRAD_NK + [(512, 512)])
def test_weight_gradient_ranges_and_variants(n, k, counters):
    """Reduction rows 1 .. 1025 (257: 192 + 65; 520: four ranges, one empty, fused; 1025: eight ranges, two empty, two
    launches) and 1300 x 512 x 512 (one empty range): bias or not, db behind dw or apart, counters or not, accumulate = 1 onto
    non-zero dw / db with one range, fused and in two launches (reference: the prior contents plus the float64 product)."""
    cases = [c for c in de.WGRAD if (c.N, c.K) == (n, k)]
    assert len(cases) == len(de.WGRAD_VARIANTS) * (1 if n == 512 else len(de.WGRAD_ROWS))
    fails, outs = _run_all(f"wgrad/{n}x{k}", cases, counters)
    for c in cases:   # the fused hand-off against the two-launch reduction of the same ranges
        if c.id.endswith("-plain"):
            a, b = outs[c.id]["dwdb"], outs[c.id.replace("-plain", "-nocnt")]["dwdb"]
            if not torch.equal(a, b):
                fails.append(f"{c.id}: dw | db differ between counters given and not")
    _finish(fails)


@pytest.mark.parametrize("prec", [1, 3])
def test_bf16_operand_modes_on_few_rows(prec, counters):
    cases = [c for c in de.PRECISION if c.opts["prec"] == prec]
    fails, _ = _run_all(f"prec{prec}", cases, counters)
    _finish(fails)


def test_partial_last_slab_behind_a_full_ring(counters):
    """Reduction 196 unsplit: three full slabs and a partial fourth on the two-slab register ring (its drain ran one pass short
    and dropped such a tail: every width of the model is a multiple of 128, so nothing else reaches it)."""
    fails, _ = _run_all("tail", de.TAIL, counters)
    _finish(fails)


@pytest.mark.parametrize("prec", [1, 0])
def test_bf16_storage_twin_on_few_rows(prec, counters):
    """lotus_b16_linear_fwd / _dgrad / _wgrad on rows 5, 64, 65 (and, bf16 operands, a reduction of 228 behind the four-slab
    ring): precision 1 is the twin's vectorised path, precision 0 its exact-product fallback; the recorded ring depth tells
    which ran.  bf16 buffers carry the same guard rows."""
    cases = [c for c in de.TWIN if c.opts["prec"] == prec]
    fails, _ = _run_all(f"b16/prec{prec}", cases, counters)
    _finish(fails)


def test_bf16_storage_path_as_ops_selects_it():
    """Through ops in bf16-storage mode (ops.storage: operand precision 1 always): 5 rows at 64 x 64 run the vectorised bf16
    product (four-slab ring) — the row count does not send a forward product to the fallback, its activation operand is
    k-contiguous — and the 90-wide layer runs the exact-product fallback (guarded form, no ring).  Values against float64
    with the storage bar of tests/test_gpu_bf16_ops.py."""
    from robot_3dlotus_amd import ops

    g = torch.Generator().manual_seed(5)
    rec = {}
    for n, want in ((64, (1, 64, 64, 32, 1, 1, 0, 4)), (90, (1, 64, 64, 32, 1, 0, 0, 1))):
        x = torch.randn(5, 64, generator=g).bfloat16()
        w = (torch.randn(n, 64, generator=g) / 8).bfloat16().float()
        b = torch.randn(n, generator=g)
        with ops.storage(torch.bfloat16):
            y, _ = ops.linear_fwd(x.cuda(), w.cuda(), b.cuda())
            route = tuple(ops.last_dense_route())
        assert y.dtype == torch.bfloat16 and route == want, (n, route)
        ref = x.double() @ w.double().t() + b.double()
        rec[f"5x{n}x64"] = float((y.double().cpu() - ref).abs().max()) / float(ref.abs().max())
        assert rec[f"5x{n}x64"] < dr.R_STORE, rec
    ledger.record(TAG + "b16/ops", **rec)


@pytest.mark.parametrize("call", ["fwd", "dgrad", "dgrad_ln", "wgrad"])
def test_few_rows_case(call, counters):
    """The FEW rows of the table: 1 .. 257 rows on a wide and a narrow output, weight gradients over 1024 / 1061 / 2085 rows
    with counters, plain and accumulating.  In this process they are gemm_kernel runs; in the child interpreter of the test
    below (de.FEW_ENV) every one must be a gemm_dma_kernel run, four-range weight gradients fused — same references, same bars.
    dgrad_ln is NOT the LayerNorm epilogue here: that kernel needs 128 row tiles whatever the switches say, so these rows are
    the two-launch path (dn = dy w checked in memory, nparts = lotus_layernorm_bwd_parts) and family 2 is its plain product."""
    cases = [c for c in de.FEW if c.call == call]
    fails, _ = _run_all(f"few/{'dgrad_ln_two_launch' if call == 'dgrad_ln' else call}", cases, counters)
    _finish(fails)


def test_lds_dma_kernels_on_few_rows_in_a_child_interpreter():
    """The dispatcher never gives gemm_dma_kernel fewer than 16 384 rows, and reads its thresholds once per process: one fresh
    interpreter with the documented switches runs test_few_rows_case on those kernels (the route assertion fails the child if
    anything falls back to gemm_kernel)."""
    assert not CHILD
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "test_few_rows_case"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, **de.FEW_ENV), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "4 passed" in r.stdout and "skipped" not in r.stdout and "deselected" in r.stdout, r.stdout[-500:]
