"""The submanifold convolution on the edge shapes of tests/conv_edges.py, one test per row: the generic kernel at the widths
of the shipped YAML's level 0 (32 -> 32, 6 -> 32 at 5^3) and at 96 / 192 columns; the thin-input stem kernel at every CIN
template and on 1 / 31 / 32 / 33 rows; the pair-compacted kernel at every width, at gx > 1, on both sides of every tap-split
boundary and through its OVERFLOW PHASES (257 distinct rows, an empty half-phase, a wrapping probe chain, two row tiles
sharing the flag, a solid 21^3 block); the bf16 operand modes on the pair kernel and on the output-stationary one; the weight
gradient over 1 .. 2049 rows, direct and reduced, accumulating, with db null / apart / behind dw; the bf16-storage twin.

Every call is the raw C-ABI entry point (tests/conv_run.py) into caller-owned buffers pre-filled with a sentinel and followed by
64 guard rows; the workspace has exactly the size handed over.  After each call the recorded route (lotus_conv_last_route) must
be the row's literal, two runs must be bit-equal, no sentinel may be left and no guard touched.  References are the float64
restatement of the gather; bars are in tests/conv_run.py.  Measured errors: ledger, conv_edges/<row id>.
tests/test_conv_phase_plan_host.py guarantees that the overflow rows overflow in the sequence they name."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import conv_edges as ce  # noqa: E402
import conv_run as cr  # noqa: E402
import ledger  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get("LOTUS_CONV_OS") == "0" or os.environ.get("LOTUS_CONV_OS_F32") == "1"
TAG = "conv_edges/" + ("os0/" if os.environ.get("LOTUS_CONV_OS") == "0" else "osf32/" if os.environ.get("LOTUS_CONV_OS_F32") == "1" else "")
MAIN = [r for g, rows in ce.GROUPS.items() if g not in ("OS", "OSF32") for r in rows]


def _one(rid):
    row = ce.BY_ID[rid]
    rec, fails = cr.run(row, expect=ce.expected_route(row, os.environ))
    ledger.record(TAG + rid, **rec)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rid", [r.id for r in MAIN])
def test_conv_row(rid):
    _one(rid)


@pytest.mark.parametrize("rid", [r.id for r in ce.OS])
def test_os_row(rid):
    """bf16 / bf16x3 operands with KD % 64 == 0: conv_os_kernel here, conv_pairs_kernel in the child with LOTUS_CONV_OS=0."""
    _one(rid)


@pytest.mark.parametrize("rid", [r.id for r in ce.OSF32])
def test_osf32_row(rid):
    """Exact fp32 products: conv_pairs_kernel here, conv_os_kernel<0, ...> in the child with LOTUS_CONV_OS_F32=1."""
    _one(rid)


@pytest.mark.parametrize("rid", [r.id for r in ce.REFUSE])
def test_refusal(rid):
    fails = cr.run_refusal(ce.BY_ID[rid])
    assert not fails, "\n".join(fails)


def _child(env, test, count):
    assert not CHILD
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", test],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert f"{count} passed" in r.stdout and "deselected" in r.stdout, r.stdout[-500:]


def test_bf16_modes_on_the_pair_kernel_in_a_child_interpreter():
    """LOTUS_CONV_OS is read once per process: a fresh interpreter runs test_os_row with the switch off; the route assertion
    fails the child if a row stays on conv_os_kernel."""
    _child(ce.OS_ENV, "test_os_row", len(ce.OS))


def test_fp32_on_the_output_stationary_kernel_in_a_child_interpreter():
    """LOTUS_CONV_OS_F32=1 (opt-in): a fresh interpreter runs test_osf32_row on conv_os_kernel<0, NS, 64>."""
    _child(ce.OSF32_ENV, "test_osf32_row", len(ce.OSF32))
