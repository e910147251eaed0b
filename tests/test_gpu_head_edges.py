"""The kernels of csrc/pool_head.hip on the edge shapes of tests/head_edges.py: the trajectory head's hidden layer over every
row-lane geometry of its backward (widths 4 .. 1024, rows around the 64 of a block, three accumulating steps, behind the
8192-block cap of the forward), the trajectory losses (one block: B T 3 around 256, B beyond 256, the LDS limit, masks with holes,
saturated logits), the per-step heatmap cross entropy (clouds shorter than the 32 slices, two to four bin passes, empty targets,
zero weights), the soft position targets and the arg-max decode against oracle/labels.py (robot clouds, far ground truth, exact ties
across lanes, half-waves, waves and slices), the per-cloud maximum (column guard, second column group, 1 .. 257 rows, ties across
splits and lanes) and the elementwise kernels across their grid caps, every dropout mask against its numpy restatement; the
bf16-storage twin on a subset.

Each row runs the raw C-ABI calls into guarded caller-owned buffers, twice (tests/head_run.py: references, bars, input
conditions).  Measured errors: ledger, head_edges/<row id>."""
import pytest

pytestmark = pytest.mark.gpu

import head_edges as he  # noqa: E402
import head_run as hr  # noqa: E402
import ledger  # noqa: E402


@pytest.mark.parametrize("row_id", [r.id for r in he.ROWS])
def test_head_edge(row_id):
    row = he.BY_ID[row_id]
    try:
        rec, fails = hr.run(row)
    except AssertionError:
        raise
    except Exception as e:      # a launch or device error: nothing more is started on the device in this session
        pytest.exit(f"{row.id}: {type(e).__name__}: {e}", returncode=3)
    ledger.record("head_edges/" + row.id, why=row.why, **rec)
    assert not fails, "\n".join(fails[:40])
