"""The fp32 weight gradient of the submanifold convolution on the tiles of conv_wgrad_kernel<BM, BN>: widths that give a
full 128 x 128 tile (128 x 128), a half-empty wide tile (cout 192, cin 192) and mixed sides (128 x 64, 64 x 128), over one, two
and three row splits, on tables with a quarter of the taps present, with a tap that has no pair at all, and with taps whose
pair count in a split is a multiple of the slab depth (16 pairs) minus one, exact, and plus one.

Every case is run under the dispatcher's own tile (64 x 64: the wide tiles measured slower in the step, profiles/r07_conv_wgrad.md)
and with 128 on every side that can take it (LOTUS_CONV_WG_TILE=128, read at every call), through the raw C-ABI entry point
into guarded buffers, twice.  The recorded route must name the tile that ran; two runs must be bit-equal; dw and db must match
the float64 sum dw[c][t][k] = sum_p dy[p][c] x[nbr[t][p]][k], db = colsum(dy) within the bar of the existing fp32
weight-gradient rows (tests/conv_run.py: 5e-6 * max(1, |ref|max)); and the two tiles must agree BIT FOR BIT, because every
output element sums its pairs in the same order whatever the tile.  (The same inputs through the library of the parent commit
gave the same bits as both, for these 25 shapes and for the four wide levels of the bench batch: profiles/r07_conv_wgrad.md.)"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_run as cr  # noqa: E402

T = 27
CHUNK = 1024          # rows per split (the default of LOTUS_CONV_WG_CHUNK)
SLAB = 16             # pairs per slab
BAR = 5e-6            # tests/conv_run.py, fp32 wgrad / bgrad
ROWS = [1, 63, 257, 1025, 2049]
SHAPES = [(128, 128), (192, 128), (128, 64), (64, 128), (256, 192)]      # (cout, cin)
TABLES = ["quarter", "emptytap", "slabedge"]
EDGE_TAPS = {3: SLAB - 1, 4: SLAB, 5: SLAB + 1, 6: 2 * SLAB - 1, 7: 2 * SLAB + 1, 8: 4 * SLAB}
# (db, accumulate): db absent / its own buffer / behind dw in one buffer (dw | db reduced in one pass when split)
VARIANTS = [("none", 0), ("sep", 0), ("tail", 1)]


def _side(width):
    return 128 if (width >= 128 and width % 64 == 0) else 64


def expected_tile(rule, cout, cin):
    return (64, 64) if rule == "auto" else (_side(cout), _side(cin))


@functools.lru_cache(maxsize=None)
def table(kind, n):
    """int32 nbr[T][n]: the centre tap is the identity; the others hold a uniformly random row with probability 1/4."""
    rng = np.random.default_rng(1000 * TABLES.index(kind) + n)
    nbr = np.where(rng.random((T, n)) < 0.25, rng.integers(0, n, size=(T, n)), -1).astype(np.int32)
    if kind == "emptytap":
        nbr[5] = -1
    if kind == "slabedge":
        for p0 in range(0, n, CHUNK):
            rows = np.arange(p0, min(n, p0 + CHUNK))
            for t, count in EDGE_TAPS.items():
                nbr[t, rows] = -1
                pick = rng.choice(rows, min(count, len(rows)), replace=False)
                nbr[t, pick] = rng.integers(0, n, size=len(pick))
    nbr[T // 2] = np.arange(n, dtype=np.int32)
    return nbr


@functools.lru_cache(maxsize=4)
def case(kind, n, cout, cin):
    """-> (dy, x, prior dw | db, nbr, float64 dw, float64 db), computed once per case and left unchanged."""
    g = torch.Generator().manual_seed(7 * n + 3 * cin + cout + TABLES.index(kind))
    dy, x = torch.randn(n, cout, generator=g), torch.randn(n, cin, generator=g)
    prior = torch.randn(cout * T * cin + cout, generator=g) * 3.0
    nbr = table(kind, n)
    dw = cr.wgrad_ref(dy.double(), x.double(), torch.from_numpy(nbr).long()).reshape(-1)
    return dy, x, prior, nbr, dw, dy.double().sum(0)


def run_once(c, n, cout, cin, db, acc, rule, monkeypatch):
    """One call under a tile rule, twice.  -> (dw, db or None) of the first run, after the route, guard and repeat checks."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi, ops

    dy, x, prior, nbr = c[:4]
    wsz = cout * T * cin
    if rule == "auto":
        monkeypatch.delenv("LOTUS_CONV_WG_TILE", raising=False)
    else:
        monkeypatch.setenv("LOTUS_CONV_WG_TILE", rule)
    bufs = dict(dy=cr.Buf(n, cout), x=cr.Buf(n, cin))
    bufs["dy"].view.copy_(dy)
    bufs["x"].view.copy_(x)
    if db == "tail":
        bufs["dwdb"] = cr.Buf(wsz + cout, 1)
        out_w, out_b = bufs["dwdb"].view, bufs["dwdb"].view.data_ptr() + 4 * wsz
    else:
        bufs["dw"] = cr.Buf(wsz, 1)
        out_w, out_b = bufs["dw"].view, None
        if db == "sep":
            bufs["db"] = cr.Buf(cout, 1)
            out_b = bufs["db"].view
    nbytes = _capi.query("lotus_subm_conv_wgrad_workspace", n, T, cin, cout)
    bufs["workspace"] = cr.Buf(nbytes // 4, 1)      # exactly the size handed over
    dnbr = torch.from_numpy(nbr).cuda()
    nsplit = -(-n // CHUNK)
    bm, bn = expected_tile(rule, cout, cin)
    want = (ops.CONV_WGRAD, 2, bm, bn, 0, nsplit, CHUNK, 1 if (nsplit == 1 and not acc) else 0)
    written = [k for k in ("dw", "db", "dwdb") if k in bufs]
    runs = []
    for _ in range(2):
        for k in written:
            if acc:
                bufs[k].view.copy_((prior if k == "dwdb" else prior[:wsz] if k == "dw" else prior[wsz:]).view(-1, 1))
            else:
                bufs[k].view.fill_(cr.FILL)
        cr.device("wgrad tiles", _capi.call, "lotus_subm_conv_wgrad", bufs["dy"].view, bufs["x"].view, out_w, out_b, dnbr, n, T, cin, cout,
                  acc, 0, bufs["workspace"].view, nbytes)
        assert tuple(ops.last_conv_route()) == want, (rule, tuple(ops.last_conv_route()), want)
        cr.device("wgrad tiles", torch.cuda.synchronize)
        runs.append({k: bufs[k].view.clone() for k in written})
    for k in written:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k} differs between two runs ({rule})"
    for k, b in bufs.items():
        assert b.guard_intact(), f"{k}: rows past the end were written ({rule})"
    if db == "tail":
        flat = runs[0]["dwdb"].reshape(-1)
        return flat[:wsz], flat[wsz:]
    return runs[0]["dw"].reshape(-1), (runs[0]["db"].reshape(-1) if db == "sep" else None)


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("cout,cin", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_wgrad_tiles(n, cout, cin, kind, monkeypatch):
    c = case(kind, n, cout, cin)
    prior, ref_w, ref_b = c[2], c[4], c[5]
    wsz = cout * T * cin
    if kind == "emptytap":
        assert not (c[3][5] >= 0).any()
    if kind == "slabedge" and n > 4 * SLAB:
        counts = {int((c[3][t, :CHUNK] >= 0).sum()) for t in EDGE_TAPS}
        assert {SLAB - 1, SLAB, SLAB + 1} <= counts
    for db, acc in VARIANTS:
        want_w = ref_w + (prior[:wsz].double() if acc else 0.0)
        want_b = ref_b + (prior[wsz:].double() if acc else 0.0)
        outs = {}
        for rule in ("auto", "128"):
            got_w, got_b = run_once(c, n, cout, cin, db, acc, rule, monkeypatch)
            assert not bool((got_w == cr.FILL).any()), f"dw: elements still hold the sentinel ({rule})"
            e = float((got_w.double().cpu() - want_w).abs().max()) / max(1.0, float(want_w.abs().max()))
            print(f"n {n} {cout}x{cin} {kind} db {db} acc {acc} tile {rule}: dw error {e:.3e}")
            assert e <= BAR, f"dw error {e:.3e} > {BAR:.0e} (db {db}, accumulate {acc}, tile {rule})"
            if got_b is not None:
                e = float((got_b.double().cpu() - want_b).abs().max()) / max(1.0, float(want_b.abs().max()))
                print(f"n {n} {cout}x{cin} {kind} db {db} acc {acc} tile {rule}: db error {e:.3e}")
                assert e <= BAR, f"db error {e:.3e} > {BAR:.0e} (db {db}, accumulate {acc}, tile {rule})"
            outs[rule] = (got_w, got_b)
        assert torch.equal(outs["128"][0], outs["auto"][0]), f"dw of the wide tile is not bit-equal to 64 x 64 (db {db}, accumulate {acc})"
        if outs["auto"][1] is not None:
            assert torch.equal(outs["128"][1], outs["auto"][1]), f"db of the wide tile is not bit-equal to 64 x 64 (db {db}, accumulate {acc})"
