"""Edge shapes of the submanifold convolution and the kernel each of them must run on (test infrastructure, not collected).

One row per call of lotus_subm_conv / lotus_subm_conv_wgrad: `Row(id, call, scene, cin, cout, T, opts, route, why)`.  `route` is
what lotus_conv_last_route must report afterwards, Route(family, mode, rows, cols, prec, nz, tpz, aux) (fields:
include/lotus_hip.h); `why` names the branch the row is there to enter.

The routes are literals, written down from the dispatcher's documented rules and not computed with its code:
  * the pair-compacted kernel (3) takes T = 27 with packed weights, 16-byte aligned operands, KD % 32 == 0 and an output width
    of 64 (NCS 2: two 64-row tiles per block) or a multiple of 128 (NCS 4: one tile, 128 columns).  Its taps are split 9 ways
    (3 taps per block) while the grid is small: 3 ways from n = 32641 (ND 64), 16321 (128), 8129 (256), 4033 (512), 2689 (768),
    unsplit from 98177, 49089, 24513, 12225, 8129; a split needs a workspace of nz * n * ND floats.  Any of these missing ->
    the generic kernel (1), without a word;
  * bf16 / bf16x3 operands with KD % 64 == 0 go to the output-stationary kernel (4): 128-row blocks, 64 or 128 columns, KCH 128
    for precision 1 with KD % 128 == 0, else 64; at ND 768 it splits 3 ways from n = 1793 and not at all from 5377.
    LOTUS_CONV_OS=0 sends them to the pair kernel, LOTUS_CONV_OS_F32=1 sends exact fp32 products to (4);
  * the thin-input stem kernel (2) takes mode 0, cin <= 8, cout % 64 == 0, T <= 128 and a workspace of T * cin * cout floats;
  * the generic kernel (1) has 128-row tiles, 64 columns up to an output width of 64 and 128 above;
  * the weight gradient splits the rows in chunks of 1024; one chunk without `accumulate` writes dw / db directly (aux 1);
    cin <= 8 with cout % 64 == 0 and NO db is the stem kernel (8), bf16 operand modes are (7), the rest (6).

Scenes are the integer-grid builders of tests/edge_layouts.py (`el:<name>:<ksize>`) and SYNTHETIC neighbour tables: the entry
point's contract is a gather, so any int [T][n] table with entries in [-1, n) is a legal input
    fwd   y[i]  = b + add[i] + sum_t x[nbr[t][i]] w[:, t, :]^T        dgrad  the same with w[:, T-1-t, :]
    wgrad dw[c][t][k] = sum_p dy[p][c] x[nbr[t][p]][k],  db = colsum(dy)
with the centre tap kept fully active (the bias gradient and lotus_conv_dup_mask rely on it).  The overflow scenes construct
the number of distinct neighbour rows of a 64-row tile and tap range exactly; `phase_plan` restates the pair kernel's tiling
in numpy and tests/test_conv_phase_plan_host.py asserts each row's literal phase sequence against it, so the GPU rows enter
the branches they name.  tests/test_conv_routes_host.py asserts every route without a device; tests/test_gpu_conv_edges.py
runs the rows (tests/conv_run.py: references, bars)."""
import collections
import functools

import numpy as np

Route = collections.namedtuple("Route", "family mode rows cols prec nz tpz aux")
Row = collections.namedtuple("Row", "id call scene cin cout T opts route why")
Scene = collections.namedtuple("Scene", "nbr n extra")      # nbr int32 [T][n]; extra: builder-specific facts

GUARD = 64
MODE = {"fwd": 0, "dgrad": 1}
TPZ = {1: 27, 3: 9, 9: 3}
HT = 256               # resident rows (hash slots) per row tile of conv_pairs_kernel
WG_CHUNK = 1024        # rows per split of the weight gradient


def _gen(call, bn, T=27):
    return Route(1, MODE[call], 128, bn, 0, 1, T, 0)


def _stem(cin_t, T=125):
    return Route(2, 0, 32, 64, 0, 1, T, cin_t)


def _pairs(call, cols, nz, prec=0):
    return Route(3, MODE[call], 64, cols, prec, nz, TPZ[nz], 0)


def _os(call, cols, nz, prec, kch):
    return Route(4, MODE[call], 128, cols, prec, nz, TPZ[nz], kch)


def _wg(family, nsplit, direct, prec=0):
    return Route(family, 2, 64, 8 if family == 8 else 64, prec, nsplit, WG_CHUNK, direct)


# ---------------------------------------------------------------------------------------------------------- scenes
def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)


def _random_table(rng, n, T, p):
    """Centre tap = identity; every other entry present with probability p, naming a uniformly random row."""
    nbr = np.where(rng.random((T, n)) < p, rng.integers(0, n, size=(T, n)), -1).astype(np.int32)
    nbr[T // 2] = np.arange(n, dtype=np.int32)
    return nbr


def hash_bucket(ids):
    """Home slot of a row id in the pair kernel's table: bits 16 .. 23 of id * 2654435761 (mod 2^32)."""
    return ((np.asarray(ids, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(2 ** 32) >> np.uint64(16)) % np.uint64(HT)


def _fill_tile(nbr, tile, taps, ids):
    """Plant `ids` into the taps of one tile.  The even-numbered taps of the list are full (64 rows), the odd-numbered ones have
    a hole at every fourth row (48 rows, the holes shifting from tap to tap), so the k-th PAIR of a tap is not its k-th row: a
    phase after the first finds a pair's row only through the compacted row list.  The e-th active entry (tap-major) gets
    ids[e % len(ids)]: every id is used once there are at least len(ids) entries."""
    r, e = np.arange(64), 0
    for k, t in enumerate(taps):
        act = r if k % 2 == 0 else r[(r + k) % 4 != 0]
        col = np.full(64, -1, dtype=np.int32)
        col[act] = ids[(e + np.arange(len(act))) % len(ids)]
        nbr[t, tile * 64:tile * 64 + 64] = col
        e += len(act)


def _ids_257(rng, n):
    return rng.choice(np.arange(64, n), 257, replace=False).astype(np.int32)


def _plant_257(nbr, tile, ids):
    """Taps 0 .. 8 of the tile: 512 entries that cycle through ids 0 .. 255 (224 entries in taps 0 .. 3, 224 in 4 .. 7), the 257th
    id once in tap 4 (a full tap)."""
    _fill_tile(nbr, tile, range(9), ids[:256])
    nbr[4, tile * 64] = ids[256]


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> Scene.  Names: el:<edge_layouts scene>:<ksize> | rand:<n>:<T>:<percent> | emptytap:<n> | centreonly:<n> | ovf...  |
    solid21"""
    rng = np.random.default_rng(_seed(name))
    kind, *arg = name.split(":")
    if kind == "el":
        import edge_layouts as el
        from frontend_util import fe

        pc, counts, _ = el.conv_scenes(arg[0])
        rel = fe.grid_coord(pc[:, :3].numpy())
        batch = fe.offset2batch(counts)
        nbr = np.ascontiguousarray(fe.neighbour_table(rel, batch.astype(np.int32), int(arg[1])).T.astype(np.int32))
        extra = {}
        if arg[0] == "dups":
            ser = fe.serialization(rel, batch)
            extra = dict(code0=ser["code"][0].astype(np.int64), order0=ser["order"][0].astype(np.int32))
        return Scene(nbr, nbr.shape[1], extra)
    if kind == "rand":
        n, T, pct = int(arg[0]), int(arg[1]), int(arg[2])
        return Scene(_random_table(rng, n, T, pct / 100.0), n, {})
    if kind == "emptytap":       # tap 5 has no pair at all
        n = int(arg[0])
        nbr = _random_table(rng, n, 27, 0.3)
        nbr[5] = -1
        return Scene(nbr, n, dict(empty_tap=5))
    if kind == "centreonly":     # the second chunk of 1024 rows has its centre tap and nothing else
        n = int(arg[0])
        nbr = _random_table(rng, n, 27, 0.3)
        keep = nbr[13].copy()
        nbr[:, WG_CHUNK:2 * WG_CHUNK] = -1
        nbr[13] = keep
        return Scene(nbr, n, dict(bare_chunk=1))
    if kind in ("ovf256", "ovf257", "ovfempty"):        # ND 768: one tile per block, 43 tiles -> taps split 3 ways
        n = 2752
        nbr = _random_table(rng, n, 27, 0.05)
        if kind == "ovf256":
            _fill_tile(nbr, 0, range(9), rng.choice(np.arange(64, n), 256, replace=False).astype(np.int32))
        elif kind == "ovf257":
            _plant_257(nbr, 0, _ids_257(rng, n))
        else:                     # taps 0 .. 3 empty, taps 4 .. 8 with 64 / 48 / 64 / 48 / 64 rows, all 288 distinct
            nbr[0:4, 0:64] = -1
            _fill_tile(nbr, 0, range(4, 9), rng.choice(np.arange(64, n), 288, replace=False).astype(np.int32))
        return Scene(nbr, n, {})
    if kind == "ovfnz1":          # ND 768 from 8129 rows: all 27 taps in one block; tile 0 has 64 or 48 distinct rows in every tap, all different
        n = 8192
        nbr = _random_table(rng, n, 27, 0.05)
        ids = rng.choice(np.arange(64, n), 26 * 64, replace=False).astype(np.int32)
        _fill_tile(nbr, 0, [t for t in range(27) if t != 13], ids)
        return Scene(nbr, n, {})
    if kind == "ovfwrap":         # ND 256 from 8129 rows: taps split 3 ways; the 256 ids of tile 0 all hash into slots >= 192
        n = 8192
        nbr = _random_table(rng, n, 27, 0.05)
        good = np.nonzero(hash_bucket(np.arange(n)) >= 192)[0]
        ids = rng.choice(good[good >= 64], 256, replace=False).astype(np.int32)
        _fill_tile(nbr, 0, range(9), ids)
        return Scene(nbr, n, dict(qualifying=len(good), ids=ids))
    if kind == "ovfncs2":         # ND 64 from 32641 rows: two tiles per block share the overflow flag; 511 tiles + 10 rows
        n = 511 * 64 + 10
        nbr = _random_table(rng, n, 27, 0.03)
        for tile in (0, 3, 510):  # block 0: rt 0 overflows; block 1: rt 1; block 255: rt 0, next to the partial last tile
            _plant_257(nbr, tile, _ids_257(rng, n))
        return Scene(nbr, n, {})
    if kind == "solid21":         # a solid 21^3 block stored in random order: 9261 rows, every interior row has all 27 taps
        from frontend_util import fe

        g = np.stack(np.meshgrid(*[np.arange(21)] * 3, indexing="ij"), -1).reshape(-1, 3)
        g = g[rng.permutation(len(g))].astype(np.int32)
        batch = np.zeros(len(g), dtype=np.int64)
        nbr = np.ascontiguousarray(fe.neighbour_table(g, batch.astype(np.int32), 3).T.astype(np.int32))
        curve = fe.serialization(g, batch)["order"][0].astype(np.int32)
        return Scene(nbr, len(g), dict(curve=curve))
    raise KeyError(name)


def rowidx_of(row):
    """The processing order the row hands over: None, the identity, a random permutation or the scene's curve order."""
    how = row.opts.get("rowidx")
    sc = scene(row.scene)
    if how is None:
        return None
    if how == "identity":
        return np.arange(sc.n, dtype=np.int32)
    if how == "perm":
        return np.random.default_rng(_seed(row.scene) + 1).permutation(sc.n).astype(np.int32)
    if how == "curve":
        return sc.extra["curve"]
    raise KeyError(how)


def check_table(nbr):
    T, n = nbr.shape
    assert nbr.dtype == np.int32 and nbr.min() >= -1 and nbr.max() < n
    assert (nbr[T // 2] >= 0).all(), "the centre tap must be fully active"


# ------------------------------------------------------------------------------------- the pair kernel's tiling, restated
def distinct_rows(nbr, rows, t0, t1):
    v = nbr[t0:t1][:, rows]
    return int(np.unique(v[v >= 0]).size)


def phase_plan(nbr, rowidx, ND, nz, blocks=None):
    """conv_pairs_kernel's phases: 64-row tiles in `rowidx` order (two per block at ND 64, else one), tpz = ceil(T / nz) taps
    per blockIdx.z, one attempt per tap span; an attempt overflows when ANY row tile of the block names more than 256 distinct
    rows, the span is then halved (at least 1) and tried again from the same tap.  -> {(block, z): [taps of every attempt,
    negative where it overflowed]}."""
    T, n = nbr.shape
    tpz, nrt = -(-T // nz), 2 if ND == 64 else 1
    order = np.arange(n) if rowidx is None else np.asarray(rowidx)
    ntiles = -(-n // 64)
    out = {}
    for b in (range(-(-ntiles // nrt)) if blocks is None else blocks):
        tiles = [order[(b * nrt + rt) * 64:(b * nrt + rt) * 64 + 64] for rt in range(nrt)]
        for z in range(nz):
            t0, ze = z * tpz, min(T, (z + 1) * tpz)
            span, seq = ze - t0, []
            while t0 < ze:
                t1 = min(ze, t0 + span)
                worst = max([distinct_rows(nbr, r, t0, t1) for r in tiles if len(r) * (t1 - t0) > HT] or [0])
                if worst > HT:
                    seq.append(-(t1 - t0))
                    span = max(1, (t1 - t0) // 2)
                    continue
                seq.append(t1 - t0)
                t0 = t1
            out[(b, z)] = seq
    return out


# ------------------------------------------------------------------------------------------------------------ rows
EDGE = ["el:n1:3", "el:n63:3", "el:n64:3", "el:n65:3", "el:isolated:3", "el:line:3", "el:solid:3", "el:dups:3", "el:many_tiny:3"]
SHORT = {"el:n1:3": "n1", "el:n63:3": "n63", "el:n64:3": "n64", "el:n65:3": "n65", "el:isolated:3": "isolated", "el:line:3": "line",
         "el:solid:3": "solid", "el:dups:3": "dups", "el:many_tiny:3": "many_tiny", "el:solid:5": "solid5"}


def _sid(s):
    return SHORT.get(s, s.replace(":", "_"))


def _row(group, call, sc, cin, cout, route, why, T=27, tag="", **opts):
    rid = f"{group}-{call}-{_sid(sc)}-{cin}x{cout}" + (f"-{tag}" if tag else "")
    return Row(rid, call, sc, cin, cout, T, opts, route, why)


def _generic_rows():
    out = []
    scenes = ["el:n1:3", "el:n63:3", "el:n64:3", "el:n65:3", "rand:127:27:30", "rand:128:27:30", "rand:129:27:30", "el:isolated:3",
              "el:solid:3", "el:many_tiny:3"]
    orders = [None, "identity", "perm"]
    for i, sc in enumerate(scenes):       # the level-0 width of the shipped YAML: ND % 64 != 0 keeps it off the pair kernel
        for j, call in enumerate(("fwd", "dgrad")):
            o = orders[(i + j) % 3]
            out.append(_row("a", call, sc, 32, 32, _gen(call, 64), "32 -> 32: ND % 64 != 0 although packed weights and a workspace are "
                            f"given; column guard at 32 of a 64-column tile; rowidx {o}", tag=f"ri_{o}", w_t=1, ws="query", rowidx=o))
    out.append(_row("a", "dgrad", "el:dups:3", 32, 32, _gen("dgrad", 64), "duplicate voxels, mirrored taps only (the table as a gather)",
                    tag="mirror", rowidx="perm"))
    out.append(_row("a", "dgrad", "el:dups:3", 32, 32, _gen("dgrad", 64), "duplicate voxels through lotus_conv_dup_fold / _mask: the "
                    "gradient of the forward as computed", tag="fold", rowidx="perm", fold=1))
    for sc, T in (("rand:1:125:20", 125), ("el:n65:5", 125), ("rand:129:125:20", 125), ("el:solid:5", 125)):
        out.append(_row("a", "fwd", sc, 6, 32, _gen("fwd", 64, 125), "the YAML stem 6 -> 32 at 5^3: cout % 64 != 0 skips the thin-input "
                        "kernel although its workspace is given; KD 6 is one guarded 16-deep slab", T=T, ws="stem"))
    for sc in ("el:n1:3", "el:n65:3", "rand:129:27:30", "el:solid:3"):
        for call in ("fwd", "dgrad"):
            out.append(_row("a", call, sc, 96, 96, _gen(call, 128), "96 -> 96: BN 128 with the column guard at 96", w_t=1, ws="query"))
    for sc in ("el:n65:3", "rand:129:27:30", "el:solid:3"):
        out.append(_row("a", "fwd", sc, 64, 192, _gen("fwd", 128), "ND 192 > 64 and ND % 128 != 0: two column blocks, the second "
                        "half empty", w_t=1, ws="query", rowidx="perm"))
    for sc in ("el:n65:3", "el:solid:3"):
        for call in ("fwd", "dgrad"):
            out.append(_row("a", call, sc, 64, 64, _gen(call, 64), "64 -> 64 without packed weights", tag="no_wt", ws="query"))
            out.append(_row("a", call, sc, 64, 64, _gen(call, 64), "64 -> 64 with packed weights but no workspace: nine tap groups "
                            "need one, the call falls through to the generic kernel", tag="no_ws", w_t=1))
    return out


def _stem_rows():
    out = []
    tmpl = {4: 4, 5: 0, 6: 6, 7: 7, 8: 8}
    for cin in (4, 5, 6, 7, 8):
        for sc in ("rand:1:125:20", "rand:31:125:20", "rand:32:125:20", "rand:33:125:20", "el:solid:5"):
            out.append(_row("b", "fwd", sc, cin, 64, _stem(tmpl[cin]), f"CIN template {tmpl[cin]}; "
                            + ("125 active taps per interior row against STEM_TP = 128" if sc == "el:solid:5" else "a 32-row block boundary"),
                            T=125, ws="stem"))
        for sc in ("rand:33:125:20", "el:solid:5"):
            out.append(_row("b", "fwd", sc, cin, 128, _stem(tmpl[cin]), "a second column block", T=125, ws="stem"))
        out.append(_row("b", "fwd", "rand:33:125:20", cin, 32, _gen("fwd", 64, 125), "cout 32: the same call on the generic kernel",
                        T=125, ws="stem"))
    out.append(_row("b", "fwd", "rand:33:125:20", 7, 64, _gen("fwd", 64, 125), "no workspace: the stem call falls through to the generic "
                    "kernel", T=125, tag="no_ws"))
    return out


PAIR_WIDTHS = [(32, 64), (96, 64), (64, 128), (32, 256), (32, 512), (32, 768), (256, 128)]      # (KD, ND)
# rows at which tap_splits changes, per output width: (last row with 9 groups, first with 3), (last with 3, first with 1)
NZ_EDGES = {64: ((32640, 32641), (98176, 98177)), 128: ((16320, 16321), (49088, 49089)), 256: ((8128, 8129), (24512, 24513)),
            512: ((4032, 4033), (12224, 12225)), 768: ((2688, 2689), (8128, 8129))}


def _cc(call, kd, nd):
    return (kd, nd) if call == "fwd" else (nd, kd)


def _pair_rows():
    out = []
    for kd, nd in PAIR_WIDTHS:
        cols = 64 if nd == 64 else 128
        scenes = EDGE if (kd, nd) in ((32, 64), (64, 128)) else ["el:n1:3", "el:n65:3", "el:solid:3", "el:dups:3"]
        for i, sc in enumerate(scenes):
            for j, call in enumerate(("fwd", "dgrad")):
                o = [None, "perm", "identity"][(i + j) % 3]
                out.append(_row("c", call, sc, *_cc(call, kd, nd), _pairs(call, cols, 9),
                                f"KD {kd} -> ND {nd}: nkc = {kd // (32 if nd != 64 else 16)}, {nd // cols} column block(s), 9 tap groups "
                                f"of 3; rowidx {o}", tag=f"ri_{o}", w_t=1, ws="pairs", rowidx=o))
    for k in range(1, 8):    # gx = 3 column blocks: gridDim.x * gridDim.y = 3 k takes every residue mod 8 in 1 .. 7
        n = 64 * k - 7
        out.append(_row("c", "fwd", f"rand:{n}:27:30", 32, 384, _pairs("fwd", 128, 9), f"XCD remap with gx = 3 and {k} row tile(s): "
                        f"{3 * k} blocks per tap group, {3 * k % 8} mod 8; partial last tile", w_t=1, ws="pairs", rowidx="perm"))
    for nd, ((a9, a3), (b3, b1)) in NZ_EDGES.items():
        cols = 64 if nd == 64 else 128
        for n, nz in ((a9, 9), (a3, 3), (b3, 3), (b1, 1)):
            out.append(_row("c", "fwd", f"rand:{n}:27:8", 32, nd, _pairs("fwd", cols, nz), f"tap_splits boundary at ND {nd}: {n} rows -> "
                            f"{nz} group(s)" + ("; two row tiles per block" if nd == 64 else ""), w_t=1, ws="pairs"))
    for n, nz in ((2689, 3), (8129, 1)):
        out.append(_row("c", "dgrad", f"rand:{n}:27:8", 768, 32, _pairs("dgrad", 128, nz), f"input gradient at the ND 768 boundary: {nz} "
                        "group(s)", w_t=1, ws="pairs", rowidx="perm"))
    return out


def _overflow_rows():
    p3, p1 = _pairs("fwd", 128, 3), _pairs("fwd", 128, 1)
    out = [
        _row("d", "fwd", "ovf256", 32, 768, p3, "exactly 256 distinct rows in taps 0 .. 8 of tile 0: the table is full, one phase",
             w_t=1, ws="pairs", phases={(0, 0): [9]}, distinct={(0, 0, 9): 256}),
        _row("d", "fwd", "ovf257", 32, 768, p3, "257 distinct rows: one overflow, then phases of 4, 4 and 1 taps with the ids re-read "
             "from global memory", w_t=1, ws="pairs", phases={(0, 0): [-9, 4, 4, 1]}, distinct={(0, 0, 9): 257, (0, 0, 4): 224, (0, 4, 8): 224}),
        _row("d", "dgrad", "ovf257", 768, 32, _pairs("dgrad", 128, 3), "the same phases on the mirrored weights", w_t=1, ws="pairs",
             phases={(0, 0): [-9, 4, 4, 1]}, distinct={(0, 0, 9): 257}),
        _row("d", "fwd", "ovfnz1", 32, 768, p1, "all 27 taps in one block, 64 or 48 distinct rows per tap: 27 overflows to 13, 6, then "
             "nine phases of 3", w_t=1, phases={(0, 0): [-27, -13, -6] + [3] * 9},
             distinct={(0, 0, 27): 14 * 64 + 13 * 48, (0, 0, 13): 7 * 64 + 6 * 48, (0, 0, 6): 336, (0, 0, 3): 176, (0, 12, 15): 176}),
        _row("d", "fwd", "ovfempty", 64, 768, p3, "taps 0 .. 3 empty, 4 .. 8 with 64 or 48 rows each: the first half-phase has ngr == 0; "
             "nkc = 2 runs its fill loop once", w_t=1, ws="pairs", phases={(0, 0): [-9, 4, 4, 1]}, distinct={(0, 0, 9): 288, (0, 0, 4): 0, (0, 4, 8): 224}),
        _row("d", "fwd", "ovfempty", 96, 768, p3, "the same with nkc = 3: the ngr == 0 fill loop issues and stores twice", w_t=1,
             ws="pairs", phases={(0, 0): [-9, 4, 4, 1]}, distinct={(0, 0, 9): 288, (0, 0, 4): 0}),
        _row("d", "fwd", "ovfwrap", 32, 256, _pairs("fwd", 128, 3), "256 ids that all hash into slots >= 192: the probe chain wraps "
             "from 255 to 0; two column blocks walk the same tile", w_t=1, ws="pairs", phases={(0, 0): [9]}, distinct={(0, 0, 9): 256}),
    ]
    n2 = {(0, 0): [-9, 4, 4, 1], (1, 0): [-9, 4, 4, 1], (255, 0): [-9, 4, 4, 1], (2, 0): [9], (0, 1): [9]}
    for call in ("fwd", "dgrad"):
        out.append(_row("d", call, "ovfncs2", *_cc(call, 32, 64), _pairs(call, 64, 3), "two row tiles share one overflow flag: rt 0 "
                        "overflows in block 0, rt 1 in block 1, and the tile beside it is re-phased; block 255 overflows next to the "
                        "10-row last tile", w_t=1, ws="pairs", phases=n2, distinct={(0, 0, 9): 257, (1, 0, 9): None, (3, 0, 9): 257, (510, 0, 9): 257}))
    out.append(_row("d", "fwd", "solid21", 32, 256, _pairs("fwd", 128, 3), "a solid 21^3 block in random storage order: every 64-row "
                    "tile overflows in every tap group", w_t=1, ws="pairs", overflowing="all"))
    # (in curve order a tap group of 9 never overflows here — an aligned 64-row tile is a 4 x 4 x 4 cell with a 4 x 6 x 6 slab
    # per group — so the curve row runs all 27 taps in one block, ND 768: 11 of the 145 tiles straddle cells and overflow)
    out.append(_row("d", "fwd", "solid21", 32, 768, _pairs("fwd", 128, 1), "the same block in curve order through rowidx, all 27 taps "
                    "in one block: the tiles whose 64 rows straddle cells overflow (27 -> 13, 13, 1), the others fit", tag="curve", w_t=1,
                    rowidx="curve", overflowing=11))
    return out


OS_ENV = {"LOTUS_CONV_OS": "0"}          # child interpreter: the bf16 operand modes on the pair kernel
OSF32_ENV = {"LOTUS_CONV_OS_F32": "1"}   # child interpreter: exact fp32 products on the output-stationary kernel


def _prec_rows():
    out = []
    for prec in (1, 3):
        for kd, nd in [(32, 64), (96, 64), (32, 256), (96, 128)]:
            cols = 64 if nd == 64 else 128
            for sc in ("el:n1:3", "el:n65:3", "el:solid:3"):
                for call in ("fwd", "dgrad"):
                    out.append(_row("e", call, sc, *_cc(call, kd, nd), _pairs(call, cols, 9, prec), f"precision {prec} with KD % 64 != 0 "
                                    "stays on the pair kernel: " + ("hi-only" if prec == 1 else "hi + lo") + " packing and image",
                                    tag=f"p{prec}", w_t=1, ws="pairs", prec=prec, rowidx="perm"))
    return out


def _os_rows():
    out = []
    for prec in (1, 3):
        for kd, nd in [(64, 64), (128, 128), (64, 256), (128, 64)]:
            cols = 64 if nd == 64 else 128
            kch = 128 if (prec == 1 and kd % 128 == 0) else 64
            for sc in ("rand:1:27:30", "rand:127:27:30", "rand:128:27:30", "rand:129:27:30", "el:isolated:3", "el:solid:3"):
                for call in ("fwd", "dgrad") if sc in ("rand:129:27:30", "el:solid:3") else ("fwd",):
                    why = f"precision {prec}, KD {kd}: conv_os_kernel<{prec}, {cols // 32}, {kch}>"
                    if sc == "el:isolated:3":
                        why += "; the wave ballot skips 26 taps"
                    out.append(_row("e", call, sc, *_cc(call, kd, nd), _os(call, cols, 9, prec, kch), why, tag=f"p{prec}", w_t=1, ws="pairs",
                                    prec=prec, rowidx="perm", os0=_pairs(call, cols, 9, prec)))
        # os_splits at ND 768 (3 groups from 1793 rows, 1 from 5377); on the pair kernel the same rows split 9 / 9 / 3 / 3 ways
        for n, nz, nz0 in ((1792, 9, 9), (1793, 3, 9), (5376, 3, 3), (5377, 1, 3)) if prec == 1 else ((1793, 3, 9), (5377, 1, 3)):
            out.append(_row("e", "fwd", f"rand:{n}:27:8", 64, 768, _os("fwd", 128, nz, prec, 64), f"os_splits boundary: {n} rows -> {nz} "
                            "group(s)", tag=f"p{prec}", w_t=1, ws="pairs", prec=prec, os0=_pairs("fwd", 128, nz0, prec)))
    return out


def _osf32_rows():
    out = []
    for kd, nd in [(64, 64), (128, 128), (64, 256)]:
        cols = 64 if nd == 64 else 128
        for sc in ("rand:129:27:30", "el:solid:3"):
            for call in ("fwd", "dgrad"):
                out.append(_row("e", call, sc, *_cc(call, kd, nd), _pairs(call, cols, 9), "exact fp32 products: the pair kernel by default, "
                                f"conv_os_kernel<0, {cols // 32}, 64> under LOTUS_CONV_OS_F32=1", tag="f32", w_t=1, ws="pairs",
                                rowidx="perm", osf32=_os(call, cols, 9, 0, 64)))
    return out


WG_ROWS = [1, 255, 256, 1023, 1024, 1025, 2049]


def _wg_route(cin, cout, n, acc, db, prec=0):
    nsplit = -(-n // WG_CHUNK)
    direct = 1 if (nsplit == 1 and not acc) else 0
    if cin <= 8 and cout % 64 == 0 and db == "none":
        return _wg(8, nsplit, direct)
    return _wg(7 if prec else 6, nsplit, direct, prec)


def _wgrad_rows():
    out = []

    def add(n, cin, cout, acc, db, T=27, prec=0, sc=None, why=""):
        sc = sc or f"rand:{n}:{T}:{30 if T == 27 else 10}"
        r = _wg_route(cin, cout, n, acc, db, prec)
        text = (f"{n} rows: {r.nz} slab(s), " + ("written directly" if r.aux else "reduced") + f"; accumulate {acc}; db {db}"
                + ("; dw and db in ONE reduction" if (db == "tail" and not r.aux) else "") + (f"; {why}" if why else ""))
        out.append(_row("f", "wgrad", sc, cin, cout, r, text, T=T, tag=f"acc{acc}_db{db}" + (f"_p{prec}" if prec else ""),
                        accumulate=acc, db=db, prec=prec))

    for n in WG_ROWS:
        for acc in (0, 1):
            for db in ("none", "sep", "tail"):
                add(n, 32, 32, acc, db)
    for cin, cout, T in ((6, 32, 125), (96, 96, 27), (64, 192, 27), (256, 128, 27)):
        add(255, cin, cout, 0, "tail", T)
        add(1025, cin, cout, 0, "tail", T)
        add(2049, cin, cout, 1, "sep", T)
    for n, acc in ((255, 0), (1025, 0), (1025, 1)):
        add(n, 7, 64, acc, "none", 125, why="the thin-input kernel")
        add(n, 7, 64, acc, "tail", 125, why="with db the thin input runs on the MFMA kernel")
    add(33, 7, 128, 0, "none", 125, why="the thin-input kernel on two channel blocks")
    for prec in (1, 3):
        for cin, cout in ((32, 32), (96, 64), (64, 64)):
            add(255, cin, cout, 0, "tail", prec=prec)
            add(1025, cin, cout, 0, "tail", prec=prec)
        add(1025, 64, 64, 1, "sep", prec=prec)
    add(1025, 32, 32, 0, "tail", sc="emptytap:1025", why="tap 5 has no pair: its slice of dw is zero in both slabs")
    add(2049, 32, 32, 0, "tail", sc="centreonly:2049", why="the middle chunk has only its centre tap: 26 of its blocks see no pair")
    add(2049, 64, 64, 0, "tail", prec=1, sc="centreonly:2049", why="the same on the bf16 kernel")
    return out


def _twin_rows():
    """The bf16-storage twin (lotus_b16_*): activations bf16 in memory, weights and accumulation fp32; precision 1 as ops passes."""
    b = dict(b16=1, prec=1, w_t=1, ws="pairs", rowidx="perm")
    out = []
    for call in ("fwd", "dgrad"):
        out.append(_row("g", call, "el:n65:3", 32, 32, _gen(call, 64), "twin on the generic kernel", tag="b16", b16=1, prec=1, rowidx="perm"))
        out.append(_row("g", call, "el:solid:3", *_cc(call, 32, 64), _pairs(call, 64, 9, 1), "twin on the pair kernel, NCS 2", tag="b16", **b))
        out.append(_row("g", call, "rand:129:27:30", *_cc(call, 128, 128), _os(call, 128, 9, 1, 128), "twin on conv_os_kernel, KCH 128: the "
                        "loaded row bytes are the operand, two row stages in flight", tag="b16", **b))
    out.append(_row("g", "fwd", "el:solid:3", 64, 64, _os("fwd", 64, 9, 1, 64), "twin on conv_os_kernel, NS 2", tag="b16", **b))
    out.append(_row("g", "fwd", "el:n65:3", 32, 256, _pairs("fwd", 128, 9, 1), "twin on the pair kernel, NCS 4, two column blocks", tag="b16", **b))
    out.append(_row("g", "fwd", "ovf257", 32, 768, _pairs("fwd", 128, 3, 1), "twin through the overflow phases", tag="b16",
                    **dict(b, rowidx=None, phases={(0, 0): [-9, 4, 4, 1]}, distinct={(0, 0, 9): 257})))
    out.append(_row("g", "fwd", "el:n65:3", 64, 64, _pairs("fwd", 64, 9, 0), "a tap plan and exact products handed to the twin: the plan "
                    "is ignored (family 3, never 5)", tag="b16_plan_p0", **dict(b, prec=0, tap_plan=1)))
    out.append(_row("g", "fwd", "el:n65:3", 64, 64, _os("fwd", 64, 9, 1, 64), "a tap plan handed to the twin at precision 1: ignored "
                    "(family 4, never 5)", tag="b16_plan_p1", **dict(b, tap_plan=1)))
    out.append(_row("g", "wgrad", "rand:1025:27:30", 32, 32, _wg(7, 2, 0, 1), "twin weight gradient over two slabs, dw | db in one "
                    "reduction", tag="b16", b16=1, prec=1, accumulate=0, db="tail"))
    return out


def _refusal_rows():
    g = _gen("fwd", 64)    # (never recorded: a refusal leaves the record of the call before it)
    return [
        _row("h", "fwd", "el:n65:3", 64, 64, g, "precision 2 is refused before any launch", tag="prec2", w_t=1, ws="pairs", prec=2, refuse=-1),
        _row("h", "transpose", "el:n65:3", 48, 64, g, "lotus_conv_weight_transpose with cin 48: unsupported, nothing packed", tag="cin48",
             refuse=-3),
        _row("h", "fwd", "el:n65:3", 64, 64, g, "a tap plan with a workspace four bytes short of the partial slab: a hard error, not a "
             "fall-through", tag="plan_short_ws", w_t=1, tap_plan=1, ws="tap_short", refuse=-1),
    ]


GENERIC = _generic_rows()
STEM = _stem_rows()
PAIRS = _pair_rows()
OVERFLOW = _overflow_rows()
PREC = _prec_rows()
OS = _os_rows()
OSF32 = _osf32_rows()
WGRAD = _wgrad_rows()
TWIN = _twin_rows()
REFUSE = _refusal_rows()
GROUPS = dict(GENERIC=GENERIC, STEM=STEM, PAIRS=PAIRS, OVERFLOW=OVERFLOW, PREC=PREC, OS=OS, OSF32=OSF32, WGRAD=WGRAD, TWIN=TWIN)
TABLE = [r for g in GROUPS.values() for r in g]
BY_ID = {r.id: r for r in TABLE + REFUSE}
assert len(BY_ID) == len(TABLE) + len(REFUSE), [i for i, c in collections.Counter(r.id for r in TABLE + REFUSE).items() if c > 1]
GROUP_OF = {r.id: g for g, rows in GROUPS.items() for r in rows}


def expected_route(row, environ):
    """The row's route in a process with this environment (the switches are read once per process)."""
    if environ.get("LOTUS_CONV_OS") == "0" and "os0" in row.opts:
        return row.opts["os0"]
    if environ.get("LOTUS_CONV_OS_F32") == "1" and "osf32" in row.opts:
        return row.opts["osf32"]
    return row.route


# ---------------------------------------------------------------------------------------------------- the call itself
def dims(row):
    """-> (n, KD, ND) of a fwd / dgrad row."""
    n = scene(row.scene).n
    return (n, row.cin, row.cout) if row.call == "fwd" else (n, row.cout, row.cin)


def entry(row, name=None):
    name = name or ("lotus_subm_conv_wgrad" if row.call == "wgrad" else "lotus_subm_conv")
    return "lotus_b16_" + name[len("lotus_"):] if row.opts.get("b16") else name


def buffers(row):
    """-> {name: (rows, cols, written, kind)}; kind 'act' (bf16 in the twin) | 'f32'."""
    n, o = scene(row.scene).n, row.opts
    wsz = row.cout * row.T * row.cin
    if row.call == "wgrad":
        b = dict(dy=(n, row.cout, 0, "act"), x=(n, row.cin, 0, "act"))
        if o["db"] == "tail":
            b["dwdb"] = (wsz + row.cout, 1, 1, "f32")
        else:
            b["dw"] = (wsz, 1, 1, "f32")
            if o["db"] == "sep":
                b["db"] = (row.cout, 1, 1, "f32")
        return b
    n, kd, nd = dims(row)
    b = dict(x=(n, kd, 0, "act"), w=(wsz, 1, 0, "f32"), y=(n, nd, 1, "act"))
    if o.get("add", 1):
        b["add"] = (n, nd, 0, "act")
    if row.call == "fwd":
        b["bias"] = (1, nd, 0, "f32")
    if o.get("w_t"):
        b["w_t"] = (2 * wsz, 1, 0, "f32")
    return b


def workspace_bytes(row, query=None):
    """Bytes of the workspace the row hands over (0: a null pointer).  'pairs': nz * n * ND floats of the widest split among the
    row's routes, nothing when unsplit; 'stem': T * cin * cout floats; 'query': lotus_subm_conv_workspace (needs `query`);
    'tap_short': four bytes less than the tap-grouped slab; wgrad: lotus_subm_conv_wgrad_workspace."""
    n, o = scene(row.scene).n, row.opts
    if row.call == "wgrad":
        return query(entry(row, "lotus_subm_conv_wgrad_workspace"), n, row.T, row.cin, row.cout)
    how = o.get("ws")
    if how is None:
        return 0
    _, kd, nd = dims(row)
    if how == "pairs":
        nz = max(r.nz for r in (row.route, o.get("os0", row.route), o.get("osf32", row.route)))
        return nz * n * nd * 4 if nz > 1 else 0
    if how == "stem":
        return row.T * row.cin * row.cout * 4
    if how == "query":
        return query(entry(row, "lotus_subm_conv_workspace"), n, row.cin, row.cout)
    if how == "tap_short":
        return 27 * ((n + 63) // 64 * 64) * nd * 4 - 4
    raise KeyError(how)


def arguments(row, ptr, ws, ws_bytes):
    """The argument list of the entry point (without the stream).  ptr: {buffer name: pointer-like}; absent -> NULL."""
    n, o, g = scene(row.scene).n, row.opts, ptr.get
    if row.call == "wgrad":
        dw, db = (g("dwdb"), g("dwdb_db")) if "dwdb" in ptr else (g("dw"), g("db"))
        return (g("dy"), g("x"), dw, db, g("nbr"), n, row.T, row.cin, row.cout, o.get("accumulate", 0), o.get("prec", 0), ws, ws_bytes)
    return (MODE[row.call], g("x"), g("w"), g("w_t"), g("bias"), g("add"), g("y"), g("nbr"), g("rowidx"), n, row.T, row.cin, row.cout,
            o.get("prec", 0), g("tap_plan"), ws, ws_bytes)
