"""Edge shapes of the trajectory-head, label, cloud-max and elementwise kernels of csrc/pool_head.hip (test infrastructure, not
collected).

One row per shape: `Row(id, group, shape, opts, why)`; `why` names the branch the row is there to enter.  Groups:

  step      lotus_step_act_fwd / _bwd: shape (M, C); three steps (own bias, seed, dh, dbias) into one dbase, accumulate 0, 1, 1
  step0     ... with no rows            stepid   bias = 0, act = NONE: the forward is lotus_dropout
  mploss    lotus_mp_loss_fwd / _bwd: shape (B, T, nrot, ga)
  posce     lotus_pos_ce_fwd / _bwd: shape = rows per cloud; opts nb, tgt ('soft' | 'onehot' | 'zero'), scale
  tgt       lotus_pos_targets: shape = rows per cloud; opts nb, ld, kind, robot ('none' | 'seventh' | 'cloud'), far, ties
  dec       lotus_pos_decode_max: shape = rows per cloud; opts nb, ld, mode ('random' | 'ties' | 'first' | 'last')
  cloudmax  lotus_cloud_max_fwd / _bwd: shape = rows per cloud; opts C
  dropout / add / droppath   shape n or (M, C); opts p, x

tests/test_head_args_host.py runs self_check() and the input conditions without a device; tests/test_gpu_head_edges.py runs the
rows (tests/head_run.py: references, bars).  A retuned geometry (rows per block, splits, grid caps) makes self_check() fail on the
rows that name the edge: move the row so that it still enters the branch."""
import collections

Row = collections.namedtuple("Row", "id group shape opts why")

ACT_NONE, ACT_GELU, ACT_LEAKY = 0, 1, 2
# the geometry the rows are built around (csrc/pool_head.hip)
SA_ROWS, SA_FWD_CAP, EW_CAP, CM_SPLITS, SLICES, MP_THREADS, MP_MAX_B = 64, 8192, 4096, 8, 32, 256, 8192

# ------------------------------------------------------------------------------------------------- STEP
STEP_SHAPES = {4: [1, 64, 65, 300], 8: [65], 64: [4097], 128: [1, 7, 8, 9, 63, 64, 65, 128, 193], 256: [130], 1024: [1, 65]}
STEP_CAP = (16385, 512)
STEP_DROP = {(300, 4): 0.1, (65, 128): 0.1, (130, 256): 0.1, (4097, 64): 0.1, STEP_CAP: 0.1, (193, 128): 0.5}
STEP_ACT = {(128, 128): ACT_NONE, (65, 8): ACT_GELU}
STEP_TWIN = [(65, 128), (300, 4), (130, 256)]


def _step_why(M, C):
    lanes = 256 // (C // 4)
    blocks = -(-M // SA_ROWS)
    return f"{lanes} row lanes over {blocks} block(s) of {SA_ROWS} rows, last block {M - (blocks - 1) * SA_ROWS} row(s)"


def _step_rows():
    out = []
    for C, ms in STEP_SHAPES.items():
        for M in ms:
            o = dict(act=STEP_ACT.get((M, C), ACT_LEAKY), p=STEP_DROP.get((M, C), 0.0))
            if (M, C) in STEP_TWIN:
                o["b16"] = 1
            out.append(Row(f"step-{M}x{C}", "step", (M, C), o, _step_why(M, C)))
    M, C = STEP_CAP
    out.append(Row(f"step-{M}x{C}-cap", "step", (M, C), dict(act=ACT_LEAKY, p=STEP_DROP[STEP_CAP]),
                   "total4 = 2 097 280 > 8192 x 256: the last 128 quads in the stride pass; 257 backward blocks"))
    out.append(Row("step-0x128", "step0", (0, 128), dict(act=ACT_LEAKY, p=0.0), "no rows: out and dbase untouched, dbias zeroed"))
    out.append(Row("stepid-77x132", "stepid", (77, 132), dict(act=ACT_NONE, p=0.1), "bias 0, no activation: lotus_step_act_fwd is lotus_dropout"))
    return out


STEP = _step_rows()

# ------------------------------------------------------------------------------------------------- MPLOSS
MPLOSS = [
    Row("mp-1x1x1", "mploss", (1, 1, 1, 7), dict(mask="prefix"), "one cloud, one step, one rotation bin: lse = the logit, CE 0"),
    Row("mp-1x5x72", "mploss", (1, 5, 72, 7), dict(mask="prefix"), "one cloud: msum_b has one entry, the prefix is T long"),
    Row("mp-7x5x72-ga8", "mploss", (7, 5, 72, 8), dict(mask="prefix", b16=1), "ga = 8: openness at column 7, prefixes 1 .. T"),
    Row("mp-7x5x72-holes", "mploss", (7, 5, 72, 7), dict(mask="holes"), "masks with holes"),
    Row("mp-7x5x72-step0", "mploss", (7, 5, 72, 7), dict(mask="step0"), "every cloud active at step 0 only"),
    Row("mp-7x5x72-sat", "mploss", (7, 5, 72, 7), dict(mask="prefix", scale=30.0), "logits x 30: BCE and lse saturated, all finite"),
    Row("mp-85x1x72", "mploss", (85, 1, 72, 7), dict(mask="prefix"), "B T 3 = 255: one pass, one idle thread"),
    Row("mp-86x1x72", "mploss", (86, 1, 72, 7), dict(mask="prefix"), "B T 3 = 258: two threads take a second pass"),
    Row("mp-257x3x72", "mploss", (257, 3, 72, 7), dict(mask="prefix", b16=1), "B beyond the 256 threads that fill msum_b"),
    Row("mp-8192x1x2", "mploss", (8192, 1, 2, 7), dict(mask="prefix"), "the admitted LDS limit (32 KiB of msum_b)"),
]

# ------------------------------------------------------------------------------------------------- POSCE
POSCE_LAYOUTS = {"a": (1,), "b": (1, 2, 31, 32, 33), "c": (63, 64, 65, 257), "d": (4099,)}


def _posce(name, nb, why, **o):
    tag = "".join(f"-{k}{v}" for k, v in o.items() if k != "scale") + ("-x60" if "scale" in o else "")
    return Row(f"posce-{name}-nb{nb}{tag}", "posce", POSCE_LAYOUTS[name], dict(dict(tgt="soft", scale=1.0), nb=nb, **o), why)


POSCE = [
    _posce("a", 2, "one point, two bins: 31 of 32 slices empty"),
    _posce("b", 34, "clouds shorter than / around the 32 slices; nb = 34: a second bin pass with two lanes"),
    _posce("b", 30, "one-hot targets on short clouds", tgt="onehot"),
    _posce("b", 100, "nb = 100: four bin passes, the last with four lanes; one (cloud, axis) without target mass", tgt="zero"),
    _posce("c", 32, "slices of 1 - 9 points, nb = 32: exactly one bin pass"),
    _posce("c", 100, "logits x 60: exp(x - max) underflows off the maximum", scale=60.0),
    _posce("c", 30, "a (cloud, axis) whose target is all zero: loss 0, gradient exactly 0", tgt="zero"),
    _posce("d", 30, "one cloud of 4099 points: 128 or 129 points per slice, 16 - 17 steps of 8"),
    _posce("d", 2, "4099 points of two bins: 30 of 32 lanes idle"),
]

# ------------------------------------------------------------------------------------------------- LABELS
LABEL_LAYOUTS = {"a": (1,), "b": (1, 2, 31, 32, 33, 65), "c": (300,), "t": (5, 300)}


def _tgt(name, nb, ld, kind, robot, why, **o):
    tag = "".join(f"-{k}" for k in o)
    return Row(f"tgt-{name}-nb{nb}-ld{ld}-{kind}-{robot}{tag}", "tgt", LABEL_LAYOUTS[name], dict(nb=nb, ld=ld, kind=kind, robot=robot, **o), why)


def _dec(name, nb, ld, mode, why, **o):
    return Row(f"dec-{name}-nb{nb}-ld{ld}-{mode}" + ("-b16" if o.get("b16") else ""), "dec", LABEL_LAYOUTS[name], dict(nb=nb, ld=ld, mode=mode, **o), why)


LABELS = [
    _tgt("a", 2, 3, "plain", "none", "one point, two bins, row stride 3"),
    _tgt("a", 2, 7, "dist", "none", "one point, two bins, 'dist' weights"),
    _tgt("b", 30, 7, "plain", "seventh", "clouds shorter than the 32 slices; a seventh of the points are robot points"),
    _tgt("b", 30, 3, "dist", "seventh", "... 'dist', row stride 3"),
    _tgt("b", 100, 3, "plain", "cloud", "every point of one cloud is a robot point: the nearest candidate, a robot point, is the target"),
    _tgt("b", 100, 7, "dist", "cloud", "... 'dist'; nb = 100 > 32: four bin passes"),
    _tgt("b", 30, 7, "plain", "seventh", "one cloud whose gt is 3 m away: no weight, one-hot nearest candidate", far=1),
    _tgt("b", 2, 3, "dist", "none", "nb = 2 in a batch; one cloud 3 m away", far=1),
    _tgt("c", 30, 7, "dist", "seventh", "one cloud of 300 points"),
    _tgt("c", 100, 3, "plain", "none", "300 points of 100 bins"),
    _tgt("t", 30, 7, "plain", "none", "exact ties of the nearest candidate: bins of one point, points of one slice, slices, waves", ties=1),
    _tgt("t", 100, 3, "dist", "none", "exact ties, nb = 100, 'dist'", ties=1),
    _dec("a", 2, 3, "random", "one point, two bins"),
    _dec("b", 30, 7, "random", "clouds shorter than the 32 slices"),
    _dec("b", 100, 3, "random", "nb = 100, row stride 3"),
    _dec("c", 30, 7, "random", "one cloud of 300 points"),
    _dec("t", 30, 7, "ties", "equal maximal logits across lanes, half-waves, waves and slices: the first index wins"),
    _dec("t", 100, 3, "ties", "... and across bin passes of one lane (nb = 100)"),
    _dec("t", 30, 7, "last", "the maximum at the last bin of the last point"),
    _dec("t", 30, 3, "first", "the maximum at the first bin of the first point"),
    _dec("b", 30, 7, "random", "bf16 logits: the twin decodes the same coordinates", b16=1),
]

# ------------------------------------------------------------------------------------------------- CLOUDMAX
CM_COUNTS = (1, 7, 8, 9, 33, 255, 256, 257)
CM_WHY = {4: "one column quad: 31 of 32 quad lanes idle behind q * 4 < C", 64: "half a column group",
          132: "a second column group holding one quad", 768: "six column groups"}
CLOUDMAX = [Row(f"cloudmax-{C}" + ("-b16" if C == 132 else ""), "cloudmax", CM_COUNTS, dict(C=C, **({"b16": 1} if C == 132 else {})),
                CM_WHY[C] + "; clouds of 1 .. 257 rows around 8 splits x 32 row lanes") for C in (4, 64, 132, 768)]

# ------------------------------------------------------------------------------------------------- ELEMENTWISE
ELEMENTWISE = [
    Row("dropout-1", "dropout", 1, dict(p=0.1), "one element without a pair partner"),
    Row("dropout-1048576", "dropout", 1048576, dict(p=0.1), "exactly the 4096-block cap"),
    Row("dropout-1048577", "dropout", 1048577, dict(p=0.1), "the cap plus one: one element in the stride pass"),
    Row("dropout-1050001", "dropout", 1050001, dict(p=0.1), "above the cap, odd length: the last element has no pair partner"),
    Row("dropout-1050001-p0", "dropout", 1050001, dict(p=0.0), "p = 0: a copy"),
    Row("add-4", "add", 4, {}, "n = 4: one quad, one thread"),
    Row("add-4194308", "add", 4194308, {}, "n / 4 = 1 048 577 quads: the cap plus one"),
    Row("droppath-1x4", "droppath", (1, 4), dict(p=0.25, x=0), "one row of one quad, x null"),
    Row("droppath-1x4-p0", "droppath", (1, 4), dict(p=0.0, x=0), "p = 0, x null: a copy"),
    Row("droppath-4097x1024", "droppath", (4097, 1024), dict(p=0.25, x=1), "total4 = 1 048 832 above the cap, x given"),
    Row("droppath-4097x1024-p0", "droppath", (4097, 1024), dict(p=0.0, x=1), "p = 0 above the cap: x + branch"),
]

ROWS = STEP + MPLOSS + POSCE + LABELS + CLOUDMAX + ELEMENTWISE
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def slice_bounds(nn, s):
    """Points [p0, p1) of slice s of a cloud of nn points (pos_ce_part_kernel, pos_tgt_part_kernel, pos_argmax_part_kernel)."""
    return nn * s // SLICES, nn * (s + 1) // SLICES


def tie_sites(nn, nb):
    """Per axis, the (point, bin) sites of a tie row in a cloud of nn >= 300 points, the first of them the expected winner:
    axis 0: two bins of one point (two lanes; with nb > 32 also the second pass of the first lane) and the next point of the slice
    (the other half-wave); axis 1: points 0 and 2 of one slice (waves 0 and 1) and point 8 of it (the second step of wave 0);
    axis 2: points of slices 3, 17 and 31 (the last point of the cloud)."""
    assert nn >= 300 and nb >= 30
    a, _ = slice_bounds(nn, 5)
    b, b1 = slice_bounds(nn, 9)
    assert b1 - b >= 9
    j2 = [3 + 32] if nb > 35 else []
    return [[(a, 3), (a, 20)] + [(a, j) for j in j2] + [(a + 1, 3)],
            [(b, 7), (b + 2, 7), (b + 8, 7)],
            [(slice_bounds(nn, 3)[0] + 1, 11), (slice_bounds(nn, 17)[0], 11), (nn - 1, 11)]]


def self_check():
    """The edges the table promises, from its own numbers (runs on the CPU)."""
    ids = set(BY_ID)
    assert all(r.why and len(r.why) > 10 for r in ROWS)
    # STEP: widths 4 .. 1024 give 256 .. 1 row lanes; the row counts of the issue; dropout and activation spread
    assert {256 // (C // 4) for C in STEP_SHAPES} == {256, 128, 16, 8, 4, 1}
    assert STEP_SHAPES[128] == [1, 7, 8, 9, SA_ROWS - 1, SA_ROWS, SA_ROWS + 1, 2 * SA_ROWS, 3 * SA_ROWS + 1] and 256 // (128 // 4) == 8
    assert STEP_SHAPES[4] == [1, SA_ROWS, SA_ROWS + 1, 300] and 256 // (4 // 4) > SA_ROWS
    assert -(-4097 // SA_ROWS) == 65 > 4 * 16                        # lotus_reduce_parts: 16 partial lanes walk more than 4 each
    M, C = STEP_CAP
    assert M * C // 4 == 2097280 and SA_FWD_CAP * 256 == 2097152 and M * C // 4 - SA_FWD_CAP * 256 == 128 and -(-M // SA_ROWS) == 257
    ps = [r.opts["p"] for r in STEP if r.group == "step"]
    assert ps.count(0.1) >= 4 and ps.count(0.5) == 1 and ps.count(0.0) > 8
    acts = [r.opts["act"] for r in STEP if r.group == "step"]
    assert acts.count(ACT_NONE) == 1 and acts.count(ACT_GELU) == 1
    assert all(r.opts["p"] == 0.0 and r.opts["act"] == ACT_LEAKY for r in STEP if r.group == "step" and r.shape[0] < SA_ROWS)
    assert {r.shape for r in STEP if r.opts.get("b16")} == set(STEP_TWIN) == {(65, 128), (300, 4), (130, 256)}
    assert all(256 % (r.shape[1] // 4) == 0 for r in STEP if r.group in ("step", "step0"))
    assert {"step-0x128", "stepid-77x132"} <= ids
    # MPLOSS
    shapes = [r.shape for r in MPLOSS]
    for s in [(1, 1, 1, 7), (1, 5, 72, 7), (7, 5, 72, 8), (85, 1, 72, 7), (86, 1, 72, 7), (257, 3, 72, 7), (8192, 1, 2, 7)]:
        assert s in shapes, s
    assert 85 * 3 == MP_THREADS - 1 and 86 * 3 == MP_THREADS + 2 and 257 > MP_THREADS and 8192 == MP_MAX_B
    assert {r.opts["mask"] for r in MPLOSS} == {"prefix", "holes", "step0"}
    assert [r.shape for r in MPLOSS if r.opts.get("scale") == 30.0] == [(7, 5, 72, 7)]
    assert {r.shape for r in MPLOSS if r.opts.get("b16")} == {(7, 5, 72, 8), (257, 3, 72, 7)}
    # POSCE
    assert set(POSCE_LAYOUTS.values()) == {(1,), (1, 2, 31, 32, 33), (63, 64, 65, 257), (4099,)}
    assert {r.shape for r in POSCE} == set(POSCE_LAYOUTS.values()) and {r.opts["nb"] for r in POSCE} == {2, 30, 32, 34, 100}
    assert {r.opts["tgt"] for r in POSCE} == {"soft", "onehot", "zero"} and [r.opts["scale"] for r in POSCE].count(60.0) == 1
    assert any(r.shape == (1,) and r.opts["nb"] == 2 for r in POSCE) and 34 - SLICES == 2
    # LABELS
    tg, dc = [r for r in LABELS if r.group == "tgt"], [r for r in LABELS if r.group == "dec"]
    assert {r.shape for r in tg} >= {(1,), (1, 2, 31, 32, 33, 65), (300,)} and {r.opts["nb"] for r in tg} == {2, 30, 100}
    assert {r.opts["ld"] for r in tg} == {3, 7} and {r.opts["kind"] for r in tg} == {"plain", "dist"}
    assert {r.opts["robot"] for r in tg} == {"none", "seventh", "cloud"}
    assert any(r.opts.get("far") for r in tg) and sum(1 for r in tg if r.opts.get("ties")) >= 2
    assert any(r.opts.get("far") and r.opts["nb"] == 2 and len(r.shape) > 1 for r in tg)
    assert {r.opts["mode"] for r in dc} == {"random", "ties", "first", "last"} and sum(1 for r in dc if r.opts.get("b16")) == 1
    assert {r.opts["ld"] for r in dc} == {3, 7} and {r.opts["nb"] for r in dc} == {2, 30, 100}
    for nb in (30, 100):
        sites = tie_sites(300, nb)
        sl = lambda p: [s for s in range(SLICES) if slice_bounds(300, s)[0] <= p < slice_bounds(300, s)[1]][0]  # noqa: E731
        grp = lambda p: (p - slice_bounds(300, sl(p))[0]) % 8  # noqa: E731
        (p0, j0), (p1, j1) = sites[0][0], sites[0][1]
        assert p0 == p1 and j0 % 32 != j1 % 32                                                   # two lanes of one half-wave
        assert sl(sites[0][-1][0]) == sl(p0) and grp(sites[0][-1][0]) == grp(p0) + 1 and grp(p0) % 2 == 0   # the other half-wave
        pa, pb, pc = (s[0] for s in sites[1])
        assert sl(pa) == sl(pb) == sl(pc) and grp(pa) // 2 != grp(pb) // 2 and grp(pa) == grp(pc) and pc - pa == 8
        assert len({sl(p) for p, _ in sites[2]}) == 3 and sites[2][-1][0] == 299
        assert all(site[0] == min(site) for site in sites)                                       # the winner is the first index
    assert [3 + 32] == [j for _, j in tie_sites(300, 100)[0] if j >= 32]
    # CLOUDMAX
    assert {r.opts["C"] for r in CLOUDMAX} == {4, 64, 132, 768} and all(r.shape == (1, 7, 8, 9, 33, 255, 256, 257) for r in CLOUDMAX)
    assert CM_SPLITS * 32 == 256 and [r.opts["C"] for r in CLOUDMAX if r.opts.get("b16")] == [132] and -(-132 // 128) == 2
    # ELEMENTWISE
    assert {r.shape for r in ELEMENTWISE if r.group == "dropout"} == {1, EW_CAP * 256, EW_CAP * 256 + 1, 1050001}
    assert {r.opts["p"] for r in ELEMENTWISE if r.group == "dropout"} == {0.1, 0.0}
    assert {r.shape for r in ELEMENTWISE if r.group == "add"} == {4, 4 * (EW_CAP * 256 + 1)}
    dp = [r for r in ELEMENTWISE if r.group == "droppath"]
    assert {r.shape for r in dp} == {(1, 4), (4097, 1024)} and 4097 * 1024 // 4 == 1048832 > EW_CAP * 256
    assert {(r.opts["p"], r.opts["x"]) for r in dp} == {(0.25, 0), (0.0, 0), (0.25, 1), (0.0, 1)}
    return len(ROWS)
