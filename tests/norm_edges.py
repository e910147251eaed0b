"""Edge shapes of the normalisation kernels and the launch plan each of them must land in (test infrastructure, not collected).

One row per shape: `Row(id, family, shape, C, opts)`; `shape` is the row count M (ln, bn, silu: the element count) or the rows
per cloud (ada).  PLAN[id] holds, as literal numbers, what lotus_norm_plan / lotus_adanorm_plan must report for the row: the
branch the row is there to enter (csrc/norm.hip, csrc/adanorm.hip):

  ln_fwd  (lanes per row, quads per lane, rows per block, grid)              16 / 32 / 64 lanes, 1 - 4 quads
  ln_bwd  (lanes per row, quads per lane, rows per block, grid, passes)      4 - 64 lanes; grid = partial rows of the parameter
                                                                             reduction, capped at 1024 (then passes > 1)
  bn2/bn3 (row slots, threads per row, column slabs, grid, groups, rows every slot walks, slots that walk one more): the
          statistics in two launches (grid <= 512) and fused (grid <= 256 in groups of 16; the forward walk is unrolled 8 rows
          deep, the backward walk 2)
  bn_apply (grid, blocks per column period, cap hit)
  ada     (chunks per cloud G, elementwise grid, column-period grid, cap hit, lanes per row, quads per lane of the LayerNorm
          site: 0, 0 where it refuses the width)

tests/test_norm_plan_host.py asserts PLAN on a machine without a device; tests/test_gpu_norm_edges.py runs the rows
(tests/norm_run.py).  A retuned geometry makes the host test fail on the rows that name the edge: move the row's shape so that
it still enters the branch, then update the numbers."""
import collections

Row = collections.namedtuple("Row", "id family shape C opts")

GUARD = 64
ACT_NONE, ACT_GELU, ACT_LEAKY = 0, 1, 2
KIND = {"ln_fwd": 0, "ln_bwd": 1, "bn2": 2, "bn3": 3, "bn_apply": 4}
LN_EPS, BN_EPS, BN_MOMENTUM = 1e-5, 1e-3, 0.01
DROP_P = 0.1

# ------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = [4, 12, 64, 68, 128, 132, 256, 260, 512, 516, 768, 1024]   # both sides of every lane rule
LN_REFUSED = [1028, 66, 0]
FULL = dict(res=1, add=1)
# rows per block of (forward, backward): 64 -> (16, 64), 128 -> (8, 32), 768 -> (4, 4); M = 0, 1, each count - 1 / + 0 / + 1,
# and 2 x the backward count + 1 (a second block of the backward)
LN_ROWS = {64: [0, 1, 15, 16, 17, 63, 64, 65, 129], 128: [0, 1, 7, 8, 9, 31, 32, 33, 65], 768: [0, 1, 3, 4, 5, 9]}
LN_CAPPED = [(8193, 768), (8209, 768), (131073, 64)]
LN_VARIANTS = {"plain": dict(), "res": dict(res=1), "add": dict(add=1), "nostat": dict(res=1, add=1, nostat=1),
               "acc": dict(res=1, add=1, accumulate=1)}
LN_OPTION_WIDTHS = [64, 768, 132]
LN_PARTS = [1, 31, 32, 33, 127, 128, 129, 1024]   # partial rows of colpart_reduce_kernel at C = 768: M = 8 x parts


def _ln_rows():
    out = [Row(f"ln-300x{C}", "ln", 300, C, dict(FULL)) for C in LN_WIDTHS]
    for C, ms in LN_ROWS.items():
        out += [Row(f"ln-{M}x{C}", "ln", M, C, dict(FULL)) for M in ms]
    out += [Row(f"ln-{M}x{C}-capped", "ln", M, C, dict(FULL, deferred=1)) for M, C in LN_CAPPED]
    for C in LN_OPTION_WIDTHS:
        out += [Row(f"ln-77x{C}-{name}", "ln", 77, C, dict(o)) for name, o in LN_VARIANTS.items()]
        out.append(Row(f"ln-300x{C}-deferred", "ln", 300, C, dict(FULL, deferred=1)))
        out.append(Row(f"ln-300x{C}-dz", "ln", 300, C, dict(FULL, dz=1)))
    out.append(Row("ln-77x768-deferred-acc", "ln", 77, 768, dict(FULL, deferred=1, accumulate=1)))
    out.append(Row("ln-8193x768-dz", "ln", 8193, 768, dict(FULL, dz=1)))
    out += [Row(f"ln-parts{n}", "ln", 8 * n, 768, dict(deferred=1)) for n in LN_PARTS]
    return out


LN = _ln_rows()

# ------------------------------------------------------------------------------------------------- BatchNorm
# fused statistics at C = 768 (one row slot per block, 16 rows per block): grids 1, 1, 1, 2, 16, 16, 17, 17, 18, 255, 256, 256, and
# twice the 256 cap; groups 1, 2 and 16; 8193: the 512 cap of the two-launch grid; 10923: the 4096 cap of the apply grid; 4, 5, 6:
# with the rest, every count of rows left over by the walk that is unrolled 8 deep
BN_768 = [1, 2, 16, 17, 241, 256, 257, 272, 273, 4080, 4081, 4096, 4097, 8209, 8193, 10923, 4, 5, 6]
BN_OTHER = {64: [1, 255, 256, 257, 4097], 256: [65, 1025], 28: [35, 36, 37], 1028: [17, 300], 60: [300], 132: [300]}
BN_ACT_ROWS = [(257, 768), (37, 28), (4097, 64)]   # these also run without activation and with LeakyReLU


def _bn_rows():
    out = [Row(f"bn-{M}x768", "bn", M, 768, dict(act=ACT_GELU)) for M in BN_768]
    for C, ms in BN_OTHER.items():
        out += [Row(f"bn-{M}x{C}", "bn", M, C, dict(act=ACT_GELU)) for M in ms]
    for M, C in BN_ACT_ROWS:
        out += [Row(f"bn-{M}x{C}-act{a}", "bn", M, C, dict(act=a)) for a in (ACT_NONE, ACT_LEAKY)]
    out += [Row(f"bn-0x{C}-two-launch", "bn0", 0, C, dict(act=ACT_GELU)) for C in (64, 768)]
    return out


BN = _bn_rows()

# ------------------------------------------------------------------------------------------------- AdaNorm (fp32 only)
ADA_LAYOUTS = {"b1": (7,), "b2": (7, 9), "b3": (7, 9, 1), "b4": (7, 9, 1, 30), "b5": (7, 9, 1, 30, 2),   # the four cloud lanes
               "tiny100": (3,) * 100,
               "chunks2": (700, 1, 200),          # G = 2: the 1-row cloud has an empty chunk
               "empty1": (0, 5, 0, 0, 300, 0),    # G = 1
               "empty2": (0, 1500, 0, 37)}        # G = 2: dmod of the empty clouds exactly zero
ADA_WIDTHS = [4, 64, 68, 128, 260, 768, 1024, 1028]   # on chunks2; 1028: BatchNorm only, the LayerNorm refuses it


def _ada_rows():
    out = []
    for name, counts in ADA_LAYOUTS.items():
        out += [Row(f"ada-{name}x{C}", "ada", counts, C, {}) for C in (64, 260) if not (name == "chunks2" and C == 64)]
    out += [Row(f"ada-chunks2x{C}", "ada", ADA_LAYOUTS["chunks2"], C, {}) for C in ADA_WIDTHS if C != 260]
    out.append(Row("ada-chunks63x64", "ada", (16128,), 64, {}))
    out.append(Row("ada-chunks64capx64", "ada", (16385,), 64, {}))
    out.append(Row("ada-applycapx768", "ada", (10923,), 768, {}))
    return out


ADA = _ada_rows()
SILU = [Row(f"silu-{n}", "silu", n, 0, {}) for n in (1, 255, 257, 262147)]   # 262147: the grid-stride loop behind 1024 blocks

# ------------------------------------------------------------------------------------------------- bf16-storage twin
TWIN = ([Row(f"b16-ln-300x{C}", "ln", 300, C, dict(FULL, b16=1, dz=1)) for C in (64, 68, 132, 516, 768)] +
        [Row("b16-ln-8193x768-capped", "ln", 8193, 768, dict(FULL, b16=1))] +
        [Row(f"b16-bn-{M}x768", "bn", M, 768, dict(act=ACT_GELU, b16=1)) for M in (1, 17, 257, 4097)] +
        [Row(f"b16-bn-{M}x28", "bn", M, 28, dict(act=ACT_GELU, b16=1)) for M in (35, 36, 37)] +
        [Row("b16-bn-4097x64", "bn", 4097, 64, dict(act=ACT_GELU, b16=1)), Row("b16-bn-300x1028", "bn", 300, 1028, dict(act=ACT_GELU, b16=1))])

ROWS = LN + BN + ADA + SILU + TWIN
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def rows_of(row):
    """M of a row (the sum over its clouds)."""
    return sum(row.shape) if row.family == "ada" else row.shape


def plan_queries(row):
    """-> [(plan key, entry point, arguments before `out`)] of the row."""
    if row.family == "ln":
        return [(k, "lotus_norm_plan", (KIND[k], row.shape, row.C)) for k in ("ln_fwd", "ln_bwd")]
    if row.family == "bn":
        return [(k, "lotus_norm_plan", (KIND[k], row.shape, row.C)) for k in ("bn2", "bn3", "bn_apply")]
    if row.family == "bn0":
        return [("bn2", "lotus_norm_plan", (KIND["bn2"], 0, row.C))]
    if row.family == "ada":
        return [("ada", "lotus_adanorm_plan", (rows_of(row), len(row.shape), row.C))]
    return []


PLAN_FIELDS = {"ln_fwd": 4, "ln_bwd": 5, "bn2": 7, "bn3": 7, "bn_apply": 3, "ada": 6}

# BEGIN PLAN (literal numbers; see the module docstring)
PLAN = {
    'ln-300x4': {'ln_fwd': (16, 1, 16, 19), 'ln_bwd': (4, 1, 64, 3, 2)},
    'ln-300x12': {'ln_fwd': (16, 1, 16, 19), 'ln_bwd': (4, 1, 64, 3, 2)},
    'ln-300x64': {'ln_fwd': (16, 1, 16, 19), 'ln_bwd': (4, 4, 64, 3, 2)},
    'ln-300x68': {'ln_fwd': (32, 1, 8, 38), 'ln_bwd': (8, 3, 32, 5, 2)},
    'ln-300x128': {'ln_fwd': (32, 1, 8, 38), 'ln_bwd': (8, 4, 32, 5, 2)},
    'ln-300x132': {'ln_fwd': (64, 1, 4, 75), 'ln_bwd': (16, 3, 16, 10, 2)},
    'ln-300x256': {'ln_fwd': (64, 1, 4, 75), 'ln_bwd': (16, 4, 16, 10, 2)},
    'ln-300x260': {'ln_fwd': (64, 2, 4, 75), 'ln_bwd': (32, 3, 8, 19, 2)},
    'ln-300x512': {'ln_fwd': (64, 2, 4, 75), 'ln_bwd': (32, 4, 8, 19, 2)},
    'ln-300x516': {'ln_fwd': (64, 3, 4, 75), 'ln_bwd': (64, 3, 4, 38, 2)},
    'ln-300x768': {'ln_fwd': (64, 3, 4, 75), 'ln_bwd': (64, 3, 4, 38, 2)},
    'ln-300x1024': {'ln_fwd': (64, 4, 4, 75), 'ln_bwd': (64, 4, 4, 38, 2)},
    'ln-0x64': {'ln_fwd': (16, 1, 16, 0), 'ln_bwd': (4, 4, 64, 1, 0)},
    'ln-1x64': {'ln_fwd': (16, 1, 16, 1), 'ln_bwd': (4, 4, 64, 1, 1)},
    'ln-15x64': {'ln_fwd': (16, 1, 16, 1), 'ln_bwd': (4, 4, 64, 1, 1)},
    'ln-16x64': {'ln_fwd': (16, 1, 16, 1), 'ln_bwd': (4, 4, 64, 1, 1)},
    'ln-17x64': {'ln_fwd': (16, 1, 16, 2), 'ln_bwd': (4, 4, 64, 1, 1)},
    'ln-63x64': {'ln_fwd': (16, 1, 16, 4), 'ln_bwd': (4, 4, 64, 1, 1)},
    'ln-64x64': {'ln_fwd': (16, 1, 16, 4), 'ln_bwd': (4, 4, 64, 1, 1)},
    'ln-65x64': {'ln_fwd': (16, 1, 16, 5), 'ln_bwd': (4, 4, 64, 1, 2)},
    'ln-129x64': {'ln_fwd': (16, 1, 16, 9), 'ln_bwd': (4, 4, 64, 2, 2)},
    'ln-0x128': {'ln_fwd': (32, 1, 8, 0), 'ln_bwd': (8, 4, 32, 1, 0)},
    'ln-1x128': {'ln_fwd': (32, 1, 8, 1), 'ln_bwd': (8, 4, 32, 1, 1)},
    'ln-7x128': {'ln_fwd': (32, 1, 8, 1), 'ln_bwd': (8, 4, 32, 1, 1)},
    'ln-8x128': {'ln_fwd': (32, 1, 8, 1), 'ln_bwd': (8, 4, 32, 1, 1)},
    'ln-9x128': {'ln_fwd': (32, 1, 8, 2), 'ln_bwd': (8, 4, 32, 1, 1)},
    'ln-31x128': {'ln_fwd': (32, 1, 8, 4), 'ln_bwd': (8, 4, 32, 1, 1)},
    'ln-32x128': {'ln_fwd': (32, 1, 8, 4), 'ln_bwd': (8, 4, 32, 1, 1)},
    'ln-33x128': {'ln_fwd': (32, 1, 8, 5), 'ln_bwd': (8, 4, 32, 1, 2)},
    'ln-65x128': {'ln_fwd': (32, 1, 8, 9), 'ln_bwd': (8, 4, 32, 2, 2)},
    'ln-0x768': {'ln_fwd': (64, 3, 4, 0), 'ln_bwd': (64, 3, 4, 1, 0)},
    'ln-1x768': {'ln_fwd': (64, 3, 4, 1), 'ln_bwd': (64, 3, 4, 1, 1)},
    'ln-3x768': {'ln_fwd': (64, 3, 4, 1), 'ln_bwd': (64, 3, 4, 1, 1)},
    'ln-4x768': {'ln_fwd': (64, 3, 4, 1), 'ln_bwd': (64, 3, 4, 1, 1)},
    'ln-5x768': {'ln_fwd': (64, 3, 4, 2), 'ln_bwd': (64, 3, 4, 1, 2)},
    'ln-9x768': {'ln_fwd': (64, 3, 4, 3), 'ln_bwd': (64, 3, 4, 2, 2)},
    'ln-8193x768-capped': {'ln_fwd': (64, 3, 4, 2049), 'ln_bwd': (64, 3, 4, 1024, 3)},
    'ln-8209x768-capped': {'ln_fwd': (64, 3, 4, 2053), 'ln_bwd': (64, 3, 4, 1024, 3)},
    'ln-131073x64-capped': {'ln_fwd': (16, 1, 16, 8193), 'ln_bwd': (4, 4, 64, 1024, 3)},
    'ln-77x64-plain': {'ln_fwd': (16, 1, 16, 5), 'ln_bwd': (4, 4, 64, 1, 2)},
    'ln-77x64-res': {'ln_fwd': (16, 1, 16, 5), 'ln_bwd': (4, 4, 64, 1, 2)},
    'ln-77x64-add': {'ln_fwd': (16, 1, 16, 5), 'ln_bwd': (4, 4, 64, 1, 2)},
    'ln-77x64-nostat': {'ln_fwd': (16, 1, 16, 5), 'ln_bwd': (4, 4, 64, 1, 2)},
    'ln-77x64-acc': {'ln_fwd': (16, 1, 16, 5), 'ln_bwd': (4, 4, 64, 1, 2)},
    'ln-300x64-deferred': {'ln_fwd': (16, 1, 16, 19), 'ln_bwd': (4, 4, 64, 3, 2)},
    'ln-300x64-dz': {'ln_fwd': (16, 1, 16, 19), 'ln_bwd': (4, 4, 64, 3, 2)},
    'ln-77x768-plain': {'ln_fwd': (64, 3, 4, 20), 'ln_bwd': (64, 3, 4, 10, 2)},
    'ln-77x768-res': {'ln_fwd': (64, 3, 4, 20), 'ln_bwd': (64, 3, 4, 10, 2)},
    'ln-77x768-add': {'ln_fwd': (64, 3, 4, 20), 'ln_bwd': (64, 3, 4, 10, 2)},
    'ln-77x768-nostat': {'ln_fwd': (64, 3, 4, 20), 'ln_bwd': (64, 3, 4, 10, 2)},
    'ln-77x768-acc': {'ln_fwd': (64, 3, 4, 20), 'ln_bwd': (64, 3, 4, 10, 2)},
    'ln-300x768-deferred': {'ln_fwd': (64, 3, 4, 75), 'ln_bwd': (64, 3, 4, 38, 2)},
    'ln-300x768-dz': {'ln_fwd': (64, 3, 4, 75), 'ln_bwd': (64, 3, 4, 38, 2)},
    'ln-77x132-plain': {'ln_fwd': (64, 1, 4, 20), 'ln_bwd': (16, 3, 16, 3, 2)},
    'ln-77x132-res': {'ln_fwd': (64, 1, 4, 20), 'ln_bwd': (16, 3, 16, 3, 2)},
    'ln-77x132-add': {'ln_fwd': (64, 1, 4, 20), 'ln_bwd': (16, 3, 16, 3, 2)},
    'ln-77x132-nostat': {'ln_fwd': (64, 1, 4, 20), 'ln_bwd': (16, 3, 16, 3, 2)},
    'ln-77x132-acc': {'ln_fwd': (64, 1, 4, 20), 'ln_bwd': (16, 3, 16, 3, 2)},
    'ln-300x132-deferred': {'ln_fwd': (64, 1, 4, 75), 'ln_bwd': (16, 3, 16, 10, 2)},
    'ln-300x132-dz': {'ln_fwd': (64, 1, 4, 75), 'ln_bwd': (16, 3, 16, 10, 2)},
    'ln-77x768-deferred-acc': {'ln_fwd': (64, 3, 4, 20), 'ln_bwd': (64, 3, 4, 10, 2)},
    'ln-8193x768-dz': {'ln_fwd': (64, 3, 4, 2049), 'ln_bwd': (64, 3, 4, 1024, 3)},
    'ln-parts1': {'ln_fwd': (64, 3, 4, 2), 'ln_bwd': (64, 3, 4, 1, 2)},
    'ln-parts31': {'ln_fwd': (64, 3, 4, 62), 'ln_bwd': (64, 3, 4, 31, 2)},
    'ln-parts32': {'ln_fwd': (64, 3, 4, 64), 'ln_bwd': (64, 3, 4, 32, 2)},
    'ln-parts33': {'ln_fwd': (64, 3, 4, 66), 'ln_bwd': (64, 3, 4, 33, 2)},
    'ln-parts127': {'ln_fwd': (64, 3, 4, 254), 'ln_bwd': (64, 3, 4, 127, 2)},
    'ln-parts128': {'ln_fwd': (64, 3, 4, 256), 'ln_bwd': (64, 3, 4, 128, 2)},
    'ln-parts129': {'ln_fwd': (64, 3, 4, 258), 'ln_bwd': (64, 3, 4, 129, 2)},
    'ln-parts1024': {'ln_fwd': (64, 3, 4, 2048), 'ln_bwd': (64, 3, 4, 1024, 2)},
    'bn-1x768': {'bn2': (1, 192, 1, 1, 0, 1, 0), 'bn3': (1, 192, 1, 1, 1, 1, 0), 'bn_apply': (3, 3, 0)},
    'bn-2x768': {'bn2': (1, 192, 1, 1, 0, 2, 0), 'bn3': (1, 192, 1, 1, 1, 2, 0), 'bn_apply': (3, 3, 0)},
    'bn-16x768': {'bn2': (1, 192, 1, 1, 0, 16, 0), 'bn3': (1, 192, 1, 1, 1, 16, 0), 'bn_apply': (6, 3, 0)},
    'bn-17x768': {'bn2': (1, 192, 1, 2, 0, 8, 1), 'bn3': (1, 192, 1, 2, 1, 8, 1), 'bn_apply': (9, 3, 0)},
    'bn-241x768': {'bn2': (1, 192, 1, 16, 0, 15, 1), 'bn3': (1, 192, 1, 16, 1, 15, 1), 'bn_apply': (93, 3, 0)},
    'bn-256x768': {'bn2': (1, 192, 1, 16, 0, 16, 0), 'bn3': (1, 192, 1, 16, 1, 16, 0), 'bn_apply': (96, 3, 0)},
    'bn-257x768': {'bn2': (1, 192, 1, 17, 0, 15, 2), 'bn3': (1, 192, 1, 17, 2, 15, 2), 'bn_apply': (99, 3, 0)},
    'bn-272x768': {'bn2': (1, 192, 1, 17, 0, 16, 0), 'bn3': (1, 192, 1, 17, 2, 16, 0), 'bn_apply': (102, 3, 0)},
    'bn-273x768': {'bn2': (1, 192, 1, 18, 0, 15, 3), 'bn3': (1, 192, 1, 18, 2, 15, 3), 'bn_apply': (105, 3, 0)},
    'bn-4080x768': {'bn2': (1, 192, 1, 255, 0, 16, 0), 'bn3': (1, 192, 1, 255, 16, 16, 0), 'bn_apply': (1530, 3, 0)},
    'bn-4081x768': {'bn2': (1, 192, 1, 256, 0, 15, 241), 'bn3': (1, 192, 1, 256, 16, 15, 241), 'bn_apply': (1533, 3, 0)},
    'bn-4096x768': {'bn2': (1, 192, 1, 256, 0, 16, 0), 'bn3': (1, 192, 1, 256, 16, 16, 0), 'bn_apply': (1536, 3, 0)},
    'bn-4097x768': {'bn2': (1, 192, 1, 257, 0, 15, 242), 'bn3': (1, 192, 1, 256, 16, 16, 1), 'bn_apply': (1539, 3, 0)},
    'bn-8209x768': {'bn2': (1, 192, 1, 512, 0, 16, 17), 'bn3': (1, 192, 1, 256, 16, 32, 17), 'bn_apply': (3081, 3, 0)},
    'bn-8193x768': {'bn2': (1, 192, 1, 512, 0, 16, 1), 'bn3': (1, 192, 1, 256, 16, 32, 1), 'bn_apply': (3075, 3, 0)},
    'bn-10923x768': {'bn2': (1, 192, 1, 512, 0, 21, 171), 'bn3': (1, 192, 1, 256, 16, 42, 171), 'bn_apply': (4098, 3, 1)},
    'bn-4x768': {'bn2': (1, 192, 1, 1, 0, 4, 0), 'bn3': (1, 192, 1, 1, 1, 4, 0), 'bn_apply': (3, 3, 0)},
    'bn-5x768': {'bn2': (1, 192, 1, 1, 0, 5, 0), 'bn3': (1, 192, 1, 1, 1, 5, 0), 'bn_apply': (3, 3, 0)},
    'bn-6x768': {'bn2': (1, 192, 1, 1, 0, 6, 0), 'bn3': (1, 192, 1, 1, 1, 6, 0), 'bn_apply': (3, 3, 0)},
    'bn-1x64': {'bn2': (16, 16, 1, 1, 0, 0, 1), 'bn3': (16, 16, 1, 1, 1, 0, 1), 'bn_apply': (1, 1, 0)},
    'bn-255x64': {'bn2': (16, 16, 1, 1, 0, 15, 15), 'bn3': (16, 16, 1, 1, 1, 15, 15), 'bn_apply': (8, 1, 0)},
    'bn-256x64': {'bn2': (16, 16, 1, 1, 0, 16, 0), 'bn3': (16, 16, 1, 1, 1, 16, 0), 'bn_apply': (8, 1, 0)},
    'bn-257x64': {'bn2': (16, 16, 1, 2, 0, 8, 1), 'bn3': (16, 16, 1, 2, 1, 8, 1), 'bn_apply': (9, 1, 0)},
    'bn-4097x64': {'bn2': (16, 16, 1, 17, 0, 15, 17), 'bn3': (16, 16, 1, 17, 2, 15, 17), 'bn_apply': (129, 1, 0)},
    'bn-65x256': {'bn2': (4, 64, 1, 2, 0, 8, 1), 'bn3': (4, 64, 1, 2, 1, 8, 1), 'bn_apply': (9, 1, 0)},
    'bn-1025x256': {'bn2': (4, 64, 1, 17, 0, 15, 5), 'bn3': (4, 64, 1, 17, 2, 15, 5), 'bn_apply': (129, 1, 0)},
    'bn-35x28': {'bn2': (36, 7, 1, 1, 0, 0, 35), 'bn3': (36, 7, 1, 1, 1, 0, 35), 'bn_apply': (7, 7, 0)},
    'bn-36x28': {'bn2': (36, 7, 1, 1, 0, 1, 0), 'bn3': (36, 7, 1, 1, 1, 1, 0), 'bn_apply': (7, 7, 0)},
    'bn-37x28': {'bn2': (36, 7, 1, 1, 0, 1, 1), 'bn3': (36, 7, 1, 1, 1, 1, 1), 'bn_apply': (7, 7, 0)},
    'bn-17x1028': {'bn2': (1, 256, 2, 2, 0, 8, 1), 'bn3': (1, 256, 2, 2, 1, 8, 1), 'bn_apply': (257, 257, 0)},
    'bn-300x1028': {'bn2': (1, 256, 2, 19, 0, 15, 15), 'bn3': (1, 256, 2, 19, 2, 15, 15), 'bn_apply': (257, 257, 0)},
    'bn-300x60': {'bn2': (17, 15, 1, 2, 0, 8, 28), 'bn3': (17, 15, 1, 2, 1, 8, 28), 'bn_apply': (15, 15, 0)},
    'bn-300x132': {'bn2': (7, 33, 1, 3, 0, 14, 6), 'bn3': (7, 33, 1, 3, 1, 14, 6), 'bn_apply': (33, 33, 0)},
    'bn-257x768-act0': {'bn2': (1, 192, 1, 17, 0, 15, 2), 'bn3': (1, 192, 1, 17, 2, 15, 2), 'bn_apply': (99, 3, 0)},
    'bn-257x768-act2': {'bn2': (1, 192, 1, 17, 0, 15, 2), 'bn3': (1, 192, 1, 17, 2, 15, 2), 'bn_apply': (99, 3, 0)},
    'bn-37x28-act0': {'bn2': (36, 7, 1, 1, 0, 1, 1), 'bn3': (36, 7, 1, 1, 1, 1, 1), 'bn_apply': (7, 7, 0)},
    'bn-37x28-act2': {'bn2': (36, 7, 1, 1, 0, 1, 1), 'bn3': (36, 7, 1, 1, 1, 1, 1), 'bn_apply': (7, 7, 0)},
    'bn-4097x64-act0': {'bn2': (16, 16, 1, 17, 0, 15, 17), 'bn3': (16, 16, 1, 17, 2, 15, 17), 'bn_apply': (129, 1, 0)},
    'bn-4097x64-act2': {'bn2': (16, 16, 1, 17, 0, 15, 17), 'bn3': (16, 16, 1, 17, 2, 15, 17), 'bn_apply': (129, 1, 0)},
    'bn-0x64-two-launch': {'bn2': (16, 16, 1, 1, 0, 0, 0)},
    'bn-0x768-two-launch': {'bn2': (1, 192, 1, 1, 0, 0, 0)},
    'ada-b1x64': {'ada': (1, 1, 1, 0, 16, 1)},
    'ada-b1x260': {'ada': (1, 1, 65, 0, 64, 2)},
    'ada-b2x64': {'ada': (1, 1, 1, 0, 16, 1)},
    'ada-b2x260': {'ada': (1, 3, 65, 0, 64, 2)},
    'ada-b3x64': {'ada': (1, 1, 1, 0, 16, 1)},
    'ada-b3x260': {'ada': (1, 3, 65, 0, 64, 2)},
    'ada-b4x64': {'ada': (1, 2, 2, 0, 16, 1)},
    'ada-b4x260': {'ada': (1, 6, 65, 0, 64, 2)},
    'ada-b5x64': {'ada': (1, 2, 2, 0, 16, 1)},
    'ada-b5x260': {'ada': (1, 7, 65, 0, 64, 2)},
    'ada-tiny100x64': {'ada': (1, 10, 10, 0, 16, 1)},
    'ada-tiny100x260': {'ada': (1, 39, 65, 0, 64, 2)},
    'ada-chunks2x260': {'ada': (2, 115, 130, 0, 64, 2)},
    'ada-empty1x64': {'ada': (1, 10, 10, 0, 16, 1)},
    'ada-empty1x260': {'ada': (1, 39, 65, 0, 64, 2)},
    'ada-empty2x64': {'ada': (2, 49, 49, 0, 16, 1)},
    'ada-empty2x260': {'ada': (2, 196, 260, 0, 64, 2)},
    'ada-chunks2x4': {'ada': (2, 2, 2, 0, 16, 1)},
    'ada-chunks2x64': {'ada': (2, 29, 29, 0, 16, 1)},
    'ada-chunks2x68': {'ada': (2, 30, 34, 0, 32, 1)},
    'ada-chunks2x128': {'ada': (2, 57, 57, 0, 32, 1)},
    'ada-chunks2x768': {'ada': (2, 338, 339, 0, 64, 3)},
    'ada-chunks2x1024': {'ada': (2, 451, 451, 0, 64, 4)},
    'ada-chunks2x1028': {'ada': (2, 453, 514, 0, 0, 0)},
    'ada-chunks63x64': {'ada': (63, 504, 504, 0, 16, 1)},
    'ada-chunks64capx64': {'ada': (64, 513, 513, 0, 16, 1)},
    'ada-applycapx768': {'ada': (43, 4096, 4098, 1, 64, 3)},
    'b16-ln-300x64': {'ln_fwd': (16, 1, 16, 19), 'ln_bwd': (4, 4, 64, 3, 2)},
    'b16-ln-300x68': {'ln_fwd': (32, 1, 8, 38), 'ln_bwd': (8, 3, 32, 5, 2)},
    'b16-ln-300x132': {'ln_fwd': (64, 1, 4, 75), 'ln_bwd': (16, 3, 16, 10, 2)},
    'b16-ln-300x516': {'ln_fwd': (64, 3, 4, 75), 'ln_bwd': (64, 3, 4, 38, 2)},
    'b16-ln-300x768': {'ln_fwd': (64, 3, 4, 75), 'ln_bwd': (64, 3, 4, 38, 2)},
    'b16-ln-8193x768-capped': {'ln_fwd': (64, 3, 4, 2049), 'ln_bwd': (64, 3, 4, 1024, 3)},
    'b16-bn-1x768': {'bn2': (1, 192, 1, 1, 0, 1, 0), 'bn3': (1, 192, 1, 1, 1, 1, 0), 'bn_apply': (3, 3, 0)},
    'b16-bn-17x768': {'bn2': (1, 192, 1, 2, 0, 8, 1), 'bn3': (1, 192, 1, 2, 1, 8, 1), 'bn_apply': (9, 3, 0)},
    'b16-bn-257x768': {'bn2': (1, 192, 1, 17, 0, 15, 2), 'bn3': (1, 192, 1, 17, 2, 15, 2), 'bn_apply': (99, 3, 0)},
    'b16-bn-4097x768': {'bn2': (1, 192, 1, 257, 0, 15, 242), 'bn3': (1, 192, 1, 256, 16, 16, 1), 'bn_apply': (1539, 3, 0)},
    'b16-bn-35x28': {'bn2': (36, 7, 1, 1, 0, 0, 35), 'bn3': (36, 7, 1, 1, 1, 0, 35), 'bn_apply': (7, 7, 0)},
    'b16-bn-36x28': {'bn2': (36, 7, 1, 1, 0, 1, 0), 'bn3': (36, 7, 1, 1, 1, 1, 0), 'bn_apply': (7, 7, 0)},
    'b16-bn-37x28': {'bn2': (36, 7, 1, 1, 0, 1, 1), 'bn3': (36, 7, 1, 1, 1, 1, 1), 'bn_apply': (7, 7, 0)},
    'b16-bn-4097x64': {'bn2': (16, 16, 1, 17, 0, 15, 17), 'bn3': (16, 16, 1, 17, 2, 15, 17), 'bn_apply': (129, 1, 0)},
    'b16-bn-300x1028': {'bn2': (1, 256, 2, 19, 0, 15, 15), 'bn3': (1, 256, 2, 19, 2, 15, 15), 'bn_apply': (257, 257, 0)},
}
# END PLAN
