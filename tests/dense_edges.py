"""Edge shapes of the dense layers and the kernel each of them must run on (test infrastructure, not collected).

One row per call of a C-ABI dense entry point: `Case(id, call, M, N, K, opts, route)`.  M, N, K are the entry point's own
arguments (fwd: y[M, N] = x[M, K] w[N, K]^T; dgrad / dgrad_ln: dx[M, K] = dy[M, N] w[N, K]; wgrad: dw[N, K] = dy[M, N]^T
x[M, K]).  `route` is what lotus_dense_last_route must report afterwards: Route(family, bm, bn, bk, nz, fast, fused).

The routes are written down from the dispatcher's documented rules, not computed with its code:
  * gemm_kernel (family 1) has 64 x 64 tiles; exact fp32 products on these small grids stage 64-deep slabs, weight
    gradients and the bf16 / bf16x3 operand modes 32-deep ones;
  * FAST needs 16-byte aligned operands and widths that are multiples of 4 — an output width of 90, 217 or 5, a reduction
    of 6 or 774, or an operand 4 bytes off a 16-byte boundary give the guarded form;
  * a forward / input-gradient product splits its reduction (workspace given) in powers of two while a range stays >= 384
    deep; with arrival counters and FAST the split is fused, else it is two launches;
  * a weight gradient over M rows splits in powers of two while a range stays >= 128 rows; up to 4 ranges are fused when
    counters are given;
  * gemm_dma_kernel (family 2) takes exact products of >= 16 384 rows whose 128-row tiles give >= 400 blocks (>= 128 with the
    LayerNorm epilogue): 128 x 128 x 16 above 64 output columns, 128 x 64 x 32 up to 64; weight gradients on ~256 blocks.

tests/test_dense_routes_host.py asserts every row on a machine without a device (the host path runs to the launch);
tests/test_gpu_dense_edges.py and tests/test_gpu_gemm_dma.py run the rows on the GPU."""
import collections

Route = collections.namedtuple("Route", "family bm bn bk nz fast fused")
Case = collections.namedtuple("Case", "id call M N K opts route")

GUARD = 64
ACT_NONE, ACT_GELU, ACT_LEAKY = 0, 1, 2
ENTRY = {"fwd": "lotus_linear_fwd", "dgrad": "lotus_linear_dgrad", "dgrad_ln": "lotus_linear_dgrad_ln", "wgrad": "lotus_linear_wgrad"}

ROWS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257]
PAIRS = [(64, 64), (192, 64), (68, 128), (128, 36), (90, 128), (217, 128), (5, 64), (64, 6)]   # (output width, reduction)
GUARDED_PAIRS = {(90, 128), (217, 128), (5, 64), (64, 6)}
# every epilogue of the model: forward bias / saved pre-activation / GELU | LeakyReLU / residual / dropout 0.25; input
# gradient act'(pre) / add / dropout
FWD_EPI = {"gelu_pre": dict(bias=1, pre=1, act=ACT_GELU),
           "leaky_res_drop": dict(bias=1, act=ACT_LEAKY, residual=1, drop=0.25)}
DGRAD_EPI = {"gelu_add": dict(pre=1, act=ACT_GELU, add=1),
             "leaky_add_drop": dict(pre=1, act=ACT_LEAKY, add=1, drop=0.25)}
FULL_FWD = dict(bias=1, pre=1, act=ACT_GELU, residual=1, drop=0.25)
FULL_DGRAD = dict(pre=1, act=ACT_GELU, add=1, drop=0.25)


def _gk(bk, nz=1, fast=1, fused=0):
    return Route(1, 64, 64, bk, nz, fast, fused)


def _mnk(call, rows, out, red):
    return (rows, out, red) if call == "fwd" else (rows, red, out)


def _grid_cases():
    """Forward and input gradient on few rows: every epilogue on every (rows, width pair), one set with the activation
    operand 4 bytes off a 16-byte boundary."""
    out = []
    for call, epis in (("fwd", FWD_EPI), ("dgrad", DGRAD_EPI)):
        for (o, r) in PAIRS:
            fast = 0 if (o, r) in GUARDED_PAIRS else 1
            for rows in ROWS:
                for name, epi in epis.items():
                    out.append(Case(f"{call}-{rows}x{o}x{r}-{name}", call, *_mnk(call, rows, o, r), dict(epi), _gk(64, fast=fast)))
        for (o, r) in [(64, 64), (192, 64), (68, 128), (128, 36)]:
            for rows in ROWS:
                epi = dict(FULL_FWD if call == "fwd" else FULL_DGRAD, misalign=1)
                out.append(Case(f"{call}-{rows}x{o}x{r}-off4", call, *_mnk(call, rows, o, r), epi, _gk(64, fast=0)))
    return out


# (rows, output width, reduction) -> (ranges, FAST)
SPLITK = [((65, 64, 772), 2, 1),      # 448 + 324
          ((130, 192, 1540), 4, 1),   # 3 x 448 + 196
          ((7, 64, 6148), 16, 1),     # 13 x 448 + 324, the last two ranges empty
          ((65, 64, 774), 2, 0),      # reduction % 4 != 0: guarded kernel, two launches whatever is given
          ((65, 90, 772), 1, 0)]      # output width % 4 != 0: no split


def _splitk_cases():
    out = []
    for call, full in (("fwd", FULL_FWD), ("dgrad", FULL_DGRAD)):
        for (rows, o, r), nz, fast in SPLITK:
            for counters in (1, 0):
                opts = dict(full, ws=1, counters=counters)
                route = _gk(64, nz=nz, fast=fast, fused=1 if (counters and fast and nz > 1) else 0)
                out.append(Case(f"{call}-splitk-{rows}x{o}x{r}-{'cnt' if counters else 'nocnt'}", call, *_mnk(call, rows, o, r), opts, route))
    return out


# reduction rows -> ranges of gemm_kernel's weight gradient (257: 192 + 65; 520: 192 / 192 / 136 / 0; 1025: 5 x 192 + 65 + 0 + 0)
WGRAD_ROWS = {1: 1, 2: 1, 63: 1, 64: 1, 65: 1, 127: 1, 129: 1, 257: 2, 520: 4, 1025: 8}
WGRAD_NK = [(64, 64), (192, 64), (68, 36), (90, 128), (5, 64), (217, 128)]
WGRAD_GUARDED = {(90, 128), (5, 64), (217, 128)}
WGRAD_FUSE_MAX = 4
# bias, db in a buffer of its own, counters, accumulate
WGRAD_VARIANTS = {"plain": dict(bias=1, counters=1),
                  "nobias": dict(bias=0, counters=1),
                  "sepdb": dict(bias=1, sep_db=1, counters=0),
                  "nocnt": dict(bias=1, counters=0),
                  "acc": dict(bias=1, counters=1, accumulate=1),
                  "acc_nocnt_sepdb": dict(bias=1, sep_db=1, counters=0, accumulate=1)}


def _wgrad_route(nz, fast, opts, bk=32):
    fused = 1 if (opts.get("counters") and fast and 1 < nz <= WGRAD_FUSE_MAX) else 0
    return _gk(bk, nz=nz, fast=fast, fused=fused)


def _wgrad_cases():
    out = []
    for (n, k) in WGRAD_NK:
        fast = 0 if (n, k) in WGRAD_GUARDED else 1
        for rows, nz in WGRAD_ROWS.items():
            for name, opts in WGRAD_VARIANTS.items():
                out.append(Case(f"wgrad-{rows}x{n}x{k}-{name}", "wgrad", rows, n, k, dict(opts), _wgrad_route(nz, fast, opts)))
    for name, opts in WGRAD_VARIANTS.items():   # a level-3 shape: 8 ranges of 192, the last one empty
        out.append(Case(f"wgrad-1300x512x512-{name}", "wgrad", 1300, 512, 512, dict(opts), _wgrad_route(8, 1, opts)))
    return out


def _precision_cases():
    """bf16 (1) and bf16x3 (3) operands: 32-deep slabs."""
    out = []
    for prec in (1, 3):
        for (o, r) in [(64, 64), (192, 64)]:
            for rows in (1, 5, 65, 129):
                out.append(Case(f"fwd-{rows}x{o}x{r}-prec{prec}", "fwd", rows, o, r, dict(bias=1, prec=prec), _gk(32)))
                out.append(Case(f"dgrad-{rows}x{o}x{r}-prec{prec}", "dgrad", rows, r, o, dict(prec=prec), _gk(32)))
            for rows in (65, 257, 520):
                opts = dict(bias=1, counters=1, prec=prec)
                out.append(Case(f"wgrad-{rows}x{o}x{r}-prec{prec}", "wgrad", rows, o, r, opts, _wgrad_route(WGRAD_ROWS[rows], 1, opts)))
    return out


def _dma(bm, bn, bk, nz=1, fused=0):
    return Route(2, bm, bn, bk, nz, 1, fused)


def _dma_cases():
    """The smallest shapes the dispatcher gives to the LDS-DMA kernels."""
    out = []
    wide, narrow = _dma(128, 128, 16), _dma(128, 64, 32)
    for (m, n, k), route in [((16385, 512, 128), wide), ((16411, 448, 48), wide), ((16511, 512, 128), wide),
                             ((51205, 64, 64), narrow), ((51205, 48, 96), narrow)]:
        for name, epi in dict(FWD_EPI, full=FULL_FWD).items():
            out.append(Case(f"dma-fwd-{m}x{n}x{k}-{name}", "fwd", m, n, k, dict(epi), route))
    for (m, n, k), route in [((16411, 128, 512), wide), ((51205, 256, 64), narrow)]:
        for name, epi in dict(DGRAD_EPI, plain={}).items():
            out.append(Case(f"dma-dgrad-{m}x{n}x{k}-{name}", "dgrad", m, n, k, dict(epi), route))
    for rows in (16385, 16511):
        for c, route in ((64, narrow), (128, wide)):
            for dz in (1, 0):
                out.append(Case(f"dma-dgrad_ln-{rows}x{3 * c}x{c}-{'dz' if dz else 'nodz'}", "dgrad_ln", rows, 3 * c, c,
                                dict(add=1, dz=dz, ln_fused=1), route))
    # weight gradients: ~256 blocks, ranges of >= 256 rows.  16411 rows in 64 ranges of 320: 51 full, 91 rows, 12 empty
    for (m, n, k), route in [((16411, 256, 256), _dma(128, 128, 16, nz=64)), ((32805, 256, 64), _dma(128, 64, 32, nz=128)),
                             ((32805, 192, 64), _dma(128, 64, 32, nz=128)), ((32805, 64, 256), _dma(64, 128, 32, nz=128)),
                             ((65573, 64, 64), _dma(64, 64, 32, nz=256))]:
        for name in ("plain", "nobias", "acc"):
            out.append(Case(f"dma-wgrad-{m}x{n}x{k}-{name}", "wgrad", m, n, k, dict(WGRAD_VARIANTS[name]), route))
    return out


# The switches of the child interpreter that puts the LDS-DMA kernels on few rows (documented in include/lotus_hip.h; read
# once per process): any row count, any grid, weight gradients on ~4 blocks
FEW_ENV = {"LOTUS_GEMM_DMA_MINROWS": "1", "LOTUS_GEMM_DMA_MINBLOCKS": "1", "LOTUS_GEMM_DMA_WGRAD_BLOCKS": "4"}
FEW_ROWS = [1, 2, 31, 127, 128, 129, 257]
FEW_WGRAD_ROWS = {1024: 8, 1061: 8, 2085: 16}    # rows -> ranges under the default thresholds (gemm_kernel, two launches)


def _few_cases():
    """Few rows on both tiles of gemm_dma_kernel.  `route` holds under FEW_ENV; opts["default"] is the route of the same call
    without the switches.  The LayerNorm epilogue needs 128 row tiles whatever the switches say (gemm_route refuses: the
    call then is lotus_linear_dgrad — on the LDS-DMA tile of its width under FEW_ENV — and lotus_layernorm_bwd).  So the
    EPI = 2 kernel never runs on few rows; what the few-dgrad_ln_two_launch rows assert is that refusal: family 2 is the
    plain product, `dn` holds dy w and nparts is lotus_layernorm_bwd_parts(M, K), not ceil(M / 128) by construction."""
    out = []
    wide, narrow = _dma(128, 128, 16), _dma(128, 64, 32)
    for rows in FEW_ROWS:
        for tile, route, (o, r) in (("wide", wide, (192, 48)), ("narrow", narrow, (64, 96))):
            out.append(Case(f"few-fwd-{tile}-{rows}x{o}x{r}", "fwd", rows, o, r, dict(FULL_FWD, default=_gk(64)), route))
            out.append(Case(f"few-dgrad-{tile}-{rows}x{r}x{o}", "dgrad", rows, r, o, dict(FULL_DGRAD, default=_gk(64)), route))
        for c, route in ((64, narrow), (128, wide)):
            # (NOT the LayerNorm epilogue: the recorded product is the plain input gradient of the two-launch path)
            out.append(Case(f"few-dgrad_ln_two_launch-{rows}x{3 * c}x{c}", "dgrad_ln", rows, 3 * c, c,
                            dict(add=1, dz=1, default=_gk(64)), route))
    for rows, nz in FEW_WGRAD_ROWS.items():
        # one 64 x 64 tile: four ranges (1061 rows: 3 x 320 + 101); 192 x 128 is two 128 x 128 tiles: two ranges
        for (n, k), route in (((64, 64), _dma(64, 64, 32, nz=4, fused=1)), ((192, 128), _dma(128, 128, 16, nz=2, fused=1))):
            for name in ("plain", "acc"):
                opts = dict(WGRAD_VARIANTS[name], default=_gk(32, nz=nz))
                out.append(Case(f"few-wgrad-{rows}x{n}x{k}-{name}", "wgrad", rows, n, k, opts, route))
    return out


def _tail_cases():
    """A reduction that leaves gemm_kernel's register ring one PARTIAL slab more than the ring is deep, unsplit: 196 = 3 x 64 + 4
    on the two-slab ring of the exact product (the split ranges of 324 are the same tail behind five slabs)."""
    out = []
    for rows in (5, 65):
        out.append(Case(f"fwd-{rows}x64x196-tail", "fwd", rows, 64, 196, dict(FULL_FWD), _gk(64)))
        out.append(Case(f"dgrad-{rows}x196x64-tail", "dgrad", rows, 196, 64, dict(FULL_DGRAD), _gk(64)))
    return out


def _twin_cases():
    """The bf16-storage twin (lotus_b16_*: activations bf16 in memory, parameters and accumulation fp32) on rows 5, 64, 65.
    precision 1 is its vectorised path (bf16 MFMA, 32-deep slabs, a four-slab register ring on these row counts), precision 0
    its exact-product fallback (fp32 MFMA on 32-deep slabs, no ring).  opts["depth"] pins the ring depth, which is what tells
    the two apart.  228 = 7 x 32 + 4 leaves the four-slab ring one partial slab more than it is deep."""
    out = []
    for prec, depth in ((1, 4), (0, 1)):
        for rows in (5, 64, 65):
            for (o, r) in [(64, 64), (192, 64)] + ([(64, 228)] if prec == 1 else []):
                t = dict(b16=1, prec=prec, depth=depth)
                out.append(Case(f"b16-fwd-{rows}x{o}x{r}-prec{prec}", "fwd", rows, o, r, dict(FULL_FWD, **t), _gk(32)))
                out.append(Case(f"b16-dgrad-{rows}x{r}x{o}-prec{prec}", "dgrad", rows, r, o, dict(FULL_DGRAD, **t), _gk(32)))
            for (n, k) in [(64, 64), (192, 64)]:
                opts = dict(WGRAD_VARIANTS["plain"], b16=1, prec=prec, depth=depth)
                out.append(Case(f"b16-wgrad-{rows}x{n}x{k}-prec{prec}", "wgrad", rows, n, k, opts, _gk(32)))
    # What SELECTS the exact-product fallback when precision 1 is asked for (as ops always does in this mode) is a width that
    # is no multiple of 4 — the 90-wide head layer — not the row count: the activation operand of a forward / input-gradient
    # product is k-contiguous, so rows 5 and 65 above stay on the vectorised path.
    for rows in (5, 65):
        t = dict(b16=1, prec=1, depth=1)
        out.append(Case(f"b16-fwd-{rows}x90x128-prec1-fallback", "fwd", rows, 90, 128, dict(FULL_FWD, **t), _gk(32, fast=0)))
        out.append(Case(f"b16-dgrad-{rows}x128x90-prec1-fallback", "dgrad", rows, 128, 90, dict(FULL_DGRAD, **t), _gk(32, fast=0)))
    # (the weight gradient reduces over the rows: 228 of them are the same partial eighth slab on its ring)
    out.append(Case("b16-wgrad-228x64x64-prec1", "wgrad", 228, 64, 64, dict(WGRAD_VARIANTS["plain"], b16=1, prec=1, depth=4), _gk(32)))
    return out


# gemm_kernel's thresholds, in 64 x 64 output tiles: slabs 64 deep up to 512 tiles, 32 up to 2048, 16 above; the two-slab
# register ring up to 8192 tiles.  (rows, output width) on the threshold | the first grid past it -> slab depth, ring depth
BOUND_TILES = {512: (((32768, 64), 64, 2), ((32769, 64), 32, 2)),
               2048: (((8192, 1024), 32, 2), ((8192, 1088), 16, 2)),
               8192: (((8192, 4096), 16, 2), ((8192, 4160), 16, 1))}
B16_RING_MAX_ROWS = 8192    # the twin's four-slab ring: products over <= 8192 rows


def _bound_cases():
    """Host-only rows (not in TABLE: the GPU tests do not run them) on each side of every threshold of gemm_kernel's slab and
    ring depth.  A reduction of 8 and fewer than 400 128-row tiles keep the rows off the LDS-DMA kernels.  The twin's ring goes
    by the rows of the activation operand: M of a forward / input-gradient product, the reduction of a weight gradient (64
    ranges of 128 rows here)."""
    out = []
    for pair in BOUND_TILES.values():
        for (rows, o), bk, depth in pair:
            for call in ("fwd", "dgrad"):
                out.append(Case(f"bound-{call}-{rows}x{o}x8", call, *_mnk(call, rows, o, 8), dict(depth=depth), _gk(bk)))
    for rows, depth in ((B16_RING_MAX_ROWS, 4), (B16_RING_MAX_ROWS + 1, 1)):
        t = dict(b16=1, prec=1, depth=depth)
        for call in ("fwd", "dgrad"):
            out.append(Case(f"bound-b16-{call}-{rows}x64x64", call, rows, 64, 64, dict(t), _gk(32)))
        out.append(Case(f"bound-b16-wgrad-{rows}x64x64", "wgrad", rows, 64, 64, dict(t, bias=1), _gk(32, nz=64)))
    return out


def default_route(case):
    """The route of `case` in a process without FEW_ENV."""
    return case.opts.get("default", case.route)


GRID = _grid_cases()
SPLIT = _splitk_cases()
WGRAD = _wgrad_cases()
PRECISION = _precision_cases()
DMA = _dma_cases()
FEW = _few_cases()
TAIL = _tail_cases()
TWIN = _twin_cases()
BOUNDS = _bound_cases()
TABLE = GRID + SPLIT + WGRAD + PRECISION + DMA + FEW + TAIL + TWIN
BY_ID = {c.id: c for c in TABLE}
assert len(BY_ID) == len(TABLE)


def select(cases, **match):
    """Rows of `cases` whose call / M / N / K equal the given values."""
    return [c for c in cases if all(getattr(c, k) == v for k, v in match.items())]


# ---------------------------------------------------------------------------------------------------- the call itself
def buffers(case):
    """-> {name: (rows, cols, written)} of every float buffer the call is given (activations and parameters alike)."""
    M, N, K, o = case.M, case.N, case.K, case.opts
    if case.call == "fwd":
        b = dict(x=(M, K, 0), w=(N, K, 0), y=(M, N, 1))
        if o.get("bias"):
            b["bias"] = (1, N, 0)
        if o.get("residual"):
            b["residual"] = (M, N, 0)
        if o.get("pre"):
            b["pre"] = (M, N, 1)
    elif case.call == "dgrad":
        b = dict(dy=(M, N, 0), w=(N, K, 0), dx=(M, K, 1))
        if o.get("pre"):
            b["pre"] = (M, K, 0)
        if o.get("add"):
            b["add"] = (M, K, 0)
    elif case.call == "dgrad_ln":
        b = dict(dy=(M, N, 0), w=(N, K, 0), x=(M, K, 0), mean=(1, M, 0), rstd=(1, M, 0), gamma=(1, K, 0), dx=(M, K, 1), dn=(M, K, 1))
        if o.get("add"):
            b["add"] = (M, K, 0)
        if o.get("dz"):
            b["dz"] = (M, K, 1)
    else:
        b = dict(dy=(M, N, 0), x=(M, K, 0))
        if o.get("bias") and not o.get("sep_db"):
            b["dwdb"] = (N * K + N, 1, 1)      # dw, and db contiguous behind it
        else:
            b["dw"] = (N * K, 1, 1)
            if o.get("bias"):
                b["db"] = (N, 1, 1)
    return b


def entry(case, name=None):
    """The entry point (or the size query `name`) of this row: the bf16-storage twin where the row asks for it."""
    name = name or ENTRY[case.call]
    return "lotus_b16_" + name[len("lotus_"):] if case.opts.get("b16") else name


B16_ACTIVATIONS = {"fwd": ("x", "residual", "y", "pre"), "dgrad": ("dy", "dx", "pre", "add"), "wgrad": ("dy", "x")}


def is_bf16(case, name):
    """Whether buffer `name` of this row is a bf16 activation tensor (twin rows; parameters and gradients of parameters stay fp32)."""
    return bool(case.opts.get("b16")) and name in B16_ACTIVATIONS[case.call]


def misaligned(case):
    """The operand that starts 4 bytes off a 16-byte boundary (or None)."""
    return None if not case.opts.get("misalign") else ("x" if case.call == "fwd" else "dy")


def workspace_query(case):
    """-> (size query, its arguments) of the split-K workspace this call is given, or None."""
    if case.call == "wgrad":
        return "lotus_linear_wgrad_workspace", (case.M, case.N, case.K)
    if case.opts.get("ws"):
        return "lotus_linear_workspace", (case.M, case.N, case.K)
    return None


def arguments(case, ptr, ws=None, ws_bytes=0, counters=None, ln_ws=None, ln_ws_bytes=0, nparts=None):
    """The argument list of the entry point (without the stream).  ptr: {buffer name: pointer-like}; absent -> NULL."""
    M, N, K, o = case.M, case.N, case.K, case.opts
    g = ptr.get
    drop, seed, prec = float(o.get("drop", 0.0)), 1000 + M + N + K, o.get("prec", 0)
    cnt = counters if o.get("counters") else None
    if case.call == "fwd":
        return (g("x"), g("w"), g("bias"), g("residual"), g("y"), g("pre"), M, N, K, o.get("act", 0), drop, seed, prec, ws, ws_bytes, cnt)
    if case.call == "dgrad":
        return (g("dy"), g("w"), g("dx"), g("pre"), g("add"), M, N, K, o.get("act", 0), drop, seed, prec, ws, ws_bytes, cnt)
    if case.call == "dgrad_ln":
        return (g("dy"), g("w"), g("x"), g("mean"), g("rstd"), g("gamma"), g("add"), g("dx"), g("dn"), g("dz"),
                0.1 if o.get("dz") else 0.0, seed, M, N, K, prec, ws, ws_bytes, cnt, ln_ws, ln_ws_bytes, nparts)
    dw, db = (g("dwdb"), g("dwdb_db")) if "dwdb" in ptr else (g("dw"), g("db"))
    return (g("dy"), g("x"), dw, db, M, N, K, o.get("accumulate", 0), prec, ws, ws_bytes, cnt)


def drop_seed(case):
    return 1000 + case.M + case.N + case.K
