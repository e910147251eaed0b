"""The launch plans of tests/norm_edges.py on a machine without a device: lotus_norm_plan / lotus_adanorm_plan are pure host
functions of the shape, built from the helpers the launches use, so the branch every row of the table is there to enter is
pinned before any GPU test runs.  Also here: the argument checks of the norm entry points (refused widths, C <= 0, no rows on
the fused statistics), which must answer LOTUS_E_ARG before any arithmetic on C and before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import norm_edges as ne
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib()


def _plan(L, entry, args, fields):
    out = (ctypes.c_int * 8)(*([-7] * 8))
    rc = L.fn[entry](*args, ctypes.addressof(out))
    assert rc == 0, (entry, args, rc, L.last_error())
    assert list(out[fields:]) == [-7] * (8 - fields), (entry, args, "writes past its documented fields")
    return tuple(out[:fields])


@pytest.mark.parametrize("group", ["LN", "BN", "ADA", "TWIN"])
def test_every_row_of_the_table_has_its_plan(lib, group):
    rows = getattr(ne, group)
    assert rows
    wrong = []
    for row in rows:
        queries = ne.plan_queries(row)
        assert queries and set(ne.PLAN[row.id]) == {k for k, _, _ in queries}, row.id
        for key, entry, args in queries:
            want = ne.PLAN[row.id][key]
            assert len(want) == ne.PLAN_FIELDS[key], (row.id, key)
            for e in (entry, entry.replace("lotus_", "lotus_b16_")) if entry == "lotus_norm_plan" else (entry,):
                got = _plan(lib, e, args, ne.PLAN_FIELDS[key])
                if got != tuple(want):
                    wrong.append((row.id, e, key, tuple(want), got))
        if row.family == "ln":
            assert lib.fn["lotus_layernorm_bwd_parts"](row.shape, row.C) == ne.PLAN[row.id]["ln_bwd"][3], row.id
            assert lib.fn["lotus_b16_layernorm_bwd_parts"](row.shape, row.C) == ne.PLAN[row.id]["ln_bwd"][3], row.id
        if row.family == "ada":
            G, B = ne.PLAN[row.id]["ada"][0], len(row.shape)
            assert lib.fn["lotus_adanorm_workspace"](ne.rows_of(row), B, row.C) == G * B * 2 * row.C * 4, row.id
    assert not wrong, "\n".join(f"{i} {e} {k}: the table says {w}, the library plans {g}" for i, e, k, w, g in wrong[:30])
    assert set(ne.PLAN) == {r.id for r in ne.ROWS if ne.plan_queries(r)}


def test_the_table_holds_what_it_says():
    """The edges the table promises, read from its literal numbers (not from the library)."""
    P = ne.PLAN
    # LayerNorm: 16 / 32 / 64 lanes forward with 1 - 4 quads, 4 - 64 lanes backward; a last quad column owned by one lane
    fwd = {C: P[f"ln-300x{C}"]["ln_fwd"][:2] for C in ne.LN_WIDTHS}
    bwd = {C: P[f"ln-300x{C}"]["ln_bwd"][:2] for C in ne.LN_WIDTHS}
    assert {l for l, _ in fwd.values()} == {16, 32, 64} and {q for _, q in fwd.values()} == {1, 2, 3, 4}
    assert {l for l, _ in bwd.values()} == {4, 8, 16, 32, 64}
    assert fwd[64] == (16, 1) and fwd[68] == (32, 1) and fwd[128] == (32, 1) and fwd[132] == (64, 1) and fwd[1024] == (64, 4)
    for C in (68, 132, 260, 516):      # (C / 4) % lanes == 1 behind whole columns: the last quad column belongs to lane 0 alone
        assert (C // 4) % bwd[C][0] == 1 and bwd[C][1] > 1, C
        assert C < 260 or ((C // 4) % fwd[C][0] == 1 and fwd[C][1] > 1), C
    for C, ms in ne.LN_ROWS.items():
        rf, rb = P[f"ln-1x{C}"]["ln_fwd"][2], P[f"ln-1x{C}"]["ln_bwd"][2]
        assert {0, 1, rf - 1, rf, rf + 1, rb - 1, rb, rb + 1, 2 * rb + 1} == set(ms), C
        assert P[f"ln-{2 * rb + 1}x{C}"]["ln_bwd"][3] == 2 and P[f"ln-{rb + 1}x{C}"]["ln_bwd"][3] == 1
        assert P[f"ln-0x{C}"]["ln_fwd"][3] == 0 and P[f"ln-0x{C}"]["ln_bwd"][3:] == (1, 0)
    assert P["ln-8193x768-capped"]["ln_bwd"] == (64, 3, 4, 1024, 3) and 8193 - 2 * 1024 * 4 == 1      # last pass: one row
    assert P["ln-8209x768-capped"]["ln_bwd"][3:] == (1024, 3)
    assert P["ln-131073x64-capped"]["ln_bwd"] == (4, 4, 64, 1024, 3) and P["ln-131073x64-capped"]["ln_bwd"][2] * 2 * 1024 == 131072
    assert [P[f"ln-parts{n}"]["ln_bwd"][3] for n in ne.LN_PARTS] == ne.LN_PARTS == [1, 31, 32, 33, 127, 128, 129, 1024]
    # BatchNorm, fused statistics at C = 768
    grids = [P[f"bn-{M}x768"]["bn3"][3] for M in ne.BN_768[:14]]
    assert grids == [1, 1, 1, 2, 16, 16, 17, 17, 18, 255, 256, 256, 256, 256]
    assert {P[f"bn-{M}x768"]["bn3"][4] for M in ne.BN_768} == {1, 2, 16}
    assert P["bn-257x768"]["bn3"][4] == 2 and 17 % 16 == 1                                          # a group of one block
    per_slot = {P[f"bn-{M}x768"]["bn3"][5] for M in ne.BN_768[:14]}
    assert min(per_slot) == 1 and max(per_slot) == 32
    walked = {n + k for M in ne.BN_768 for n, extra in [P[f"bn-{M}x768"]["bn3"][5:7]] for k in ((0, 1) if extra else (0,))}
    assert {n % 8 for n in walked} == set(range(8)) and {n % 2 for n in walked} == {0, 1}       # leftovers of both unrolled walks
    assert P["bn-8193x768"]["bn2"][3] == 512 and P["bn-4097x768"]["bn2"][3] == 257
    assert P["bn-4097x64"]["bn3"][3:5] == (17, 2)
    assert [P[f"bn-{M}x28"]["bn3"][:2] for M in (35, 36, 37)] == [(36, 7)] * 3 and 256 - 36 * 7 == 4  # 4 idle threads
    assert [P[f"bn-{M}x28"]["bn3"][5:7] for M in (35, 36, 37)] == [(0, 35), (1, 0), (1, 1)]
    assert P["bn-300x60"]["bn3"][:2] == (17, 15) and P["bn-300x132"]["bn3"][:2] == (7, 33)
    assert P["bn-300x1028"]["bn3"][:3] == (1, 256, 2) and P["bn-300x1028"]["bn_apply"][1] == 257
    assert P["bn-257x768"]["bn_apply"][1] == 3 and P["bn-37x28"]["bn_apply"][1] == 7
    assert P["bn-10923x768"]["bn_apply"] == (4098, 3, 1) and P["bn-8209x768"]["bn_apply"][2] == 0
    # AdaNorm
    assert [P[f"ada-b{b}x64"]["ada"][0] for b in range(1, 6)] == [1] * 5
    assert P["ada-chunks2x64"]["ada"][0] == 2 and P["ada-chunks63x64"]["ada"][0] == 63 and P["ada-chunks64capx64"]["ada"][0] == 64
    assert 16385 > 64 * 256                                                                         # ... and capped there
    assert P["ada-empty1x64"]["ada"][0] == 1 and P["ada-empty2x64"]["ada"][0] == 2
    assert P["ada-applycapx768"]["ada"][1:4] == (4096, 4098, 1)
    assert P["ada-chunks2x1028"]["ada"][4:] == (0, 0) and P["ada-chunks2x1024"]["ada"][4:] == (64, 4)
    assert {r.C for r in ne.ADA if r.shape == ne.ADA_LAYOUTS["chunks2"]} == set(ne.ADA_WIDTHS)
    assert len(ne.TWIN) == 15


# ------------------------------------------------------------------------------------------------- argument checks
_NORM = ("layernorm", "batchnorm", "adaln", "adabn", "adanorm", "norm_plan")
_INTS = {"M": 5, "B": 2, "mod_ld": 8192, "dmod_ld": 8192, "nparts": 1, "act": 1, "train": 1, "training": 1, "accumulate": 0, "kind": 0}
_LN_ONLY = ("layernorm_fwd", "layernorm_bwd", "layernorm_bwd_params", "adaln_fwd", "adaln_bwd")   # refuse 1028 and 66 as well


def _entries(L):
    """Every norm entry point and query that takes a width C (lotus_linear_dgrad_ln belongs to the dense table)."""
    return sorted(n for n, (_, _, names) in L.protos.items() if any(k in n for k in _NORM) and "C" in names and "linear" not in n)


def _call(L, name, C, **over):
    restype, argtypes, names = L.protos[name]
    host = np.zeros(1 << 16, dtype=np.float64)           # 512 KiB: what a call with M = 5 rows could touch before it is refused
    args = []
    for ty, nm in zip(argtypes, names):
        if nm in over:
            args.append(over[nm])
        elif nm == "C":
            args.append(C)
        elif ty is ctypes.c_void_p:
            args.append(None if nm == "stream" else host.ctypes.data)
        elif ty is ctypes.c_size_t:
            args.append(1 << 30)
        elif ty is ctypes.c_float:
            args.append(1e-3)
        else:
            args.append(_INTS.get(nm, 0))
    return L.fn[name](*args), host


needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="calls entry points with host pointers: only safe without a device")


@needs_no_device
def test_every_norm_entry_point_refuses_a_width_of_zero_or_less(lib):
    names = _entries(lib)
    assert len(names) >= 2 * 18 + 9 and "lotus_batchnorm_stats" in names and "lotus_b16_batchnorm_apply_sums" in names, names
    for name in names:
        for C in (0, -4):
            for kind in (range(5) if "norm_plan" in name else [0]):
                rc, _ = _call(lib, name, C, kind=kind)
                if lib.protos[name][0] is ctypes.c_size_t or name.endswith("layernorm_bwd_parts"):
                    assert rc == 0, (name, C, rc)            # a size or a count: nothing to allocate, nothing to reduce
                else:
                    assert rc == E_ARG, (name, C, rc, lib.last_error())


@needs_no_device
def test_layernorm_entry_points_refuse_unsupported_widths(lib):
    assert ne.LN_REFUSED == [1028, 66, 0]
    for name in _entries(lib):
        if not name.endswith(_LN_ONLY):
            continue
        for C in ne.LN_REFUSED:
            rc, _ = _call(lib, name, C)
            assert rc == E_ARG, (name, C, rc)
    out = (ctypes.c_int * 8)()
    for C in ne.LN_REFUSED:
        for entry in ("lotus_norm_plan", "lotus_b16_norm_plan"):
            assert lib.fn[entry](0, 5, C, ctypes.addressof(out)) == E_ARG and lib.fn[entry](1, 5, C, ctypes.addressof(out)) == E_ARG
        assert lib.fn["lotus_layernorm_bwd_parts"](5, C) == 0
    assert lib.fn["lotus_norm_plan"](3, 5, 66, ctypes.addressof(out)) == E_ARG          # no whole quads
    assert lib.fn["lotus_norm_plan"](3, 5, 1028, ctypes.addressof(out)) == 0            # the BatchNorm takes it
    assert lib.fn["lotus_norm_plan"](5, 5, 64, ctypes.addressof(out)) == E_ARG and lib.fn["lotus_norm_plan"](0, 5, 64, None) == E_ARG
    assert lib.fn["lotus_adanorm_plan"](5, 2, 1028, ctypes.addressof(out)) == 0 and tuple(out[4:6]) == (0, 0)
    assert lib.fn["lotus_adanorm_plan"](5, 2, 66, ctypes.addressof(out)) == E_ARG and lib.fn["lotus_adanorm_plan"](5, 0, 64, ctypes.addressof(out)) == E_ARG


@needs_no_device
def test_fused_statistics_refuse_a_batch_of_no_rows(lib):
    for base in ("batchnorm_stats_fused", "batchnorm_bwd_stats_fused", "batchnorm_bwd_stats_fused_params"):
        for name in ("lotus_" + base, "lotus_b16_" + base):
            rc, _ = _call(lib, name, 64, M=0)
            assert rc == E_ARG, (name, rc)
    # the two-launch statistics take M = 0: the call gets as far as the launch (which has no device here)
    rc, _ = _call(lib, "lotus_batchnorm_stats", 64, M=0)
    assert rc == -2, rc
