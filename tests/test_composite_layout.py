"""The buffer layouts of the composite entry points (csrc/blocks.cpp), pinned against a fixture.

Each sub-block kind defines its `saved` / `grads` / `tmp` layout once in blocks.cpp; the size queries, the forward and backward
entry points, the pair and lotus_composite_grads_layout all read that definition, and ops.py learns the gradient offsets from
the query.  tests/golden/composite_layout.json was written by tests/golden/make_golden_composite_layout.py at the commit BEFORE
that, when every one of these places spelled the layout out by hand: the totals the library reported, and the slices the
autograd nodes of ops.py took out of the `grads` slab.  CPU only: size and layout queries, nothing is launched."""
import json
import os
import threading

import numpy as np
import pytest

import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_layout.json")
with open(FIXTURE) as _f:
    GOLDEN = json.load(_f)
BUILDS = {"fp32": "lotus_", "b16": "lotus_b16_"}
GRADS_TOTAL = {"ffn": ("lotus_ffn_grads_floats", "C Hd"), "selfattn": ("lotus_selfattn_grads_floats", "C H"),
               "crossattn": ("lotus_crossattn_grads_floats", "C H Cc"), "crossattn_kv": ("lotus_crossattn_kv_grads_floats", "C H"),
               "cpe": ("lotus_cpe_grads_floats", "C"), "pair": ("lotus_pair_grads_floats", "C H Hd")}
PAIR_PARTS = ("cpe", "selfattn", "ffn", "crossattn_kv", "ffn")


@pytest.fixture(scope="module")
def fn():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib().fn


def layout(fn, prefix, kind, w, cap=64):
    off, length = np.full(cap, -1, dtype=np.int64), np.full(cap, -1, dtype=np.int64)
    n = fn[prefix + "composite_grads_layout"](GOLDEN["kinds"].index(kind), w["C"], w["H"], w["Hd"], w["Cc"], off.ctypes.data,
                                              length.ctypes.data, cap)
    assert 0 < n <= cap, (kind, n)
    return [[int(a), int(b)] for a, b in zip(off[:n], length[:n])]


def test_fixture_covers_the_grid_the_layouts_can_go_wrong_on():
    g = GOLDEN["grid"]
    assert {(p["C"], p["H"]) for p in g} >= {(64, 2), (128, 4), (256, 8), (512, 16), (768, 32), (24, 4)}
    assert {p["M"] for p in g} >= {1, 361, 1450, 6077, 65537} and {p["L"] for p in g} == {1, 128}
    assert {p["G"] for p in g} == {1, 3} and {p["n_extra"] for p in g} == {0, 1}
    assert any((p["C"] // p["H"]) % 4 for p in g)   # a head dimension that the 4-float rounding pads
    want = {f"lotus_{k}_{q}" for k in ("ffn", "selfattn", "crossattn", "crossattn_kv", "cpe", "pair")
            for q in ("saved_floats", "grads_floats", "tmp_floats", "ws_main_bytes", "ws_side_bytes")}
    assert set(GOLDEN["queries"]) == want | {"lotus_cpe_ws_conv_bytes", "lotus_pair_ws_conv_bytes", "lotus_pair_acts_floats"}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_size_queries_return_the_fixture_totals(fn, build):
    for name, args in GOLDEN["queries"].items():
        f = fn[BUILDS[build] + name[len("lotus_"):]]
        got = [f(*[p[a] for a in args]) for p in GOLDEN["grid"]]
        bad = [(p, g, w) for p, g, w in zip(GOLDEN["grid"], got, GOLDEN["values"][build][name]) if g != w]
        assert not bad, (name, len(bad), bad[0])


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_grads_layout_is_what_the_autograd_nodes_sliced(fn, build):
    checked = 0
    for w in GOLDEN["grads_slices"]:
        for kind in GOLDEN["kinds"]:
            got, want = layout(fn, BUILDS[build], kind, w), w["fields"][kind]
            if want is None:   # the pair's Python split asserted that nothing is padded: no reference where the rounding pads
                assert kind == "pair" and (w["C"] // w["H"]) % 4
                continue
            assert got == [list(f) for f in want], (kind, w["C"], w["H"])
            checked += 1
    assert checked >= 6 * len(GOLDEN["grads_slices"]) - 1


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_grads_fields_are_disjoint_aligned_and_inside_the_slab(fn, build):
    for w in GOLDEN["grads_slices"]:
        sub = {}
        for kind in GOLDEN["kinds"]:
            fields = sub[kind] = layout(fn, BUILDS[build], kind, w)
            name, args = GRADS_TOTAL[kind]
            total = fn[BUILDS[build] + name[len("lotus_"):]](*[w[a] for a in args.split()])
            end = 0
            for off, length in fields:   # slab order: ascending, so disjoint means each starts at or after the previous end
                assert off >= end and off % 4 == 0 and length > 0, (kind, w, off, length, end)
                end = off + length
            assert end <= total, (kind, w, end, total)
        # the pair is its five sub-blocks one after the other, each shifted by the totals of those before it
        want, base = [], 0
        for part in PAIR_PARTS:
            want += [[base + off, length] for off, length in sub[part]]
            name, args = GRADS_TOTAL[part]
            base += fn[BUILDS[build] + name[len("lotus_"):]](*[w[a] for a in args.split()])
        assert sub["pair"] == want, w


def test_layout_query_reports_the_count_beyond_cap_and_refuses_an_unknown_kind(fn):
    w = GOLDEN["grads_slices"][0]
    assert len(layout(fn, "lotus_", "pair", w)) == 38
    off, length = np.full(4, -1, dtype=np.int64), np.full(4, -1, dtype=np.int64)
    assert fn["lotus_composite_grads_layout"](5, w["C"], w["H"], w["Hd"], w["Cc"], off.ctypes.data, length.ctypes.data, 3) == 38
    assert off[3] == -1 and length[3] == -1 and off[2] > 0   # nothing written past cap
    before = fn["lotus_last_error"]()   # (whatever an earlier test of the session left on this thread)
    got = []   # (the error message is thread-local: provoked on a thread of its own, this thread's stays as it was for later tests)

    def unknown_kind():
        got.append((fn["lotus_composite_grads_layout"](6, 64, 2, 256, 256, None, None, 0), fn["lotus_last_error"]()))

    t = threading.Thread(target=unknown_kind)
    t.start()
    t.join()
    assert got[0][0] < 0 and b"kind 6" in got[0][1]
    assert fn["lotus_last_error"]() == before


def test_pair_argument_names_come_from_the_library_in_the_order_python_spelled_them(fn):
    assert fn["lotus_pair_ptr_names"]().decode().split() == GOLDEN["pair_ptr_names"]
    assert fn["lotus_pair_int_names"]().decode().split() == GOLDEN["pair_int_names"]
    assert fn["lotus_pair_nptr"]() == len(GOLDEN["pair_ptr_names"]) and fn["lotus_pair_nint"]() == len(GOLDEN["pair_int_names"])
    from robot_3dlotus_amd import ops

    _, pp, pi, slots = ops._pair_tables()
    assert [n for n, _ in sorted(pp.items(), key=lambda kv: kv[1])] == GOLDEN["pair_ptr_names"]
    assert [n for n, _ in sorted(pi.items(), key=lambda kv: kv[1])] == GOLDEN["pair_int_names"]
    assert slots == [GOLDEN["pair_ptr_names"].index(n) for n in ops._PAIR_PARAM_SLOTS] and len(slots) == 38


def test_ops_views_follow_the_library_layout(fn):
    """ops._grad_views on a CPU slab filled with its own indices: every returned tensor starts where the fixture says the
    node's backward used to slice, in the node's return order, with the weights' 2-D shapes."""
    import torch
    from robot_3dlotus_amd import ops

    shapes = lambda C, Hd, Cc, cs: {"ffn": [(Hd, C), (C, Hd)], "selfattn": [(3 * C, C), (C, C)], "crossattn": [(C, C), (2 * C, Cc), (C, C)],
                                    "crossattn_kv": [(C, C), (C, C)], "cpe": [cs, (C, C)]}
    for w in GOLDEN["grads_slices"]:
        C, H, Hd, Cc = w["C"], w["H"], w["Hd"], w["Cc"]
        if C > 256:   # (float32 holds the indices of these slabs exactly; the wide ones add nothing but time)
            continue
        cshape = torch.Size((C, 3, 3, 3, C))
        two = shapes(C, Hd, Cc, tuple(cshape))
        two["pair"] = sum((two[k] for k in PAIR_PARTS), [])
        for kind, okind in (("ffn", "ffn"), ("selfattn", "self"), ("crossattn", "cross"), ("crossattn_kv", "crosskv"), ("cpe", "cpe"),
                            ("pair", "pair")):
            name, args = GRADS_TOTAL[kind]
            slab = torch.arange(fn[name](*[w[a] for a in args.split()]), dtype=torch.float32)
            views = ops._grad_views(slab, okind, C, H, Hd, Cc, cshape)
            want = w["fields"][kind] or layout(fn, "lotus_", kind, w)   # (the padded pair: checked against the parts above)
            if kind in ("cpe", "pair"):   # CpeFn / PairFn return dcw, dcb, dlw, dlb, dg, db
                want = [want[i] for i in (4, 5, 2, 3, 0, 1)] + want[6:]
            assert [(int(v.reshape(-1)[0]), v.numel()) for v in views] == [tuple(f) for f in want], (kind, C)
            assert all(v.is_contiguous() and v._base is slab for v in views)
            two_d = [tuple(v.shape) for v in views if v.dim() != 1]
            assert two_d == two[kind], (kind, C)
