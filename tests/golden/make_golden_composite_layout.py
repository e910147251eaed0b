"""Write tests/golden/composite_layout.json: the buffer layouts of the composite entry points (csrc/blocks.cpp) as they were
BEFORE each sub-block kind got one layout definition.  Run once, at that parent commit, on a box without a GPU:

    python tests/golden/make_golden_composite_layout.py

The fixture holds, over the grid below,
  * every lotus_{ffn,selfattn,crossattn,crossattn_kv,cpe,pair}_*_floats / *_ws_*_bytes value of the fp32 build and of its
    bf16-storage twin (size queries only: nothing is launched),
  * the (offset, length) of every parameter gradient inside the `grads` slab, in slab order, from the slicing arithmetic the
    autograd nodes of ops.py used at that commit (written out once below, copied from CpeFn / FfnFn / SelfAttnFn /
    CrossAttnFn / CrossAttnKvFn.backward and _pair_grad_sizes),
  * ops._PP_NAMES / _PI_NAMES: the pair's argument tables as Python spelled them.
tests/test_composite_layout.py compares the library of the current commit against it.
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "composite_layout.json")

# (C, H): the five v1 stage widths with their heads, the tiny preset (64, 2), and one width whose head dimension is no
# multiple of 4 floats (d = 6: the al4 rounding of the q/k-norm gradients pads)
WIDTHS = [(64, 2), (128, 4), (256, 8), (512, 16), (768, 32), (24, 4)]
ROWS = [1, 361, 1450, 6077, 65537]
CC = 256          # context channels of every preset
PATCH = 128


def grid():
    out = []
    for (C, H), M, L, G, n_extra in itertools.product(WIDTHS, ROWS, (1, 128), (1, 3), (0, 1)):
        npad = (M + PATCH - 1) // PATCH * PATCH
        out.append({"M": M, "C": C, "H": H, "Hd": 4 * C, "Cc": CC, "L": L, "G": G, "n_extra": n_extra, "npad": npad,
                    "nblocks": npad // PATCH, "nblocks_ca": (M + 63) // 64 * G})
    return out


QUERIES = {
    "lotus_ffn_saved_floats": "M C Hd", "lotus_ffn_grads_floats": "C Hd", "lotus_ffn_tmp_floats": "M C Hd",
    "lotus_ffn_ws_main_bytes": "M C Hd", "lotus_ffn_ws_side_bytes": "M C Hd",
    "lotus_selfattn_saved_floats": "M C H npad", "lotus_selfattn_grads_floats": "C H", "lotus_selfattn_tmp_floats": "M C n_extra",
    "lotus_selfattn_ws_main_bytes": "M C H nblocks", "lotus_selfattn_ws_side_bytes": "M C",
    "lotus_crossattn_saved_floats": "M C H L", "lotus_crossattn_grads_floats": "C H Cc", "lotus_crossattn_tmp_floats": "M C L G",
    "lotus_crossattn_ws_main_bytes": "M C H L Cc nblocks_ca", "lotus_crossattn_ws_side_bytes": "M C L Cc",
    "lotus_crossattn_kv_saved_floats": "M C H", "lotus_crossattn_kv_grads_floats": "C H", "lotus_crossattn_kv_tmp_floats": "M C L G",
    "lotus_crossattn_kv_ws_main_bytes": "M C H nblocks_ca", "lotus_crossattn_kv_ws_side_bytes": "M C",
    "lotus_cpe_saved_floats": "M C", "lotus_cpe_grads_floats": "C", "lotus_cpe_tmp_floats": "M C", "lotus_cpe_ws_main_bytes": "M C",
    "lotus_cpe_ws_conv_bytes": "M C", "lotus_cpe_ws_side_bytes": "M C",
    "lotus_pair_acts_floats": "M C", "lotus_pair_saved_floats": "M C H Hd npad", "lotus_pair_grads_floats": "C H Hd",
    "lotus_pair_tmp_floats": "M C Hd n_extra L G", "lotus_pair_ws_main_bytes": "M C H Hd nblocks nblocks_ca",
    "lotus_pair_ws_side_bytes": "M C Hd", "lotus_pair_ws_conv_bytes": "M C",
}
KINDS = ("ffn", "selfattn", "crossattn", "crossattn_kv", "cpe", "pair")   # kind codes 0..5 of the layout query


def _al4(n):
    return (n + 3) & ~3


def python_slices(kind, C, H, Hd, Cc):
    """(offset, length) of each gradient in the slab, as the backward methods of ops.py sliced it."""
    d = C // H
    d4 = _al4(d)
    o1 = 2 * _al4(C)
    head = [(0, C), (_al4(C), C)]
    if kind == "ffn":
        o2 = o1 + _al4(Hd * C + Hd)
        return head + [(o1, Hd * C), (o1 + Hd * C, Hd), (o2, C * Hd), (o2 + C * Hd, C)]
    if kind == "selfattn":
        o2 = o1 + _al4(3 * C * C + 3 * C)
        o3 = o2 + 4 * d4
        return head + [(o1, 3 * C * C), (o1 + 3 * C * C, 3 * C), (o2, d), (o2 + d4, d), (o2 + 2 * d4, d), (o2 + 3 * d4, d),
                       (o3, C * C), (o3 + C * C, C)]
    if kind == "crossattn":
        o2 = o1 + _al4(C * C + C)
        o3 = o2 + _al4(2 * C * Cc + 2 * C)
        o4 = o3 + 4 * d4
        return head + [(o1, C * C), (o1 + C * C, C), (o2, 2 * C * Cc), (o2 + 2 * C * Cc, 2 * C), (o3, d), (o3 + d4, d),
                       (o3 + 2 * d4, d), (o3 + 3 * d4, d), (o4, C * C), (o4 + C * C, C)]
    if kind == "crossattn_kv":
        o2 = o1 + _al4(C * C + C)
        o3 = o2 + 4 * d4
        return head + [(o1, C * C), (o1 + C * C, C), (o2, d), (o2 + d4, d), (o2 + 2 * d4, d), (o2 + 3 * d4, d), (o3, C * C),
                       (o3 + C * C, C)]
    if kind == "cpe":
        o2 = o1 + _al4(C * C + C)
        return head + [(o1, C * C), (o1 + C * C, C), (o2, C * 27 * C), (o2 + C * 27 * C, C)]
    if kind == "pair":   # _pair_grad_sizes + Tensor.split: only valid while nothing is padded, which it asserted
        if not (C % 4 == 0 and d % 4 == 0 and Hd % 4 == 0):
            return None
        cpe = [C, C, C * C, C, 27 * C * C, C]
        att = [C, C, 3 * C * C, 3 * C, d, d, d, d, C * C, C]
        ffn = [C, C, Hd * C, Hd, C * Hd, C]
        ca = [C, C, C * C, C, d, d, d, d, C * C, C]
        out, o = [], 0
        for n in cpe + att + ffn + ca + ffn:
            out.append((o, n))
            o += n
        return out
    raise KeyError(kind)


def main():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi, ops

    fn = _capi.lib().fn
    g = grid()
    values = {}
    for build, prefix in (("fp32", "lotus_"), ("b16", "lotus_b16_")):
        values[build] = {name: [fn[prefix + name[6:]](*[p[a] for a in args.split()]) for p in g] for name, args in QUERIES.items()}
    widths = sorted({(p["C"], p["H"], p["Hd"], p["Cc"]) for p in g})
    slices = [{"C": C, "H": H, "Hd": Hd, "Cc": Cc, "fields": {k: python_slices(k, C, H, Hd, Cc) for k in KINDS}}
              for C, H, Hd, Cc in widths]
    doc = {"grid": g, "queries": {n: a.split() for n, a in QUERIES.items()}, "values": values, "kinds": list(KINDS),
           "grads_slices": slices, "pair_ptr_names": list(ops._PP_NAMES), "pair_int_names": list(ops._PI_NAMES)}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(g), "grid points")


if __name__ == "__main__":
    main()
