"""Diagnostic: stand-alone timing of the patch attention with the relative-position term (lotus_attention_rpe_fwd / _bwd,
csrc/attention_rpe.hip) against the existing exact-fp32 tile kernels (lotus_attention_fwd / _bwd) on the same tiles, per level of
the v1 hierarchy at the bench size (16 clouds of 4096 points, the flash patching: K = 128).  Microseconds per call, best of three
runs of ten.   python tools/rpe_bench.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops, synth
    from robot_3dlotus_amd.frontend import FrontEnd

    batch = synth.synth_batch(16, 4096, seed=0)
    perms = [[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0], [0, 2, 1, 3]]
    levels = FrontEnd(5).build(batch["pc_fts"].cuda(), batch["npoints_in_batch"], batch["txt_lens"], perms)
    bnd = ops.rpe_bound(128)
    out = {}

    def timeit(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / 10 * 1e3)
        return round(best, 1)

    for lv, C, H in ((0, 64, 2), (0, 128, 4), (1, 128, 4), (2, 256, 8), (3, 512, 16), (4, 768, 32)):
        L = levels[lv]
        d = C // H
        g = torch.Generator(device="cuda").manual_seed(lv)
        qkv = torch.randn(L.n, 3 * C, device="cuda", generator=g)
        dout = torch.randn(L.n, C, device="cuda", generator=g)
        table = torch.randn(3 * (2 * bnd + 1), H, device="cuda", generator=g) * 0.02
        att = torch.empty(L.n, C, device="cuda")
        lse = torch.empty(L.npad, H, device="cuda")
        dqkv = torch.empty(L.n, 3 * C, device="cuda")
        extra = torch.empty(max(L.n_extra, 1), 2 * C, device="cuda")
        for tag, qn in (("norm", (torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"))), ("plain", None)):
            a = (qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, L.gidx, L.gidx, L.owner, L.self_tiles)
            tail = (L.kext, L.ext_pos, L.n_extra, extra)
            key = f"L{lv} C{C} H{H} {tag} tiles {L.n_self_tiles}"
            out[key] = {
                "fwd": timeit(lambda: ops.attention_fwd(*a, L.n_self_tiles, qn, qn, att, lse, H, d)),
                "fwd_rpe": timeit(lambda: ops.attention_rpe_fwd(*a, L.n_self_tiles, qn, qn, att, lse, H, d, L.grid, table, bnd)),
                "bwd": timeit(lambda: ops.attention_bwd(*a, L.self_blocks, L.n_self_tiles, qn, qn, att, dout, lse, dqkv, 3 * C, 0,
                                                        dqkv, 3 * C, C, 2 * C, 0, 0, H, d, 0.0, 0, *tail)),
                "bwd_rpe": timeit(lambda: ops.attention_rpe_bwd(*a, L.self_blocks, L.n_self_tiles, qn, qn, att, dout, lse, dqkv,
                                                                3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, H, d, L.grid, table, bnd, 0.0, 0,
                                                                *tail)),
            }
    import hashlib
    from robot_3dlotus_amd import _capi
    print(json.dumps({"library_sha256": hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16], "us_per_call": out},
                     indent=1))


if __name__ == "__main__":
    main()
