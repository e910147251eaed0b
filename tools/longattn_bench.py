"""Diagnostic: stand-alone timing of the patch attention above 128 rows per patch (lotus_attention_long_fwd / _bwd,
csrc/attention_long.hip) at K = 256 and K = 1024 against the existing exact-fp32 tile kernels (lotus_attention_fwd / _bwd) at
K = 128 on the same rows: the levels of the v1 hierarchy at the bench size (16 clouds of 4096 points) whose clouds are longer than
128 points, with the H x d of those levels.  Microseconds per call (best of three runs of ten) and, since a patch of K rows has K
times as many (query, key) pairs per row as one of 128, picoseconds per pair and the ratio to K = 128.
    python tools/longattn_bench.py"""
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
    levels = {K: FrontEnd(5, patch_size=K).build(batch["pc_fts"].cuda(), batch["npoints_in_batch"], batch["txt_lens"], perms)
              for K in (128, 256, 1024)}
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

    for lv, C, H in ((0, 64, 2), (0, 128, 4), (1, 128, 4), (2, 256, 8)):
        d = C // H
        n = levels[128][lv].n
        g = torch.Generator(device="cuda").manual_seed(lv)
        qkv = torch.randn(n, 3 * C, device="cuda", generator=g)
        dout = torch.randn(n, C, device="cuda", generator=g)
        att = torch.empty(n, C, device="cuda")
        dqkv = torch.empty(n, 3 * C, device="cuda")
        for tag, qn in (("norm", (torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"))), ("plain", None)):
            key = f"L{lv} C{C} H{H} {tag} rows {n}"
            out[key] = {}
            for K in (128, 256, 1024):
                L = levels[K][lv]
                assert L.n == n
                lse = torch.empty(L.npad, H, device="cuda")
                extra = torch.empty(max(L.n_extra, 1), 2 * C, device="cuda")
                a = (qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, L.gidx, L.gidx, L.owner, L.self_tiles)
                tail = (L.kext, L.ext_pos, L.n_extra, extra)
                pairs = float((L.self_tiles[:, 1].double() * L.self_tiles[:, 3].double()).sum()) * H
                if K == 128:
                    fwd = timeit(lambda: ops.attention_fwd(*a, L.n_self_tiles, qn, qn, att, lse, H, d))
                    bwd = timeit(lambda: ops.attention_bwd(*a, L.self_blocks, L.n_self_tiles, qn, qn, att, dout, lse, dqkv, 3 * C, 0,
                                                           dqkv, 3 * C, C, 2 * C, 0, 0, H, d, 0.0, 0, *tail))
                elif not ops.long_tiles(L):
                    continue
                else:
                    fwd = timeit(lambda: ops.attention_long_fwd(*a, L.n_self_tiles, qn, qn, att, lse, H, d, L.tile_max))
                    bwd = timeit(lambda: ops.attention_long_bwd(*a, L.self_blocks, L.n_self_tiles, qn, qn, att, dout, lse, dqkv,
                                                                3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, H, d, L.tile_max, 0.0, 0, *tail))
                out[key][f"K{K}"] = {"tiles": L.n_self_tiles, "tile_max": L.tile_max, "fwd_us": fwd, "bwd_us": bwd,
                                     "fwd_ps_per_pair": round(fwd * 1e6 / pairs, 3), "bwd_ps_per_pair": round(bwd * 1e6 / pairs, 3)}
            base = out[key]["K128"]
            for K in (256, 1024):
                r = out[key].get(f"K{K}")
                if r:
                    r["fwd_per_pair_vs_K128"] = round(r["fwd_ps_per_pair"] / base["fwd_ps_per_pair"], 2)
                    r["bwd_per_pair_vs_K128"] = round(r["bwd_ps_per_pair"] / base["bwd_ps_per_pair"], 2)
    import hashlib
    from robot_3dlotus_amd import _capi
    print(json.dumps({"library_sha256": hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16], "results": out}, indent=1))


if __name__ == "__main__":
    main()
