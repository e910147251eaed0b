"""SimplePolicyPTV3Concat (preset concat_yaml) at 16 x 4096: the context stem (concat.CtxStemFn: thin convolution of the point
columns + lotus_ctx_taps_fwd / _bwd over a [B, 125, cout] table) against the direct stem — the [N, c_pc + 256] concatenation
materialised and sent through the library's own conv_fwd / conv_wgrad / conv_dgrad, as the reference computes it — forward + loss +
backward in samples/s, and the stem node alone (forward + backward) in milliseconds.

    python tools/concat_bench.py [--steps 20] [--windows 5] [--out path.json]

The variants alternate window by window in one process (same model object, same batch, same warm-up); each reports the median of
its windows.  The direct stem pads the concatenation from 262 to 264 columns (two zero columns, zero weights): the duplicate-voxel
pass of the input gradient takes multiples of 4.  The library hash is recorded.  Kernel means: run this tool once under a kernel
trace with --steps 5 --windows 1.  Nothing is asserted.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import robot_3dlotus_amd  # noqa: E402,F401
from robot_3dlotus_amd import _capi, concat, config as lcfg, ops, synth  # noqa: E402
from robot_3dlotus_amd.policy import MODEL_FACTORY  # noqa: E402
import adanorm_util as au  # noqa: E402

CtxStemFn = concat.CtxStemFn


class DirectStemFn(torch.autograd.Function):
    """concat.CtxStemFn's contract through the materialised concatenation: x = [pc | ctx[b(i)] | 0 pad] [N, 264], one convolution,
    its weight gradient, and d ctx as per-cloud sums of the input gradient's context columns."""

    @staticmethod
    def forward(ctx, pc, cvec, w_pc, w_ctx, g, b, rmean, rvar, lvl, training):
        cout, c_pc, Cc = w_pc.shape[0], w_pc.shape[-1], cvec.shape[1]
        T = w_ctx.shape[0] // cout
        pad = (-(c_pc + Cc)) % 4
        x = torch.cat([pc, cvec[lvl.batch.long()], pc.new_zeros(pc.shape[0], pad)], 1)
        w = torch.cat([w_pc.reshape(cout, T, c_pc), w_ctx.view(T, cout, Cc).permute(1, 0, 2), w_pc.new_zeros(cout, T, pad)], 2)
        w = w.reshape(cout, 5, 5, 5, c_pc + Cc + pad).contiguous()
        c = ops.conv_fwd(x, w, None, lvl.nbr125, lvl.order[0])
        y, mean, invstd = ops.bn_fwd(c, g, b, rmean, rvar, training, ops.ACT_GELU)
        ctx.meta = (lvl, training, c_pc, Cc, T)
        ctx.save_for_backward(x, w, g, b, c, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, g, b, c, mean, invstd = ctx.saved_tensors
        lvl, training, c_pc, Cc, T = ctx.meta
        cout = w.shape[0]
        dc, dg, db = ops.bn_bwd(dy.contiguous(), c, mean, invstd, g, b, training, ops.ACT_GELU)
        dw, _ = ops.conv_wgrad(dc, x, w.shape, lvl.nbr125, need_bias=False)
        dx = ops.conv_dgrad(dc, w, lvl.nbr125, lvl.order[0], lvl=lvl)
        ops.sync_side_stream()
        dw = dw.view(cout, T, -1)
        dcvec = dx.new_zeros(len(lvl.counts), Cc).index_add_(0, lvl.batch.long(), dx[:, c_pc:c_pc + Cc])
        dw_ctx = dw[..., c_pc:c_pc + Cc].permute(1, 0, 2).reshape(T * cout, Cc)
        return None, dcvec, dw[..., :c_pc].reshape(cout, 5, 5, 5, c_pc), dw_ctx, dg, db, None, None, None, None


def _dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in b.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = lcfg.preset("concat_yaml")
    model = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
    batch = au.last_token_batch(synth.synth_batch(a.clouds, a.points, seed=0, rot_type="euler"))
    batch["pc_fts"] = batch["pc_fts"][:, :6].contiguous()
    batch = _dev(batch)

    def step():
        _, losses = model(batch, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        for p in model.parameters():
            p.grad = None

    def with_stem(fn):
        def run():
            concat.CtxStemFn = fn
            try:
                step()
            finally:
                concat.CtxStemFn = CtxStemFn
        return run

    # the stem node alone, on the level tables and tensors of one pass of the model
    bb = model.ptv3_model
    with torch.no_grad():
        pb = model.prepare_ptv3_batch(model.prepare_batch(dict(batch)))
    lvl = bb.frontend.build(pb["feat"], pb["counts"], pb["context_counts"], [[0, 1, 2, 3]] * bb.num_stages)[0]
    st = bb.embedding.stem
    cvec = pb["stem_context"].detach().clone().requires_grad_(True)
    dout = torch.randn(lvl.n, st.conv.weight.shape[0], device="cuda")

    def stem_only(fn):
        def run():
            w_pc, w_ctx = concat.split_stem_weight(st.conv.weight, bb.pc_channels)
            y = fn.apply(pb["feat"], cvec, w_pc, w_ctx, st.norm.weight, st.norm.bias, st.norm.running_mean.clone(),
                         st.norm.running_var.clone(), lvl, True)
            y.backward(dout)
            st.conv.weight.grad = st.norm.weight.grad = st.norm.bias.grad = cvec.grad = None
        return run

    variants = {"concat_yaml_ctx_stem": with_stem(CtxStemFn), "concat_yaml_direct_stem": with_stem(DirectStemFn)}
    stems = {"stem_ctx_ms": stem_only(CtxStemFn), "stem_direct_ms": stem_only(DirectStemFn)}
    for f in list(variants.values()) + list(stems.values()):
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    rates = {k: [] for k in list(variants) + list(stems)}
    for _ in range(a.windows):
        for k, f in list(variants.items()) + list(stems.items()):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates[k].append(a.clouds * a.steps / dt if k in variants else 1e3 * dt / a.steps)
    res = {k: float(np.median(v)) for k, v in rates.items()}
    res["windows"] = rates
    res["ctx_over_direct"] = res["concat_yaml_ctx_stem"] / res["concat_yaml_direct_stem"]
    res["stem_direct_over_ctx"] = res["stem_direct_ms"] / res["stem_ctx_ms"]
    res["clouds"], res["points"], res["rows"], res["n_dup"] = a.clouds, a.points, int(lvl.n), int(lvl.n_dup)
    res["taps_present_mean"] = float((lvl.nbr125 >= 0).float().sum(0).mean().item())
    res["library_sha256_16"] = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
