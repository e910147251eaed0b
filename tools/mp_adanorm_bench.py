"""MotionPlannerPTV3AdaNorm (preset mp_yaml) at 8 x 4096: the soft trajectory head fused (ops.TrajSoftPosFn: lotus_mp_softpos_fwd /
_bwd, one pass over the point features each way) against the same model with the head composed from the per-step entry points
that were there before it (lotus_step_act_fwd -> lotus_softpos_fwd per step; lotus_softpos_bwd -> linear_wgrad / linear_dgrad ->
lotus_step_act_bwd), forward + loss + backward, samples/s.

    python tools/mp_adanorm_bench.py [--steps 20] [--windows 5] [--out path.json]

The variants alternate window by window in one process (same model object, same batch, same warm-up); each reports the median of
its windows.  The published `mp` preset (MotionPlannerPTV3CA, heat-map head) runs in the same alternation as context.  The library
hash is recorded.  Kernel means: run this tool once under a kernel trace with --steps 5 --windows 1.
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
from robot_3dlotus_amd import _capi, config as lcfg, ops, synth  # noqa: E402
from robot_3dlotus_amd.policy import MODEL_FACTORY  # noqa: E402
import mp_ada_util as mu  # noqa: E402

FusedFn = ops.TrajSoftPosFn


class ComposedSoftPosFn(torch.autograd.Function):
    """ops.TrajSoftPosFn from the per-step entry points: T hidden layers written, read by the 4-column product, kept for the weight
    gradient; backward accumulates dbase over T launches."""

    @staticmethod
    def forward(ctx, base, step_bias, w3, b3, pc_fts, lvl, temp, drop_p, seed):
        T = step_bias.shape[0]
        M, C = base.shape
        hs, es, xts, sts = [], [], [], []
        for t in range(T):
            h = torch.empty_like(base)
            ops.call("lotus_step_act_fwd", base, step_bias[t], h, M, C, ops.ACT_LEAKY, float(drop_p), ops.mix_seed(seed, t))
            e, xt, st = ops.softpos_fwd(h, w3, b3, pc_fts, lvl, temp)
            hs.append(h); es.append(e); xts.append(xt); sts.append(st)
        ctx.save_for_backward(base, step_bias, w3, pc_fts, *hs, *es, *xts, *sts)
        ctx.meta = (lvl, float(temp), float(drop_p), int(seed), T)
        return torch.stack(xts, 1)

    @staticmethod
    def backward(ctx, g):
        lvl, temp, p, seed, T = ctx.meta
        base, step_bias, w3, pc_fts = ctx.saved_tensors[:4]
        rest = ctx.saved_tensors[4:]
        hs, es, xts, sts = rest[:T], rest[T:2 * T], rest[2 * T:3 * T], rest[3 * T:]
        M, C = base.shape
        dbase, dsb = torch.empty_like(base), torch.empty_like(step_bias)
        ws = ops._ws(ops.query("lotus_step_act_bwd_workspace", M, C), base.device)
        into = None
        for t in range(T):
            de = ops.softpos_bwd(g[:, t].contiguous(), es[t], pc_fts, lvl, sts[t], xts[t], temp)
            into = ops.linear_wgrad(de, hs[t], into=into)
            dh = ops.linear_dgrad(de, w3)
            ops.call("lotus_step_act_bwd", dh, base, step_bias[t], dbase, dsb[t], M, C, ops.ACT_LEAKY, p, ops.mix_seed(seed, t),
                     1 if t else 0, ws, ws.numel())
        ops.sync_side_stream()
        return dbase, dsb, into[0], into[1], None, None, None, None, None


def _dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "gt_trajs_disc_pos_probs" else v))
            for k, v in b.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = lcfg.preset("mp_yaml")
    model = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
    batch = _dev(mu.mp_batch(a.clouds, a.points, False, 0, cfg.ptv3_config.in_channels))
    cfg_mp = lcfg.preset("mp")
    published = MODEL_FACTORY[cfg_mp.model_class](cfg_mp).cuda().train()
    batch_mp = _dev(synth.synth_batch_mp(a.clouds, a.points, seed=0))

    def step(m, b):
        _, losses = m(b, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        for p in m.parameters():
            p.grad = None

    def fused():
        ops.TrajSoftPosFn = FusedFn
        step(model, batch)

    def composed():
        ops.TrajSoftPosFn = ComposedSoftPosFn
        try:
            step(model, batch)
        finally:
            ops.TrajSoftPosFn = FusedFn

    variants = {"mp_yaml_fused": fused, "mp_yaml_composed": composed, "mp_published": lambda: step(published, batch_mp)}
    for f in variants.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    rates = {k: [] for k in variants}
    for _ in range(a.windows):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            rates[k].append(a.clouds * a.steps / (time.perf_counter() - t0))
    res = {k: float(np.median(v)) for k, v in rates.items()}
    res["windows"] = rates
    res["fused_over_composed"] = res["mp_yaml_fused"] / res["mp_yaml_composed"]
    res["clouds"], res["points"] = a.clouds, a.points
    res["library_sha256_16"] = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
