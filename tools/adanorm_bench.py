"""SimplePolicyPTV3AdaNorm (v1) against SimplePolicyPTV3CA (v1) at 16 x 4096: forward + loss + backward, samples/s.

    python tools/adanorm_bench.py [--steps 20] [--windows 5] [--out path.json]

The two models alternate window by window in one process (same batch, same warm-up); each reports the median of its
windows.  The AdaNorm batch carries one instruction token per cloud (txt_reduce 'mean', instr_embed_type 'last').
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import robot_3dlotus_amd  # noqa: E402,F401
from robot_3dlotus_amd import config as lcfg, synth  # noqa: E402
from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA  # noqa: E402
import adanorm_util as au  # noqa: E402


def _dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in b.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    batch = au.last_token_batch(synth.augment_clouds(synth.synth_batch(16, 4096, seed=0), seed=1))
    models = {"adanorm": SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).cuda().train(),
              "ca": SimplePolicyPTV3CA(lcfg.preset("v1")).cuda().train()}
    b = _dev(batch)

    def step(m):
        _, losses = m(b, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        for p in m.parameters():
            p.grad = None

    for m in models.values():
        for _ in range(a.warmup):
            step(m)
    torch.cuda.synchronize()
    rates = {k: [] for k in models}
    for _ in range(a.windows):
        for k, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(m)
            torch.cuda.synchronize()
            rates[k].append(16 * a.steps / (time.perf_counter() - t0))
    res = {k: float(np.median(v)) for k, v in rates.items()}
    res["windows"] = rates
    res["adanorm_over_ca"] = res["adanorm"] / res["ca"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
