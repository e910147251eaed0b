"""The regression action head (preset v1_reg: heatmap_mlp positions, euler rotations) against the published head (preset v1)
at 16 x 4096: forward + loss + backward, samples/s.

    python tools/reghead_bench.py [--steps 20] [--windows 5] [--out path.json]
    rocprofv3 --kernel-trace --stats -- python tools/reghead_bench.py --steps 5 --windows 1     # per-kernel means

The two models alternate window by window in ONE process (same clouds and instructions, same warm-up; the v1_reg batch carries
rotation labels in (-1, 1) instead of bins); each reports the median and the range of its windows.  The v1 path is the
yardstick: the regression head does strictly less work (4 instead of 90 logit columns, no [N, 90] cross entropy), so its median
is expected not to lie below v1's by more than the spread of the v1 windows.
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
from robot_3dlotus_amd import _capi, config as lcfg, synth  # noqa: E402
from robot_3dlotus_amd.policy import SimplePolicyPTV3CA  # noqa: E402


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
    models = {"v1_reg": SimplePolicyPTV3CA(lcfg.preset("v1_reg")).cuda().train(),
              "v1": SimplePolicyPTV3CA(lcfg.preset("v1")).cuda().train()}
    batches = {"v1_reg": _dev(synth.augment_clouds(synth.synth_batch(16, 4096, seed=0, rot_type="euler"), seed=1)),
               "v1": _dev(synth.augment_clouds(synth.synth_batch(16, 4096, seed=0), seed=1))}

    def step(k):
        m = models[k]
        _, losses = m(batches[k], compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        for p in m.parameters():
            p.grad = None

    for k in models:
        for _ in range(a.warmup):
            step(k)
    torch.cuda.synchronize()
    rates = {k: [] for k in models}
    for _ in range(a.windows):
        for k in models:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(k)
            torch.cuda.synchronize()
            rates[k].append(16 * a.steps / (time.perf_counter() - t0))
    res = {k: float(np.median(v)) for k, v in rates.items()}
    res["range"] = {k: [float(min(v)), float(max(v))] for k, v in rates.items()}
    res["windows"] = rates
    res["v1_reg_over_v1"] = res["v1_reg"] / res["v1"]
    res["v1_spread"] = res["range"]["v1"][1] - res["range"]["v1"][0]
    res["v1_reg_not_below_v1_by_more_than_its_spread"] = bool(res["v1_reg"] >= res["v1"] - res["v1_spread"])
    res["library_sha256_16"] = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
