"""SimplePolicyPTV3AdaNorm (v1) against SimplePolicyPTV3CA (v1) at 16 x 4096: forward + loss + backward, samples/s.

    python tools/adanorm_bench.py [--steps 20] [--windows 5] [--out path.json]
    python tools/adanorm_bench.py --rehearsal [--steps 20] [--windows 5] [--out path.json]
    python tools/adanorm_bench.py --presets adanorm_v1,adanorm_v1_plain [--steps 20] [--windows 5] [--out path.json]
    python tools/adanorm_bench.py --presets adanorm_yaml --add-coords qk [--steps 20] [--windows 5] [--out path.json]

The two models alternate window by window in one process (same batch, same warm-up); each reports the median of its
windows.  The AdaNorm batch carries one instruction token per cloud (txt_reduce 'mean', instr_embed_type 'last').

--presets A,B: two presets of config.preset() instead (built through policy.MODEL_FACTORY), e.g. the AdaNorm policy with and
without q/k LayerNorm in the patch attention; reports both medians, the window rates, B over A and the library hash.

--add-coords {none,qk,qkv}: ptv3_config.add_coords_in_attn of the presets.  With ONE preset name the preset as it is (A) alternates
with the preset under that mode (B, reported as "<name>+<mode>"): the cost of the coordinate term of the patch attention; with two
names the mode is set in both.  A preset with 6 input channels / 'euler' rotations (the shipped YAML) gets the batch cut and
labelled for it.

--rehearsal: the one-rank RCCL rehearsal of the data-parallel AdaNorm step (LOTUS_FORCE_COLLECTIVES=1, nccl backend: every
collective of the step goes through the real library on one device) against the plain AdaNorm step, alternating windows in one
process on the training stream.  The rehearsal step is parallel.GradReducer + parallel.enable_sync_batchnorm — bucketed AVG
all-reduces from backward hooks, the split BatchNorm passes with their fp64 statistics messages — and reports both medians,
their ratio and the statistics messages per step (9 forward + 9 backward for the five-stage v1 model).
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
    ap.add_argument("--rehearsal", action="store_true", help="one-rank RCCL data-parallel step against the plain AdaNorm step")
    ap.add_argument("--presets", default=None, help="A,B: two presets of config.preset() to alternate instead of AdaNorm / CA")
    ap.add_argument("--add-coords", default="none", choices=("none", "qk", "qkv"),
                    help="add_coords_in_attn of the presets; with one preset name: the preset as it is against the preset with it")
    a = ap.parse_args()
    if a.rehearsal:
        return rehearsal(a)
    torch.manual_seed(0)
    batch = au.last_token_batch(synth.augment_clouds(synth.synth_batch(16, 4096, seed=0), seed=1))
    batches = {}
    if a.presets:
        from robot_3dlotus_amd.policy import MODEL_FACTORY

        names = a.presets.split(",")
        if a.add_coords != "none" and len(names) == 1:
            variants = [(names[0], "none"), (f"{names[0]}+{a.add_coords}", a.add_coords)]
        else:
            assert len(names) == 2 and names[0] != names[1], "--presets takes two different preset names: A,B"
            variants = [(n, a.add_coords) for n in names]
        models = {}
        for label, mode in variants:
            cfg = lcfg.preset(label.split("+")[0])
            if a.add_coords != "none":
                cfg.ptv3_config.add_coords_in_attn = mode
            models[label] = MODEL_FACTORY[cfg.model_class](cfg).cuda().train()
            if cfg.action_config.rot_pred_type == "euler" or cfg.ptv3_config.in_channels != batch["pc_fts"].shape[1]:
                bb = au.last_token_batch(synth.augment_clouds(synth.synth_batch(16, 4096, seed=0, rot_type=cfg.action_config.rot_pred_type),
                                                              seed=1))
                bb["pc_fts"] = bb["pc_fts"][:, :cfg.ptv3_config.in_channels].contiguous()
                batches[label] = _dev(bb)
    else:
        assert a.add_coords == "none", "--add-coords goes with --presets"
        models = {"adanorm": SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).cuda().train(),
                  "ca": SimplePolicyPTV3CA(lcfg.preset("v1")).cuda().train()}
    b = _dev(batch)
    for k in models:
        batches.setdefault(k, b)
    batch_of = {id(m): batches[k] for k, m in models.items()}

    def step(m):
        _, losses = m(batch_of[id(m)], compute_loss=True, compute_final_action=False)
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
    ka, kb = list(models)
    res[f"{ka}_over_{kb}" if not a.presets else f"{kb}_over_{ka}"] = (res[ka] / res[kb]) if not a.presets else (res[kb] / res[ka])
    if a.presets:
        import hashlib

        from robot_3dlotus_amd import _capi
        res["library_sha256_16"] = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def rehearsal(a):
    import hashlib

    import torch.distributed as dist

    from robot_3dlotus_amd import _capi, ops, parallel

    os.environ["LOTUS_FORCE_COLLECTIVES"] = "1"
    parallel.init_distributed()
    torch.cuda.set_stream(parallel.training_stream())
    torch.manual_seed(0)
    b = _dev(au.last_token_batch(synth.augment_clouds(synth.synth_batch(16, 4096, seed=0), seed=1)))
    plain = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).cuda().train()
    model = SimplePolicyPTV3AdaNorm(lcfg.preset("adanorm_v1")).cuda().train()
    model.load_state_dict(plain.state_dict())
    reducer = parallel.GradReducer(model, bucket_mb=32.0)
    parallel.enable_sync_batchnorm()
    hook = ops.BnState.reduce
    assert hook is not None, "the statistics hook was not installed (no process group?)"
    params = list(plain.parameters())

    def step_plain():
        ops.BnState.reduce = None
        for p in params:
            p.grad = None
        _, losses = plain(b, compute_loss=True, compute_final_action=False)
        losses["total"].backward()

    def step_dp():
        ops.BnState.reduce = hook
        reducer.zero_grad()
        _, losses = model(b, compute_loss=True, compute_final_action=False)
        losses["total"].backward()
        reducer.finish()

    steps = {"plain": step_plain, "rehearsal": step_dp}
    for f in steps.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    rates = {k: [] for k in steps}
    msgs = 0
    for _ in range(a.windows):
        for k, f in steps.items():
            torch.cuda.synchronize()
            m0 = parallel.BN_MESSAGES
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            rates[k].append(16 * a.steps / (time.perf_counter() - t0))
            if k == "rehearsal":
                msgs = (parallel.BN_MESSAGES - m0) / a.steps
            else:
                assert parallel.BN_MESSAGES == m0, "the plain step sent statistics messages"
    res = {k: float(np.median(v)) for k, v in rates.items()}
    res["windows"] = rates
    res["rehearsal_over_plain"] = res["rehearsal"] / res["plain"]
    res["bn_messages_per_step"] = msgs
    res["dist_backend"] = dist.get_backend()
    res["native_rccl_lanes"] = {"comm": reducer._lane_comm is not None, "main": reducer._lane_main is not None,
                                "streams_independent": reducer.lanes_independent}
    res["inplace_fraction"] = reducer.inplace_floats / max(1, reducer.inplace_floats + reducer.copied_floats)
    res["library_sha256_16"] = hashlib.sha256(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:16]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ops.BnState.reduce = None
    torch.cuda.synchronize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
