"""Shared helpers of the SimplePolicyPTV3AdaNorm fixtures (tests/golden/make_golden_adanorm.py) and their tests: case table,
batch derivation, gradient sketches.  No reference import here (the GPU tests use this module too)."""
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (reference variant, preset, txt_reduce, clouds, points, ragged, data seed, weight seed, train, full forward)
CASES = {
    "adanorm_tiny_scaled_train": ("tiny", "adanorm_tiny", "mean", 2, 512, False, 21, 31, True, False),
    "adanorm_v1_scaled_train": ("v1", "adanorm_v1", "attn", 2, 1024, True, 22, 32, True, True),
    "adanorm_v1_scaled_eval": ("v1", "adanorm_v1", "attn", 2, 1024, True, 23, 32, False, True),
    "adanorm_tinyctx_scaled_train": ("tinyctx", "adanorm_tinyctx", "mean", 2, 600, True, 24, 33, True, False),
}
GRAD_KEYS_SAMPLE = 48
SKETCH_K = 16  # random projections per sketched gradient
XT_SAMPLE = 16384  # position logits kept by a train-mode fixture (eval-mode fixtures keep all of them)


_WHOLE_SITES = ("norm", "modulation", "txt_", "pose_embedding", "stepid_embedding")


def stored_whole(name, shape):
    """The vector gradients of the norms (affines, qk-norms), the modulations (biases) and the context layers are stored whole;
    every other gradient (weight matrices, convolution kernels, the other biases) as a sketch (grad_sketch), which keeps each
    fixture small."""
    return len(shape) == 1 and any(s in name for s in _WHOLE_SITES)


def last_token_batch(batch):
    """instr_embed_type='last': one instruction token per cloud (what txt_reduce == 'mean' requires)."""
    lens = list(batch["txt_lens"])
    last = np.cumsum(lens) - 1
    out = dict(batch)
    out["txt_embeds"] = batch["txt_embeds"][torch.from_numpy(last)].contiguous()
    out["txt_lens"] = [1] * len(lens)
    return out


def case_batch(name):
    from robot_3dlotus_amd import synth

    _, _, reduce, B, n, ragged, dseed = CASES[name][:7]
    batch = synth.synth_batch(B, n, ragged=ragged, seed=dseed)
    return last_token_batch(batch) if reduce == "mean" else batch


def case_config(name):
    from robot_3dlotus_amd import config as lcfg

    cfg = lcfg.preset(CASES[name][1])
    cfg.action_config.txt_reduce = CASES[name][2]
    return cfg


def grad_sketch(g):
    """[SKETCH_K] float64 = U^T G v for the gradient as a matrix G [rows, cols] (rows = output dimension) and fixed Gaussian
    U [rows, K], v [cols]: a linear function of the WHOLE tensor, E ||U^T E v||^2 = K ||E||_F^2 for any error E, so a relative
    error of the sketch estimates the relative Frobenius error of the gradient."""
    g = np.asarray(g, dtype=np.float64).reshape(g.shape[0], -1)
    rows, cols = g.shape
    v = np.random.default_rng([7, cols]).standard_normal(cols)
    u = np.random.default_rng([11, rows]).standard_normal((rows, SKETCH_K))
    return u.T @ (g @ v)


def xt_sample_index(numel):
    """Fixed positions (sorted) of the flattened position logits that a train-mode fixture stores."""
    n = min(XT_SAMPLE, numel)
    return np.sort(np.random.default_rng([13, numel]).choice(numel, n, replace=False))


def pack_grads(named):
    """[(name, fp32 numpy gradient)] -> the fixture arrays: names, norms, leading entries, whole vectors, sketches (a handful
    of arrays instead of several per parameter: a zip member per array costs more than the data of most of them)."""
    names = [n for n, _ in named]
    P = len(names)
    head = np.full((P, GRAD_KEYS_SAMPLE), np.nan, np.float32)
    norm = np.zeros(P, np.float64)
    sketch = np.full((P, SKETCH_K), np.nan, np.float64)
    whole, off = [], [0]
    for i, (_, g) in enumerate(named):
        norm[i] = np.linalg.norm(g.astype(np.float64))
        h = g.reshape(-1)[:GRAD_KEYS_SAMPLE]
        head[i, :h.size] = h
        if stored_whole(names[i], g.shape):
            whole.append(g.reshape(-1).astype(np.float32))
        else:
            sketch[i] = grad_sketch(g)
        off.append(off[-1] + (g.size if stored_whole(names[i], g.shape) else 0))
    return {"g_names": np.array(json.dumps(names)), "g_norm": norm, "g_head": head, "g_sketch": sketch,
            "g_whole": np.concatenate(whole) if whole else np.zeros(0, np.float32), "g_whole_off": np.array(off, np.int64)}


def unpack_grads(fx):
    """-> {name: (norm, head, whole vector | None, sketch | None)} from a fixture written with pack_grads."""
    names = json.loads(str(fx["g_names"]))
    off = fx["g_whole_off"]
    out = {}
    for i, n in enumerate(names):
        head = fx["g_head"][i]
        head = head[np.isfinite(head)]
        whole = fx["g_whole"][off[i]:off[i + 1]] if off[i + 1] > off[i] else None
        sk = fx["g_sketch"][i] if whole is None else None
        out[n] = (float(fx["g_norm"][i]), head, whole, sk)
    return out


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
