"""parallel.GradReducer's slab arena on the device: the HIP nodes write their weight gradients straight into the reducer's
flat buffer (ops.GRAD_ARENA), and every gradient must be the one the same net computes without a reducer — PER PARAMETER, bit
for bit: the arena changes WHERE a gradient is written, not which kernel writes it (every served slab is 256-byte aligned, so
the route rules of the dense and convolution weight gradients see the alignment of a fresh allocation).

Toy nets of ops.LinearFn (tests/dp_util.py) in learnt, swapped and skipped node order, both join modes, with the weight-gradient
stream late (tests/side_stall.py); whole models with dropout on; gradient accumulation; and the optimiser trajectory under a
one-rank communicator with parameters whose usage flips."""
import json
import os
import subprocess
import sys

import pytest
import torch

import dp_util as du
import ledger
import side_stall

pytestmark = pytest.mark.gpu

JOINS = ["node", "end"]
W, ROWS = 64, 200            # Lin(64 -> 64): a slab of 4160 floats; Lin(64 -> 5): 325 floats (384 padded); x [200, 64]
EACH = du.mb(2)              # every layout unit in a bucket of its own


def _mods():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops, parallel

    return ops, parallel


def _x(seed):
    return torch.randn(ROWS, W, generator=torch.Generator().manual_seed(seed)).cuda()


def _reducer(net, bucket_mb=EACH):
    _, parallel = _mods()
    red = parallel.GradReducer(net, bucket_mb=bucket_mb)
    return red, du.ArenaLog(red)


class _Join:
    def __init__(self, join):
        self.join = join

    def __enter__(self):
        _mods()[0].set_wgrad_join(self.join)

    def __exit__(self, *a):
        torch.cuda.synchronize()
        _mods()[0].set_wgrad_join("node")


# ------------------------------------------------------------------------------------------------ toy nets, world 1
@pytest.mark.parametrize("join", JOINS)
def test_branches_learnt_and_swapped_order(join):
    sizes = [W, W, 5, W]
    net = du.Branches("hip", sizes, W).cuda()
    total = sum(p.numel() for p in net.parameters())
    base = [0, 1, 2, 3]
    # learning step, first arena step, steady step, two equal slabs swapped, all reversed (a request of another size), learnt again
    plan = [base, base, base, [1, 0, 2, 3], [3, 2, 1, 0], base]
    seen, compared = [], 0
    with _Join(join):
        red, log = _reducer(net)
        for k, order in enumerate(plan):
            x = _x(10 + k)
            inplace, copied, n = du.run_step(red, net, (x, order), du.plain_grads(net, x, order))
            assert n == 9 and inplace + copied == total
            seen.append((inplace, copied, len(log.take())))
            compared += n
    assert len({red._slot[b.weight] for b in net.br}) == 4
    assert seen[0] == (0, total, 0), seen
    assert seen[1] == seen[2] == seen[5] == (total - 3, 3, 4), seen      # everything but `scale` is born in its slot
    assert seen[3] == (4160 + 325, 2 * 4160 + 3, 4), seen     # branches 0 and 1 got each other's slab and were copied home
    assert seen[4] == (0, total, 1), seen                     # the second request has another size: the serving ends there
    ledger.record(f"reducer_arena_branches[{join}]", compared=compared, served=[s[2] for s in seen],
                  inplace_share=[s[0] / total for s in seen])


@pytest.mark.parametrize("join", JOINS)
def test_chain_with_a_skipped_node(join):
    net = du.Chain("hip", W).cuda()
    total = sum(p.numel() for p in net.parameters())
    plan = [1, 1, 1, 0, 1, 0]
    seen, compared = [], 0
    with _Join(join):
        red, log = _reducer(net)
        for k, use in enumerate(plan):
            x = _x(20 + k)
            want = du.plain_grads(net, x, bool(use))
            inplace, copied, n = du.run_step(red, net, (x, bool(use)), want)
            seen.append((use, n, inplace, copied, len(log.take())))
            compared += n
    # b skipped: c is born in place, a is served b's slab and copied home
    assert seen[0] == (1, 6, 0, total, 0), seen
    assert all(s == ((1, 6, total, 0, 3) if s[0] else (0, 4, 4160, 4160, 2)) for s in seen[1:]), seen
    ledger.record(f"reducer_arena_chain[{join}]", compared=compared, served=[s[4] for s in seen],
                  inplace_share=[s[2] / (s[2] + s[3]) for s in seen])


@pytest.mark.parametrize("join", JOINS)
def test_swapped_step_with_the_weight_gradient_stream_late(join):
    """The gradients of the swapped nodes are moved out of each other's slab: that copy must wait for the weight-gradient
    stream, which is still parked when the critical stream reaches the flush."""
    ops, _ = _mods()
    net = du.Branches("hip", [W, W, 5, W], W).cuda()
    base, swapped = [0, 1, 2, 3], [1, 0, 2, 3]
    x = _x(31)
    try:
        ops.enable_side_stream(False)          # the reference: one stream, nothing to race
        torch.cuda.synchronize()
        want = du.plain_grads(net, x, swapped)
        ops.enable_side_stream(True)
        ops.set_wgrad_join(join)
        red, log = _reducer(net)
        for k in range(2):
            du.run_step(red, net, (_x(32 + k), base))
        # one unstalled swapped step, timed: sizes the stall
        red.zero_grad()
        loss = net(x, swapped)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss.backward()
        e1.record()
        red.finish()
        n0 = du.check_step(red, net, want)
        ms = side_stall.stall_ms_for(e0.elapsed_time(e1))
        log.take()
        red.zero_grad()
        loss = net(x, swapped)
        with side_stall.Stall(join, ms) as st:
            loss.backward()
        red.finish()
        n1 = du.check_step(red, net, want)
        longest = st.check()
    finally:
        torch.cuda.synchronize()
        ops.enable_side_stream(True)
        ops.set_wgrad_join("node")
    assert longest <= side_stall.CAP_MS * 1.2 + 1.0, longest
    assert n0 == n1 == 9 and len(log.take()) == 4 and st.nodes == (4 if join == "node" else 1), (n0, n1, st.nodes)
    ledger.record(f"reducer_arena_stalled_swap[{join}]", compared=n0 + n1, stalled_nodes=st.nodes)


def test_gradient_accumulation_switches_the_arena_off():
    ops, _ = _mods()
    net = du.Branches("hip", [W, W, 5], W).cuda()
    total = sum(p.numel() for p in net.parameters())
    order = [0, 1, 2]
    red, log = _reducer(net)
    for k in range(2):
        du.run_step(red, net, (_x(40 + k), order))
    assert len(log.take()) == 3 and ops.GRAD_ARENA is None
    x1, x2 = _x(42), _x(43)
    want = du.plain_grads_accum(net, [(x1, order), (x2, [1, 0, 2])])
    c0, i0 = red.copied_floats, red.inplace_floats
    red.zero_grad()
    with red.no_sync():
        net(x1, order).backward()
    net(x2, [1, 0, 2]).backward()
    red.finish()
    n = du.check_step(red, net, want)
    assert red._arena_off and ops.GRAD_ARENA is None and not log.take()
    assert (red.copied_floats - c0, red.inplace_floats - i0) == (total, 0)
    # ... and for good: the next plain step packs by copy too
    x = _x(44)
    inplace, copied, n2 = du.run_step(red, net, (x, order), du.plain_grads(net, x, order))
    assert (inplace, copied) == (0, total) and not log.take()
    ledger.record("reducer_arena_accumulation", compared=n + n2, served=0)


# ------------------------------------------------------------------------------------------------ whole models
def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _model_case(preset):
    """-> (model class, configuration, host batch): synth_batch(2, 400, ragged) through the adapter the model's own tests use."""
    import adanorm_util as au
    import mp_ada_util as mu
    from robot_3dlotus_amd import config as lcfg, synth
    from robot_3dlotus_amd.motion_planner import MotionPlannerPTV3AdaNorm
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm, SimplePolicyPTV3CA, SimplePolicyPTV3Concat

    cfg = lcfg.preset(preset)
    if preset == "mp_ada_tiny":
        return MotionPlannerPTV3AdaNorm, cfg, mu.mp_batch(2, 400, True, 50, 4)
    batch = synth.synth_batch(2, 400, ragged=True, seed=50)
    if preset == "tiny":
        return SimplePolicyPTV3CA, cfg, batch
    if preset == "adanorm_tiny":
        cfg.action_config.txt_reduce = "mean"
    return {"adanorm_tiny": SimplePolicyPTV3AdaNorm, "concat_tiny": SimplePolicyPTV3Concat}[preset], cfg, au.last_token_batch(batch)


@pytest.mark.parametrize("preset", ["tiny", "adanorm_tiny", "concat_tiny", "mp_ada_tiny"])
def test_whole_model_three_steps_with_dropout(preset):
    """Three train-mode steps, dropout on, with the reducer against three without from the same state: torch's seed and the
    step counter in the state dict give both runs the same masks (tests/test_gpu_side_stream_lifetime.py).

    Measured on MI355X, in-place share of steps 2 and 3 / served slabs / tensors compared (all bit-equal): tiny 0.99946 / 13 /
    438, adanorm_tiny 0.99822 / 28 / 354, mp_ada_tiny 0.66066 / 25 / 345, concat_tiny 0.99568 / 18 / 300 — 0.23974 / 17 while
    the gradient of embedding.stem.conv.weight (75.6 % of that model's gradient floats) was assembled by autograd from the two
    slices of concat.split_stem_weight instead of in a slab (ops.SplitStemWeightFn)."""
    from weights_util import seeded_state_dict

    ops, _ = _mods()
    cls, cfg, host = _model_case(preset)
    batch = _dev(host)
    sd = seeded_state_dict(cls(cfg).state_dict(), 7, "scaled")

    def run(with_reducer):
        torch.manual_seed(5)
        m = cls(cfg)
        m.load_state_dict(sd)
        m = m.cuda().train()
        m.ptv3_model.order_perms = [[2, 0, 1, 3], [1, 3, 0, 2]]
        assert m.ptv3_model.proj_drop > 0.0
        red = log = None
        if with_reducer:
            red, log = _reducer(m, 0.5)
        else:
            assert ops.GRAD_ARENA is None
        steps = []
        for _ in range(3):
            if red is not None:
                i0, c0 = red.inplace_floats, red.copied_floats
                red.zero_grad()
            else:
                m.zero_grad(set_to_none=True)
            _, losses = m(batch, compute_loss=True, compute_final_action=False)
            losses["total"].backward()
            if red is not None:
                red.finish()
            torch.cuda.synchronize()
            grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}
            grads["loss"] = losses["total"].detach().clone()
            info = (red.inplace_floats - i0, red.copied_floats - c0, len(log.take())) if red is not None else None
            steps.append((grads, info))
        return steps

    got, want = run(True), run(False)
    bad, compared = [], 0
    for k, ((g, _), (w, _)) in enumerate(zip(got, want)):
        assert g.keys() == w.keys()
        for n in w:
            if w[n] is None or g[n] is None:
                if not (w[n] is None and g[n] is None):
                    bad.append((k, n, "one side has no gradient"))
                continue
            compared += 1
            if not torch.equal(g[n], w[n]):
                bad.append((k, n, float((g[n] - w[n]).abs().max()), float(w[n].abs().max())))
    assert compared > 3 * 50
    assert not bad, f"{len(bad)} of {compared} differ (step, parameter, max |diff|, max |plain|): {bad[:12]}"
    assert not torch.equal(want[0][0]["loss"], want[1][0]["loss"])            # (the masks do change from step to step)
    shares = [i / (i + c) for _, (i, c, _) in got]
    served = [s for _, (_, _, s) in got]
    print(f"{preset}: in-place shares {shares}, served slabs {served}, {compared} tensors")
    ledger.record(f"reducer_arena_model[{preset}]", compared=compared, inplace_share=shares, served=served)
    assert shares[0] == 0.0 and served[0] == 0 and shares[1] > 0.5 and shares[2] > 0.5 and served[1] == served[2] > 0, (shares, served)


# ------------------------------------------------------------------------------------------------ optimiser trajectory, one-rank communicator
_TRAJECTORY_SCRIPT = r"""
import os, sys, json
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch, torch.distributed as dist
import robot_3dlotus_amd
from robot_3dlotus_amd import ops, optim, parallel
import dp_util as du
os.environ["LOTUS_FORCE_COLLECTIVES"] = "1"
parallel.init_distributed()
dev = torch.device("cuda", 0)
torch.cuda.set_stream(parallel.training_stream())
USE_B, USE_AUX, CLIP = [1, 1, 0, 1, 0, 0, 1], [0, 1, 0, 1, 1, 0, 0], 1e-3
net_a = du.Chain("hip", 64, aux=5).to(dev)
net_b = du.twin(net_a)
red = parallel.GradReducer(net_a, bucket_mb=du.mb(2))
log = du.ArenaLog(red)
res = {"native": red._lane_comm is not None and red._lane_main is not None, "forced": bool(red._force)}
mk = lambda net: optim.AdamW(net.parameters(), lr=1e-2, weight_decay=0.01)
opt_a, opt_b = mk(net_a), mk(net_b)
names = [n for n, _ in net_a.named_parameters()]
pa, pb = dict(net_a.named_parameters()), dict(net_b.named_parameters())
bad, norms, served, compared = [], [], [], 0
for k, (ub, ua) in enumerate(zip(USE_B, USE_AUX)):
    x = torch.randn(200, 64, generator=torch.Generator().manual_seed(70 + k)).to(dev)
    # side A: the reducer's protocol, norm and update from its flat buffer
    red.zero_grad()
    net_a(x, bool(ub), bool(ua)).backward()
    red.finish()
    na = opt_a.clip_grad_norm_(CLIP, reducer=red)
    opt_a.step(reducer=red)
    torch.cuda.synchronize()
    # side B: no reducer (and no arena: finish() has taken it away); an unused parameter has .grad None
    for p in net_b.parameters():
        p.grad = None
    assert ops.GRAD_ARENA is None
    net_b(x, bool(ub), bool(ua)).backward()
    nb = opt_b.clip_grad_norm_(CLIP)
    torch.cuda.synchronize()
    gb = {n: (None if p.grad is None else p.grad.clone()) for n, p in pb.items()}
    opt_b.step()
    torch.cuda.synchronize()
    served.append(len(log.take()))
    norms.append(float(nb))
    if not torch.equal(na, nb):
        bad.append((k, "norm", float(na), float(nb)))
    mask = red.used_mask.tolist()
    for i, n in enumerate(names):
        v = red.view_of(pa[n])
        if gb[n] is None:
            if bool(v.ne(0).any()) or mask[red._index[pa[n]]] != 0:
                bad.append((k, n, "unused: slot not zero or flag set"))
        elif not torch.equal(v, gb[n]) or mask[red._index[pa[n]]] != 1:
            bad.append((k, n, "view_of", float((v - gb[n]).abs().max())))
        for what, ta, tb in (("param", pa[n].data, pb[n].data), ("exp_avg", opt_a.state[pa[n]]["exp_avg"], opt_b.state[pb[n]]["exp_avg"]),
                             ("exp_avg_sq", opt_a.state[pa[n]]["exp_avg_sq"], opt_b.state[pb[n]]["exp_avg_sq"])):
            compared += 1
            if not torch.equal(ta, tb):
                bad.append((k, n, what, float((ta - tb).abs().max())))
torch.cuda.synchronize()
opt_a._usage(red)
res["steps_a"] = [opt_a.state[pa[n]]["step"] for n in names]
res["steps_b"] = [opt_b.state[pb[n]]["step"] for n in names]
res.update(bad=bad[:20], n_bad=len(bad), norms=norms, clip=CLIP, served=served, compared=compared,
           inplace_share=red.inplace_floats / (red.inplace_floats + red.copied_floats))
print("RESULT " + json.dumps(res))
dist.destroy_process_group()
"""


@pytest.mark.parametrize("native", ["1", "0"])
def test_optimiser_trajectory_with_flipping_parameters(native):
    """Chain + auxiliary head, seven steps in which b and the head flip between used and unused (used -> unused, unused ->
    used, unused in the first step, used every other step): clip norm, parameters and both moments equal, bit for bit, to the
    same net without a reducer, through the native RCCL lanes and through ProcessGroupNCCL."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["LOTUS_DP_NATIVE"] = native
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % root + _TRAJECTORY_SCRIPT], capture_output=True, text=True, timeout=180,
                       env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["forced"] and res["native"] == (native == "1"), res
    # a condition of the test: the clip coefficient is below 1 in every step, so a norm that left a gradient out would show
    assert len(res["norms"]) == 7 and min(res["norms"]) > res["clip"], res["norms"]
    assert res["n_bad"] == 0, res["bad"]
    assert res["steps_a"] == res["steps_b"], res
    assert res["served"][0] == 0 and min(res["served"][1:]) >= 1, res["served"]
    ledger.record(f"reducer_arena_trajectory[native={native}]", compared=res["compared"], served=res["served"],
                  inplace_share=res["inplace_share"])
