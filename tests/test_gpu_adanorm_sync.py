"""SimplePolicyPTV3AdaNorm data parallel: the split (statistics -> message -> apply) adaptive BatchNorm passes of
csrc/adanorm.hip against float64 torch, two ranks on one device through parallel.GradReducer + SyncBatchNorm statistics, the
full-size model once, and the one-rank RCCL rehearsal tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from test_gpu_adanorm import COUNTS, _Lvl, _mods, _ref_mod  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 3e-5        # test_adabn_kernels_against_float64: relative to max(1, |ref|max)
TOL_RUNNING = 1e-5


# ------------------------------------------------------------------------------------ split halves vs float64
def _cuts(counts):
    """Cloud lists of the two "ranks": prefix / suffix at the middle, and the 1-cloud / rest cut.  A single cloud cannot be cut:
    its partner is an EMPTY shard (one cloud of no rows), which sends a zero message and still has to finish the statistics."""
    B = len(counts)
    if B == 1:
        return [(list(counts), [0])]
    return [(list(counts[:k]), list(counts[k:])) for k in sorted({B // 2, 1})]


def _inputs(C, counts, seed):
    M, B = sum(counts), len(counts)
    torch.manual_seed(seed)
    x = (torch.randn(M, C) * 1.5 + 0.3).cuda()
    g, b = (1 + 0.2 * torch.randn(C)).cuda(), (0.2 * torch.randn(C)).cuda()
    rm0, rv0 = (0.1 * torch.randn(C)).cuda(), (0.5 + torch.rand(C)).cuda()
    slab, mod = _mods(B, C, 2 * C + 20, C + 1)
    dy = torch.randn(M, C).cuda()
    return x, g, b, rm0, rv0, slab, mod, dy


def _reference(x, g, b, rm0, rv0, mod, dy, counts):
    C = x.shape[1]
    xd = x.double().requires_grad_()
    gd, bd = g.double().requires_grad_(), b.double().requires_grad_()
    md = mod.double().requires_grad_()
    sh, sc, _ = _ref_mod(counts, md)
    rmd, rvd = rm0.double().clone(), rv0.double().clone()
    n = torch.nn.functional.batch_norm(xd, rmd, rvd, gd, bd, True, 0.01, 1e-3)
    yr = torch.nn.functional.gelu(n * (1 + sc) + sh)
    yr.backward(dy.double())
    return {"y": yr.detach(), "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad, "dmod": md.grad, "running_mean": rmd,
            "running_var": rvd}


def _errors(got, ref):
    """name -> (error, bar): max |got - ref| relative to max(1, |ref|max); the running statistics absolute."""
    out = {}
    for k, r in ref.items():
        e = (got[k].double() - r).abs().max().item() if r.numel() else 0.0
        if k.startswith("running"):
            out[k] = (e, TOL_RUNNING)
        else:
            out[k] = (e / max(1.0, r.abs().max().item() if r.numel() else 0.0), TOL)
    return out


def _fused(x, g, b, rm0, rv0, slab, mod, dy, counts):
    """The un-split kernels (one process, no statistics hook) on the same input: the error to read the split route's next to."""
    from robot_3dlotus_amd import adanorm as an, ops

    assert ops.BnState.reduce is None
    lvl = _Lvl(counts)
    C = x.shape[1]
    rm, rv = rm0.clone(), rv0.clone()
    dslab = torch.full_like(slab, 7.0)
    dmod = dslab[:, 12:12 + 2 * C]
    y, mean, invstd = an.adabn_fwd(x, g, b, rm, rv, mod, lvl, True)
    dx, dg, db = an.adabn_bwd(dy, x, mean, invstd, g, b, mod, dmod, lvl, True)
    return {"y": y, "dx": dx, "dgamma": dg, "dbeta": db, "dmod": dmod.clone(), "running_mean": rm, "running_var": rv}


def _split_two_parts(x, g, b, rm0, rv0, slab, mod, dy, parts):
    """Statistics on each part, the two fp64 messages added with torch (the all-reduce), the apply halves on each part."""
    from robot_3dlotus_amd import adanorm as an, ops
    from robot_3dlotus_amd.ops import ACT_GELU

    C = x.shape[1]
    dslab = torch.full_like(slab, 7.0)
    dmod_all = dslab[:, 12:12 + 2 * C]
    rows = np.concatenate([[0], np.cumsum([sum(p) for p in parts])])
    clouds = np.concatenate([[0], np.cumsum([len(p) if sum(p) else 0 for p in parts])])
    P = []
    for r, counts in enumerate(parts):
        empty = sum(counts) == 0
        xs, dys = x[rows[r]:rows[r + 1]], dy[rows[r]:rows[r + 1]]
        if empty:   # the empty shard: a modulation row of its own (never read), no row of the d mod slab
            md, dm = torch.zeros(1, 2 * C, device="cuda"), torch.full((1, 2 * C), 7.0, device="cuda")
        else:
            md, dm = mod[clouds[r]:clouds[r + 1]], dmod_all[clouds[r]:clouds[r + 1]]
        P.append(dict(x=xs, dy=dys, mod=md, dmod=dm, lvl=_Lvl(counts), rm=rm0.clone(), rv=rv0.clone(), empty=empty))
    # forward: local sums -> sum of the messages -> apply
    for p in P:
        p["fs"] = torch.zeros(2 * C + 1, dtype=torch.float64, device="cuda")   # (a rank without rows sends zeros)
        if not p["empty"]:
            ops._bn_stats(p["x"], p["fs"])
    total = sum(p["fs"] for p in P)
    assert total[2 * C].item() == x.shape[0]
    for p in P:
        p["y"], p["mean"], p["invstd"] = an._adabn_apply_sums(p["x"], total.clone(), g, b, p["rm"], p["rv"], p["mod"], p["lvl"], ACT_GELU)
    # backward: partials + fixed-order reduce (d gamma, d beta, d mod, local message) -> sum of the messages -> apply
    for p in P:
        p["bs"] = torch.zeros(2 * C + 1, dtype=torch.float64, device="cuda")
        if p["empty"]:
            p["dg"] = p["db"] = torch.zeros(C, device="cuda")
        else:
            p["dg"], p["db"] = an._adabn_bwd_stats(p["dy"], p["x"], p["mean"], p["invstd"], g, b, p["mod"], p["dmod"], p["lvl"], ACT_GELU,
                                                   p["bs"])
            # the message is (gamma d beta, gamma d gamma, rows) of the local rows: its fp64 sums over the clouds against the fp32
            # d beta / d gamma of the same launch, which are themselves held to TOL
            assert p["bs"][2 * C].item() == p["x"].shape[0]
            for lo, v in ((0, p["db"]), (C, p["dg"])):
                want = g.double() * v.double()
                assert (p["bs"][lo:lo + C] - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())
    btotal = sum(p["bs"] for p in P)
    for p in P:
        p["dx"] = an._adabn_bwd_apply_sums(p["dy"], p["x"], p["mean"], p["invstd"], g, b, p["mod"], p["lvl"], ACT_GELU, btotal.clone())
    torch.cuda.synchronize()
    # every "rank" ends with the same statistics
    for k in ("mean", "invstd", "rm", "rv"):
        assert torch.equal(P[0][k], P[1][k]), k
    return {"y": torch.cat([p["y"] for p in P]), "dx": torch.cat([p["dx"] for p in P]), "dgamma": P[0]["dg"] + P[1]["dg"],
            "dbeta": P[0]["db"] + P[1]["db"], "dmod": dmod_all.clone(), "running_mean": P[0]["rm"], "running_var": P[0]["rv"]}, dslab


@pytest.mark.parametrize("C", [64, 128, 256, 512, 768])
@pytest.mark.parametrize("layout", list(COUNTS))
def test_split_halves_against_float64(C, layout):
    """Two "ranks" in one process.  Every figure is printed with the un-split fp32 kernels' error on the same input next to it."""
    counts = COUNTS[layout]
    for parts in _cuts(counts):
        x, g, b, rm0, rv0, slab, mod, dy = _inputs(C, counts, C + sum(counts) + len(parts[0]))
        ref = _reference(x, g, b, rm0, rv0, mod, dy, counts)
        got, dslab = _split_two_parts(x, g, b, rm0, rv0, slab, mod, dy, parts)
        again, dslab2 = _split_two_parts(x, g, b, rm0, rv0, slab, mod, dy, parts)
        err = _errors(got, ref)
        base = _errors(_fused(x, g, b, rm0, rv0, slab, mod, dy, counts), ref)
        report = {k: f"split {err[k][0]:.2e} fused {base[k][0]:.2e} bar {err[k][1]:.0e}" for k in err}
        print(f"C={C} {layout} cut={len(parts[0])}|{len(parts[1])}: {report}")
        assert (dslab[:, :12] == 7.0).all() and (dslab[:, 12 + 2 * C:] == 7.0).all()   # nothing outside the norm's slice is written
        for k in got:
            assert torch.equal(got[k], again[k]), ("second run differs", k)
        assert torch.equal(dslab, dslab2)
        bad = {k: report[k] for k in err if not err[k][0] < err[k][1]}
        assert not bad, (C, layout, parts, bad)


@pytest.mark.parametrize("C", [64, 128, 256, 512, 768])
@pytest.mark.parametrize("layout", list(COUNTS))
def test_split_route_with_an_identity_reduce_meets_the_fused_bars(C, layout, monkeypatch):
    """adabn_fwd / adabn_bwd with a statistics hook that changes nothing (one part): the split route on the public path."""
    from robot_3dlotus_amd import adanorm as an, ops

    counts = COUNTS[layout]
    x, g, b, rm0, rv0, slab, mod, dy = _inputs(C, counts, C + sum(counts))
    ref = _reference(x, g, b, rm0, rv0, mod, dy, counts)
    base = _errors(_fused(x, g, b, rm0, rv0, slab, mod, dy, counts), ref)
    sent = []
    monkeypatch.setattr(ops.BnState, "reduce", lambda sums: sent.append(tuple(sums.shape)))
    lvl = _Lvl(counts)

    def run(training=True):
        rm, rv = rm0.clone(), rv0.clone()
        dslab = torch.full_like(slab, 7.0)
        dmod = dslab[:, 12:12 + 2 * C]
        y, mean, invstd = an.adabn_fwd(x, g, b, rm, rv, mod, lvl, training)
        dx, dg, db = an.adabn_bwd(dy, x, mean, invstd, g, b, mod, dmod, lvl, training)
        return {"y": y, "dx": dx, "dgamma": dg, "dbeta": db, "dmod": dmod.clone(), "running_mean": rm, "running_var": rv}, dslab

    got, dslab = run()
    assert sent == [(2 * C + 1,)] * 2                      # one message per direction
    again, _ = run()
    err = _errors(got, ref)
    report = {k: f"split {err[k][0]:.2e} fused {base[k][0]:.2e} bar {err[k][1]:.0e}" for k in err}
    print(f"C={C} {layout} identity reduce: {report}")
    assert (dslab[:, :12] == 7.0).all() and (dslab[:, 12 + 2 * C:] == 7.0).all()
    assert all(torch.equal(got[k], again[k]) for k in got)
    bad = {k: report[k] for k in err if not err[k][0] < err[k][1]}
    assert not bad, (C, layout, bad)
    # eval mode sends nothing and is today's path bit for bit
    del sent[:]
    ev, _ = run(training=False)
    assert sent == []
    monkeypatch.setattr(ops.BnState, "reduce", None)
    ev0, _ = run(training=False)
    assert all(torch.equal(ev[k], ev0[k]) for k in ev)


# ------------------------------------------------------------------------------------ two ranks on one device
WORKER_LIMIT_S = 420


def _worker(rank, world, port, q, mode, trace_dir):
    try:
        import faulthandler
        _fh = open(os.path.join(trace_dir, f"adanorm_sync_{mode}_worker_{rank}.trace"), "w")
        faulthandler.dump_traceback_later(WORKER_LIMIT_S - 30, file=_fh, exit=False)   # where is a stuck worker? (diagnostic)
        (_worker_tiny if mode == "tiny" else _worker_full)(rank, world, port, q)
        faulthandler.cancel_dump_traceback_later()
    except BaseException as e:  # report instead of leaving the parent to time out
        import traceback
        q.put((rank, {"error": f"{type(e).__name__}: {e}\n{traceback.format_exc()}"}))
        raise


def _setup(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", LOTUS_DIST_BACKEND="gloo")
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import parallel

    parallel.init_distributed()


def _dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in b.items()}


def _worker_tiny(rank, world, port, q):
    _setup(rank, world, port)
    import adanorm_util as au
    from robot_3dlotus_amd import config as lcfg, ops, parallel, synth
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm
    from weights_util import seeded_state_dict

    cfg = lcfg.preset("adanorm_tiny")
    sd = seeded_state_dict(SimplePolicyPTV3AdaNorm(cfg).state_dict(), 3, "scaled")
    perms = [[1, 0, 3, 2], [2, 3, 0, 1]]
    S = 2

    def build(convert=False, local=False):
        m = SimplePolicyPTV3AdaNorm(cfg)
        m.load_state_dict(sd)
        if convert:
            m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
        m = m.cuda().train()
        if local:   # the one-process side of a comparison, inside a two-rank group: rank-local statistics are what is wanted here
            m.ptv3_model._sync_bn_checked = True
        assert m.ptv3_model.num_stages == S
        m.ptv3_model.proj_drop = m.ptv3_model.attn_drop = 0.0
        m.act_proj_head.dropout = 0.0
        m.ptv3_model.order_perms = perms
        return m

    def batch(B, n, seed):
        return au.last_token_batch(synth.synth_batch(B, n, ragged=True, seed=seed))

    def run(m, b, red, scale=1.0):
        if red is not None:
            red.zero_grad()
        else:
            m.zero_grad(set_to_none=True)
        _, losses = m(_dev(b), compute_loss=True, compute_final_action=False)
        (losses["total"] * scale).backward()
        if red is not None:
            red.finish()
        torch.cuda.synchronize()
        assert all(p.grad is not None for p in m.parameters())
        return torch.cat([p.grad.flatten() for p in m.parameters()]).clone()

    res = {}
    # (a) replicated shard: reducer-averaged gradients == one process on that shard; (d) message counts
    shard = batch(2, 400, 50)
    m = build()
    red = parallel.GradReducer(m, bucket_mb=0.5)
    parallel.enable_sync_batchnorm()
    n0 = parallel.BN_MESSAGES
    g_dp = run(m, shard, red)
    res["messages_per_train_step"] = parallel.BN_MESSAGES - n0
    res["messages_expected"] = 2 * (1 + 2 * (S - 1))
    rs_dp = m.ptv3_model.embedding.stem.norm.norm.running_var.clone()
    g_dp2 = run(m, shard, red)   # from the second backward on the nodes write their gradients into the bucket buffer
    g_dp3 = run(m, shard, red)
    res["messages_three_steps"] = parallel.BN_MESSAGES - n0
    res["arena_inplace_fraction"] = red.inplace_floats / max(1, red.inplace_floats + red.copied_floats)
    res["arena_steps_equal"] = bool(torch.equal(g_dp2, g_dp3)) and ((g_dp3 - g_dp).norm() / g_dp.norm()).item() < 1e-6
    n1 = parallel.BN_MESSAGES
    m.eval()
    with torch.no_grad():
        m(_dev(shard), compute_loss=False)
    torch.cuda.synchronize()
    res["messages_eval"] = parallel.BN_MESSAGES - n1
    ops.BnState.reduce = None
    m1 = build(local=True)
    g_1 = run(m1, shard, None)
    res["replicated_rel_err"] = ((g_dp - g_1).norm() / g_1.norm()).item()
    res["replicated_rv_err"] = (rs_dp - m1.ptv3_model.embedding.stem.norm.norm.running_var).abs().max().item()
    # (e) converted containers, no explicit enable_sync_batchnorm(): the first forward switches the statistics on
    assert ops.BnState.reduce is None
    mc = build(convert=True)
    redc = parallel.GradReducer(mc, bucket_mb=0.5)
    n2 = parallel.BN_MESSAGES
    g_c = run(mc, shard, redc)
    res["converted_hook_installed"] = ops.BnState.reduce is not None
    res["converted_messages"] = parallel.BN_MESSAGES - n2
    res["converted_rel_err"] = ((g_c - g_1).norm() / g_1.norm()).item()
    res["converted_equals_explicit"] = bool(torch.equal(g_c, g_dp))
    # (b) different shards: identical gradients and running statistics on both ranks
    parallel.enable_sync_batchnorm()
    m2 = build()
    red2 = parallel.GradReducer(m2, bucket_mb=0.5)
    g_r = run(m2, batch(2, 400, 60 + rank), red2)
    buf = [torch.zeros_like(g_r) for _ in range(world)]
    dist.all_gather(buf, g_r)
    res["cross_rank_diff"] = (buf[0] - buf[1]).abs().max().item()
    rv = torch.cat([m2.ptv3_model.enc.enc1.down.norm[0].norm.running_var, m2.ptv3_model.embedding.stem.norm.norm.running_mean,
                    m2.ptv3_model.dec.dec0.up.proj[1].norm.running_var, m2.ptv3_model.dec.dec0.up.proj_skip[1].norm.running_mean])
    rvs = [torch.zeros_like(rv) for _ in range(world)]
    dist.all_gather(rvs, rv)
    res["cross_rank_rv_diff"] = (rvs[0] - rvs[1]).abs().max().item()
    res["finite"] = bool(torch.isfinite(g_r).all()) and bool(torch.isfinite(rv).all())
    # (c) UNEQUAL shards of one batch (3 clouds / 1 cloud, common bounding box) against one process on the whole batch
    full = synth.align_extents(batch(4, 500, 70))
    shards = [[0, 1, 2], [3]]
    parallel.enable_sync_batchnorm()
    m3 = build()
    red3 = parallel.GradReducer(m3, bucket_mb=0.5)
    g3 = run(m3, synth.take_clouds(full, shards[rank]), red3, scale=parallel.shard_loss_scale(len(shards[rank]), 4, world))
    rv3 = m3.ptv3_model.enc.enc1.down.norm[0].norm.running_var.clone()
    ops.BnState.reduce = None
    m4 = build(local=True)
    g4 = run(m4, full, None)
    res["unequal_shards_rel_err"] = ((g3 - g4).norm() / g4.norm()).item()
    per, o = [], 0
    for p_ in m4.parameters():
        a, b_ = g3[o:o + p_.numel()], g4[o:o + p_.numel()]
        per.append(((a - b_).norm() / (b_.norm() + 1e-3 * g4.norm())).item())
        o += p_.numel()
    res["unequal_shards_worst_param"] = max(per)
    res["unequal_shards_rv_err"] = (rv3 - m4.ptv3_model.enc.enc1.down.norm[0].norm.running_var).abs().max().item()
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _worker_full(rank, world, port, q):
    _setup(rank, world, port)
    from robot_3dlotus_amd import config as lcfg, parallel, synth
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm

    torch.manual_seed(5)
    cfg = lcfg.preset("adanorm_v1")
    cfg.action_config.txt_reduce = "attn"              # whole instructions: txt_attn_fc is one of the reducer's parameters
    m = SimplePolicyPTV3AdaNorm(cfg).cuda().train()
    assert any(n.startswith("txt_attn_fc") for n, _ in m.named_parameters())
    red = parallel.GradReducer(m, bucket_mb=32.0)      # (broadcasts rank 0's parameters and buffers)
    parallel.enable_sync_batchnorm()
    b = synth.augment_clouds(synth.synth_batch(4, 4096, seed=10 + rank), seed=20 + rank)
    n0 = parallel.BN_MESSAGES
    red.zero_grad()
    _, losses = m(_dev(b), compute_loss=True, compute_final_action=False)
    losses["total"].backward()
    red.finish()
    torch.cuda.synchronize()
    res = {"messages": parallel.BN_MESSAGES - n0, "stages": m.ptv3_model.num_stages,
           "all_grads": all(p.grad is not None for p in m.parameters())}
    g = torch.cat([p.grad.flatten() for p in m.parameters()])
    rs = torch.cat([mod.running_var for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)])
    res["finite"] = bool(torch.isfinite(g).all()) and bool(torch.isfinite(rs).all()) and all(
        bool(torch.isfinite(v).all()) for v in losses.values())
    for name, t in (("cross_rank_diff", g), ("cross_rank_rv_diff", rs)):
        buf = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(buf, t)
        res[name] = (buf[0] - buf[1]).abs().max().item()
    res["grad_norm"] = g.norm().item()
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _run_two_ranks(port, mode, trace_dir):
    """Both workers under ONE time limit: the parent waits once, then kills what is still alive; no second attempt."""
    import queue
    import time

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q, mode, trace_dir)) for r in range(2)]
    for p in ps:
        p.start()
    out, deadline = {}, time.monotonic() + WORKER_LIMIT_S
    try:
        while len(out) < len(ps):
            r, res = q.get(timeout=max(0.1, deadline - time.monotonic()))
            out[r] = res
            if "error" in res:      # the other rank would wait in a collective for ever
                break
    except queue.Empty:
        pass
    done = len(out) == len(ps) and all("error" not in r for r in out.values())
    for p in ps:
        p.join(timeout=60 if done else 5)
        if p.is_alive():
            p.kill()
            p.join(timeout=10)
    for r, res in out.items():
        assert "error" not in res, res["error"]
    if len(out) < len(ps):
        traces = "".join(open(f).read() for f in (os.path.join(trace_dir, f"adanorm_sync_{mode}_worker_{r}.trace") for r in range(2))
                         if os.path.exists(f))
        pytest.fail(f"two-rank workers did not finish within {WORKER_LIMIT_S} s\n" + traces[-4000:])
    return out


def test_two_rank_adanorm_data_parallel_on_device(tmp_path):
    out = _run_two_ranks(33600 + (os.getpid() % 1000), "tiny", str(tmp_path))
    for r, res in sorted(out.items()):
        print(f"rank {r}: {json.dumps(res)}")
    for r, res in out.items():
        assert res["finite"], res
        # (a) replicated shard
        assert res["replicated_rel_err"] < 1e-5, res
        assert res["replicated_rv_err"] < 1e-6, res
        # (b) different shards
        assert res["cross_rank_diff"] == 0.0, res
        assert res["cross_rank_rv_diff"] == 0.0, res
        # (c) unequal shards against one process on the whole batch
        assert res["unequal_shards_rel_err"] < 1e-5 and res["unequal_shards_worst_param"] < 1e-5, res
        assert res["unequal_shards_rv_err"] < 1e-6, res
        # (d) 2 (1 + 2 (S - 1)) statistics messages per training step, none in eval
        assert res["messages_per_train_step"] == res["messages_expected"] == 6, res
        assert res["messages_three_steps"] == 18 and res["messages_eval"] == 0, res
        # (e) convert_sync_batchnorm alone gives the gradients of (a)
        assert res["converted_hook_installed"] and res["converted_messages"] == 6, res
        assert res["converted_rel_err"] < 1e-5, res
        # the modulation slab (and the other nodes' slabs) are born in the reducer's bucket buffer from the second step on
        assert res["arena_steps_equal"] and res["arena_inplace_fraction"] > 0.5, res


def test_full_size_two_ranks_one_step(tmp_path):
    """adanorm_v1 (txt_reduce 'attn'), two ranks x 4 clouds x 4096 points on one device, one training step."""
    out = _run_two_ranks(35600 + (os.getpid() % 1000), "full", str(tmp_path))
    for r, res in sorted(out.items()):
        print(f"rank {r}: {json.dumps(res)}")
    for r, res in out.items():
        assert res["stages"] == 5 and res["messages"] == 18, res
        assert res["finite"] and res["all_grads"] and res["grad_norm"] > 0, res
        assert res["cross_rank_diff"] == 0.0 and res["cross_rank_rv_diff"] == 0.0, res


def test_rehearsal_tool_runs():
    """tools/adanorm_bench.py --rehearsal: the one-rank RCCL data-parallel step next to the plain step (smoke, no threshold)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "adanorm_bench.py"), "--rehearsal", "--steps", "3", "--windows", "1",
                        "--warmup", "3"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(json.dumps(out))
    assert out["plain"] > 0 and out["rehearsal"] > 0 and out["rehearsal_over_plain"] > 0
    assert out["bn_messages_per_step"] == 18 and out["dist_backend"] == "nccl"
