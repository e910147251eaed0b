"""What the weight-gradient stream reads must stay allocated until the join that orders the critical stream behind it.

Every autograd node of ops.py, per launch (composites off) and two of them as composites, and three whole models: one
forward + backward with the side stream OFF (one stream, nothing to race: the reference) against the same with the side
stream on and STALLED (tests/side_stall.py) so that the critical stream finishes each node — and recycles whatever the
caching allocator was given back — before the first weight-gradient kernel of that node runs.  Both join modes.  The stream
modes are bit-identical (test_full_size_stream_modes_bit_identical), so the bar is torch.equal on the
output, every input gradient, every parameter gradient and a handed-over dz; the one exception is the composite FFN at the
fused LayerNorm-backward shape (M >= 16384, C <= 128), compared to 3e-6 as tests/test_gpu_blocks.py does there.

The nodes are driven as in tests/test_gpu_blocks.py: same scene, same parameter recipes."""
import pytest
import torch

import side_stall

pytestmark = pytest.mark.gpu

JOINS = ["node", "end"]


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops

    return ops


_LEVELS = {}


def _levels(dup):
    """The scene of tests/test_gpu_blocks.py (built once per process: the tables are read-only)."""
    if dup not in _LEVELS:
        from robot_3dlotus_amd import synth
        from robot_3dlotus_amd.frontend import FrontEnd

        batch = synth.synth_batch(3, 1500, ragged=True, seed=11)
        if dup:
            batch = synth.augment_clouds(batch, seed=12)
        lv = FrontEnd(2).build(batch["pc_fts"].cuda(), batch["npoints_in_batch"], batch["txt_lens"], [[0, 1, 2, 3]] * 2)
        _LEVELS[dup] = (batch, lv)
    return _LEVELS[dup]


def _params(g, shapes):
    return [None if s is None else
            (torch.randn(*s, generator=g) * (0.1 if len(s) == 1 else 1.0 / s[-1] ** 0.5)).cuda().requires_grad_(True) for s in shapes]


def _outs(y, inputs, extra=()):
    torch.cuda.synchronize()
    return [y.detach().clone()] + [t.grad.clone() for t in inputs if t is not None and t.grad is not None] + [e.clone() for e in extra]


def _check(run, join, composite, names=None, rel=None):
    ops = _ops()
    try:
        ops.set_composites(composite)
        ref, got, st = side_stall.run_modes(run, join)
    finally:
        ops.set_composites(True)
    print(f"stalled nodes {st.nodes}, stall {st.ms:.2f} ms")
    side_stall.assert_same(ref, got, names, rel)
    return st


# ------------------------------------------------------------------------------------------------ FfnFn
FFN_NAMES = ["y", "dx", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2", "dz_out"]


def _ffn_run(M, C, hand, dpath=0.0, bf16=False):
    ops = _ops()

    def run(backward):
        g = torch.Generator().manual_seed(M + C)
        x = torch.randn(M, C, generator=g).cuda()
        ps = [t.cuda().requires_grad_(True) for t in (1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g),
                                                      torch.randn(4 * C, C, generator=g) / C ** 0.5, 0.1 * torch.randn(4 * C, generator=g),
                                                      torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5, 0.1 * torch.randn(C, generator=g))]
        dy = torch.randn(M, C, generator=g).cuda()
        if bf16:
            x, dy = x.bfloat16(), dy.bfloat16()
        x.requires_grad_(True)
        h_in = ops.Handoff() if hand == "inout" else None
        h_out = ops.Handoff() if hand in ("out", "inout") else None
        if h_out is not None:
            h_out.arm(0.1, 777)          # the previous sub-block wants dx pre-masked with (0.1, 777)
        with ops.storage(torch.bfloat16 if bf16 else None):
            y = ops.FfnFn.apply(x, *ps, 0.1, 12345, h_in, h_out, dpath)
            if h_in is not None:
                # the next sub-block's LayerNorm backward: it leaves dy pre-masked with the mask this node armed
                assert h_in.drop is not None
                h_in.ptr, h_in.dz = dy.data_ptr(), ops.dropout(dy, *h_in.drop)
        backward(lambda: y.backward(dy))
        if h_in is not None:
            assert h_in.dz is None, "the hand-over was not taken"
        return _outs(y, [x] + ps, [h_out.dz] if h_out is not None else [])

    return run


@pytest.mark.parametrize("M,C", [(361, 768), (1450, 512), (6077, 256), (65536, 64)])
@pytest.mark.parametrize("hand", ["none", "out", "inout"])
@pytest.mark.parametrize("join", JOINS)
def test_ffn_per_launch(M, C, hand, join):
    _check(_ffn_run(M, C, hand), join, False, FFN_NAMES)


@pytest.mark.parametrize("join", JOINS)
def test_ffn_per_launch_drop_path(join):
    """DropPath on the branch: the situation of the shipped YAML (drop_path 0.1), a per-launch FfnFn that hands over."""
    _check(_ffn_run(1450, 512, "out", dpath=0.1), join, False, FFN_NAMES)


@pytest.mark.parametrize("join", JOINS)
def test_ffn_per_launch_bf16_storage(join):
    _check(_ffn_run(1450, 512, "out", bf16=True), join, False, FFN_NAMES)


@pytest.mark.parametrize("M,C", [(1450, 512), (65536, 64)])
@pytest.mark.parametrize("join", JOINS)
def test_ffn_composite(M, C, join):
    """The composite keeps what the side stream reads in `tmp`, a local of backward(): nothing is allocated between its
    release and the node's join."""
    fused_ln = M >= 16384 and C <= 128   # LayerNorm backward as the epilogue of the fc1 input gradient: tests/test_gpu_blocks.py
    _check(_ffn_run(M, C, "inout"), join, True, FFN_NAMES, rel=3e-6 if fused_ln else None)


# ------------------------------------------------------------------------------------------------ SelfAttnFn
@pytest.mark.parametrize("C,H", [(64, 2), (128, 4)])
@pytest.mark.parametrize("qk_norm", [True, False])
@pytest.mark.parametrize("join", JOINS)
def test_selfattn_per_launch(C, H, qk_norm, join):
    ops = _ops()
    _, lv = _levels(False)
    lvl, d = lv[0], C // H
    names = ["y", "dx", "dgamma", "dbeta", "dwqkv", "dbqkv"] + (["dqn_w", "dqn_b", "dkn_w", "dkn_b"] if qk_norm else []) + ["dwp", "dbp"]

    def run(backward):
        g = torch.Generator().manual_seed(C)
        x = torch.randn(lvl.n, C, generator=g).cuda().requires_grad_(True)
        qk = [(d,)] * 4 if qk_norm else [None] * 4
        ps = _params(g, [(C,), (C,), (3 * C, C), (3 * C,)] + qk + [(C, C), (C,)])
        dy = torch.randn(lvl.n, C, generator=g).cuda()
        hand = ops.Handoff()
        y = ops.SelfAttnFn.apply(x, *ps, lvl, H, 0.1, 4242, 0.1, hand)
        backward(lambda: y.backward(dy))
        return _outs(y, [x] + ps)

    _check(run, join, False, names)


# ------------------------------------------------------------------------------------------------ CrossAttnFn / CrossAttnKvFn
def _ca_levels(batch_lv):
    """Level 0, and a level whose cross-attention key side is split into groups (ca_groups > 1) if the scene gives one."""
    _, lv = batch_lv
    out = [lv[0]]
    if lv[0].ca_groups == 1:
        out += [l for l in lv[1:] if l.ca_groups > 1][:1]
    return out


@pytest.mark.parametrize("C,H", [(64, 2), (256, 8)])
@pytest.mark.parametrize("join", JOINS)
def test_crossattn_per_launch(C, H, join):
    ops = _ops()
    batch, lv = _levels(False)
    d, Cc = C // H, 256
    L = sum(batch["txt_lens"])
    names = ["y", "dx", "dcontext", "dgamma", "dbeta", "dwq", "dbq", "dwkv", "dbkv", "dqn_w", "dqn_b", "dkn_w", "dkn_b", "dwp", "dbp",
             "dz_out"]
    for lvl in _ca_levels((batch, lv)):
        def run(backward):
            g = torch.Generator().manual_seed(C + 1)
            x = torch.randn(lvl.n, C, generator=g).cuda().requires_grad_(True)
            ctxt = torch.randn(L, Cc, generator=g).cuda().requires_grad_(True)
            ps = _params(g, [(C,), (C,), (C, C), (C,), (2 * C, Cc), (2 * C,), (d,), (d,), (d,), (d,), (C, C), (C,)])
            dy = torch.randn(lvl.n, C, generator=g).cuda()
            h_in, h_out = ops.Handoff(), ops.Handoff()
            h_out.arm(0.1, 99)
            y = ops.CrossAttnFn.apply(x, ctxt, *ps, lvl, H, 0.1, 777, 0.1, h_in, h_out)
            backward(lambda: y.backward(dy))
            return _outs(y, [x, ctxt] + ps, [h_out.dz])

        _check(run, join, False, names)


@pytest.mark.parametrize("C,H", [(64, 2), (256, 8)])
@pytest.mark.parametrize("join", JOINS)
def test_crossattn_kv_per_launch(C, H, join):
    """kv from a ProjBank of three slices (tests/test_gpu_round4.py): the backward pass is CrossAttnKvFn, then ProjAllFn."""
    ops = _ops()
    batch, lv = _levels(False)
    d, Cc = C // H, 256
    L = sum(batch["txt_lens"])
    widths = [2 * 128, 2 * C, 2 * 64]   # the middle slice belongs to the block under test
    for lvl in _ca_levels((batch, lv)):
        def run(backward):
            g = torch.Generator().manual_seed(C + 1)
            x = torch.randn(lvl.n, C, generator=g).cuda().requires_grad_(True)
            ctxt = torch.randn(L, Cc, generator=g).cuda().requires_grad_(True)
            ps = _params(g, [(C,), (C,), (C, C), (C,), (d,), (d,), (d,), (d,), (C, C), (C,)])
            kvw = _params(g, [s for w in widths for s in ((w, Cc), (w,))])
            dy = torch.randn(lvl.n, C, generator=g).cuda()
            bank = ops.ProjBank()
            sl = ops.ProjAllFn.apply(ctxt, bank, None, *kvw)
            h_in, h_out = ops.Handoff(), ops.Handoff()
            h_out.arm(0.1, 99)
            y = ops.CrossAttnKvFn.apply(x, sl[1], *ps, lvl, H, 0.1, 777, 0.1, h_in, h_out, bank, 1)
            # the other two slices get a gradient too (as the other blocks' backward passes would write them)
            loss = (y * dy).sum() + (sl[0] * 0.5).sum() + (sl[2] * -0.25).sum()
            backward(loss.backward)
            return _outs(y, [x, ctxt] + ps + kvw, [h_out.dz])

        st = _check(run, join, False)
        assert join == "end" or st.nodes == 2, st.nodes   # CrossAttnKvFn and ProjAllFn


# ------------------------------------------------------------------------------------------------ CpeFn
CPE_NAMES = ["y", "dx", "dxs", "dcw", "dcb", "dlw", "dlb", "dgamma", "dbeta"]


def _cpe_run(C, same, dup):
    ops = _ops()
    _, lv = _levels(dup)
    lvl = lv[0]
    assert (lvl.n_dup > 0) == dup

    def run(backward):
        g = torch.Generator().manual_seed(C + 2)
        x = torch.randn(lvl.n, C, generator=g).cuda().requires_grad_(True)
        xs = x if same else torch.randn(lvl.n, C, generator=g).cuda().requires_grad_(True)
        cw = (torch.randn(C, 3, 3, 3, C, generator=g) / (C * 9) ** 0.5).cuda().requires_grad_(True)
        ps = _params(g, [(C,), (C, C), (C,), (C,), (C,)])
        dy = torch.randn(lvl.n, C, generator=g).cuda()
        wt = ops.conv_weight_t(cw.detach())
        y = ops.CpeFn.apply(x, xs, cw, *ps, lvl, wt)
        backward(lambda: y.backward(dy))
        return _outs(y, [x] + ([] if same else [xs]) + [cw] + ps)

    return run, [n for n in CPE_NAMES if not (same and n == "dxs")]


@pytest.mark.parametrize("C,same", [(64, True), (128, False)])
@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("join", JOINS)
def test_cpe_per_launch(C, same, dup, join):
    run, names = _cpe_run(C, same, dup)
    _check(run, join, False, names)


@pytest.mark.parametrize("join", JOINS)
def test_cpe_composite(join):
    run, names = _cpe_run(64, True, False)
    _check(run, join, True, names)


# ------------------------------------------------------------------------------------------------ nodes that keep their operands as locals
# PoolFn, UnpoolFn, StemFn and LinearFn hold what the side stream reads in locals of backward() itself, released when it
# returns, right in front of the join: green before and after the hold.  Pinned here, at level 0 -> 1 of the scene.
def _bn(C):
    return torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")


@pytest.mark.parametrize("join", JOINS)
def test_pool_per_launch(join):
    ops = _ops()
    _, lv = _levels(False)
    lvl, child, Ci, C = lv[0], lv[1], 64, 128

    def run(backward):
        g = torch.Generator().manual_seed(7)
        x = torch.randn(lvl.n, Ci, generator=g).cuda().requires_grad_(True)
        ps = _params(g, [(C, Ci), (C,), (C,), (C,)])
        dy = torch.randn(child.n, C, generator=g).cuda()
        y = ops.PoolFn.apply(x, *ps, *_bn(C), child, True)
        backward(lambda: y.backward(dy))
        return _outs(y, [x] + ps)

    _check(run, join, False, ["y", "dx", "dw", "dbias", "dgamma", "dbeta"])


@pytest.mark.parametrize("join", JOINS)
def test_unpool_per_launch(join):
    ops = _ops()
    _, lv = _levels(False)
    lvl, child, Cc, Cp, C = lv[0], lv[1], 128, 64, 64

    def run(backward):
        g = torch.Generator().manual_seed(8)
        xc = torch.randn(child.n, Cc, generator=g).cuda().requires_grad_(True)
        xp = torch.randn(lvl.n, Cp, generator=g).cuda().requires_grad_(True)
        pu = _params(g, [(C, Cc), (C,), (C,), (C,)])
        pk = _params(g, [(C, Cp), (C,), (C,), (C,)])
        dx, dskip = torch.randn(lvl.n, C, generator=g).cuda(), torch.randn(lvl.n, C, generator=g).cuda()
        y, skip = ops.UnpoolFn.apply(xc, xp, *pu, *_bn(C), *pk, *_bn(C), child, True)
        backward(lambda: torch.autograd.backward([y, skip], [dx, dskip]))
        return _outs(y, [xc, xp] + pu + pk, [skip.detach()])

    _check(run, join, False)


@pytest.mark.parametrize("join", JOINS)
def test_stem_per_launch(join):
    """With an input gradient wanted (the motion planner's learned label embedding) the stem's weight gradient forks too."""
    ops = _ops()
    _, lv = _levels(False)
    lvl, Ci, C = lv[0], 6, 64

    def run(backward):
        g = torch.Generator().manual_seed(9)
        x = torch.randn(lvl.n, Ci, generator=g).cuda().requires_grad_(True)
        cw = (torch.randn(C, 5, 5, 5, Ci, generator=g) / 30).cuda().requires_grad_(True)
        ps = _params(g, [(C,), (C,)])
        dy = torch.randn(lvl.n, C, generator=g).cuda()
        y = ops.StemFn.apply(x, cw, *ps, *_bn(C), lvl, True)
        backward(lambda: y.backward(dy))
        return _outs(y, [x, cw] + ps)

    _check(run, join, False, ["y", "dx", "dcw", "dgamma", "dbeta"])


@pytest.mark.parametrize("join", JOINS)
def test_linear_per_launch(join):
    ops = _ops()
    _, lv = _levels(False)
    M, K, N = lv[0].n, 64, 128

    def run(backward):
        g = torch.Generator().manual_seed(10)
        x = torch.randn(M, K, generator=g).cuda().requires_grad_(True)
        ps = _params(g, [(N, K), (N,)])
        dy = torch.randn(M, N, generator=g).cuda()
        y = ops.LinearFn.apply(x, *ps)
        backward(lambda: y.backward(dy))
        return _outs(y, [x] + ps)

    _check(run, join, False, ["y", "dx", "dw", "db"])


# ------------------------------------------------------------------------------------------------ whole models
def _dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if k == "disc_pos_probs" else v))
            for k, v in batch.items()}


def _model_run(make, batch, perms):
    """One train-mode forward + backward of a fresh model, dropout on; the step seed comes from torch's seed and the step
    counter in the state dict, so every run draws the same masks (test_drop_path_rows_and_backward relies on the same)."""
    def run(backward):
        torch.manual_seed(5)
        m = make().cuda().train()
        m.ptv3_model.order_perms = perms
        _, losses = m(batch, compute_loss=True, compute_final_action=False)
        backward(losses["total"].backward)
        torch.cuda.synchronize()
        named = list(m.named_parameters())
        assert all(p.grad is not None for _, p in named)
        run.names = ["loss_" + k for k in sorted(losses)] + [n for n, _ in named]
        return [losses[k].detach().clone() for k in sorted(losses)] + [p.grad.clone() for _, p in named]

    return run


def _model_check(run, join):
    ref, got, st = side_stall.run_modes(run, join)
    print(f"stalled nodes {st.nodes}, stall {st.ms:.2f} ms")
    side_stall.assert_same(ref, got, run.names)
    return st


def test_model_ca_tiny_drop_path():
    """The shipped-YAML situation: drop_path 0.1 makes every FfnFn of a Block a per-launch node that receives a hand-over."""
    import golden_util as gu
    from robot_3dlotus_amd import config as lcfg, synth
    from robot_3dlotus_amd.policy import SimplePolicyPTV3CA
    from weights_util import seeded_state_dict

    cfg = lcfg.preset("tiny")
    cfg.ptv3_config.drop_path = 0.1
    sd = seeded_state_dict(gu.state_template(cfg), 5, "scaled")
    batch = _dev(synth.synth_batch(2, 512, ragged=True, seed=42))

    def make():
        m = SimplePolicyPTV3CA(cfg)
        m.load_state_dict(sd)
        return m

    st = _model_check(_model_run(make, batch, [[2, 0, 1, 3], [1, 3, 0, 2]]), "node")
    assert st.nodes > 1, st.nodes


def _adanorm_run():
    import adanorm_util as au
    from robot_3dlotus_amd.policy import SimplePolicyPTV3AdaNorm
    from weights_util import seeded_state_dict

    case = "adanorm_tiny_scaled_train"
    cfg = au.case_config(case)
    batch = _dev(au.case_batch(case))
    sd = seeded_state_dict(SimplePolicyPTV3AdaNorm(cfg).state_dict(), au.CASES[case][7], "scaled")

    def make():
        m = SimplePolicyPTV3AdaNorm(cfg)
        m.load_state_dict(sd)
        return m

    return _model_run(make, batch, [[2, 0, 1, 3], [1, 3, 0, 2]])


def test_model_adanorm_tiny_node_join():
    """Every AdaNorm model trains through the per-launch bodies."""
    st = _model_check(_adanorm_run(), "node")
    assert st.nodes > 1, st.nodes


def test_model_adanorm_tiny_end_join():
    """One stall at the first fork of the backward pass, the join at its end."""
    st = _model_check(_adanorm_run(), "end")
    assert st.nodes == 1, st.nodes
