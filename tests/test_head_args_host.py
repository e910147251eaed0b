"""The table of tests/head_edges.py on a machine without a device: its self-check, the input conditions of every row
(tests/head_run.py draws the inputs on the CPU), the numpy restatement of the dropout mask on its own, and the argument checks of
the entry points of csrc/pool_head.hip, which must answer LOTUS_E_ARG before any launch."""
import numpy as np
import pytest
import torch

import head_edges as he
import head_run as hr
import robot_3dlotus_amd  # noqa: F401
from robot_3dlotus_amd import _capi

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _capi.lib()


def test_the_table_holds_what_it_says():
    assert he.self_check() == len(he.ROWS) >= 70
    assert {r.group for r in he.ROWS} == set(hr._GROUP)


# ------------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("row_id", [r.id for r in he.STEP if r.group in ("step", "stepid")])
def test_step_inputs_keep_clear_of_the_kink(row_id):
    row = he.BY_ID[row_id]
    base, bias, dh = hr.step_inputs(row)
    M, C = row.shape
    assert base.shape == (M, C) and bias.shape == (3, C) and dh.shape == (3, M, C)
    if row.opts["act"] != he.ACT_NONE:
        pre = base.double()[None] + bias.double()[:, None, :]
        assert float(pre.abs().min()) >= 1e-5
    if row.opts.get("b16"):
        assert torch.equal(base, base.bfloat16().float()) and torch.equal(dh, dh.bfloat16().float())
    assert len({hr.step_seed(M, C, t) for t in range(3)}) == 3 and all(hr.step_seed(M, C, t) >> 32 for t in range(3))
    if row.group == "stepid":
        assert not bool(bias.any())
    else:
        assert not torch.equal(bias[0], bias[1]) and not torch.equal(dh[0], dh[1])


@pytest.mark.parametrize("row_id", [r.id for r in he.MPLOSS])
def test_trajectory_loss_inputs(row_id):
    row = he.BY_ID[row_id]
    B, T, nrot, ga = row.shape
    v = hr.mp_inputs(row)
    mask, gt = v["mask"].view(B, T), v["gt"]
    assert bool((mask.sum(1) >= 1).all()) and set(mask.unique().tolist()) <= {0.0, 1.0}
    bins = gt[:, 3:6]
    assert bool(((bins >= 0) & (bins < nrot) & (bins == bins.round())).all())
    assert set(gt[:, ga - 1].unique().tolist()) <= {0.0, 1.0}
    if row.opts["mask"] == "prefix":
        lens = mask.sum(1)
        assert bool((mask[:, :-1] >= mask[:, 1:]).all()) and float(lens.max()) == T and float(lens.min()) == (1 if B > 1 else T)
    elif row.opts["mask"] == "holes":
        assert bool((mask[:, :-1] < mask[:, 1:]).any())            # an inactive step before an active one
    else:
        assert bool((mask[:, 0] == 1).all()) and float(mask.sum()) == B
    if row.opts.get("b16"):
        assert torch.equal(v["ae"], v["ae"].bfloat16().float())
    ref = hr.mp_reference(row, v)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    g = hr.G5
    assert len(set(g)) == 5 and all(g) and min(g) < 0 and hr.POS_W != 1 and hr.ROT_W != 1


def test_position_ce_inputs():
    for row in he.POSCE:
        xt, tgt, g = hr.posce_inputs(row)
        n, nb = sum(row.shape), row.opts["nb"]
        assert xt.shape == (n, 3 * nb) and tgt.numel() == 3 * n * nb and g.numel() == 3 * len(row.shape)
        nz = g[g != 0]
        assert bool((g == 0).any()) and bool((g < 0).any()) and len(set(nz.tolist())) == nz.numel()
        ce, lse, tsum, dxt = hr.posce_reference(row, xt, tgt, g)
        assert bool(torch.isfinite(ce).all()) and bool(torch.isfinite(dxt).all())
        if row.opts["tgt"] == "zero":
            assert int((tsum == 0).sum()) == 1 and float(ce[tsum == 0]) == 0.0
        elif row.opts["tgt"] == "onehot":
            assert bool((tsum == 1).all())


def test_label_tie_rows_tie_exactly():
    """The tie rows hold what they promise: coordinates in eighths, and per axis of the long cloud exactly the planned points
    share the smallest distance, each with two bins."""
    from oracle import labels as ol

    for row in (r for r in he.LABELS if r.opts.get("ties")):
        pc, gt, robot, bin_size, xyz = hr.label_inputs(row)
        nb = row.opts["nb"]
        assert bin_size == 0.25 and robot is None
        assert bool((pc[:, :3] * 8 == np.round(pc[:, :3] * 8)).all()) and bool((gt[:, :3] * 8 == np.round(gt[:, :3] * 8)).all())
        for b, x in enumerate(xyz):
            d = np.abs(gt[b, None, :3, None] - ol.candidates(x, bin_size, nb // 2)).transpose(1, 0, 2).reshape(3, -1)
            for c in range(3):
                tied = np.nonzero(d[c] == d[c].min())[0]
                want = sorted({p for p, _ in he.tie_sites(len(x), nb)[c]}) if len(x) >= 300 else list(range(len(x)))
                assert sorted(set(tied // nb)) == want and len(tied) == 2 * len(want) and d[c].min() == 0.125
                ref = ol.disc_gt_pos_prob(x, gt[b, :3], bin_size, nb // 2, row.opts["kind"])
                assert ref[c].argmax() == tied[0] and ref[c].max() == 1.0


def test_decode_tie_rows_tie_exactly():
    for row in (r for r in he.LABELS if r.group == "dec" and r.opts["mode"] != "random"):
        xt = hr.dec_logits(row)
        nb, mode = row.opts["nb"], row.opts["mode"]
        assert bool((xt * 4 == (xt * 4).round()).all())
        o = 0
        for nn in row.shape:
            lg = xt[o:o + nn].view(nn, 3, nb).permute(1, 0, 2).reshape(3, -1)
            o += nn
            for c in range(3):
                at = torch.nonzero(lg[c] == lg[c].max()).view(-1).tolist()
                if mode == "first":
                    assert at == [0]
                elif mode == "last":
                    assert at == [nn * nb - 1]
                elif nn >= 300:
                    assert at == sorted(p * nb + j for p, j in he.tie_sites(nn, nb)[c])
                else:
                    assert at == list(range(nn * nb))


def test_cloud_max_inputs_hold_the_promised_ties():
    for row in he.CLOUDMAX:
        x, dy, add = hr.cloudmax_inputs(row)
        assert bool((x * 4 == (x * 4).round()).all())
        o = 0
        for nn in row.shape:
            seg = x[o:o + nn]
            o += nn
            chunk = -(-nn // he.CM_SPLITS)
            assert bool((seg[:, 0] == seg[0, 0]).all())
            assert int(seg[:, 1].argmax()) == nn - 1 and int((seg[:, 1] == seg[:, 1].max()).sum()) == 1
            if nn > chunk:
                rows = torch.nonzero(seg[:, 2] == seg[:, 2].max()).view(-1)
                assert len({int(r) // chunk for r in rows}) >= 2
            if chunk >= 2:
                rows = torch.nonzero(seg[:, 3] == seg[:, 3].max()).view(-1)
                assert len(rows) >= 2 and len({int(r) // chunk for r in rows}) == 1 and len({(int(r) % chunk) % 32 for r in rows[:2]}) == 2


# ------------------------------------------------------------------------------------------------- the numpy mask alone
def test_numpy_mask_restatement():
    idx = np.arange(1 << 20, dtype=np.uint64)
    seed = (0x1234 << 32) | 0x9ABCDEF0
    assert hr.drop_setup(0.0) == (0, np.float32(1.0)) and bool((hr.keep_scale(seed, idx, 0.0) == 1).all())
    assert hr.drop_setup(0.1) == (6553, np.float32(1.0 / (1.0 - 6553 / 65536.0))) and hr.drop_setup(0.5)[0] == 32768
    assert hr.drop_setup(1e-7)[0] == 1 and hr.drop_setup(0.25) == (16384, np.float32(4.0 / 3.0))
    for p in (0.1, 0.5):
        t16, inv = hr.drop_setup(p)
        s = hr.keep_scale(seed, idx, p)
        assert set(np.unique(s).tolist()) == {0.0, float(inv)} and s.dtype == np.float32
        keep = 1.0 - t16 / 65536.0
        assert abs(float((s != 0).mean()) - keep) <= 5 * (keep * (1 - keep) / idx.size) ** 0.5
        assert abs(float(s.astype(np.float64).mean()) - 1.0) <= 5 * float(inv) * (keep * (1 - keep) / idx.size) ** 0.5
        # one hash per pair: its low half decides the even, its high half the odd element
        h = hr.hash32(seed, idx[: idx.size // 2])
        assert np.array_equal(s[0::2] != 0, (h & np.uint32(0xFFFF)) >= t16) and np.array_equal(s[1::2] != 0, (h >> np.uint32(16)) >= t16)
    # the hash by hand, in Python integers, on indices and seeds with high halves
    def by_hand(seed, i):
        m = 0xFFFFFFFF
        x = ((i & m) * 0x9E3779B1 + (seed & m)) & m
        x ^= ((i >> 32) * 0x7FEB352D + (seed >> 32)) & m
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & m
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & m
        return x ^ (x >> 16)

    for s_, i in ((0, 0), (seed, 1), (seed, (5 << 32) | 77), ((1 << 62) | 3, (1 << 40) + 1)):
        assert int(hr.hash32(s_, np.array([i], dtype=np.uint64))[0]) == by_hand(s_, i)
    assert not np.array_equal(hr.hash32(seed, idx[:64]), hr.hash32(seed + (1 << 32), idx[:64]))


# ------------------------------------------------------------------------------------------------- argument checks
needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="calls entry points with host pointers: only safe without a device")

_DEFAULTS = dict(M=5, C=128, B=2, T=2, nrot=4, ga=7, nb=4, n=8, nc=2, ld=7, kind=0, act=2, accumulate=0, p=0.1, drop_p=0.1, pos_w=1.5,
                 rot_w=0.7, bin_size=0.01, seed=1, drop_seed=1)


def _call(L, name, host, **over):
    import ctypes

    restype, argtypes, names = L.protos[name]
    args = []
    for ty, nm in zip(argtypes, names):
        if nm in over:
            args.append(over[nm])
        elif ty is ctypes.c_void_p:
            args.append(None if nm == "stream" else host.ctypes.data)
        elif ty is ctypes.c_size_t:
            args.append(1 << 30)
        else:
            args.append(_DEFAULTS[nm])
    return L.fn[name](*args)


def _both(name):
    return (name, name.replace("lotus_", "lotus_b16_", 1))


@needs_no_device
def test_head_entry_points_refuse_bad_arguments(lib):
    host = np.zeros(1 << 16, dtype=np.float64)
    assert host.ctypes.data % 16 == 0
    refusals = [
        ("lotus_step_act_bwd", dict(C=12)), ("lotus_step_act_bwd", dict(C=2048)), ("lotus_step_act_bwd", dict(C=0)),
        ("lotus_step_act_bwd", dict(workspace_bytes=lib.fn["lotus_step_act_bwd_workspace"](5, 128) - 1)),
        ("lotus_step_act_fwd", dict(C=0)), ("lotus_step_act_fwd", dict(drop_p=1.0)),
        ("lotus_mp_loss_fwd", dict(B=8193)), ("lotus_mp_loss_fwd", dict(ga=6)), ("lotus_mp_loss_fwd", dict(T=0)), ("lotus_mp_loss_fwd", dict(nrot=0)),
        ("lotus_mp_loss_bwd", dict(B=8193)), ("lotus_mp_loss_bwd", dict(T=0)), ("lotus_mp_loss_bwd", dict(nrot=0)), ("lotus_mp_loss_bwd", dict(B=0)),
        ("lotus_pos_targets", dict(nb=5)), ("lotus_pos_targets", dict(workspace_bytes=lib.fn["lotus_pos_workspace"](2) - 1)),
        ("lotus_pos_decode_max", dict(nb=5)), ("lotus_pos_decode_max", dict(workspace_bytes=lib.fn["lotus_pos_workspace"](2) - 1)),
        ("lotus_cloud_max_fwd", dict(x=host.ctypes.data + 4)), ("lotus_cloud_max_fwd", dict(workspace_bytes=lib.fn["lotus_cloud_max_workspace"](2, 128) - 1)),
        ("lotus_dropout", dict(p=1.0)), ("lotus_drop_path", dict(C=6)),
        ("lotus_loss_fwd", dict(ga=6)), ("lotus_pos_ce_fwd", dict(nb=0)),
    ]
    for name in ("lotus_pool_max_fwd", "lotus_pool_max_bwd", "lotus_unpool_fwd", "lotus_unpool_bwd", "lotus_cloud_max_bwd", "lotus_cloud_max_fwd"):
        refusals += [(name, dict(C=0)), (name, dict(C=-4))]
    for name in ("lotus_loss_fwd", "lotus_loss_bwd"):
        refusals += [(name, dict(nb=0)), (name, dict(nb=-2)), (name, dict(nrot=0)), (name, dict(nrot=-1))]
    refusals += [("lotus_pos_ce_bwd", dict(nb=0)), ("lotus_pos_ce_bwd", dict(nb=-2))]
    assert lib.fn["lotus_abi_version"]() == 3
    for base, over in refusals:
        for name in _both(base):
            assert name in lib.protos, name
            # with its defaults the call passes every check and gets as far as the launch, which has no device here ...
            assert _call(lib, name, host) == -2, (name, lib.last_error())
            # ... so the refusal is that of the one argument
            rc = _call(lib, name, host, **over)
            assert rc == E_ARG, (name, over, rc, lib.last_error())
    assert not host.any()
