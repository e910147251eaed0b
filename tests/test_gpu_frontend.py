"""GPU parity of the integer front-end (csrc/front_end.hip) against the oracle: bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import front_end as fe  # noqa: E402
from frontend_util import assert_levels_equal, count_duplicates  # noqa: E402


def _levels(batch, n_levels, perms):
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    pc = batch["pc_fts"].cuda()
    fr = FrontEnd(n_levels)
    lv = fr.build(pc, batch["npoints_in_batch"], batch["txt_lens"], perms, need_coord=True)
    torch.cuda.synchronize()
    return lv, fr


@pytest.mark.parametrize("B,n,ragged,seed", [(1, 512, False, 0), (3, 700, True, 1), (4, 2048, True, 2), (16, 4096, False, 3),
                                             # the batch sizes the README quotes throughput at: 155 648 ... 524 288 points, past
                                             # the first segment of the radix scan and the first round of the pooling carry
                                             (38, 4096, False, 4), (64, 4096, False, 5), (128, 4096, False, 6), (64, 4096, True, 7),
                                             (1, 4096, False, 8), (1, 100, False, 9)])
def test_frontend_bit_exact(B, n, ragged, seed):
    from robot_3dlotus_amd import synth

    batch = synth.synth_batch(B, n, ragged=ragged, seed=seed)
    rng = np.random.default_rng(seed)
    n_levels = 5
    perms = [rng.permutation(4).tolist() for _ in range(n_levels)]
    ref = fe.build_all_levels(batch["pc_fts"][:, :3].numpy(), batch["npoints_in_batch"], n_levels, perms=perms)
    got, fr = _levels(batch, n_levels, perms)
    assert_levels_equal(ref, got, n_levels, batch["txt_lens"])
    assert fr.depth_bound == ref[0]["depth"]
    # second call uses the tightened depth bound (fewer radix passes) and must agree
    got2, _ = _levels(batch, n_levels, perms)
    for a, b in zip(got, got2):
        assert torch.equal(a.order, b.order) and torch.equal(a.nbr27, b.nbr27)


def test_frontend_duplicate_voxels_lowest_index():
    """Trap 5: duplicate voxels -> stable (code, index) order, hash keeps the lowest index."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import synth

    batch = synth.synth_batch(2, 600, ragged=False, seed=5)
    pc = batch["pc_fts"].clone()
    pc[10, :3] = pc[3, :3]       # exact duplicates inside cloud 0
    pc[700, :3] = pc[650, :3]    # and inside cloud 1
    batch["pc_fts"] = pc
    perms = [[0, 1, 2, 3]] * 3
    ref = fe.build_all_levels(pc[:, :3].numpy(), batch["npoints_in_batch"], 3, perms=perms)
    got, _ = _levels(batch, 3, perms)
    for s in range(3):
        np.testing.assert_array_equal(got[s].order.cpu().numpy(), ref[s]["order"])
        np.testing.assert_array_equal(got[s].nbr27.cpu().numpy().T, ref[s]["nbr27"])


def test_frontend_determinism_and_properties_full_size():
    """BASELINE full size (16 x 4096): run twice -> identical; order[inverse] == arange; every padded
    patch <= 128 rows; pooled points keep the code hierarchy."""
    from robot_3dlotus_amd import synth

    batch = synth.synth_batch(16, 4096, seed=9)
    perms = [[2, 0, 3, 1]] * 5
    a, _ = _levels(batch, 5, perms)
    b, _ = _levels(batch, 5, perms)
    for x, y in zip(a, b):
        assert torch.equal(x.order, y.order) and torch.equal(x.code, y.code) and torch.equal(x.nbr27, y.nbr27)
        ar = torch.arange(x.n, device="cuda", dtype=torch.int32)
        for k in range(4):
            assert torch.equal(x.order[k][x.inverse[k].long()], ar)
            c = x.code[k][x.order[k].long()]
            assert (c[1:] >= c[:-1]).all()
        assert int(x.self_tiles[:, 1].max()) <= 128
    assert a[0].n == 65536


def _build_and_compare(batch, n_levels, seed, fr=None):
    """One batch through the oracle and through FrontEnd (`fr`: an existing object, else a fresh one): bit-exact."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    rng = np.random.default_rng(seed)
    perms = [rng.permutation(4).tolist() for _ in range(n_levels)]
    ref = fe.build_all_levels(batch["pc_fts"][:, :3].numpy(), batch["npoints_in_batch"], n_levels, perms=perms)
    fr = fr or FrontEnd(n_levels)
    got = fr.build(batch["pc_fts"].cuda(), batch["npoints_in_batch"], batch["txt_lens"], perms, need_coord=True)
    torch.cuda.synchronize()
    assert_levels_equal(ref, got, n_levels, batch["txt_lens"])
    return ref, got, fr


def _batch_of_counts(counts, seed):
    """A synth_batch-shaped dict (the fields the front-end reads) whose clouds have exactly `counts` points."""
    from robot_3dlotus_amd import synth

    rng = np.random.default_rng(seed)
    pcs = [synth.synth_cloud(rng, n) for n in counts]
    return {"pc_fts": torch.from_numpy(np.concatenate(pcs, 0)), "npoints_in_batch": list(counts),
            "txt_lens": [int(t) for t in rng.integers(6, 20, size=len(counts))]}


def _moved(batch, row, metres):
    """The batch with point `row` moved by `metres` along x, y and z: an outlier that sets the serialisation depth."""
    out = dict(batch)
    pc = batch["pc_fts"].clone()
    pc[row, :3] += metres
    out["pc_fts"] = pc
    return out


def test_frontend_augmented_clouds_count_their_duplicates():
    """Rotation + jitter puts 1-7 % of the points into an occupied voxel: the order, the hash and n_dup at 16 x 4096."""
    from robot_3dlotus_amd import synth

    batch = synth.augment_clouds(synth.synth_batch(16, 4096, seed=31), seed=32)
    ref, got, _ = _build_and_compare(batch, 5, 31)
    n_dup = count_duplicates(ref[0]["grid"], ref[0]["batch"])
    assert 0.01 * 65536 <= n_dup <= 0.07 * 65536, n_dup
    assert got[0].n_dup == n_dup
    assert all(g.n_dup == 0 for g in got[1:])


TINY_COUNTS = [1, 2, 127, 128, 129, 255, 256, 257, 1, 4096]


def test_frontend_tiny_clouds_at_the_patch_edges():
    """Clouds of 1 .. 2 K + 1 points at level 0 (no padding up to K, K - 1 borrowed rows at K + 1, none at 2 K) and ~20-point
    clouds at the deep levels; the tile lists (self_tiles, ca_tiles, ca_blocks) tile every level exactly."""
    batch = _batch_of_counts(TINY_COUNTS, 41)
    ref, got, _ = _build_and_compare(batch, 5, 41)     # (assert_levels_equal checks the tile lists of every level)
    assert ref[0]["depth"] == 6 and count_duplicates(ref[0]["grid"], ref[0]["batch"]) == 0
    assert got[0].counts == TINY_COUNTS and got[0].n_extra == 127 + 1 + 127
    assert got[4].counts[0] == 1 and got[4].counts[8] == 1 and max(got[4].counts) < 128
    assert got[0].ca_groups == 8 and got[4].ca_groups == 1


@pytest.mark.parametrize("metres,depth", [(40.0, 12), (-40.0, 12)])
def test_frontend_deep_grid(metres, depth):
    """One depth pixel 40 m away (real clouds contain them before cropping): serialisation depth 12 instead of the synthetic
    scenes' 7.  At -40 m the outlier is the batch minimum, so every other point sits at grid ~4000."""
    from robot_3dlotus_amd import synth

    batch = _moved(synth.synth_batch(4, 2048, seed=51), 3000, metres)
    ref, got, fr = _build_and_compare(batch, 5, 51)
    assert ref[0]["depth"] == depth and fr.depth_bound == depth
    if metres < 0:
        assert np.median(ref[0]["grid"]) > 3900


def test_frontend_depth_bound_sequence():
    """ONE FrontEnd object: the bound on the serialisation depth (= the number of radix passes) tightens to the first batch,
    a deeper batch raises the device flag and is rebuilt with the loose bound, a shallow batch tightens it again, a batch
    deeper than 16 levels is an error that leaves the object usable."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import synth
    from robot_3dlotus_amd.frontend import FrontEnd

    shallow = synth.synth_batch(4, 2048, seed=61)
    deep = _moved(synth.synth_batch(4, 2048, ragged=True, seed=62), 100, 40.0)
    too_deep = _moved(shallow, 5000, 700.0)
    fr = FrontEnd(5)
    launches, launch0 = [], fr._launch

    def counting_launch(*a, **kw):
        launches.append(fr.depth_bound)
        return launch0(*a, **kw)

    fr._launch = counting_launch
    assert fr.depth_bound == 16
    ref, _, _ = _build_and_compare(shallow, 5, 61, fr)
    assert ref[0]["depth"] == 7 and fr.depth_bound == 7 and launches == [16]
    ref, _, _ = _build_and_compare(deep, 5, 62, fr)
    assert ref[0]["depth"] == 12 and fr.depth_bound == 12
    assert launches == [16, 7, 16], "the deep batch was not rebuilt after the device flag"
    _build_and_compare(shallow, 5, 63, fr)
    assert fr.depth_bound == 7 and launches == [16, 7, 16, 12]
    assert fe.serialized_depth(fe.grid_coord(too_deep["pc_fts"][:, :3].numpy())) == 17
    with pytest.raises(ValueError, match="depth 17"):
        fr.build(too_deep["pc_fts"].cuda(), too_deep["npoints_in_batch"], too_deep["txt_lens"], [[0, 1, 2, 3]] * 5)
    torch.cuda.synchronize()
    _build_and_compare(shallow, 5, 64, fr)
    assert fr.depth_bound == 7


def test_frontend_rejects_a_cloud_smaller_than_its_pooling_pyramid():
    """5 levels need 2^4 voxels of extent; a cloud spanning < 8 voxels per axis has depth <= 3."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd.frontend import FrontEnd

    rng = np.random.default_rng(71)
    pc = torch.from_numpy(rng.uniform(0.0, 0.075, size=(300, 7)).astype(np.float32))
    assert fe.serialized_depth(fe.grid_coord(pc[:, :3].numpy())) == 3
    with pytest.raises(NotImplementedError, match="pooling_depth 0"):
        FrontEnd(5).build(pc.cuda(), [200, 100], [7, 9], [[0, 1, 2, 3]] * 5)
    torch.cuda.synchronize()


_TABLES = ("grid", "batch", "code", "order", "inverse", "nbr27", "nbr125", "gidx", "owner", "kext", "ext_pos", "self_tiles",
           "self_blocks", "ca_tiles", "ca_blocks", "cluster", "seg_start", "members", "coord", "off")


@pytest.mark.parametrize("finish_on_side", [True, False])
def test_frontend_prefetch_equals_build(finish_on_side, monkeypatch):
    """launch() on a side stream + finish() (the prefetch of the next batch under the backward pass) returns the tables of
    build(), whichever stream builds the exactly sized half."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import frontend, synth

    monkeypatch.setattr(frontend, "FINISH_ON_SIDE", finish_on_side)
    batch = synth.synth_batch(64, 4096, seed=5)
    perms = [[1, 3, 0, 2], [0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1], [1, 0, 2, 3]]
    pc = batch["pc_fts"].cuda()
    a = frontend.FrontEnd(5).build(pc, batch["npoints_in_batch"], batch["txt_lens"], perms, need_coord=True)
    fr = frontend.FrontEnd(5)
    side = torch.cuda.Stream()
    for _ in range(2):   # loose bound, then the tightened one
        pend = fr.launch(pc, batch["npoints_in_batch"], perms, stream=side)
        b = fr.finish(pend, batch["txt_lens"], need_coord=True)
        torch.cuda.synchronize()
        for s, (x, y) in enumerate(zip(a, b)):
            assert (x.n, x.counts, x.depth, x.npad, x.n_extra, x.n_dup) == (y.n, y.counts, y.depth, y.npad, y.n_extra, y.n_dup)
            for name in _TABLES:
                tx, ty = getattr(x, name), getattr(y, name)
                assert (tx is None) == (ty is None), (s, name)
                if tx is not None:
                    if name == "ext_pos":   # (one unspecified element when the level borrows no row)
                        tx, ty = tx[:x.n_extra], ty[:y.n_extra]
                    assert torch.equal(tx, ty), (s, name)
