"""parallel.GradReducer's slab arena on the host: layout, trainer order, changed node order, skipped nodes, accounting.

The arena decides WHERE a gradient lives; it is a host-side mechanism, so it is tested here with pure-torch stand-ins of the
backward nodes (tests/dp_util.py: SlabLinear takes its `dw | db` slab from ops._grad_slab as ops.linear_wgrad does) and with
the arena switched on for host tensors (GradReducer.arena_on_host).  Both sides of every comparison run the same torch
operations on the same values, so every bar is bit equality, per parameter, by name."""
import itertools

import pytest
import torch

import dp_util as du

W = 8                       # width of the toy layers: Lin(8 -> 8) is a slab of 72 floats (128 padded), Lin(8 -> 5) one of 45 (64)
EACH, ONE = du.mb(2), 32.0  # bucket caps: every layout unit in its own bucket / one bucket


def _x(seed, rows=6):
    return torch.randn(rows, W, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ layout
class _Bag(torch.nn.Module):
    """Parameters only: odd units of 1, 3, 5 and 217 floats, four (weight, bias) pairs whose gradients share a slab of
    45, 72, 325 and 4160 floats, and two parameters that never get a gradient."""
    SLABS = {"s45": (5, 8), "s72": (8, 8), "s325": (5, 64), "s4160": (64, 64)}

    def __init__(self):
        super().__init__()
        for n in (1, 3, 5, 217):
            setattr(self, f"o{n}", torch.nn.Parameter(torch.zeros(n)))
        for name, (n, k) in self.SLABS.items():
            setattr(self, name + "w", torch.nn.Parameter(torch.zeros(n, k)))
            setattr(self, name + "b", torch.nn.Parameter(torch.zeros(n)))
        self.cold1, self.cold2 = torch.nn.Parameter(torch.zeros(7)), torch.nn.Parameter(torch.zeros(2, 3))


LAYOUT_ROWS = {
    # odd units in front of, between and behind slabs
    "odd_first": "o3 s45w s45b s72w s72b o1 s325w s325b o217 s4160w s4160b o5",
    "slab_first": "s4160w s4160b o1 s45w s45b o217 o5 s325w s325b s72w s72b o3",
    # the bias arrives before the weight, and another parameter between the two of one slab
    "bias_first": "o5 s72b s72w o3 s325b o1 s325w s45b s45w o217 s4160b s4160w",
    "odd_only_tail": "s45w s45b s72w s72b s325w s325b s4160w s4160b o1 o3 o5 o217",
}


@pytest.mark.parametrize("cap", [2, 200, 5000, 1 << 23], ids=["each", "cap200", "cap5000", "one"])
@pytest.mark.parametrize("row", sorted(LAYOUT_ROWS))
def test_layout_aligns_slabs_and_tiles_the_flat_buffer(row, cap):
    bag = _Bag()
    named = dict(bag.named_parameters())
    red = du.host_reducer(bag, du.mb(cap))
    order = [named[n] for n in LAYOUT_ROWS[row].split()]
    cold = [bag.cold1, bag.cold2]
    ids = {s: k for k, s in enumerate(_Bag.SLABS)}
    sizes = [n * k + n for n, k in _Bag.SLABS.values()]
    where = {}
    for s, (n, k) in _Bag.SLABS.items():
        where[named[s + "w"]], where[named[s + "b"]] = (ids[s], 0), (ids[s], n * k)

    def snapshot():
        red._layout(order, cold, (sizes, where))
        base = red.flat.data_ptr()
        return (dict(red._slab_at), list(red.buckets), {n: (p_view.data_ptr() - base) // 4 for n, p in named.items()
                                                       for p_view in [red.view_of(p)]}, dict((n, red._slot[p]) for n, p in named.items()))

    slab_at, buckets, at, slot = snapshot()
    assert red.flat.data_ptr() % 256 == 0
    assert all(v % 64 == 0 for v in slab_at.values()), slab_at          # float offsets: 64 floats = 256 bytes
    # the buckets tile the flat buffer in order
    assert buckets[0][0] == 0 and buckets[-1][1] == red.flat.numel(), buckets
    assert all(a[1] == b[0] and a[0] < a[1] for a, b in zip(buckets, buckets[1:])), buckets
    # every parameter owns one view of its own shape inside its bucket, and the views are pairwise disjoint
    assert set(at) == set(named) and all(red.view_of(p).shape == p.shape for p in named.values())
    spans = sorted((at[n], at[n] + named[n].numel(), n) for n in named)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    assert all(buckets[slot[n]][0] <= lo and hi <= buckets[slot[n]][1] for lo, hi, n in spans), (spans, buckets)
    # a slab lies whole (with its padding to 64 floats) inside ONE bucket, its parameters at the node's own offsets
    for s, k in ids.items():
        lo, hi = slab_at[k], slab_at[k] + (sizes[k] + 63) // 64 * 64
        b = slot[s + "w"]
        assert slot[s + "b"] == b and buckets[b][0] <= lo and hi <= buckets[b][1], (s, lo, hi, buckets)
        assert at[s + "w"] == lo and at[s + "b"] == lo + where[named[s + "b"]][1]
    # the cold parameters form the trailing bucket
    assert slot["cold1"] == slot["cold2"] == len(buckets) - 1 and at["cold2"] + 6 == red.flat.numel()
    # a pure function of (order, cold, slabs): every rank computes the same layout
    assert snapshot() == (slab_at, buckets, at, slot)


# ------------------------------------------------------------------------------------------------ trainer order
@pytest.mark.parametrize("zero", ["first", "last"])
def test_arena_engages_whatever_the_zero_grad_order(zero):
    """zero = "last": the first backward runs with no zero_grad() before it (a trainer that clears at the END of its step)."""
    net = du.Branches("cpu", [W, 5, W], W)
    red = du.host_reducer(net, EACH)
    log = du.ArenaLog(red)
    order = [0, 1, 2]
    total = sum(p.numel() for p in net.parameters())
    steps = []
    for k in range(4):
        x = _x(10 + k)
        steps.append(du.run_step(red, net, (x, order), du.plain_grads(net, x, order), zero)[:2] + (len(log.take()),))
    # step 1 learns; step 2 is the first whose slabs come from the flat buffer; from the third step on at the latest
    assert steps[0] == (0, total, 0), steps
    assert all(s == (total - 3, 3, 3) for s in steps[2:]), steps     # everything but `scale` is born in place
    assert steps[1] == steps[2], steps


# ------------------------------------------------------------------------------------------------ changed node order
def _learn(net, red, args, steps=2):
    for k in range(steps):
        du.run_step(red, net, args(k), du.plain_grads(net, *args(k)))


def test_swapped_order_in_different_buckets_keeps_every_gradient():
    """Two equal-sized nodes, each in its own bucket, run in swapped order: each is served the OTHER's slab."""
    net = du.Branches("cpu", [5, 5], W)
    red = du.host_reducer(net, EACH)
    log = du.ArenaLog(red)
    _learn(net, red, lambda k: (_x(20 + k), [0, 1]))
    a, b = net.br
    assert red._slot[a.weight] == red._slot[a.bias] != red._slot[b.weight] == red._slot[b.bias], red._slot.values()
    log.take()
    x = _x(29)
    want = du.plain_grads(net, x, [1, 0])
    assert not torch.equal(want["br.0.weight"], want["br.1.weight"]) and not torch.equal(want["br.0.bias"], want["br.1.bias"])
    inplace, copied, n = du.run_step(red, net, (x, [1, 0]), want)
    assert n == 5 and len(log.take()) == 2 and (inplace, copied) == (0, 93)   # both slabs served, both gradients moved home
    # ... and the learnt order is served in place again
    x = _x(30)
    assert du.run_step(red, net, (x, [0, 1]), du.plain_grads(net, x, [0, 1]))[:2] == (90, 3)


@pytest.mark.parametrize("cap", [2, 129, 1 << 23], ids=["each", "two_per_bucket", "one"])
def test_every_creation_order_of_five_branches(cap, monkeypatch):
    """Four equal-sized branches and one of another size, learnt in one order, then created in all 120."""
    monkeypatch.setenv("LOTUS_DIAG_NO_TAPER", "1")   # (the tapered tail would give the last three units a bucket each)
    sizes = [W, W, 5, W, W]
    net = du.Branches("cpu", sizes, W)
    red = du.host_reducer(net, du.mb(cap))
    log = du.ArenaLog(red)
    base = [0, 1, 2, 3, 4]
    _learn(net, red, lambda k: (_x(40 + k), base))
    nb = len(red.buckets)
    assert nb == {2: 6, 129: 3, 1 << 23: 1}[cap], red.buckets
    total = sum(p.numel() for p in net.parameters())
    served = moved = 0
    for k, order in enumerate(itertools.permutations(base)):
        x = _x(100 + k)
        inplace, copied, n = du.run_step(red, net, (x, list(order)), du.plain_grads(net, x, list(order)))
        assert n == 11 and inplace + copied == total
        served += len(log.take())
        moved += copied - 3
    # the sweep did go through the arena and through the moves (a request of another size ends the serving for its step)
    assert served >= 2 * 120 and moved > 0, (served, moved)


def test_a_slab_of_a_flushed_bucket_is_not_served():
    """Branch 1's gradients arrive WITHOUT a slab request (plain torch), early enough for its bucket to leave before the
    node at that slab's position asks: the request must be refused, and serving stops for the step."""
    net = du.Branches("cpu", [5, 5, 5], W)
    red = du.host_reducer(net, EACH)
    red.sparse_hooks = False   # a counting hook on every parameter: a bucket leaves with its last gradient, whichever that is
    log = du.ArenaLog(red)
    _learn(net, red, lambda k: (_x(50 + k), [0, 1, 2]))     # backward: scale, 2, 1, 0
    log.take()

    def loss(m, x):
        # created 0, 1, 2 — backward runs 2, 1, 0 as learnt — but branch 1 goes through torch's own linear: no slab request
        t0 = torch.tanh(m.br[0](x)).mean()
        t1 = torch.sin(torch.nn.functional.linear(x, m.br[1].weight, m.br[1].bias)).mean()
        return m.scale.square().sum() * (t0 + t1 + torch.sigmoid(m.br[2](x)).mean())

    x = _x(59)
    tw = du.twin(net)
    loss(tw, x).backward()
    want = {n: p.grad.clone() for n, p in tw.named_parameters()}
    red.zero_grad()
    loss(net, x).backward()
    assert red._flushed[red._slot[net.br[1].weight]] and red._flushed[red._slot[net.br[2].weight]]   # left from their hooks
    red.finish()
    du.check_step(red, net, want)
    # branch 2's slab sits in the first slab bucket and is served (position 0); its bucket and then branch 1's — complete
    # without any request — leave; position 1 is branch 1's slab: its bucket is gone, so branch 0 gets a plain tensor
    assert len(log.take()) == 1


# ------------------------------------------------------------------------------------------------ skipped nodes, forced collectives
@pytest.fixture
def one_rank_gloo(monkeypatch):
    import torch.distributed as dist

    monkeypatch.setenv("LOTUS_FORCE_COLLECTIVES", "1")
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


PLAN = [1, 1, 0, 1, 0, 0, 1]   # 1: node b of a -> [b] -> c runs in that step


def test_skipped_node_under_forced_collectives(one_rank_gloo):
    """find_unused_parameters: in a step that skips b, a is served b's slab — which finish() zero-fills for b."""
    net = du.Chain("cpu", W)
    red = du.host_reducer(net, EACH)
    assert red._force and red.world == 1
    log = du.ArenaLog(red)
    seen = []
    for k, use in enumerate(PLAN):
        x = _x(60 + k)
        want = du.plain_grads(net, x, bool(use))
        assert (want["b.weight"] is None) == (not use)
        inplace, copied, n = du.run_step(red, net, (x, bool(use)), want)
        seen.append((use, n, inplace, copied, len(log.take())))
    assert len({red._slot[m.weight] for m in (net.a, net.b, net.c)}) == 3
    # steps 3.. : b used -> three slabs in place; b skipped -> c in place, a moved out of b's slab and home by copy
    assert seen[0] == (1, 6, 0, 216, 0) and all(s == ((1, 6, 216, 0, 3) if s[0] else (0, 4, 72, 72, 2)) for s in seen[1:]), seen


def test_skipped_node_of_another_size_ends_the_serving(one_rank_gloo):
    net = du.Chain("cpu", W, mid=6)     # slabs a: 54, b: 42, c: 56 floats
    red = du.host_reducer(net, EACH)
    log = du.ArenaLog(red)
    seen = []
    for k, use in enumerate(PLAN):
        x = _x(70 + k)
        inplace, copied, n = du.run_step(red, net, (x, bool(use)), du.plain_grads(net, x, bool(use)))
        seen.append((use, n, inplace, copied, len(log.take())))
    # b skipped: c is served (position 0), a asks for 54 floats at b's position (42) -> refused, and packed by copy
    assert seen[0] == (1, 6, 0, 152, 0) and all(s == ((1, 6, 152, 0, 3) if s[0] else (0, 4, 56, 54, 1)) for s in seen[1:]), seen


# ------------------------------------------------------------------------------------------------ accounting
def test_inplace_and_copied_floats_account_for_every_gradient():
    net = du.Chain("cpu", W, aux=5)
    red = du.host_reducer(net, du.mb(129))
    numel = {n: p.numel() for n, p in net.named_parameters()}
    plan = [(1, 0), (1, 0), (1, 0), (0, 0), (1, 1), (1, 0), (0, 1), (1, 0)]     # (b used, auxiliary head used)
    for k, (use_b, use_aux) in enumerate(plan):
        x = _x(80 + k)
        want = du.plain_grads(net, x, bool(use_b), bool(use_aux))
        inplace, copied, _ = du.run_step(red, net, (x, bool(use_b), bool(use_aux)), want)
        assert inplace + copied == sum(numel[n] for n, w in want.items() if w is not None), (k, inplace, copied)
        if k in (1, 2, 5, 7):   # the learnt graph again: every float of the toy is a slab float
            assert (inplace, copied) == (216, 0), (k, inplace, copied)
    # steady state of a net with a non-slab parameter: the in-place share is slab floats over all floats
    net = du.Branches("cpu", [W, 5, W], W)
    red = du.host_reducer(net, ONE)
    for k in range(4):
        inplace, copied, _ = du.run_step(red, net, (_x(90 + k), [0, 1, 2]))
    total = sum(p.numel() for p in net.parameters())
    assert (inplace, copied) == (total - 3, 3) and inplace / (inplace + copied) == (total - 3) / total


# ------------------------------------------------------------------------------------------------ the Concat stem's one parameter
@pytest.mark.parametrize("use", ["both", "pc", "ctx"])
def test_split_stem_weight_gradient_is_one_slab(use):
    """concat.split_stem_weight: the same two operands and the same gradient as autograd's own slices, bit for bit — and the
    gradient of the one parameter is the slab ops._grad_slab handed out (so a reducer's arena can own it)."""
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import concat, ops

    g = torch.Generator().manual_seed(3)
    w = torch.randn(6, 5, 5, 5, 11, generator=g, requires_grad=True)
    c_pc, T = 4, 125
    a0, b0 = w[..., :c_pc].contiguous(), w[..., c_pc:].reshape(6, T, -1).permute(1, 0, 2).reshape(T * 6, -1).contiguous()
    a1, b1 = concat.split_stem_weight(w, c_pc)
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and a1.is_contiguous() and b1.is_contiguous()
    ga, gb = torch.randn(a0.shape, generator=g), torch.randn(b0.shape, generator=g)
    pick = {"both": lambda a, b: ([a, b], [ga, gb]), "pc": lambda a, b: ([a], [ga]), "ctx": lambda a, b: ([b], [gb])}[use]
    torch.autograd.backward(*pick(a0, b0))
    want, w.grad = w.grad.clone(), None
    handed = []
    ops.GRAD_ARENA = lambda n, dev: handed.append(torch.full((n,), float("nan"))) or handed[-1]
    try:
        torch.autograd.backward(*pick(a1, b1))
    finally:
        ops.GRAD_ARENA = None
    assert torch.equal(w.grad, want)
    assert len(handed) == 1 and handed[0].numel() == w.numel() and w.grad.data_ptr() == handed[0].data_ptr()
