"""Host test (no GPU) of the invariant behind tests/test_gpu_side_stream_lifetime.py: a tensor handed to ops._OnSide(...)
inside a `_joined` backward stays alive until the join that orders the critical stream behind the weight-gradient stream —
although the body dropped it — and not a moment longer than that.  The side stream is stubbed (ops._side, ops._SIDES, the
C-ABI stream link); the tensors are CPU tensors watched through weakrefs; the nodes run under the real autograd engine, so
the end-of-backward callback of the "end" mode is the engine's own."""
import gc
import weakref

import pytest
import torch


class _Fake:
    """What the stubs record: the tensors' weakrefs, and which of them were alive at each join."""

    def __init__(self):
        self.refs, self.at_join, self.after_drop = [], [], []

    def alive(self):
        gc.collect()
        return [r() is not None for r in self.refs]


SIDE_PTR, MAIN_PTR = 22, 11


@pytest.fixture
def side(monkeypatch):
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi, ops

    fake = _Fake()
    stream = object()

    def call_raw(name, *a):
        # lotus_streamlink_wait(link, waited-for stream, waiting stream): the join is the main stream waiting for the side stream
        if name == "lotus_streamlink_wait" and a[1] == SIDE_PTR:
            fake.at_join.append(fake.alive())

    monkeypatch.setattr(_capi, "call_raw", call_raw)
    monkeypatch.setattr(_capi, "stream_ptr", lambda: MAIN_PTR)
    monkeypatch.setattr(_capi, "STREAM_OVERRIDE", 0)
    monkeypatch.setattr(ops, "_SIDES", [(stream, SIDE_PTR)])
    monkeypatch.setattr(ops, "SIDE", stream)
    monkeypatch.setattr(ops, "_LINK", 1)
    monkeypatch.setattr(ops, "_SIDE_ON", True)
    monkeypatch.setattr(ops, "_side", lambda: stream if ops._IN_NODE > 0 else None)
    monkeypatch.setattr(ops, "_JOIN", "node")
    monkeypatch.setattr(ops, "_END_CB_PENDING", False)
    assert ops._IN_NODE == 0 and not ops._HELD
    fake.ops = ops
    yield fake
    ops._HELD.clear()


def _node(fake, fail=False):
    """An autograd node whose backward forks twice and drops what the side stream reads before it goes on (as
    ops.ffn_branch_bwd does with dz2 and dh when it returns)."""
    ops = fake.ops

    def body():
        for _ in range(2):
            t = torch.ones(8)
            fake.refs.append(weakref.ref(t))
            with ops._OnSide(t, None):
                assert fake.ops._capi.STREAM_OVERRIDE == SIDE_PTR
            del t
        fake.after_drop.append(fake.alive())

    class Node(torch.autograd.Function):
        @ops._fwd
        def forward(ctx, x):
            return x * 2.0

        @ops._joined
        def backward(ctx, dy):
            body()
            if fail:
                raise RuntimeError("backward failed")
            return dy * 2.0

    return Node


def _backward(node, n=1):
    x = torch.ones(3, requires_grad=True)
    y = x
    for _ in range(n):
        y = node.apply(y)
    y.sum().backward()
    return x.grad


@pytest.mark.parametrize("join", ["node", "end"])
def test_reads_outlive_the_body_until_the_join(side, monkeypatch, join):
    ops = side.ops
    monkeypatch.setattr(ops, "_JOIN", join)
    g = _backward(_node(side), n=2)
    assert torch.equal(g, torch.full((3,), 4.0))
    # (1) alive after the body dropped them, i.e. when the node hands control back to `_joined`
    assert side.after_drop == [[True, True], [join == "end", join == "end", True, True]], side.after_drop
    # (2) alive at the join that covers them: each node's ("node"), the single one at the end of the pass ("end")
    if join == "node":
        assert side.at_join == [[True, True], [False, False, True, True]], side.at_join
    else:
        assert side.at_join == [[True, True, True, True]], side.at_join
    # (3) released behind it; nothing is retained once no node is running
    assert ops._IN_NODE == 0 and not ops._END_CB_PENDING and ops._capi.STREAM_OVERRIDE == 0
    assert side.alive() == [False] * 4
    assert not ops._HELD


def test_a_failing_node_releases_what_it_held(side):
    ops = side.ops
    with pytest.raises(RuntimeError, match="backward failed"):
        _backward(_node(side, fail=True))
    assert side.after_drop == [[True, True]]
    assert side.at_join == [[True, True]], "the node's join is made on the way out of a failing node, too"
    assert ops._IN_NODE == 0
    assert side.alive() == [False, False]


def test_a_failing_pass_in_end_mode_releases_at_the_next_forward(side, monkeypatch):
    """The engine drops its queued callbacks when a node raises: the next forward notices (ops._abandoned_backward), joins and
    releases, or _HELD would grow for good."""
    ops = side.ops
    monkeypatch.setattr(ops, "_JOIN", "end")
    with pytest.raises(RuntimeError, match="backward failed"):
        _backward(_node(side, fail=True))
    assert ops._IN_NODE == 0 and ops._END_CB_PENDING and side.alive() == [True, True] and side.at_join == []
    _node(side).apply(torch.ones(3))
    assert not ops._END_CB_PENDING and side.at_join == [[True, True]]
    assert side.alive() == [False, False] and not ops._HELD


def test_no_hold_without_a_side_stream(side, monkeypatch):
    """One stream (the side stream off): nothing to order, nothing held."""
    ops = side.ops
    monkeypatch.setattr(ops, "_side", lambda: None)
    monkeypatch.setattr(ops, "SIDE", None)
    _backward(_node_plain(side))
    assert side.after_drop == [[False, False]] and side.at_join == []


def _node_plain(fake):
    ops = fake.ops

    class Node(torch.autograd.Function):
        @ops._fwd
        def forward(ctx, x):
            return x * 2.0

        @ops._joined
        def backward(ctx, dy):
            for _ in range(2):
                t = torch.ones(8)
                fake.refs.append(weakref.ref(t))
                with ops._OnSide(t, None):
                    assert ops._capi.STREAM_OVERRIDE == 0
                del t
            fake.after_drop.append(fake.alive())
            return dy * 2.0

    return Node
