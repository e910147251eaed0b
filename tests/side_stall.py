"""Test-only harness: make the weight-gradient ("side") stream LATE on purpose.

The backward nodes of ops.py fork their weight-gradient launches to a second stream and join it at the end of the node
("node") or of the backward pass ("end").  Whether a tensor the side stream reads may be recycled by the critical stream
before that join only shows when the side stream is behind — which, in a quiet process, it never is.  `Stall` parks a sleep
kernel on the side stream in front of the first fork of every node (of the pass, in "end" mode), long enough for the
critical stream to finish the whole node first, and PROVES afterwards with events that it was: a run in which the side
stream was not still parked when the critical stream reached the join fails ("stall ineffective"), it never passes.

Nothing here touches memory outside torch's caching allocator: a recycled block gives a wrong number, not a fault."""
import torch

FLOOR_MS, CAP_MS = 2.0, 250.0

_CYCLES_PER_MS = None
_INDEPENDENT = None


def _mods():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import _capi, ops

    return ops, _capi


def side_stream():
    """The stream ops._side() adopts as the weight-gradient stream (it exists before the first backward)."""
    return _mods()[1].step_stream("side")


def cycles_per_ms():
    """torch.cuda._sleep counts device clock ticks; their rate is measured once per process with a pair of timing events."""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        torch.cuda._sleep(1000)  # (loads the kernel)
        torch.cuda.synchronize()
        n, rate = 1_000_000, None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            assert ms > 0.0, ms
            rate = n / ms
            if ms >= 2.0:   # long enough for the launch overhead not to matter
                break
            n = int(rate * 5.0)
        _CYCLES_PER_MS = rate
    return _CYCLES_PER_MS


def assert_streams_independent():
    """A kernel parked on the side stream must not hold the current stream back (they could share a hardware queue): then
    a stall would only delay everything and prove nothing.  Asked once per process, asserted before every stalled run."""
    global _INDEPENDENT
    if _INDEPENDENT is None:
        _, _capi = _mods()
        torch.cuda.synchronize()
        _INDEPENDENT = _capi.query("lotus_stream_probe", side_stream().cuda_stream, torch.cuda.current_stream().cuda_stream, 30)
    assert _INDEPENDENT == 1, f"lotus_stream_probe(side, current) = {_INDEPENDENT}: a parked side stream holds the critical stream"


def stall_ms_for(backward_ms):
    """Twice the time of the whole unstalled backward pass (every node's critical-stream work is shorter), within
    [FLOOR_MS, CAP_MS]: never mistaken for a hang, every test stays in the seconds."""
    return min(max(2.0 * backward_ms, FLOOR_MS), CAP_MS)


class Stall:
    """with Stall(join, ms) as st: loss.backward()   then, after torch.cuda.synchronize(), st.check().

    Wraps (for the duration of the block) the fork points ops._OnSide.__enter__ (per launch) and ops._side_ctx (composite) and
    the join points ops.sync_side_stream ("node") / ops._end_of_backward ("end").  Per node: [sleep, event `parked`] on the side
    stream in front of the first fork; event `reached` on the current stream in front of the join."""

    def __init__(self, join, ms):
        assert join in ("node", "end") and FLOOR_MS <= ms <= CAP_MS, (join, ms)
        self.join, self.ms = join, ms
        self.cycles = int(ms * cycles_per_ms())
        self.pending = None      # `parked` event of the node (pass) being enqueued
        self.done = False        # "end": the single stall has been placed
        self.pairs = []          # (reached, parked, started) per joined node
        self.unjoined = 0

    # -- the stall itself
    def _park(self):
        side = side_stream()
        started, parked = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            started.record()
            torch.cuda._sleep(self.cycles)
            parked.record()
        self.pending = (parked, started)

    def _fork(self):
        if self.ops._side() is None:
            return
        if self.join == "node":
            if self.pending is None:
                self._park()
        elif not self.done:
            self.done = True
            self._park()

    def _reached(self):
        if self.pending is not None:
            reached = torch.cuda.Event(enable_timing=True)
            reached.record()
            self.pairs.append((reached,) + self.pending)
            self.pending = None

    def __enter__(self):
        assert_streams_independent()
        ops, _ = _mods()
        self.ops = ops
        assert ops._JOIN == self.join and ops._SIDE_ON, (ops._JOIN, ops._SIDE_ON)
        self.orig = (ops._OnSide.__enter__, ops._side_ctx, ops.sync_side_stream, ops._end_of_backward)
        o_enter, o_ctx, o_sync, o_end = self.orig
        st = self

        def enter(onside):
            st._fork()
            return o_enter(onside)

        def side_ctx(*a, **k):
            st._fork()
            return o_ctx(*a, **k)

        def sync(target=None):
            if st.join == "node" and target is None:
                st._reached()
            return o_sync(target)

        def end_of_backward():
            st._reached()
            return o_end()

        ops._OnSide.__enter__, ops._side_ctx, ops.sync_side_stream, ops._end_of_backward = enter, side_ctx, sync, end_of_backward
        return self

    def __exit__(self, *a):
        ops = self.ops
        ops._OnSide.__enter__, ops._side_ctx, ops.sync_side_stream, ops._end_of_backward = self.orig
        if self.pending is not None:   # a fork whose join never came inside the block (an exception, normally)
            self.unjoined += 1
            self.pending = None

    @property
    def nodes(self):
        return len(self.pairs)

    def check(self):
        """After torch.cuda.synchronize(): every stalled node's critical-stream work was done while the side stream was
        still parked, and no stall outlasted the cap by more than scheduling noise.  -> the longest stall in ms."""
        assert self.unjoined == 0, f"{self.unjoined} stalled fork(s) without a join"
        assert self.pairs, "stall ineffective: no node forked to the side stream"
        longest = 0.0
        for i, (reached, parked, started) in enumerate(self.pairs):
            lead = reached.elapsed_time(parked)   # >= 0: the critical stream stood at the join before the sleep ended
            assert lead >= 0.0, f"stall ineffective: node {i} of {len(self.pairs)} reached its join {-lead:.3f} ms after the " \
                                f"side stream was released (stall {self.ms:.2f} ms)"
            longest = max(longest, started.elapsed_time(parked))
        return longest


def run_modes(run, join):
    """run(backward) builds its inputs, runs forward, calls backward(fn) with fn = the closure that runs the backward pass,
    synchronises and returns the list of tensors to compare.  -> (reference, stalled, Stall): the reference with the side
    stream off (one stream: nothing to race), the subject with the side stream on and stalled in join mode `join`; in
    between, one unstalled run with the side stream on, timed, that sizes the stall.  The allocator starts empty each time."""
    ops, _ = _mods()
    box = {}

    def plain(fn):
        fn()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        box["t"] = (e0, e1)

    def stalled(fn):
        with Stall(join, box["ms"]) as st:
            box["st"] = st
            fn()

    try:
        ops.enable_side_stream(False)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        ref = run(plain)
        ops.enable_side_stream(True)
        ops.set_wgrad_join(join)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        run(timed)
        torch.cuda.synchronize()
        box["ms"] = stall_ms_for(box["t"][0].elapsed_time(box["t"][1]))
        torch.cuda.empty_cache()
        got = run(stalled)
        torch.cuda.synchronize()
    finally:
        ops.enable_side_stream(True)
        ops.set_wgrad_join("node")
    st = box["st"]
    longest = st.check()
    assert longest <= CAP_MS * 1.2 + 1.0, f"a stall took {longest:.1f} ms"
    return ref, got, st


def assert_same(ref, got, names=None, rel=None):
    """torch.equal on every pair (or |a - b| <= rel * max(1, max|a|) where the two paths sum in another order); reports every
    output that differs and by how much."""
    assert len(ref) == len(got), (len(ref), len(got))
    bad = []
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape, (i, a.shape, b.shape)
        err = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
        ok = torch.equal(a, b) if rel is None else err <= rel * max(1.0, float(a.abs().max()))
        if not ok:
            bad.append((names[i] if names else i, err, float(a.abs().max())))
    assert not bad, "differs from the one-stream run (output, max |diff|, max |ref|): " + ", ".join(
        f"{n}: {e:.3e} / {s:.3e}" for n, e, s in bad)
