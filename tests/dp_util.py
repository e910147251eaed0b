"""Test-only: toy nets and checks for parallel.GradReducer's slab arena (ops.GRAD_ARENA -> GradReducer._arena).

The arena hands a backward node its place in the reducer's flat buffer as the node's `dw | db` output slab.  It matches a
request by position and size only, so what needs testing is a step whose nodes run in another order than the learnt one, or
skip a node — with gradients compared PER PARAMETER, bit for bit, against the same net without a reducer.

kind "cpu": `SlabLinear`, a pure-torch autograd node whose backward takes its slab from ops._grad_slab exactly as
ops.linear_wgrad does (the arena is a host-side mechanism: no device needed); kind "hip": ops.LinearFn."""
import torch


def _ops():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import ops

    return ops


def _parallel():
    import robot_3dlotus_amd  # noqa: F401
    from robot_3dlotus_amd import parallel

    return parallel


class SlabLinear(torch.autograd.Function):
    """y = x w^T + b; backward writes dw | db into ONE slab of N*K + N floats from ops._grad_slab (ops.linear_wgrad's layout)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return x @ w.t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, K = w.shape
        buf = _ops()._grad_slab(N * K + N, dy.device)
        dw, db = buf[:N * K].view(N, K), buf[N * K:]
        torch.mm(dy.t(), x, out=dw)
        torch.sum(dy, 0, out=db)
        return dy @ w, dw, db


def linear(kind, x, w, b):
    assert kind in ("cpu", "hip"), kind
    return SlabLinear.apply(x, w, b) if kind == "cpu" else _ops().LinearFn.apply(x, w, b)


class Lin(torch.nn.Module):
    def __init__(self, kind, k, n, g):
        super().__init__()
        self.kind = kind
        self.weight = torch.nn.Parameter(torch.randn(n, k, generator=g) / k ** 0.5)
        self.bias = torch.nn.Parameter(0.1 * torch.randn(n, generator=g))

    def forward(self, x):
        return linear(self.kind, x, self.weight, self.bias)


# one nonlinearity per branch: with the same one, two equal-sized branches over one input would have gradients that differ
# only through their weights' effect on y — and with equal weights not at all: a swap would be invisible
_NONLIN = (torch.tanh, torch.sin, torch.sigmoid, torch.cos, torch.atan, torch.exp)


class Branches(torch.nn.Module):
    """`len(sizes)` parallel branches Lin(width -> sizes[i]) over one input; loss = sum(scale^2) * sum_i mean(f_i(branch_i(x))),
    the branches CREATED in the order given to forward() (backward runs them in the reverse of it).  `scale` is a 3-float
    parameter: its gradient arrives first, an odd unit in front of every slab."""

    def __init__(self, kind, sizes, width, seed=0):
        super().__init__()
        self.args = (kind, tuple(sizes), width, seed)
        g = torch.Generator().manual_seed(seed)
        assert len(sizes) <= len(_NONLIN)
        self.br = torch.nn.ModuleList([Lin(kind, width, n, g) for n in sizes])
        self.scale = torch.nn.Parameter(1.0 + 0.1 * torch.randn(3, generator=g))

    def forward(self, x, order):
        total = None
        for i in order:
            t = _NONLIN[i](self.br[i](x)).mean()
            total = t if total is None else total + t
        return self.scale.square().sum() * total


class Chain(torch.nn.Module):
    """a -> [b] -> c, Lin(width -> mid), Lin(mid -> mid), Lin(mid -> width) (mid = width: three equal slabs), and an optional
    auxiliary head Lin(mid -> aux) on a's output.  forward(x, use_b, use_aux=False) -> loss."""

    def __init__(self, kind, width, mid=None, aux=0, seed=0):
        super().__init__()
        self.args = (kind, width, mid, aux, seed)
        mid = width if mid is None else mid
        g = torch.Generator().manual_seed(seed)
        self.a, self.b, self.c = Lin(kind, width, mid, g), Lin(kind, mid, mid, g), Lin(kind, mid, width, g)
        self.aux = Lin(kind, mid, aux, g) if aux else None

    def forward(self, x, use_b, use_aux=False):
        h = torch.tanh(self.a(x))
        loss = torch.sigmoid(self.aux(h)).mean() if use_aux else 0.0
        if use_b:
            h = torch.sin(self.b(h))
        return self.c(h).square().mean() + loss


def twin(net):
    """The same net (same class, arguments, parameter values, device) with no reducer hooks on its parameters."""
    t = type(net)(*net.args)
    t.load_state_dict(net.state_dict())
    return t.to(next(net.parameters()).device)


def plain_grads(net, *args):
    """{name: gradient or None} of net(*args) computed by a twin of `net` with no reducer and no arena."""
    return plain_grads_accum(net, [args])


def plain_grads_accum(net, calls):
    """plain_grads over several micro-batches: one backward per entry of `calls`, accumulated by autograd."""
    ops = _ops()
    t = twin(net)
    arena, ops.GRAD_ARENA = ops.GRAD_ARENA, None
    try:
        for args in calls:
            t(*args).backward()
    finally:
        ops.GRAD_ARENA = arena
    if next(t.parameters()).is_cuda:
        torch.cuda.synchronize()
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in t.named_parameters()}


def check_step(red, net, want):
    """After red.finish(): per parameter, by name — a used one has `.grad` and its slice of the flat buffer BIT-equal to
    want[name]; an unused one has `.grad is None` and, where collectives ran (every bucket is flushed then), an all-zero slice;
    the usage mask says which is which.  -> number of tensors compared."""
    if red.flat.is_cuda:
        torch.cuda.synchronize()
    collectives = red.world > 1 or red._force
    bad, n = [], 0
    for name, p in net.named_parameters():
        w = want[name]
        if w is not None:
            n += 1
            if p.grad is None or not torch.equal(p.grad, w) or not torch.equal(red.view_of(p), w):
                bad.append((name, "no gradient" if p.grad is None else float((p.grad - w).abs().max()),
                            float((red.view_of(p) - w).abs().max())))
        else:
            if p.grad is not None:
                bad.append((name, "unused, but .grad is set"))
            if collectives and bool(red.view_of(p).ne(0).any()):
                bad.append((name, "unused, but its slot is not zero"))
    assert not bad, f"(parameter, max |.grad - plain|, max |view_of - plain|): {bad}"
    if collectives:
        index = {p: i for i, p in enumerate(red.params)}
        mask = red.used_mask.tolist()
        assert all(mask[index[p]] == (0 if want[name] is None else 1) for name, p in net.named_parameters()), (mask, want.keys())
    return n


class ArenaLog:
    """Wraps red._arena: records every slab served out of the flat buffer as (offset in floats, floats) and asserts its
    256-byte alignment BEFORE the node gets it — a misaligned slab ends the step as a Python exception in front of the launch."""

    def __init__(self, red):
        ops = _ops()
        self.red, self.inner, self.served = red, red._arena, []
        red._arena = self
        if getattr(ops.GRAD_ARENA, "__self__", None) is red:
            ops.GRAD_ARENA = self

    def __call__(self, n, dev):
        t = self.inner(n, dev)
        flat = self.red.flat
        if t is not None and flat.data_ptr() <= t.data_ptr() < flat.data_ptr() + 4 * flat.numel():
            assert t.data_ptr() % 256 == 0, f"slab of {n} floats served at byte {t.data_ptr() - flat.data_ptr()} of the flat " \
                                            f"buffer (base % 256 = {flat.data_ptr() % 256}): not 256-byte aligned"
            self.served.append(((t.data_ptr() - flat.data_ptr()) // 4, n))
        return t

    def take(self):
        s, self.served = self.served, []
        return s


def mb(floats):
    """bucket_mb that gives GradReducer a cap of exactly `floats` elements."""
    return (floats + 0.5) * 4 / (1 << 20)


def host_reducer(net, bucket_mb, **kw):
    """A reducer over host tensors WITH the slab arena (off by default there: no HIP node asks for slabs on the host)."""
    parallel = _parallel()

    class HostArenaReducer(parallel.GradReducer):
        arena_on_host = True

    red = HostArenaReducer(net, bucket_mb=bucket_mb, **kw)
    red._arena_off = False
    return red


def run_step(red, net, args, want=None, zero="first"):
    """One step of the reducer's protocol, zero_grad() in front ("first") or behind ("last", a trainer that clears after its
    optimiser step); with `want`, check_step in between.  -> (floats born in place, floats copied, tensors compared) of this step."""
    i0, c0 = red.inplace_floats, red.copied_floats
    if zero == "first":
        red.zero_grad()
    net(*args).backward()
    red.finish()
    n = check_step(red, net, want) if want is not None else 0
    if zero == "last":
        red.zero_grad()
    return red.inplace_floats - i0, red.copied_floats - c0, n
