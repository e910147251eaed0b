"""Autograd operators over the C-ABI (csrc/liblotus_hip.so).

One `torch.autograd.Function` per sub-block of the reference model, each with a hand-written
backward that chains the HIP kernels (fused epilogues, no temporaries beyond what backward needs):

  CpeFn        x + LN(Linear(SubMConv3d(xs)))                      Block.cpe    model.py:615-625,660-662
  SelfAttnFn   x + proj(patch_attention(qkv(LN(x))))               Block.attn   model.py:664-667,468-557
  FfnFn        x + fc2(GELU(fc1(LN(x))))                           Block.mlp / CABlock.mlp
  CrossAttnFn  x + proj(cross_attention(q(LN(x)), kv(context)))    CABlock.attn model_ca.py:135-140
  CrossAttnKvFn  ... with kv a slice of the ProjBank               (the default: kv_group)
  ProjAllFn    Linear_j(context) / Linear_j(SiLU(context)), all j  the kv of every CABlock / the modulation of every PDNorm
  StemFn / PoolFn / UnpoolFn                                       Embedding, SerializedPooling, SerializedUnpooling
  HeadLossFn / RegHeadLossFn                                       ActionHead+loss: published / with heatmap_mlp positions
                                                                   and / or euler / quat rotations (csrc/reg_head.hip)
The per-launch bodies are functions shared by the nodes that run them: cpe_ / selfattn_ / ffn_ / crossattn_branch_fwd / _bwd,
head_trunk_fwd / _bwd, cloud_max_fwd.
PyTorch provides device memory, the stream and the autograd graph; all arithmetic is in the kernels.
"""
import collections
import ctypes
import os

import torch

from . import _capi
from ._capi import call, query, WS

ACT_NONE, ACT_GELU, ACT_LEAKY = 0, 1, 2
BN_EPS, BN_MOMENTUM = 1e-3, 0.01
CALL_LOG = None  # bench.py sets this to a list to record the (kind, M, N, K) of every dense launch
EVENT_LOG = None  # ... and this to a list to get (kind, M, N, K, start event, end event) of every dense launch, recorded on
                  # the stream the launch went to (the timed quantities of bench.py's in-step roofline figure)


DenseRoute = collections.namedtuple("DenseRoute", "family bm bn bk nz fast fused depth")
FAMILY_GEMM, FAMILY_GEMM_DMA, FAMILY_GEMM_DMA_TAP = 1, 2, 3


def last_dense_route():
    """The kernel this thread's last dense product was given to (lotus_dense_last_route): family 1 gemm_kernel, 2
    gemm_dma_kernel, 3 gemm_dma_tap_kernel; block tile; split count; FAST or guarded form; fused split-K; staging-ring depth
    (family 1) or LDS stages.  Set when the launch is chosen, so it is there after a launch that failed, too."""
    out = (ctypes.c_int * 8)()
    _capi.call_raw("lotus_dense_last_route", ctypes.addressof(out))
    return DenseRoute(*out)


ConvRoute = collections.namedtuple("ConvRoute", "family mode rows cols prec nz tpz aux")
(CONV_GENERIC, CONV_STEM, CONV_PAIRS, CONV_OS, CONV_TAP, CONV_WGRAD, CONV_WGRAD_BF16, CONV_WGRAD_STEM) = range(1, 9)


def last_conv_route():
    """The kernel this thread's last convolution launch was given to (lotus_conv_last_route; fields in include/lotus_hip.h):
    family 1 generic, 2 thin-input stem, 3 pair-compacted, 4 output-stationary, 5 tap-grouped, 6 / 7 / 8 weight gradient
    (fp32, bf16 operands, thin-input stem); mode 0 fwd / 1 dgrad / 2 wgrad; block tile; operand precision; tap groups (or row
    splits) and taps (rows) per group; aux.  Set when the kernel is chosen, so it is there after a launch that failed, too."""
    out = (ctypes.c_int * 8)()
    _capi.call_raw("lotus_conv_last_route", ctypes.addressof(out))
    return ConvRoute(*out)


AttnRoute = collections.namedtuple("AttnRoute", "family direction targ precision norm threads lds_bytes tail")
ATTN_FWD, ATTN_BWD, ATTN_BWD2, ATTN_XQ, ATTN_XQ2 = range(1, 6)
ATTN_RPE_FWD, ATTN_RPE_BWD = 6, 7  # lotus_attention_rpe_fwd / _bwd (csrc/attn_route.h)
ATTN_LONG_FWD, ATTN_LONG_BWD = 8, 9  # lotus_attention_long_fwd / _bwd: tiles above 128 rows (csrc/attn_route.h)
ATTN_LONG_MAX = 1024  # LOTUS_ATTN_LONG_MAX (include/lotus_hip.h): the longest tile the long kernels take


def last_attn_route():
    """The kernel this thread's last attention launch was given to (lotus_attention_last_route; fields in include/lotus_hip.h):
    family 1 tile forward, 2 tile backward on bf16 / bf16x3 operands, 3 tile backward in fp32, 4 / 5 one lane per query (keys in
    LDS / in registers), 6 / 7 tile forward / backward with the relative-position term, 8 / 9 forward / backward over tiles above
    128 rows (key images walked with an online softmax); direction 0 fwd / 1 bwd; template argument; operand precision; with the q/k norm; threads; dynamic LDS
    bytes; tail (bit 0 fix-up, bit 1 norm-gradient reduction, bit 2 table-gradient merge follow).  Set when the kernel is chosen, so it is there after a
    launch that failed, too."""
    out = (ctypes.c_int * 8)()
    _capi.call_raw("lotus_attention_last_route", ctypes.addressof(out))
    return AttnRoute(*out)


class _Timed:
    """Bracket a dense launch with HIP events on the stream it is enqueued on (diagnostic; only when EVENT_LOG is set)."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        if EVENT_LOG is None:
            return self
        # inside a weight-gradient block the launches go to the side stream although torch's current stream is unchanged
        self.st = _SIDES[_CUR][0] if _capi.STREAM_OVERRIDE else torch.cuda.current_stream()
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e0.record(self.st)
        return self

    def __exit__(self, *a):
        if EVENT_LOG is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(self.st)
            EVENT_LOG.append(self.key + (self.e0, e1))


# Weight gradients are off the critical path of backward (nothing downstream consumes them before the
# optimiser / gradient all-reduce) and their kernels are latency-bound streams over dy and x, while the
# dgrad chain is MFMA-bound: running them on a second HIP stream lets the two overlap on the CUs.
# Fork/join per autograd node: the side stream waits for the main stream before each weight-gradient launch
# and every backward() ends with the main stream waiting for the side stream (`_joined`), so whatever
# consumes the returned gradients (accumulation, the GradReducer hooks, the optimiser) is ordered after them.
# On by default; LOTUS_SIDE_STREAM=0 (or enable_side_stream(False)) keeps everything on one stream.
#
# set_wgrad_join("end") defers the join to ONE wait at the end of the backward pass (an autograd engine
# callback): the weight-gradient kernels of a node may then still be running while the main stream is
# several nodes further down the dgrad chain.  Valid when nothing reads a parameter gradient during
# backward — i.e. `.grad is None` on entry (zero_grad(set_to_none=True): autograd adopts the tensor without
# touching it) and no per-parameter hooks; the GradReducer (hooks) and gradient accumulation need the
# default "node".
#
# In BOTH modes the tensors the side stream reads are held until the join that orders the main stream behind it, so the
# caching allocator (which knows of no use on another stream) cannot hand their memory to the main stream early: "node" keeps
# them in the node's own list (_NODE_HELD, dropped by `_joined` right behind its join — a body such as ffn_branch_bwd frees its
# temporaries when it returns, and the node goes on allocating after that), "end" in _HELD until the end-of-backward join
# (_hold_for_side).
SIDE = None
_SIDE_ON = os.environ.get("LOTUS_SIDE_STREAM", "1") != "0"
_STEM_WGRAD_MAIN = True  # the last weight gradient of a backward pass runs on the critical stream, idle by then (+0.45 %)
_JOIN = "node"
_END_CB_PENDING = False


_PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 3}
_M64 = (1 << 64) - 1


def mix_seed(seed, k=0):
    """splitmix64 finaliser of (seed, k): a well-mixed 64-bit sub-seed.  The device mask hash adds the low word of the
    seed to index * odd constant and XORs the high word in before its own finaliser (csrc/common.h lotus_hash32), so seeds
    that differ by small integers would give index-shifted copies of one stream; every dropout site therefore gets
    its seed through this function (layer, use site, step and rank all enter as `k` of a nested call)."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def dist_rank():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(os.environ.get("RANK", "0"))


def _env_precision():
    v = os.environ.get("LOTUS_GEMM_PREC", "0")
    return int(v) if v in ("1", "3") else 0


_PREC = _env_precision()  # precision code the next forward pass captures (see set_gemm_precision / precision())


class storage:
    """Context manager: activation STORAGE type of the forward passes started inside.  torch.float32 (default) runs the
    lotus_* entry points; torch.bfloat16 runs their bf16-storage twins (lotus_b16_*, include/lotus_hip_b16.h): every
    activation tensor in HBM is bf16, parameters / parameter gradients / statistics / accumulation stay fp32 — the
    "bf16 activations, fp32 master weights" mode of BASELINE configs[4].  The operand precision inside is 'bf16'
    (one bf16 MFMA product, fp32 accumulate).  Like the precision, the storage type is captured per autograd node and
    replayed in its backward, so models of both kinds coexist in one process."""

    def __init__(self, dtype, shadows=False):
        assert dtype in (None, torch.float32, torch.bfloat16), dtype
        self.bf = dtype is torch.bfloat16
        # shadows: the dense layers read bf16 SHADOWS of their weights (WeightShadows) where a parameter carries one —
        # precision code 5 of the lotus_b16_linear_* entry points; master weights, gradients and the optimiser stay fp32
        self.code = 5 if (self.bf and shadows) else 1

    def __enter__(self):
        global _PREC
        self.prev = (_capi.BF16, _PREC)
        _capi.BF16 = self.bf
        if self.bf:
            _PREC = self.code
        return self

    def __exit__(self, *a):
        global _PREC
        _capi.BF16, _PREC = self.prev


def set_gemm_precision(mode):
    """Default operand precision of the dense, sparse-convolution and attention products for forward passes started
    from now on: 'fp32' = fp32 MFMA, exact products (default, the 1e-4 logit parity mode); 'bf16x3' = split-bf16 products
    hi*hi + hi*lo + lo*hi with fp32 accumulation (~2^-17 per product; measured max logit error 2.2e-5, +23-27 % step
    throughput); 'bf16' = bf16 operands (the bf16 compute mode of BASELINE configs[4]; +20-35 %).

    Host-side only: the precision is an argument of every C-ABI call (no state in the library).  Each autograd node
    captures it in forward and replays it in backward, and a model with a `gemm_precision` attribute overrides this
    default for its own forward passes (`with ops.precision(mode)`), so models of different precisions coexist."""
    global _PREC
    _PREC = _PRECISIONS[mode]


def get_gemm_precision():
    return {v_: k for k, v_ in _PRECISIONS.items()}[_PREC]


class precision:
    """Context manager: operand precision of the forward passes started inside (None = leave the default)."""

    def __init__(self, mode):
        self.code = None if mode is None else _PRECISIONS[mode]

    def __enter__(self):
        global _PREC
        self.prev = _PREC
        if self.code is not None:
            _PREC = self.code
        return self

    def __exit__(self, *a):
        global _PREC
        _PREC = self.prev


def set_wgrad_join(mode):
    global _JOIN
    assert mode in ("node", "end")
    sync_side_stream()
    _JOIN = mode


def enable_side_stream(on=True):
    global SIDE, _SIDE_ON
    _SIDE_ON = bool(on)
    if not on:
        sync_side_stream()
        SIDE = None
        _SIDES.clear()


_IN_NODE = 0  # > 0 while a `_joined` backward is running: only then is the join guaranteed


_NSIDE = 1     # one weight-gradient stream: a second one measured 766 vs 796 samples/s (round 1), 880 vs 930 (round 4)
_SIDES = []     # [(torch.cuda.Stream, hipStream_t)]: weight-gradient producers go round-robin over these
_RR = 0         # next side stream
_CUR = 0        # side stream of the _OnSide block being executed
_LINK = 0       # lotus_streamlink handle (event ring) used for every fork / join


def _side():
    global SIDE, _LINK
    if not _SIDE_ON or _IN_NODE == 0:
        return None
    if SIDE is None:
        # measured and not kept: more than one side stream (766 vs 796 samples/s), CU-masked side streams (side stream on 7/8,
        # 3/4 or 31/32 of the CUs: 923-931 / 929-932 / 875-879 against 930: reserving CUs for the critical stream buys
        # nothing), a lowest-priority side stream (+0.1 %)
        for _ in range(_NSIDE):
            st = _capi.step_stream("side") if not _SIDES else torch.cuda.Stream(priority=_capi.STREAM_PRIORITY)
            _SIDES.append((st, st.cuda_stream))
        if not _LINK:
            _LINK = query("lotus_streamlink_create", 256)
            if not _LINK:
                raise _capi.LotusError("lotus_streamlink_create failed: " + _capi.lib().last_error())
        SIDE = _SIDES[0][0]
    return SIDE


def sync_side_stream(target=None):
    """The current stream (or the stream with raw handle `target`) waits for everything enqueued on the
    weight-gradient stream(s)."""
    if SIDE is not None:
        cur = _capi.stream_ptr() if target is None else target
        for _, ptr in _SIDES:
            _capi.call_raw("lotus_streamlink_wait", _LINK, ptr, cur)


def _side_ws(nbytes, dev):
    """Workspace of the side-stream producer being enqueued (one per side stream); (re)allocated under that stream
    so the caching allocator orders its reuse after the stream's work."""
    slot = 16 + _CUR
    b = WS.buf.get((dev, slot))
    if b is None or b.numel() < nbytes:
        with torch.cuda.stream(_SIDES[_CUR][0]):
            b = WS.get(nbytes, dev, slot=slot)
    return b


class _OnSide:
    """Run a weight-gradient producer on a side stream after the main stream's pending work.  Outputs are
    allocated by the caller on the main stream (they stay alive until after the join); `reads` are the tensors
    the side-stream kernels consume, kept alive from here until the join.  Inside the block every ops.call() enqueues on the side stream
    (_capi.STREAM_OVERRIDE); torch's current stream is left alone — nothing in these blocks launches ATen kernels —
    and the fork is one event record + stream wait through the C-ABI stream link."""

    def __init__(self, *reads):
        self.reads = reads

    def __enter__(self):
        global _RR, _CUR
        self.on = _side() is not None
        if not self.on:
            return self
        _CUR = _RR
        _RR = (_RR + 1) % _NSIDE
        side, ptr = _SIDES[_CUR]
        _capi.call_raw("lotus_streamlink_wait", _LINK, _capi.stream_ptr(), ptr)
        # until the join the memory must not go back to the main stream, whatever the caller does with its own references
        if _JOIN == "end":
            _hold_for_side(self.reads, side)
        elif _NODE_HELD is not None:
            _NODE_HELD.append(self.reads)
        _capi.STREAM_OVERRIDE = ptr
        return self

    def __exit__(self, *a):
        if self.on:
            _capi.STREAM_OVERRIDE = 0


_HELD = []  # tensors the weight-gradient stream reads, kept alive until the end-of-backward join (deferred-join mode)
# "node" mode: the `reads` of every fork of the `_joined` node being run, dropped behind its join; None outside such a node
# (the weight packing in forward forks too: it reads parameters only, and its caller joins)
_NODE_HELD = None


def _hold_for_side(reads, side):
    """Deferred-join mode: what the side stream reads must not be recycled by the main stream before the join.  Inside a
    backward pass (the end-of-backward callback is queued) the tensors are simply HELD until that join — `record_stream` would
    make the caching allocator answer every one of them with an event record on the side stream the moment autograd releases
    it: ~300 marker packets of ~5 us per step in between the weight-gradient kernels.  Outside a backward pass (weight packing in
    forward) there is no join to wait for: record_stream."""
    if _END_CB_PENDING:
        _HELD.extend(t for t in reads if t is not None)
    else:
        for t in reads:
            if t is not None:
                t.record_stream(side)


def _end_of_backward():
    global _END_CB_PENDING
    _END_CB_PENDING = False
    sync_side_stream()
    _HELD.clear()  # (freed behind the join: whatever re-uses the memory is enqueued after it)


def _abandoned_backward():
    """A forward pass starts while the end-of-backward callback of an earlier backward pass is still pending: that pass raised (the
    autograd engine drops its queued callbacks then — e.g. an out-of-memory error the trainer catches and skips).  Join the side
    stream and release what was held for it, or every later backward would append to _HELD for good and never join again
    (ADVICE r5)."""
    global _END_CB_PENDING
    _END_CB_PENDING = False
    sync_side_stream()
    _HELD.clear()


def _fwd(fn):
    """forward() decorator: the node remembers the operand precision it was computed in."""
    def wrapped(ctx, *args):
        if _END_CB_PENDING and _IN_NODE == 0:
            _abandoned_backward()
        ctx.prec, ctx.bf = _PREC, _capi.BF16
        return fn(ctx, *args)
    return staticmethod(wrapped)


def _joined(fn):
    """backward() decorator: join the side stream before the gradients leave the node ("node"), or once at the
    end of the backward pass ("end"); the node's products run in the precision its forward captured.  "node": what the node's
    forks read (_NODE_HELD) is released behind the join, also when the node raises."""
    def wrapped(ctx, *grads):
        global _IN_NODE, _END_CB_PENDING, _PREC, _NODE_HELD
        _IN_NODE += 1
        prev, _PREC = _PREC, getattr(ctx, "prec", _PREC)
        prev_bf, _capi.BF16 = _capi.BF16, getattr(ctx, "bf", _capi.BF16)
        outer, _NODE_HELD = _NODE_HELD, ([] if _JOIN == "node" else None)
        try:
            if _JOIN == "end" and _SIDE_ON and not _END_CB_PENDING:
                _END_CB_PENDING = True
                torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)
            return fn(ctx, *grads)
        finally:
            _PREC = prev
            _capi.BF16 = prev_bf
            _IN_NODE -= 1
            try:
                if _JOIN == "node":
                    sync_side_stream()
            finally:
                _NODE_HELD = outer  # (freed behind the join: whatever re-uses the memory is enqueued after it)
    return staticmethod(wrapped)


def _ws(nbytes, dev):
    return WS.get(nbytes, dev, slot=0)


_COUNTERS = {}


def _counters(dev):
    """Zeroed arrival counters of the fused split-K products, one buffer per stream that launches them (the kernels
    leave them zero)."""
    return _counters_for(dev, _capi.STREAM_OVERRIDE or _capi.stream_ptr())


def _counters_for(dev, ptr):
    """The counter buffer of the stream with raw handle `ptr`.  First use: the zero-fill is enqueued ON that stream (a
    fill on torch's current stream would not be ordered before a side-stream launch whose fork event was already
    recorded: a counter that starts non-zero never reaches gridDim.z - 1 and the tile is never written)."""
    key = (dev, ptr)
    c = _COUNTERS.get(key)
    if c is None:
        owner = next((st for st, sp in _SIDES if sp == ptr), None)
        if owner is not None and ptr != _capi.stream_ptr():
            with torch.cuda.stream(owner):
                c = torch.zeros(query("lotus_splitk_counters_bytes"), dtype=torch.uint8, device=dev)
        else:
            c = torch.zeros(query("lotus_splitk_counters_bytes"), dtype=torch.uint8, device=dev)
        _COUNTERS[key] = c
    return c


def _pa(prec=None):
    """Operand precision for the attention / convolution entry points (and for dense layers given fp32 master weights):
    the shadow flag (5) only concerns the weight pointer of lotus_linear_fwd / _dgrad."""
    code = _PREC if prec is None else prec
    return 1 if code == 5 else code


def _wk(*ws):
    """-> (weights to hand to the kernels, precision code): in shadow mode (precision 5) and when EVERY given parameter
    carries a bf16 shadow (WeightShadows), the shadows and 5; else the fp32 masters and the plain code."""
    if _PREC == 5:
        sh = [getattr(w, "_lotus_b16", None) for w in ws]
        if all(t is not None for t in sh):
            return sh, 5
    return list(ws), _pa()


class WeightShadows:
    """bf16 shadows of a model's dense-layer weights: BASELINE configs[4] stores "bf16 activations / weights with fp32 master
    weights" (job_scripts/train_3dlotus_policy_peract.sh:42-44,61).  The fp32 Parameter stays what autograd, the optimiser
    and the checkpoint see; `p._lotus_b16` is what the bf16-storage products read.  The fused AdamW (optim.AdamW) rewrites
    the shadow in the launch that updates the master; any other in-place change of a master (another optimiser,
    load_state_dict, .copy_) bumps the tensor's version counter and refresh() recasts — one multi-tensor launch."""

    def __init__(self, params):
        self.params = [p for p in params if p.dtype == torch.float32 and p.numel() % 4 == 0]
        self.tables = None

    def invalidate(self):
        """Force the next refresh() to recast every shadow: for code that rewrites masters behind the version counter
        (`p.data.copy_()`, `p.data = ...`, a parameter swap, another raw-pointer kernel) — ADVICE r4."""
        for p in self.params:
            p._lotus_b16_ver = -1

    def refresh(self):
        stale = False
        for p in self.params:
            sh = getattr(p, "_lotus_b16", None)
            if sh is None or sh.device != p.device or sh.shape != p.shape:
                p._lotus_b16 = torch.empty(p.shape, dtype=torch.bfloat16, device=p.device)
                p._lotus_b16_ver = -1
                self.tables = None
            # a shadow is current for (version counter, storage address): `p.data = other` keeps the version but moves the storage
            if p._lotus_b16_ver != p._version or getattr(p, "_lotus_b16_ptr", None) != p.data_ptr():
                stale = True
        if not stale:
            return
        dev = self.params[0].device
        key = tuple(p.data_ptr() for p in self.params)
        if self.tables is None or self.tables[0] != key:
            import numpy as np
            chunk = query("lotus_mt_chunk")
            numel = [p.numel() for p in self.params]
            ch = [(t, c) for t, n in enumerate(numel) for c in range((n + chunk - 1) // chunk)]
            i64 = lambda v: torch.tensor(v, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)  # noqa: E731
            self.tables = (key, i64(list(key)), i64([p._lotus_b16.data_ptr() for p in self.params]), i64(numel),
                           torch.from_numpy(np.asarray(ch, dtype=np.int32)).pin_memory().to(dev, non_blocking=True), len(ch))
        _, src, dst, numel, chunks, nch = self.tables
        call("lotus_shadow_cast", src, dst, numel, chunks, nch)
        for p in self.params:
            p._lotus_b16_ver = p._version
            p._lotus_b16_ptr = p.data_ptr()


# Weight-gradient slabs of a backward node (the flat fp32 buffer its parameter gradients are views of).  A data-parallel reducer
# can own that memory: GRAD_ARENA(n_floats, device) -> a slice of its bucket buffer (or None), so that the gradients are born where
# the all-reduce reads them and the bucket flush has nothing to pack (parallel.GradReducer._arena).
GRAD_ARENA = None


def _grad_slab(n, dev):
    if GRAD_ARENA is not None:
        t = GRAD_ARENA(int(n), dev)
        if t is not None:
            return t
    return torch.empty(int(n), dtype=torch.float32, device=dev)


def _empty_like_rows(x, cols):
    return torch.empty(x.shape[0], cols, dtype=x.dtype, device=x.device)


# ------------------------------------------------------------------------------------ primitives
def _wprec(w, prec=None):
    """Precision code of a dense product from the weight tensor it is given: a bf16 weight IS a shadow (code 5), an fp32
    weight never is — a wrong pairing would make the kernel misread the matrix."""
    if w.dtype == torch.bfloat16:
        assert _capi.BF16, "bf16 weight shadows belong to the bf16-storage mode"
        return 5
    return _pa(prec)


def linear_fwd(x, w, b, residual=None, act=ACT_NONE, save_pre=False, drop_p=0.0, seed=0, prec=None):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=x.dtype, device=x.device)
    pre = torch.empty_like(y) if save_pre else None
    if CALL_LOG is not None:
        CALL_LOG.append(("fwd", M, N, K))
    nb = query("lotus_linear_workspace", M, N, K) if M <= 8192 else 0
    ws = _ws(nb, x.device) if nb else None
    with _Timed(("fwd", M, N, K)):
        call("lotus_linear_fwd", x, w, b, residual, y, pre, M, N, K, act, float(drop_p), int(seed),
             _wprec(w, prec), ws, nb, _counters(x.device) if nb else None)
    return y, pre


def linear_dgrad(dy, w, pre=None, add=None, act=ACT_NONE, drop_p=0.0, seed=0, prec=None):
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, dtype=dy.dtype, device=dy.device)
    if CALL_LOG is not None:
        CALL_LOG.append(("dgrad", M, N, K))
    nb = query("lotus_linear_workspace", M, N, K) if M <= 8192 else 0
    ws = _ws(nb, dy.device) if nb else None
    with _Timed(("dgrad", M, N, K)):
        call("lotus_linear_dgrad", dy, w, dx, pre, add, M, N, K, act, float(drop_p), int(seed),
             _wprec(w, prec), ws, nb, _counters(dy.device) if nb else None)
    return dx


def linear_wgrad(dy, x, need_bias=True, prec=None, into=None):
    """dw = dy^T x, db = colsum(dy) on the weight-gradient stream.  `into` = (dw, db) of an earlier call: accumulate
    into them (ordered on that stream; adding the results on the main stream would race with the side stream)."""
    M, N = dy.shape
    K = x.shape[1]
    if into is None:
        buf = _grad_slab(N * K + (N if need_bias else 0), dy.device)
        dw = buf[:N * K].view(N, K)              # one contiguous gradient slab -> a single split-K reduce launch
        db = buf[N * K:] if need_bias else None
    else:
        dw, db = into
    if CALL_LOG is not None:
        CALL_LOG.append(("wgrad", M, N, K))
    nbytes = query("lotus_linear_wgrad_workspace", M, N, K)
    with _OnSide(dy, x):
        ws = _side_ws(nbytes, dy.device) if _side() is not None else WS.get(nbytes, dy.device, slot=0)
        with _Timed(("wgrad", M, N, K)):
            call("lotus_linear_wgrad", dy, x, dw, db, M, N, K, 0 if into is None else 1, _pa(prec), ws,
                 ws.numel(), _counters(dy.device))
    return dw, db


_ADA_WS_SLOT = 6  # workspace slot of the adaptive norms' (P, Q) partials (main stream)


def _n_clouds(lvl):
    return len(lvl.counts)


def ln_fwd(x, g, b, res=None, eps=1e-5, save=True, mod=None, lvl=None):
    """LN(x) g + b (+ res).  mod = [B, 2C] (row stride free) of [shift | scale], one row per cloud of `lvl`: the adaptive PDNorm
    (model.py:257-303), (LN(x) g + b) (1 + scale_b) + shift_b (+ res); None: the plain LayerNorm."""
    M, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if save else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if save else None
    if mod is None:
        call("lotus_layernorm_fwd", x, res, g, b, y, mean, rstd, M, C, float(eps))
    else:
        call("lotus_adaln_fwd", x, res, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), y, mean, rstd, M, C, float(eps))
    return y, mean, rstd


class Handoff:
    """Backward-pass hand-over between two consecutive sub-blocks of a stage.  Forward order: A -> B, where A ends
    with proj / fc2 dropout (p, seed).  B's backward finishes with a LayerNorm backward that produces dx — exactly the
    gradient A's backward receives, and the first thing A would do with it is dz = dropout_mask(p, seed) * dx in a kernel
    of its own.  B's LayerNorm backward writes dz as a second output instead and parks it here; A picks it up if the
    gradient it was handed is that very tensor (B was the only consumer of A's output)."""
    __slots__ = ("drop", "ptr", "dz")

    def __init__(self):
        self.drop, self.ptr, self.dz = None, 0, None

    def arm(self, p, seed):      # A.forward: this is the mask my backward will need
        self.drop, self.ptr, self.dz = ((float(p), int(seed)) if p > 0.0 else None), 0, None

    def take(self, dy):          # A.backward
        dz, self.dz = self.dz, None
        return dz if (dz is not None and self.ptr == dy.data_ptr() and dz.shape == dy.shape) else None

    @staticmethod
    def offer(hand, dx):         # B.backward -> (dz_out, p, seed) for the LayerNorm backward that writes dx
        if hand is None or hand.drop is None:
            return None, 0.0, 0
        dz = torch.empty_like(dx)
        hand.ptr, hand.dz = dx.data_ptr(), dz
        return (dz,) + hand.drop


def _masked(dy, p, seed, hand):
    """dz = dropout mask * dy for a backward pass: from the hand-over if the producer of dy left it, else a launch."""
    if hand is not None:
        dz = hand.take(dy)
        if dz is not None:
            return dz
    return dropout(dy, p, seed)


def ln_bwd(dy, x, mean, rstd, g, add=None, hand=None, b=None, mod=None, dmod=None, lvl=None):
    """-> dx (+ add), dgamma, dbeta.  With `mod` (see ln_fwd; needs b) d mod is written into `dmod` ([B, 2C] view) by the one
    adaptive launch, which takes no hand-over."""
    M, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    if mod is not None:
        B = _n_clouds(lvl)
        ws = WS.get(query("lotus_adanorm_workspace", M, B, C), x.device, slot=_ADA_WS_SLOT)
        call("lotus_adaln_bwd", dy, x, mean, rstd, g, b, mod, mod.stride(0), lvl.off, B, add, dx, dg, db, dmod, dmod.stride(0), M, C,
             ws, ws.numel())
        return dx, dg, db
    dz, dp, dseed = Handoff.offer(hand, dx)
    nbytes = query("lotus_layernorm_bwd_workspace", M, C)
    if _side() is None:
        ws = _ws(nbytes, x.device)
        call("lotus_layernorm_bwd", dy, x, mean, rstd, g, add, dx, dg, db, M, C, 0, dz, dp, dseed, ws, ws.numel())
        return dx, dg, db
    # dx on the main stream; the parameter-gradient reduction of the column partials (own workspace slot, joined
    # at the end of the node like every other weight gradient) on the side stream
    # ("end" join: the partials must outlive an unknown amount of main-stream progress -> a fresh buffer)
    ws = WS.get(nbytes, x.device, slot=4) if _JOIN == "node" else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    call("lotus_layernorm_bwd", dy, x, mean, rstd, g, add, dx, None, None, M, C, 0, dz, dp, dseed, ws, ws.numel())
    with _OnSide(ws):
        call("lotus_layernorm_bwd_params", ws, M, C, dg, db, 0)
    return dx, dg, db


def linear_dgrad_ln(dy, w, x, mean, rstd, g, add=None, drop=None):
    """dx = LN'(dy w; x, mean, rstd, g) + add, dz = dx * mask(drop = (p, seed)), dgamma, dbeta: the input gradient of a linear
    layer fused with the backward of the LayerNorm that feeds it (lotus_linear_dgrad_ln; one kernel where 128-wide tiles
    cover whole rows of many-row levels, the two launches otherwise).  Test / diagnostic entry: the model reaches it through
    the composite backward passes of csrc/blocks.cpp."""
    import numpy as np
    M, N = dy.shape
    K = w.shape[1]
    dx, dn = torch.empty_like(x), torch.empty_like(x)
    dg = torch.empty(K, dtype=torch.float32, device=x.device)
    db = torch.empty(K, dtype=torch.float32, device=x.device)
    dz = torch.empty_like(x) if drop else None
    dp, dseed = drop if drop else (0.0, 0)
    nbytes = query("lotus_layernorm_bwd_workspace", M, K)
    lws = _ws(nbytes, x.device)
    nb = query("lotus_linear_workspace", M, N, K) if M <= 8192 else 0
    ws = WS.get(nb, x.device, slot=5) if nb else None
    nparts = np.zeros(1, dtype=np.int32)
    call("lotus_linear_dgrad_ln", dy, w, x, mean, rstd, g, add, dx, dn, dz, float(dp), int(dseed), M, N, K, _pa(None), ws, nb,
         _counters(x.device) if nb else None, lws, lws.numel(), int(nparts.ctypes.data))
    call("lotus_layernorm_bwd_params_n", lws, int(nparts[0]), K, dg, db, 0)
    return dx, dg, db, dz, int(nparts[0])


def conv_weight_t(w, prec=None):
    """[cout, k,k,k, cin] -> packed MFMA weight fragments for the forward and the input-gradient convolution
    (2 * w.numel() floats; layout in csrc/conv_pairs.hip); use them with the precision they were packed for."""
    cout, cin = w.shape[0], w.shape[-1]
    T = w.numel() // (cout * cin)
    wt = torch.empty(2 * w.numel(), dtype=torch.float32, device=w.device)
    call("lotus_conv_weight_transpose", w, wt, cout, T, cin, _pa(prec))
    return wt


_NO_PACK = {}


def conv_tap_active(lvl, C):
    """True when the 3^3 convolutions of width C at this level take the tap-grouped path of lotus_subm_conv (exact fp32
    products, fp32 storage, a tap plan on the level and an eligible shape): they read the module's own weight tensor, so
    their packed copy need not be produced."""
    return _PREC == 0 and not _capi.BF16 and getattr(lvl, "tap_plan", None) is not None and \
        query("lotus_conv_tap_eligible", lvl.n, C, C) == 1


def no_pack(dev):
    """Stand-in for the packed weights of a convolution that does not read them (null pointer at the C-ABI)."""
    t = _NO_PACK.get(dev)
    if t is None:
        t = _NO_PACK[dev] = torch.empty(0, dtype=torch.float32, device=dev)
    return t


def prepack_conv_weights(weights):
    """Pack the 3^3 convolution weights of a whole forward pass up front, on the weight-gradient stream when it is
    enabled: nine small launches leave the critical stream (they ran in front of every Block.cpe) and overlap the stem.
    The caller orders its stream after them with sync_side_stream() before the first use."""
    global _IN_NODE
    outs = [torch.empty(2 * w.numel(), dtype=torch.float32, device=w.device) for w in weights]
    _IN_NODE += 1  # (the side stream is otherwise reserved for backward nodes)
    try:
        with _OnSide(*weights):
            for w, o in zip(weights, outs):
                cout, cin = w.shape[0], w.shape[-1]
                call("lotus_conv_weight_transpose", w, o, cout, w.numel() // (cout * cin), cin, _pa())
    finally:
        _IN_NODE -= 1
    return outs


def _conv_ws(n, cin, cout, dev):
    nbytes = query("lotus_subm_conv_workspace", n, cin, cout)
    return WS.get(nbytes, dev, slot=2) if nbytes else None


def conv_fwd(x, w, b, nbr, rowidx, add=None, w_t=None, prec=None, tap_plan=None):
    n, cin = x.shape
    cout, T = w.shape[0], nbr.shape[0]
    y = torch.empty(n, cout, dtype=x.dtype, device=x.device)
    if T == 27:
        ws = _conv_ws(n, cin, cout, x.device)
    else:  # thin-input stem kernel: room for the transposed weights
        ws = WS.get(4 * T * cin * cout, x.device, slot=2) if cin <= 8 else None
    call("lotus_subm_conv", 0, x, w, w_t, b, add, y, nbr, rowidx, n, T, cin, cout, _pa(prec), tap_plan, ws,
         ws.numel() if ws is not None else 0)
    return y


def conv_dgrad(dy, w, nbr, rowidx, add=None, w_t=None, lvl=None, prec=None, tap_plan=None):
    """Input gradient of conv_fwd.  The kernel walks the mirrored taps of the forward table, which is the transposed
    pair list exactly when every voxel holds one point; `lvl.n_dup != 0` (augmented real clouds: 1-7 % of the points
    share a cell, SURVEY.md Trap 5) adds the fold / mask passes of lotus_conv_dup_* that make it the true gradient."""
    n, cout = dy.shape
    cin, T = w.shape[-1], nbr.shape[0]
    dups = lvl is not None and lvl.n_dup != 0
    if dups:
        dyr = torch.empty_like(dy)
        call("lotus_conv_dup_fold", dy, lvl.code[0], lvl.order[0], n, cout, dyr)
        dy = dyr
    dx = torch.empty(n, cin, dtype=dy.dtype, device=dy.device)
    ws = _conv_ws(n, cin, cout, dy.device) if T == 27 else None
    call("lotus_subm_conv", 1, dy, w, w_t, None, add, dx, nbr, rowidx, n, T, cin, cout, _pa(prec), tap_plan, ws,
         ws.numel() if ws is not None else 0)
    if dups:
        call("lotus_conv_dup_mask", dx, add, nbr[T // 2], n, cin)
    return dx


def conv_wgrad(dy, x, w_shape, nbr, need_bias=True, prec=None, side=True):
    """side=False keeps the launch on the current stream (the stem: the last weight gradient of a backward pass, when the
    critical stream has nothing left to do and the side stream still has a queue)."""
    n, cout = dy.shape
    cin, T = x.shape[1], nbr.shape[0]
    nw = cout * T * cin
    buf = _grad_slab(nw + (cout if need_bias else 0), dy.device)
    dw = buf[:nw].view(w_shape)
    db = buf[nw:] if need_bias else None
    nbytes = query("lotus_subm_conv_wgrad_workspace", n, T, cin, cout)
    if not side:
        ws = WS.get(nbytes, dy.device, slot=0)
        call("lotus_subm_conv_wgrad", dy, x, dw, db, nbr, n, T, cin, cout, 0, _pa(prec), ws, ws.numel())
        return dw, db
    with _OnSide(dy, x, nbr):
        ws = _side_ws(nbytes, dy.device) if _side() is not None else WS.get(nbytes, dy.device, slot=0)
        # thin-input stem (cin <= 8): one VALU kernel in every mode, exact fp32
        call("lotus_subm_conv_wgrad", dy, x, dw, db, nbr, n, T, cin, cout, 0, _pa(prec), ws, ws.numel())
    return dw, db


def dropout(x, p, seed):
    if p <= 0.0:
        return x
    y = torch.empty_like(x)
    call("lotus_dropout", x, y, x.numel(), float(p), int(seed))
    return y


def pos_targets(pc_fts, off, batch_idx, gt, nb, bin_size, kind="plain", robot_mask=None):
    """Soft position targets on the device (get_disc_gt_pos_prob, utils/action_position_utils.py:7-46), in the
    concatenated per-cloud [3][n_b * nb] layout the loss consumes.  pc_fts: f32 [N, >=3]; gt: f32 [B, >=3]."""
    N, B = pc_fts.shape[0], gt.shape[0]
    tgt = torch.empty(N * 3 * nb, dtype=torch.float32, device=pc_fts.device)
    ws = _ws(query("lotus_pos_workspace", B), pc_fts.device)
    rm = None if robot_mask is None else robot_mask.to(torch.uint8).contiguous()
    call("lotus_pos_targets", pc_fts, pc_fts.stride(0), off, batch_idx, gt, gt.stride(0), rm, B, N, nb, float(bin_size),
         {"plain": 0, "dist": 1}[kind], tgt, ws, ws.numel())
    return tgt


def pos_decode_max(xt, pc_fts, off, B, nb, bin_size):
    """get_best_pos_from_disc_pos(best='max') (utils/action_position_utils.py:48-64) for every cloud: f64 [B, 3]."""
    out = torch.empty(B, 3, dtype=torch.float64, device=xt.device)
    ws = _ws(query("lotus_pos_workspace", B), xt.device)
    call("lotus_pos_decode_max", xt, pc_fts, pc_fts.stride(0), off, B, nb, float(bin_size), out, ws, ws.numel())
    return out


def pos_decode_ens1(xt, pc_fts, counts, nb, bin_size):
    """get_best_pos_from_disc_pos(best='ens1') (utils/action_position_utils.py:66-85) for every cloud: f64 [B, 3].  An
    evaluation-time option of the reference (eval_simple_policy.py:63,83), evaluated on the host like there: per (cloud,
    axis) the softmax of the logits (on the device), then the probabilities summed per 5 mm cell in order of decreasing
    probability (sequential float32 accumulation, as the reference's dict of numpy scalars does it), the first cell with the
    strictly largest sum wins.  Vectorised: sort, np.add.at over cell ids in first-appearance order."""
    import numpy as np

    B = len(counts)
    pos_bins = nb // 2
    shift = np.arange(-pos_bins, pos_bins) * bin_size                      # float64, as the reference builds it
    out = np.zeros((B, 3), dtype=np.float64)
    xyz_all = pc_fts[:, :3].detach().float().cpu().numpy()
    lo = 0
    for b, n in enumerate(counts):
        lg = xt[lo:lo + n].detach().float().view(n, 3, nb).permute(1, 0, 2).reshape(3, n * nb)   # 'n (c b) -> c (n b)'
        prob = torch.softmax(lg, -1).cpu().numpy()
        xyz = xyz_all[lo:lo + n]
        for c in range(3):
            cands = (xyz[:, c:c + 1] + shift[None, :]).reshape(-1)          # float32 + float64 -> float64
            vox = np.round(cands / 0.005).astype(np.int32)
            order = np.argsort(-prob[c])
            v_s, p_s = vox[order], prob[c][order]
            uniq, first, inv = np.unique(v_s, return_index=True, return_inverse=True)
            acc = np.zeros(len(uniq), dtype=p_s.dtype)
            np.add.at(acc, inv, p_s)                                        # sequential, in visiting order
            visit = np.argsort(first, kind="stable")                        # cells in order of first appearance
            out[b, c] = int(uniq[visit[np.argmax(acc[visit])]]) * 0.005     # argmax: the first of the largest sums
        lo += n
    return torch.from_numpy(out).to(xt.device)


def sum_slabs(part):
    """part [G, ...] -> sum over G in fixed order (one launch; G == 1: the slab itself)."""
    if part.shape[0] == 1:
        return part[0]
    out = torch.empty_like(part[0])
    n = out.numel()
    call("lotus_sum_slabs", part, out, n, n, part.shape[0])
    return out


def drop_path(branch, x, p, seed):
    """x + DropPath(branch) (x may be None: the per-row mask alone, i.e. the backward map); timm.DropPath semantics, one
    draw per point row (model.py:655-657)."""
    M, C = branch.shape
    y = torch.empty_like(branch)
    call("lotus_drop_path", branch, x, y, M, C, float(p), int(seed))
    return y


def add(a, b):
    y = torch.empty_like(a)
    call("lotus_add", a, b, y, a.numel())
    return y


# Test-only taps of the two arg-max tables of the model (SerializedPooling's segment max, model.py:760-765, and the head's
# per-cloud max, simple_policy_ptv3.py:117-119).  ARG_TAP: a list that receives (kind, int32 table) in forward order.
# A third routing decision of the same kind ("leaky"): the sign pattern of the head's LeakyReLU(0.02) pre-activation
# (simple_policy_ptv3.py:42,113-115) — a pre-activation within rounding of zero gets slope 1 in one arithmetic and 0.02 in the
# other; the tap / injection is the saved pre-activation tensor itself (only its signs matter to backward).
# ARG_INJECT: a list of int32 tables consumed in the same order — the backward pass then routes the gradient of every
# (segment, channel) to the row the INJECTED table names while the forward values stay the kernel's own.  This is how
# tests/test_gpu_fullsize_oracle.py separates "a near-tie was broken the other way" (a discrete re-routing both fp32
# implementations are entitled to) from a defect: with the oracle's table injected every gradient must meet 1e-4.
ARG_TAP = None
ARG_INJECT = None


def _arg_hook(kind, arg):
    if ARG_TAP is not None:
        ARG_TAP.append((kind, arg))
    if ARG_INJECT:
        k2, inj = ARG_INJECT.pop(0)
        assert k2 == kind and tuple(inj.shape) == tuple(arg.shape), (k2, kind, tuple(inj.shape), tuple(arg.shape))
        return inj.to(device=arg.device, dtype=arg.dtype).contiguous()
    return arg


class BnState:
    """Batch statistics hook: `reduce(sums)` all-reduces the fp64 vector (sum, sumsq, count) across
    ranks when SyncBatchNorm semantics are wanted (train_simple_policy.py:116-117); None = local."""
    reduce = None


def _bn_stats(x, sums):
    M, C = x.shape
    ws = _ws(query("lotus_batchnorm_workspace", M, C), x.device)
    if _BN_FUSED and x.is_cuda and M > 0:  # one launch (last-arrival reduction), the sums alone
        call("lotus_batchnorm_stats_fused", x, sums, None, None, None, None, M, C, 0.0, 0.0, ws, ws.numel(), _bn_counter(x.device))
        return
    call("lotus_batchnorm_stats", x, sums, M, C, ws, ws.numel())


def _bn_apply(x, mean, invstd, g, b, act, mod=None, lvl=None):
    M, C = x.shape
    y = torch.empty_like(x)
    if mod is None:
        call("lotus_batchnorm_apply", x, mean, invstd, g, b, y, M, C, act)
    else:
        call("lotus_adabn_apply", x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), y, M, C, act)
    return y


def _bn_apply_sums(x, sums, g, b, rmean, rvar, act, momentum=BN_MOMENTUM, eps=BN_EPS, mod=None, lvl=None):
    """statistics -> (message) -> apply: the apply pass finishes mean / invstd / running averages from the (all-reduced) sums
    itself (SyncBatchNorm forward: one launch less between the all-reduce and the consumer)."""
    M, C = x.shape
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    if mod is None:
        call("lotus_batchnorm_apply_sums", x, sums, g, b, y, mean, invstd, rmean, rvar, M, C, act, float(eps), float(momentum))
    else:
        call("lotus_adabn_apply_sums", x, sums, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), y, mean, invstd, rmean, rvar,
             M, C, act, float(eps), float(momentum))
    return y, mean, invstd


def _bn_finish(x, sums, g, b, rmean, rvar, training, act, momentum, eps, mod=None, lvl=None):
    if training and x.is_cuda:
        return _bn_apply_sums(x, sums, g, b, rmean, rvar, act, momentum, eps, mod, lvl)
    C = x.shape[1]
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    if training:
        call("lotus_batchnorm_finalize", sums, mean, invstd, rmean, rvar, C, float(eps), float(momentum))
    else:
        call("lotus_batchnorm_eval_stats", rmean, rvar, mean, invstd, C, float(eps))
    return _bn_apply(x, mean, invstd, g, b, act, mod, lvl), mean, invstd


_BN_FUSED = True  # one-launch BatchNorm statistics (two-level last-arrival reduction); False: the partials + reduce launches
_BN_CNT_OFF = None


def _bn_counter(dev):
    """The BatchNorm arrival counters of the stream being launched on (tail of the zeroed split-K counter buffer)."""
    global _BN_CNT_OFF
    if _BN_CNT_OFF is None:
        _BN_CNT_OFF = query("lotus_bn_counters_offset")
    return _counters(dev).data_ptr() + _BN_CNT_OFF


def bn_fwd(x, g, b, rmean, rvar, training, act, momentum=BN_MOMENTUM, eps=BN_EPS, mod=None, lvl=None):
    """act(BN(x) g + b): batch statistics (+ running-average update) in training, running ones in eval; with a statistics hook
    (BnState.reduce: SyncBatchNorm) the training pass is statistics -> one fp64 message (sum x, sum x^2, rows) -> apply.
    mod / lvl as in ln_fwd: act((BN(x) g + b) (1 + scale_b) + shift_b) — the same statistics, the adaptive apply entry."""
    sums = None
    if training and _BN_FUSED and BnState.reduce is None and x.shape[0] > 0:
        # local batch statistics: statistics, their reduction, mean / invstd and the running averages in ONE launch
        M, C = x.shape
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _ws(query("lotus_batchnorm_workspace", M, C), x.device)
        call("lotus_batchnorm_stats_fused", x, sums, mean, invstd, rmean, rvar, M, C, float(eps), float(momentum), ws, ws.numel(),
             _bn_counter(x.device))
        return _bn_apply(x, mean, invstd, g, b, act, mod, lvl), mean, invstd
    if training:
        sums = torch.empty(2 * x.shape[1] + 1, dtype=torch.float64, device=x.device)
        _bn_stats(x, sums)
        if BnState.reduce is not None:
            BnState.reduce(sums)
    return _bn_finish(x, sums, g, b, rmean, rvar, training, act, momentum, eps, mod, lvl)


def bn_fwd_pair(xa, pa, xb, pb, training, act, momentum=BN_MOMENTUM, eps=BN_EPS):
    """Two independent BatchNorms (the two branches of SerializedUnpooling) with ONE statistics message when
    SyncBatchNorm is on: the all-reduces are latency-bound, 26 -> 18 per step.  pa / pb = (g, b, rmean, rvar[, mod, lvl])."""
    if not training or BnState.reduce is None:
        return (bn_fwd(xa, *pa[:4], training, act, momentum, eps, *pa[4:]),
                bn_fwd(xb, *pb[:4], training, act, momentum, eps, *pb[4:]))
    na, nb_ = 2 * xa.shape[1] + 1, 2 * xb.shape[1] + 1
    sums = torch.empty(na + nb_, dtype=torch.float64, device=xa.device)
    _bn_stats(xa, sums[:na])
    _bn_stats(xb, sums[na:])
    BnState.reduce(sums)
    return (_bn_finish(xa, sums[:na], *pa[:4], training, act, momentum, eps, *pa[4:]),
            _bn_finish(xb, sums[na:], *pb[:4], training, act, momentum, eps, *pb[4:]))


def _bn_bwd_stats(dy, x, mean, invstd, g, b, act, sums, want_params=False, mod=None, dmod=None, lvl=None):
    """sums = (sum dz, sum dz * xhat, M) of the local rows; want_params: also (dgamma, dbeta) as fp32 vectors taken from those
    LOCAL sums (SyncBatchNorm: before the all-reduce overwrites them) — written by the statistics kernel itself on the GPU.
    With `mod` (the split backward only): dgamma, dbeta (local, as above), d mod into `dmod` and the fp64 message
    sums = (gamma dbeta, gamma dgamma, rows) from the adaptive partial pass and its fixed-order reduction."""
    M, C = x.shape
    if mod is not None:
        B = _n_clouds(lvl)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = WS.get(query("lotus_adanorm_workspace", M, B, C), x.device, slot=_ADA_WS_SLOT)
        call("lotus_adabn_bwd_stats", dy, x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, B, dg, db, dmod, dmod.stride(0), sums,
             M, C, act, ws, ws.numel())
        return dg, db
    ws = _ws(query("lotus_batchnorm_workspace", M, C), x.device)
    if want_params and _BN_FUSED and M > 0 and x.is_cuda:
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        call("lotus_batchnorm_bwd_stats_fused_params", dy, x, mean, invstd, g, b, sums, dg, db, M, C, act, ws, ws.numel(), _bn_counter(x.device))
        return dg, db
    if want_params:
        _bn_bwd_stats(dy, x, mean, invstd, g, b, act, sums)
        return sums[C:2 * C].float(), sums[:C].float()
    if _BN_FUSED and M > 0:
        call("lotus_batchnorm_bwd_stats_fused", dy, x, mean, invstd, g, b, sums, M, C, act, ws, ws.numel(), _bn_counter(x.device))
    else:
        call("lotus_batchnorm_bwd_stats", dy, x, mean, invstd, g, b, sums, M, C, act, ws, ws.numel())


def _bn_bwd_apply(dy, x, mean, invstd, g, b, training, act, sums, reduced, mod=None, dmod=None, lvl=None):
    # dgamma / dbeta are the LOCAL sums (gradient averaging across ranks is the reducer's job);
    # dx uses the statistics of the whole (all-rank) batch
    M, C = x.shape
    dx = torch.empty_like(x)
    if mod is not None:  # (the split backward: `reduced` and d mod come from _bn_bwd_stats)
        dg, db = reduced
        call("lotus_adabn_bwd_apply_sums", dy, x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, _n_clouds(lvl), sums, dx, M, C, act)
    elif reduced is not None:  # (dg, db) were taken from the local sums before the all-reduce
        dg, db = reduced
        call("lotus_batchnorm_bwd_apply", dy, x, mean, invstd, g, b, sums, dx, None, None, M, C, act, 1, 0)
    else:  # local statistics: the apply kernel writes the parameter gradients itself
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        call("lotus_batchnorm_bwd_apply", dy, x, mean, invstd, g, b, sums, dx, dg, db, M, C, act,
             1 if training else 0, 0)
    return dx, dg, db


def bn_bwd(dy, x, mean, invstd, g, b, training, act, mod=None, dmod=None, lvl=None):
    """-> dx, dgamma, dbeta (+ d mod into `dmod`): statistics -> (one fp64 message when SyncBatchNorm is on) -> apply; the
    adaptive norm with local statistics is one entry point."""
    M, C = x.shape
    split = training and BnState.reduce is not None
    if mod is not None and not split:
        B = _n_clouds(lvl)
        dx = torch.empty_like(x)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = WS.get(query("lotus_adanorm_workspace", M, B, C), x.device, slot=_ADA_WS_SLOT)
        call("lotus_adabn_bwd", dy, x, mean, invstd, g, b, mod, mod.stride(0), lvl.off, B, dx, dg, db, dmod, dmod.stride(0), M, C, act,
             1 if training else 0, ws, ws.numel())
        return dx, dg, db
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    reduced = _bn_bwd_stats(dy, x, mean, invstd, g, b, act, sums, split, mod, dmod, lvl)
    if split:
        BnState.reduce(sums)
    return _bn_bwd_apply(dy, x, mean, invstd, g, b, training, act, sums, reduced, mod, dmod, lvl)


def bn_bwd_pair(a, bb, training, act):
    """Backward of bn_fwd_pair: a / bb = (dy, x, mean, invstd, g, b[, mod, dmod, lvl]); one statistics message for both."""
    if not training or BnState.reduce is None:
        return bn_bwd(*a[:6], training, act, *a[6:]), bn_bwd(*bb[:6], training, act, *bb[6:])
    Ca, Cb = a[1].shape[1], bb[1].shape[1]
    na = 2 * Ca + 1
    sums = torch.empty(na + 2 * Cb + 1, dtype=torch.float64, device=a[1].device)
    sa, sb = sums[:na], sums[na:]
    ra = _bn_bwd_stats(*a[:6], act, sa, True, *a[6:])
    rb = _bn_bwd_stats(*bb[:6], act, sb, True, *bb[6:])
    BnState.reduce(sums)
    return _bn_bwd_apply(*a[:6], training, act, sa, ra, *a[6:]), _bn_bwd_apply(*bb[:6], training, act, sb, rb, *bb[6:])


def silu(x, dy=None):
    """SiLU(x), or dy SiLU'(x) when dy is given."""
    y = torch.empty_like(x)
    call("lotus_ada_silu", x, dy, y, x.numel())
    return y


def _qk_norms(qn, kn):
    """(qn, kn) as two (weight, bias) pairs; None, None -> the null pointers that select the kernels without the norm."""
    if qn is None and kn is None:
        return (None, None), (None, None)
    if qn is None or kn is None:
        raise ValueError("attention: q_norm and k_norm are given together or not at all")
    return qn, kn


def attention_fwd(q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, ntiles, qn, kn, out, lse, H, d,
                  drop_p=0.0, seed=0, prec=None, k_max=0):
    """qn / kn = (weight, bias) of q_norm / k_norm, or both None: attention without q/k normalisation (fp32 only)."""
    qn, kn = _qk_norms(qn, kn)
    call("lotus_attention_fwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, ntiles,
         qn[0], qn[1], kn[0], kn[1], out, out.stride(0), lse, H, d, float(d ** -0.5), 1e-6, float(drop_p), int(seed),
         _pa(prec), int(k_max))


def attention_bwd(q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks, qn, kn, out,
                  dout, lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off, part_stride, atomic, H, d, drop_p=0.0, seed=0,
                  kext=None, ext_pos=None, n_extra=0, dkv_extra=None, prec=None, k_max=0):
    """-> the gradients of q_norm / k_norm (weight, bias, weight, bias); four None when qn = kn = None (no q/k norm)."""
    dev = q.device
    plain = qn is None and kn is None
    qn, kn = _qk_norms(qn, kn)
    if plain:  # no norm partials: the entry point takes neither gradient outputs nor a workspace
        call("lotus_attention_bwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks,
             None, None, None, None, out, dout, out.stride(0), lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off,
             part_stride, atomic, kext, ext_pos, n_extra, dkv_extra, None, None, None, None, 0, H, d, float(d ** -0.5), 1e-6,
             float(drop_p), int(seed), _pa(prec), int(k_max), None, 0)
        return [None] * 4
    grads = [torch.empty(d, dtype=torch.float32, device=dev) for _ in range(4)]
    ws = _ws(query("lotus_attention_bwd_workspace", nblocks, H), dev)
    call("lotus_attention_bwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks,
         qn[0], qn[1], kn[0], kn[1], out, dout, out.stride(0), lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off,
         part_stride, atomic, kext, ext_pos, n_extra, dkv_extra, grads[0], grads[1], grads[2], grads[3], 0, H, d, float(d ** -0.5), 1e-6, float(drop_p),
         int(seed), _pa(prec), int(k_max), ws, ws.numel())
    return grads


def rpe_bound(patch_size):
    """pos_bnd of RPE for a configured patch size, by the reference's own expression (model.py:311): 15 at 128, since
    512 ** (1 / 3) is 7.999..."""
    return int((4 * patch_size) ** (1 / 3) * 2)


def attention_rpe_fwd(q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, ntiles, qn, kn, out, lse, H, d, grid,
                      table, bnd, drop_p=0.0, seed=0):
    """attention_fwd with the relative-position term (model.py:307-326, :518-527): grid int32 [n, 3], table = rpe.rpe_table
    [3 (2 bnd + 1), H].  Exact fp32, fp32 storage."""
    assert not _capi.BF16, "the relative-position term of the attention runs with fp32 activation storage"
    qn, kn = _qk_norms(qn, kn)
    call("lotus_attention_rpe_fwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, ntiles,
         qn[0], qn[1], kn[0], kn[1], out, out.stride(0), lse, H, d, float(d ** -0.5), 1e-6, float(drop_p), int(seed),
         grid, table, int(bnd))


_RPE_WS_SLOT = 8  # workspace slot of the relative-position backward: norm partials and table-gradient partials (main stream)


def attention_rpe_bwd(q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks, qn, kn, out,
                      dout, lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off, part_stride, H, d, grid, table, bnd, drop_p=0.0,
                      seed=0, kext=None, ext_pos=None, n_extra=0, dkv_extra=None):
    """-> (the gradients of q_norm / k_norm: weight, bias, weight, bias — four None when qn = kn = None, dtable).  Plain stores;
    the table gradient is written on the calling stream, without atomics."""
    assert not _capi.BF16, "the relative-position term of the attention runs with fp32 activation storage"
    dev = q.device
    plain = qn is None and kn is None
    qn, kn = _qk_norms(qn, kn)
    grads = [None] * 4 if plain else [torch.empty(d, dtype=torch.float32, device=dev) for _ in range(4)]
    dtable = torch.empty_like(table)
    ws = WS.get(query("lotus_attention_rpe_bwd_workspace", nblocks, H, int(bnd)), dev, slot=_RPE_WS_SLOT)
    call("lotus_attention_rpe_bwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks,
         qn[0], qn[1], kn[0], kn[1], out, dout, out.stride(0), lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off,
         part_stride, kext, ext_pos, n_extra, dkv_extra, grads[0], grads[1], grads[2], grads[3], 0, H, d, float(d ** -0.5), 1e-6,
         float(drop_p), int(seed), grid, table, int(bnd), dtable, ws, ws.numel())
    return grads, dtable


def attention_long_fwd(q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, ntiles, qn, kn, out, lse, H, d, len_max,
                       drop_p=0.0, seed=0):
    """attention_fwd over tiles of up to ATTN_LONG_MAX rows (patch sizes 256, 512, 1024; model.py:529-551): len_max = the longest
    q_len / k_len of a tile, declared by the caller.  Exact fp32, fp32 storage; its own dropout numbering (include/lotus_hip.h)."""
    assert not _capi.BF16, "the patch attention above 128 rows runs with fp32 activation storage"
    qn, kn = _qk_norms(qn, kn)
    call("lotus_attention_long_fwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, ntiles,
         qn[0], qn[1], kn[0], kn[1], out, out.stride(0), lse, H, d, float(d ** -0.5), 1e-6, float(drop_p), int(seed), int(len_max))


def long_tiles(lvl):
    """Whether the level's patch attention runs on the long kernels: its longest self-attention tile has more than 128 rows
    (Level.tile_max, from the host plan).  A level of a model with patch size 256 / 512 / 1024 whose clouds all fit 128-row tiles
    keeps the 128-row kernels and its composite."""
    return getattr(lvl, "tile_max", 0) > 128


_LONG_WS_SLOT = 9  # workspace slot of the long-patch backward: delta and the norm partials (main stream)


def attention_long_bwd(q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks, qn, kn, out,
                       dout, lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off, part_stride, H, d, len_max, drop_p=0.0,
                       seed=0, kext=None, ext_pos=None, n_extra=0, dkv_extra=None):
    """-> the gradients of q_norm / k_norm (weight, bias, weight, bias); four None when qn = kn = None.  Plain stores, no atomics;
    lse is [npos, H] and every tile lies inside its rows."""
    assert not _capi.BF16, "the patch attention above 128 rows runs with fp32 activation storage"
    dev = q.device
    plain = qn is None and kn is None
    qn, kn = _qk_norms(qn, kn)
    grads = [None] * 4 if plain else [torch.empty(d, dtype=torch.float32, device=dev) for _ in range(4)]
    npos = int(lse.shape[0])
    ws = WS.get(query("lotus_attention_long_bwd_workspace", nblocks, H, int(len_max), npos), dev, slot=_LONG_WS_SLOT)
    call("lotus_attention_long_bwd", q, q_ld, q_off, kv, kv_ld, k_off, v_off, qidx, kidx, owner, tiles, blocks, nblocks,
         qn[0], qn[1], kn[0], kn[1], out, dout, out.stride(0), lse, dq, dq_ld, dq_off, dkv, dkv_ld, dk_off, dv_off,
         part_stride, kext, ext_pos, n_extra, dkv_extra, grads[0], grads[1], grads[2], grads[3], 0, H, d, float(d ** -0.5), 1e-6,
         float(drop_p), int(seed), int(len_max), npos, ws, ws.numel())
    return grads


# ------------------------------------------------------------------------------------ composite fast path
# One C call per sub-block direction (csrc/blocks.cpp) instead of one per launch: same entry points, same order, same
# streams -> bit-identical results (tests/test_gpu_blocks.py), ~70 % less interpreter time inside the sub-blocks.  The
# per-launch bodies below stay as the readable reference and serve the diagnostics (bench.py's per-launch event log).
_COMPOSITE = os.environ.get("LOTUS_PY_BLOCKS", "0") != "1"
_SIZE_CACHE = {}


def composites_enabled():
    # (one weight-gradient stream: a handed-over dz is only known to be ordered on the stream its producer forked to)
    return _COMPOSITE and CALL_LOG is None and EVENT_LOG is None and _NSIDE == 1


def set_composites(on):
    global _COMPOSITE
    _COMPOSITE = bool(on)


def _queries(prefix, dims, spec):
    return dims.split(), [(prefix + q.split(":")[0], q.split(":")[1].split(",")) for q in spec.split()]


# kind -> (names of its dims, its size queries with their arguments in the order _sizes returns them)
_SIZE_QUERIES = {
    "ffn": _queries("lotus_ffn_", "M C Hd", "saved_floats:M,C,Hd grads_floats:C,Hd tmp_floats:M,C,Hd ws_main_bytes:M,C,Hd ws_side_bytes:M,C,Hd"),
    "self": _queries("lotus_selfattn_", "M C H npad nblocks n_extra", "saved_floats:M,C,H,npad grads_floats:C,H tmp_floats:M,C,n_extra "
                     "ws_main_bytes:M,C,H,nblocks ws_side_bytes:M,C"),
    "cross": _queries("lotus_crossattn_", "M C H L Cc nblocks G", "saved_floats:M,C,H,L grads_floats:C,H,Cc tmp_floats:M,C,L,G "
                      "ws_main_bytes:M,C,H,L,Cc,nblocks ws_side_bytes:M,C,L,Cc"),
    "crosskv": _queries("lotus_crossattn_kv_", "M C H L nblocks G", "saved_floats:M,C,H grads_floats:C,H tmp_floats:M,C,L,G "
                        "ws_main_bytes:M,C,H,nblocks ws_side_bytes:M,C"),
    "pair": _queries("lotus_pair_", "M C H Hd npad nst n_extra L nca G", "acts_floats:M,C saved_floats:M,C,H,Hd,npad grads_floats:C,H,Hd "
                     "tmp_floats:M,C,Hd,n_extra,L,G ws_main_bytes:M,C,H,Hd,nst,nca ws_side_bytes:M,C,Hd ws_conv_bytes:M,C"),
    "cpe": _queries("lotus_cpe_", "n C", "saved_floats:n,C grads_floats:C tmp_floats:n,C ws_main_bytes:n,C ws_side_bytes:n,C ws_conv_bytes:n,C"),
}


def _sizes(kind, *dims):
    key = (kind, _capi.BF16) + dims
    v = _SIZE_CACHE.get(key)
    if v is None:
        names, queries = _SIZE_QUERIES[kind]
        d = dict(zip(names, dims))
        assert len(d) == len(dims) == len(names), (kind, dims)
        v = _SIZE_CACHE[key] = tuple(query(q, *[d[a] for a in args]) for q, args in queries)
    return v


# Where each parameter gradient lies in the `grads` slab of a composite is defined in csrc/blocks.cpp, next to the code that
# writes it, and asked for here (lotus_composite_grads_layout: (offset, length) per field in slab order).  What Python adds per
# kind is the order in which the autograd node returns them and the 2-D shapes of the weights: (field, shape or None) below.
_GRAD_KINDS = {"ffn": 0, "self": 1, "cross": 2, "crosskv": 3, "cpe": 4, "pair": 5}


def _grad_returns(kind, C, Hd, Cc, cshape):
    cpe = ((4, cshape), 5, (2, (C, C)), 3, 0, 1)   # returned as dcw, dcb, dlw, dlb, dg, db
    att = (0, 1, (2, (3 * C, C)), 3, 4, 5, 6, 7, (8, (C, C)), 9)
    ffn = (0, 1, (2, (Hd, C)), 3, (4, (C, Hd)), 5)
    ca = (0, 1, (2, (C, C)), 3, 4, 5, 6, 7, (8, (C, C)), 9)
    cross = (0, 1, (2, (C, C)), 3, (4, (2 * C, Cc)), 5, 6, 7, 8, 9, (10, (C, C)), 11)
    subs = {"ffn": (ffn,), "self": (att,), "cross": (cross,), "crosskv": (ca,), "cpe": (cpe,), "pair": (cpe, att, ffn, ca, ffn)}[kind]
    out, first = [], 0
    for sub in subs:   # (the pair: its five sub-blocks one after the other, i.e. the 38 parameters in _PAIR_PARAM_SLOTS order)
        out += [(first + f[0], f[1]) if isinstance(f, tuple) else (first + f, None) for f in sub]
        first += len(sub)
    return out


def _grad_views(grads, kind, C, H=1, Hd=0, Cc=0, cshape=None):
    """The parameter gradients of a composite backward as views of its `grads` slab, in the node's return order.  The plan
    (split sizes, then chunk index and shape per returned tensor) is computed once per (kind, dims)."""
    key = ("grads", kind, C, H, Hd, Cc, cshape)
    plan = _SIZE_CACHE.get(key)
    if plan is None:
        import numpy as np
        off, length = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int64)
        n = query("lotus_composite_grads_layout", _GRAD_KINDS[kind], C, H, Hd, Cc, off.ctypes.data, length.ctypes.data, 64)
        returns = _grad_returns(kind, C, Hd, Cc, cshape)
        if not 0 < n <= 64 or sorted(f for f, _ in returns) != list(range(n)):
            raise _capi.LotusError(f"lotus_composite_grads_layout({kind}) reports {n} fields, ops returns {len(returns)}")
        sizes, chunk, end = [], {}, 0
        for f in range(n):   # split sizes: the fields, and the padding between them as chunks of their own
            if off[f] > end:
                sizes.append(int(off[f]) - end)
            chunk[f] = len(sizes)
            sizes.append(int(length[f]))
            end = int(off[f] + length[f])
        if grads.numel() > end:
            sizes.append(grads.numel() - end)
        plan = _SIZE_CACHE[key] = (sizes, tuple((chunk[f], shape) for f, shape in returns))
    parts = grads.split(plan[0])
    return tuple([parts[i] if shape is None else parts[i].view(shape) for i, shape in plan[1]])


def _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, reads, rows):
    """What every composite backward allocates -> (grads, tmp, main workspace, side stream pointer or 0, its workspace, that
    workspace's bytes, its counters); `reads`: what the side stream reads besides tmp (see _side_ctx)."""
    grads = _grad_slab(n_grads, dev)
    tmp = torch.empty(n_tmp, dtype=torch.float32, device=dev)
    side, wss, cs = _side_ctx(dev, ws_side, (tmp,) + reads, rows)
    wsm = _ws(ws_main if side else max(ws_main, ws_side), dev)  # no side stream: the weight gradients use it too
    return grads, tmp, wsm, side, wss, (wss.numel() if wss is not None else 0), cs


def _side_ctx(dev, ws_side_bytes, reads, rows=0):
    """(side stream pointer or 0, its workspace, its counters) for a composite backward; the tensors the side stream reads
    are held until the join (as _OnSide does; in the "node" mode they are locals of the node's backward() as well)."""
    global _CUR
    if _side() is None:  # (measured and not kept: the big levels' weight gradients on the critical stream, 907 / 883 / 861 vs 930)
        return 0, None, None
    _CUR = 0
    st, ptr = _SIDES[0]
    if _JOIN == "end":
        _hold_for_side(reads, st)
    elif _NODE_HELD is not None:
        _NODE_HELD.append(reads)
    ws = _side_ws(ws_side_bytes, dev)
    return ptr, ws, _counters_for(dev, ptr)


# ------------------------------------------------------------------------------------ sub-blocks
# Every node that ends or begins in a norm takes trailing `mod = None, bank = None, j = 0`: the [B, 2C] modulation slice of an
# adaptive PDNorm (adanorm.py; None = the plain norm), and the bank whose grad_slice(j) the norm's backward writes d mod into
# (returned as the gradient of `mod`).  The composite (one C call) branches are plain LayerNorm with q/k norm only; with `mod`,
# without q/k norm, with DropPath or with composites off a node runs per launch: its norm, then the bodies below.
def _dmod(mod, site):
    return None if mod is None else site[0].grad_slice(site[1])


def cpe_branch_fwd(xs, cw, cb, lw, lb, lvl, wt):
    """-> (c, l) = SubMConv3d_3(xs), Linear(c): the input of the sub-block's norm, and what its backward needs."""
    c = conv_fwd(xs, cw, cb, lvl.nbr27, lvl.order[0], w_t=wt, tap_plan=lvl.tap_plan)
    l, _ = linear_fwd(c, lw, lb)
    return c, l


def cpe_branch_bwd(dl, dy, xs, cw, lw, c, lvl, wt, same):
    """dl = the norm's input gradient, dy = the node's -> (dx, dxs | None, dcw, dcb, dlw, dlb)."""
    dlw, dlb = linear_wgrad(dl, c)
    dc = linear_dgrad(dl, lw)
    dcw, dcb = conv_wgrad(dc, xs, cw.shape, lvl.nbr27)
    if same:  # d x = dy (residual) + conv dgrad
        dx = conv_dgrad(dc, cw, lvl.nbr27, lvl.order[0], add=dy, w_t=wt, lvl=lvl, tap_plan=lvl.tap_plan)
        return dx, None, dcw, dcb, dlw, dlb
    dxs = conv_dgrad(dc, cw, lvl.nbr27, lvl.order[0], w_t=wt, lvl=lvl, tap_plan=lvl.tap_plan)
    return dy, dxs, dcw, dcb, dlw, dlb


def coord_add_fwd(y, W, Cw, coord, cproj):
    """In place: y[:, j] += (coord cproj^T)[:, j % Cw] for j < W (W = Cw or 2 Cw; the other columns of y are not touched).  coord
    [N, 3] fp32 with any row stride (the [:, :3] view of pc_fts at level 0), cproj = coords_proj.weight [Cw, 3] (model.py:484-495)."""
    assert not _capi.BF16, "the coordinate term of the attention runs with fp32 activation storage"
    call("lotus_coord_add_fwd", y, y.stride(0), W, Cw, coord, coord.stride(0), cproj, y.shape[0])


_COORD_WS_SLOT = 7  # workspace slot of the coordinate term's weight-gradient partials (main stream)


def coord_add_wgrad(dy, W, Cw, coord):
    """-> d cproj [Cw, 3] = sum over the rows of (dy[:, :Cw] (+ dy[:, Cw:2 Cw] when W = 2 Cw))^T coord, on the calling stream."""
    assert not _capi.BF16, "the coordinate term of the attention runs with fp32 activation storage"
    n = dy.shape[0]
    dP = torch.empty(Cw, 3, dtype=torch.float32, device=dy.device)
    ws = WS.get(query("lotus_coord_add_workspace", n, W, Cw), dy.device, slot=_COORD_WS_SLOT)
    call("lotus_coord_add_wgrad", dy, dy.stride(0), W, Cw, coord, coord.stride(0), n, dP, ws, ws.numel())
    return dP


def selfattn_branch_fwd(n, x, wqkv, bqkv, qn, kn, wp, bp, lvl, H, drop_p, seed, attn_p, dpath, coord=None, cproj=None, cmode=None,
                        rpe=None):
    """n = norm(x) -> (y, qkv, att, lse), y = x + DropPath(drop(proj(PatchAttention(qkv(n))))); qn / kn = (weight, bias), or
    both None for attention without q/k normalisation.  coord / cproj / cmode: add_coords_in_attn (model.py:484-495) — 'qkv' adds
    coord cproj^T to `n` IN PLACE before the qkv product (the caller saves that n: it is what the product's weight gradient reads),
    'qk' adds it to the q and the k columns of the product.  rpe = (rpe_table [3 (2 bnd + 1), H], bnd): the patch attention runs
    with the relative-position term (enable_rpe, model.py:307-326, :518-527) over the level's grid coordinates."""
    N, C = x.shape
    if cmode == "qkv":
        coord_add_fwd(n, C, C, coord, cproj)
    qkv, _ = linear_fwd(n, wqkv, bqkv)
    if cmode == "qk":
        coord_add_fwd(qkv, 2 * C, C, coord, cproj)
    att = torch.empty(N, C, dtype=x.dtype, device=x.device)
    lse = torch.empty(lvl.npad, H, dtype=torch.float32, device=x.device)
    if long_tiles(lvl):  # tiles above 128 rows: key images walked with an online softmax (csrc/attention_long.hip)
        if rpe is not None:
            raise NotImplementedError("the relative-position term is built for patches of at most 128 rows")
        attention_long_fwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lvl.gidx, lvl.gidx, lvl.owner, lvl.self_tiles,
                           lvl.n_self_tiles, qn, kn, att, lse, H, C // H, lvl.tile_max, attn_p, mix_seed(seed, 1))
    elif rpe is None:
        attention_fwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lvl.gidx, lvl.gidx, lvl.owner, lvl.self_tiles,
                      lvl.n_self_tiles, qn, kn, att, lse, H, C // H, attn_p, mix_seed(seed, 1))
    else:
        attention_rpe_fwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lvl.gidx, lvl.gidx, lvl.owner, lvl.self_tiles,
                          lvl.n_self_tiles, qn, kn, att, lse, H, C // H, lvl.grid, rpe[0], rpe[1], attn_p, mix_seed(seed, 1))
    if dpath > 0.0:
        br, _ = linear_fwd(att, wp, bp, drop_p=drop_p, seed=seed)
        y = drop_path(br, x, dpath, mix_seed(seed, 5))
    else:
        y, _ = linear_fwd(att, wp, bp, residual=x, drop_p=drop_p, seed=seed)
    return y, qkv, att, lse


def selfattn_branch_bwd(dy, n, qkv, att, lse, wqkv, qn, kn, wp, lvl, H, p, seed, attn_p, dpath, hand, coord=None, cmode=None,
                        rpe=None):
    """-> (dn, dwqkv, dbqkv, gq, bq, gk, bk, dwp, dbp, dcproj, dtable); `hand`: the hand-over that may hold dy pre-masked (or
    None).  gq, bq, gk, bk are None when qn = kn = None; dcproj is None without the coordinate term (cmode None), dtable without
    the relative-position term (rpe None)."""
    N, C = n.shape
    dyb = drop_path(dy, None, dpath, mix_seed(seed, 5)) if dpath > 0.0 else dy
    dz = _masked(dyb, p, seed, hand)
    dwp, dbp = linear_wgrad(dz, att)
    datt = linear_dgrad(dz, wp)
    # every (point, q|k|v column) is written exactly once by its owner position; the k/v gradients of the
    # borrowed tail-patch copies go to a small side buffer and are added afterwards (no atomics, no memset)
    dqkv = torch.empty(N, 3 * C, dtype=n.dtype, device=n.device)
    extra = torch.empty(max(lvl.n_extra, 1), 2 * C, dtype=n.dtype, device=n.device)
    dtable = None
    if long_tiles(lvl):
        gq, bq, gk, bk = attention_long_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lvl.gidx, lvl.gidx, lvl.owner,
                                            lvl.self_tiles, lvl.self_blocks, lvl.n_self_tiles, qn, kn, att,
                                            datt, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, H, C // H, lvl.tile_max, attn_p,
                                            mix_seed(seed, 1), lvl.kext, lvl.ext_pos, lvl.n_extra, extra)
    elif rpe is None:
        gq, bq, gk, bk = attention_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lvl.gidx, lvl.gidx, lvl.owner,
                                       lvl.self_tiles, lvl.self_blocks, lvl.n_self_tiles, qn, kn, att,
                                       datt, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, 0, H, C // H, attn_p, mix_seed(seed, 1),
                                       lvl.kext, lvl.ext_pos, lvl.n_extra, extra)
    else:
        (gq, bq, gk, bk), dtable = attention_rpe_bwd(qkv, 3 * C, 0, qkv, 3 * C, C, 2 * C, lvl.gidx, lvl.gidx, lvl.owner,
                                                     lvl.self_tiles, lvl.self_blocks, lvl.n_self_tiles, qn, kn, att,
                                                     datt, lse, dqkv, 3 * C, 0, dqkv, 3 * C, C, 2 * C, 0, H, C // H, lvl.grid,
                                                     rpe[0], rpe[1], attn_p, mix_seed(seed, 1), lvl.kext, lvl.ext_pos,
                                                     lvl.n_extra, extra)
    dwqkv, dbqkv = linear_wgrad(dqkv, n)
    dcproj = coord_add_wgrad(dqkv, 2 * C, C, coord) if cmode == "qk" else None
    dn = linear_dgrad(dqkv, wqkv)
    if cmode == "qkv":
        dcproj = coord_add_wgrad(dn, C, C, coord)
    return dn, dwqkv, dbqkv, gq, bq, gk, bk, dwp, dbp, dcproj, dtable


def ffn_branch_fwd(n, x, w1, b1, w2, b2, drop_p, seed, dpath):
    """n = norm(x) -> (y, a, hpre), y = x + DropPath(drop(fc2(a))), a = drop(GELU(hpre)), hpre = fc1(n)."""
    a, hpre = linear_fwd(n, w1, b1, act=ACT_GELU, save_pre=True, drop_p=drop_p, seed=seed)
    if dpath > 0.0:
        br, _ = linear_fwd(a, w2, b2, drop_p=drop_p, seed=mix_seed(seed, 1))
        y = drop_path(br, x, dpath, mix_seed(seed, 5))
    else:
        y, _ = linear_fwd(a, w2, b2, residual=x, drop_p=drop_p, seed=mix_seed(seed, 1))
    return y, a, hpre


def ffn_branch_bwd(dy, n, hpre, a, w1, w2, p, seed, dpath, hand):
    """-> (dn, dw1, db1, dw2, db2); `hand` as in selfattn_branch_bwd."""
    dyb = drop_path(dy, None, dpath, mix_seed(seed, 5)) if dpath > 0.0 else dy
    dz2 = _masked(dyb, p, mix_seed(seed, 1), hand)
    dw2, db2 = linear_wgrad(dz2, a)
    dh = linear_dgrad(dz2, w2, pre=hpre, act=ACT_GELU, drop_p=p, seed=seed)
    dw1, db1 = linear_wgrad(dh, n)
    dn = linear_dgrad(dh, w1)
    return dn, dw1, db1, dw2, db2


def crossattn_branch_fwd(n, x, wq, bq, kv, qn, kn, wp, bp, lvl, H, drop_p, seed, attn_p, own=None):
    """n = LN(x), kv = [k | v] [L, 2C] (row stride free: a ProjBank slice) -> (y, q, att, lse, kv), y = x + drop(proj(CrossAttention(
    q(n), kv))).  own = (context, wkv, bkv) instead of kv: the block's own projection (CrossAttnFn), launched behind q's."""
    N, C = x.shape
    q, _ = linear_fwd(n, wq, bq)
    if own is not None:
        kv, _ = linear_fwd(*own)
    att = torch.empty(N, C, dtype=x.dtype, device=x.device)
    lse = torch.empty(N, H, dtype=torch.float32, device=x.device)
    attention_fwd(q, C, 0, kv, kv.stride(0), 0, C, None, None, None, lvl.ca_tiles, lvl.n_ca_tiles, qn, kn, att, lse, H, C // H,
                  attn_p, mix_seed(seed, 1), k_max=lvl.ca_kmax)
    y, _ = linear_fwd(att, wp, bp, residual=x, drop_p=drop_p, seed=seed)
    return y, q, att, lse, kv


def crossattn_branch_bwd(dy, n, q, kv, att, lse, wq, qn, kn, wp, lvl, H, p, seed, attn_p, hand, dkv=None, own=None):
    """-> (dn, dwq, dbq, gq, bq, gk, bk, dwp, dbp) + own's (dwkv, dbkv, dctx).  d kv goes to `dkv`, an [L, 2C] view (a ProjBank
    gradient slice): written by the attention backward itself when the level has one key-side slot, else summed into it by
    lotus_sum_slabs_ld.  own = (context, wkv, d context wanted) instead: the slots are summed into a fresh tensor (lotus_sum_slabs;
    one slot: the slab itself) and the kv products follow, in front of q's.  The composite entry points make the same choice of
    reduce kernel per path (csrc/blocks.cpp); the two kernels need not round alike."""
    N, C = n.shape
    dz = _masked(dy, p, seed, hand)
    dwp, dbp = linear_wgrad(dz, att)
    datt = linear_dgrad(dz, wp)
    dq = torch.empty(N, C, dtype=n.dtype, device=n.device)
    G, L = lvl.ca_groups, kv.shape[0]
    if own is not None or G > 1:
        part = torch.empty(G, L, 2 * C, dtype=n.dtype, device=n.device)
        tgt, tld, tps = part, 2 * C, L * 2 * C
    else:
        tgt, tld, tps = dkv, dkv.stride(0), 0
    gq, bq, gk, bk = attention_bwd(q, C, 0, kv, kv.stride(0), 0, C, None, None, None, lvl.ca_tiles, lvl.ca_blocks, lvl.n_ca_blocks,
                                   qn, kn, att, datt, lse, dq, C, 0, tgt, tld, 0, C, tps, 0, H, C // H, attn_p, mix_seed(seed, 1),
                                   k_max=lvl.ca_kmax)
    mine = ()
    if own is not None:
        context, wkv, want_dctx = own
        dkv = sum_slabs(part)
        mine = linear_wgrad(dkv, context) + (linear_dgrad(dkv, wkv) if want_dctx else None,)
    elif G > 1:
        call("lotus_sum_slabs_ld", part, dkv, L, 2 * C, dkv.stride(0), L * 2 * C, G)
    dwq, dbq = linear_wgrad(dq, n)
    dn = linear_dgrad(dq, wq)
    return (dn, dwq, dbq, gq, bq, gk, bk, dwp, dbp) + mine


class CpeFn(torch.autograd.Function):
    """x1 = x + LN(Linear(SubMConv3d_3(xs))).  In the encoder xs is x; in the decoder xs is the
    stale proj_skip branch (SURVEY.md Trap 3), hence two tensor inputs."""

    @_fwd
    def forward(ctx, x, xs, cw, cb, lw, lb, g, b, lvl, wt=None, mod=None, bank=None, j=0):
        same = xs is x
        if wt is None:
            wt = conv_weight_t(cw)
        ctx.lvl, ctx.same, ctx.site = lvl, same, (bank, j)
        n_, C = x.shape
        (lwk,), pc = _wk(lw)
        ctx.wk, ctx.pc = (lwk,), pc
        ctx.comp = (mod is None and composites_enabled() and C % 64 == 0 and (C == 64 or C % 128 == 0) and cw.shape[0] == C
                    and cw.shape[-1] == C)
        if ctx.comp:
            n_saved, _, _, ws_main, _, ws_conv = _sizes("cpe", n_, C)
            saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
            y = torch.empty_like(x)
            ws = _ws(ws_main, x.device)
            wc = WS.get(ws_conv, x.device, slot=2)
            _capi.call_raw("lotus_cpe_fwd", x, xs, cw, wt, cb, lwk, lb, g, b, y, saved, lvl.nbr27, lvl.order[0], lvl.tap_plan, n_, C, pc, ws,
                           ws.numel(), wc, wc.numel(), _counters(x.device), _capi.stream_ptr())
            ctx.save_for_backward(xs, cw, lw, g, saved, wt)
            return y
        c, l = cpe_branch_fwd(xs, cw, cb, lwk, lb, lvl, wt)
        y, mean, rstd = ln_fwd(l, g, b, res=x, mod=mod, lvl=lvl)
        ctx.save_for_backward(xs, cw, lw, g, c, l, mean, rstd, wt, b, mod)
        return y

    @_joined
    def backward(ctx, dy):
        lvl = ctx.lvl
        dy = dy.contiguous()
        if ctx.comp:
            xs, cw, lw, g, saved, wt = ctx.saved_tensors
            n_, C = xs.shape
            dev = xs.device
            _, n_grads, n_tmp, ws_main, ws_side, ws_conv = _sizes("cpe", n_, C)
            grads, tmp, wsm, side, wss, wss_bytes, cs = _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, (saved, xs, lvl.nbr27), n_)
            dxc = torch.empty_like(xs)
            wc = WS.get(ws_conv, dev, slot=2)
            _capi.call_raw("lotus_cpe_bwd", dy, xs, cw, wt, ctx.wk[0], g, saved, dxc, 1 if ctx.same else 0, grads, tmp, lvl.nbr27,
                           lvl.order[0], lvl.tap_plan, lvl.code[0], lvl.n_dup, n_, C, ctx.pc, wsm, wsm.numel(), wc, wc.numel(), wss,
                           wss_bytes, _counters(dev), cs, _LINK, 0, _capi.stream_ptr(), side)
            return ((dxc, None) if ctx.same else (dy, dxc)) + _grad_views(grads, "cpe", C, cshape=cw.shape) + (None,) * 5
        xs, cw, lw, g, c, l, mean, rstd, wt, b, mod = ctx.saved_tensors
        dmod = _dmod(mod, ctx.site)
        dl, dg, db = ln_bwd(dy, l, mean, rstd, g, b=b, mod=mod, dmod=dmod, lvl=lvl)
        return cpe_branch_bwd(dl, dy, xs, cw, ctx.wk[0], c, lvl, wt, ctx.same) + (dg, db, None, None, dmod, None, None)


class FfnFn(torch.autograd.Function):
    """y = x + drop(fc2(drop(GELU(fc1(LN(x))))))   (MLP, model.py:577-583; pre-norm residual)."""

    @_fwd
    def forward(ctx, x, g, b, w1, b1, w2, b2, drop_p, seed, hand_in=None, hand_out=None, dpath=0.0, lvl=None, mod=None, bank=None,
                j=0):
        # dpath > 0: DropPath on the branch (Block.mlp only, training only; model.py:672) — its own elementwise pass, the
        # per-launch path, no hand-over of a pre-masked gradient (the published models train with drop_path 0)
        ctx.drop = (drop_p, seed)
        ctx.dpath = float(dpath)
        if dpath > 0.0:
            hand_in = None
        ctx.hands = (hand_in, hand_out)
        if hand_in is not None:
            hand_in.arm(drop_p, mix_seed(seed, 1))
        ctx.lvl, ctx.site = lvl, (bank, j)  # (lvl: the level whose clouds modulate, with `mod` only)
        ctx.comp = mod is None and composites_enabled() and x.shape[1] % 4 == 0 and dpath == 0.0
        (w1k, w2k), pc = _wk(w1, w2)
        ctx.wk, ctx.pc = (w1k, w2k), pc
        if ctx.comp:
            M, C = x.shape
            Hd = w1.shape[0]
            n_saved, _, _, ws_main, _ = _sizes("ffn", M, C, Hd)
            saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
            y = torch.empty_like(x)
            ws = _ws(ws_main, x.device)
            _capi.call_raw("lotus_ffn_fwd", x, g, b, w1k, b1, w2k, b2, y, saved, M, C, Hd, float(drop_p), int(seed),
                           mix_seed(seed, 1), pc, ws, ws.numel(), _counters(x.device), _capi.stream_ptr())
            ctx.save_for_backward(x, g, w1, w2, saved)
            return y
        n, mean, rstd = ln_fwd(x, g, b, mod=mod, lvl=lvl)
        y, a, hpre = ffn_branch_fwd(n, x, w1k, b1, w2k, b2, drop_p, seed, dpath)
        ctx.save_for_backward(x, g, w1, w2, n, hpre, a, mean, rstd, b, mod)
        return y

    @_joined
    def backward(ctx, dy):
        p, seed = ctx.drop
        hand_in, hand_out = ctx.hands
        dy = dy.contiguous()
        if ctx.comp:
            x, g, w1, w2, saved = ctx.saved_tensors
            M, C = x.shape
            Hd, dev = w1.shape[0], x.device
            _, n_grads, n_tmp, ws_main, ws_side = _sizes("ffn", M, C, Hd)
            dz_in = hand_in.take(dy) if hand_in is not None else None
            grads, tmp, wsm, side, wss, wss_bytes, cs = _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, (saved, dy, dz_in), M)
            dx = torch.empty_like(x)
            dz_out, po, so = Handoff.offer(hand_out, dx)
            _capi.call_raw("lotus_ffn_bwd", dy, dz_in, x, g, ctx.wk[0], ctx.wk[1], saved, dx, dz_out, po, so, grads, tmp, M, C, Hd, float(p),
                           int(seed), mix_seed(seed, 1), ctx.pc, wsm, wsm.numel(), wss, wss_bytes, _counters(dev), cs, _LINK, 0,
                           _capi.stream_ptr(), side)
            return (dx,) + _grad_views(grads, "ffn", C, Hd=Hd) + (None,) * 9
        x, g, w1, w2, n, hpre, a, mean, rstd, b, mod = ctx.saved_tensors
        dn, dw1, db1, dw2, db2 = ffn_branch_bwd(dy, n, hpre, a, ctx.wk[0], ctx.wk[1], p, seed, ctx.dpath, hand_in)
        dmod = _dmod(mod, ctx.site)
        dx, dg, db = ln_bwd(dn, x, mean, rstd, g, add=dy, hand=hand_out, b=b, mod=mod, dmod=dmod, lvl=ctx.lvl)
        return (dx, dg, db, dw1, db1, dw2, db2) + (None,) * 6 + (dmod, None, None)


class SelfAttnFn(torch.autograd.Function):
    """y = x + drop(proj(PatchAttention(qkv(LN(x)))))   (SerializedAttention flash path)."""

    @_fwd
    def forward(ctx, x, g, b, wqkv, bqkv, qnw, qnb, knw, knb, wp, bp, lvl, H, drop_p, seed, attn_p=0.0, hand_in=None, dpath=0.0,
                mod=None, bank=None, j=0, coord=None, cproj=None, cmode=None, rpe_table=None, rpe_bnd=0):
        """qnw = qnb = knw = knb = None: a block without q_norm / k_norm (qk_norm False).  coord / cproj / cmode: the level's
        float coordinates [N, 3], coords_proj.weight [C, 3] and 'qk' | 'qkv' (add_coords_in_attn, model.py:484-495); the node then
        runs per launch, fp32 storage.  rpe_table / rpe_bnd: rpe.rpe_table [3 (2 bnd + 1), H] and pos_bnd (enable_rpe,
        model.py:307-326): the same rule — per launch, fp32 storage and exact-fp32 operands."""
        N, C = x.shape
        d = C // H
        ctx.meta = (lvl, H, d, drop_p, seed, attn_p)
        ctx.dpath = float(dpath)  # DropPath on the branch (model.py:666), see FfnFn
        if dpath > 0.0:
            hand_in = None
        ctx.hand_in = hand_in
        if hand_in is not None:
            hand_in.arm(drop_p, seed)
        ctx.site = (bank, j)
        ctx.comp = (coord is None and rpe_table is None and mod is None and qnw is not None and composites_enabled() and C % 4 == 0
                    and dpath == 0.0 and not long_tiles(lvl))  # (tiles above 128 rows: per launch, as the coordinate and RPE terms)
        if long_tiles(lvl) and _capi.BF16:
            raise NotImplementedError("patch sizes above 128 run with fp32 activation storage only")
        ctx.cmode = None
        if coord is not None:
            if cmode not in ("qk", "qkv") or cproj is None:
                raise ValueError(f"SelfAttnFn: coord needs cproj and cmode 'qk' | 'qkv', got cmode={cmode!r}")
            if _capi.BF16:
                raise NotImplementedError("add_coords_in_attn runs with fp32 activation storage only")
            ctx.cmode = cmode
        ctx.rpe_bnd = None
        if rpe_table is not None:
            if _capi.BF16:
                raise NotImplementedError("enable_rpe runs with fp32 activation storage only")
            if rpe_table.shape != (3 * (2 * int(rpe_bnd) + 1), H):
                raise ValueError(f"SelfAttnFn: rpe_table {tuple(rpe_table.shape)} is not [3 (2 bnd + 1), H] for bnd={rpe_bnd}, H={H}")
            ctx.rpe_bnd = int(rpe_bnd)
        (wqkvk, wpk), pc = _wk(wqkv, wp)
        ctx.wk, ctx.pc = (wqkvk, wpk), pc
        if ctx.comp:
            n_saved, _, _, ws_main, _ = _sizes("self", N, C, H, lvl.npad, lvl.n_self_tiles, lvl.n_extra)
            saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
            y = torch.empty_like(x)
            ws = _ws(ws_main, x.device)
            _capi.call_raw("lotus_selfattn_fwd", x, g, b, wqkvk, bqkv, qnw, qnb, knw, knb, wpk, bp, y, saved, lvl.gidx, lvl.owner,
                           lvl.self_tiles, lvl.n_self_tiles, lvl.npad, N, C, H, float(d ** -0.5), float(drop_p), int(seed),
                           float(attn_p), mix_seed(seed, 1), pc, ws, ws.numel(), _counters(x.device), _capi.stream_ptr())
            ctx.save_for_backward(x, g, wqkv, qnw, qnb, knw, knb, wp, saved)
            return y
        n, mean, rstd = ln_fwd(x, g, b, mod=mod, lvl=lvl)
        qn, kn = ((qnw, qnb), (knw, knb)) if qnw is not None else (None, None)
        y, qkv, att, lse = selfattn_branch_fwd(n, x, wqkvk, bqkv, qn, kn, wpk, bp, lvl, H, drop_p, seed, attn_p, dpath,
                                               coord, cproj, ctx.cmode,
                                               None if rpe_table is None else (rpe_table, ctx.rpe_bnd))
        ctx.coord = coord  # (no gradient flows to it: kept as an attribute, like the level's tables)
        ctx.save_for_backward(x, g, wqkv, qnw, qnb, knw, knb, wp, n, qkv, att, lse, mean, rstd, b, mod, rpe_table)
        return y

    @_joined
    def backward(ctx, dy):
        lvl, H, d, p, seed, attn_p = ctx.meta
        dy = dy.contiguous()
        if ctx.comp:
            x, g, wqkv, qnw, qnb, knw, knb, wp, saved = ctx.saved_tensors
            N, C = x.shape
            dev = x.device
            _, n_grads, n_tmp, ws_main, ws_side = _sizes("self", N, C, H, lvl.npad, lvl.n_self_tiles, lvl.n_extra)
            dz_in = ctx.hand_in.take(dy) if ctx.hand_in is not None else None
            grads, tmp, wsm, side, wss, wss_bytes, cs = _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, (saved, dy, dz_in), N)
            dx = torch.empty_like(x)
            _capi.call_raw("lotus_selfattn_bwd", dy, dz_in, x, g, ctx.wk[0], qnw, qnb, knw, knb, ctx.wk[1], saved, dx, grads, tmp, lvl.gidx,
                           lvl.owner, lvl.self_tiles, lvl.self_blocks, lvl.n_self_tiles, lvl.kext, lvl.ext_pos, lvl.n_extra, lvl.npad,
                           N, C, H, float(d ** -0.5), float(p), int(seed), float(attn_p), mix_seed(seed, 1), ctx.pc, wsm, wsm.numel(),
                           wss, wss_bytes, _counters(dev), cs, _LINK, 0, _capi.stream_ptr(), side)
            return (dx,) + _grad_views(grads, "self", C, H) + (None,) * 15
        x, g, wqkv, qnw, qnb, knw, knb, wp, n, qkv, att, lse, mean, rstd, b, mod, rpe_table = ctx.saved_tensors
        qn, kn = ((qnw, qnb), (knw, knb)) if qnw is not None else (None, None)
        rpe = None if rpe_table is None else (rpe_table, ctx.rpe_bnd)
        dn, dwqkv, dbqkv, gq, bq, gk, bk, dwp, dbp, dcproj, dtable = selfattn_branch_bwd(
            dy, n, qkv, att, lse, ctx.wk[0], qn, kn, ctx.wk[1], lvl, H, p, seed, attn_p, ctx.dpath, ctx.hand_in, ctx.coord, ctx.cmode,
            rpe)
        dmod = _dmod(mod, ctx.site)
        dx, dg, db = ln_bwd(dn, x, mean, rstd, g, add=dy, b=b, mod=mod, dmod=dmod, lvl=lvl)
        return (dx, dg, db, dwqkv, dbqkv, gq, bq, gk, bk, dwp, dbp) + (None,) * 7 + (dmod, None, None, None, dcproj, None, dtable, None)


class CrossAttnFn(torch.autograd.Function):
    """y = x + drop(proj(CrossAttention(q(LN(x)), kv(context))))   (model_ca.py:46-101, :135-140)."""

    @_fwd
    def forward(ctx, x, context, g, b, wq, bq, wkv, bkv, qnw, qnb, knw, knb, wp, bp, lvl, H, drop_p, seed, attn_p=0.0,
                hand_in=None, hand_out=None):
        N, C = x.shape
        d = C // H
        ctx.meta = (lvl, H, d, drop_p, seed, attn_p)
        ctx.hands = (hand_in, hand_out)
        if hand_in is not None:
            hand_in.arm(drop_p, seed)
        ctx.comp = composites_enabled() and C % 4 == 0
        (wqk, wkvk, wpk), pc = _wk(wq, wkv, wp)
        ctx.wk, ctx.pc = (wqk, wkvk, wpk), pc
        if ctx.comp:
            L, Cc = context.shape
            n_saved, _, _, ws_main, _ = _sizes("cross", N, C, H, L, Cc, lvl.n_ca_blocks, lvl.ca_groups)
            saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
            y = torch.empty_like(x)
            ws = _ws(ws_main, x.device)
            _capi.call_raw("lotus_crossattn_fwd", x, context, g, b, wqk, bq, wkvk, bkv, qnw, qnb, knw, knb, wpk, bp, y, saved,
                           lvl.ca_tiles, lvl.n_ca_tiles, N, C, H, L, Cc, float(d ** -0.5), float(drop_p), int(seed), float(attn_p),
                           mix_seed(seed, 1), pc, lvl.ca_kmax, ws, ws.numel(), _counters(x.device), _capi.stream_ptr())
            ctx.save_for_backward(x, context, g, wq, wkv, qnw, qnb, knw, knb, wp, saved)
            return y
        n, mean, rstd = ln_fwd(x, g, b)
        y, q, att, lse, kv = crossattn_branch_fwd(n, x, wqk, bq, None, (qnw, qnb), (knw, knb), wpk, bp, lvl, H, drop_p, seed, attn_p,
                                                  own=(context, wkvk, bkv))
        ctx.save_for_backward(x, context, g, wq, wkv, qnw, qnb, knw, knb, wp, n, q, kv, att, lse, mean, rstd)
        return y

    @_joined
    def backward(ctx, dy):
        lvl, H, d, p, seed, attn_p = ctx.meta
        hand_in, hand_out = ctx.hands
        dy = dy.contiguous()
        if ctx.comp:
            x, context, g, wq, wkv, qnw, qnb, knw, knb, wp, saved = ctx.saved_tensors
            N, C = x.shape
            L, Cc = context.shape
            dev, G = x.device, lvl.ca_groups
            _, n_grads, n_tmp, ws_main, ws_side = _sizes("cross", N, C, H, L, Cc, lvl.n_ca_blocks, G)
            dz_in = hand_in.take(dy) if hand_in is not None else None
            grads, tmp, wsm, side, wss, wss_bytes, cs = _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, (saved, dy, dz_in, context), N)
            dx = torch.empty_like(x)
            dctx = torch.empty_like(context) if ctx.needs_input_grad[1] else None
            dz_out, po, so = Handoff.offer(hand_out, dx)
            _capi.call_raw("lotus_crossattn_bwd", dy, dz_in, x, context, g, ctx.wk[0], ctx.wk[1], qnw, qnb, knw, knb, ctx.wk[2], saved, dx, dctx, dz_out,
                           po, so, grads, tmp, lvl.ca_tiles, lvl.ca_blocks, lvl.n_ca_blocks, G, N, C, H, L, Cc, float(d ** -0.5),
                           float(p), int(seed), float(attn_p), mix_seed(seed, 1), ctx.pc, lvl.ca_kmax, wsm, wsm.numel(), wss,
                           wss_bytes, _counters(dev), cs, _LINK, 0, _capi.stream_ptr(), side)
            return (dx, dctx) + _grad_views(grads, "cross", C, H, Cc=Cc) + (None,) * 7
        x, context, g, wq, wkv, qnw, qnb, knw, knb, wp, n, q, kv, att, lse, mean, rstd = ctx.saved_tensors
        dn, dwq, dbq, gq, bq_, gk, bk_, dwp, dbp, dwkv, dbkv, dctx = crossattn_branch_bwd(
            dy, n, q, kv, att, lse, ctx.wk[0], (qnw, qnb), (knw, knb), ctx.wk[2], lvl, H, p, seed, attn_p, hand_in,
            own=(context, ctx.wk[1], ctx.needs_input_grad[1]))
        dx, dg, db = ln_bwd(dn, x, mean, rstd, g, add=dy, hand=hand_out)
        return dx, dctx, dg, db, dwq, dbq, dwkv, dbkv, gq, bq_, gk, bk_, dwp, dbp, None, None, None, None, None, None, None


class ProjBank:
    """Projections of ONE shared context for every consumer of a forward pass (ProjAllFn): `slab` [rows, sum w_j] holds consumer
    j's in columns offs[j] : offs[j] + widths[j] (`slices[j]`); `dslab` (same shape, allocated by the first backward that needs
    it) collects the gradients, each consumer's backward writing its own column slice.  The consumers: the CABlocks (their keys /
    values, ptv3) or the PDNorms ([shift | scale], adanorm)."""
    __slots__ = ("slab", "dslab", "offs", "widths", "slices")

    def slice(self, j):
        return self.slices[j]

    def grad_slice(self, j):
        if self.dslab is None:
            self.dslab = torch.empty_like(self.slab)
        return self.dslab[:, self.offs[j]:self.offs[j] + self.widths[j]]


class ProjAllFn(torch.autograd.Function):
    """slice_j = Linear_j(pre(context)) for every consumer j in ONE product, pre(context) [rows, Cc] x cat(W_j) [sum w_j, Cc];
    pre = None, or "silu" (the PDNorm modulations).  model_ca.py:46-67 evaluates the nine [L, 256] x [256, 2C_b] kv products one
    by one, each 3 row tiles tall; v1's 40 PDNorms are 24 064 columns.  The weights stay the modules' own parameters; their
    concatenation is one copy launch per step.  Returns the column slices (views of one slab).  Backward: one weight-gradient and
    one input-gradient product over the gradient slab that the consumers' backward passes filled."""

    @_fwd
    def forward(ctx, context, bank, pre, *wb):
        # (shadows, precision 5, exist under bf16 storage only; the AdaNorm models are fp32: "silu" always reads the masters)
        assert pre is None or (pre == "silu" and not _capi.BF16), pre
        ws, bs = wb[0::2], wb[1::2]
        wks, _ = _wk(*ws)   # (bf16 storage with weight shadows: the concatenation of the shadows, half the copy)
        W = torch.cat(wks, 0)
        bias = torch.cat(bs, 0)
        s = silu(context) if pre else context
        slab, _ = linear_fwd(s, W, bias)
        bank.slab, bank.dslab = slab, None
        bank.widths = [w.shape[0] for w in ws]
        bank.offs = [0]
        for w_ in bank.widths[:-1]:
            bank.offs.append(bank.offs[-1] + w_)
        bank.slices = tuple(slab[:, o:o + w_] for o, w_ in zip(bank.offs, bank.widths))
        ctx.bank, ctx.pre = bank, pre
        ctx.save_for_backward(context, s, W)
        return bank.slices

    @_joined
    def backward(ctx, *gs):
        context, s, W = ctx.saved_tensors
        bank = ctx.bank
        for j, g in enumerate(gs):  # normally every g IS its slice of the slab (written in place by the consumer's backward)
            sl = bank.grad_slice(j)
            if g is None:
                sl.zero_()
            elif g.data_ptr() != sl.data_ptr() or g.stride() != sl.stride():
                sl.copy_(g)
        dslab = bank.dslab
        dW, db = linear_wgrad(dslab, s)
        dctx = linear_dgrad(dslab, W) if ctx.needs_input_grad[0] else None
        out = [silu(context, dctx) if ctx.pre and dctx is not None else dctx, None, None]
        for o, w_ in zip(bank.offs, bank.widths):
            out += [dW[o:o + w_], db[o:o + w_]]
        bank.dslab = None
        return tuple(out)


class CrossAttnKvFn(torch.autograd.Function):
    """CrossAttnFn with the keys / values taken from a ProjBank slice (projected once for all blocks by ProjAllFn):
    y = x + drop(proj(CrossAttention(q(LN(x)), kv)))   (model_ca.py:46-101, :135-140)."""

    @_fwd
    def forward(ctx, x, kv, g, b, wq, bq, qnw, qnb, knw, knb, wp, bp, lvl, H, drop_p, seed, attn_p, hand_in, hand_out, bank, bidx):
        N, C = x.shape
        d = C // H
        ctx.meta = (lvl, H, d, drop_p, seed, attn_p, bank, bidx)
        ctx.hands = (hand_in, hand_out)
        if hand_in is not None:
            hand_in.arm(drop_p, seed)
        L, kv_ld = kv.shape[0], kv.stride(0)
        ctx.comp = composites_enabled() and C % 4 == 0
        (wqk, wpk), pc = _wk(wq, wp)
        ctx.wk, ctx.pc = (wqk, wpk), pc
        if ctx.comp:
            n_saved, _, _, ws_main, _ = _sizes("crosskv", N, C, H, L, lvl.n_ca_blocks, lvl.ca_groups)
            saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
            y = torch.empty_like(x)
            ws = _ws(ws_main, x.device)
            _capi.call_raw("lotus_crossattn_kv_fwd", x, kv, kv_ld, g, b, wqk, bq, qnw, qnb, knw, knb, wpk, bp, y, saved, lvl.ca_tiles,
                           lvl.n_ca_tiles, N, C, H, float(d ** -0.5), float(drop_p), int(seed), float(attn_p), mix_seed(seed, 1), pc,
                           lvl.ca_kmax, ws, ws.numel(), _counters(x.device), _capi.stream_ptr())
            ctx.save_for_backward(x, kv, g, wq, qnw, qnb, knw, knb, wp, saved)
            return y
        n, mean, rstd = ln_fwd(x, g, b)
        y, q, att, lse, _ = crossattn_branch_fwd(n, x, wqk, bq, kv, (qnw, qnb), (knw, knb), wpk, bp, lvl, H, drop_p, seed, attn_p)
        ctx.save_for_backward(x, kv, g, wq, qnw, qnb, knw, knb, wp, n, q, att, lse, mean, rstd)
        return y

    @_joined
    def backward(ctx, dy):
        lvl, H, d, p, seed, attn_p, bank, bidx = ctx.meta
        hand_in, hand_out = ctx.hands
        dy = dy.contiguous()
        dkv = bank.grad_slice(bidx)
        if ctx.comp:
            x, kv, g, wq, qnw, qnb, knw, knb, wp, saved = ctx.saved_tensors
            N, C = x.shape
            L, dev, G = kv.shape[0], x.device, lvl.ca_groups
            _, n_grads, n_tmp, ws_main, ws_side = _sizes("crosskv", N, C, H, L, lvl.n_ca_blocks, G)
            dz_in = hand_in.take(dy) if hand_in is not None else None
            grads, tmp, wsm, side, wss, wss_bytes, cs = _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, (saved, dy, dz_in), N)
            dx = torch.empty_like(x)
            dz_out, po, so = Handoff.offer(hand_out, dx)
            _capi.call_raw("lotus_crossattn_kv_bwd", dy, dz_in, x, kv, kv.stride(0), g, ctx.wk[0], qnw, qnb, knw, knb, ctx.wk[1], saved, dx, dkv,
                           dkv.stride(0), dz_out, po, so, grads, tmp, lvl.ca_tiles, lvl.ca_blocks, lvl.n_ca_blocks, G, N, C, H, L,
                           float(d ** -0.5), float(p), int(seed), float(attn_p), mix_seed(seed, 1), ctx.pc, lvl.ca_kmax, wsm, wsm.numel(),
                           wss, wss_bytes, _counters(dev), cs, _LINK, 0, _capi.stream_ptr(), side)
            return (dx, dkv) + _grad_views(grads, "crosskv", C, H) + (None,) * 9
        x, kv, g, wq, qnw, qnb, knw, knb, wp, n, q, att, lse, mean, rstd = ctx.saved_tensors
        dn, dwq, dbq, gq, bq_, gk, bk_, dwp, dbp = crossattn_branch_bwd(
            dy, n, q, kv, att, lse, ctx.wk[0], (qnw, qnb), (knw, knb), ctx.wk[1], lvl, H, p, seed, attn_p, hand_in, dkv=dkv)
        dx, dg, db = ln_bwd(dn, x, mean, rstd, g, add=dy, hand=hand_out)
        return (dx, dkv, dg, db, dwq, dbq, gq, bq_, gk, bk_, dwp, dbp) + (None,) * 9


# ------------------------------------------------------------------------------------ (Block, CABlock) pair in one call
# "auto" (default): the pair node is used where the host, not the GPU, sets the pace — bf16 storage, and every stage whose
# LEVEL holds fewer than ~40 k points (round 6: decided per stage, not per step: 7 of the 9 stages of the 16 x 4096 step, host
# floor 10.8 -> 8.0 ms per step at unchanged throughput, 1 083.3 against 1 083.4 samples/s — a process on a slow host stays
# GPU-bound) — and the five sub-block nodes on the large levels.  Measured on MI355X (A/B inside one call): the pair node lowers
# the host's enqueue time per step from 12.1 to 8.4 ms and lifts the PerAct bf16 step at 16 clouds from 1216-1356 to
# 1447-1452 samples/s, but costs the fp32 step at 16 x 4096 points 1.5 % (880 -> 866): its temporaries of all five
# sub-blocks are one allocation per pair, while separate nodes hand the same few hundred MB back to the allocator and get
# them again for the next sub-block (smaller live footprint in the 256 MB Infinity Cache / TLB).
_PAIR = {"0": False, "1": True}.get(os.environ.get("LOTUS_PAIR", "auto"), "auto")
_PAIR_AUTO_ROWS = 40000
_PP = None  # name -> index tables of the pair's argument arrays, from the library's own lists (csrc/blocks.cpp PAIR_PTRS / PAIR_INTS)
# parameter slots of PairFn in call order -> their names in the library's pointer list
_PAIR_PARAM_SLOTS = ("CW CB LW LB G0 B0 G1 B1 WQKV BQKV QNW QNB KNW KNB WP BP G2 B2 W1 B1F W2 B2F G3 B3 WQ BQ CQNW CQNB CKNW CKNB CWP2 CBP2 "
                     "G4 B4 W3 B3F W4 B4F").split()
_PAIR_LINEAR = (2, 8, 14, 18, 20, 24, 30, 34, 36)   # indices (in that order) of the dense-layer weights: candidates for bf16 shadows


def pair_enabled(rows, rows0=None):
    """rows: points of the level the stage runs on, rows0: points of the step's input level (the "auto" rule looks at them)."""
    if not composites_enabled():
        return False
    if _PAIR == "auto":
        if _capi.BF16:
            return True
        if BnState.reduce is not None or GRAD_ARENA is not None:
            # data parallel: the pair node hands its 38 gradients to the reducer at once, the buckets leave in bursts (one-rank
            # rehearsal 1 055-1 056 against 1 058-1 062 samples/s) — per step as in round 5
            return (rows if rows0 is None else rows0) <= _PAIR_AUTO_ROWS
        return rows <= _PAIR_AUTO_ROWS
    return _PAIR


def set_pair(on):
    """True / False, or "auto" (see above)."""
    global _PAIR
    _PAIR = on if on == "auto" else bool(on)


def _pair_tables():
    global _PP
    if _PP is None:
        import numpy as np
        names = [query(q) for q in ("lotus_pair_ptr_names", "lotus_pair_int_names")]
        pp, pi = ({n: i for i, n in enumerate((s if isinstance(s, str) else s.decode()).split())} for s in names)
        _PP = (np, pp, pi, [pp[n] for n in _PAIR_PARAM_SLOTS])   # (a slot name the library does not list: KeyError with the name)
    return _PP


class PairFn(torch.autograd.Function):
    """Block i + CABlock i of a stage (model_ca.py:270-310) as ONE autograd node over csrc/blocks.cpp lotus_pair_fwd / _bwd:
    the launches of CpeFn -> SelfAttnFn -> FfnFn -> CrossAttnKvFn -> FfnFn in the same order on the same streams
    (bit-identical, tests/test_gpu_round4.py), one Python -> C transition and one set of buffers per direction.
    Inputs: x, xs (x itself in the encoder, the stale skip branch for the first Block of a decoder stage), the block's
    ProjBank slice, the packed convolution weights, the 38 parameters in _PAIR_PARAM_SLOTS order, and a meta tuple."""

    @_fwd
    def forward(ctx, x, xs, kv, wt, *rest):
        np, PP, PI, slots = _pair_tables()
        params, meta = rest[:38], rest[38]
        lvl, lvl_ca, H, Hd, drop_p, attn_p, s_self, s_f1, s_cross, s_f2, bank, bidx = meta
        M, C = x.shape
        L = kv.shape[0]
        same = xs is x
        dev = x.device
        n_acts, n_saved, n_grads, n_tmp, ws_main, ws_side, ws_conv = _sizes(
            "pair", M, C, H, Hd, lvl.npad, lvl.n_self_tiles, lvl.n_extra, L, lvl_ca.n_ca_blocks, lvl_ca.ca_groups)
        acts = torch.empty(n_acts, dtype=torch.float32, device=dev)
        saved = torch.empty(n_saved, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        ws = _ws(ws_main, dev)
        wc = WS.get(ws_conv, dev, slot=2)
        # dense-layer weights: bf16 shadows when this forward runs in shadow mode and every one of them has a shadow
        lin = [params[i] for i in _PAIR_LINEAR]
        link, pc = _wk(*lin)
        P = np.zeros(len(PP), dtype=np.uint64)
        I = np.zeros(len(PI), dtype=np.uint64)
        for slot, t in zip(slots, params):
            P[slot] = t.data_ptr()
        for i, t in zip(_PAIR_LINEAR, link):
            P[slots[i]] = t.data_ptr()
        P[PP["X"]], P[PP["XS"]], P[PP["KV"]], P[PP["Y"]] = x.data_ptr(), xs.data_ptr(), kv.data_ptr(), y.data_ptr()
        P[PP["ACTS"]], P[PP["SAVED"]], P[PP["CWP"]] = acts.data_ptr(), saved.data_ptr(), wt.data_ptr()
        P[PP["NBR27"]], P[PP["ORDER0"]], P[PP["CODE0"]] = lvl.nbr27.data_ptr(), lvl.order[0].data_ptr(), lvl.code[0].data_ptr()
        P[PP["TAPPLAN"]] = lvl.tap_plan.data_ptr() if lvl.tap_plan is not None else 0
        P[PP["GIDX"]], P[PP["OWNER"]], P[PP["STILES"]] = lvl.gidx.data_ptr(), lvl.owner.data_ptr(), lvl.self_tiles.data_ptr()
        P[PP["SBLOCKS"]], P[PP["KEXT"]], P[PP["EXTPOS"]] = lvl.self_blocks.data_ptr(), lvl.kext.data_ptr(), lvl.ext_pos.data_ptr()
        P[PP["CATILES"]], P[PP["CABLOCKS"]] = lvl_ca.ca_tiles.data_ptr(), lvl_ca.ca_blocks.data_ptr()
        P[PP["WS_MAIN"]], P[PP["WS_CONV"]] = ws.data_ptr(), wc.data_ptr()
        P[PP["CNT_MAIN"]], P[PP["STREAM"]] = _counters(dev).data_ptr(), _capi.stream_ptr()
        for k, v_ in (("M", M), ("C", C), ("H", H), ("HD", Hd), ("NPAD", lvl.npad), ("NSTILES", lvl.n_self_tiles),
                      ("NEXTRA", lvl.n_extra), ("L", L), ("NCATILES", lvl_ca.n_ca_tiles), ("NCABLOCKS", lvl_ca.n_ca_blocks),
                      ("G", lvl_ca.ca_groups), ("KMAX", lvl_ca.ca_kmax), ("NDUP", lvl.n_dup & 0xFFFFFFFF), ("SAME", 1 if same else 0),
                      ("PREC", pc), ("KV_LD", kv.stride(0)), ("WS_MAIN", ws.numel()), ("WS_CONV", wc.numel()),
                      ("SEED_SELF", s_self), ("SEED_FFN1", s_f1), ("SEED_CROSS", s_cross), ("SEED_FFN2", s_f2)):
            I[PI[k]] = v_
        F = np.array([float(drop_p), float(attn_p), float((C // H) ** -0.5)], dtype=np.float64)
        _capi.call_raw("lotus_pair_fwd", P.ctypes.data, I.ctypes.data, F.ctypes.data)
        ctx.save_for_backward(xs, kv, wt, acts, saved)
        ctx.keep = (params, link)   # parameters (leaves) and their shadows: referenced, not version-tracked
        ctx.tabs = (P, I, F)
        ctx.meta = (lvl, lvl_ca, H, Hd, same, bank, bidx, M, C, L)
        return y

    @_joined
    def backward(ctx, dy):
        np, PP, PI, slots = _pair_tables()
        xs, kv, wt, acts, saved = ctx.saved_tensors
        params, _ = ctx.keep
        lvl, lvl_ca, H, Hd, same, bank, bidx, M, C, L = ctx.meta
        P, I, F = ctx.tabs
        dev = xs.device
        dy = dy.contiguous()
        _, _, n_grads, n_tmp, ws_main, ws_side, ws_conv = _sizes(
            "pair", M, C, H, Hd, lvl.npad, lvl.n_self_tiles, lvl.n_extra, L, lvl_ca.n_ca_blocks, lvl_ca.ca_groups)
        grads, tmp, wsm, side, wss, wss_bytes, cs = _bwd_buffers(n_grads, n_tmp, ws_main, ws_side, dev, (saved, acts, dy, xs, kv, lvl.nbr27), M)
        dx = torch.empty_like(dy)
        dxs = None if same else torch.empty_like(xs)
        dkv = bank.grad_slice(bidx)
        wc = WS.get(ws_conv, dev, slot=2)
        P[PP["DY"]], P[PP["DX"]], P[PP["DXS"]] = dy.data_ptr(), dx.data_ptr(), (0 if dxs is None else dxs.data_ptr())
        P[PP["DKV"]], P[PP["GRADS"]], P[PP["TMP"]] = dkv.data_ptr(), grads.data_ptr(), tmp.data_ptr()
        P[PP["WS_MAIN"]], P[PP["WS_CONV"]], P[PP["WS_SIDE"]] = wsm.data_ptr(), wc.data_ptr(), (0 if wss is None else wss.data_ptr())
        P[PP["CNT_MAIN"]], P[PP["CNT_SIDE"]] = _counters(dev).data_ptr(), (0 if cs is None else cs.data_ptr())
        P[PP["STREAM"]], P[PP["SIDE"]] = _capi.stream_ptr(), side
        I[PI["WS_MAIN"]], I[PI["WS_CONV"]], I[PI["WS_SIDE"]] = wsm.numel(), wc.numel(), wss_bytes
        I[PI["DKV_LD"]], I[PI["LINK"]] = dkv.stride(0), _LINK
        _capi.call_raw("lotus_pair_bwd", P.ctypes.data, I.ctypes.data, F.ctypes.data)
        return (dx, dxs, dkv, None) + _grad_views(grads, "pair", C, H, Hd, cshape=params[0].shape) + (None,)


class StemFn(torch.autograd.Function):
    """Embedding: GELU(BN(SubMConv3d_5(x)))   (model.py:844-861; conv has no bias)."""

    @_fwd
    def forward(ctx, x, cw, g, b, rmean, rvar, lvl, training, mod=None, bank=None, j=0):
        c = conv_fwd(x, cw, None, lvl.nbr125, lvl.order[0])
        y, mean, invstd = bn_fwd(c, g, b, rmean, rvar, training, ACT_GELU, mod=mod, lvl=lvl)
        ctx.save_for_backward(x, cw, g, b, c, mean, invstd, mod)
        ctx.meta = (lvl, training, (bank, j))
        return y

    @_joined
    def backward(ctx, dy):
        x, cw, g, b, c, mean, invstd, mod = ctx.saved_tensors
        lvl, training, site = ctx.meta
        dmod = _dmod(mod, site)
        dc, dg, db = bn_bwd(dy.contiguous(), c, mean, invstd, g, b, training, ACT_GELU, mod, dmod, lvl)
        # policy (no input gradient): this is the LAST weight gradient of the backward pass and the critical stream has
        # nothing after the BatchNorm backward above — run it here instead of queueing it behind the side stream's tail
        dcw, _ = conv_wgrad(dc, x, cw.shape, lvl.nbr125, need_bias=False, side=ctx.needs_input_grad[0] or not _STEM_WGRAD_MAIN)
        # the policy feeds raw point features (no gradient); the motion planner concatenates a learned label embedding
        dx = conv_dgrad(dc, cw, lvl.nbr125, lvl.order[0], lvl=lvl) if ctx.needs_input_grad[0] else None
        return dx, dcw, dg, db, None, None, None, None, dmod, None, None


class SplitStemWeightFn(torch.autograd.Function):
    """stem.conv.weight [cout, 5, 5, 5, c_pc + Cc] -> (W_pc [cout, 5, 5, 5, c_pc], W_ctx [T * cout, Cc] tap-major), the two
    operands of concat.CtxStemFn.  One node instead of autograd's slices, so that the gradient of the ONE parameter — three
    quarters of the gradient floats of the tiny Concat policy — is assembled in a slab of _grad_slab like every other weight
    gradient (a data-parallel reducer then owns that memory) by two strided copies: no zero-filled full-size temporaries, no sum."""

    @staticmethod
    def forward(ctx, w, c_pc):
        ctx.meta = (tuple(w.shape), int(c_pc))
        cout, T = w.shape[0], w.shape[1] * w.shape[2] * w.shape[3]
        w_pc = w[..., :c_pc].contiguous()
        w_ctx = w[..., c_pc:].reshape(cout, T, -1).permute(1, 0, 2).reshape(T * cout, -1)
        return w_pc, w_ctx.contiguous()

    @staticmethod
    def backward(ctx, dw_pc, dw_ctx):
        shape, c_pc = ctx.meta
        cout, T = shape[0], shape[1] * shape[2] * shape[3]
        src = dw_pc if dw_pc is not None else dw_ctx
        if _JOIN == "end":
            sync_side_stream()  # (the copies below are ATen kernels of the current stream; the operands come from the side stream)
        n = cout * T * shape[4]
        dw = _grad_slab(n, src.device)[:n].view(shape)
        if dw_pc is None:
            dw[..., :c_pc].zero_()
        else:
            dw[..., :c_pc].copy_(dw_pc)
        if dw_ctx is None:
            dw[..., c_pc:].zero_()
        else:
            dw[..., c_pc:].copy_(dw_ctx.reshape(T, cout, -1).permute(1, 0, 2).reshape(cout, *shape[1:4], -1))
        return dw, None


class PoolFn(torch.autograd.Function):
    """SerializedPooling: GELU(BN(segment_max(Linear(x))))   (model.py:760-790)."""

    @_fwd
    def forward(ctx, x, w, bias, g, b, rmean, rvar, child, training, mod=None, bank=None, j=0):
        """(an adaptive norm sees the pooled level's clouds)"""
        (wk,), _ = _wk(w)
        ctx.wk = wk
        proj, _ = linear_fwd(x, wk, bias)
        C = w.shape[0]
        pooled = torch.empty(child.n, C, dtype=x.dtype, device=x.device)
        arg = torch.empty(child.n, C, dtype=torch.int32, device=x.device)
        call("lotus_pool_max_fwd", proj, child.members, child.seg_start, child.n, C, pooled, arg)
        if ARG_TAP is not None or ARG_INJECT:
            arg = _arg_hook("pool", arg)
        y, mean, invstd = bn_fwd(pooled, g, b, rmean, rvar, training, ACT_GELU, mod=mod, lvl=child)
        ctx.save_for_backward(x, w, g, b, pooled, arg, mean, invstd, mod)
        ctx.meta = (child, training, (bank, j))
        return y

    @_joined
    def backward(ctx, dy):
        x, w, g, b, pooled, arg, mean, invstd, mod = ctx.saved_tensors
        child, training, site = ctx.meta
        C = w.shape[0]
        dmod = _dmod(mod, site)
        dpool, dg, db = bn_bwd(dy.contiguous(), pooled, mean, invstd, g, b, training, ACT_GELU, mod, dmod, child)
        dproj = torch.empty(x.shape[0], C, dtype=x.dtype, device=x.device)
        call("lotus_pool_max_bwd", dpool, arg, child.cluster, x.shape[0], C, dproj)
        dw, dbias = linear_wgrad(dproj, x)
        dx = linear_dgrad(dproj, ctx.wk)
        return dx, dw, dbias, dg, db, None, None, None, None, dmod, None, None


class UnpoolFn(torch.autograd.Function):
    """SerializedUnpooling: skip = GELU(BN(Linear_skip(parent))), up = GELU(BN(Linear(point)));
    returns (skip + up[cluster], skip)   (model.py:817-828).  `skip` alone feeds the decoder CPE conv.  Adaptive norms: `up` is
    modulated (modu, slice ju) per cloud of the coarse level `child`, `skip` (mods, js) per cloud of the fine one, `lvl`."""

    @_fwd
    def forward(ctx, xc, xp, wu, bu, gu, betau, rmu, rvu, ws_, bs, gs, betas, rms, rvs, child, training, modu=None, mods=None,
                bank=None, ju=0, js=0, lvl=None):
        (wuk, wsk), _ = _wk(wu, ws_)
        ctx.wk = (wuk, wsk)
        lu, _ = linear_fwd(xc, wuk, bu)
        ls, _ = linear_fwd(xp, wsk, bs)
        (up, mu, iu), (skip, ms, is_) = bn_fwd_pair(lu, (gu, betau, rmu, rvu, modu, child), ls, (gs, betas, rms, rvs, mods, lvl),
                                                    training, ACT_GELU)
        x = torch.empty_like(skip)
        call("lotus_unpool_fwd", skip, up, child.cluster, skip.shape[0], skip.shape[1], x)
        ctx.save_for_backward(xc, xp, wu, gu, betau, ws_, gs, betas, lu, ls, mu, iu, ms, is_, modu, mods)
        ctx.meta = (child, training, lvl, (bank, ju), (bank, js))
        return x, skip

    @_joined
    def backward(ctx, dx, dskip):
        xc, xp, wu, gu, betau, ws_, gs, betas, lu, ls, mu, iu, ms, is_, modu, mods = ctx.saved_tensors
        child, training, lvl, su, ss = ctx.meta
        C = wu.shape[0]
        dx = dx.contiguous()
        dup = torch.empty(child.n, C, dtype=dx.dtype, device=dx.device)
        call("lotus_unpool_bwd", dx, child.members, child.seg_start, child.n, C, dup)
        dsk = add(dx, dskip.contiguous()) if dskip is not None else dx
        dmu, dms = _dmod(modu, su), _dmod(mods, ss)
        (dlu, dgu, dbetau), (dls, dgs, dbetas) = bn_bwd_pair((dup, lu, mu, iu, gu, betau, modu, dmu, child),
                                                            (dsk, ls, ms, is_, gs, betas, mods, dms, lvl), training, ACT_GELU)
        dwu, dbu = linear_wgrad(dlu, xc)
        dxc = linear_dgrad(dlu, ctx.wk[0])
        dws, dbs = linear_wgrad(dls, xp)
        dxp = linear_dgrad(dls, ctx.wk[1])
        return (dxc, dxp, dwu, dbu, dgu, dbetau, None, None, dws, dbs, dgs, dbetas) + (None,) * 4 + (dmu, dms, None, None, None, None)


class LinearFn(torch.autograd.Function):
    """Plain nn.Linear (txt_fc, simple_policy_ptv3.py:387,414)."""

    @_fwd
    def forward(ctx, x, w, b):
        y, _ = linear_fwd(x, w, b)
        ctx.save_for_backward(x, w)
        return y

    @_joined
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dw, db = linear_wgrad(dy, x, need_bias=ctx.needs_input_grad[2])
        dx = linear_dgrad(dy, w) if ctx.needs_input_grad[0] else None
        return dx, dw, (db if ctx.needs_input_grad[2] else None)


def cloud_max_fwd(x, lvl):
    """-> (pc [B, C] = torch.stack([torch.max(x, 0)[0] for x in torch.split(feat, npoints_in_batch)]), simple_policy_ptv3.py:117-119
    / motion_planner_ptv3.py:117-119; arg [B, C] int32 = the row each maximum came from, test taps applied)."""
    B, C = len(lvl.counts), x.shape[1]
    pc = torch.empty(B, C, dtype=x.dtype, device=x.device)
    arg = torch.empty(B, C, dtype=torch.int32, device=x.device)
    ws = _ws(query("lotus_cloud_max_workspace", B, C), x.device)
    call("lotus_cloud_max_fwd", x, lvl.off, B, C, pc, arg, ws, ws.numel())
    if ARG_TAP is not None or ARG_INJECT:
        arg = _arg_hook("cloud", arg)
    return pc, arg


def head_trunk_fwd(x, hw0, hb0, aw0, ab0, aw3, ab3, lvl, drop_p, seed, heat):
    """What every ActionHead computes (simple_policy_ptv3.py:113-120): the hidden heat-map layer h, the per-cloud max, the action
    MLP; heat(h) = the node's own second heat-map layer, launched right behind h.  -> (h, hpre, heat(h), pc, arg, a, apre, ae)."""
    h, hpre = linear_fwd(x, hw0, hb0, act=ACT_LEAKY, save_pre=True, drop_p=drop_p, seed=seed)
    if ARG_TAP is not None or ARG_INJECT:
        hpre = _arg_hook("leaky", hpre)
    pos = heat(h)
    pc, arg = cloud_max_fwd(x, lvl)
    a, apre = linear_fwd(pc, aw0, ab0, act=ACT_LEAKY, save_pre=True, drop_p=drop_p, seed=mix_seed(seed, 1))
    ae, _ = linear_fwd(a, aw3, ab3)
    return h, hpre, pos, pc, arg, a, apre, ae


def head_trunk_bwd(dae_o, dxt, x, hw0, hw3, aw0, aw3, h, hpre, pc, arg, a, apre, lvl, p, seed):
    """dae_o = d ae, dxt = d heat(h) -> (dx, dhw0, dhb0, dhw3, dhb3, daw0, dab0, daw3, dab3), the head nodes' argument order."""
    # action branch (B rows)
    daw3, dab3 = linear_wgrad(dae_o, a)
    dapre = linear_dgrad(dae_o, aw3, pre=apre, act=ACT_LEAKY, drop_p=p, seed=mix_seed(seed, 1))
    daw0, dab0 = linear_wgrad(dapre, pc)
    dpc = linear_dgrad(dapre, aw0)
    # heatmap branch (N rows)
    dhw3, dhb3 = linear_wgrad(dxt, h)
    dhpre = linear_dgrad(dxt, hw3, pre=hpre, act=ACT_LEAKY, drop_p=p, seed=seed)
    dhw0, dhb0 = linear_wgrad(dhpre, x)
    dxh = linear_dgrad(dhpre, hw0)
    dx = torch.empty_like(x)
    call("lotus_cloud_max_bwd", dpc, arg, lvl.batch, x.shape[0], x.shape[1], dxh, dx)
    return dx, dhw0, dhb0, dhw3, dhb3, daw0, dab0, daw3, dab3


class HeadLossFn(torch.autograd.Function):
    """ActionHead (heatmap_disc / max / euler_disc) + compute_loss, simple_policy_ptv3.py:113-157,
    :308-373.  Returns (losses[4] = pos, rot, open, total; xt [N, 3*2*pos_bins]; ae [B, 217])."""

    @_fwd
    def forward(ctx, x, hw0, hb0, hw3, hb3, aw0, ab0, aw3, ab3, lvl, tgt, gt, pos_w, rot_w, drop_p, seed, with_loss):
        dev = x.device
        B = len(lvl.counts)
        h, hpre, xt, pc, arg, a, apre, ae = head_trunk_fwd(x, hw0, hb0, aw0, ab0, aw3, ab3, lvl, drop_p, seed,
                                                           lambda h: linear_fwd(h, hw3, hb3)[0])
        losses = torch.zeros(4, dtype=torch.float32, device=dev)
        nb = xt.shape[1] // 3
        nrot = (ae.shape[1] - 1) // 3
        stats = torch.empty(query("lotus_loss_stats_floats", B), dtype=torch.float32, device=dev)
        dae = torch.empty(ae.shape, dtype=torch.float32, device=dev)  # saved gradient factors stay fp32
        if with_loss:
            call("lotus_loss_fwd", xt, ae, tgt, gt, lvl.off, B, nb, nrot, gt.shape[1], float(pos_w), float(rot_w),
                 losses, stats, dae)
        ctx.save_for_backward(x, hw0, hw3, aw0, aw3, h, hpre, xt, pc, arg, a, apre, stats, dae, tgt)
        ctx.meta = (lvl, pos_w, rot_w, drop_p, seed, with_loss, nb, nrot)
        ctx.mark_non_differentiable(xt, ae)
        return losses, xt, ae

    @_joined
    def backward(ctx, gl, _gxt, _gae):
        x, hw0, hw3, aw0, aw3, h, hpre, xt, pc, arg, a, apre, stats, dae, tgt = ctx.saved_tensors
        lvl, pos_w, rot_w, p, seed, with_loss, nb, nrot = ctx.meta
        assert with_loss, "backward through the head requires compute_loss=True"
        dxt = torch.empty_like(xt)
        dae_o = torch.empty(dae.shape, dtype=xt.dtype, device=x.device)
        call("lotus_loss_bwd", xt, tgt, lvl.off, lvl.batch, stats, dae, gl.contiguous(), float(pos_w), float(rot_w), len(lvl.counts),
             x.shape[0], nb, nrot, dxt, dae_o)
        return head_trunk_bwd(dae_o, dxt, x, hw0, hw3, aw0, aw3, h, hpre, pc, arg, a, apre, lvl, p, seed) + (None,) * 8


ROT_KINDS = {"euler_disc": 0, "euler": 1, "quat": 2}  # rot_kind of lotus_reg_loss_fwd


def softpos_fwd(h, w3, b3, pc_fts, lvl, temp):
    """e = h w3^T + b3 [N, 4] and the per-cloud soft position xt [B, 3] = sum_i softmax_i(e_i0 / temp) (xyz_i + e_i[1:4])
    (simple_policy_ptv3.py:83-103); pc_fts [N, >= 3] fp32 with unit column stride.  -> (e, xt, stats [B, 2] f64 = max, lse)."""
    N, C = h.shape
    B = len(lvl.counts)
    assert pc_fts.dtype == torch.float32 and pc_fts.stride(1) == 1 and pc_fts.shape[0] == N and w3.shape == (4, C)
    e = torch.empty(N, 4, dtype=torch.float32, device=h.device)
    xt = torch.empty(B, 3, dtype=torch.float32, device=h.device)
    stats = torch.empty(B, 2, dtype=torch.float64, device=h.device)
    ws = _ws(query("lotus_softpos_workspace", B), h.device)
    call("lotus_softpos_fwd", h, w3, b3, pc_fts, pc_fts.stride(0), lvl.off, B, N, C, float(temp), e, xt, stats, ws, ws.numel())
    return e, xt, stats


def softpos_bwd(g, e, pc_fts, lvl, stats, xt, temp):
    """de [N, 4] of softpos_fwd from g [B, 3] = dL / dxt."""
    de = torch.empty_like(e)
    call("lotus_softpos_bwd", g, e, pc_fts, pc_fts.stride(0), lvl.batch, stats, xt, len(lvl.counts), e.shape[0], float(temp), de)
    return de


class RegHeadLossFn(torch.autograd.Function):
    """ActionHead with a regression option (pos_pred_type 'heatmap_mlp' and / or rot_pred_type 'euler' / 'quat') +
    compute_loss, simple_policy_ptv3.py:46-53,83-103,113-157,:308-373.  fp32 activation storage.  Returns (losses[4] = pos,
    rot, open, total; xt = the soft position [B, 3] ('heatmap_mlp') or the heat-map logits [N, 3*2*pos_bins];
    the rotation = ae for 'euler_disc', ae[:, :3] for 'euler', the normalised quaternion [B, 4]; xo = ae[:, -1]).
    pc_fts [N, >= 3] holds the coordinates (row stride = its width); temp = pos_heatmap_temp."""

    @_fwd
    def forward(ctx, x, hw0, hb0, hw3, hb3, aw0, ab0, aw3, ab3, lvl, tgt, gt, pc_fts, pos_type, rot_type, temp, pos_w, rot_w,
                drop_p, seed, with_loss):
        assert not _capi.BF16, "the regression head runs with fp32 activation storage"
        dev = x.device
        B = len(lvl.counts)
        mlp, kind = pos_type == "heatmap_mlp", ROT_KINDS[rot_type]
        if mlp:   # -> (e, xt, stats)
            heat = lambda h: softpos_fwd(h, hw3, hb3, pc_fts, lvl, temp)  # noqa: E731
        else:
            heat = lambda h: (None, linear_fwd(h, hw3, hb3)[0], None)  # noqa: E731
        h, hpre, (e, xt, stats), pc, arg, a, apre, ae = head_trunk_fwd(x, hw0, hb0, aw0, ab0, aw3, ab3, lvl, drop_p, seed, heat)
        W = ae.shape[1]
        nb = 0 if mlp else xt.shape[1] // 3
        nrot = (W - 1) // 3 if kind == 0 else 0
        losses = torch.zeros(4, dtype=torch.float32, device=dev)
        dae = torch.empty(B, W, dtype=torch.float32, device=dev)
        dpos = torch.empty(B, 3, dtype=torch.float32, device=dev)
        xr = torch.empty(B, 4, dtype=torch.float32, device=dev) if kind == 2 else None
        ce = None
        if with_loss and not mlp:
            ce = torch.empty(query("lotus_loss_stats_floats", B), dtype=torch.float32, device=dev)
            call("lotus_pos_ce_fwd", xt, tgt, lvl.off, B, nb, ce)
        if with_loss or kind == 2:
            call("lotus_reg_loss_fwd", ae, gt if with_loss else None, xt if (with_loss and mlp) else None, ce, 4, B, W,
                 gt.shape[1] if with_loss else 0, kind, nrot, float(pos_w), float(rot_w), losses, dae, dpos, xr)
        empty = x.new_empty(0)
        ctx.save_for_backward(x, hw0, hw3, aw0, aw3, h, hpre, xt, pc, arg, a, apre, dae, dpos, pc_fts,
                              e if mlp else empty, stats if mlp else empty, ce if ce is not None else empty,
                              tgt if not mlp else empty)
        ctx.meta = (lvl, pos_w, rot_w, drop_p, seed, with_loss, mlp, nb, float(temp))
        rot = xr if kind == 2 else (ae[:, :3] if kind == 1 else ae)
        xo = ae[:, -1]
        ctx.mark_non_differentiable(xt, rot, xo)
        return losses, xt, rot, xo

    @_joined
    def backward(ctx, gl, _gxt, _grot, _gxo):
        x, hw0, hw3, aw0, aw3, h, hpre, xt, pc, arg, a, apre, dae, dpos, pc_fts, e, stats, ce, tgt = ctx.saved_tensors
        lvl, pos_w, rot_w, p, seed, with_loss, mlp, nb, temp = ctx.meta
        assert with_loss, "backward through the head requires compute_loss=True"
        B, W = dae.shape
        dae_o = torch.empty_like(dae)
        gpos = torch.empty_like(dpos)
        call("lotus_reg_loss_bwd", dae, dpos, gl.contiguous(), float(pos_w), float(rot_w), B, W, dae_o, gpos)
        # d e [N, 4] of the soft position, or d xt of the heat-map cross entropy
        if mlp:
            dxt = softpos_bwd(gpos, e, pc_fts, lvl, stats, xt, temp)
        else:
            dxt = torch.empty_like(xt)
            call("lotus_pos_ce_bwd", xt, tgt, lvl.off, lvl.batch, ce, gpos, B, x.shape[0], nb, dxt)
        return head_trunk_bwd(dae_o, dxt, x, hw0, hw3, aw0, aw3, h, hpre, pc, arg, a, apre, lvl, p, seed) + (None,) * 12


class StepHeadFn(torch.autograd.Function):
    """Heat-map branch of the trajectory head for ALL steps (motion_planner_ptv3.py:88-97,113-114):
    xt_t = Linear3(dropout(LeakyReLU(base + step_bias[t]))), t = 0..T-1, with `base` = the point-feature part of the first
    Linear (shared by the steps).  The hidden layers are never kept: backward regenerates them (same counter-hash masks),
    accumulates d base over the steps in the activation-backward kernel and sums the weight gradients of the T products."""

    @_fwd
    def forward(ctx, base, step_bias, w3, b3, drop_p, seed):
        T = step_bias.shape[0]
        M, C = base.shape
        outs = []
        for t in range(T):
            h = torch.empty_like(base)
            call("lotus_step_act_fwd", base, step_bias[t], h, M, C, ACT_LEAKY, float(drop_p), mix_seed(seed, t))
            outs.append(linear_fwd(h, w3, b3)[0])
        ctx.save_for_backward(base, step_bias, w3)
        ctx.meta = (float(drop_p), int(seed))
        return tuple(outs)

    @_joined
    def backward(ctx, *dxts):
        base, step_bias, w3 = ctx.saved_tensors
        p, seed = ctx.meta
        T = step_bias.shape[0]
        M, C = base.shape
        dbase = torch.empty_like(base)
        dsb = torch.empty_like(step_bias)
        dw3 = db3 = None
        ws = _ws(query("lotus_step_act_bwd_workspace", M, C), base.device)
        first = True
        keep = []  # everything the weight-gradient stream reads stays alive until the node's join (h_t and a contiguous
        #            copy of dxt_t would otherwise be recycled by the allocator while wgrad_t is still in flight)
        for t in range(T):
            if dxts[t] is None:
                dsb[t].zero_()
                continue
            dxt = dxts[t].contiguous()
            h = torch.empty_like(base)
            keep.append((dxt, h))
            if _JOIN == "end" and _side() is not None:
                dxt.record_stream(_SIDES[0][0]); h.record_stream(_SIDES[0][0])
            call("lotus_step_act_fwd", base, step_bias[t], h, M, C, ACT_LEAKY, p, mix_seed(seed, t))
            dw3, db3 = linear_wgrad(dxt, h, into=None if dw3 is None else (dw3, db3))
            dh = linear_dgrad(dxt, w3)
            call("lotus_step_act_bwd", dh, base, step_bias[t], dbase, dsb[t], M, C, ACT_LEAKY, p, mix_seed(seed, t),
                 0 if first else 1, ws, ws.numel())
            first = False
        if first:
            dbase.zero_()
        # `keep` dies with this frame: whatever re-uses the blocks is enqueued after the join `_joined` performs next
        return dbase, dsb, dw3, db3, None, None


class PosCEFn(torch.autograd.Function):
    """Soft-target heatmap cross entropy per (cloud, axis): F.cross_entropy(rearrange(pred, 'c n b -> c (n b)'),
    probs, reduction='none') of motion_planner_ptv3.py:329-334 for one trajectory step.  Returns [B, 3]."""

    @_fwd
    def forward(ctx, xt, tgt, lvl):
        B = len(lvl.counts)
        nb = xt.shape[1] // 3
        stats = torch.empty(query("lotus_loss_stats_floats", B), dtype=torch.float32, device=xt.device)
        call("lotus_pos_ce_fwd", xt, tgt, lvl.off, B, nb, stats)
        ctx.save_for_backward(xt, tgt, stats)
        ctx.lvl = lvl
        return stats[:B * 12].view(B, 3, 4)[:, :, 0].clone()

    @_joined
    def backward(ctx, g):
        xt, tgt, stats = ctx.saved_tensors
        lvl = ctx.lvl
        dxt = torch.empty_like(xt)
        call("lotus_pos_ce_bwd", xt, tgt, lvl.off, lvl.batch, stats, g.contiguous().float(), len(lvl.counts), xt.shape[0],
             xt.shape[1] // 3, dxt)
        return dxt, None, None


class TrajLossFn(torch.autograd.Function):
    """The [B, T]-sized losses of the motion planner in one launch (motion_planner_ptv3.py:327-397): masked rotation
    cross entropy, openness / stop BCE and the masked mean of the heatmap cross entropies ce [B, T, 3].  Returns the
    vector (pos, rot, open, stop, total)."""

    @_fwd
    def forward(ctx, ae, ce, gt, stop, mask, nrot, pos_w, rot_w):
        B, T = mask.shape
        ae, ce = ae.contiguous(), ce.contiguous().float()
        losses = torch.empty(5, dtype=torch.float32, device=ae.device)
        dae = torch.empty(ae.shape, dtype=torch.float32, device=ae.device)  # saved gradient factors stay fp32
        dce = torch.empty_like(ce)
        call("lotus_mp_loss_fwd", ae, gt, stop, mask, ce, B, T, nrot, gt.shape[-1], float(pos_w), float(rot_w), losses, dae, dce)
        ctx.save_for_backward(dae, dce)
        ctx.dims = (B, T, nrot, float(pos_w), float(rot_w))
        return losses

    @_joined
    def backward(ctx, g):
        dae, dce = ctx.saved_tensors
        B, T, nrot, pos_w, rot_w = ctx.dims
        dae_o = torch.empty(dae.shape, dtype=torch.bfloat16 if _capi.BF16 else torch.float32, device=dae.device)
        dce_o = torch.empty_like(dce)
        call("lotus_mp_loss_bwd", dae, dce, g.contiguous().float(), pos_w, rot_w, B, T, nrot, dae_o, dce_o)
        return dae_o, dce_o, None, None, None, None, None, None


class TrajSoftPosFn(torch.autograd.Function):
    """Heat-map branch of the soft trajectory head for ALL steps in one pass (motion_planner_ptv3.py:89-109, pos_pred_type
    'heatmap_mlp'): xt[b, t] = sum_i softmax_i(e_ti0 / temp) (coord_i + e_ti[1:4]) with e_t = dropout(LeakyReLU(base +
    step_bias[t])) W3^T + b3.  The hidden layers never reach memory, forward or backward (lotus_mp_softpos_fwd / _bwd); the
    mask of step t is StepHeadFn's (mix_seed(seed, t)).  pc_fts [N, >= 3] holds the coordinates.  Returns xt [B, T, 3]."""

    @_fwd
    def forward(ctx, base, step_bias, w3, b3, pc_fts, lvl, temp, drop_p, seed):
        assert not _capi.BF16, "the soft trajectory head runs with fp32 activation storage"
        T = step_bias.shape[0]
        N, C = base.shape
        B = len(lvl.counts)
        dev = base.device
        e = torch.empty(T, N, 4, dtype=torch.float32, device=dev)
        xt = torch.empty(B, T, 3, dtype=torch.float32, device=dev)
        stats = torch.empty(B, T, 2, dtype=torch.float64, device=dev)
        ws = _ws(query("lotus_mp_softpos_workspace", B, T), dev)
        call("lotus_mp_softpos_fwd", base, step_bias, w3, b3, pc_fts, pc_fts.stride(0), lvl.off, B, N, C, T, float(temp),
             float(drop_p), int(seed), e, xt, stats, ws, ws.numel())
        ctx.save_for_backward(base, step_bias, w3, e, pc_fts, stats, xt)
        ctx.meta = (lvl, float(temp), float(drop_p), int(seed))
        return xt

    @_joined
    def backward(ctx, g):
        base, step_bias, w3, e, pc_fts, stats, xt = ctx.saved_tensors
        lvl, temp, p, seed = ctx.meta
        T = step_bias.shape[0]
        N, C = base.shape
        dbase, dsb, dw3 = torch.empty_like(base), torch.empty_like(step_bias), torch.empty_like(w3)
        db3 = torch.empty(4, dtype=torch.float32, device=base.device)
        ws = _ws(query("lotus_mp_softpos_bwd_workspace", N, C, T), base.device)
        call("lotus_mp_softpos_bwd", g.contiguous().float(), base, step_bias, w3, e, pc_fts, pc_fts.stride(0), lvl.batch, stats, xt,
             len(lvl.counts), N, C, T, temp, p, seed, dbase, dsb, dw3, db3, ws, ws.numel())
        return dbase, dsb, dw3, db3, None, None, None, None, None


class TrajRegLossFn(torch.autograd.Function):
    """The [B, T]-sized losses of the motion planner with the soft position in one launch (motion_planner_ptv3.py:338-397):
    masked MSE of xt [B*T, 3] with ONE global normalisation, masked rotation cross entropy, openness / stop BCE.  Returns the
    vector (pos, rot, open, stop, total)."""

    @_fwd
    def forward(ctx, ae, xt, gt, stop, mask, nrot, pos_w, rot_w):
        assert not _capi.BF16, "the soft trajectory head runs with fp32 activation storage"
        B, T = mask.shape
        ae, xt = ae.contiguous(), xt.contiguous()
        losses = torch.empty(5, dtype=torch.float32, device=ae.device)
        dae = torch.empty(ae.shape, dtype=torch.float32, device=ae.device)
        dxt = torch.empty_like(xt)
        call("lotus_mp_reg_loss_fwd", ae, gt, stop, mask, xt, B, T, nrot, gt.shape[-1], float(pos_w), float(rot_w), losses, dae, dxt)
        ctx.save_for_backward(dae, dxt)
        ctx.dims = (B, T, nrot, float(pos_w), float(rot_w))
        return losses

    @_joined
    def backward(ctx, g):
        dae, dxt = ctx.saved_tensors
        B, T, nrot, pos_w, rot_w = ctx.dims
        dae_o, dxt_o = torch.empty_like(dae), torch.empty_like(dxt)
        call("lotus_mp_reg_loss_bwd", dae, dxt, g.contiguous().float(), pos_w, rot_w, B, T, nrot, dae_o, dxt_o)
        return dae_o, dxt_o, None, None, None, None, None, None


class CloudMaxFn(torch.autograd.Function):
    """cloud_max_fwd as a node of its own (the motion planner's action branch)."""

    @_fwd
    def forward(ctx, x, lvl):
        y, arg = cloud_max_fwd(x, lvl)
        ctx.save_for_backward(arg)
        ctx.lvl, ctx.n = lvl, x.shape[0]
        return y

    @_joined
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        dx = torch.empty(ctx.n, dy.shape[1], dtype=dy.dtype, device=dy.device)
        call("lotus_cloud_max_bwd", dy.contiguous(), arg, ctx.lvl.batch, ctx.n, dy.shape[1], None, dx)
        return dx, None
