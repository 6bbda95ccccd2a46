"""Thin Python wrappers over the C-ABI (include/drn_hip.h): tensors in, kernel launches out.

Nothing here computes: every function marshals device pointers / shapes into a
libdrn_hip.so call on torch's current HIP stream.  Missing library or a non-zero
return code raises (no fallback).
"""
import ctypes
import numbers

import torch

from . import _lib
from ._lib import GemmDesc, WgradDesc, check, lib

F32, BF16 = 0, 1


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise _lib.DrnError("unsupported dtype %s (float32 / bfloat16 only)" % t.dtype)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.DrnError("drn_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback" % t.device)


def gemm_desc(A, B, C, M, N, Cin, taps=1, stride=1, pad=0, mode=0, Lout=None, Lsrc=None, lda=None, ldb=None,
              ldc=None, bias=None, gate=None, ldg=0, stats=None, C2=None, ldc2=None, accumulate=False, out_f32=False, sumsq=None,
              gate_bwd=None):
    """gate_bwd: dict(act, ld_act, dct, ldt, dgate, dsum) -- the data gradient feeds the input stage's gate backward, which then
    happens in the launch's epilogue (DrnGemmDesc::gb_*; gemm_nt_w4c_kernel only: ask gemm_nt_plan)."""
    _need_gpu(A, B, C, bias, gate, stats, C2)
    Lout = M if Lout is None else Lout
    Lsrc = Lout if Lsrc is None else Lsrc
    gb = gate_bwd or {}
    _need_gpu(gb.get("act"), gb.get("dct"), gb.get("dgate"), gb.get("dsum"))
    return GemmDesc(A=_p(A), B=_p(B), C=_p(C), C2=_p(C2), bias=_p(bias), gate=_p(gate), stats=_p(stats),
                    M=M, N=N, Cin=Cin, taps=taps, stride=stride, pad=pad, mode=mode, Lout=Lout, Lsrc=Lsrc,
                    lda=Cin if lda is None else lda, ldb=taps * Cin if ldb is None else ldb,
                    ldc=N if ldc is None else ldc, ldg=ldg, accumulate=int(accumulate),
                    ldc2=(N if ldc is None else ldc) if ldc2 is None else ldc2, out_f32=int(out_f32), sumsq=_p(sumsq),
                    gb_act=_p(gb.get("act")), gb_dct=_p(gb.get("dct")), gb_dgate=_p(gb.get("dgate")), gb_dsum=_p(gb.get("dsum")),
                    gb_ld_act=int(gb.get("ld_act", 0)), gb_ldt=int(gb.get("ldt", 0)))


# Optional per-launch timing of the MFMA kernels (bench.py): a list collecting (tag, flops, start_event, end_event),
# the events recorded on the same stream the kernels run on.
kernel_timer = None
# Split-K (drn_gemm_nt_splitk: one launch, the last-arriving split of a tile sums the partial tiles) for problems that cannot
# fill the chip (<= 160 tiles of 128x128 on 256 CUs): conv0 forward (128 tiles x 204 K-steps) 157 -> 69 us 4-way.  With warm
# operands the 12-48-step pyramid GEMMs gain nothing from it (the exchange costs 4-8 us: scripts/bench_splitk.py), but inside
# the step, where their operands are cold, 2-4 splits of >= 12 K-steps each put twice the loads in flight: -25 us per step.
SPLITK_MIN_KSTEPS = 24
SPLITK_STEPS_PER_SPLIT = 12     # a bf16 split owns at least that many K-steps
# Workgroups a split launch aims for.  256 = one 8-wave workgroup per CU on the 4-slot ring (three K-tiles of loads in flight
# against cold operands) rather than 512 = two per CU on 2-slot rings: conv0's forward (128 tiles x 204 K-steps) 4 -> 2 splits, the
# step 2.222 -> 2.209 ms at T = 256 in one process (384: 2.237, 192 = conv0 unsplit: 2.27), T = 32 unchanged.
KSPLIT_WGS = 256


def _timed(tag, flops, launch):
    if kernel_timer is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    kernel_timer.append((tag, flops, e0, e1))


def _ksplit(descs, dtype):
    """Split-K factor for a launch (one problem, or -- bf16 -- a group of them) that cannot fill 256 CUs with 128x128 tiles."""
    tiles = sum(((d.M + 127) // 128) * ((d.N + 127) // 128) for d in descs)
    nkt = min((d.taps * d.Cin) // (64 if dtype == BF16 else 32) for d in descs)
    # exact-f32 (parity) mode keeps round 1's rule -- split only the long-K single problems -- so its summation orders, and
    # with them the ReLU decisions the tolerance tests were calibrated on, stay what they were
    if dtype != BF16 and len(descs) > 1:
        return 1
    if tiles > 160 or nkt < (SPLITK_MIN_KSTEPS if dtype == BF16 else 96):
        return 1
    return max(1, min(8, (KSPLIT_WGS if dtype == BF16 else 512) // tiles, nkt // (SPLITK_STEPS_PER_SPLIT if dtype == BF16 else 6)))


# One long-K bf16 k = 3 convolution with 16-64 tiles of 256x256 (conv0's forward: 32 tiles x 204 K-steps): full-width tiles on the
# 4-wave kernel, the K loop split so that ~256 workgroups exist, fp32 partial planes + a second launch that adds them
# (drn_gemm_nt_splitk256) -- half the L2 -> LDS bytes of the 128x128 in-launch split below.  Built and tested, off by default (the in-launch
# W4H split below takes conv0's forward first); SPLITK256 = True turns it on.
SPLITK256 = False


def _ksplit256(descs, dtype):
    if not SPLITK256 or dtype != BF16 or len(descs) != 1:
        return 1
    d = descs[0]
    if d.gate or d.C2 or d.accumulate or d.out_f32:
        return 1
    if d.taps != 3 or d.stride != 1 or d.pad != 1 or d.mode not in (0, 1) or d.Lout != d.Lsrc or d.M % 256 or d.N % 256 or d.Cin % 64 or d.M % d.Lout:
        return 1
    if d.ldc % 8 or (d.C or 0) % 16:
        return 1
    tiles = (d.M // 256) * (d.N // 256)
    nkt = (d.taps * d.Cin) // 64
    if tiles > 64 or tiles < 16 or nkt < 96:
        return 1
    # a multiple of the 3 taps: the splits of a tile that sit a whole tap apart walk the same channel blocks of the same source
    # rows at the same time (all splits of a tile run on one XCD: grid x = tile), so the input is mostly read from HBM once
    per_tap = (256 // tiles) // 3
    per = nkt // 3
    while per_tap > 1 and per % per_tap:
        per_tap -= 1
    return 3 * per_tap if per_tap >= 1 and per // per_tap >= 8 else 1


NT_KIND_TILE128, NT_KIND_TILE256, NT_KIND_W4, NT_KIND_W4C, NT_KIND_W4H = 0, 1, 2, 3, 4


def gemm_nt_plan(descs, dtype):
    """The kernel drn_gemm_nt would pick for these problems (NT_KIND_*), asked of the library itself (drn_gemm_nt_plan)."""
    arr = (GemmDesc * len(descs))(*descs)
    kind = lib().drn_gemm_nt_plan(arr, len(descs), dtype)
    if kind < 0:
        check(kind, "drn_gemm_nt_plan")
    return kind


# One long-K bf16 problem with few output tiles (conv0's forward: 8192 x 256 x 13056 = 64 tiles of 256 x 128, 204 K-steps) on the
# 4-wave kernel's half-width tiles with the K loop split INSIDE the launch so that ~256 workgroups exist (gemm_nt_w4h_kernel:
# partial accumulators exchanged through the workspace, the last-arriving split of a tile sums them in split order).
# With the K loop in tap-major order this lost to 128x128 tiles split 2 ways (91 against 84 us: every 128-byte piece of conv0's
# 71 MB input sits in a DRAM page of its own and was fetched three times, once per tap, 68 K-steps apart; with the rows of A aliased
# -- scripts/experiments/conv0_alias_bench.py -- the same launch took 56 us).  Split k = 3 launches over >= 2048 input channels now
# walk K as (channel block, tap) (W4HT_LOOP_ASM, drn_tune "w4h_tapil"): the three taps of a channel block read the same lines one
# K-step after the other.  conv0's forward 85.8 -> 70.0 us alone and 81.9 -> 75.4 us inside the step (one box each, both paths
# traced); the step itself moves inside its noise (2.007 -> 2.002 ms).  KSPLIT_W4H = False switches it off.
KSPLIT_W4H = True


def _ksplit_w4h(descs, dtype):
    if not KSPLIT_W4H or dtype != BF16 or len(descs) != 1:
        return 1
    d = descs[0]
    if d.M % 256 or d.N % 128 or d.Cin % 64:
        return 1
    tiles, nkt = (d.M // 256) * (d.N // 128), (d.taps * d.Cin) // 64
    if tiles > 128 or nkt < 96:
        return 1
    ks = min(8, KSPLIT_WGS // tiles, nkt // 24)
    while ks > 1 and -(-nkt // -(-nkt // ks)) != ks:           # every split non-empty
        ks -= 1
    if ks < 2:
        return 1
    arr = (GemmDesc * 1)(d)
    return ks if lib().drn_gemm_nt_splitk_plan(arr, 1, ks, dtype) == NT_KIND_W4H else 1


# The in-launch split-K exchanges (partial tiles published write-through, a ticket, the last arriver sums) must CONFIRM their stores
# before the ticket whenever a kernel of another queue may run beside the launch: with one, the ticket overtook a partial about once
# in 10^5 launches of skinny_group_kernel inside the replayed two-branch graph (qdense.hip has the measurements; that kernel and the
# loss kernel always confirm with a returning read-modify-write per stored address, it costs them nothing).  The GEMM kernels'
# exchanges have never shown the window, but nobody standing here can prove a single queue (the Trainer's prefetch copies run on their
# own stream beside the replay, RCCL's kernels beside backward, a second graph branch beside the first), so every launch confirms by
# READ-BACK -- an sc1 load of every stored request, +12 us per step at T = 256, the variant that closed the window on the proven
# kernel (0 events in 120 k replays against 7) -- which is what the library does when the call's `ksplit` carries no flag.  The mode
# travels WITH THE CALL (DRN_KSPLIT_CONFIRM_* bits, include/drn_hip.h): no process-wide switch.  XCHG_CONFIRM = "0" / "1" select
# "nothing" / "returning atomics" for stress tests and A/Bs (scripts/experiments), "2" = the default.
KSPLIT_CONFIRM_ATOMIC, KSPLIT_CONFIRM_NONE = 0x20000, 0x80000
XCHG_CONFIRM = "2"


def _ksplit_arg(ks):
    return ks | (KSPLIT_CONFIRM_NONE if XCHG_CONFIRM == "0" else KSPLIT_CONFIRM_ATOMIC if XCHG_CONFIRM == "1" else 0)


def gemm_nt(descs, dtype):
    arr = (GemmDesc * len(descs))(*descs)
    flops = sum(2.0 * d.M * d.N * d.taps * d.Cin for d in descs)
    ks = _ksplit_w4h(descs, dtype)
    if ks > 1:
        d0 = descs[0]
        dev = torch.device("cuda", torch.cuda.current_device())
        ws = torch.empty(ks * d0.M * d0.N, dtype=torch.float32, device=dev)
        tag = "gemm_nt[bf16] g=1 M=%d N=%d K=%d mode=%d splitK=%d(w4h)" % (d0.M, d0.N, d0.taps * d0.Cin, d0.mode, ks)
        return _timed(tag, flops, lambda: check(lib().drn_gemm_nt_splitk_grouped(arr, 1, _ksplit_arg(ks), _p(ws), _p(_counters(dev)), dtype, _stream()),
                                                "drn_gemm_nt_splitk_grouped"))
    ks = _ksplit256(descs, dtype)
    if ks > 1:
        d0 = descs[0]
        dev = torch.device("cuda", torch.cuda.current_device())
        ws = workspace(ks * d0.M * d0.N, dev)
        tag = "gemm_nt[bf16] g=1 M=%d N=%d K=%d mode=%d splitK256=%d" % (d0.M, d0.N, d0.taps * d0.Cin, d0.mode, ks)
        return _timed(tag, flops, lambda: check(lib().drn_gemm_nt_splitk256(arr, ks, _p(ws), dtype, _stream()), "drn_gemm_nt_splitk256"))
    ks = _ksplit(descs, dtype)
    if ks > 1:
        d0 = descs[0]
        dev = torch.device("cuda", torch.cuda.current_device())
        tiles = sum(((d.M + 127) // 128) * ((d.N + 127) // 128) for d in descs)
        ws = torch.empty(ks * tiles * 128 * 128, dtype=torch.float32, device=dev)
        tag = "gemm_nt[%s] g=%d M=%d N=%d K=%d mode=%d splitK=%d" % ("bf16" if dtype == BF16 else "f32", len(descs),
                                                                     sum(d.M for d in descs), d0.N, d0.taps * d0.Cin, d0.mode, ks)
        return _timed(tag, flops, lambda: check(lib().drn_gemm_nt_splitk_grouped(arr, len(descs), _ksplit_arg(ks), _p(ws), _p(_counters(dev)),
                                                                                 dtype, _stream()), "drn_gemm_nt_splitk_grouped"))
    d0 = descs[0]
    tag = "gemm_nt[%s] g=%d M=%d N=%d K=%d mode=%d" % ("bf16" if dtype == BF16 else "f32", len(descs),
                                                      sum(d.M for d in descs), d0.N, d0.taps * d0.Cin, d0.mode)
    _timed(tag, flops, lambda: check(lib().drn_gemm_nt(arr, len(descs), dtype, _stream()), "drn_gemm_nt"))


def wgrad_desc(dY, X, M, Lout=None, Lsrc=None, ldy=None, ldx=None):
    _need_gpu(dY, X)
    Lout = M if Lout is None else Lout
    return WgradDesc(dY=_p(dY), X=_p(X), M=M, Lout=Lout, Lsrc=Lout if Lsrc is None else Lsrc,
                     ldy=dY.shape[-1] if ldy is None else ldy, ldx=X.shape[-1] if ldx is None else ldx)


class WgradPending(object):
    """A caller-owned list of deferred weight-gradient reduces (DrnWgradPending, include/drn_hip.h) + the workspaces it references.
    `ranges`: [(first byte, one past the last)] of the gradient memory whose reduces may be deferred into this list -- a launch finds
    its list by where its dW lives (pending_for), so nothing process-wide says "defer": two models in one process own two lists over
    disjoint buckets and never see each other's items, and a gradient written anywhere else is reduced at once."""

    def __init__(self, ranges=()):
        from ._lib import WgradPending as _Struct
        self.c = _Struct()                 # all-zero = empty
        self.ws = []
        self.ranges = [(int(lo), int(hi)) for lo, hi in ranges]

    def __len__(self):
        return int(self.c.n)

    def reset(self):
        """Drop whatever is recorded (a backward that raised leaves items behind: the next step must not run them)."""
        self.c.n = 0
        del self.ws[:]

    def covers(self, ptr):
        return any(lo <= ptr < hi for lo, hi in self.ranges)

    def outputs(self):
        return [(int(self.c.it[i].out), int(self.c.it[i].N) * int(self.c.it[i].taps) * int(self.c.it[i].Cin)) for i in range(len(self))]


_armed = []          # WgradPending lists currently accepting items (armed by their owners between zero() and collect())


def wgrad_arm(pend):
    if not any(q is pend for q in _armed):
        _armed.append(pend)


def wgrad_disarm(pend):
    _armed[:] = [q for q in _armed if q is not pend]


def pending_for(dWs):
    """The armed list whose ranges hold EVERY one of the given gradients, else None (reduce at once)."""
    ptrs = [dW.data_ptr() for dW in dWs]
    for q in _armed:
        if all(q.covers(x) for x in ptrs):
            return q
    return None


_persistent = {}


def persistent_buffer(key, n, device, dtype=torch.float32):
    """A buffer that keeps its address for the life of the process (per key and size): small per-step outputs that a LATER launch of
    the same or of the next step reads -- the squared-sum partials the gradient-writing kernels leave for the optimizer's norm pass --
    must not move between an eager step and a captured one."""
    k = (key, int(n), str(device), dtype)
    buf = _persistent.get(k)
    if buf is None:
        # never evicted: the addresses are baked into captured hipGraphs (BatchNorm-backward tags, the one-launch LSTM's workspace,
        # squared-sum partials); the buffers are a few KB each
        buf = _persistent[k] = torch.zeros(int(n), dtype=dtype, device=device)
    return buf


last_reduce_bytes = 0


def wgrad_reduce_pending(pend, sumsq=False):
    """Run every reduce recorded in `pend` in ONE launch on the current stream (drn_wgrad_reduce_pending).  sumsq=True: the launch also
    leaves the squared sums of what it wrote; returns (ranges [(data_ptr, elements)] of the reduced gradients, partials tensor) -- or
    None when nothing was pending."""
    global last_reduce_bytes
    L = lib()
    n = len(pend)
    res = None
    ref = ctypes.byref(pend.c)
    if n > 0:
        last_reduce_bytes = int(L.drn_wgrad_pending_bytes(ref))      # (for the profile tables: the launch's HBM-roofline denominator)
    if n > 0 and sumsq:
        ranges = pend.outputs()
        blocks = int(L.drn_wgrad_pending_blocks(ref))
        dev = torch.device("cuda", torch.cuda.current_device())
        part = persistent_buffer(("wgrad_reduce_all", ranges[0][0]), blocks, dev)
        check(L.drn_wgrad_reduce_pending(ref, _p(part), _stream()), "drn_wgrad_reduce_pending")
        res = (ranges, part)
    elif n > 0:
        check(L.drn_wgrad_reduce_pending(ref, None, _stream()), "drn_wgrad_reduce_pending")
    del pend.ws[:]
    return res


def gemm_wgrad(descs, dW, N, Cin, taps=1, stride=1, pad=0, w_layout=0, accumulate=False, dtype=F32):
    """dW (fp32) = sum over all groups / rows of dY^T * im2col(X); see include/drn_hip.h."""
    _need_gpu(dW)
    assert dW.dtype == torch.float32 and dW.is_contiguous()
    m_total = sum(d.M for d in descs)
    n_ws = lib().drn_wgrad_ws_elems(m_total, N, Cin, taps)
    ws = torch.empty(max(int(n_ws), 1), dtype=torch.float32, device=dW.device)
    arr = (WgradDesc * len(descs))(*descs)
    pend = pending_for([dW])
    tag = "gemm_wgrad[%s] g=%d M=%d N=%d K=%d" % ("bf16" if dtype == BF16 else "f32", len(descs), m_total, N, taps * Cin)
    _timed(tag, 2.0 * m_total * N * taps * Cin,
           lambda: check(lib().drn_gemm_wgrad(arr, len(descs), _p(dW), N, Cin, taps, stride, pad, w_layout, int(accumulate),
                                              _p(ws), dtype, ctypes.byref(pend.c) if pend is not None else None, _stream()),
                         "drn_gemm_wgrad"))
    if pend is not None:
        pend.ws.append(ws)                          # alive until the flush


def gemm_wgrad_multi(descs, dWs, N, Cin, taps=1, stride=1, pad=0, w_layout=0, accumulate=False, dtype=F32):
    """len(descs) independent weight gradients of equal N / taps (different weights / row counts) in one launch.  Cin: one int, or
    one per problem (the FPN laterals)."""
    for dW in dWs:
        _need_gpu(dW)
        assert dW.dtype == torch.float32 and dW.is_contiguous()
    cins = None
    if not isinstance(Cin, int):
        cins = (ctypes.c_int32 * len(descs))(*[int(c) for c in Cin])
        Cin = max(int(c) for c in Cin)
    n_ws = len(descs) * int(lib().drn_wgrad_ws_elems(max(d.M for d in descs), N, Cin, taps))
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dWs[0].device)
    arr = (WgradDesc * len(descs))(*descs)
    ptrs = (ctypes.c_void_p * len(dWs))(*[dW.data_ptr() for dW in dWs])
    m_total = sum(d.M for d in descs)
    pend = pending_for(dWs)
    tag = "gemm_wgrad_multi[%s] n=%d M=%d N=%d K=%d" % ("bf16" if dtype == BF16 else "f32", len(descs), m_total, N, taps * Cin)
    flops = sum(2.0 * d.M * N * taps * (cins[i] if cins is not None else Cin) for i, d in enumerate(descs))
    _timed(tag, flops,
           lambda: check(lib().drn_gemm_wgrad_multi(arr, len(descs), ptrs, N, Cin, cins, taps, stride, pad, w_layout, int(accumulate),
                                                    _p(ws), dtype, ctypes.byref(pend.c) if pend is not None else None, _stream()),
                         "drn_gemm_wgrad_multi"))
    if pend is not None:
        pend.ws.append(ws)


# ---------------------------------------------------------------------------------------------
# HBM-bound helpers
# ---------------------------------------------------------------------------------------------
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}
_ws_cache = {}
_ws_retired = []          # outgrown buffers stay allocated: a hipGraph captured earlier still writes to them on replay


def workspace(n_floats, device):
    """A grow-only fp32 scratch buffer per device AND stream (stream-ordered reuse on torch's current stream; two streams
    that run side by side -- drn_amd.graph.DualStreamStep -- never share one)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < n_floats:
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(int(n_floats * 1.25) + 1024, dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


def cast(x, dtype):
    """fp32 -> compute dtype (contiguous)."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(x.shape, dtype=TORCH_DT[dtype], device=x.device)
    check(lib().drn_cast(_p(x), _p(out), ctypes.c_int64(x.numel()), dtype, _stream()), "drn_cast")
    return out


def cast_transpose(x, dtype):
    """fp32 (M, K) -> (compute-dtype copy (M, K), its transpose (K, M)) in one pass."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    M, K = x.shape
    out = torch.empty((M, K), dtype=TORCH_DT[dtype], device=x.device)
    outT = torch.empty((K, M), dtype=TORCH_DT[dtype], device=x.device)
    if CAST_THROTTLE > 0:
        check(lib().drn_cast_transpose_throttled(_p(x), _p(out), _p(outT), M, K, dtype, CAST_THROTTLE, _stream()), "drn_cast_transpose_throttled")
    else:
        check(lib().drn_cast_transpose(_p(x), _p(out), _p(outT), M, K, dtype, _stream()), "drn_cast_transpose")
    return out, outT


# > 0: cast_transpose runs with at most that many workgroups resident (set by schedules that run the input preparation beside
# the query encoder: drn_amd.graph.ForkedStep)
CAST_THROTTLE = 0


def transpose2d(x, dtype):
    """(M, K) row-major -> (K, M) row-major, compute dtype, one LDS-tiled pass."""
    _need_gpu(x)
    M, K = x.shape
    assert x.stride(1) == 1
    out = torch.empty((K, M), dtype=x.dtype, device=x.device)
    check(lib().drn_transpose2d(_p(x), x.stride(0), _p(out), M, M, K, dtype, _stream()), "drn_transpose2d")
    return out


def pack_weight(w, perm, dtype):
    """out = w.permute(perm).contiguous() in compute dtype; w is a 3-D fp32 parameter (any strides)."""
    _need_gpu(w)
    assert w.dtype == torch.float32 and w.dim() == 3
    shape = [w.shape[i] for i in perm]
    st = [w.stride(i) for i in perm]
    out = torch.empty(shape, dtype=TORCH_DT[dtype], device=w.device)
    check(lib().drn_pack_weight(_p(w), _p(out), shape[0], shape[1], shape[2], ctypes.c_int64(st[0]), ctypes.c_int64(st[1]),
                                ctypes.c_int64(st[2]), dtype, _stream()), "drn_pack_weight")
    return out


def _row_stride(out):
    """Elements between consecutive rows of `out` viewed as (rows, C); size-1 dims carry meaningless strides."""
    for dim in range(out.dim() - 2, -1, -1):
        if out.shape[dim] > 1:
            return out.stride(dim)
    return 0


def pack_weights_into(items, dtype):
    """items: [(w, perm, out)] -- refresh existing re-laid copies `out` of fp32 weights `w` in one launch.  `out` may be a
    column block of a wider buffer (its row stride is honoured)."""
    from ._lib import PackDesc
    arr = (PackDesc * len(items))()
    for i, (w, perm, out) in enumerate(items):
        _need_gpu(w, out)
        d = arr[i]
        d.in_, d.out = _p(w), _p(out)
        d.A, d.B, d.C = (w.shape[j] for j in perm)
        d.sa, d.sb, d.sc = (w.stride(j) for j in perm)
        d.ldo = _row_stride(out)
    check(lib().drn_pack_weights(arr, len(items), dtype, _stream()), "drn_pack_weights")


_qd_counters = {}


def _counters(device):
    """DRN_QD_COUNTERS zeroed int32 arrival counters per device and stream for the K-split dense kernels (they re-arm
    themselves)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    c = _qd_counters.get(key)
    if c is None:
        c = _qd_counters[key] = torch.zeros(_lib.QD_COUNTERS, dtype=torch.int32, device=device)
    return c


def skinny_group(probs):
    """probs: list of dict(X (M<=64, K) fp32 [row stride % 4 == 0], W (N, K) contiguous, bias=None, mask=None, relu=False,
    Y=None): Y = X W^T (+bias)(ReLU)(zero where mask <= 0) for all problems in ONE launch (per DRN_QD_MAX problems).
    Returns the outputs.  Exact-fp32 MFMA, deterministic (drn_amd/csrc/qdense.hip)."""
    outs = []
    for c0 in range(0, len(probs), _lib.QD_MAX):
        chunk = probs[c0:c0 + _lib.QD_MAX]
        arr = (_lib.SkinnyDesc * len(chunk))()
        dev = chunk[0]["X"].device
        for d, q in zip(arr, chunk):
            X, W = q["X"], q["W"]
            _need_gpu(X, W)
            M, K = X.shape
            N = W.shape[0]
            assert W.shape[1] == K and W.is_contiguous() and X.stride(1) == 1 and W.dtype == torch.float32
            assert X.dtype in (torch.float32, torch.bfloat16)       # bf16 rows: the bf16 model's low-precision backward products
            Y = q.get("Y")
            if Y is None:
                Y = torch.empty((M, N), dtype=torch.float32, device=dev)
            mask = q.get("mask")
            d.X, d.W, d.bias, d.mask, d.Y = _p(X), _p(W), _p(q.get("bias")), _p(mask), _p(Y)
            d.ldx, d.ldy, d.ldm = X.stride(0), Y.stride(0), (mask.stride(0) if mask is not None else 0)
            d.M, d.N, d.K, d.relu = M, N, K, int(bool(q.get("relu")))
            d.x_dtype = BF16 if X.dtype == torch.bfloat16 else F32
            outs.append(Y)
        n_ws = int(lib().drn_skinny_group_ws_elems(arr, len(chunk)))
        ws = workspace(n_ws, dev) if n_ws else None
        check(lib().drn_skinny_group(arr, len(chunk), _p(ws), _p(_counters(dev)), _stream()), "drn_skinny_group")
    return outs


def skinny_linear(x, W, bias=None, relu=False, mask=None):
    """y = x W^T (+ bias)(ReLU) for batch-sized x (M <= 64 rows), fp32."""
    return skinny_group([dict(X=x, W=W, bias=bias, relu=relu, mask=mask)])[0]


def skinny_rows(X, W, bias=None):
    """Y = X W^T for a taller X (e.g. clips x words rows): 64-row blocks of X as the problems of grouped launches."""
    M = X.shape[0]
    Y = torch.empty((M, W.shape[0]), dtype=torch.float32, device=X.device)
    skinny_group([dict(X=X[r:r + 64], W=W, bias=bias, Y=Y[r:r + 64]) for r in range(0, M, 64)])
    return Y


def outer_wgrad(probs, lowp=False):
    """probs: list of dict(dY (M, N), X (M, K) or None, dW (N, K) or None, db=None, db2=None): dW = dY^T X, db = db2 = column
    sums of dY, all problems in one launch per DRN_QD_MAX (drn_amd/csrc/qdense.hip).  lowp (the bf16 model): operands rounded to
    bf16 on their way into the MFMA, fp32 accumulation."""
    for c0 in range(0, len(probs), _lib.QD_MAX):
        chunk = probs[c0:c0 + _lib.QD_MAX]
        arr = (_lib.OuterDesc * len(chunk))()
        for d, q in zip(arr, chunk):
            dY, X, dW = q["dY"], q.get("X"), q.get("dW")
            _need_gpu(dY, X, dW)
            assert dY.stride(1) == 1 and dY.dtype == torch.float32
            d.dY, d.X, d.dW, d.db, d.db2 = _p(dY), _p(X), _p(dW), _p(q.get("db")), _p(q.get("db2"))
            d.ldy, d.M, d.N = dY.stride(0), dY.shape[0], dY.shape[1]
            if dW is not None:
                assert X.stride(1) == 1 and X.shape[0] == dY.shape[0] and dW.stride(1) == 1 and dW.shape == (dY.shape[1], X.shape[1])
                d.ldx, d.ldw, d.K = X.stride(0), dW.stride(0), X.shape[1]
        check(lib().drn_outer_wgrad(arr, len(chunk), BF16 if lowp else F32, _stream()), "drn_outer_wgrad")


def skinny_ok(M, N, K):
    return M <= 64 and K % 4 == 0


def touch(t):
    """Stream a tensor through the caches (drn_touch)."""
    check(lib().drn_touch(_p(t), ctypes.c_int64(t.numel() * t.element_size()), _stream()), "drn_touch")


def copy_multi(pairs):
    """pairs: [(dst, src or None)] device tensors -- one launch (drn_copy_multi).  Contiguous pairs of equal byte size are flat
    copies (src None: zero-fill); a 2-D `src` with fewer columns than the contiguous 2-D `dst` (same rows, same dtype) is copied into
    the leading columns and the rest of every row is zeroed."""
    n = len(pairs)
    assert 1 <= n <= 8
    rows2d = (ctypes.c_int32 * (3 * n))()
    for i, (d, s_) in enumerate(pairs):
        _need_gpu(d, s_)
        assert d.is_contiguous()
        if s_ is None or (s_.is_contiguous() and s_.numel() == d.numel() and s_.dtype == d.dtype):
            continue
        assert s_.dim() == 2 and d.dim() == 2 and s_.dtype == d.dtype and s_.shape[0] == d.shape[0] and s_.shape[1] <= d.shape[1] \
            and s_.stride(1) == 1, "copy_multi: a padded pair needs (rows, <= cols) -> (rows, cols) of one dtype"
        es = d.element_size()
        rows2d[3 * i], rows2d[3 * i + 1], rows2d[3 * i + 2] = s_.shape[1] * es, s_.stride(0) * es, d.shape[1] * es
    srcs = (ctypes.c_void_p * n)(*[s_.data_ptr() if s_ is not None else None for _, s_ in pairs])
    dsts = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    nbytes = (ctypes.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in pairs])
    check(lib().drn_copy_multi(srcs, dsts, nbytes, rows2d, n, _stream()), "drn_copy_multi")


def pos_feat(start_end):
    """(B, T, 2) fp64 / fp32 proposal boundaries -> (B, T, 3) fp32 [start, end, end - start] (main_model.py:51-55)."""
    _need_gpu(start_end)
    se = start_end.contiguous()
    out = torch.empty(se.shape[:-1] + (3,), dtype=torch.float32, device=se.device)
    check(lib().drn_pos_feat(_p(se), int(se.dtype == torch.float64), _p(out), se.numel() // 2, _stream()), "drn_pos_feat")
    return out


def pos_embed_fwd(feat, W, b, out2d, ld_out, M, C, dtype):
    check(lib().drn_pos_embed_fwd(_p(feat), _p(W), _p(b), _p(out2d), ld_out, M, C, dtype, _stream()), "drn_pos_embed_fwd")


def pos_embed_bwd(dout, ld, feat, M, C, dW, db, dtype, accumulate=False):
    ws = workspace(1024 * C, dW.device)
    check(lib().drn_pos_embed_bwd(_p(dout), ld, _p(feat), M, C, _p(dW), _p(db), int(accumulate), _p(ws), dtype, _stream()),
          "drn_pos_embed_bwd")


def conv_tail_bwd(dY, ld_dy, B, Lo, Cout, wd_tail, ldw, k, stride, pad, feat, L, P, dW, db, dtype, accumulate=False):
    """Position-embedding gradients through the conv that reads the embedding (drn_conv_tail_bwd)."""
    L_ = lib()
    ws = workspace(int(L_.drn_conv_tail_bwd_ws_elems(B * Lo, k, Cout)), dW.device)
    check(L_.drn_conv_tail_bwd(_p(dY), ld_dy, B, Lo, Cout, _p(wd_tail), ctypes.c_int64(ldw), k, stride, pad, _p(feat), L, P, _p(dW),
                               _p(db), int(accumulate), _p(ws), dtype, _stream()), "drn_conv_tail_bwd")


def pairsum_add(dst, ld_dst, src, ld_src, Mdst, C, dtype, accumulate=True):
    check(lib().drn_pairsum_add(_p(dst), ld_dst, _p(src), ld_src, Mdst, C, int(accumulate), dtype, _stream()), "drn_pairsum_add")


def pairsum_chain3(d0, own1, d1, own2, d2, M1, C, dtype):
    """d1 = own1 + pairs(d0), d2 = own2 + pairs(d1) in one launch (all row strides C); the bits of two pairsum_add_to launches."""
    check(lib().drn_pairsum_chain3(_p(d0), C, _p(own1), C, _p(d1), C, _p(own2), C, _p(d2), C, M1, C, dtype, _stream()), "drn_pairsum_chain3")


def pairsum_add_to(dst, ld_dst, base, ld_base, src, ld_src, Mdst, C, dtype):
    check(lib().drn_pairsum_add_to(_p(dst), ld_dst, _p(base), ld_base, _p(src), ld_src, Mdst, C, dtype, _stream()), "drn_pairsum_add_to")


def gate_fwd(z, ld_z, gate, out, ld_out, nseq, L, C, dtype):
    """out[s, t, :C] = z[s, t, :C] * gate[s]  (the level-0 query gate as its own pass, see drn_amd.graph.ForkedStep)."""
    check(lib().drn_gate_fwd(_p(z), ld_z, _p(gate), gate.stride(0), _p(out), ld_out, nseq, L, C, dtype, _stream()), "drn_gate_fwd")


def gate_gather_fwd(z, ld_z, gate, pos, ld_pos, vid, V, out, ld_out, Q, L, C, P, dtype, vid_host=None):
    """out[q, t, :C] = z[vid[q], t, :C] * gate[q] and out[q, t, C:C+P] = pos[vid[q], t, :P] (drn_gate_gather_fwd): Q queries over V
    shared videos, written into conv0's (Q, L, C+P) input.  vid: (Q,) int32 on the device; vid_host: an optional host copy (int32,
    contiguous) -- given, an index outside [0, V) raises before the launch; without it the kernel writes zeros for such a query."""
    _need_gpu(z, gate, pos, vid, out)
    if vid.dtype != torch.int32 or not vid.is_contiguous() or vid.numel() != Q:
        raise _lib.DrnError("gate_gather_fwd: vid must be a contiguous int32 tensor of %d entries" % Q)
    host = None
    if vid_host is not None:
        if vid_host.is_cuda or vid_host.dtype != torch.int32 or not vid_host.is_contiguous() or vid_host.numel() != Q:
            raise _lib.DrnError("gate_gather_fwd: vid_host must be a contiguous int32 host tensor of %d entries" % Q)
        host = ctypes.c_void_p(vid_host.data_ptr())
    check(lib().drn_gate_gather_fwd(_p(z), ld_z, _p(gate), gate.stride(0), _p(pos), ld_pos, _p(vid), host, V, _p(out), ld_out, Q, L, C, P,
                                    dtype, _stream()), "drn_gate_gather_fwd")


def gate_gather_packed(rows, pad_row, prop_off, gate, pq, pv, vids, out, L, C, P, dtype, pq_host=None):
    """out[p, t, :C] = rows[src, :C] * gate[pq[p]] and out[p, t, C:C+P] = rows[src, C:C+P] with v = vids[pv[p]] and
    src = prop_off[v] + t while t is below video v's proposal count, else pad_row (drn_gate_gather_packed): conv0's whole (Q, L, C+P)
    input in one launch from a packed index (drn_amd.SearchIndex: rows (n_rows, >= C+P), prop_off (Nv + 1,) int32 on the device).
    pq, pv: (Q,) int32 on the device, vids: (Vc,) int32 store positions on the device; a slot or a position out of range reads the
    pad row.  pq_host: an optional host copy of pq (int32, contiguous) -- given, an entry outside [0, S) raises before the launch;
    without it pq is the caller's to keep in range.  P may be 0."""
    _need_gpu(rows, prop_off, gate, pq, pv, vids, out)
    Q = int(pq.numel())
    for name, t, n in (("pq", pq, Q), ("pv", pv, Q), ("vids", vids, int(vids.numel())), ("prop_off", prop_off, int(prop_off.numel()))):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != n or n < 1:
            raise _lib.DrnError("gate_gather_packed: %s must be a contiguous 1-d int32 tensor (pq and pv of the same length)" % name)
    if rows.dim() != 2 or rows.stride(1) != 1 or gate.dim() != 2 or gate.stride(1) != 1 or gate.dtype != torch.float32:
        raise _lib.DrnError("gate_gather_packed: rows must be (n_rows, C + P) and gate (S, C) float32, both with unit column stride")
    if out.dim() != 3 or tuple(out.shape[:2]) != (Q, L) or not out.is_contiguous() or out.dtype != rows.dtype:
        raise _lib.DrnError("gate_gather_packed: out must be a contiguous (%d, %d, >= C + P) tensor of the rows' dtype" % (Q, L))
    host = None
    if pq_host is not None:
        if pq_host.is_cuda or pq_host.dtype != torch.int32 or not pq_host.is_contiguous() or pq_host.numel() != Q:
            raise _lib.DrnError("gate_gather_packed: pq_host must be a contiguous int32 host tensor of %d entries" % Q)
        host = ctypes.c_void_p(pq_host.data_ptr())
    _timed("gate_gather_packed", 0, lambda: check(lib().drn_gate_gather_packed(
        _p(rows), rows.stride(0), int(rows.shape[0]), int(pad_row), _p(prop_off), int(prop_off.numel()) - 1, _p(gate), gate.stride(0),
        int(gate.shape[0]), _p(pq), host, _p(pv), _p(vids), int(vids.numel()), _p(out), int(out.shape[2]), Q, L, C, P, dtype, _stream()),
        "drn_gate_gather_packed"))


def quantize_rows_mx8(x, codes, scales):
    """x (n, C) float32 / bfloat16, C % 32 == 0 -> codes (n, C) uint8 (OCP e4m3fn) and scales (n, C / 32) uint8 (e8m0: one
    power-of-two scale per 32 columns), written in place by one launch (drn_quantize_rows_mx8; drn_amd.index.mx8_quantize is the
    definition).  All three with unit column stride; codes / scales may be row slices of wider tables."""
    for name, t, width in (("codes", codes, int(x.shape[-1])), ("scales", scales, int(x.shape[-1]) // 32)):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1 or tuple(t.shape) != (int(x.shape[0]), width):
            raise _lib.DrnError("quantize_rows_mx8: %s must be a (%d, %d) uint8 tensor with unit column stride" % (name, x.shape[0], width))
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.DrnError("quantize_rows_mx8: x must be (n, C) with unit column stride")
    _need_gpu(x, codes, scales)
    _timed("quantize_rows_mx8", 0, lambda: check(lib().drn_quantize_rows_mx8(
        _p(x), x.stride(0), int(x.shape[0]), int(x.shape[1]), _p(codes), codes.stride(0), _p(scales), scales.stride(0), dtype_code(x),
        _stream()), "drn_quantize_rows_mx8"))


def gate_gather_packed_q8(codes, scales, pos, pad_row, prop_off, gate, pq, pv, vids, out, L, C, P, dtype, pq_host=None):
    """gate_gather_packed on a quantised index (drn_gate_gather_packed_q8): the gated columns of row src are
    float(codes[src, c]) * 2^(scales[src, c // 32] - 127) -- codes (n_rows, >= C) and scales (n_rows, >= C / 32) uint8 as
    quantize_rows_mx8 writes them -- and the position columns pos[src, :P] in out's dtype (pos None with P = 0).  Everything else as
    there; the output is bit for bit gate_gather_packed's on rows holding the dequantised values."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2 or codes.stride(1) != 1 \
            or scales.stride(1) != 1 or codes.shape[0] != scales.shape[0] or codes.shape[1] < C or scales.shape[1] * 32 < C:
        raise _lib.DrnError("gate_gather_packed_q8: codes (n_rows, >= C) and scales (n_rows, >= C / 32) must be uint8 with unit column stride")
    if (pos is None) != (P == 0) or (pos is not None and (pos.dim() != 2 or pos.stride(1) != 1 or pos.dtype != out.dtype
                                                          or pos.shape[0] != codes.shape[0] or pos.shape[1] < P)):
        raise _lib.DrnError("gate_gather_packed_q8: pos must be (n_rows, >= P) of out's dtype with unit column stride (None with P = 0)")
    _need_gpu(codes, scales, pos, prop_off, gate, pq, pv, vids, out)
    Q = int(pq.numel())
    for name, t, n in (("pq", pq, Q), ("pv", pv, Q), ("vids", vids, int(vids.numel())), ("prop_off", prop_off, int(prop_off.numel()))):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != n or n < 1:
            raise _lib.DrnError("gate_gather_packed_q8: %s must be a contiguous 1-d int32 tensor (pq and pv of the same length)" % name)
    if gate.dim() != 2 or gate.stride(1) != 1 or gate.dtype != torch.float32:
        raise _lib.DrnError("gate_gather_packed_q8: gate must be (S, C) float32 with unit column stride")
    if out.dim() != 3 or tuple(out.shape[:2]) != (Q, L) or not out.is_contiguous() or dtype_code(out) != dtype:
        raise _lib.DrnError("gate_gather_packed_q8: out must be a contiguous (%d, %d, >= C + P) tensor of the given dtype" % (Q, L))
    host = None
    if pq_host is not None:
        if pq_host.is_cuda or pq_host.dtype != torch.int32 or not pq_host.is_contiguous() or pq_host.numel() != Q:
            raise _lib.DrnError("gate_gather_packed_q8: pq_host must be a contiguous int32 host tensor of %d entries" % Q)
        host = ctypes.c_void_p(pq_host.data_ptr())
    _timed("gate_gather_packed_q8", 0, lambda: check(lib().drn_gate_gather_packed_q8(
        _p(codes), codes.stride(0), _p(scales), scales.stride(0), _p(pos), pos.stride(0) if pos is not None else 0, int(codes.shape[0]),
        int(pad_row), _p(prop_off), int(prop_off.numel()) - 1, _p(gate), gate.stride(0), int(gate.shape[0]), _p(pq), host, _p(pv), _p(vids),
        int(vids.numel()), _p(out), int(out.shape[2]), Q, L, C, P, dtype, _stream()), "drn_gate_gather_packed_q8"))


def gate_quantize_weights_mx8(w, gate, D, Dp, wcodes, wscales):
    """conv0's gated weights of S sentences in the index's block-scaled FP8 format, one launch (drn_gate_quantize_weights_mx8;
    drn_amd.index.mx8_gate_weights is the definition): w (3, Cout, >= D) float32, tap-major with unit column stride and contiguous
    rows (functional.packed(weight, (2, 0, 1), F32)), gate (S, >= D) float32 -> wcodes (S, 3, Cout, >= Dp) and wscales
    (S, 3, Cout, >= Dp / 32) uint8, written in place; their leading three dims contiguous (column slices of wider buffers are allowed),
    columns [D, Dp) zero codes."""
    D, Dp = int(D), int(Dp)
    if w.dim() != 3 or w.shape[0] != 3 or w.dtype != torch.float32 or w.stride(2) != 1 or w.stride(0) != w.shape[1] * w.stride(1) \
            or w.shape[2] < D:
        raise _lib.DrnError("gate_quantize_weights_mx8: w must be (3, Cout, >= D) float32, tap-major with unit column stride")
    if gate.dim() != 2 or gate.stride(1) != 1 or gate.dtype != torch.float32 or gate.shape[1] < D:
        raise _lib.DrnError("gate_quantize_weights_mx8: gate must be (S, >= D) float32 with unit column stride")
    S, Cout = int(gate.shape[0]), int(w.shape[1])
    if D < 1 or Dp < D or Dp % 32:
        raise _lib.DrnError("gate_quantize_weights_mx8: Dp = %d must be a multiple of 32 and at least D = %d" % (Dp, D))
    for name, t, width in (("wcodes", wcodes, Dp), ("wscales", wscales, Dp // 32)):
        if t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[:3]) != (S, 3, Cout) or t.shape[3] < width or t.stride(3) != 1 \
                or t.stride(1) != Cout * t.stride(2) or t.stride(0) != 3 * Cout * t.stride(2):
            raise _lib.DrnError("gate_quantize_weights_mx8: %s must be a (%d, 3, %d, >= %d) uint8 tensor with unit column stride"
                                % (name, S, Cout, width))
    _need_gpu(w, gate, wcodes, wscales)
    _timed("gate_quantize_weights_mx8", 0, lambda: check(lib().drn_gate_quantize_weights_mx8(
        _p(w), w.stride(1), _p(gate), gate.stride(0), S, Cout, D, Dp, _p(wcodes), wcodes.stride(2), _p(wscales), wscales.stride(2),
        _stream()), "drn_gate_quantize_weights_mx8"))


def _conv0_mx8_operands(who, codes, scales, pos, prop_off, wcodes, wscales, wpos, pq, pv, vids, dests, L, C, P, pq_host, wide=False):
    """The argument checks conv0_mx8 and conv0_mx8_bn share -> (S, Cout, Q, pq_host's pointer or None).  dests: (name, tensor) pairs, each
    a contiguous (Q, L, Cout) bfloat16 or float32 tensor; wide: a column slice of a contiguous (Q, L, >= Cout) tensor serves as well."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2 or codes.stride(1) != 1 \
            or scales.stride(1) != 1 or codes.shape[0] != scales.shape[0] or codes.shape[1] < C or scales.shape[1] * 32 < C:
        raise _lib.DrnError("%s: codes (n_rows, >= C) and scales (n_rows, >= C / 32) must be uint8 with unit column stride" % who)
    if C < 32 or C % 32 or P < 0 or P % 32:
        raise _lib.DrnError("%s: C = %d and P = %d must be multiples of 32 (C at least 32)" % (who, C, P))
    if wcodes.dtype != torch.uint8 or wscales.dtype != torch.uint8 or wcodes.dim() != 4 or wscales.dim() != 4 or not wcodes.is_contiguous() \
            or not wscales.is_contiguous() or wcodes.shape[1] != 3 or wcodes.shape[3] != C \
            or tuple(wscales.shape) != tuple(wcodes.shape[:3]) + (C // 32,):
        raise _lib.DrnError("%s: wcodes (S, 3, Cout, C) and wscales (S, 3, Cout, C / 32) must be contiguous uint8" % who)
    S, Cout = int(wcodes.shape[0]), int(wcodes.shape[2])
    if Cout % 16:
        raise _lib.DrnError("%s: Cout = %d is not a multiple of 16" % (who, Cout))
    if (pos is None) != (P == 0) or (pos is not None and (pos.dim() != 2 or pos.stride(1) != 1 or pos.dtype != torch.bfloat16
                                                          or pos.shape[0] != codes.shape[0] or pos.shape[1] < P)):
        raise _lib.DrnError("%s: pos must be (n_rows, >= P) bfloat16 with unit column stride (None with P = 0)" % who)
    if (wpos is None) != (P == 0) or (wpos is not None and (wpos.dtype != torch.bfloat16 or tuple(wpos.shape) != (3, Cout, P)
                                                            or not wpos.is_contiguous())):
        raise _lib.DrnError("%s: wpos must be a contiguous (3, %d, %d) bfloat16 tensor (None with P = 0)" % (who, Cout, P))
    _need_gpu(codes, scales, pos, prop_off, wcodes, wscales, wpos, pq, pv, vids, *[t for _, t in dests])
    Q = int(pq.numel())
    for name, t, n in (("pq", pq, Q), ("pv", pv, Q), ("vids", vids, int(vids.numel())), ("prop_off", prop_off, int(prop_off.numel()))):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != n or n < 1:
            raise _lib.DrnError("%s: %s must be a contiguous 1-d int32 tensor (pq and pv of the same length)" % (who, name))
    for name, t in dests:
        if t is None or t.dim() != 3 or tuple(t.shape) != (Q, L, Cout) or t.dtype not in (torch.bfloat16, torch.float32) \
                or not (t.is_contiguous() or (wide and t.stride(2) == 1 and t.stride(1) >= Cout and t.stride(0) == L * t.stride(1))):
            raise _lib.DrnError("%s: %s must be a contiguous (%d, %d, %d) bfloat16 or float32 tensor" % (who, name, Q, L, Cout))
    host = None
    if pq_host is not None:
        if pq_host.is_cuda or pq_host.dtype != torch.int32 or not pq_host.is_contiguous() or pq_host.numel() != Q:
            raise _lib.DrnError("%s: pq_host must be a contiguous int32 host tensor of %d entries" % (who, Q))
        host = ctypes.c_void_p(pq_host.data_ptr())
    return S, Cout, Q, host


def conv0_mx8(codes, scales, pos, pad_row, prop_off, wcodes, wscales, wpos, pq, pv, vids, raw, L, C, P, pq_host=None):
    """conv0 (k = 3, stride 1, pad 1, no bias) of the input gate_gather_packed_q8 would have written, straight from the quantised
    index on block-scaled FP8 MFMAs (drn_conv0_mx8; drn_amd.index.mx8_conv0_reference is the definition): codes / scales / pos /
    pad_row / prop_off / pq / pv / vids / pq_host as there, with pos in bfloat16; wcodes (S, 3, Cout, C) and wscales
    (S, 3, Cout, C / 32) as gate_quantize_weights_mx8 writes them, contiguous; wpos (3, Cout, P) bfloat16 contiguous (None with
    P = 0): conv0's position weights, tap-major.  raw: (Q, L, Cout) contiguous, bfloat16 or float32, written in place.
    C % 32 == 0, P % 32 == 0, Cout % 16 == 0."""
    S, Cout, Q, host = _conv0_mx8_operands("conv0_mx8", codes, scales, pos, prop_off, wcodes, wscales, wpos, pq, pv, vids, [("raw", raw)],
                                           L, C, P, pq_host)
    flops = 2.0 * Q * L * Cout * 3 * (C + P)
    _timed("conv0_mx8", flops, lambda: check(lib().drn_conv0_mx8(
        _p(codes), codes.stride(0), _p(scales), scales.stride(0), _p(pos), pos.stride(0) if pos is not None else 0, int(codes.shape[0]),
        int(pad_row), _p(prop_off), int(prop_off.numel()) - 1, _p(wcodes), _p(wscales), _p(wpos), S, _p(pq), host, _p(pv), _p(vids),
        int(vids.numel()), _p(raw), Cout, int(raw.dtype == torch.float32), Q, L, C, P, Cout, _stream()), "drn_conv0_mx8"))


# The tiles drn_conv0_mx8_bn_tile ships, (rows of the flattened (pair, t) output, channels): the wide one, drn_conv0_mx8_bn's, first.
CONV0_MX8_WIDE = (256, 256)
CONV0_MX8_TILES = (CONV0_MX8_WIDE, (128, 64), (64, 64))
# drn_conv0_mx8_bn_choose's rule (MXN_SMALL_UPTO_16THS / MXN_MID_UPTO_16THS of csrc/qconv.hip; tests/test_search_mx8tiles_cpu.py holds the
# two together): with W = cdiv(Q L, 256) cdiv(Cout, 256) wide-tile workgroups, 64 x 64 while 16 W <= CONV0_MX8_SMALL_UPTO_16THS x CUs,
# 128 x 64 while 16 W <= CONV0_MX8_MID_UPTO_16THS x CUs, wide above.
CONV0_MX8_SMALL_UPTO_16THS = 3
CONV0_MX8_MID_UPTO_16THS = 8


def _conv0_mx8_tile_arg(tile):
    """tile of conv0_mx8_bn -> None (the wide tile through drn_conv0_mx8_bn), "auto" or a shipped (rows, cols); anything else raises."""
    if tile is None:
        return None
    if isinstance(tile, str):
        if tile == "auto":
            return tile
    elif isinstance(tile, (tuple, list)) and len(tile) == 2 and all(type(v) is int for v in tile) and tuple(tile) in CONV0_MX8_TILES:
        return tuple(tile)
    raise _lib.DrnError("conv0_mx8_bn: tile must be None, \"auto\" or one of %s, not %r" % (list(CONV0_MX8_TILES), tile))


def conv0_mx8_bn_tile(Q, L, Cout):
    """(rows, cols) of the tile conv0_mx8_bn(tile="auto") takes for Q pairs of L rows and Cout channels on the current device
    (drn_conv0_mx8_bn_choose): a function of (Q L, Cout) and the device's compute-unit count alone."""
    rows, cols = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().drn_conv0_mx8_bn_choose(int(Q), int(L), int(Cout), ctypes.byref(rows), ctypes.byref(cols)), "drn_conv0_mx8_bn_choose")
    return int(rows.value), int(cols.value)


def conv0_mx8_bn(codes, scales, pos, pad_row, prop_off, wcodes, wscales, wpos, pq, pv, vids, ss, gate, out, gated, L, C, P, pq_host=None,
                 tile=None):
    """conv0_mx8 -> eval BatchNorm -> ReLU (-> gate) in ONE launch on LDS-staged tiles, without the raw tensor (drn_conv0_mx8_bn): the
    operands of conv0_mx8; ss (2, Cout) float32 contiguous as bn_eval_scale_shift writes it, or None for the bare convolution; gate
    (Q, >= Cout) float32 with unit column stride, one row per PAIR as bn_apply_multi takes it, or None; out and gated (None exactly
    when gate is) (Q, L, Cout) tensors of one dtype, bfloat16 or float32, contiguous or column slices of contiguous wider ones, written
    in place (nothing past a row's Cout columns is written):
    out = relu(acc * scale + shift) from the fp32 accumulator, gated = that, unrounded, times the pair's gate row.
    tile: None, the wide 256 x 256 tile through drn_conv0_mx8_bn; "auto", the tile conv0_mx8_bn_tile names for this grid; or one of
    CONV0_MX8_TILES (drn_conv0_mx8_bn_tile).  Every tile writes bit for bit the same out / gated; the launch tag is conv0_mx8_bn."""
    tile = _conv0_mx8_tile_arg(tile)
    if (gate is None) != (gated is None):
        raise _lib.DrnError("conv0_mx8_bn: gate and gated must come together (a gated output needs a gate)")
    dests = [("out", out)] + ([("gated", gated)] if gated is not None else [])
    S, Cout, Q, host = _conv0_mx8_operands("conv0_mx8_bn", codes, scales, pos, prop_off, wcodes, wscales, wpos, pq, pv, vids, dests, L, C,
                                           P, pq_host, wide=True)
    if gated is not None and gated.dtype != out.dtype:
        raise _lib.DrnError("conv0_mx8_bn: out and gated must have one dtype")
    if ss is not None and (ss.dtype != torch.float32 or tuple(ss.shape) != (2, Cout) or not ss.is_contiguous()):
        raise _lib.DrnError("conv0_mx8_bn: ss must be a contiguous (2, %d) float32 tensor" % Cout)
    if gate is not None and (gate.dtype != torch.float32 or gate.dim() != 2 or gate.shape[0] != Q or gate.shape[1] < Cout
                             or gate.stride(1) != 1):
        raise _lib.DrnError("conv0_mx8_bn: gate must be (%d, >= %d) float32 with unit column stride" % (Q, Cout))
    _need_gpu(ss, gate)
    flops = 2.0 * Q * L * Cout * 3 * (C + P)
    args = (_p(codes), codes.stride(0), _p(scales), scales.stride(0), _p(pos), pos.stride(0) if pos is not None else 0, int(codes.shape[0]),
            int(pad_row), _p(prop_off), int(prop_off.numel()) - 1, _p(wcodes), _p(wscales), _p(wpos), S, _p(pq), host, _p(pv), _p(vids),
            int(vids.numel()), _p(ss), _p(gate), gate.stride(0) if gate is not None else 0, _p(out), out.stride(1), _p(gated),
            gated.stride(1) if gated is not None else 0, int(out.dtype == torch.float32), Q, L, C, P, Cout)
    if tile == "auto":                                   # (the chooser, by its module name: what a test or a benchmark replaces)
        tile = conv0_mx8_bn_tile(Q, L, Cout)
    if tile is None:
        _timed("conv0_mx8_bn", flops, lambda: check(lib().drn_conv0_mx8_bn(*args, _stream()), "drn_conv0_mx8_bn"))
    else:
        _timed("conv0_mx8_bn", flops, lambda: check(lib().drn_conv0_mx8_bn_tile(*args, tile[0], tile[1], _stream()), "drn_conv0_mx8_bn_tile"))


def pool_props_lds_rows(B, D, dtype):
    """Rows of one video the LDS path of drn_pool_props holds for B clips of D elements (0: the element-wise path)."""
    return int(lib().drn_pool_props_lds_rows(int(B), int(D), int(dtype)))


def pool_props(feats, seg_off, prop_off, win, pse, vids, T, out, out_pse, vids_host=None, counts_host=None, max_rows=0, tag=None):
    """out[b, t] = max over rows seg_off[v] + lo .. seg_off[v] + hi of feats, out_pse[b, t] = pse[prop_off[v] + t] for v = vids[b],
    [lo, hi] = win[prop_off[v] + t], t < the video's proposal count; zeros past it (drn_pool_props: one launch, every element of
    out (B, T, D) and out_pse (B, T, 2) written once).  vids: (B,) int32 on the device.  vids_host / counts_host: optional host copies
    (int32, contiguous) of the indices and of the clips' proposal counts -- given, an index outside [0, Nv) or a count above T
    raises before the launch; without vids_host the kernel writes zeros for such a clip.  tag: name under ops.kernel_timer."""
    _need_gpu(feats, seg_off, prop_off, win, pse, vids, out, out_pse)
    B, Nv = int(vids.numel()), int(seg_off.numel()) - 1
    D = int(feats.shape[-1])
    for name, t, dt in (("seg_off", seg_off, torch.int64), ("prop_off", prop_off, torch.int32), ("win", win, torch.int32),
                        ("pse", pse, torch.float64), ("vids", vids, torch.int32), ("out_pse", out_pse, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise _lib.DrnError("pool_props: %s must be a contiguous %s tensor" % (name, dt))
    if out.dtype != feats.dtype or not out.is_contiguous() or not feats.is_contiguous() or tuple(out.shape) != (B, T, D) \
            or tuple(out_pse.shape) != (B, T, 2) or prop_off.numel() != Nv + 1 or win.shape[0] != pse.shape[0]:
        raise _lib.DrnError("pool_props: out must be a contiguous (%d, %d, %d) %s tensor and out_pse (%d, %d, 2)"
                            % (B, T, D, feats.dtype, B, T))
    host = []
    for name, t in (("vids_host", vids_host), ("counts_host", counts_host)):
        if t is not None and (t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != B):
            raise _lib.DrnError("pool_props: %s must be a contiguous int32 host tensor of %d entries" % (name, B))
        host.append(ctypes.c_void_p(t.data_ptr()) if t is not None and B else None)
    d = _lib.PoolPropsDesc(feats=_p(feats), seg_off=_p(seg_off), prop_off=_p(prop_off), win=_p(win), pse=_p(pse), vids=_p(vids),
                           vids_host=host[0], counts_host=host[1], out=_p(out), out_pse=_p(out_pse), Nv=Nv, B=B, T=int(T), D=D,
                           dtype=dtype_code(feats), max_rows=int(max_rows))
    if B == 0 or T == 0:
        return                                                                  # (nothing to write; data_ptr() of an empty tensor is null)
    _timed(tag or "pool_props", 0, lambda: check(lib().drn_pool_props(ctypes.byref(d), _stream()), "drn_pool_props"))


def gate_bwd(dG, ld_dg, act, ld_act, gate, dC, ld_dc, add, ld_add, dgate, nseq, L, C, dtype, dsum=None):
    """dC = (add or 0) + dG * gate; dgate = sum_t dG * act; dsum (nseq, C) fp32 = sum_t dG * gate."""
    check(lib().drn_gate_bwd(_p(dG), ld_dg, _p(act), ld_act, _p(gate), gate.stride(0), _p(add), ld_add, _p(dC), ld_dc, _p(dgate),
                             dgate.stride(0), _p(dsum), nseq, L, C, dtype, _stream()), "drn_gate_bwd")


def gate_bwd_t(dG, ld_dg, act, ld_act, gate, dCT, dgate, nseq, L, C, dtype, dsum=None):
    """dCT (C, nseq*L) = (dG * gate)^T; dgate = sum_t dG * act; dsum (nseq, C) = sum_t dG * gate."""
    check(lib().drn_gate_bwd_t(_p(dG), ld_dg, _p(act), ld_act, _p(gate), gate.stride(0), _p(dCT), ctypes.c_int64(dCT.stride(0)),
                               _p(dgate), dgate.stride(0), _p(dsum), nseq, L, C, dtype, _stream()), "drn_gate_bwd_t")


def colsum(X, ld, M, C, out, dtype, accumulate=False):
    ws = workspace(64 * C, out.device)
    check(lib().drn_colsum(_p(X), ld, M, C, _p(out), int(accumulate), _p(ws), dtype, _stream()), "drn_colsum")


# ---------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------
def bn_finalize(groups, C, gamma, beta, conv_bias, running_mean, running_var, momentum, eps):
    """groups: list of (stats, tiles, M, scale_shift, save)."""
    arr = (_lib.BnGroup * len(groups))(*[_lib.BnGroup(stats=_p(s), tiles=t, M=m, scale_shift=_p(ss), save=_p(sv))
                                         for (s, t, m, ss, sv) in groups])
    check(lib().drn_bn_finalize(arr, len(groups), C, _p(gamma), _p(beta), _p(conv_bias), _p(running_mean), _p(running_var),
                                ctypes.c_float(momentum), ctypes.c_float(eps), _stream()), "drn_bn_finalize")


def bn_finalize_multi(groups, C):
    """groups: list of dicts(stats, tiles, M, ss, save, gamma, beta, conv_bias, running_mean, running_var, momentum, eps);
    one launch, groups processed in order (they may share a BatchNorm module or not)."""
    arr = (_lib.BnFinDesc * len(groups))(*[
        _lib.BnFinDesc(stats=_p(g["stats"]), tiles=g["tiles"], M=g["M"], scale_shift=_p(g["ss"]), save=_p(g["save"]),
                       gamma=_p(g["gamma"]), beta=_p(g["beta"]), conv_bias=_p(g.get("conv_bias")),
                       running_mean=_p(g.get("running_mean")), running_var=_p(g.get("running_var")),
                       momentum=g["momentum"], eps=g["eps"]) for g in groups])
    check(lib().drn_bn_finalize_multi(arr, len(groups), C, _stream()), "drn_bn_finalize_multi")


def bn_apply_multi(levels, C, dtype, relu=True):
    """levels: list of dicts(raw, ld_raw, ss, out, ld_out, M, L[, up, ld_up, gate, gated, ld_gated]): one launch."""
    arr = (_lib.BnApplyDesc * len(levels))()
    for d, v in zip(arr, levels):
        gate = v.get("gate")
        d.raw, d.scale_shift, d.out = _p(v["raw"]), _p(v["ss"]), _p(v["out"])
        d.up, d.gate, d.gated = _p(v.get("up")), _p(gate), _p(v.get("gated"))
        d.ld_raw, d.ld_out, d.ld_up = v["ld_raw"], v["ld_out"], v.get("ld_up", 0)
        d.ldg, d.ld_gated = (gate.stride(0) if gate is not None else 0), v.get("ld_gated", 0)
        d.M, d.L = v["M"], v["L"]
    check(lib().drn_bn_apply_multi(arr, len(levels), C, int(relu), dtype, _stream()), "drn_bn_apply_multi")


def bn_train_apply(levels, C, dtype, relu=True):
    """Train-mode BatchNorm (+ReLU) forward of up to DRN_MAX_GROUPS levels in ONE launch (C % 64 == 0): levels = list of dicts
    with the statistics side (stats, tiles, ss, save, gamma, beta[, conv_bias, running_mean, running_var], momentum, eps) and
    the apply side (raw, ld_raw, out, ld_out, M, L[, up, ld_up, gate, gated, ld_gated]) of drn_bn_finalize_multi +
    drn_bn_apply_multi; the groups' running statistics are updated in list order."""
    arr = _bn_train_descs(levels)
    check(lib().drn_bn_train_apply(arr, len(levels), C, int(relu), dtype, _stream()), "drn_bn_train_apply")


def _bn_train_descs(levels):
    arr = (_lib.BnTrainDesc * len(levels))()
    for d, v in zip(arr, levels):
        gate = v.get("gate")
        d.stats, d.scale_shift, d.save, d.gamma, d.beta = _p(v.get("stats")), _p(v["ss"]), _p(v["save"]), _p(v["gamma"]), _p(v["beta"])
        d.conv_bias, d.running_mean, d.running_var = _p(v.get("conv_bias")), _p(v.get("running_mean")), _p(v.get("running_var"))
        d.raw, d.out, d.up, d.gate, d.gated = _p(v["raw"]), _p(v["out"]), _p(v.get("up")), _p(gate), _p(v.get("gated"))
        d.momentum, d.eps, d.tiles = v["momentum"], v["eps"], v["tiles"]
        d.ld_raw, d.ld_out, d.ld_up = v["ld_raw"], v["ld_out"], v.get("ld_up", 0)
        d.ldg, d.ld_gated = (gate.stride(0) if gate is not None else 0), v.get("ld_gated", 0)
        d.M, d.L = v["M"], v["L"]
    return arr


# conv -> BN(train) -> ReLU in ONE launch (drn_conv_bn_train): built, bit-identical to the two-launch path and stress-tested
# (tests/test_conv_bn_gpu.py) -- and OFF by default, because it measures slower inside the step (DESIGN.md section 8, round 4:
# FPN + heads forward 274 vs 257 us).  After a workgroup's K loop the hand-off is publish -> wait -> merge, three memory-side round
# trips plus 45 MB of L2-bypassing statistics reads per launch (11-13 us), against ~3 us of epilogue + a 6-15 us BatchNorm launch
# that reads the same statistics out of L2.  BN_FUSE = True turns it on (never together with DRN_FORCE_DEVICE, the test mode that
# puts several ranks on ONE GPU: its in-kernel wait needs the whole grid resident on a device this process owns).
BN_FUSE = False
DRN_ERR_UNSUPPORTED = -3


_bn_tagged = {}


def _bn_tagged_ws(device, nbytes):
    """(workspace, generation word) of the one-launch conv->BN kernel per device and stream: 64-bit {value, generation} pairs,
    zero at first and afterwards written by that kernel only (a pair is valid when it carries the current launch's generation,
    so the buffer is never cleared); grows in powers of two from 16 MB (a new, zeroed buffer; the generation keeps counting)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    ent = _bn_tagged.get(key)
    if ent is None or ent[0].numel() * 8 < nbytes:
        n = 1 << 21
        while n * 8 < nbytes:
            n *= 2
        gen = ent[1] if ent is not None else torch.zeros(1, dtype=torch.int32, device=device)
        retired = ent[2] + [ent[0]] if ent is not None else []      # (a captured hipGraph may still point into the old buffer)
        ent = _bn_tagged[key] = (torch.zeros(n, dtype=torch.int64, device=device), gen, retired)
    return ent[0], ent[1]


def conv_bn_train(descs, levels, dtype, relu=True, up_group=None):
    """descs: gemm_desc per group (no bias / gate / C2; `stats` unused); levels: the bn_train_apply dicts of the same groups
    (raw = the GEMM's C; `stats` unused).  up_group[i] = j: out_i += nearest_x2(out_j) inside the launch (the FPN top-down chain).
    -> True when launched; False when this launch cannot be fused (the caller runs gemm_nt + bn_train_apply)."""
    if not BN_FUSE or _ksplit(descs, dtype) > 1:
        return False
    arr = (GemmDesc * len(descs))(*descs)
    barr = _bn_train_descs(levels)
    ug = (ctypes.c_int32 * len(descs))(*[int(u) for u in up_group]) if up_group is not None else None
    dev = torch.device("cuda", torch.cuda.current_device())
    nbytes = int(lib().drn_conv_bn_train_ws_bytes(arr, len(descs)))
    ws, gen = _bn_tagged_ws(dev, nbytes)
    d0 = descs[0]
    flops = sum(2.0 * d.M * d.N * d.taps * d.Cin for d in descs)
    tag = "gemm_nt[%s] g=%d M=%d N=%d K=%d mode=0 +bn" % ("bf16" if dtype == BF16 else "f32", len(descs), sum(d.M for d in descs), d0.N,
                                                           d0.taps * d0.Cin)
    rc = []
    _timed(tag, flops, lambda: rc.append(lib().drn_conv_bn_train(arr, barr, len(descs), int(relu), ug, _p(ws), ctypes.c_int64(ws.numel() * 8),
                                                                 _p(gen), dtype, _stream())))
    if rc[0] == DRN_ERR_UNSUPPORTED:
        if kernel_timer is not None:
            kernel_timer.pop()
        return False
    check(rc[0], "drn_conv_bn_train")
    return True


# conv -> BN(eval) -> ReLU in ONE launch (drn_conv_bn_eval): eval BatchNorm is a per-channel affine map, so it runs in the GEMM's
# epilogue and the raw tensor is never written.  Opt-in (functional.fused_eval); conv_bn_eval_launches counts the launches that ran.
KSPLIT_EVAL_RELU = 0x1000000
conv_bn_eval_launches = 0


def _bn_apply_descs(levels):
    arr = (_lib.BnApplyDesc * len(levels))()
    for d, v in zip(arr, levels):
        gate = v.get("gate")
        d.raw, d.scale_shift, d.out = _p(v.get("raw")), _p(v["ss"]), _p(v["out"])
        d.up, d.gate, d.gated = _p(v.get("up")), _p(gate), _p(v.get("gated") if gate is not None else None)
        d.ld_raw, d.ld_out, d.ld_up = v.get("ld_raw", 0), v["ld_out"], v.get("ld_up", 0)
        d.ldg, d.ld_gated = (gate.stride(0) if gate is not None else 0), v.get("ld_gated", 0)
        d.M, d.L = v["M"], v["L"]
    return arr


def _conv_bn_eval_call(descs, levels, dtype, relu, plan):
    """-> the library's return code: the launch (or, plan=True, the kernel kind it would run on) with the split gemm_nt would choose for
    the same problems, so that a stage keeps its kernel and its K order; DRN_ERR_UNSUPPORTED where that split has no fused form."""
    global conv_bn_eval_launches
    arr = (GemmDesc * len(descs))(*descs)
    barr = _bn_apply_descs(levels)
    ks = _ksplit_w4h(descs, dtype)
    if ks == 1:
        if _ksplit256(descs, dtype) > 1:
            return DRN_ERR_UNSUPPORTED
        ks = _ksplit(descs, dtype)
        if ks > 1 and len(descs) > 1:          # the grouped K-split has no fused form
            return DRN_ERR_UNSUPPORTED
    d0 = descs[0]
    if plan:
        return lib().drn_conv_bn_eval_splitk_plan(arr, barr, ks, dtype) if ks > 1 else lib().drn_conv_bn_eval_plan(arr, barr, len(descs), dtype)
    flops = sum(2.0 * d.M * d.N * d.taps * d.Cin for d in descs)
    tag = "gemm_nt[%s] g=%d M=%d N=%d K=%d mode=0 +bn(eval)%s" % ("bf16" if dtype == BF16 else "f32", len(descs), sum(d.M for d in descs), d0.N,
                                                                 d0.taps * d0.Cin, " splitK=%d" % ks if ks > 1 else "")
    rc = []
    if ks > 1:
        dev = torch.device("cuda", torch.cuda.current_device())
        tiles = ((d0.M + 127) // 128) * ((d0.N + 127) // 128)
        ws = torch.empty(ks * max(tiles * 128 * 128, d0.M * d0.N), dtype=torch.float32, device=dev)
        arg = _ksplit_arg(ks) | (KSPLIT_EVAL_RELU if relu else 0)
        _timed(tag, flops, lambda: rc.append(lib().drn_conv_bn_eval_splitk(arr, barr, arg, _p(ws), _p(_counters(dev)), dtype, _stream())))
    else:
        _timed(tag, flops, lambda: rc.append(lib().drn_conv_bn_eval(arr, barr, len(descs), int(relu), dtype, _stream())))
    if rc[0] == DRN_ERR_UNSUPPORTED and kernel_timer is not None:
        kernel_timer.pop()
    if rc[0] == 0:
        conv_bn_eval_launches += 1
    return rc[0]


def conv_bn_eval(descs, levels, dtype, relu=True):
    """descs: gemm_desc per group (no bias / gate / C2 / stats; C is not written and may be None); levels: the bn_apply_multi dicts of
    the same groups (`raw` unused, no `up`).  -> True when launched; False when the library cannot serve this launch
    (DRN_ERR_UNSUPPORTED): the caller runs gemm_nt + bn_apply_multi."""
    rc = _conv_bn_eval_call(descs, levels, dtype, relu, False)
    if rc == DRN_ERR_UNSUPPORTED:
        return False
    check(rc, "drn_conv_bn_eval")
    return True


def conv_bn_eval_plan(descs, levels, dtype):
    """The kernel conv_bn_eval would run these problems on (NT_KIND_*), or None where it would return False."""
    rc = _conv_bn_eval_call(descs, levels, dtype, False, True)
    if rc == DRN_ERR_UNSUPPORTED:
        return None
    if rc < 0:
        check(rc, "drn_conv_bn_eval_plan")
    return rc


def conv_bn_train_timeouts(reset=True):
    """Workgroups of fused conv->BN launches that gave up waiting for their tile column (0 in a healthy run).  Synchronises."""
    return int(lib().drn_conv_bn_train_timeouts(int(reset)))


BN_BWD_ONE = True      # (False = reduce + apply launches, drn_bn_bwd_multi)


def bn_bwd_multi(levels, C, dtype, relu=True):
    """levels: list of dicts(dout, ld_dout, raw, ld_raw, ss, save, gamma, draw, ld_draw, dgamma, dbeta, accumulate, M)."""
    def fill(with_gb):
        arr = (_lib.BnBwdDesc * len(levels))()
        for d, v in zip(arr, levels):
            d.dout, d.raw, d.scale_shift, d.save, d.gamma = _p(v["dout"]), _p(v["raw"]), _p(v["ss"]), _p(v["save"]), _p(v["gamma"])
            d.draw, d.dgamma, d.dbeta = _p(v["draw"]), _p(v["dgamma"]), _p(v["dbeta"])
            d.ld_dout, d.ld_raw, d.ld_draw, d.accumulate, d.M = v["ld_dout"], v["ld_raw"], v["ld_draw"], int(v["accumulate"]), v["M"]
            gb = v.get("gb") if with_gb else None
            if gb is not None:
                d.gb_dg, d.gb_gate, d.gb_dgate = _p(gb["dg"]), _p(gb["gate"]), _p(gb["dgate"])
                d.gb_ld_dg, d.gb_ldg, d.gb_L = gb["ld_dg"], gb["ldg"], gb["L"]
        return arr

    def ungate():
        # the query-gate backward as launches of its own (drn_gate_bwd) for the levels that asked for it inside the BatchNorm launch
        for v in levels:
            gb = v.get("gb")
            if gb is not None:
                C_ = C
                d_new = torch.empty_like(gb["dg"]) if v["dout"] is None else torch.empty_like(v["dout"])
                gate_bwd(gb["dg"], gb["ld_dg"], gb["act"], gb["ld_act"], gb["gate"], d_new, C_, v["dout"], v["ld_dout"], gb["dgate"],
                         v["M"] // gb["L"], gb["L"], C_, dtype)
                v["dout"], v["ld_dout"] = d_new, C_
                v["gb"] = None

    has_gb = any(v.get("gb") is not None for v in levels)
    arr = fill(has_gb)
    if BN_BWD_ONE:
        # one launch when the grid fits the chip at once (drn_bn_bwd_one): the tagged-pair workspace is zero at birth and keeps the
        # launch generation afterwards -- one buffer per size AND stream (launches on one stream are ordered; two streams running
        # same-sized passes at once must not share tags and the generation word)
        nbytes = int(lib().drn_bn_bwd_one_ws_bytes(arr, len(levels), C, dtype))
        if nbytes == 0 and has_gb:            # not with the gate backward inside: that one as its own launch, then ask again
            ungate()
            has_gb = False
            arr = fill(False)
            nbytes = int(lib().drn_bn_bwd_one_ws_bytes(arr, len(levels), C, dtype))
        if nbytes > 0:
            tws = persistent_buffer(("bn_bwd_one", torch.cuda.current_stream().cuda_stream), nbytes // 8, levels[0]["draw"].device,
                                    torch.int64)
            rc = lib().drn_bn_bwd_one(arr, len(levels), C, int(relu), _p(tws), ctypes.c_int64(nbytes), dtype, _stream())
            if rc != DRN_ERR_UNSUPPORTED:
                check(rc, "drn_bn_bwd_one")
                return
    if has_gb:
        ungate()
        arr = fill(False)
    ws = workspace(len(levels) * 515 * C, levels[0]["draw"].device)
    check(lib().drn_bn_bwd_multi(arr, len(levels), C, int(relu), _p(ws), dtype, _stream()), "drn_bn_bwd_multi")


def check_watchdogs():
    """Raise if any in-launch exchange gave up waiting since the last call (one-launch BatchNorm backward, fused conv -> BN, the
    one-launch BiLSTM forward): such a launch lets its outputs through INVALID and only bumps a device counter -- which somebody has to
    read.  Synchronises; drn_amd.trainer calls it at the end of every epoch and evaluation, bench.py after every timed region."""
    bad = {}
    for name, fn in (("drn_bn_bwd_one", "drn_bn_bwd_one_timeouts"), ("drn_conv_bn_train", "drn_conv_bn_train_timeouts"),
                     ("drn_lstm_seq_fwd", "drn_lstm_seq_fwd_timeouts")):
        n = int(getattr(lib(), fn)(1))
        if n:
            bad[name] = n
    if bad:
        raise _lib.DrnError("in-launch exchange watchdog fired (workgroups that gave up waiting; the step's results are invalid): %s" % bad)


def bn_bwd_one_timeouts(reset=True):
    """Workgroups of one-launch BatchNorm backward passes that gave up waiting for their channel tile (0 in a healthy run).  Synchronises."""
    return int(lib().drn_bn_bwd_one_timeouts(int(reset)))


def bn_eval_scale_shift(C, gamma, beta, conv_bias, running_mean, running_var, eps, ss):
    check(lib().drn_bn_eval_scale_shift(C, _p(gamma), _p(beta), _p(conv_bias), _p(running_mean), _p(running_var),
                                        ctypes.c_float(eps), _p(ss), _stream()), "drn_bn_eval_scale_shift")


def bn_apply(raw, ld_raw, ss, out, ld_out, M, C, L, dtype, up=None, ld_up=0, gate=None, gated=None, ld_gated=0, relu=True):
    check(lib().drn_bn_apply(_p(raw), ld_raw, _p(ss), _p(out), ld_out, M, C, L, _p(up), ld_up, _p(gate),
                             gate.stride(0) if gate is not None else 0, _p(gated), ld_gated, int(relu), dtype, _stream()),
          "drn_bn_apply")


def bn_bwd(dout, ld_dout, raw, ld_raw, ss, save, gamma, draw, ld_draw, dgamma, dbeta, accumulate, M, C, dtype, relu=True):
    ws = workspace(515 * C, draw.device)
    check(lib().drn_bn_bwd(_p(dout), ld_dout, _p(raw), ld_raw, _p(ss), _p(save), _p(gamma), _p(draw), ld_draw, _p(dgamma),
                           _p(dbeta), int(accumulate), M, C, int(relu), _p(ws), dtype, _stream()), "drn_bn_bwd")


# ---------------------------------------------------------------------------------------------
# 1-2 channel heads and losses
# ---------------------------------------------------------------------------------------------
def head_groups(xs, dxs=None, scales=None):
    """xs: list of (tensor2d_or_slice, ldx, M, L)."""
    gs = []
    for i, (x, ldx, M, L) in enumerate(xs):
        gs.append(_lib.HeadGroup(X=_p(x), dX=_p(dxs[i]) if dxs is not None else None, ldx=ldx, M=M, L=L,
                                 scale=ctypes.c_void_p(scales.data_ptr() + 4 * i) if scales is not None else None))
    return (_lib.HeadGroup * len(gs))(*gs)


def _head_calls(calls):
    """calls: list of dicts(groups (HeadGroup array), W, N, C, taps, exp_mode, + bias/out/z (forward) or dout/out/z/dW/dbias/
    dscale/ws (backward), optionally accumulate_dx / accumulate_dw (default 0: overwrite)).  Up to 2 heads share one launch
    (drn_amd/csrc/heads.hip)."""
    arr = (_lib.HeadCall * len(calls))()
    for d, c in zip(arr, calls):
        d.groups = ctypes.cast(c["groups"], ctypes.c_void_p)
        d.ngroups, d.N, d.C, d.taps, d.exp_mode = len(c["groups"]), c["N"], c["C"], c["taps"], int(c["exp_mode"])
        d.accumulate_dx, d.accumulate_dw = int(c.get("accumulate_dx", 0)), int(c.get("accumulate_dw", 0))
        d.dscale_stride = c["dscale"].stride(0) if c.get("dscale") is not None and c["dscale"].numel() > 1 else 1
        d.W, d.bias, d.out, d.z = _p(c["W"]), _p(c.get("bias")), _p(c.get("out")), _p(c.get("z"))
        d.dout, d.dW, d.dbias, d.dscale, d.ws = _p(c.get("dout")), _p(c.get("dW")), _p(c.get("dbias")), _p(c.get("dscale")), _p(c.get("ws"))
    arr._groups = [c["groups"] for c in calls]        # the nested host arrays live as long as the descriptor array that points to them
    return arr


def heads_fwd(calls, dtype):
    for c0 in range(0, len(calls), 2):
        chunk = calls[c0:c0 + 2]
        check(lib().drn_heads_fwd(_head_calls(chunk), len(chunk), dtype, _stream()), "drn_heads_fwd")


def heads_bwd(calls, dtype):
    """Each call gets its own slice of the per-device workspace (drn_heads_ws_elems floats)."""
    for c0 in range(0, len(calls), 2):
        chunk = calls[c0:c0 + 2]
        sizes = [int(lib().drn_heads_ws_elems(sum(int(g.M) for g in c["groups"]), c["N"], c["C"], c["taps"])) for c in chunk]
        ws = workspace(sum(sizes), chunk[0]["dW"].device)
        off = 0
        for c, n in zip(chunk, sizes):
            c["ws"] = ws[off:off + n]
            off += n
        check(lib().drn_heads_bwd(_head_calls(chunk), len(chunk), dtype, _stream()), "drn_heads_bwd")


def head_out_fwd(groups, W, bias, N, C, taps, exp_mode, out, z, dtype):
    heads_fwd([dict(groups=groups, W=W, bias=bias, N=N, C=C, taps=taps, exp_mode=exp_mode, out=out, z=z)], dtype)


def head_out_bwd(groups, W, dout, out, z, N, C, taps, exp_mode, accumulate_dx, dW, dbias, dscale, R, dtype):
    heads_bwd([dict(groups=groups, W=W, dout=dout, out=out, z=z, N=N, C=C, taps=taps, exp_mode=exp_mode,
                    accumulate_dx=accumulate_dx, dW=dW, dbias=dbias, dscale=dscale)], dtype)


def loss_levels(levels):
    """levels: list of (L, stride, lo, hi)."""
    return (_lib.LossLevel * len(levels))(*[_lib.LossLevel(L=L, stride=s, lo=lo, hi=hi) for (L, s, lo, hi) in levels])


def fcos_loss_fwd(levels, B, logits, reg, iou, gt, gamma, alpha, target_scale, iou_stage, out6, labels=None, bumps=None):
    """out6 (6 floats) = loss_cls, loss_reg, loss_iou, n_pos, n_iou_pos, sum of the three losses.  gt (B, 2) fp32 or fp64.
    bumps: [(int64 device counter, increment)] applied by the same launch (BatchNorm num_batches_tracked)."""
    assert out6.numel() >= 6 and gt.dtype in (torch.float32, torch.float64) and gt.is_contiguous()
    ws = workspace(5 * ((logits.shape[0] + 255) // 256), logits.device)
    nb = len(bumps) if bumps else 0
    arr = (_lib.CounterBump * nb)(*[_lib.CounterBump(counter=_p(t), inc=int(n)) for t, n in bumps]) if nb else None
    check(lib().drn_fcos_loss_fwd(levels, len(levels), B, _p(logits), _p(reg), _p(iou), _p(gt), int(gt.dtype == torch.float64),
                                  ctypes.c_float(gamma), ctypes.c_float(alpha), ctypes.c_float(target_scale), int(iou_stage), _p(out6),
                                  _p(labels), _p(ws), _p(_counters(logits.device)[-1:]), arr, nb, _stream()), "drn_fcos_loss_fwd")


def fcos_loss_bwd(levels, B, logits, reg, iou, gt, gamma, alpha, target_scale, iou_stage, out6, g3, dlogits, dreg, diou):
    """g3: upstream gradients (1-element fp32 tensors or None) of loss_cls, loss_reg, loss_iou."""
    check(lib().drn_fcos_loss_bwd(levels, len(levels), B, _p(logits), _p(reg), _p(iou), _p(gt), int(gt.dtype == torch.float64),
                                  ctypes.c_float(gamma), ctypes.c_float(alpha), ctypes.c_float(target_scale), int(iou_stage), _p(out6),
                                  _p(g3[0]), _p(g3[1]), _p(g3[2]), _p(dlogits), _p(dreg), _p(diou), _stream()), "drn_fcos_loss_bwd")


def focal_fwd(logits, targets, gamma, alpha):
    """Per-element sigmoid focal losses (N, C); the reference's fcos_core._C.sigmoid_focalloss_forward."""
    _need_gpu(logits, targets)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    assert targets.dtype == torch.int32 and targets.is_contiguous() and targets.numel() == logits.shape[0]
    out = torch.empty_like(logits)
    check(lib().drn_focal_fwd(_p(logits), _p(targets), ctypes.c_int64(logits.shape[0]), logits.shape[1], ctypes.c_float(gamma),
                              ctypes.c_float(alpha), _p(out), _stream()), "drn_focal_fwd")
    return out


def focal_bwd(logits, targets, d_losses, gamma, alpha):
    """d_logits (N, C) = d_losses * d loss / d logit; the reference's fcos_core._C.sigmoid_focalloss_backward."""
    _need_gpu(logits, targets, d_losses)
    assert d_losses.dtype == torch.float32 and d_losses.is_contiguous() and d_losses.shape == logits.shape
    out = torch.empty_like(logits)
    check(lib().drn_focal_bwd(_p(logits), _p(targets), _p(d_losses), ctypes.c_int64(logits.shape[0]), logits.shape[1],
                              ctypes.c_float(gamma), ctypes.c_float(alpha), _p(out), _stream()), "drn_focal_bwd")
    return out


def iou_loss_fwd(pred, target, weight=None):
    """out2 = (loss, signed divisor) of the stand-alone IOULoss (drn_iou_loss_fwd; model/layers/iou_loss.py:6-24)."""
    _need_gpu(pred, target, weight)
    assert pred.dtype == torch.float32 and pred.is_contiguous() and pred.dim() == 2 and pred.shape[1] == 2 and target.shape == pred.shape
    assert weight is None or (weight.dtype == torch.float32 and weight.is_contiguous() and weight.numel() == pred.shape[0])
    out2 = torch.empty(2, dtype=torch.float32, device=pred.device)
    check(lib().drn_iou_loss_fwd(_p(pred), _p(target), _p(weight), ctypes.c_int64(pred.shape[0]), _p(out2), _stream()), "drn_iou_loss_fwd")
    return out2


def iou_loss_bwd(pred, target, weight, out2, gout, want_pred=True, want_target=False):
    dpred = torch.empty_like(pred) if want_pred else None
    dtarget = torch.empty_like(target) if want_target else None
    check(lib().drn_iou_loss_bwd(_p(pred), _p(target), _p(weight), ctypes.c_int64(pred.shape[0]), _p(out2), _p(gout), _p(dpred),
                                 _p(dtarget), _stream()), "drn_iou_loss_bwd")
    return dpred, dtarget


# ---------------------------------------------------------------------------------------------
# query-encoder LSTM recurrence
# ---------------------------------------------------------------------------------------------
def lstm_step_fwd(xproj, whf, whr, biases, hseq, cseq, gates, out, hprev_t, lens, B, L, H, s, qvec=None, hseq16=None):
    """biases = (b_ih_f, b_hh_f, b_ih_r, b_hh_r); lens int64 on the device; layouts in include/drn_hip.h.  qvec (B, 4H) or None:
    the [first ; last] sentence vector, written by the steps that produce its rows.  whf / whr: W_hh (4H, H) fp32, or bf16 copies."""
    _need_gpu(xproj, out)
    assert whf.dtype == whr.dtype and whf.is_contiguous() and whr.is_contiguous()
    check(lib().drn_lstm_step_fwd(_p(xproj), _p(whf), _p(whr), BF16 if whf.dtype == torch.bfloat16 else F32, _p(biases[0]), _p(biases[1]), _p(biases[2]), _p(biases[3]),
                                  _p(hseq), _p(cseq), _p(gates), _p(out), _p(hprev_t), _p(qvec), _p(hseq16), _p(lens), B, L, H, s, _stream()),
          "drn_lstm_step_fwd")


# True = the fp16-state BiLSTM forward as ONE launch (drn_lstm_seq_fwd: hidden states handed over between resident workgroups as
# fp16 words whose spare exponent bit carries the launch parity, one wave polling one word per producer; bit-identical).  Third
# measurement of the idea, third null: 54.1 us for 8 steps against 8 x 7.3 = 58.4, the step 1.981 vs 1.982 ms -- a hand-off through
# memory costs ~5 us whatever replaces the kernel boundary (every thread polling its own words: 62.5 us).  Kept, tested, off.
LSTM_SEQ = False


def lstm_seq_fwd(xproj, whf, whr, biases, hseq, cseq, gates, out, hprev_t, lens, B, L, H, qvec=None):
    """The fp16-state forward recurrence as ONE launch (drn_lstm_seq_fwd; the bits of L lstm_step_fwd launches with hseq16).  Returns
    False -- nothing launched -- when the grid does not fit the chip at once."""
    _need_gpu(xproj, out)
    assert whf.dtype == torch.float32 and whf.is_contiguous() and whr.is_contiguous()
    nbytes = int(lib().drn_lstm_seq_fwd_ws_bytes(B, L, H))
    ws = persistent_buffer(("lstm_seq", B, L, H), nbytes // 8, xproj.device, torch.int64)
    rc = lib().drn_lstm_seq_fwd(_p(xproj), _p(whf), _p(whr), _p(biases[0]), _p(biases[1]), _p(biases[2]), _p(biases[3]), _p(hseq), _p(cseq),
                                _p(gates), _p(out), _p(hprev_t), _p(qvec), _p(ws), ctypes.c_int64(nbytes), _p(lens), B, L, H, _stream())
    if rc == DRN_ERR_UNSUPPORTED:
        return False
    check(rc, "drn_lstm_seq_fwd")
    return True


def lstm_seq_fwd_timeouts(reset=True):
    return int(lib().drn_lstm_seq_fwd_timeouts(int(reset)))


def lstm_bwd_first(dout, gates, cseq, dgates, dc, dh_pass, lens, B, L, H, dqvec=None, dgates16=None):
    check(lib().drn_lstm_bwd_first(_p(dout), _p(gates), _p(cseq), _p(dgates), _p(dc), _p(dh_pass), _p(dqvec), _p(dgates16), _p(lens), B, L, H,
                                   _stream()), "drn_lstm_bwd_first")


def lstm_step_bwd(dout, gates, cseq, wtf, wtr, dgates, dc, dh_pass, lens, B, L, H, s, dqvec=None, dgates16=None):
    assert wtf.dtype == wtr.dtype and wtf.is_contiguous() and wtr.is_contiguous()
    check(lib().drn_lstm_step_bwd(_p(dout), _p(gates), _p(cseq), _p(wtf), _p(wtr), BF16 if wtf.dtype == torch.bfloat16 else F32, _p(dgates), _p(dc), _p(dh_pass), _p(dqvec),
                                  _p(dgates16), _p(lens), B, L, H, s, _stream()), "drn_lstm_step_bwd")


def postprocess(levels, B, logits, reg, iou, thr, top_n, downsample):
    """Eval post-processor on the loss-layout head outputs.  Returns (det (B,R,2), scores (B,R), locs (B,R), counts (B,nl))."""
    _need_gpu(logits, reg)
    R = sum(int(l.L) for l in levels)
    dev = logits.device
    det = torch.empty((B, R, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((B, R), dtype=torch.float32, device=dev)
    locs = torch.empty((B, R), dtype=torch.float32, device=dev)
    counts = torch.empty((B, len(levels)), dtype=torch.int32, device=dev)
    check(lib().drn_postprocess(levels, len(levels), B, _p(logits), _p(reg), _p(iou), ctypes.c_float(thr), int(top_n),
                                ctypes.c_float(downsample), _p(det), _p(scores), _p(locs), _p(counts), _stream()), "drn_postprocess")
    return det, scores, locs, counts


def eval_recall(det, scores, counts, gt, ious, max_topk):
    """first_hit (B, len(ious)) int32 on the device: 0-based position, among the temporal-NMS survivors of clip b at IoU threshold
    ious[q], of the first one that overlaps gt[b] by >= ious[q]; max_topk when none of the first max_topk does
    (drn_eval_recall; utils/evaluate_utils.py:131-215).  ious: a device tensor of doubles."""
    _need_gpu(det, scores, counts, gt, ious)
    B, R = scores.shape
    assert gt.dtype in (torch.float32, torch.float64) and gt.is_contiguous() and ious.dtype == torch.float64
    out = torch.empty((B, ious.numel()), dtype=torch.int32, device=det.device)
    check(lib().drn_eval_recall(_p(det), _p(scores), _p(counts), B, counts.shape[1], R, _p(gt), int(gt.dtype == torch.float64), _p(ious),
                                ious.numel(), int(max_topk), _p(out), _stream()), "drn_eval_recall")
    return out


def select_moments(det, scores, counts, overlap, k):
    """The first k temporal-NMS survivors of every clip, best first, from drn_postprocess's buffers (drn_select_moments;
    utils/evaluate_utils.py:91-107,186-212).  -> seg (B, k, 2), score (B, k), level (B, k) int32, index (B, k) int32, n (B,) int32 on
    the device; no host synchronisation."""
    _need_gpu(det, scores, counts)
    B, R = scores.shape
    assert det.dtype == torch.float32 and scores.dtype == torch.float32 and counts.dtype == torch.int32
    assert det.is_contiguous() and scores.is_contiguous() and counts.is_contiguous() and det.shape == (B, R, 2)
    dev, k = det.device, int(k)
    seg = torch.empty((B, max(k, 0), 2), dtype=torch.float32, device=dev)
    score = torch.empty((B, max(k, 0)), dtype=torch.float32, device=dev)
    level = torch.empty((B, max(k, 0)), dtype=torch.int32, device=dev)
    index = torch.empty((B, max(k, 0)), dtype=torch.int32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().drn_select_moments(_p(det), _p(scores), _p(counts), B, counts.shape[1], R, float(overlap), k, _p(seg), _p(score),
                                   _p(level), _p(index), _p(n), _stream()), "drn_select_moments")
    return seg, score, level, index, n


def merge_state(S, k, device):
    """The running best-k state of S sentences for merge_moments: (seg (S, k, 2), score (S, k), video (S, k) int32, level (S, k) int32,
    rank (S, k) int32, n (S,) int32), uninitialised -- the first merge (first=True) never reads it."""
    S, k = int(S), max(int(k), 0)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)
    return (torch.empty((S, k, 2), dtype=torch.float32, device=device), torch.empty((S, k), dtype=torch.float32, device=device),
            i32(S, k), i32(S, k), i32(S, k), i32(S))


def merge_moments(moments, vids, num_videos, state, first):
    """One chunk of a search across videos (drn_merge_moments): `moments` = select_moments' (seg, score, level, index, n) for
    P = S * Vc (sentence, chunk slot) pairs, pair p = (p // Vc, p % Vc); vids (Vc,) int32 on the device = the slots' store positions
    (outside [0, num_videos): a padded slot, skipped); state = merge_state(S, k, ...), updated IN PLACE to each sentence's best k of
    (its state entries + the chunk's entries that are no fallback moment and have a finite score), ordered by score descending, video
    position ascending, rank ascending.  first: True / False, or a (1,) int32 DEVICE tensor read by the launch (non-zero: the state
    coming in is ignored) -- what a captured graph needs to serve every chunk.  No host synchronisation."""
    seg, score, level, index, n = moments
    st_seg, st_score, st_video, st_level, st_rank, st_n = state
    _need_gpu(seg, score, level, index, n, vids, *state)
    P, kv = (int(x) for x in score.shape)
    S, k = (int(x) for x in st_score.shape)
    Vc = int(vids.numel())
    flag = first if torch.is_tensor(first) else None
    if flag is not None:
        _need_gpu(flag)
    for name, t, dt, shape in (("seg", seg, torch.float32, (P, kv, 2)), ("score", score, torch.float32, (P, kv)),
                               ("level", level, torch.int32, (P, kv)), ("index", index, torch.int32, (P, kv)), ("n", n, torch.int32, (P,)),
                               ("vids", vids, torch.int32, (Vc,)), ("state seg", st_seg, torch.float32, (S, k, 2)),
                               ("state score", st_score, torch.float32, (S, k)), ("state video", st_video, torch.int32, (S, k)),
                               ("state level", st_level, torch.int32, (S, k)), ("state rank", st_rank, torch.int32, (S, k)),
                               ("state n", st_n, torch.int32, (S,)), ("first", flag, torch.int32, (1,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.DrnError("merge_moments: %s must be a contiguous %s %s tensor" % (name, shape, dt))
    if S * Vc != P:
        raise _lib.DrnError("merge_moments: %d pairs are not %d sentences x %d chunk slots" % (P, S, Vc))
    check(lib().drn_merge_moments(_p(seg), _p(score), _p(level), _p(index), _p(n), S, Vc, kv, _p(vids), int(num_videos), k,
                                  0 if flag is not None else int(bool(first)), _p(flag), _p(st_seg), _p(st_score), _p(st_video),
                                  _p(st_level), _p(st_rank), _p(st_n), _stream()), "drn_merge_moments")
    return state


def merge_moments_ragged(moments, pair_video, pair_off, num_videos, state, first):
    """merge_moments for one chunk of P pairs in any assignment to sentences (drn_merge_moments_ragged): pair_video (P,) int32 on the
    device = the store position of pair p's video (outside [0, num_videos): a padded pair, skipped), pair_off (S + 1,) int32 on the
    device = sentence s owns the pairs [pair_off[s], pair_off[s + 1]) of the chunk; pairs outside every range take no part.  state,
    first, the candidates and the order are merge_moments'.  A sentence without a pair keeps its state (first false) or is left
    empty (first true).  No host synchronisation: pair_off is not read back, the launch clamps what it reads from it."""
    seg, score, level, index, n = moments
    st_seg, st_score, st_video, st_level, st_rank, st_n = state
    _need_gpu(seg, score, level, index, n, pair_video, pair_off, *state)
    P, kv = (int(x) for x in score.shape)
    S, k = (int(x) for x in st_score.shape)
    flag = first if torch.is_tensor(first) else None
    if flag is not None:
        _need_gpu(flag)
    for name, t, dt, shape in (("seg", seg, torch.float32, (P, kv, 2)), ("score", score, torch.float32, (P, kv)),
                               ("level", level, torch.int32, (P, kv)), ("index", index, torch.int32, (P, kv)), ("n", n, torch.int32, (P,)),
                               ("pair_video", pair_video, torch.int32, (P,)), ("pair_off", pair_off, torch.int32, (S + 1,)),
                               ("state seg", st_seg, torch.float32, (S, k, 2)), ("state score", st_score, torch.float32, (S, k)),
                               ("state video", st_video, torch.int32, (S, k)), ("state level", st_level, torch.int32, (S, k)),
                               ("state rank", st_rank, torch.int32, (S, k)), ("state n", st_n, torch.int32, (S,)),
                               ("first", flag, torch.int32, (1,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise _lib.DrnError("merge_moments_ragged: %s must be a contiguous %s %s tensor" % (name, shape, dt))
    check(lib().drn_merge_moments_ragged(_p(seg), _p(score), _p(level), _p(index), _p(n), S, P, kv, _p(pair_video), _p(pair_off),
                                         int(num_videos), k, 0 if flag is not None else int(bool(first)), _p(flag), _p(st_seg),
                                         _p(st_score), _p(st_video), _p(st_level), _p(st_rank), _p(st_n), _stream()),
          "drn_merge_moments_ragged")
    return state


def search_recall(hits, gt_video, gt, ious):
    """Score a search against ground truth on the device (drn_search_recall): hits = Grounder.search's Hits (or anything with its seg
    (S, K, 2) float32, video (S, K) int32 and n (S,) int32), gt_video (S,) int32 store positions, gt (S, 2) float32 / float64 start and
    end as fractions of the video, ious (I,) float64 -- all on the device -> first_hit (S, I + 1) int32 on the device: column i < I
    the position of the first hit in the right video with tIoU >= ious[i], column I the number of distinct videos ranked before the
    right one, K where there is none (metrics.search_first_hits is the host twin; metrics.recall_from_first_hits turns either kind
    of column into recalls).  No host synchronisation."""
    seg, video, n = hits.seg, hits.video, hits.n
    _need_gpu(seg, video, n, gt_video, gt, ious)
    if video.dim() != 2:
        raise _lib.DrnError("search_recall: video must be a (S, K) tensor, not %s" % (tuple(video.shape),))
    S, K = (int(x) for x in video.shape)
    I = int(ious.numel())
    if gt.dtype not in (torch.float32, torch.float64):
        raise _lib.DrnError("search_recall: gt must be float32 or float64, not %s" % gt.dtype)
    for name, t, dt, shape in (("seg", seg, torch.float32, (S, K, 2)), ("video", video, torch.int32, (S, K)), ("n", n, torch.int32, (S,)),
                               ("gt_video", gt_video, torch.int32, (S,)), ("gt", gt, gt.dtype, (S, 2)), ("ious", ious, torch.float64, (I,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DrnError("search_recall: %s must be a contiguous %s %s tensor" % (name, shape, dt))
    out = torch.empty((S, I + 1), dtype=torch.int32, device=video.device)
    check(lib().drn_search_recall(_p(seg), _p(video), _p(n), _p(gt_video), _p(gt), int(gt.dtype == torch.float64), _p(ious), S, K, I,
                                  _p(out), _stream()), "drn_search_recall")
    return out


def shortlist_ws_keys(V, S, n):
    """The 8-byte keys of workspace drn_shortlist_topn needs: S * ceil(V / SHORTLIST_BLOCK) * min(n, SHORTLIST_BLOCK)."""
    return int(S) * (-(-int(V) // _lib.SHORTLIST_BLOCK)) * min(int(n), _lib.SHORTLIST_BLOCK)


def shortlist_segments_ws_keys(nblocks, S, n):
    """The 8-byte keys of workspace drn_shortlist_segments_topn needs: K + ceil(K / 2), K = S * nblocks * min(n, SHORTLIST_SEG_BLOCK)."""
    K = int(S) * int(nblocks) * min(int(n), _lib.SHORTLIST_SEG_BLOCK)
    return K + (K + 1) // 2


def _q8_table(what, codes, scales, queries):
    """The checks a block-scaled FP8 table shares between the two quantised shortlists -> (rows, E)."""
    cs, qs = tuple(codes.shape), queries.shape
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or len(cs) != 2 or not codes.is_contiguous() or not scales.is_contiguous() \
            or cs[1] % 32 or tuple(scales.shape) != (cs[0], cs[1] // 32):
        raise _lib.DrnError("%s: codes (rows, E) and scales (rows, E / 32) must be contiguous uint8 tensors with E a multiple of 32" % what)
    if len(qs) != 2 or not queries.is_contiguous() or queries.dtype not in (torch.float32, torch.bfloat16) or qs[1] != cs[1]:
        raise _lib.DrnError("%s: queries must be a contiguous (S, %d) float32 / bfloat16 tensor" % (what, cs[1]))
    return cs


def allow_words(V):
    """The int32 words of one row of a packed allow mask over V videos: ceil(V / 32)."""
    return -(-int(V) // 32)


def pack_allow(mask, words):
    """mask (V,) or (S, V) bool on the device -> words (W,) or (S, W) int32, W = allow_words(V), written in place, every word: bit
    v & 31 of word v >> 5 = mask[..., v], zero bits past V (drn_pack_allow; drn_amd.retrieve.pack_allow_reference is the definition).
    One launch (tag pack_allow); the mask is not read on the host."""
    _need_gpu(mask, words)
    if mask.dtype != torch.bool or mask.dim() not in (1, 2) or mask.shape[-1] < 1 or mask.shape[0] < 1 or not mask.is_contiguous():
        raise _lib.DrnError("pack_allow: the mask must be a contiguous bool tensor (V,) or (S, V) with V >= 1 and S >= 1, not %s %s"
                            % (mask.dtype, tuple(mask.shape)))
    V = int(mask.shape[-1])
    shape = tuple(mask.shape[:-1]) + (allow_words(V),)
    if words.dtype != torch.int32 or tuple(words.shape) != shape or not words.is_contiguous():
        raise _lib.DrnError("pack_allow: words must be a contiguous %s torch.int32 tensor" % (shape,))
    S = 1 if mask.dim() == 1 else int(mask.shape[0])
    _timed("pack_allow", 0.0, lambda: check(lib().drn_pack_allow(_p(mask), S, V, _p(words), _stream()), "drn_pack_allow"))
    return words


def _allow_stride(what, allow, V, S):
    """The checks of a packed mask for V videos and S sentences -> allow_stride: 0 for a shared mask (W,), W for one (S, W)."""
    W = allow_words(V)
    if allow.dtype != torch.int32 or not allow.is_contiguous() or tuple(allow.shape) not in ((W,), (S, W)):
        raise _lib.DrnError("%s: allow must be a contiguous torch.int32 tensor (%d,) or (%d, %d) -- ceil(V / 32) packed words a row "
                            "(drn_amd.retrieve.pack_allow makes them) -- not %s %s" % (what, W, S, W, allow.dtype, tuple(allow.shape)))
    return 0 if allow.dim() == 1 else W


def _allow_args(what, allow, V, S):
    """An optional packed mask as the entries take it -> (mask pointer, allow_stride): (NULL, 0) without one, else _allow_stride's checks."""
    if allow is None:
        return None, 0
    stride = _allow_stride(what, allow, V, S)
    return _p(allow), stride


def _shortlist_buffers(what, S, n, need, ws, ids, scores, counts, rows=None, cap=_lib.SHORTLIST_MAX):
    """The checks the shortlist wrappers share: n (at most cap), the output buffers and the workspace."""
    if not 1 <= n <= cap:
        raise _lib.DrnError("%s: n = %d outside [1, %d]" % (what, n, cap))
    outs = (("ids", ids, torch.int32, (S, n)), ("scores", scores, torch.float32, (S, n)), ("counts", counts, torch.int32, (S,)))
    if rows is not None:
        outs += (("rows", rows, torch.int32, (S, n)),)
    for name, t, dt, shape in outs:
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous %s %s tensor" % (what, name, shape, dt))
    if ws.dtype != torch.int64 or not ws.is_contiguous() or ws.numel() < need:
        raise _lib.DrnError("%s: ws must be a contiguous int64 tensor of at least %d elements" % (what, need))


def _segment_tables(what, offsets, blk_vid, vid_blk):
    """The checks of a ragged table's device tables -> (V, nblocks)."""
    if offsets.dim() != 1 or offsets.numel() < 2 or blk_vid.dim() != 1 or blk_vid.numel() < 2:
        raise _lib.DrnError("%s: offsets must be (V + 1,) and blk_vid (nblocks + 1,), V >= 1 and nblocks >= 1" % what)
    V, nblocks = int(offsets.numel()) - 1, int(blk_vid.numel()) - 1
    for name, t, shape in (("offsets", offsets, (V + 1,)), ("blk_vid", blk_vid, (nblocks + 1,)), ("vid_blk", vid_blk, (V,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous %s torch.int32 tensor" % (what, name, shape))
    return V, nblocks


def _plain_table(what, emb, queries):
    """The checks a plain table shares between the shortlist wrappers -> (rows, E)."""
    es, qs = emb.shape, queries.shape
    if len(es) != 2 or len(qs) != 2 or not emb.is_contiguous() or not queries.is_contiguous() or emb.dtype != queries.dtype or es[1] != qs[1]:
        raise _lib.DrnError("%s: emb (rows, E) and queries (S, E) must be contiguous and of one dtype and width" % what)
    return int(es[0]), int(es[1])


def _shortlist_entry(table, queries, seg, n, ws, outs, allow):
    """The eight entries behind shortlist_topn (seg = ()) and shortlist_segments_topn (seg = (offsets, blk_vid, vid_blk)).  ONE name --
    shortlist[_segments]_topn[_q8][_allow], _q8 for a (codes, scales) pair and _allow for a mask -- is the prefix of every refusal, the
    timer's tag and, behind drn_, the C symbol; the arguments follow include/drn_hip.h: table, queries, [the segment tables], [allow,
    allow_stride], [R], V, [nblocks], E, S, n, dtype, ws, its keys, the outputs, the stream."""
    q8 = isinstance(table, (tuple, list))
    what = "shortlist%s_topn%s%s" % ("_segments" if seg else "", "_q8" if q8 else "", "" if allow is None else "_allow")
    tensors = (tuple(table) if q8 else (table,)) + (queries,) + seg
    _need_gpu(*(tensors + (allow, ws) + outs))
    n = int(n)
    rows, E = _q8_table(what, table[0], table[1], queries) if q8 else _plain_table(what, table, queries)
    S = int(queries.shape[0])
    if seg:
        V, nblocks = _segment_tables(what, *seg)
        need, sizes = shortlist_segments_ws_keys(nblocks, S, n), (rows, V, nblocks)
    else:
        V = rows
        need, sizes = shortlist_ws_keys(V, S, n), (V,)
    _shortlist_buffers(what, S, n, need, ws, *outs)
    mask = () if allow is None else _allow_args(what, allow, V, S)
    args = tuple(_p(t) for t in tensors) + mask + sizes + (E, S, n, dtype_code(queries), _p(ws), int(min(ws.numel(), 0x7fffffff))) \
        + tuple(_p(t) for t in outs)
    _timed(what, 2.0 * S * rows * E, lambda: check(getattr(lib(), "drn_" + what)(*args, _stream()), "drn_" + what))
    return outs


def shortlist_topn(table, queries, n, ws, ids, scores, counts, allow=None):
    """Each sentence's best n rows of a table by dot product with its row of `queries` (S, E), into ids (S, n) int32, scores (S, n)
    float32 and counts (S,) int32, all written in place (drn_amd.retrieve.shortlist_reference is the definition: finite scores only, score
    descending then position ascending, -1 / 0 past the list).  table: emb (V, E), contiguous like the queries and of their dtype
    (float32 / bfloat16), or a pair (codes, scales) of a block-scaled FP8 table -- codes (V, E) and scales (V, E / 32) uint8 as
    quantize_rows_mx8 writes them, E % 32 == 0 -- beside float32 / bfloat16 queries, whose dtype chooses the MFMA chain: the result is
    then bit for bit that over drn_amd.index.mx8_dequantize(codes, scales, queries.dtype).  allow: None, or a packed mask (W,) -- one
    for every sentence -- or (S, W) int32 on the device, W = allow_words(V), bit v & 31 of word v >> 5 set = video v may be listed, bits
    past V ignored (shortlist_reference(..., allow=) is the definition): a listed score has the unmasked bits, the mask is not read on
    the host, and None reaches the unmasked entry, which takes no mask at all.  ws: an int64 tensor of at least
    shortlist_ws_keys(V, S, n) elements.  One C entry and one tag per kind of call (drn_shortlist_topn[_q8][_allow]; the tag is the
    name without drn_): two launches on the current stream, no host synchronisation."""
    return _shortlist_entry(table, queries, (), n, ws, (ids, scores, counts), allow)


def shortlist_segments_topn(table, queries, offsets, blk_vid, vid_blk, n, ws, ids, scores, counts, rows, allow=None):
    """Each sentence's best n videos of a RAGGED table by their best row: table (R, E) or (codes, scales), queries (S, E) and allow --
    over the V VIDEOS, not the rows -- as in shortlist_topn; offsets (V + 1,), blk_vid (nblocks + 1,) and vid_blk (V,) int32 on the device
    (the rows of each video and the block plan, drn_amd.retrieve.plan_segment_blocks) -> ids, scores (S, n), counts (S,) and rows (S, n)
    int32, all written in place (drn_amd.retrieve.segment_shortlist_reference is the definition, with allow= under a mask; a quantised
    table answers bit for bit like its mx8_dequantize).  ws: an int64 tensor of at least shortlist_segments_ws_keys(nblocks, S, n)
    elements.  One C entry and one tag per kind of call (drn_shortlist_segments_topn[_q8][_allow]): three launches on the current
    stream; the tables and the mask are not read on the host and nothing is synchronised."""
    return _shortlist_entry(table, queries, (offsets, blk_vid, vid_blk), n, ws, (ids, scores, counts, rows), allow)


def shortlist_deep(table, queries, seg, n, ws, outs, allow):
    """The DEEP shortlist, 1 <= n <= SHORTLIST_DEEP_MAX, behind ONE entry and one tag (drn_shortlist_deep / shortlist_deep) for all
    four tables: table is emb or a pair (codes, scales), seg is () or (offsets, blk_vid, vid_blk), outs is (ids, scores, counts) or
    (ids, scores, counts, rows) -- each as in shortlist_topn / shortlist_segments_topn, with their checks, their workspace sizes
    (shortlist_ws_keys / shortlist_segments_ws_keys) and their definitions.  allow is REQUIRED: a packed mask (W,) or (S, W) int32 on
    the device (a caller without a filter passes a row of all-ones words).  Two launches on a plain table, three on a ragged one, on
    the current stream; nothing is read on the host."""
    what = "shortlist_deep"
    if allow is None:
        raise _lib.DrnError("%s: allow is required: a packed mask (pass a row of all-ones words to list every video)" % what)
    q8 = isinstance(table, (tuple, list))
    seg, outs = tuple(seg), tuple(outs)
    if len(seg) not in (0, 3) or len(outs) != (4 if seg else 3):
        raise _lib.DrnError("%s: seg must be () or (offsets, blk_vid, vid_blk) and outs (ids, scores, counts) or, on a ragged table, "
                            "(ids, scores, counts, rows)" % what)
    tensors = (tuple(table) if q8 else (table,)) + (queries,) + seg
    _need_gpu(*(tensors + (allow, ws) + outs))
    n = int(n)
    rows, E = _q8_table(what, table[0], table[1], queries) if q8 else _plain_table(what, table, queries)
    S = int(queries.shape[0])
    if seg:
        V, nblocks = _segment_tables(what, *seg)
        need = shortlist_segments_ws_keys(nblocks, S, n)
    else:
        V, nblocks = rows, 0
        need = shortlist_ws_keys(V, S, n)
    _shortlist_buffers(what, S, n, need, ws, *outs, cap=_lib.SHORTLIST_DEEP_MAX)
    mask, stride = _allow_args(what, allow, V, S)
    args = (_p(table[0]), _p(table[1])) if q8 else (_p(table), None)
    args += (_p(queries),) + (tuple(_p(t) for t in seg) if seg else (None, None, None)) + (mask, stride, rows if seg else 0, V, nblocks, E, S, n,
                                                                                          dtype_code(queries), _p(ws), int(min(ws.numel(), 0x7fffffff)))
    args += tuple(_p(t) for t in outs) + (() if seg else (None,))
    _timed(what, 2.0 * S * rows * E, lambda: check(lib().drn_shortlist_deep(*args, _stream()), "drn_shortlist_deep"))
    return outs


def binary_words(E):
    """The int32 words of one row of sign codes over E columns: ceil(E / 32) (allow_words' arithmetic: the bit convention is the same)."""
    return -(-int(E) // 32)


def _shortlist_bin_entry(what, codes, E, queries, seg, n, ws, outs, allow):
    """shortlist_bin / shortlist_bin_asym: one argument list, one list of checks, the entry drn_<what> under the tag <what>."""
    if allow is None:
        raise _lib.DrnError("%s: allow is required: a packed mask (pass a row of all-ones words to list every video)" % what)
    seg, outs = tuple(seg), tuple(outs)
    if len(seg) not in (0, 3) or len(outs) != (4 if seg else 3):
        raise _lib.DrnError("%s: seg must be () or (offsets, blk_vid, vid_blk) and outs (ids, scores, counts) or, on a ragged table, "
                            "(ids, scores, counts, rows)" % what)
    _need_gpu(*((codes, queries) + seg + (allow, ws) + outs))
    E, n = int(E), int(n)
    if not 1 <= E <= _lib.BINARY_MAX_E:
        raise _lib.DrnError("%s: E = %d outside [1, %d]" % (what, E, _lib.BINARY_MAX_E))
    cs, qs = tuple(codes.shape), tuple(queries.shape)
    if codes.dtype != torch.int32 or len(cs) != 2 or cs[0] < 1 or cs[1] != binary_words(E) or not codes.is_contiguous():
        raise _lib.DrnError("%s: codes must be a contiguous (rows, %d) torch.int32 tensor, ceil(E / 32) words a row for E = %d, not %s %s"
                            % (what, binary_words(E), E, codes.dtype, cs))
    if len(qs) != 2 or qs[0] < 1 or qs[1] != E or not queries.is_contiguous() or queries.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.DrnError("%s: queries must be a contiguous (S, %d) float32 / bfloat16 tensor" % (what, E))
    rows, S = int(cs[0]), int(qs[0])
    if seg:
        V, nblocks = _segment_tables(what, *seg)
        need = shortlist_segments_ws_keys(nblocks, S, n)
    else:
        V, nblocks = rows, 0
        need = shortlist_ws_keys(V, S, n)
    _shortlist_buffers(what, S, n, need, ws, *outs, cap=_lib.SHORTLIST_DEEP_MAX)
    mask, stride = _allow_args(what, allow, V, S)
    args = (_p(codes), _p(queries)) + (tuple(_p(t) for t in seg) if seg else (None, None, None))
    args += (mask, stride, rows if seg else 0, V, nblocks, E, S, n, dtype_code(queries), _p(ws), int(min(ws.numel(), 0x7fffffff)))
    args += tuple(_p(t) for t in outs) + (() if seg else (None,))
    # (per (sentence, row): E bit products and E additions, as the dot product they stand for)
    _timed(what, 2.0 * S * rows * E, lambda: check(getattr(lib(), "drn_" + what)(*args, _stream()), "drn_" + what))
    return outs


def shortlist_bin(codes, E, queries, seg, n, ws, outs, allow):
    """The BINARY shortlist, 1 <= n <= SHORTLIST_DEEP_MAX, behind one entry and one tag (drn_shortlist_bin / shortlist_bin): codes
    (rows, W) int32 sign codes, W = binary_words(E), 1 <= E <= BINARY_MAX_E (drn_amd.binary.binary_quantize_reference is the format);
    queries (S, E) float32 / bfloat16, binarised by the launch; seg is () or (offsets, blk_vid, vid_blk), outs is (ids, scores, counts)
    or (ids, scores, counts, rows) -- as in shortlist_deep, with its checks and its workspace sizes (shortlist_ws_keys /
    shortlist_segments_ws_keys); drn_amd.binary.binary_shortlist_reference is the definition.  allow is REQUIRED: a packed mask (W,) or
    (S, W) int32 on the device (a caller without a filter passes a row of all-ones words).  Two launches on a plain table, three on a
    ragged one, on the current stream; nothing is read on the host."""
    return _shortlist_bin_entry("shortlist_bin", codes, E, queries, seg, n, ws, outs, allow)


def shortlist_bin_asym(codes, E, queries, seg, n, ws, outs, allow):
    """The ASYMMETRIC binary shortlist behind one entry and one tag (drn_shortlist_bin_asym / shortlist_bin_asym): the arguments, the
    checks and the workspace sizes of shortlist_bin, but the queries keep their magnitudes: score[s, r] = sum_e q[s, e] * (+-1 of bit e
    of codes[r]), every field bit for bit shortlist_deep over drn_amd.binary.binary_dequantize(codes, E, queries.dtype);
    drn_amd.binary.binary_asym_shortlist_reference is the definition.  Two launches on a plain table, three on a ragged one, on the
    current stream; nothing is read on the host."""
    return _shortlist_bin_entry("shortlist_bin_asym", codes, E, queries, seg, n, ws, outs, allow)


def shortlist_late_ws_keys(nblocks, S, n):
    """The 8-byte keys of workspace drn_shortlist_late_topn needs: S * nblocks * min(n, SHORTLIST_SEG_BLOCK)."""
    return int(S) * int(nblocks) * min(int(n), _lib.SHORTLIST_SEG_BLOCK)


def shortlist_late_topn(table, queries, lengths, offsets, blk_vid, n, ws, ids, scores, counts, allow=None):
    """The shortlist by late interaction over a ragged table: table is emb (R, E), float32 / bfloat16, or a pair (codes, scales) of a
    block-scaled FP8 table (codes (R, E) and scales (R, E / 32) uint8, E % 32 == 0); queries (S, L, E) of the table's dtype (float32 /
    bfloat16 beside codes), 1 <= L <= LATE_MAX_TOKENS; lengths (S,) int32 on the device, the live tokens of each sentence, clamped into
    [0, L] there; offsets (V + 1,) and blk_vid (nblocks + 1,) int32 on the device as in shortlist_segments_topn -> ids, scores (S, n)
    and counts (S,), written in place: each sentence's best n videos by the sum over its live tokens of the video's best row
    (drn_shortlist_late_topn / drn_shortlist_late_topn_q8; drn_amd.retrieve.late_shortlist_reference is the definition).  allow: None, or
    a packed mask as in shortlist_topn.  ws: an int64 tensor of at least shortlist_late_ws_keys(nblocks, S, n) elements.  Two
    launches on the current stream behind one entry (one tag, shortlist_late_topn); nothing is read on the host."""
    what = "shortlist_late_topn"
    q8 = isinstance(table, (tuple, list))
    _need_gpu(*((tuple(table) if q8 else (table,)) + (queries, lengths, offsets, blk_vid, ws, ids, scores, counts)
                + (() if allow is None else (allow,))))
    n = int(n)
    if queries.dim() != 3 or not queries.is_contiguous() or not 1 <= queries.shape[1] <= _lib.LATE_MAX_TOKENS:
        raise _lib.DrnError("%s: queries must be a contiguous (S, L, E) tensor with 1 <= L <= %d, not %s"
                            % (what, _lib.LATE_MAX_TOKENS, tuple(queries.shape)))
    S, L = int(queries.shape[0]), int(queries.shape[1])
    flat = queries.view(S * L, -1)
    R, E = _q8_table(what, table[0], table[1], flat) if q8 else _plain_table(what, table, flat)
    if S < 1:
        raise _lib.DrnError("%s: queries must hold a sentence at least, not %s" % (what, tuple(queries.shape)))
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,) or not lengths.is_contiguous():
        raise _lib.DrnError("%s: lengths must be a contiguous (%d,) torch.int32 tensor" % (what, S))
    V, nblocks = _rank_plan(what, offsets, blk_vid)
    _shortlist_buffers(what, S, n, shortlist_late_ws_keys(nblocks, S, n), ws, ids, scores, counts)
    mask, stride = _allow_args(what, allow, V, S)
    tail = (_p(queries), _p(lengths), _p(offsets), _p(blk_vid), mask, stride, R, V, nblocks, E, S, L, n, dtype_code(queries), _p(ws),
            int(min(ws.numel(), 0x7fffffff)), _p(ids), _p(scores), _p(counts), _stream())
    if q8:
        launch = lambda: check(lib().drn_shortlist_late_topn_q8(_p(table[0]), _p(table[1]), *tail), "drn_shortlist_late_topn_q8")
    else:
        launch = lambda: check(lib().drn_shortlist_late_topn(_p(table), *tail), "drn_shortlist_late_topn")
    _timed(what, 2.0 * S * L * R * E, launch)
    return ids, scores, counts


def shortlist_rank_ws_bytes(nblocks, S):
    """The bytes of workspace the three rank entries need: 8 * S * (1 + nblocks) -- each sentence's target key, then two int32 counts
    per (sentence, block); nblocks = ceil(V / SHORTLIST_BLOCK) on a plain table, the plan's on a ragged one."""
    return 8 * int(S) * (1 + int(nblocks))


def _rank_table(what, table, flat):
    """table: emb, or a pair (codes, scales), beside queries flattened to (rows of queries, E) -> (tensors, table pointer, scales pointer
    or None, rows, E)."""
    if isinstance(table, (tuple, list)):
        rows, E = _q8_table(what, table[0], table[1], flat)
        return tuple(table), _p(table[0]), _p(table[1]), rows, E
    rows, E = _plain_table(what, table, flat)
    if table.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.DrnError("%s: emb must be float32 / bfloat16, not %s" % (what, table.dtype))
    return (table,), _p(table), None, rows, E


def _rank_buffers(what, S, need, targets, ws, rank, score, total):
    """The checks the rank wrappers share: targets, the three outputs and the workspace."""
    for name, t, dt in (("targets", targets, torch.int32), ("rank", rank, torch.int32), ("score", score, torch.float32),
                        ("total", total, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous (%d,) %s tensor" % (what, name, S, dt))
    if ws.dtype != torch.int64 or not ws.is_contiguous() or ws.numel() * 8 < need:
        raise _lib.DrnError("%s: ws must be a contiguous int64 tensor of at least %d bytes (shortlist_rank_ws_bytes)" % (what, need))
    return int(min(ws.numel() * 8, 0x7fffffff))


def _rank_plan(what, offsets, blk_vid):
    """The checks of a ragged table's offsets and block starts -> (V, nblocks)."""
    if offsets.dim() != 1 or offsets.numel() < 2 or blk_vid.dim() != 1 or blk_vid.numel() < 2:
        raise _lib.DrnError("%s: offsets must be (V + 1,) and blk_vid (nblocks + 1,), V >= 1 and nblocks >= 1" % what)
    for name, t in (("offsets", offsets), ("blk_vid", blk_vid)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous torch.int32 tensor" % (what, name))
    return int(offsets.numel()) - 1, int(blk_vid.numel()) - 1


def shortlist_rank(table, queries, targets, ws, rank, score, total, allow=None):
    """The place of targets[s] in sentence s's FULL shortlist order over a plain table (drn_shortlist_rank;
    drn_amd.retrieve.rank_reference is the definition): table is emb (V, E), float32 / bfloat16, or a pair (codes, scales) of a
    block-scaled FP8 table; queries (S, E) of the table's dtype (float32 / bfloat16 beside codes); targets (S,) int32 ON THE DEVICE, a
    value outside [0, V) meaning "no target" -> rank (S,) int32 (-1: the target is no candidate), score (S,) float32 (the target's, with
    shortlist_topn's bits; 0 beside -1) and total (S,) int32 (the sentence's candidates), written in place.  allow: None, or a packed
    mask as in shortlist_topn.  ws: an int64 tensor of at least shortlist_rank_ws_bytes(ceil(V / SHORTLIST_BLOCK), S) bytes.
    Three launches on the current stream behind one entry (one tag, shortlist_rank); nothing is read on the host."""
    what = "shortlist_rank"
    if queries.dim() != 2:
        raise _lib.DrnError("%s: queries must be a contiguous (S, E) tensor, not %s" % (what, tuple(queries.shape)))
    tensors, tab, scl, V, E = _rank_table(what, table, queries)
    _need_gpu(*(tensors + (queries, targets, ws, rank, score, total) + (() if allow is None else (allow,))))
    S = int(queries.shape[0])
    have = _rank_buffers(what, S, shortlist_rank_ws_bytes(-(-V // _lib.SHORTLIST_BLOCK), S), targets, ws, rank, score, total)
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * S * V * E, lambda: check(lib().drn_shortlist_rank(
        tab, scl, _p(queries), _p(targets), mask, stride, V, E, S, dtype_code(queries), _p(ws), have, _p(rank), _p(score), _p(total),
        _stream()), "drn_shortlist_rank"))
    return rank, score, total


def shortlist_segments_rank(table, queries, offsets, blk_vid, targets, ws, rank, score, total, allow=None):
    """shortlist_rank over a RAGGED table, a video scoring by its best row (drn_shortlist_segments_rank;
    drn_amd.retrieve.segment_rank_reference is the definition): table (R, E) or (codes, scales); offsets (V + 1,) and blk_vid
    (nblocks + 1,) int32 on the device as in shortlist_segments_topn; a target that owns no row gets -1.  ws: at least
    shortlist_rank_ws_bytes(nblocks, S) bytes.  Every other argument as in shortlist_rank.  Three launches behind one entry (one tag,
    shortlist_segments_rank); nothing is read on the host."""
    what = "shortlist_segments_rank"
    if queries.dim() != 2:
        raise _lib.DrnError("%s: queries must be a contiguous (S, E) tensor, not %s" % (what, tuple(queries.shape)))
    tensors, tab, scl, R, E = _rank_table(what, table, queries)
    _need_gpu(*(tensors + (queries, offsets, blk_vid, targets, ws, rank, score, total) + (() if allow is None else (allow,))))
    S = int(queries.shape[0])
    V, nblocks = _rank_plan(what, offsets, blk_vid)
    have = _rank_buffers(what, S, shortlist_rank_ws_bytes(nblocks, S), targets, ws, rank, score, total)
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * S * R * E, lambda: check(lib().drn_shortlist_segments_rank(
        tab, scl, _p(queries), _p(offsets), _p(blk_vid), _p(targets), mask, stride, R, V, nblocks, E, S, dtype_code(queries), _p(ws), have,
        _p(rank), _p(score), _p(total), _stream()), "drn_shortlist_segments_rank"))
    return rank, score, total


def shortlist_late_rank(table, queries, lengths, offsets, blk_vid, targets, ws, rank, score, total, allow=None):
    """shortlist_rank by LATE INTERACTION over a ragged table (drn_shortlist_late_rank; drn_amd.retrieve.late_rank_reference is the
    definition): queries (S, L, E), 1 <= L <= LATE_MAX_TOKENS, and lengths (S,) int32 on the device as in shortlist_late_topn; a
    sentence without a live token has no candidate (rank -1, total 0).  Every other argument as in shortlist_segments_rank.  Three
    launches behind one entry (one tag, shortlist_late_rank); nothing is read on the host."""
    what = "shortlist_late_rank"
    if queries.dim() != 3 or not queries.is_contiguous() or not 1 <= queries.shape[1] <= _lib.LATE_MAX_TOKENS or queries.shape[0] < 1:
        raise _lib.DrnError("%s: queries must be a contiguous (S, L, E) tensor with S >= 1 and 1 <= L <= %d, not %s"
                            % (what, _lib.LATE_MAX_TOKENS, tuple(queries.shape)))
    S, L = int(queries.shape[0]), int(queries.shape[1])
    tensors, tab, scl, R, E = _rank_table(what, table, queries.view(S * L, -1))
    _need_gpu(*(tensors + (queries, lengths, offsets, blk_vid, targets, ws, rank, score, total) + (() if allow is None else (allow,))))
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,) or not lengths.is_contiguous():
        raise _lib.DrnError("%s: lengths must be a contiguous (%d,) torch.int32 tensor" % (what, S))
    V, nblocks = _rank_plan(what, offsets, blk_vid)
    have = _rank_buffers(what, S, shortlist_rank_ws_bytes(nblocks, S), targets, ws, rank, score, total)
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * S * L * R * E, lambda: check(lib().drn_shortlist_late_rank(
        tab, scl, _p(queries), _p(lengths), _p(offsets), _p(blk_vid), _p(targets), mask, stride, R, V, nblocks, E, S, L, dtype_code(queries),
        _p(ws), have, _p(rank), _p(score), _p(total), _stream()), "drn_shortlist_late_rank"))
    return rank, score, total


def _rank_phase(what, table, queries, lengths, plan, phase, targets, keys, cnt, allow):
    """What the three *_rank_phase wrappers share.  plan: () on a plain table, (offsets, blk_vid) on a ragged one; lengths: None unless
    late.  phase 1: targets (S,) int32 -> keys (S,) int64 (cnt must be None); phase 2: keys (S,) int64, read as thresholds -> cnt, a
    contiguous int64 tensor of at least S * blocks elements (targets must be None)."""
    phase = int(phase)
    if phase not in (1, 2):
        raise _lib.DrnError("%s: phase = %d is neither 1 (the target keys) nor 2 (the block counts)" % (what, phase))
    late = lengths is not None
    if late:
        if queries.dim() != 3 or not queries.is_contiguous() or not 1 <= queries.shape[1] <= _lib.LATE_MAX_TOKENS or queries.shape[0] < 1:
            raise _lib.DrnError("%s: queries must be a contiguous (S, L, E) tensor with S >= 1 and 1 <= L <= %d, not %s"
                                % (what, _lib.LATE_MAX_TOKENS, tuple(queries.shape)))
        S, L = int(queries.shape[0]), int(queries.shape[1])
    else:
        if queries.dim() != 2:
            raise _lib.DrnError("%s: queries must be a contiguous (S, E) tensor, not %s" % (what, tuple(queries.shape)))
        S, L = int(queries.shape[0]), 1
    tensors, tab, scl, R, E = _rank_table(what, table, queries.view(S * L, -1) if late else queries)
    _need_gpu(*(tensors + (queries, keys) + tuple(plan) + tuple(t for t in (lengths, targets, cnt, allow) if t is not None)))
    if late and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,) or not lengths.is_contiguous()):
        raise _lib.DrnError("%s: lengths must be a contiguous (%d,) torch.int32 tensor" % (what, S))
    V, nblocks = _rank_plan(what, *plan) if plan else (R, -(-R // _lib.SHORTLIST_BLOCK))
    if keys.dtype != torch.int64 or tuple(keys.shape) != (S,) or not keys.is_contiguous():
        raise _lib.DrnError("%s: keys must be a contiguous (%d,) torch.int64 tensor" % (what, S))
    if phase == 1:
        if cnt is not None or targets is None or targets.dtype != torch.int32 or tuple(targets.shape) != (S,) or not targets.is_contiguous():
            raise _lib.DrnError("%s: phase 1 takes targets, a contiguous (%d,) torch.int32 tensor, and no cnt" % (what, S))
        have = 0
    else:
        if targets is not None or cnt is None or cnt.dtype != torch.int64 or not cnt.is_contiguous() or cnt.numel() < S * nblocks:
            raise _lib.DrnError("%s: phase 2 takes cnt, a contiguous torch.int64 tensor of at least %d elements (S * blocks), and no "
                                "targets" % (what, S * nblocks))
        have = int(min(cnt.numel() * 8, 0x7fffffff))
    mask, stride = _allow_args(what, allow, V, S)
    head = (tab, scl, _p(queries)) + ((_p(lengths),) if late else ()) + tuple(_p(t) for t in plan) + (_p(targets), mask, stride)
    sizes = ((R, V, nblocks) if plan else (V,)) + (E, S) + ((L,) if late else ())
    args = head + sizes + (dtype_code(queries), phase, _p(keys), _p(cnt), have)
    # (the flop figure handed to the timer: the whole table in phase 2; phase 1 scores the targets' rows alone, which the host cannot count)
    _timed(what, 2.0 * S * L * R * E if phase == 2 else 0.0, lambda: check(getattr(lib(), "drn_" + what)(*args, _stream()), "drn_" + what))
    return keys if phase == 1 else cnt


def shortlist_rank_phase(table, queries, phase, targets, keys, cnt, allow=None):
    """ONE PHASE of shortlist_rank over a plain table (drn_shortlist_rank_phase), for a corpus kept as several tables: table, queries and
    allow as there.  phase 1: targets (S,) int32 on the device -> keys (S,) int64, the 64-bit key of each sentence's target in THIS
    table, 0 where it is no candidate (cnt = None).  phase 2: keys (S,) int64, read as THRESHOLDS in the place of the target keys ->
    cnt, a contiguous int64 tensor of at least S * ceil(V / SHORTLIST_BLOCK) elements, each two int32 counts of a (sentence, block):
    the candidates above the threshold, and the candidates (targets = None).  One launch (tag shortlist_rank_phase), the kernel and
    the bits of shortlist_rank's launch of that number; nothing is read on the host."""
    return _rank_phase("shortlist_rank_phase", table, queries, None, (), phase, targets, keys, cnt, allow)


def shortlist_segments_rank_phase(table, queries, offsets, blk_vid, phase, targets, keys, cnt, allow=None):
    """shortlist_rank_phase over a RAGGED table (drn_shortlist_segments_rank_phase): offsets (V + 1,) and blk_vid (nblocks + 1,) as in
    shortlist_segments_rank; cnt holds at least S * nblocks elements.  One launch (tag shortlist_segments_rank_phase)."""
    return _rank_phase("shortlist_segments_rank_phase", table, queries, None, (offsets, blk_vid), phase, targets, keys, cnt, allow)


def shortlist_late_rank_phase(table, queries, lengths, offsets, blk_vid, phase, targets, keys, cnt, allow=None):
    """shortlist_rank_phase by LATE INTERACTION (drn_shortlist_late_rank_phase): queries (S, L, E) and lengths (S,) as in
    shortlist_late_rank, the rest as in shortlist_segments_rank_phase.  One launch (tag shortlist_late_rank_phase)."""
    if lengths is None:
        raise _lib.DrnError("shortlist_late_rank_phase: lengths must be a contiguous (S,) torch.int32 tensor")
    return _rank_phase("shortlist_late_rank_phase", table, queries, lengths, (offsets, blk_vid), phase, targets, keys, cnt, allow)


def shortlist_rerank_ws_keys(C, S, n):
    """The 8-byte keys of workspace drn_shortlist_rerank needs: S * ceil(C / RERANK_GROUP) * min(n, RERANK_GROUP)."""
    return int(S) * (-(-int(C) // _lib.RERANK_GROUP)) * min(int(n), _lib.RERANK_GROUP)


def shortlist_rerank(table, queries, lengths, offsets, candidates, n, ws, ids, scores, counts, allow=None):
    """Rerank a candidate list: only the listed (sentence, video) pairs are scored (drn_shortlist_rerank; the *_rerank_reference
    functions of drn_amd.retrieve are the definition).  table is emb (R, E), float32 / bfloat16, or a pair (codes, scales) of a
    block-scaled FP8 table; queries (S, L, E) of the table's dtype (float32 / bfloat16 beside codes), 1 <= L <= LATE_MAX_TOKENS;
    lengths (S,) int32 on the device as in shortlist_late_topn, or None: every token is live; offsets (V + 1,) int32 on the device as
    in shortlist_segments_topn, or None: row v is video v; candidates (S, C) int32 ON THE DEVICE, 1 <= C <= RERANK_MAX_CANDIDATES, row
    s the set of positions sentence s may list -- an entry outside [0, V) means nothing, a repeat counts once -> ids, scores (S, n) and
    counts (S,), written in place, bit for bit what shortlist_late_topn gives under the mask "listed, and allowed".  allow: None, or a
    packed mask as in shortlist_topn.  ws: an int64 tensor of at least shortlist_rerank_ws_keys(C, S, n) elements.  Two launches
    on the current stream behind one entry (one tag, shortlist_rerank); nothing is read on the host -- so the flop figure handed to
    the timer is NOMINAL, 2 S L C (R / V) E: every slot a distinct valid video of the mean run, which the host cannot know."""
    what = "shortlist_rerank"
    tab, scl, R, V, E, S, L, C = _rerank_inputs(what, table, queries, lengths, offsets, candidates, (ws, ids, scores, counts, allow))
    n = int(n)
    _shortlist_buffers(what, S, n, shortlist_rerank_ws_keys(C, S, n), ws, ids, scores, counts)
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * S * L * C * (float(R) / V) * E, lambda: check(lib().drn_shortlist_rerank(
        tab, scl, _p(queries), None if lengths is None else _p(lengths), None if offsets is None else _p(offsets), _p(candidates), mask,
        stride, R, V, E, S, L, C, n, dtype_code(queries), _p(ws), int(min(ws.numel(), 0x7fffffff)), _p(ids), _p(scores), _p(counts),
        _stream()), "drn_shortlist_rerank"))
    return ids, scores, counts


def _rerank_inputs(what, table, queries, lengths, offsets, candidates, others):
    """The checks shortlist_rerank and shortlist_rerank_scores share about the table, the queries (S, L, E), lengths, offsets and
    candidates; `others` are the call's remaining tensors (None among them skipped), which must be on the GPU too -> (table pointer,
    scales pointer or None, R, V, E, S, L, C)."""
    if queries.dim() != 3 or not queries.is_contiguous() or not 1 <= queries.shape[1] <= _lib.LATE_MAX_TOKENS or queries.shape[0] < 1:
        raise _lib.DrnError("%s: queries must be a contiguous (S, L, E) tensor with S >= 1 and 1 <= L <= %d, not %s"
                            % (what, _lib.LATE_MAX_TOKENS, tuple(queries.shape)))
    S, L = int(queries.shape[0]), int(queries.shape[1])
    tensors, tab, scl, R, E = _rank_table(what, table, queries.view(S * L, -1))
    _need_gpu(*(tensors + (queries, candidates) + tuple(t for t in tuple(others) + (lengths, offsets) if t is not None)))
    if lengths is not None and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,) or not lengths.is_contiguous()):
        raise _lib.DrnError("%s: lengths must be a contiguous (%d,) torch.int32 tensor" % (what, S))
    if offsets is None:
        V = R
    else:
        if offsets.dim() != 1 or offsets.numel() < 2 or offsets.dtype != torch.int32 or not offsets.is_contiguous():
            raise _lib.DrnError("%s: offsets must be a contiguous (V + 1,) torch.int32 tensor, V >= 1" % what)
        V = int(offsets.numel()) - 1
    if candidates.dim() != 2 or candidates.dtype != torch.int32 or not candidates.is_contiguous() or int(candidates.shape[0]) != S \
            or not 1 <= candidates.shape[1] <= _lib.RERANK_MAX_CANDIDATES:
        raise _lib.DrnError("%s: candidates must be a contiguous (%d, C) torch.int32 tensor with 1 <= C <= %d, not %s %s"
                            % (what, S, _lib.RERANK_MAX_CANDIDATES, candidates.dtype, tuple(candidates.shape)))
    return tab, scl, R, V, E, S, L, int(candidates.shape[1])


def shortlist_rerank_scores(table, queries, lengths, offsets, candidates, out, allow=None, inside_only=False):
    """The scores of the LISTED pairs, the listed-pairs counterpart of shortlist_scores (drn_shortlist_rerank_scores;
    drn_amd.retrieve.rerank_scores_reference is the definition): table, queries (S, L, E), lengths, offsets, candidates (S, C) and allow as
    in shortlist_rerank -> out, float32 (S, C), written in place, exactly those elements: out may be a ROW-STRIDED view (last stride 1,
    row stride >= C).  out[s, j] is the score shortlist_rerank would list for (s, candidates[s, j]), the same bits (-0 as +0), where the
    slot is live -- its id in [0, V), no earlier slot of the row with the same id, the mask bit set, the video owning a row, the
    sentence a live token -- and the sum is finite; every other slot is -inf: finite <=> candidate.  inside_only: a slot whose id lies
    outside [0, V) is left UNTOUCHED instead of written as -inf (the shards of a corpus write one matrix, each its own slots).  One
    launch (tag shortlist_rerank_scores), no workspace; nothing is read on the host, so the flop figure is shortlist_rerank's nominal one."""
    what = "shortlist_rerank_scores"
    tab, scl, R, V, E, S, L, C = _rerank_inputs(what, table, queries, lengths, offsets, candidates, (out, allow))
    ld = _row_strided(out, S, C) if out.dtype == torch.float32 else None
    if ld is None:
        raise _lib.DrnError("%s: out must be a (%d, %d) torch.float32 tensor with last stride 1 and row stride >= %d, not %s %s with strides %s"
                            % (what, S, C, C, out.dtype, tuple(out.shape), tuple(out.stride())))
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * S * L * C * (float(R) / V) * E, lambda: check(lib().drn_shortlist_rerank_scores(
        tab, scl, _p(queries), None if lengths is None else _p(lengths), None if offsets is None else _p(offsets), _p(candidates), mask,
        stride, R, V, E, S, L, C, dtype_code(queries), int(bool(inside_only)), _p(out), ld, _stream()), "drn_shortlist_rerank_scores"))
    return out


def _row_strided(t, rows, cols):
    """Is t a (rows, cols) view whose elements lie at row * ld + column with ld >= cols -> ld, or None."""
    if t.dim() != 2 or tuple(t.shape) != (rows, cols) or (cols > 1 and t.stride(1) != 1):
        return None
    ld = int(t.stride(0)) if rows > 1 else cols
    return ld if cols <= ld < 2 ** 31 else None


def shortlist_scores(table, queries, lengths, plan, out, allow=None):
    """The WHOLE score matrix of a table (drn_shortlist_scores; drn_amd.retrieve.scores_reference is the definition): table is emb, float32
    / bfloat16, or a pair (codes, scales) of a block-scaled FP8 table; plan is () on a table of one row per video, (offsets, blk_vid)
    int32 on the device on a ragged one; lengths is None -- queries (S, E) -- or (S,) int32 on the device -- late interaction, queries
    (S, L, E), a ragged table only -> out, float32 (S, V), written in place, exactly those elements: out may be a ROW-STRIDED view (last
    stride 1, row stride >= V), such as a column slice of a wider buffer.  out[s, v] has the bits the matching shortlist entry lists
    for the pair (-0 as +0) and is -inf where the video is no candidate (no row, a score that is not finite, a clear mask bit, no
    live token).  allow: None, or a packed mask as in shortlist_topn.  One launch (tag shortlist_scores), no workspace; nothing is
    read on the host."""
    what = "shortlist_scores"
    plan = tuple(plan)
    late = lengths is not None
    if len(plan) not in (0, 2) or (late and not plan):
        raise _lib.DrnError("%s: plan must be () or (offsets, blk_vid), and lengths (late interaction) need a ragged table" % what)
    if late:
        if queries.dim() != 3 or not queries.is_contiguous() or not 1 <= queries.shape[1] <= _lib.LATE_MAX_TOKENS or queries.shape[0] < 1:
            raise _lib.DrnError("%s: queries must be a contiguous (S, L, E) tensor with S >= 1 and 1 <= L <= %d, not %s"
                                % (what, _lib.LATE_MAX_TOKENS, tuple(queries.shape)))
        S, L = int(queries.shape[0]), int(queries.shape[1])
    else:
        if queries.dim() != 2 or queries.shape[0] < 1:
            raise _lib.DrnError("%s: queries must be a contiguous (S, E) tensor with S >= 1, not %s" % (what, tuple(queries.shape)))
        S, L = int(queries.shape[0]), 1
    tensors, tab, scl, R, E = _rank_table(what, table, queries.view(S * L, -1) if late else queries)
    _need_gpu(*(tensors + (queries, out) + plan + tuple(t for t in (lengths, allow) if t is not None)))
    if late and (lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,) or not lengths.is_contiguous()):
        raise _lib.DrnError("%s: lengths must be a contiguous (%d,) torch.int32 tensor" % (what, S))
    V, nblocks = _rank_plan(what, *plan) if plan else (R, 0)
    ld = _row_strided(out, S, V) if out.dtype == torch.float32 else None
    if ld is None:
        raise _lib.DrnError("%s: out must be a (%d, %d) torch.float32 tensor with last stride 1 and row stride >= %d, not %s %s with strides %s"
                            % (what, S, V, V, out.dtype, tuple(out.shape), tuple(out.stride())))
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * S * L * R * E, lambda: check(lib().drn_shortlist_scores(
        tab, scl, _p(queries), None if lengths is None else _p(lengths), _p(plan[0]) if plan else None, _p(plan[1]) if plan else None, mask,
        stride, R if plan else 0, V, nblocks, E, S, L, dtype_code(queries), _p(out), ld, _stream()), "drn_shortlist_scores"))
    return out


def _fuse_args(what, scores, weights, missing, allow):
    """The checks the two fuse wrappers share -> (M, S, V, stride_m, ld, mode, mask pointer, allow_stride)."""
    if missing not in _lib.FUSE_MODES:
        raise _lib.DrnError("%s: missing must be one of %s, not %r" % (what, sorted(_lib.FUSE_MODES), missing))
    if scores.dim() != 3 or scores.dtype != torch.float32 or not 1 <= scores.shape[0] <= _lib.FUSE_MAX_TABLES or scores.shape[1] < 1 \
            or scores.shape[2] < 1:
        raise _lib.DrnError("%s: scores must be (M, S, V) torch.float32 with 1 <= M <= %d, S >= 1 and V >= 1, not %s %s"
                            % (what, _lib.FUSE_MAX_TABLES, scores.dtype, tuple(scores.shape)))
    M, S, V = (int(x) for x in scores.shape)
    ld = _row_strided(scores[0], S, V)
    stride_m = int(scores.stride(0)) if M > 1 else 0
    if ld is None or (M > 1 and stride_m < (S - 1) * ld + V):
        raise _lib.DrnError("%s: scores must have last stride 1, row stride >= V and matrices that do not overlap, not strides %s"
                            % (what, tuple(scores.stride())))
    if weights.dtype != torch.float32 or tuple(weights.shape) != (M,) or not weights.is_contiguous():
        raise _lib.DrnError("%s: weights must be a contiguous (%d,) torch.float32 tensor on the device" % (what, M))
    mask, stride = _allow_args(what, allow, V, S)
    return M, S, V, stride_m, ld, _lib.FUSE_MODES[missing], mask, stride


def shortlist_fuse_topn(scores, weights, missing, n, ws, ids, out_scores, counts, allow=None):
    """Each sentence's best n videos under the FUSED score of M stacked score matrices (drn_shortlist_fuse_topn;
    drn_amd.retrieve.fused_shortlist_reference is the definition): scores (M, S, V) float32 on the device, last stride 1, row stride >= V
    (what shortlist_scores writes: -inf = the video is missing from that table); weights (M,) float32 ON THE DEVICE; missing "drop" -- a
    video missing from any table is no candidate -- or "skip" -- a missing term adds nothing; 1 <= n <= SHORTLIST_DEEP_MAX -> ids,
    out_scores (S, n) and counts (S,), written in place, -1 / 0 past the list.  The fused score is ((0 + w0 * s0) + w1 * s1) + ... in
    fp32, two roundings a term.  allow: None, or a packed mask as in shortlist_topn.  ws: an int64 tensor of at least
    shortlist_ws_keys(V, S, n) elements.  Two launches (tag shortlist_fuse_topn); nothing is read on the host."""
    what = "shortlist_fuse_topn"
    _need_gpu(scores, weights, ws, ids, out_scores, counts, *(() if allow is None else (allow,)))
    M, S, V, stride_m, ld, mode, mask, stride = _fuse_args(what, scores, weights, missing, allow)
    n = int(n)
    _shortlist_buffers(what, S, n, shortlist_ws_keys(V, S, n), ws, ids, out_scores, counts, cap=_lib.SHORTLIST_DEEP_MAX)
    _timed(what, 2.0 * M * S * V, lambda: check(lib().drn_shortlist_fuse_topn(
        _p(scores), stride_m, ld, _p(weights), M, mode, mask, stride, V, S, n, _p(ws), int(min(ws.numel(), 0x7fffffff)), _p(ids),
        _p(out_scores), _p(counts), _stream()), "drn_shortlist_fuse_topn"))
    return ids, out_scores, counts


def shortlist_fuse_rank(scores, weights, missing, targets, rank, score, total, allow=None):
    """The place of targets[s] in sentence s's full order under the fused score (drn_shortlist_fuse_rank;
    drn_amd.retrieve.fused_rank_reference is the definition): scores, weights, missing and allow as in shortlist_fuse_topn; targets (S,)
    int32 ON THE DEVICE, a value outside [0, V) meaning "no target" -> rank, score, total (S,) as in shortlist_rank, written in place.
    One launch (tag shortlist_fuse_rank), no workspace; nothing is read on the host."""
    what = "shortlist_fuse_rank"
    _need_gpu(scores, weights, targets, rank, score, total, *(() if allow is None else (allow,)))
    M, S, V, stride_m, ld, mode, mask, stride = _fuse_args(what, scores, weights, missing, allow)
    for name, t, dt in (("targets", targets, torch.int32), ("rank", rank, torch.int32), ("score", score, torch.float32),
                        ("total", total, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous (%d,) %s tensor" % (what, name, S, dt))
    _timed(what, 2.0 * M * S * V, lambda: check(lib().drn_shortlist_fuse_rank(
        _p(scores), stride_m, ld, _p(weights), M, mode, _p(targets), mask, stride, V, S, _p(rank), _p(score), _p(total), _stream()),
        "drn_shortlist_fuse_rank"))
    return rank, score, total


def shortlist_fuse_rerank(scores, weights, missing, candidates, V, n, ws, ids, out_scores, counts, allow=None):
    """Each sentence's best n LISTED videos under the fused score of M stacked matrices of listed pairs' scores
    (drn_shortlist_fuse_rerank; drn_amd.retrieve.fused_rerank_reference is the definition): scores (M, S, C) float32 on the device, last
    stride 1, row stride >= C, column j of row s belonging to the video candidates[s, j] (what shortlist_rerank_scores writes; any
    matrices are safe); candidates (S, C) int32 ON THE DEVICE as in shortlist_rerank, 1 <= C <= RERANK_MAX_CANDIDATES; V the videos of
    the store the positions index; weights, missing and n as in shortlist_fuse_topn -> ids, out_scores (S, n) and counts (S,), written
    in place, -1 / 0 past the list.  A slot is listed when its id lies in [0, V), no earlier slot of the row holds the same id and
    allow -- None, or a packed mask over the V videos as in shortlist_topn -- does not exclude it; the order is the full fused
    shortlist's, by STORE POSITION.  ws: an int64 tensor of at least shortlist_ws_keys(C, S, n) elements.  Two launches (tag
    shortlist_fuse_rerank); nothing is read on the host."""
    what = "shortlist_fuse_rerank"
    _need_gpu(scores, weights, candidates, ws, ids, out_scores, counts, *(() if allow is None else (allow,)))
    M, S, C, stride_m, ld, mode, _, _ = _fuse_args(what, scores, weights, missing, None)
    V = int(V)
    if V < 1:
        raise _lib.DrnError("%s: V = %d videos, at least one is needed" % (what, V))
    if candidates.dim() != 2 or candidates.dtype != torch.int32 or not candidates.is_contiguous() or tuple(candidates.shape) != (S, C) \
            or not 1 <= C <= _lib.RERANK_MAX_CANDIDATES:
        raise _lib.DrnError("%s: candidates must be a contiguous (%d, %d) torch.int32 tensor, a column per column of scores, with 1 <= C <= %d, "
                            "not %s %s" % (what, S, C, _lib.RERANK_MAX_CANDIDATES, candidates.dtype, tuple(candidates.shape)))
    n = int(n)
    _shortlist_buffers(what, S, n, shortlist_ws_keys(C, S, n), ws, ids, out_scores, counts, cap=_lib.SHORTLIST_DEEP_MAX)
    mask, stride = _allow_args(what, allow, V, S)
    _timed(what, 2.0 * M * S * C, lambda: check(lib().drn_shortlist_fuse_rerank(
        _p(scores), stride_m, ld, _p(weights), M, mode, _p(candidates), mask, stride, V, C, S, n, _p(ws), int(min(ws.numel(), 0x7fffffff)),
        _p(ids), _p(out_scores), _p(counts), _stream()), "drn_shortlist_fuse_rerank"))
    return ids, out_scores, counts


def _rank_fuse_args(what, lists, V, weights, k0, missing, allow):
    """The checks the two rank-fusion wrappers share -> (M, S, C, V, stride_m, ld, k0, mode, mask pointer, allow_stride)."""
    if missing not in _lib.FUSE_MODES:
        raise _lib.DrnError("%s: missing must be one of %s, not %r" % (what, sorted(_lib.FUSE_MODES), missing))
    if lists.dim() != 3 or lists.dtype != torch.int32 or not 1 <= lists.shape[0] <= _lib.RANK_FUSE_MAX_LISTS or lists.shape[1] < 1 \
            or not 1 <= lists.shape[2] <= _lib.SHORTLIST_DEEP_MAX:
        raise _lib.DrnError("%s: lists must be (M, S, C) torch.int32 with 1 <= M <= %d, S >= 1 and 1 <= C <= %d, not %s %s"
                            % (what, _lib.RANK_FUSE_MAX_LISTS, _lib.SHORTLIST_DEEP_MAX, lists.dtype, tuple(lists.shape)))
    M, S, C = (int(x) for x in lists.shape)
    ld = _row_strided(lists[0], S, C)
    stride_m = int(lists.stride(0)) if M > 1 else 0
    if ld is None or (M > 1 and stride_m < (S - 1) * ld + C):
        raise _lib.DrnError("%s: lists must have last stride 1, row stride >= C and lists that do not overlap, not strides %s"
                            % (what, tuple(lists.stride())))
    V, k0 = int(V), float(k0)
    if V < 1:
        raise _lib.DrnError("%s: V = %d videos, at least one is needed" % (what, V))
    if not (0.0 <= k0 < float("inf")):
        raise _lib.DrnError("%s: k0 = %r is not a finite number >= 0" % (what, k0))
    if weights.dtype != torch.float32 or tuple(weights.shape) != (M,) or not weights.is_contiguous():
        raise _lib.DrnError("%s: weights must be a contiguous (%d,) torch.float32 tensor on the device" % (what, M))
    mask, stride = _allow_args(what, allow, V, S)
    return M, S, C, V, stride_m, ld, k0, _lib.FUSE_MODES[missing], mask, stride


def rank_fuse_topn(lists, V, weights, k0, missing, n, ids, scores, counts, allow=None):
    """Each sentence's best n videos under RECIPROCAL-RANK FUSION of M id lists (drn_rank_fuse_topn;
    drn_amd.retrieve.rank_fuse_reference is the definition): lists (M, S, C) int32 on the device, last stride 1, row stride >= C --
    other shortlists' ids, -1 padding, repeats and out-of-range values included; V the videos of the store the positions index;
    weights (M,) float32 ON THE DEVICE; k0 a finite host number >= 0; missing "skip" -- a list that does not hold the video adds
    nothing -- or "drop" -- every list must hold it; 1 <= n <= SHORTLIST_DEEP_MAX -> ids, scores (S, n) and counts (S,), written in
    place, -1 / 0 past the list.  The score is the fp32 sum, m ascending, of w[m] / (k0 + rank in list m + 1).  allow: None, or a packed
    mask as in shortlist_topn.  One launch (tag rank_fuse_topn), no workspace; nothing is read on the host."""
    what = "rank_fuse_topn"
    _need_gpu(lists, weights, ids, scores, counts, *(() if allow is None else (allow,)))
    M, S, C, V, stride_m, ld, k0, mode, mask, stride = _rank_fuse_args(what, lists, V, weights, k0, missing, allow)
    n = int(n)
    if not 1 <= n <= _lib.SHORTLIST_DEEP_MAX:
        raise _lib.DrnError("%s: n = %d outside [1, %d]" % (what, n, _lib.SHORTLIST_DEEP_MAX))
    for name, t, dt, shape in (("ids", ids, torch.int32, (S, n)), ("scores", scores, torch.float32, (S, n)), ("counts", counts, torch.int32, (S,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous %s %s tensor" % (what, name, shape, dt))
    _timed(what, 2.0 * M * S * C, lambda: check(lib().drn_rank_fuse_topn(
        _p(lists), stride_m, ld, C, M, V, _p(weights), k0, mode, mask, stride, S, n, _p(ids), _p(scores), _p(counts), _stream()),
        "drn_rank_fuse_topn"))
    return ids, scores, counts


def rank_fuse_rank(lists, V, weights, k0, missing, targets, rank, score, total, allow=None):
    """The place of targets[s] in sentence s's full order under reciprocal-rank fusion (drn_rank_fuse_rank;
    drn_amd.retrieve.rank_fuse_rank_reference is the definition): lists, V, weights, k0, missing and allow as in rank_fuse_topn; targets
    (S,) int32 ON THE DEVICE, a value outside [0, V) meaning "no target" -> rank, score, total (S,) as in shortlist_rank, written in
    place.  One launch (tag rank_fuse_rank), no workspace; nothing is read on the host."""
    what = "rank_fuse_rank"
    _need_gpu(lists, weights, targets, rank, score, total, *(() if allow is None else (allow,)))
    M, S, C, V, stride_m, ld, k0, mode, mask, stride = _rank_fuse_args(what, lists, V, weights, k0, missing, allow)
    for name, t, dt in (("targets", targets, torch.int32), ("rank", rank, torch.int32), ("score", score, torch.float32),
                        ("total", total, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous (%d,) %s tensor" % (what, name, S, dt))
    _timed(what, 2.0 * M * S * C, lambda: check(lib().drn_rank_fuse_rank(
        _p(lists), stride_m, ld, C, M, V, _p(weights), k0, mode, mask, stride, S, _p(targets), _p(rank), _p(score), _p(total), _stream()),
        "drn_rank_fuse_rank"))
    return rank, score, total


def shortlist_merge_lists(in_ids, in_scores, in_counts, in_rows, bases, n, ids, scores, counts, rows=None):
    """Merge K stacked per-shard lists a sentence into the corpus's list: in_ids, in_scores (K, S, n_in) and in_counts (K, S) as the
    shards' shortlist entries wrote them, in_rows (K, S, n_in) beside them on ragged shards or None, bases (K + 1,) int32 ON THE DEVICE
    (corpus position = bases[k] + id) -> ids, scores (S, n), counts (S,) and -- exactly when in_rows is given -- rows (S, n), written
    in place, every element (drn_shortlist_merge_lists; drn_amd.retrieve.merge_shortlists_reference is the definition).  1 <= K <=
    SHARDS_MAX, n_in and n in [1, SHORTLIST_MAX].  One launch (tag shortlist_merge_lists), no workspace; nothing is read on the host."""
    what = "shortlist_merge_lists"
    _need_gpu(in_ids, in_scores, in_counts, in_rows, bases, ids, scores, counts, rows)
    n = int(n)
    if in_ids.dim() != 3 or not 1 <= in_ids.shape[0] <= _lib.SHARDS_MAX or in_ids.shape[1] < 1 or not 1 <= in_ids.shape[2] <= _lib.SHORTLIST_MAX:
        raise _lib.DrnError("%s: in_ids must be (K, S, n_in) with 1 <= K <= %d, S >= 1 and 1 <= n_in <= %d, not %s"
                            % (what, _lib.SHARDS_MAX, _lib.SHORTLIST_MAX, tuple(in_ids.shape)))
    K, S, n_in = (int(x) for x in in_ids.shape)
    if not 1 <= n <= _lib.SHORTLIST_MAX:
        raise _lib.DrnError("%s: n = %d outside [1, %d]" % (what, n, _lib.SHORTLIST_MAX))
    if (in_rows is None) != (rows is None):
        raise _lib.DrnError("%s: rows must be given on both sides (the lists of ragged shards) or on neither" % what)
    tensors = (("in_ids", in_ids, torch.int32, (K, S, n_in)), ("in_scores", in_scores, torch.float32, (K, S, n_in)),
               ("in_counts", in_counts, torch.int32, (K, S)), ("bases", bases, torch.int32, (K + 1,)), ("ids", ids, torch.int32, (S, n)),
               ("scores", scores, torch.float32, (S, n)), ("counts", counts, torch.int32, (S,)))
    if rows is not None:
        tensors += (("in_rows", in_rows, torch.int32, (K, S, n_in)), ("rows", rows, torch.int32, (S, n)))
    for name, t, dt, shape in tensors:
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous %s %s tensor" % (what, name, shape, dt))
    _timed(what, 0.0, lambda: check(lib().drn_shortlist_merge_lists(
        _p(in_ids), _p(in_scores), _p(in_counts), _p(in_rows), _p(bases), K, S, n_in, n, _p(ids), _p(scores), _p(counts), _p(rows), _stream()),
        "drn_shortlist_merge_lists"))
    return (ids, scores, counts) if rows is None else (ids, scores, counts, rows)


def allow_slice_words(bases):
    """The int32 words a row of the K pieces drn_allow_slices writes, from HOST bases (K + 1 running sums): sum of allow_words(V_k)."""
    return sum(allow_words(int(b) - int(a)) for a, b in zip(bases[:-1], bases[1:]))


def allow_slices(words, bases, host_bases, out):
    """A packed mask over the whole corpus, words (W,) or (S, W) int32 with W = allow_words(V), -> the K shards' own packed masks back to
    back in out, a contiguous int32 tensor of rows * allow_slice_words(host_bases) elements, written in place, every word: piece k is
    (rows, allow_words(V_k)) from element rows * (the words a row of the pieces before it), its word w holding the corpus bits
    bases[k] + 32 w .. + 31 with zero bits at or past V_k (drn_allow_slices; drn_amd.retrieve.slice_allow_reference is the definition).
    bases (K + 1,) int32 ON THE DEVICE, host_bases the same K + 1 running sums on the host (they size the pieces).  One launch (tag
    allow_slices); the mask and the device's bases are not read on the host."""
    what = "allow_slices"
    _need_gpu(words, bases, out)
    K, V = len(host_bases) - 1, int(host_bases[-1])
    if not 1 <= K <= _lib.SHARDS_MAX or int(host_bases[0]) != 0 or any(int(b) <= int(a) for a, b in zip(host_bases[:-1], host_bases[1:])):
        raise _lib.DrnError("%s: host_bases must be the K + 1 running sums of 1 <= K <= %d shards of at least one video, from 0"
                            % (what, _lib.SHARDS_MAX))
    W = allow_words(V)
    if words.dtype != torch.int32 or not words.is_contiguous() or words.dim() not in (1, 2) or int(words.shape[-1]) != W or words.shape[0] < 1:
        raise _lib.DrnError("%s: words must be a contiguous torch.int32 tensor (%d,) or (S, %d) -- ceil(V / 32) packed words a row -- not %s %s"
                            % (what, W, W, words.dtype, tuple(words.shape)))
    rows = 1 if words.dim() == 1 else int(words.shape[0])
    total = allow_slice_words(host_bases)
    if bases.dtype != torch.int32 or tuple(bases.shape) != (K + 1,) or not bases.is_contiguous():
        raise _lib.DrnError("%s: bases must be a contiguous (%d,) torch.int32 tensor" % (what, K + 1))
    if out.dtype != torch.int32 or out.dim() != 1 or int(out.numel()) != rows * total or not out.is_contiguous():
        raise _lib.DrnError("%s: out must be a contiguous (%d,) torch.int32 tensor (%d rows of %d words)" % (what, rows * total, rows, total))
    _timed(what, 0.0, lambda: check(lib().drn_allow_slices(_p(words), rows, V, _p(bases), K, total, _p(out), _stream()), "drn_allow_slices"))
    return out


def shard_positions(positions, bases, out):
    """Corpus positions -> every shard's local positions: positions (S,) or (S, C) int32 ON THE DEVICE (targets; candidate lists, C <=
    RERANK_MAX_CANDIDATES), bases (K + 1,) int32 on the device -> out (K, S) / (K, S, C) int32, written in place, every element:
    out[k] = positions - bases[k] where bases[k] <= positions < bases[k + 1], else -1 (drn_shard_positions;
    drn_amd.retrieve.shard_positions_reference is the definition).  Slice [k] is what shard k's rank and rerank take.  One launch (tag
    shard_positions); nothing is read on the host."""
    what = "shard_positions"
    _need_gpu(positions, bases, out)
    if positions.dtype != torch.int32 or positions.dim() not in (1, 2) or not positions.is_contiguous() or positions.shape[0] < 1 \
            or (positions.dim() == 2 and not 1 <= positions.shape[1] <= _lib.RERANK_MAX_CANDIDATES):
        raise _lib.DrnError("%s: positions must be a contiguous torch.int32 tensor (S,) or (S, C) with S >= 1 and 1 <= C <= %d, not %s %s"
                            % (what, _lib.RERANK_MAX_CANDIDATES, positions.dtype, tuple(positions.shape)))
    if bases.dtype != torch.int32 or bases.dim() != 1 or not 2 <= bases.numel() <= _lib.SHARDS_MAX + 1 or not bases.is_contiguous():
        raise _lib.DrnError("%s: bases must be a contiguous (K + 1,) torch.int32 tensor with 1 <= K <= %d" % (what, _lib.SHARDS_MAX))
    K = int(bases.numel()) - 1
    shape = (K,) + tuple(positions.shape)
    if out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.DrnError("%s: out must be a contiguous %s torch.int32 tensor" % (what, shape))
    S, C = int(positions.shape[0]), 1 if positions.dim() == 1 else int(positions.shape[1])
    _timed(what, 0.0, lambda: check(lib().drn_shard_positions(_p(positions), _p(bases), K, S, C, _p(out), _stream()), "drn_shard_positions"))
    return out


def compact_plan(keep, offsets, k, carry, positions, new_offsets=None):
    """Shard k's step of a compaction's plan: keep, the shard's own piece of the packed mask (allow_words(V) int32 words, as
    allow_slices cuts it) or None for "every video kept"; offsets (V + 1,) int32 of a ragged shard or None; carry (K + 1, 2) int32,
    (videos kept, rows kept) before each shard -- row k is read (row 0 is written, zeros, by k = 0) and row k + 1 written;
    positions (V,) int32, the shard's slice of the corpus's map, written in place, every element: the new position, -1 where
    dropped; new_offsets, given exactly when offsets is: a 1-D int32 buffer that gets the rows kept before every kept video at its
    new position and is closed after every shard (drn_compact_plan; drn_amd.retrieve.compact_reference is the definition).  The K
    launches go in stream order, k = 0 first.  One launch (tag compact_plan), one workgroup; nothing is read on the host."""
    what = "compact_plan"
    _need_gpu(keep, offsets, carry, positions, new_offsets)
    if positions.dtype != torch.int32 or positions.dim() != 1 or positions.numel() < 1 or not positions.is_contiguous():
        raise _lib.DrnError("%s: positions must be a contiguous (V,) torch.int32 tensor with V >= 1" % what)
    V = int(positions.numel())
    if carry.dtype != torch.int32 or carry.dim() != 2 or carry.shape[1] != 2 or not 2 <= carry.shape[0] <= _lib.SHARDS_MAX + 1 \
            or not carry.is_contiguous():
        raise _lib.DrnError("%s: carry must be a contiguous (K + 1, 2) torch.int32 tensor with 1 <= K <= %d" % (what, _lib.SHARDS_MAX))
    K, k = int(carry.shape[0]) - 1, int(k)
    if not 0 <= k < K:
        raise _lib.DrnError("%s: shard k = %d outside [0, %d)" % (what, k, K))
    if keep is not None and (keep.dtype != torch.int32 or tuple(keep.shape) != (allow_words(V),) or not keep.is_contiguous()):
        raise _lib.DrnError("%s: keep must be a contiguous (%d,) torch.int32 tensor, the shard's piece of the packed mask" % (what, allow_words(V)))
    if (offsets is None) != (new_offsets is None):
        raise _lib.DrnError("%s: offsets and new_offsets must both be given (a ragged shard) or neither" % what)
    cap = 0
    if offsets is not None:
        if offsets.dtype != torch.int32 or tuple(offsets.shape) != (V + 1,) or not offsets.is_contiguous():
            raise _lib.DrnError("%s: offsets must be a contiguous (%d,) torch.int32 tensor" % (what, V + 1))
        if new_offsets.dtype != torch.int32 or new_offsets.dim() != 1 or new_offsets.numel() < 2 or not new_offsets.is_contiguous():
            raise _lib.DrnError("%s: new_offsets must be a contiguous 1-D torch.int32 tensor of at least 2 entries" % what)
        cap = int(new_offsets.numel())
    _timed(what, 0.0, lambda: check(lib().drn_compact_plan(_p(keep), _p(offsets), V, k, K, cap, _p(carry), _p(positions), _p(new_offsets),
                                                           _stream()), "drn_compact_plan"))
    return positions


def _compact_side(what, name, table):
    """One side of compact_rows, a plain tensor or a (codes, scales) pair -> (tensor of the rows, scales or None, rows, E)."""
    t, scales = table if isinstance(table, tuple) else (table, None)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or not t.is_contiguous():
        raise _lib.DrnError("%s: %s must be a contiguous (rows, E) tensor with rows >= 1 and E >= 1, not %s" % (what, name, tuple(t.shape)))
    rows, E = (int(x) for x in t.shape)
    if scales is None:
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise _lib.DrnError("%s: a plain %s must be float32 or bfloat16, not %s" % (what, name, t.dtype))
    elif t.dtype != torch.uint8 or scales.dtype != torch.uint8 or E % 32 or tuple(scales.shape) != (rows, E // 32) or not scales.is_contiguous():
        raise _lib.DrnError("%s: a quantised %s is codes (rows, E) and scales (rows, E / 32), contiguous uint8 tensors with E a multiple "
                            "of 32" % (what, name))
    return t, scales, rows, E


def compact_rows(src, src_offsets, positions, dst_offsets, dst_videos, dst, dst_row0=0, dtype=None):
    """The kept rows of ONE shard to their places in the new table.  src: the shard's table, a plain (rows, E) tensor or the pair
    (codes, scales); src_offsets (V + 1,) int32 of a ragged shard or None; positions (V,) int32, the shard's slice as compact_plan
    wrote it; dst_offsets, given exactly when src_offsets is: the new table's offsets on the device, at least dst_videos + 1 int32
    entries; dst_videos = V', the videos of the new table; dst: the rows [dst_row0, dst_row0 + len(dst)) of the new table -- the whole
    table, a row slice, or a staging buffer standing for one --, plain or a pair: a row outside it is not written
    (drn_compact_rows).  plain -> plain copies, pair -> pair copies codes and scale bytes, pair -> plain dequantises exactly; plain ->
    pair is REFUSED (stage the rows and run quantize_rows_mx8).  dtype: of the queries, needed only when both sides are pairs.  One
    launch (tag compact_rows); nothing is read on the host."""
    what = "compact_rows"
    s, s_scales, src_rows, E = _compact_side(what, "src", src)
    d, d_scales, dst_rows, Ed = _compact_side(what, "dst", dst)
    _need_gpu(s, s_scales, src_offsets, positions, dst_offsets, d, d_scales)
    if Ed != E:
        raise _lib.DrnError("%s: src has E = %d columns, dst %d" % (what, E, Ed))
    if s_scales is None and d_scales is not None:
        raise _lib.DrnError("%s: plain -> mxfp8 is not taken here (there is one quantiser): move the plain rows into a staging buffer and "
                            "run quantize_rows_mx8 on it" % what)
    if s_scales is None and d.dtype != s.dtype:
        raise _lib.DrnError("%s: src is %s, dst %s" % (what, s.dtype, d.dtype))
    plain = s if s_scales is None else d if d_scales is None else None
    if plain is None and dtype not in (torch.float32, torch.bfloat16):
        raise _lib.DrnError("%s: dtype (of the queries) must be float32 or bfloat16 between two quantised tables, not %s" % (what, dtype))
    code = dtype_code(plain) if plain is not None else (F32 if dtype == torch.float32 else BF16)
    if positions.dtype != torch.int32 or positions.dim() != 1 or positions.numel() < 1 or not positions.is_contiguous():
        raise _lib.DrnError("%s: positions must be a contiguous (V,) torch.int32 tensor with V >= 1" % what)
    V, dst_videos, dst_row0 = int(positions.numel()), int(dst_videos), int(dst_row0)
    if (src_offsets is None) != (dst_offsets is None):
        raise _lib.DrnError("%s: src_offsets and dst_offsets must both be given (ragged tables) or neither" % what)
    if dst_videos < 1 or dst_row0 < 0:
        raise _lib.DrnError("%s: dst_videos = %d below 1 or dst_row0 = %d below 0" % (what, dst_videos, dst_row0))
    if src_offsets is None:
        if src_rows != V:
            raise _lib.DrnError("%s: a table of one row a video has %d rows for %d positions" % (what, src_rows, V))
    else:
        if src_offsets.dtype != torch.int32 or tuple(src_offsets.shape) != (V + 1,) or not src_offsets.is_contiguous():
            raise _lib.DrnError("%s: src_offsets must be a contiguous (%d,) torch.int32 tensor" % (what, V + 1))
        if dst_offsets.dtype != torch.int32 or dst_offsets.dim() != 1 or dst_offsets.numel() < dst_videos + 1 or not dst_offsets.is_contiguous():
            raise _lib.DrnError("%s: dst_offsets must be a contiguous 1-D torch.int32 tensor of at least dst_videos + 1 = %d entries"
                                % (what, dst_videos + 1))
    _timed(what, 0.0, lambda: check(lib().drn_compact_rows(
        _p(s), _p(s_scales), _p(src_offsets), _p(positions), _p(dst_offsets), V, src_rows, E, int(s_scales is not None), int(d_scales is not None),
        code, dst_videos, dst_row0, dst_rows, _p(d), _p(d_scales), _stream()), "drn_compact_rows"))
    return dst


POOL_HOW = {"mean": 0, "max": 1}     # DRN_POOL_MEAN / DRN_POOL_MAX


def pool_args(what, how, group):
    """how= and group= of a pooling, for every caller (pool_segments, drn_amd.retrieve) -> group as None or a Python integer >= 1;
    anything else raises."""
    if not isinstance(how, str) or how not in POOL_HOW:
        raise _lib.DrnError("%s: how must be one of %s, not %r" % (what, tuple(POOL_HOW), how))
    if group is None:
        return None
    if isinstance(group, bool) or not isinstance(group, numbers.Integral) or not 1 <= int(group) < 2 ** 31:
        raise _lib.DrnError("%s: group must be None (one row a video) or an integer in [1, 2^31), not %r" % (what, group))
    return int(group)


def pool_segments(table, offsets, out, how="mean", group=None, out_offsets=None, out_row0=0):
    """POOL the segments of a ragged table into plain rows (drn_pool_segments; drn_amd.retrieve.pool_segments_reference is the
    definition, bit for bit).  table: the plain (R, E) rows, float32 / bfloat16, or the pair (codes, scales) of a block-scaled FP8
    table; offsets (V + 1,) int32 on the device, the table's own.  out: (rows, E) PLAIN rows of the table's dtype -- with a pair it
    is out's dtype that says how the values are dequantised --, written in place, every element: the pooled table's rows
    [out_row0, out_row0 + rows), the whole of it or a staging buffer's chunk.  how: "mean" (an fp32 sum in ascending row order, one
    division, one rounding) or "max" (ascending, x > acc ? x : acc).  group None: one row a video, out_offsets None, out_row0 + rows
    <= V, and a video without rows gives a row of +0; group = g >= 1: one row per g rows of a video, out_offsets (V + 1,) int32 on the
    device, the pooled table's own offsets (ceil(len_v / g) rows a video), which the CALLER made.  One launch (tag pool_segments);
    nothing is read on the host."""
    what = "pool_segments"
    q8 = isinstance(table, (tuple, list))
    t, scales = (table[0], table[1]) if q8 else (table, None)
    for x in (t, scales, offsets, out, out_offsets):
        if x is not None and not torch.is_tensor(x):
            raise _lib.DrnError("%s: the table, the offsets and out must be tensors" % what)
    _need_gpu(t, scales, offsets, out, out_offsets)
    group = pool_args(what, how, group)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or not t.is_contiguous():
        raise _lib.DrnError("%s: the table must be a contiguous (R, E) tensor with R >= 1 and E >= 1, not %s" % (what, tuple(t.shape)))
    R, E = (int(x) for x in t.shape)
    if q8:
        if t.dtype != torch.uint8 or scales.dtype != torch.uint8 or E % 32 or tuple(scales.shape) != (R, E // 32) or not scales.is_contiguous():
            raise _lib.DrnError("%s: a quantised table is codes (R, E) and scales (R, E / 32), contiguous uint8 tensors with E a multiple "
                                "of 32" % what)
    elif t.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.DrnError("%s: a plain table must be float32 or bfloat16, not %s" % (what, t.dtype))
    if out.dtype not in (torch.float32, torch.bfloat16) or (not q8 and out.dtype != t.dtype):
        raise _lib.DrnError("%s: out must be float32 or bfloat16, and of a plain table's dtype, not %s" % (what, out.dtype))
    if out.dim() != 2 or out.shape[0] < 1 or int(out.shape[1]) != E or not out.is_contiguous():
        raise _lib.DrnError("%s: out must be a contiguous (rows, %d) tensor with rows >= 1, not %s" % (what, E, tuple(out.shape)))
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
        raise _lib.DrnError("%s: offsets must be a contiguous (V + 1,) torch.int32 tensor with V >= 1" % what)
    V, rows, out_row0 = int(offsets.numel()) - 1, int(out.shape[0]), int(out_row0)
    if (group is None) != (out_offsets is None):
        raise _lib.DrnError("%s: out_offsets must be given exactly with group= (group=None: one row a video)" % what)
    if out_offsets is not None and (out_offsets.dtype != torch.int32 or tuple(out_offsets.shape) != (V + 1,) or not out_offsets.is_contiguous()):
        raise _lib.DrnError("%s: out_offsets must be a contiguous (%d,) torch.int32 tensor" % (what, V + 1))
    if out_row0 < 0 or out_row0 + rows > (V if group is None else R):
        raise _lib.DrnError("%s: out holds the pooled rows [%d, %d), outside [0, %d]%s"
                            % (what, out_row0, out_row0 + rows, V if group is None else R,
                               " (one row a video)" if group is None else " (a group holds at least one of the R rows)"))
    _timed(what, 0.0, lambda: check(lib().drn_pool_segments(
        _p(t), _p(scales), _p(offsets), _p(out_offsets), R, V, rows, out_row0, E, 0 if group is None else group, POOL_HOW[how],
        dtype_code(out), _p(out), _stream()), "drn_pool_segments"))
    return out


def shortlist_sharded_rank_ws_keys(blocks, S):
    """The int64 elements of the stacked workspace of a rank over K shards, from the shards' block counts (HOST integers): K * S keys,
    K * S thresholds, then the K count regions of S * blocks[k] elements each."""
    return int(S) * (2 * len(blocks) + sum(int(b) for b in blocks))


def shortlist_rank_thresholds(keys, thresholds, key):
    """The K shards' target keys -> their counting thresholds and the target's key: keys (K, S) int64 as phase 1 of the *_rank_phase
    wrappers wrote them for the local targets of shard_positions (at most one per column is not 0) -> thresholds (K, S) int64 for phase
    2 and key (S,) int64, written in place (drn_shortlist_rank_thresholds; drn_amd.retrieve.rank_thresholds_reference is the
    definition).  One launch (tag shortlist_rank_thresholds)."""
    what = "shortlist_rank_thresholds"
    _need_gpu(keys, thresholds, key)
    if keys.dtype != torch.int64 or keys.dim() != 2 or not 1 <= keys.shape[0] <= _lib.SHARDS_MAX or keys.shape[1] < 1 or not keys.is_contiguous():
        raise _lib.DrnError("%s: keys must be a contiguous (K, S) torch.int64 tensor with 1 <= K <= %d and S >= 1, not %s %s"
                            % (what, _lib.SHARDS_MAX, keys.dtype, tuple(keys.shape)))
    K, S = (int(x) for x in keys.shape)
    for name, t, shape in (("thresholds", thresholds, (K, S)), ("key", key, (S,))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous %s torch.int64 tensor" % (what, name, shape))
    _timed(what, 0.0, lambda: check(lib().drn_shortlist_rank_thresholds(_p(keys), K, S, _p(thresholds), _p(key), _stream()),
                                    "drn_shortlist_rank_thresholds"))
    return thresholds, key


def shortlist_rank_reduce_shards(key, cnt, blk_off, blocks, rank, score, total):
    """The K shards' block counts -> the corpus's TargetRank fields: key (S,) int64 from shortlist_rank_thresholds; cnt, a contiguous
    int64 tensor holding the K regions back to back, region k (S, blocks of shard k) from element S * blk_off[k]; blk_off (K + 1,) int32
    ON THE DEVICE, the running sums of the shards' blocks, and blocks = blk_off[K] as the host knows it -> rank, score, total (S,),
    written in place (drn_shortlist_rank_reduce_shards): the sums over all blocks, rank -1 and score 0 where key == 0.  One launch (tag
    shortlist_rank_reduce_shards); nothing is read on the host."""
    what = "shortlist_rank_reduce_shards"
    _need_gpu(key, cnt, blk_off, rank, score, total)
    if key.dtype != torch.int64 or key.dim() != 1 or key.numel() < 1 or not key.is_contiguous():
        raise _lib.DrnError("%s: key must be a contiguous (S,) torch.int64 tensor" % what)
    S, blocks = int(key.numel()), int(blocks)
    if blk_off.dtype != torch.int32 or blk_off.dim() != 1 or not 2 <= blk_off.numel() <= _lib.SHARDS_MAX + 1 or not blk_off.is_contiguous():
        raise _lib.DrnError("%s: blk_off must be a contiguous (K + 1,) torch.int32 tensor with 1 <= K <= %d" % (what, _lib.SHARDS_MAX))
    K = int(blk_off.numel()) - 1
    if blocks < K or cnt.dtype != torch.int64 or not cnt.is_contiguous() or cnt.numel() < S * blocks:
        raise _lib.DrnError("%s: cnt must be a contiguous torch.int64 tensor of at least %d elements (S * blocks), blocks = %d >= K = %d"
                            % (what, S * max(blocks, K), blocks, K))
    for name, t, dt in (("rank", rank, torch.int32), ("score", score, torch.float32), ("total", total, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous():
            raise _lib.DrnError("%s: %s must be a contiguous (%d,) %s tensor" % (what, name, S, dt))
    _timed(what, 0.0, lambda: check(lib().drn_shortlist_rank_reduce_shards(
        _p(key), _p(cnt), int(min(cnt.numel() * 8, 0x7fffffff)), _p(blk_off), K, S, blocks, _p(rank), _p(score), _p(total), _stream()),
        "drn_shortlist_rank_reduce_shards"))
    return rank, score, total


def plan_candidates(cand, num_videos, Sc, Nc, pairs, steps, table):
    """cand (S, N) int32 on the device -> table (steps, pairs) int32, written in place, every element (drn_plan_candidates;
    drn_amd.grounding.plan_candidates_reference is the definition): the pair_video rows of a search over device candidates.  One launch
    (tag plan_candidates); cand is not read on the host."""
    _need_gpu(cand, table)
    if cand.dim() != 2 or cand.dtype != torch.int32 or not cand.is_contiguous():
        raise _lib.DrnError("plan_candidates: cand must be a contiguous (S, N) int32 tensor")
    if table.dtype != torch.int32 or tuple(table.shape) != (int(steps), int(pairs)) or not table.is_contiguous():
        raise _lib.DrnError("plan_candidates: table must be a contiguous (%d, %d) int32 tensor" % (int(steps), int(pairs)))
    S, N = (int(x) for x in cand.shape)
    _timed("plan_candidates", 0, lambda: check(lib().drn_plan_candidates(
        _p(cand), S, N, int(num_videos), int(Sc), int(Nc), int(pairs), int(steps), _p(table), _stream()), "drn_plan_candidates"))
    return table


# ---------------------------------------------------------------------------------------------
# query-encoder glue (drn_amd/csrc/qenc.hip)
# ---------------------------------------------------------------------------------------------
def qe_embed_fwd(tokens, table, out_tm, B, L, E):
    _need_gpu(tokens, table, out_tm)
    check(lib().drn_qe_embed_fwd(_p(tokens), _p(table), _p(out_tm), B, L, E, _stream()), "drn_qe_embed_fwd")


def qe_embed_bwd(tokens, demb_tm, dtable, B, L, E, V, padding_idx):
    check(lib().drn_qe_embed_bwd(_p(tokens), _p(demb_tm), _p(dtable), B, L, E, V, padding_idx, _stream()), "drn_qe_embed_bwd")


def qe_qvec_fwd(out, lens, qvec, B, L, C):
    check(lib().drn_qe_qvec_fwd(_p(out), _p(lens), _p(qvec), B, L, C, _stream()), "drn_qe_qvec_fwd")


def qe_qvec_bwd(dqvec, lens, dout, B, L, C):
    check(lib().drn_qe_qvec_bwd(_p(dqvec), _p(lens), _p(dout), B, L, C, _stream()), "drn_qe_qvec_bwd")


def qe_attn_fwd(out, qcmd, w, bias, lens, att, cmds, B, L, C):
    _need_gpu(out, qcmd, cmds)
    check(lib().drn_qe_attn_fwd(_p(out), _p(qcmd), _p(w), _p(bias), _p(lens), _p(att), _p(cmds), B, L, C, _stream()),
          "drn_qe_attn_fwd")


def qe_attn_bwd(dcmds, att, out, qcmd, w, lens, dqcmd, dout, dw_part, dbias_part, B, L, C):
    check(lib().drn_qe_attn_bwd(_p(dcmds[0]), _p(dcmds[1]), _p(dcmds[2]), _p(att), _p(out), _p(qcmd), _p(w), _p(lens), _p(dqcmd),
                                _p(dout), _p(dw_part), _p(dbias_part), B, L, C, _stream()), "drn_qe_attn_bwd")


def colsum_segs(X, ld, M, segs):
    """segs: [(dst fp32 tensor, first column, columns)]: dst[j] = sum_m X[m][col0 + j]."""
    _need_gpu(X)
    arr = (_lib.ColSeg * len(segs))(*[_lib.ColSeg(dst=_p(d), col0=c0, n=n) for d, c0, n in segs])
    check(lib().drn_colsum_segs(_p(X), ld, M, arr, len(segs), _stream()), "drn_colsum_segs")


# ---------------------------------------------------------------------------------------------
# language-guided pooling
# ---------------------------------------------------------------------------------------------
def lgp_fwd(x, ldx, qn, out, att, B, t, C, dtype):
    check(lib().drn_lgp_fwd(_p(x), ldx, _p(qn), _p(out), C, _p(att), B, t, C, dtype, _stream()), "drn_lgp_fwd")


def lgp_bwd(x, ldx, qn, att, dout, dx, dqn, B, t, C, dtype):
    ws = workspace(B * ((t // 2 + 3) // 4) * C, dqn.device)
    check(lib().drn_lgp_bwd(_p(x), ldx, _p(qn), _p(att), _p(dout), C, _p(dx), C, _p(dqn), _p(ws), B, t, C, dtype, _stream()),
          "drn_lgp_bwd")


def mfma_sustained(iters=20000, zero_operands=False):
    """MEASUREMENT (bench.py): what the chip sustains on bf16 MFMA under its power budget -- a register-only v_mfma_f32_32x32x16_bf16 loop at
    the issue floor, random bf16 operands (or zeros).  Returns dict(tflops, clock_ghz, cycles_per_mfma).  See include/drn_hip.h."""
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = torch.empty(int(lib().drn_diag_mfma_ws_bytes()), dtype=torch.uint8, device=dev)
    tf, ghz, cyc = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    check(lib().drn_diag_mfma_sustained(_p(ws), int(iters), int(bool(zero_operands)), ctypes.byref(tf), ctypes.byref(ghz), ctypes.byref(cyc),
                                        _stream()), "drn_diag_mfma_sustained")
    return {"tflops": tf.value, "clock_ghz": ghz.value, "cycles_per_mfma": cyc.value}
