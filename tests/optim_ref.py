"""A float64 model of the clip + Adam kernels of drn_amd/csrc/optim.hip, a forward error bound for them, the predicates that say which
code path each block, quad and tile takes, and the cases the CPU and GPU tests share (tests/test_optim_ref_cpu.py,
tests/test_optim_kernels_gpu.py).  numpy only: nothing here touches a device.

What the kernels compute (include/drn_hip.h, drn_adam_bucket / drn_adam_tiled), per element, with t the device step counter:

    clip = min(1, max_norm / (sqrt(total_sumsq) + 1e-6))        (1 when max_norm <= 0)
    gh   = g * grad_scale * clip
    m    = beta1 * m0 + (1 - beta1) * gh
    v    = beta2 * v0 + (1 - beta2) * gh * gh
    p    = p0 - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

`adam_model` evaluates exactly that in float64 on the fp32 inputs the kernel receives; `adam_bound` bounds how far a correct fp32
evaluation may sit from it; `emulate_fp32` is such an evaluation (and, with `mutant=`, a subtly wrong one)."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32: one correctly rounded operation has relative error <= U
ULP = 2.0 * U             # an error of k ulps is a relative error of at most k * 2^-23
# powf: no document with the device math library's error table ships with the ROCm toolchain this project builds with, so the value is
# ASSUMED: 2 ulps (the HIP programming guide's table of device functions gives 1 ulp for powf; OpenCL's limit for pow is 16).
POW_ULPS = 2
# sqrtf and fp32 division are correctly rounded by default in clang's HIP mode (0.5 ulp); 1 ulp is what the HIP guide's table
# promises, and what is allowed here.
SQRT_ULPS = 1
DIV_ULPS = 1
SECOND_ORDER = 2.0 ** -10  # see adam_bound: every relative error is below 2^-11, so products of two of them are below 2^-11 of their sum

BLOCK = 4096              # OPT_ELEMS_PER_BLOCK
THREADS = 256             # OPT_THREADS
TILE = 64                 # rows and channels of one drn_adam_tiled tile
MAX_SKIP, MAX_EXT = 16, 8  # DRN_SUMSQ_MAX_SKIP, DRN_SUMSQ_MAX_EXT
F32, BF16 = 0, 1           # DRN_F32, DRN_BF16
CLIP_EPS = float(np.float32(1e-6))


def f32(x):
    """A scalar as the kernel receives it through a `float` argument."""
    return float(np.float32(x))


def gamma(k):
    """Higham's gamma_k for fp32: k rounded operations in a row multiply a value by (1 + theta), |theta| <= gamma(k)."""
    return k * U / (1.0 - k * U)


def vec_of(code):
    """VEC = 16 / sizeof(T) of tiled_flush."""
    return 8 if code == BF16 else 4


# ----------------------------------------------------------------------------------------------------------------------------------
# norm passes
# ----------------------------------------------------------------------------------------------------------------------------------
def nblocks(n):
    return (n + BLOCK - 1) // BLOCK


def sumsq_model(g, skip=(), ext=(), grad_scale=1.0):
    """(partials [nblocks] float64, total float64): partials[b] = sum of g^2 over block b without the elements of the `skip` ranges
    [(lo, hi), ...]; total = grad_scale^2 * (sum of the partials + sum of every array in `ext`)."""
    g = np.asarray(g, dtype=np.float64)
    n = g.shape[0]
    keep = np.ones(n, dtype=bool)
    for lo, hi in skip:
        keep[lo:hi] = False
    sq = np.where(keep, np.where(keep, g, 0.0) ** 2, 0.0)
    pad = np.zeros(nblocks(n) * BLOCK)
    pad[:n] = sq
    partials = pad.reshape(-1, BLOCK).sum(1)
    gs = f32(grad_scale)
    total = gs * gs * (partials.sum() + sum(float(np.asarray(e, dtype=np.float64).sum()) for e in ext))
    return partials, total


# The longest chain of rounded additions a term goes through.  All terms are non-negative, so if every term passes through at most k
# rounded additions the computed sum is sum x_i (1 + theta_i) with |theta_i| <= gamma(k): |computed - exact| <= gamma(k) * exact.
#   partials: a thread adds BLOCK / THREADS = 16 squares with one fmaf each (one rounding per term, the square included), wave_sum adds
#   log2(64) = 6 levels, the second wave_sum over the per-wave sums 6 more: 16 + 6 + 6 = 28.  The boundary blocks of the skip kernel
#   walk the block with stride THREADS: at most 16 terms per thread as well.
PARTIAL_CHAIN = BLOCK // THREADS + 6 + 6


def finalize_chain(npartials, ext_n=()):
    """finalize / finalize2: a thread of the 1024 adds ceil(n / 1024) partials and ceil(ne / 1024) values of every external array in
    a row, block_sum adds 6 + 6 levels, and the result is multiplied by grad_scale twice."""
    return -(-npartials // 1024) + sum(-(-ne // 1024) for ne in ext_n) + 6 + 6 + 2


def sumsq_bound(exact, chain):
    return gamma(chain) * np.asarray(exact, dtype=np.float64)


def skip_paths(n, ranges):
    """The path every block of sumsq_partials_skip_kernel takes: "clear" (the plain pass's statements), "inside" (writes 0), "boundary"
    (one or two ranges reach into it) or "extra" (three or more do: the walk over every range per element)."""
    out = []
    for b in range(nblocks(n)):
        base, end = b * BLOCK, min(n, (b + 1) * BLOCK)
        touching = [1 for lo, hi in ranges if lo < end and base < hi]
        if any(lo <= base and end <= hi for lo, hi in ranges):
            out.append("inside")
        else:
            out.append("clear" if not touching else ("extra" if len(touching) >= 3 else "boundary"))
    return out


SKIP_N = 3 * BLOCK + 5
SKIP_CASES = {
    "four_in_one_block": [(10, 20), (100, 130), (1000, 1001), (2000, 2500)],
    "sixteen": [(700 * i + 3, 700 * i + 3 + 37 * (i + 1)) for i in range(16)],
    "block_edge_and_n": [(4000, BLOCK), (BLOCK + 7, 2 * BLOCK), (SKIP_N - 3, SKIP_N)],
    "empty": [(50, 50), (BLOCK, BLOCK), (5000, 5100)],
    "everything": [(0, SKIP_N)],
    "whole_blocks": [(BLOCK, 3 * BLOCK)],
}


# ----------------------------------------------------------------------------------------------------------------------------------
# the update
# ----------------------------------------------------------------------------------------------------------------------------------
def _scalars(total_sumsq, t, lr, beta1, beta2, eps, max_norm, grad_scale):
    lr, b1, b2, eps, mx, gs = (f32(x) for x in (lr, beta1, beta2, eps, max_norm, grad_scale))
    tot = float(total_sumsq)              # (the caller passes the fp32 value the kernel is handed; it is not rounded again)
    clip = min(1.0, mx / (np.sqrt(tot) + CLIP_EPS)) if mx > 0 else 1.0
    return lr, b1, b2, eps, mx, gs, clip, 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)


def adam_model(g, m0, v0, p0, total_sumsq, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5, grad_scale=1.0):
    """(m, v, p) in float64.  Arrays: the fp32 values the kernel receives, widened; scalars: rounded to fp32 first, as the kernel's
    `float` arguments are; total_sumsq: the fp32 value handed to the kernel (the squared norm of grad_scale * g)."""
    g, m0, v0, p0 = (np.asarray(x, dtype=np.float64) for x in (g, m0, v0, p0))
    lr, b1, b2, eps, mx, gs, clip, bc1, bc2 = _scalars(total_sumsq, t, lr, beta1, beta2, eps, max_norm, grad_scale)
    gh = g * gs * clip
    m = b1 * m0 + (1.0 - b1) * gh
    v = b2 * v0 + (1.0 - b2) * gh * gh
    p = p0 - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return m, v, p


def pow_cond(beta, t):
    """beta^t / (1 - beta^t): how much 1 - powf(beta, t) amplifies powf's relative error."""
    pw = f32(beta) ** float(t)
    return pw / (1.0 - pw)


def adam_bound(g, m0, v0, p0, total_sumsq, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5, grad_scale=1.0, pow_ulps=None):
    """(dm, dv, dp): per-element bounds on |kernel - adam_model| for a correct fp32 evaluation in the kernels' operation order.
    Counts are in units of U = 2^-24 per rounded operation; S = 2 SQRT_ULPS and D = 2 DIV_ULPS are a sqrtf and a division.  A fused
    multiply-add rounds once where the separate operations round twice, so contraction only lowers a count: the bound holds either way.

      clip  = max_norm / (sqrtf(total) + 1e-6f), min with 1                 Ec = S + 1 + D     (0 when max_norm <= 0; min is exact
                                                                                                 and does not amplify an error)
      gh    = (g * grad_scale) * clip                                        Eg = Ec + 2
      m     = beta1 * m0 + (1 - beta1) * gh        |beta1 m0| : 1 (product) + 1 (sum)                      = 2
                                                   |(1-beta1) gh| : Eg + 1 (1 - beta1) + 1 (product) + 1 (sum) = Eg + 3
                                                   (absolute: the two terms may cancel)
      v     = beta2 * v0 + ((1 - beta2) * gh) * gh  beta2 v0 : 2;  (1-beta2) gh^2 : 2 Eg + 1 + 2 (products) + 1 (sum) = 2 Eg + 4
      bc1   = 1 - powf(beta1, t)                   E1 = 2 POW_ULPS * beta1^t / (1 - beta1^t) + 1
      bc2   = 1 - powf(beta2, t)                   E2 = 2 POW_ULPS * beta2^t / (1 - beta2^t) + 1
              (POW_ULPS ulps = 2 POW_ULPS U relative on beta^t; the subtraction divides it by (1 - beta^t): ~1000 x at t = 1 for beta2)
      step  = lr / bc1                             E1 + D
      isb2  = 1 / sqrtf(bc2)                       E2 / 2 + S + D
      A     = sqrtf(v) * isb2                      ev / 2 + S + (E2 / 2 + S + D) + 1,  ev = dv / v: the kernel takes the root of ITS v
      den   = A + eps                              Eden = EA * A / (A + eps) + 1
      upd   = (step * m) / den                     |upd| (E1 + D + 1 + Eden + D) + dm * step / den: the kernel divides ITS m
      p     = p0 - upd                             dp = d(upd) + U |p|        (the final subtraction rounds the result once)

    Every relative error above is asserted to be below 2^-11, so the products of two of them that a first-order count leaves out are
    below 2^-11 of their sum: the whole bound is multiplied by (1 + SECOND_ORDER), 2^-10.  Subnormal results are outside this model:
    the cases keep every non-zero intermediate a normal fp32 number (beta^t itself may underflow: 1 - beta^t is then 1 exactly).
    pow_ulps: POW_ULPS by default; 0 gives the bound of an exact powf, which the tests use to REPORT how much of powf's allowance a
    kernel needs (they assert the bound with POW_ULPS)."""
    pow_ulps = POW_ULPS if pow_ulps is None else pow_ulps
    g, m0, v0, p0 = (np.asarray(x, dtype=np.float64) for x in (g, m0, v0, p0))
    lr, b1, b2, eps, mx, gs, clip, bc1, bc2 = _scalars(total_sumsq, t, lr, beta1, beta2, eps, max_norm, grad_scale)
    S, D = 2.0 * SQRT_ULPS, 2.0 * DIV_ULPS
    Ec = S + 1 + D if mx > 0 else 0.0
    Eg = Ec + 2
    gh = g * gs * clip
    m, v, p = adam_model(g, m0, v0, p0, total_sumsq, t, lr, b1, b2, eps, mx, gs)
    dm = (2 * np.abs(b1 * m0) + (Eg + 3) * np.abs((1.0 - b1) * gh)) * U
    dv = (2 * b2 * v0 + (2 * Eg + 4) * (1.0 - b2) * gh * gh) * U
    E1 = 2.0 * pow_ulps * pow_cond(b1, t) + 1
    E2 = 2.0 * pow_ulps * pow_cond(b2, t) + 1
    ev = np.where(v > 0, dv / np.where(v > 0, v, 1.0), 0.0)
    A = np.sqrt(v) / np.sqrt(bc2)
    EA = ev / 2 + (S + E2 / 2 + S + D + 1) * U
    Eden = EA * A / (A + eps) + U
    rel = (E1 + D + 1 + D) * U + Eden
    assert float(np.max(rel, initial=0.0)) < 2.0 ** -11, "adam_bound: a relative error beyond the first-order model"
    step, den = lr / bc1, A + eps
    dupd = np.abs(step * m / den) * rel + dm * step / den
    dp = dupd + U * np.abs(p)
    k = 1.0 + SECOND_ORDER
    return dm * k, dv * k, dp * k


MUTANTS = ("eps_in_sqrt", "clip_uncapped", "clip_dropped", "scale_norm_only", "v_unclipped", "bc_t_minus_1", "no_bc2", "v_not_stored",
           "betas_swapped")


def emulate_fp32(g, m0, v0, p0, total_sumsq, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5, grad_scale=1.0, mutant=None):
    """The kernels' statements one by one in numpy.float32 (no contraction); `mutant`: one of MUTANTS, a subtly wrong kernel."""
    assert mutant is None or mutant in MUTANTS
    F = np.float32
    g, m0, v0, p0 = (np.asarray(x, dtype=F) for x in (g, m0, v0, p0))
    lr, b1, b2, eps, mx, gs = (F(x) for x in (lr, beta1, beta2, eps, max_norm, grad_scale))
    if mutant == "betas_swapped":
        b1, b2 = b2, b1
    one = F(1.0)
    with np.errstate(all="ignore"):
        tn = np.sqrt(F(total_sumsq))
        clip = mx / (tn + F(1e-6)) if mx > 0 else one
        if mutant != "clip_uncapped":
            clip = min(clip, one)
        if mutant == "clip_dropped":
            clip = one
        tt = F(t - 1 if mutant == "bc_t_minus_1" else t)
        bc1, bc2 = one - np.power(b1, tt), one - np.power(b2, tt)
        step, isb2 = lr / bc1, one / np.sqrt(bc2)
        if mutant == "no_bc2":
            isb2 = one
        gh = (g if mutant == "scale_norm_only" else g * gs) * clip
        gv = g * gs if mutant == "v_unclipped" else gh
        m = b1 * m0 + (one - b1) * gh
        v = b2 * v0 + (one - b2) * gv * gv
        if mutant == "eps_in_sqrt":
            den = np.sqrt(v * isb2 * isb2 + eps)
        else:
            den = np.sqrt(v) * isb2 + eps
        p = p0 - step * m / den
    assert m.dtype == v.dtype == p.dtype == F
    return m, (v0.copy() if mutant == "v_not_stored" else v), p


def inside(got, want, bound):
    """max of |got - want| / bound (0 where got == want; inf where a bound of 0 is missed or a value is not finite)."""
    got, want, bound = (np.asarray(x, dtype=np.float64) for x in (got, want, bound))
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(np.max(np.nan_to_num(r, nan=np.inf), initial=0.0))


def pow_allowance_used(got_p, want_p, dp, dp_exact_pow):
    """The largest share of powf's allowance an element needs: (|err| - bound with an exact powf) / (bound - bound with an exact powf),
    0 when every element is inside the bound of an exact powf.  A figure to report, not a check."""
    err = np.abs(np.asarray(got_p, dtype=np.float64) - want_p)
    room = dp - dp_exact_pow
    with np.errstate(all="ignore"):
        used = np.where(room > 0, (err - dp_exact_pow) / room, 0.0)
    return float(max(0.0, np.max(used, initial=0.0)))


# ----------------------------------------------------------------------------------------------------------------------------------
# the state and hyper-parameter table
# ----------------------------------------------------------------------------------------------------------------------------------
# (t, clipping, grad_scale, regime).  clipping: "off" max_norm = 0; "idle" max_norm = 4 x the norm; "active" max_norm = norm / 8.
CASES = [
    (1, "off", 1.0, "ordinary"),
    (1, "active", 0.125, "ordinary"),
    (1, "idle", 1.0, "tiny"),
    (2, "idle", 1.0, "wide"),
    (2, "active", 1.0, "tiny"),
    (10, "active", 1.0, "wide"),
    (10, "idle", 0.125, "tiny"),
    (10, "off", 0.125, "ordinary"),
    (1000, "active", 0.125, "ordinary"),
    (1000, "off", 1.0, "tiny"),
    (1000, "idle", 1.0, "zeros"),
    (100000, "active", 1.0, "ordinary"),
    (100000, "idle", 0.125, "wide"),
    (1, "active", 1.0, "zeros"),
]
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def case_id(row):
    return "t%d-%s-gs%g-%s" % row


def _loguniform(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)


def case_arrays(row, n, seed=0):
    """(g, m0, v0, p0) fp32 of n elements for a row of CASES, and its keyword arguments (total_sumsq, t, max_norm, grad_scale and HYPER).
    total_sumsq is the fp32 rounding of the exact squared norm of grad_scale * g: what a correct norm pass hands the update."""
    t, clipping, gs, regime = row
    rng = np.random.default_rng(1000 * seed + CASES.index(row))
    F = np.float32
    if regime == "ordinary":
        g, m0, v0 = rng.standard_normal(n), 0.3 * rng.standard_normal(n), (0.2 + np.abs(rng.standard_normal(n))) ** 2
    elif regime == "wide":
        g, m0, v0 = _loguniform(rng, n, 1e-6, 1e3), _loguniform(rng, n, 1e-6, 1e3), _loguniform(rng, n, 1e-6, 1e3) ** 2
    elif regime == "tiny":
        g, m0, v0 = _loguniform(rng, n, 1e-10, 1e-6), _loguniform(rng, n, 1e-10, 1e-6), _loguniform(rng, n, 1e-10, 1e-6) ** 2
    else:
        g = m0 = v0 = np.zeros(n)
    g, m0, v0, p0 = g.astype(F), m0.astype(F), v0.astype(F), rng.standard_normal(n).astype(F)
    total = F(f32(gs) ** 2 * float((g.astype(np.float64) ** 2).sum()))
    norm = float(np.sqrt(np.float64(total)))
    max_norm = {"off": 0.0, "idle": 4.0 * norm + 1e-3, "active": norm / 8.0}[clipping]
    if regime == "zeros" and clipping == "active":
        max_norm = 0.5                                      # the norm is 0: the coefficient is 0.5 / 1e-6, capped at 1
    kw = dict(HYPER, total_sumsq=float(total), t=t, max_norm=f32(max_norm), grad_scale=gs)
    return (g, m0, v0, p0), kw


# ----------------------------------------------------------------------------------------------------------------------------------
# drn_adam_bucket: the layout the tests use and the path every block and quad of a layout takes
# ----------------------------------------------------------------------------------------------------------------------------------
def bucket_layout():
    """The flat bucket of the tests: a list of segments dict(name, start, end, kind, addr, mirror) and n.
    kind: "tensor" (a real parameter), "pad" (NULL: alignment padding), "out" (NULL with a real extent: a tensor taken out for
    drn_adam_tiled).  addr: BYTE offset of the parameter inside a 256-byte-aligned arena (gaps between parameters; 0 for NULL);
    mirror: BYTE offset of its bf16 copy inside the mirror arena, or None.  The table's last entry lies beyond n: the last tensor is cut
    by n, not by its extent."""
    segs, addr, maddr = [], [256], [64]

    def add(name, start, end, kind="tensor", misalign=0, mirror=False):
        assert (kind == "pad" or start % 4 == 0) and (not segs or segs[-1]["end"] == start)     # tensors start on a quad (drn_amd.dist)
        s = dict(name=name, start=start, end=end, kind=kind, addr=0, mirror=None)
        if kind == "tensor":
            s["addr"] = addr[0] + misalign
            addr[0] += ((end - start) * 4 + misalign + 255) // 256 * 256 + 256          # a gap of >= 256 bytes behind every parameter
            if mirror:
                s["mirror"] = maddr[0]
                maddr[0] += ((end - start) * 2 + 63) // 64 * 64 + 64
        segs.append(s)

    n = 8 * BLOCK + 1003                                           # 33771: not a multiple of 4
    add("fast2", 0, 2 * BLOCK, mirror=True)                        # blocks 0, 1: the one-tensor fast path, with a mirror
    add("misaligned", 2 * BLOCK, 3 * BLOCK, misalign=4)            # block 2: inside one tensor, pointer 4 bytes off: scalar everywhere
    add("ten", 3 * BLOCK, 3 * BLOCK + 10, mirror=True)             # two quads and a partial one, with a mirror
    add("pad0", 3 * BLOCK + 10, 3 * BLOCK + 12, "pad")
    add("one", 3 * BLOCK + 12, 3 * BLOCK + 13)
    add("pad1", 3 * BLOCK + 13, 3 * BLOCK + 20, "pad")             # holds a whole quad: the `continue` of the quad loop
    add("taken_out", 3 * BLOCK + 20, 5 * BLOCK - 900, "out")       # 7272 elements, NULL: the rest of block 3 and most of block 4
    add("mid", 5 * BLOCK - 900, 5 * BLOCK - 900 + 5002, mirror=True)   # quads in block 4, block 5 fast, a partial last quad in block 6
    add("pad2", 6 * BLOCK + 6, 6 * BLOCK + 8, "pad")
    add("last", 6 * BLOCK + 8, n + 5)                              # quads, block 7 fast WITHOUT a mirror, block 8 cut by n
    return segs, n, addr[0], maddr[0]


def bucket_paths(seg_start, p_addr, n, mirror=None):
    """One record (block, quad, path, seg, has_mirror) per block that takes the fast path (quad = -1) and per quad of the others.
    path: "fast"; "quad" (16-byte loads); "scalar:misaligned", "scalar:tail" (the tensor ends inside the quad), "scalar:n" (the bucket
    does); "null" (NULL pointer: nothing read or written).  seg_start: nseg + 1 offsets; p_addr: byte addresses, 0 = NULL;
    mirror: byte addresses or None.  Mirrors the arithmetic of adam_bucket_kernel."""
    nseg = len(p_addr)
    out = []
    for b in range(nblocks(n)):
        base = b * BLOCK
        seg = max(i for i in range(nseg) if seg_start[i] <= base)
        s0, s1 = seg_start[seg], seg_start[seg + 1]
        if p_addr[seg] and base + BLOCK <= s1 and base + BLOCK <= n and (p_addr[seg] + 4 * (base - s0)) % 16 == 0:
            out.append((b, -1, "fast", seg, bool(mirror and mirror[seg])))
            continue
        for q in range(BLOCK // 4):
            k = base + 4 * q
            if k >= n:
                break
            while k >= seg_start[seg + 1]:
                seg += 1
            s0, s1 = seg_start[seg], seg_start[seg + 1]
            has = bool(mirror and mirror[seg])
            if not p_addr[seg]:
                out.append((b, q, "null", seg, False))
            elif k + 4 <= s1 and k + 4 <= n and (p_addr[seg] + 4 * (k - s0)) % 16 == 0:
                out.append((b, q, "quad", seg, has))
            elif k + 4 > n:
                out.append((b, q, "scalar:n", seg, has))
            elif k + 4 > s1:
                out.append((b, q, "scalar:tail", seg, has))
            else:
                out.append((b, q, "scalar:misaligned", seg, has))
    return out


def blk_seg_table(seg_start, n):
    """FusedAdam's blk_seg: the segment holding the first element of every block."""
    starts = np.asarray(seg_start[:-1], dtype=np.int64)
    return (np.searchsorted(starts, np.arange(nblocks(n), dtype=np.int64) * BLOCK, side="right") - 1).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------------------------
# drn_adam_tiled: the items of the tests and the paths their tiles take
# ----------------------------------------------------------------------------------------------------------------------------------
def tiled_items():
    """dicts(R, C, k, off_mis, p_mis, c1, c2): c1 / c2 = None or (code, ld, misalign bytes) of the [r][tap][c] / [c][tap][r] copy;
    off_mis: the item's offset inside the flat buffers modulo 4; p_mis: byte misalignment of the parameter."""
    I = lambda R, C, k, c1=None, c2=None, off_mis=0, p_mis=0: dict(R=R, C=C, k=k, c1=c1, c2=c2, off_mis=off_mis, p_mis=p_mis)
    return [
        I(130, 72, 3, (BF16, 72, 0), (BF16, 136, 0)),      # 3 x 2 tiles; ld1 = extent; ld2 padded to VEC: the nr = 2 tiles flush by element
        I(65, 136, 1, None, (F32, 65, 0)),                  # m2 only, odd ld; corner tile nr = 1, nc = 8
        I(64, 64, 2, (F32, 64, 0), None),                   # m1 only, one full tile
        I(63, 7, 1, (BF16, 7, 0), (F32, 64, 0)),            # element-wise update (S = 7); both flushes by element
        I(1, 65, 1, (F32, 65, 0), None),                    # 1-D, two tiles, element-wise update
        I(1, 136, 1, (F32, 136, 4), None),                  # 1-D, vec4 update; the copy's base 4 bytes off: flush by element
        I(130, 1, 3, (BF16, 1, 0), (BF16, 136, 0)),         # C = 1: S = 3, one-piece rows
        I(65, 65, 2, (F32, 68, 0), (BF16, 67, 0)),          # 2 x 2 tiles, S = 130: element-wise update; mixed codes; ld1 padded, ld2 odd
        I(64, 72, 1, (BF16, 80, 0), (F32, 64, 0), off_mis=2),   # vec4 shape, but off % 4 = 2
        I(1, 1, 1, (F32, 1, 0), None),                      # every divisor is 1
        I(63, 64, 3, None, (BF16, 63, 0), p_mis=4),         # parameter 4 bytes off
        I(130, 136, 3, (BF16, 136, 0), (BF16, 136, 0)),     # the largest: 3 x 3 tiles, corner nr = 2, nc = 8
        I(64, 136, 2, (F32, 136, 0), (F32, 64, 0)),         # fp32 vector flushes in both orientations
    ]


def tiled_paths(R, C, k, off, p_addr, c1=None, c2=None):
    """One record per tile: dict(tile, nr, nc, update "vec4" | "elem", flush1, flush2 "vec" | "elem" | None).  c1 / c2: None or
    (code, ld, byte address).  Mirrors adam_tiled_kernel and tiled_flush."""
    tiles_c, tiles_r = (C + TILE - 1) // TILE, (R + TILE - 1) // TILE
    S = C * k
    out = []
    for t in range(tiles_r * tiles_c):
        r0, c0 = (t // tiles_c) * TILE, (t % tiles_c) * TILE
        nr, nc = min(TILE, R - r0), min(TILE, C - c0)
        ts = nc * k
        vec4 = ts % 4 == 0 and S % 4 == 0 and p_addr % 16 == 0 and off % 4 == 0
        rec = dict(tile=t, nr=nr, nc=nc, update="vec4" if vec4 else "elem", flush1=None, flush2=None,
                   divisors=set([ts // 4 if vec4 else ts]))
        for which, c, ext in ((1, c1, nc), (2, c2, nr)):
            if c is not None:
                code, ld, addr = c
                V = vec_of(code)
                rec["flush%d" % which] = "vec" if ext % V == 0 and ld % V == 0 and addr % 16 == 0 else "elem"
                rec["divisors"] |= set([(ext + V - 1) // V, k])
        out.append(rec)
    return out
