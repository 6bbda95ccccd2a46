"""fp64 model, data and error bounds for the train-mode BatchNorm kernels (csrc/bn.hip, csrc/bn_merge.h and the statistics part of the
GEMM epilogues), shared by tests/test_bn_rows_cpu.py (which checks this file without a GPU) and tests/test_bn_rows_gpu.py.

Three things live here:

  * forward_ref / backward_ref -- nn.BatchNorm1d (training) + ReLU, the nearest-x2 upsample add and the query gate
    (model/basic_blocks.py:9-31, model/FPN.py:63-68, model/backbone.py:28-30) in float64 on the STORED values;
  * columns / affine / exact_gemm_case -- inputs with the channels a BatchNorm kernel gets wrong first (see KINDS) and GEMM operands
    whose fp32 accumulators are exact whatever the summation order;
  * the error bounds (var_bound and friends), derived below from the unit roundoff and the operation counts, and the launchers'
    threshold arithmetic mirrored in Python so that a test can say which branch its shape takes.

The bounds
----------
u = 2^-24 (fp32 round to nearest), gamma_n = n u / (1 - n u).  A slab is n <= 128 rows of one channel; xmax = max |x| of the channel.

(1) slab sum, fp32, ANY order:  |S~ - S| <= gamma_{n-1} sum|x| <= n * gamma_127 * xmax.
(2) slab mean as the epilogue's second pass uses it, m~ = fl(S~ / n):  |m~ - m| <= gamma_127 xmax + u |m~| <= DELTA := gamma_128 * xmax.
    (The issue's "slab sum error <= 128 u max|x|" is this number: the error of the slab MEAN; of the sum it is n times that.)
(3) centred second pass.  In exact arithmetic sum (x - m~)^2 = M2 + n (m~ - m)^2 (the cross term vanishes: sum (x - m) = 0).  In fp32
    every term carries the subtraction's rounding twice and the square's once, the sum of n terms gamma_{n-1}:
        |M2~ - M2| <= (1 + g) n DELTA^2 + g M2,        g := gamma_{n+2} <= A := gamma_130.
(4) merge (bn_merge_cols: Chan et al. in double; its own rounding, ~1e-16 relative, is covered by rounding A up).  With e_k the error
    of slab k's mean as the MERGE sees it (S~_k / n_k in double: |e_k| <= gamma_127 xmax <= DELTA) and e the n-weighted mean of the e_k
    (= the error of the merged mean), the between-slab term is
        sum n_k (m_k - mu + e_k - e)^2 = B + 2 sum n_k (m_k - mu)(e_k - e) + sum n_k (e_k - e)^2,     B = sum n_k (m_k - mu)^2
    and  sum n_k (e_k - e)^2 <= M DELTA^2,  |cross| <= 2 sqrt(B) sqrt(M) DELTA  (Cauchy-Schwarz).
    Dividing by M, with var = (sum M2_k + B) / M and var_between := B / M <= var:

        |mean~ - mean| <= DELTA
        |var~  - var | <= A var + 2 DELTA sqrt(var_between) + (2 + A) DELTA^2                                   (var_bound)

    This is the issue's  a var + (128 u max|x|)^2  with a = gamma_130 = 7.75e-6 -- set from the arithmetic above before any GPU run --
    plus the cross term, which the derivation does not let go of: it is linear in DELTA, and on the `offset` columns (DELTA = 0.125 std,
    var_between = var / 128) it is as large as the last.  Dropping it would need e_k uncorrelated with m_k - mu, which is a
    statement about the data, not about the arithmetic.  It is computed on the reference side (var_between of the fp64 slab means).
    A naive fp32 sum of squares carries ~u mean^2 instead: at |mean| / std = 16384 that is ~10 var against a bound of ~0.06 var
    (tests/test_bn_rows_cpu.py holds the factor to >= 10).

(5) what follows from (mean~, var~) (bn_scale_shift, bn_running_update: contraction off, so every operation rounds once), dv the
    bound (4), dm = DELTA:
        invstd = fl(1 / sqrt(var + eps)):   relative  r_i  <= dv / (2 (var + eps - dv)) + 2 u
        scale  = fl(gamma invstd):          relative  r_sc <= r_i + 2 u
        save mean = fl(mean):               dm + u |mean|
        shift  = fl(beta - fl(fl(mean) sc)):  |sc| dm + |mean sc| (r_sc + 3 u) + 2 u (|beta| + |mean sc|)
        running_mean: momentum (dm + 2 u (|mean| + |cb|)) + 3 u (|rm| + momentum |mean + cb|)
        running_var:  momentum (dv M/(M-1) + 2 u var_unb) + 3 u (|rv| + momentum var_unb)
(6) apply, y = fl(fma(x, sc, sh)) with the kernel's OWN sc, sh: one rounding, |y - (x sc + sh)| <= u (|x sc| + |sh|); ReLU is exact; the
    upsample add and the gate product round once each.  apply_bound is the issue's 2^-23 k (|x scale| + |shift|) (+ |up|) with k = 2
    -- four roundings' worth for at most three -- plus half an ulp of the output type.
    Against the fp64 scale / shift instead (end to end) the scale's error multiplies x - mean, not x:
        |out~ - out| <= |x - mean| |sc| r_sc + dm |sc| (1 + r_sc) + apply_bound                                 (out_bound)
(7) backward, draw = fma(ka, g, fma(kb, x, kc)), ka = s = gamma istd, kb = -s dg istd / M, kc = -s db / M - kb mean
    (bn_bwd_apply64_kernel and bn_bwd_one_kernel build them the same way, in fp32): kb carries 6 roundings, the `- kb mean` term of kc 7,
    kc's own sum and the two fmas one each.  kb x and kb mean cancel down to kb (x - mean), so the absolute error is set by |kb mean|:
        |draw~ - draw| <= 8 * 2^-23 |kb| max(|x|, |mean|)                    <- the cancellation term, 14 u rounded up to 16 u
                          + 4 * 2^-23 (|ka g| + |s db / M|)
                          + |s istd (x - mean)| d_dg / M + |s| d_db / M      <- dgamma / dbeta as accumulated in fp32 (d_dg, d_db: the suite's
                                                                               3e-5 max(1, sqrt(rows) / 16) formula)
                          + half an ulp of the output type                                                      (draw_bound)
"""
import math

import torch

U = 2.0 ** -24


def gamma_n(n):
    return n * U / (1.0 - n * U)


A_VAR = gamma_n(130)                 # `a` of var_bound: set from the derivation (3)-(4), not from any kernel's output
EPS = 1e-5


def delta_of(xmax):
    """DELTA of (2): the error bound of a slab mean, and of the merged mean."""
    return gamma_n(128) * xmax


def half_ulp(dtype):
    """relative half ulp of the stored type (round to nearest)"""
    return 2.0 ** -8 if dtype == torch.bfloat16 else U


# ---------------------------------------------------------------------------------------------------------------------------------
# the launchers' threshold arithmetic (csrc/bn.hip), mirrored: which branch does a shape take?
# ---------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def _vn(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def rows_per_pass(dtype):
    """RP of the (row block x 64-channel tile) kernels: rows one pass of a 256-thread workgroup covers (16 in fp32, 32 in bf16)."""
    return 256 // (64 // _vn(dtype))


def slabs(M):
    """128-row statistics slabs of M rows; bn_merge_cols keeps a thread's pairs in registers while slabs <= 64."""
    return cdiv(M, 128)


def merge_is_cached(M):
    return slabs(M) <= 64


def train_apply_rows_wg(Ms, C, dtype):
    """drn_bn_train_apply: rows per workgroup; more than 4*RP (= more than one trip of the row loop) only beyond 4096 workgroups."""
    rp4 = 4 * rows_per_pass(dtype)
    wg4 = cdiv(sum(Ms), rp4) * (C // 64)
    return rp4 * (cdiv(wg4, 4096) if wg4 > 4096 else 1)


def bwd64_rrows_arows(Ms, C, dtype):
    """bn_bwd_launch64 (C % 64 == 0, two launches) -> ([(rows per reduce block, reduce blocks, enlarged?) per level], rows per apply block)."""
    rp4 = 4 * rows_per_pass(dtype)
    ctiles = C // 64
    m_all = sum(Ms)
    rrows = cdiv(max(1, cdiv(m_all * ctiles, 512)), rp4) * rp4
    arows = 2 * rp4 if cdiv(m_all, rp4) * ctiles > 4096 else rp4
    out = []
    for M in Ms:
        rr, big = rrows, False
        if cdiv(M, rr) > 64:
            rr, big = cdiv(cdiv(M, 64), rp4) * rp4, True
        out.append((rr, cdiv(M, rr), big))
    return out, arows


def row_grid_blocks(M, nvec):
    """row_grid (drn_bn_apply*, the three-launch backward's apply): -> (blocks, passes of the stride loop, capped?)."""
    unit = nvec // math.gcd(nvec, 256)
    want = max(1, cdiv(M * nvec, 1024))
    capped = want > 4096
    want = min(want, 4096)
    blocks = cdiv(want, unit) * unit
    rstride = blocks * 256 // nvec
    return blocks, cdiv(M, rstride), capped


def bwd_one_fits(Ms, C, dtype, max_wg=512):
    """bn_bwd_one_plan without a gate backward: the one-launch kernel takes the launch when its largest row block (16 passes of RP rows)
    leaves every level at most 64 row blocks and the grid at most bn1_maxwg workgroups (smaller blocks only make more of them)."""
    rows = 16 * rows_per_pass(dtype)
    rb = [cdiv(M, rows) for M in Ms]
    return C % 64 == 0 and max(rb) <= 64 and sum(rb) * (C // 64) <= max_wg


def bwd3_nblk(Ms, C, dtype):
    """bn_bwd_launch, C % 64 != 0 (three launches): partial-sum row blocks per level."""
    cbk = cdiv(C // _vn(dtype), 64)
    m_all = sum(Ms)
    rows_blk = 64 if cbk * (m_all // 64) >= 256 else (32 if cbk * (m_all // 32) >= 256 else 16)
    return [256 if M >= 256 * rows_blk else (M // rows_blk if M >= rows_blk else 1) for M in Ms]


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
# channel (within every 64-channel tile) -> kind.  Everything else is randn * 1.5 + 0.3, the columns the rest of the suite feeds.
KINDS = {"offset": 3, "const": 10, "tiny": 17, "big": 24, "outlier": 31, "relu_off": 38, "relu_on": 45}
CONST_VALUE = 0.7                                    # not a power of two: 128 of them do not sum exactly
# (mean, std).  bf16: |mean| / std = 64 (values 0.5 apart there).  fp32: 16384 -- the naive variance's error grows with the square of
# the ratio, var_bound's cross term only linearly; at 4096 the naive error is only ~9x the bound on some columns, at 16384 it is >= 18x
# on all of tests/test_bn_rows_cpu.py's (the test asks for 10x)
OFFSET = {torch.float32: (12288.0, 0.75), torch.bfloat16: (96.0, 1.5)}
OUTLIER = {torch.float32: 1.0e4, torch.bfloat16: 9984.0}


def kind_index(C, kind):
    """channels of `kind` in a C-channel matrix (one per complete or partial 64-channel tile that reaches it)"""
    return torch.tensor([c for c in range(C) if c % 64 == KINDS[kind]], dtype=torch.long)


def columns(M, C, dtype, seed, ld=None, fill=0.0):
    """raw [M, ld] of `dtype` (CPU): columns past C hold `fill`.  See KINDS; the offset column's sign alternates from tile to tile."""
    ld = C if ld is None else ld
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    for c in range(C):
        k = c % 64
        if k == KINDS["offset"]:
            mean, std = OFFSET[dtype]
            sign = -1.0 if (c // 64) % 2 else 1.0
            x[:, c] = sign * (mean + std * torch.randn(M, generator=g))
        elif k == KINDS["const"]:
            x[:, c] = CONST_VALUE
        elif k == KINDS["tiny"]:
            x[:, c] = 1e-4 * torch.randn(M, generator=g)
        elif k == KINDS["big"]:
            x[:, c] = 1e3 * torch.randn(M, generator=g)
        elif k == KINDS["outlier"]:
            x[:, c] = torch.randn(M, generator=g)
            x[M - 1, c] = OUTLIER[dtype]                          # the last row: inside the ragged slab / row block
        elif k in (KINDS["relu_off"], KINDS["relu_on"]):
            x[:, c] = torch.randn(M, generator=g)
    out = torch.full((M, ld), fill, dtype=dtype)
    out[:, :C] = x.to(dtype)
    return out


def affine(C, seed):
    """(gamma, beta) fp32: as the suite draws them, except on the ReLU columns: gamma = 0.75, beta = -/+ 64, so that no / every element
    passes the ReLU whatever the normalised value (|xhat| <= sqrt(M) is the only limit; the tests assert it on the reference)."""
    g = torch.Generator().manual_seed(seed)
    gamma = torch.randn(C, generator=g) * 0.3 + 1.0
    beta = torch.randn(C, generator=g) * 0.2
    for c in range(C):
        if c % 64 == KINDS["relu_off"]:
            gamma[c], beta[c] = 0.75, -64.0
        elif c % 64 == KINDS["relu_on"]:
            gamma[c], beta[c] = 0.75, 64.0
    return gamma, beta


def exact_gemm_case(M, Cin, N, taps=1, L=None, seed=0):
    """-> (A [M, Cin], W [N, taps*Cin]) in bfloat16 and the exact product P [M, N] in float64 (a k = `taps`, stride 1, zero-padded
    convolution over sequences of L rows when taps == 3, tap-major weights as drn_gemm_nt takes them).

    Every product a*w and every partial sum of an output column, in ANY order, is exactly representable in fp32, so the fp32
    accumulators of a GEMM kernel equal P bit for bit and any error in the (sum, M2) pairs belongs to the statistics passes alone:
      A: channel 0 = 2.375; channel 1 = k 2^-14, |k| <= 3 (std ~1e-4); channel 2 = k / 8, |k| <= 16; channel 3 = the same with 9984 in
         the last row; channels 4.. = 16 + k / 8, 0 <= k < 8           -- all at most 8 significant bits;
      W: output column n, by n % 64 (centre tap only, so that sequence edges do not touch them): `offset` = 1 on channels 4.. (mean ~
         16.4 (Cin - 4), std ~ 0.29 sqrt(Cin - 4): 980 and 2.2 at Cin = 64), `const` = 1 on channel 0, `tiny` = 1 on channel 1, `big` =
         1024 on channel 2, `outlier` = 1 on channel 3, `relu_off` = all zero (a zero column); every other column draws {-1, 0, 1} on
         channels 0, 2, 4.. of every tap.
    Exactness is asserted here: per column, sum_c |w| max|a_c| < 2^24 quanta of the column's finest term."""
    assert Cin >= 8 and taps in (1, 3)
    L = M if L is None else L
    assert M % L == 0
    g = torch.Generator().manual_seed(seed)
    A = 16.0 + torch.randint(0, 8, (M, Cin), generator=g).double() / 8.0
    A[:, 0] = 2.375
    A[:, 1] = torch.randint(-3, 4, (M,), generator=g).double() * 2.0 ** -14
    A[:, 2] = torch.randint(-16, 17, (M,), generator=g).double() / 8.0
    A[:, 3] = torch.randint(-16, 17, (M,), generator=g).double() / 8.0
    A[M - 1, 3] = 9984.0
    quantum = torch.full((Cin,), 1.0 / 8.0, dtype=torch.float64)
    quantum[1] = 2.0 ** -14
    W = torch.randint(-1, 2, (N, taps, Cin), generator=g).double()
    W[:, :, 1] = 0.0
    W[:, :, 3] = 0.0
    mid = taps // 2
    for n in range(N):
        k = n % 64
        special = {KINDS["offset"]: (slice(4, Cin), 1.0), KINDS["const"]: (0, 1.0), KINDS["tiny"]: (1, 1.0), KINDS["big"]: (2, 1024.0),
                   KINDS["outlier"]: (3, 1.0), KINDS["relu_off"]: (0, 0.0)}.get(k)
        if special is not None:
            W[n] = 0.0
            W[n, mid, special[0]] = special[1]
    # exactness: terms of column n are multiples of q_n = min over its channels of quantum_c (the weights are integers)
    amax = A.abs().max(0).values
    wabs = W.abs().sum(1)                                                  # [N, Cin]: the taps see the same channel
    used = wabs > 0
    q = torch.where(used, quantum[None, :], torch.full_like(wabs, float("inf"))).min(1).values
    total = (wabs * amax[None, :]).sum(1)
    assert bool((total[torch.isfinite(q)] < 2.0 ** 24 * q[torch.isfinite(q)]).all()), "a partial sum may need more than 24 bits"
    Ab, Wb = A.to(torch.bfloat16), W.reshape(N, taps * Cin).to(torch.bfloat16)
    assert torch.equal(Ab.double(), A) and torch.equal(Wb.double().reshape(N, taps, Cin), W), "operands must be exact in bf16"
    return Ab, Wb, exact_product(A, W, L)


def exact_product(A, W, L):
    """float64 product of exact_gemm_case: P[b, t] = sum_j A[b, t + j - taps // 2] W[:, j]^T with zero rows outside the sequence."""
    M, Cin = A.shape
    N, taps, _ = W.shape
    x = A.reshape(M // L, L, Cin)
    P = torch.zeros(M // L, L, N, dtype=torch.float64)
    for j in range(taps):
        s = j - taps // 2
        sh = torch.zeros_like(x)
        if s == 0:
            sh = x
        elif s < 0:
            sh[:, -s:] = x[:, :L + s]
        else:
            sh[:, :L - s] = x[:, s:]
        P += sh @ W[:, j].t()
    return P.reshape(M, N)


# ---------------------------------------------------------------------------------------------------------------------------------
# the slab statistics: exact, and as a GEMM epilogue leaves them
# ---------------------------------------------------------------------------------------------------------------------------------
def _slab_view(x):
    """[M, C] -> ([K-1 or K, 128, C] full slabs, [n_last, C] ragged last slab or None)"""
    M = x.shape[0]
    full = M // 128
    return x[:full * 128].reshape(full, 128, x.shape[1]), (x[full * 128:] if M % 128 else None)


def slab_stats_fp32(x):
    """[slabs, 2, C] fp32 (sum, M2) per 128-row slab of x (any float type; the arithmetic is fp32): the slab scheme of the GEMM
    epilogues -- fp32 sum, fp32 mean, a centred fp32 second pass.  Runs where x lives; row after row with elementwise fp32
    operations (one fixed order everywhere, and the order with the largest rounding error: the bounds hold for any)."""
    xf = x.float()
    a, b = _slab_view(xf)
    parts = []
    for blk in ([a] if b is None else [a, b[None]]):
        if blk.shape[0] == 0:
            continue
        s = torch.zeros_like(blk[:, 0])
        for i in range(blk.shape[1]):
            s = s + blk[:, i]
        m = s / float(blk.shape[1])
        q = torch.zeros_like(s)
        for i in range(blk.shape[1]):
            d = blk[:, i] - m
            q = q + d * d
        parts.append(torch.stack([s, q], 1))
    return torch.cat(parts).contiguous()


def slab_stats_naive_fp32(x):
    """[slabs, 2, C] fp32 (sum, sum of squares): what an epilogue WITHOUT the centred pass would write.  Row after row with
    elementwise fp32 operations, so that the result does not depend on how a library orders its reductions."""
    xf = x.float()
    a, b = _slab_view(xf)
    parts = []
    for blk in ([a] if b is None else [a, b[None]]):
        if blk.shape[0] == 0:
            continue
        s, q = torch.zeros_like(blk[:, 0]), torch.zeros_like(blk[:, 0])
        for i in range(blk.shape[1]):
            s = s + blk[:, i]
            q = q + blk[:, i] * blk[:, i]
        parts.append(torch.stack([s, q], 1))
    return torch.cat(parts).contiguous()


def merge_slabs(stats, M):
    """bn_merge_cols in float64, statement for statement: four slab lanes (slab k -> lane k % 4) added as (0 + 1) + (2 + 3), the slab
    mean as sum * 2^-7 (or / n_last for the ragged last slab), var clamped at 0.  -> (mean, biased var)"""
    st = stats.double()
    K = st.shape[0]
    assert K == slabs(M)
    n_last = M - (K - 1) * 128
    inv_m = 1.0 / M

    def lanes(v):                                   # v [K, C] -> fixed-order sum
        acc = [torch.zeros_like(v[0]) for _ in range(4)]
        for k in range(K):
            acc[k % 4] = acc[k % 4] + v[k]
        return (acc[0] + acc[1]) + (acc[2] + acc[3])
    mean = lanes(st[:, 0]) * inv_m
    n = torch.full((K, 1), 128.0, dtype=torch.float64, device=st.device)
    inv = torch.full((K, 1), 0.0078125, dtype=torch.float64, device=st.device)
    n[K - 1] = float(n_last)
    inv[K - 1] = 0.0078125 if n_last == 128 else 1.0 / n_last
    d = st[:, 0] * inv - mean
    var = lanes(st[:, 1] + n * d * d) * inv_m
    return mean, var.clamp_min(0.0)


def merge_naive(stats, M):
    """E[x^2] - E[x]^2 from naive slab pairs, merged in float64"""
    st = stats.double()
    mean = st[:, 0].sum(0) / M
    return mean, (st[:, 1].sum(0) / M - mean * mean).clamp_min(0.0)


def exact_stats(x):
    """float64 (mean, biased var, var_between, xmax) of the columns of x: var_between = sum n_k (m_k - mean)^2 / M over the 128-row slabs."""
    xd = x.double()
    M = xd.shape[0]
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    a, b = _slab_view(xd)
    B = (128.0 * (a.mean(1) - mean) ** 2).sum(0)
    if b is not None:
        B = B + b.shape[0] * (b.mean(0) - mean) ** 2
    return mean, var, B / M, xd.abs().max(0).values


def slab_bounds(x):
    """per slab and channel, from the exact values: (exact sum, bound of |sum~ - sum|, exact M2, bound of |M2~ - M2|)  -- (1) and (3)"""
    xd = x.double()
    a, b = _slab_view(xd)
    xmax = xd.abs().max(0).values
    out = []
    for blk in ([a] if b is None else [a, b[None]]):
        if blk.shape[0] == 0:
            continue
        n = blk.shape[1]
        s = blk.sum(1)
        m2 = ((blk - s[:, None] / n) ** 2).sum(1)
        d = delta_of(xmax)
        out.append((s, (n * gamma_n(127) * xmax).expand_as(s), m2, (1 + A_VAR) * n * d * d + A_VAR * m2))
    return tuple(torch.cat([o[i] for o in out]) for i in range(4))


def var_bound(var, var_between, xmax):
    """(4): |var~ - var| <= A var + 2 DELTA sqrt(var_between) + (2 + A) DELTA^2"""
    d = delta_of(xmax)
    return A_VAR * var + 2.0 * d * torch.sqrt(var_between) + (2.0 + A_VAR) * d * d


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def upsample2(up, B, L):
    """nearest x2 along the sequence: up [B * L/2, C] -> [B * L, C]"""
    C = up.shape[1]
    return up.reshape(B, L // 2, C).repeat_interleave(2, dim=1).reshape(B * L, C)


def forward_ref(raw, gamma, beta, eps, conv_bias, running_mean, running_var, momentum, relu, up=None, gate=None, L=None,
                scale_shift=None, stats_of=None):
    """Train-mode BatchNorm (+ReLU, + nearest-x2 upsample add, * query gate) in float64 on the stored `raw` [M, C].
    stats_of: the matrix the statistics are OF when that is not the stored one (the GEMM's unrounded accumulators);
    scale_shift = (scale, shift): normalise with these (the kernel's own fp32 values) instead of the model's.
    -> dict(mean, var (biased), var_between, xmax, invstd, scale, shift, running_mean, running_var, y (before the add), out, gated)"""
    x = raw.double()
    M, C = x.shape
    L = M if L is None else L
    mean, var, varb, xmax = exact_stats(x if stats_of is None else stats_of)
    invstd = 1.0 / torch.sqrt(var + eps)
    g, b = gamma.double(), beta.double()
    scale, shift = g * invstd, b - mean * g * invstd
    r = dict(mean=mean, var=var, var_between=varb, xmax=xmax, invstd=invstd, scale=scale, shift=shift)
    cb = conv_bias.double() if conv_bias is not None else torch.zeros_like(mean)
    unb = var * (M / (M - 1.0)) if M > 1 else var
    if running_mean is not None:
        r["running_mean"] = (1.0 - momentum) * running_mean.double() + momentum * (mean + cb)
        r["running_var"] = (1.0 - momentum) * running_var.double() + momentum * unb
    sc, sh = (scale, shift) if scale_shift is None else (scale_shift[0].double(), scale_shift[1].double())
    y = x * sc + sh
    if relu:
        y = y.clamp_min(0.0)
    out = y if up is None else y + upsample2(up.double(), M // L, L)
    r.update(y=y, out=out, apply_scale=sc, apply_shift=sh)
    if gate is not None:
        r["gated"] = out * gate.double().repeat_interleave(L, dim=0)
    return r


def stat_bounds(r, gamma, beta, eps, M, conv_bias=None, running_mean=None, running_var=None, momentum=0.1):
    """(5): bounds of |kernel - forward_ref| for save (mean, invstd), ss (scale, shift) and the running statistics, per channel."""
    mean, var = r["mean"], r["var"]
    dm = delta_of(r["xmax"])
    dv = var_bound(var, r["var_between"], r["xmax"])
    assert bool((dv < 0.5 * (var + eps)).all()), "the first-order bound of invstd needs dv << var + eps"
    r_i = dv / (2.0 * (var + eps - dv)) + 2 * U
    r_sc = r_i + 2 * U
    g, b = gamma.double(), beta.double()
    sc = r["scale"].abs()
    ms = (mean * r["scale"]).abs()
    out = dict(mean=dm + U * mean.abs(), invstd=r["invstd"] * r_i, scale=sc * r_sc,
               shift=sc * dm * (1 + r_sc) + ms * (r_sc + 3 * U) + 2 * U * (b.abs() + ms), var=dv, r_sc=r_sc, dm=dm)
    if running_mean is not None:
        cb = conv_bias.double().abs() if conv_bias is not None else torch.zeros_like(mean)
        unb = var * (M / (M - 1.0)) if M > 1 else var
        out["running_mean"] = momentum * (dm + 2 * U * (mean.abs() + cb)) + 3 * U * (running_mean.double().abs() + momentum * (mean.abs() + cb))
        out["running_var"] = momentum * (dv * (M / (M - 1.0)) + 2 * U * unb) + 3 * U * (running_var.double().abs() + momentum * unb)
    return out


def apply_bound(x, sc, sh, ref, dtype, up=None, gate=None, k=2.0):
    """(6): |kernel out - fp64(x sc + sh ...)| for the kernel's own sc / sh: 2^-23 k (|x sc| + |sh| + |up|) + half an ulp of `dtype`;
    with a gate, that times |gate| plus the product's rounding."""
    mag = (x.double() * sc.double()).abs() + sh.double().abs()
    if up is not None:
        mag = mag + up.double().abs()
    b = 2.0 ** -23 * k * mag
    if gate is not None:
        b = b * gate.double().abs() + U * ref.abs()
    return b + half_ulp(dtype) * (ref.abs() + b)


def out_bound(r, sb, x, dtype, up=None, gate=None):
    """(6), end to end: |kernel out - forward_ref out| with the model's fp64 scale / shift."""
    xd = x.double()
    sc = r["scale"].abs()
    b = (xd - r["mean"]).abs() * sc * sb["r_sc"] + sb["dm"] * sc * (1 + sb["r_sc"])
    ref = r["out"] if gate is None else r["gated"]
    if gate is not None:
        b = b * gate.double().abs()
    return b + apply_bound(xd, r["scale"], r["shift"], ref, dtype, up=up, gate=gate)


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def backward_ref(lv, C, relu, shared):
    """fp64 BatchNorm(train)+ReLU backward from the values the kernels read (rounded inputs, the fp32 scale_shift and save): the
    `_expected` of tests/test_bn_bwd_one_gpu.py, so that a check isolates the kernel's arithmetic.  -> (draws, dgammas, dbetas)"""
    from test_bn_bwd_one_gpu import _expected
    return _expected(lv, C, relu, shared)


def sum_tol(rows):
    """the suite's tolerance of an fp32 column sum over `rows` rows, relative to max(1, max |sum|) (tests/test_bn_bwd_one_gpu.py)"""
    return 3e-5 * max(1.0, rows ** 0.5 / 16)


def draw_bound(v, C, relu, dg, db, rows, dtype):
    """(7), per element [M, C], for one level dict (raw, dout, ss, save, gamma as the kernels read them); dg, db: the level's fp64 sums."""
    x = v["raw"][:, :C].double()
    g = v["dout"][:, :C].double()
    sc, sh = v["ss"][:C].double(), v["ss"][C:].double()
    mean, istd = v["save"][:C].double(), v["save"][C:].double()
    if relu:
        g = torch.where(torch.addcmul(sh, x, sc) > 0, g, torch.zeros_like(g))
    M = x.shape[0]
    s = v["gamma"].double() * istd
    kb = (s * dg * istd / M).abs()
    d_dg = sum_tol(rows) * max(1.0, float(dg.abs().max()))
    d_db = sum_tol(rows) * max(1.0, float(db.abs().max()))
    ref = s * (g - db / M - (x - mean) * istd * dg / M)
    b = (8 * 2.0 ** -23 * kb * torch.maximum(x.abs(), mean.abs()) + 4 * 2.0 ** -23 * ((s * g).abs() + (s * db / M).abs())
         + (s * istd * (x - mean)).abs() * d_dg / M + s.abs() * d_db / M)
    return b + half_ulp(dtype) * (ref.abs() + b)
