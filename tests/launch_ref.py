"""float64 model of the GEMM launch contracts of include/drn_hip.h, and a comparator with per-element error bounds.

Every function takes the tensors a launch descriptor was made from (any device, any float dtype; 2-D operands may be views
with row strides wider than their data, as the descriptors' lda / ldb / ldc allow) and computes in float64 with indexing and
torch.matmul only: a convolution is a sum of per-tap shifted matmuls, no conv library.  Alongside every value r the model
returns s = sum |a * b| over the same reduction (plus |bias|, times |gate|), computed by the same matmuls on |A'| and |B|.

Given the exact operands a kernel read, its output is fixed up to fp32 accumulation error and one final rounding, so

    |got - r| <= u |r| + kappa * 2^-24 * sqrt(K) * s              (u = 2^-8 bf16 outputs, 2^-23 fp32 outputs; K = reduction length)

with 2u where a value is rounded twice.  Reductions over output rows (BatchNorm slab statistics, the gate-backward column
sums, the per-tile squared sums) combine their rows' bounds as a root-sum-square and add the reduction's own fp32 term; sums of
values rounded to bf16 first (the gate-backward sums) add a linear term for the rows whose rounding may legitimately differ.
"""
import math

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -23
EPS24 = 2.0 ** -24
# kappa = 8: the default of the contract.  It may be raised to at most 16, and only with the measured reason written here.
KAPPA = 8.0
REL_L2 = {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-5}


def unit(dtype):
    return U_BF16 if dtype == torch.bfloat16 else U_F32


def round_to(x, dtype):
    """x (float64) rounded the way a kernel rounds its fp32 value to the output dtype (fp32 first, then the dtype)."""
    return x.float().to(dtype).double()


# ---------------------------------------------------------------------------------------------------------------------
# addressing
# ---------------------------------------------------------------------------------------------------------------------
def src_rows(M, Lout, Lsrc, stride, pad, tap, mode, device):
    """Source row of every output row m for one tap, and whether it is in range (include/drn_hip.h, DrnGemmDesc):
    mode 0: A[seq*Lsrc + t*stride + tap - pad], mode 1: A[seq*Lsrc + (t + pad - tap)/stride] when divisible and in range."""
    m = torch.arange(M, device=device)
    seq, t = m // Lout, m % Lout
    if mode == 0:
        src = t * stride + tap - pad
        ok = (src >= 0) & (src < Lsrc)
    else:
        num = t + pad - tap
        ok = (num >= 0) & (num % stride == 0) & (num // stride < Lsrc)
        src = num // stride
    row = seq * Lsrc + src.clamp(0, Lsrc - 1)
    return row, ok


def tap_operand(A, M, Cin, Lout, Lsrc, stride, pad, tap, mode):
    """The (M, Cin) float64 block of the im2col view A' that multiplies tap `tap` of B; out-of-range taps read zero."""
    row, ok = src_rows(M, Lout, Lsrc, stride, pad, tap, mode, A.device)
    a = A[:, :Cin][row].double()
    return a * ok.unsqueeze(1).double()


def _product(A, Bm, M, N, Cin, taps, stride, pad, mode, Lout, Lsrc):
    """r = A' B^T and s = |A'| |B|^T, both (M, N) float64."""
    r = torch.zeros((M, N), dtype=torch.float64, device=A.device)
    s = torch.zeros_like(r)
    for tap in range(taps):
        a = tap_operand(A, M, Cin, Lout, Lsrc, stride, pad, tap, mode)
        b = Bm[:N, tap * Cin:(tap + 1) * Cin].double()
        r += a @ b.t()
        s += a.abs() @ b.abs().t()
    return r, s


# ---------------------------------------------------------------------------------------------------------------------
# expected outputs
# ---------------------------------------------------------------------------------------------------------------------
class Expect(object):
    """One output of a launch: the float64 reference, the per-element bound, the relative-L2 limit and a locator that names an
    element (row -> clip / t, column -> tap / channel)."""

    def __init__(self, name, ref, bound, rel_l2, where=None):
        self.name, self.ref, self.bound, self.rel_l2, self.where = name, ref, bound, rel_l2, where


def elem_bound(r, s, K, u, kappa=KAPPA):
    return u * r.abs() + kappa * EPS24 * math.sqrt(max(K, 1)) * s


def _rss(x, dim):
    return x.pow(2).sum(dim).sqrt()


def loc_rows(Lout, col_name="n", taps=None, Cin=None):
    """Locator for an (M, N) output: row m = (clip m // Lout, t m % Lout); column as is, or (tap, channel) when taps/Cin given."""
    def where(idx):
        m, n = idx
        col = "%s=%d" % (col_name, n) if taps is None else "col %d (tap %d, c %d)" % (n, n // Cin, n % Cin)
        return "row %d (clip %d, t %d), %s" % (m, m // Lout, m % Lout, col)
    return where


def gemm_nt_ref(A, B, M, N, Cin, taps=1, stride=1, pad=0, mode=0, Lout=None, Lsrc=None, bias=None, gate=None, C_old=None,
                out_dtype=torch.bfloat16, C2=False, stats=False, sumsq=False, gb_act=None, kappa=KAPPA):
    """Reference of one DrnGemmDesc problem.  A: (rows, >= Cin) source (row stride = lda), B: (N, >= taps*Cin), bias (N,),
    gate (M / Lout, >= N) (row stride = ldg), C_old: C before an accumulating launch.  out_dtype: the dtype of C (float32 for
    out_f32).  Flags: C2 / stats / sumsq outputs wanted; gb_act: the gate-backward epilogue (C not written).
    -> {name: Expect} for C, C2, stats, sumsq, gb_dct, gb_dgate, gb_dsum (what applies)."""
    Lout = M if Lout is None else Lout
    Lsrc = Lout if Lsrc is None else Lsrc
    K = taps * Cin
    u = unit(out_dtype)
    tol = REL_L2[out_dtype]
    acc, s_acc = _product(A, B, M, N, Cin, taps, stride, pad, mode, Lout, Lsrc)
    e_acc = kappa * EPS24 * math.sqrt(K) * s_acc          # bound on the fp32 accumulator before any rounding
    where = loc_rows(Lout)
    out = {}
    v, s_v = acc, s_acc
    if bias is not None:
        b = bias[:N].double()
        v, s_v = acc + b, s_acc + b.abs()
    g = None
    if gate is not None:
        g = gate[:, :N].double().repeat_interleave(Lout, dim=0)[:M]
    if gb_act is not None:
        # C is not written: with g = the product rounded to the dtype, dct[c][m] = dtype(g * gate), dgate = sum_t g * act,
        # dsum = sum_t g * gate (per clip)
        nseq = M // Lout
        gr = round_to(v, out_dtype)
        dct = v * g
        out["gb_dct"] = Expect("gb_dct", dct.t(), (2 * u * dct.abs() + e_acc * g.abs()).t(), 2 * tol,
                               lambda idx: "c=%d, row %d (clip %d, t %d)" % (idx[0], idx[1], idx[1] // Lout, idx[1] % Lout))
        # a row's rounded value can differ from the reference's rounding only where the accumulator bound reaches across a
        # rounding midpoint: d = the largest such move of g (one bf16 ulp, on the few rows whose bound straddles a midpoint).
        # These moves are discrete and rare, so their sum is bounded linearly -- a root-sum-square of them left the measured
        # launches no room (conv0's data gradient at T = 256 reached 0.93 of it) -- and so is the relative L2 error: a legitimate
        # flip moves one term by a bf16 ulp, which the fp32 limit (1e-5) does not admit (measured 1.7e-5), hence 2^-8.
        d = torch.maximum((round_to(v + e_acc, out_dtype) - gr).abs(), (round_to(v - e_acc, out_dtype) - gr).abs())
        act = gb_act[:M, :N].double()
        for name, w in (("gb_dgate", act), ("gb_dsum", g)):
            prod = gr * w
            ref = prod.view(nseq, Lout, N).sum(1)
            red = kappa * EPS24 * math.sqrt(Lout) * prod.abs().view(nseq, Lout, N).sum(1)
            bound = (d * w.abs()).view(nseq, Lout, N).sum(1) + red + U_F32 * ref.abs()
            out[name] = Expect(name, ref, bound, U_BF16, lambda idx: "clip %d, c=%d" % idx)
        return out
    if C2:
        out["C2"] = Expect("C2", v, elem_bound(v, s_v, K, u, kappa), tol, where)
    r, s = v, s_v
    if g is not None:
        r, s = v * g, s_v * g.abs()
    if C_old is not None:
        c = C_old[:M, :N].double()
        r, s = r + c, s + c.abs()
    out["C"] = Expect("C", r, elem_bound(r, s, K, u, kappa), tol, where)
    if stats:
        # per-128-row slab (sum, M2) of the raw fp32 accumulators (gemm_nt_kernel.h nt_bn_stats), short last slab
        nsl = (M + 127) // 128
        ref = torch.zeros((nsl, 2, N), dtype=torch.float64, device=A.device)
        bound = torch.zeros_like(ref)
        for j in range(nsl):
            x, e = acc[128 * j:128 * (j + 1)], e_acc[128 * j:128 * (j + 1)]
            R = x.shape[0]
            mean = x.mean(0)
            dev = x - mean
            m2 = dev.pow(2).sum(0)
            ref[j, 0], ref[j, 1] = x.sum(0), m2
            red = kappa * EPS24 * math.sqrt(R)
            bound[j, 0] = _rss(e, 0) + red * x.abs().sum(0) + U_F32 * x.sum(0).abs()
            bound[j, 1] = _rss(2 * dev.abs() * e, 0) + R * e.pow(2).mean(0) + red * m2 + U_F32 * m2
        out["stats"] = Expect("stats", ref, bound, 1e-5,
                              lambda idx: "slab %d (rows %d..%d), %s, n=%d" % (idx[0], 128 * idx[0], min(M, 128 * idx[0] + 128) - 1,
                                                                                 "sum" if idx[1] == 0 else "M2", idx[2]))
    if sumsq:
        tm, tn = M // 256, N // 256
        order = w4_block_tiles(M, N)
        sq = r.pow(2).view(tm, 256, tn, 256)
        ref_t = sq.sum((1, 3))
        eb = elem_bound(r, s, K, U_F32, kappa)
        bnd_t = _rss((2 * r.abs() * eb).view(tm, 256, tn, 256), (1, 3)) + kappa * EPS24 * 256 * ref_t + U_F32 * ref_t
        idx = torch.tensor([a * tn + b for a, b in order], device=A.device)
        out["sumsq"] = Expect("sumsq", ref_t.reshape(-1)[idx], bnd_t.reshape(-1)[idx], 1e-5,
                              lambda i: "block %d = tile (rows %d.., cols %d..)" % (i[0], 256 * order[i[0]][0], 256 * order[i[0]][1]))
    return out


def w4_block_tiles(M, N, swizzle=3):
    """(tile row, tile column) of every workgroup of a single-problem 256x256-tile launch, in launch (blockIdx) order: the
    library's default order (gemm_nt_kernel.h: bit 0 XCD-contiguous runs, bit 1 eight tile rows down a column first).
    DrnGemmDesc::sumsq holds one value per workgroup in this order."""
    tiles_m, tiles_n = M // 256, N // 256
    nb = tiles_m * tiles_n
    res = []
    for bid in range(nb):
        b = bid
        if swizzle:
            q, rr, xcd, j = nb >> 3, nb & 7, bid & 7, bid >> 3
            b = (xcd * (q + 1) if xcd < rr else rr * (q + 1) + (xcd - rr) * q) + j
        tm, tn = b // tiles_n, b % tiles_n
        if swizzle & 2:
            per = 8 * tiles_n
            gid = b // per
            first = gid * 8
            gsm = min(tiles_m - first, 8)
            rem = b - gid * per
            tm, tn = first + rem % gsm, rem // gsm
        res.append((tm, tn))
    return res


def wgrad_ref(problems, N, Cin, taps=1, stride=1, pad=0, w_layout=0, dW_old=None, kappa=KAPPA):
    """dW[n][tap][c] = sum over the problems' rows of dY[m][n] * X[src(m, tap)][c] (mode-0 addressing of X); problems: list of
    dict(dY (M, >= N), X (rows, >= Cin), M, Lout, Lsrc).  Every problem accumulates into the one dW (drn_gemm_wgrad groups).
    -> Expect of dW in layout 0 ([N][taps][Cin]) or 1 ([N][Cin][taps]), fp32."""
    dev = problems[0]["dY"].device
    r = torch.zeros((N, taps, Cin), dtype=torch.float64, device=dev)
    s = torch.zeros_like(r)
    K = 0
    for p in problems:
        M = p["M"]
        dy = p["dY"][:M, :N].double()
        for tap in range(taps):
            x = tap_operand(p["X"], M, Cin, p["Lout"], p["Lsrc"], stride, pad, tap, 0)
            r[:, tap] += dy.t() @ x
            s[:, tap] += dy.abs().t() @ x.abs()
        K += M
    if w_layout == 1:
        r, s = r.transpose(1, 2).contiguous(), s.transpose(1, 2).contiguous()
    if dW_old is not None:
        old = dW_old.double().reshape(r.shape)
        r, s = r + old, s + old.abs()
    if w_layout == 1:
        where = lambda i: "n=%d, c=%d, tap %d" % i
    else:
        where = lambda i: "n=%d, tap %d, c=%d" % i
    return Expect("dW", r, elem_bound(r, s, K, U_F32, kappa), REL_L2[torch.float32], where)


def skinny_ref(X, W, bias=None, mask=None, relu=False, kappa=KAPPA):
    """drn_skinny_group: Y = X W^T (+ bias)(ReLU)(0 where mask <= 0); bf16 rows X: W rounded to bf16 as well."""
    x = X.double()
    w = W.double() if X.dtype != torch.bfloat16 else W.to(torch.bfloat16).double()
    r, s = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        r, s = r + bias.double(), s + bias.double().abs()
    if relu:
        r = r.clamp_min(0)
    if mask is not None:
        keep = (mask[:, :r.shape[1]] > 0).double()
        r, s = r * keep, s * keep
    return Expect("Y", r, elem_bound(r, s, X.shape[1], U_F32, kappa), REL_L2[torch.float32], lambda i: "m=%d, n=%d" % i)


def outer_ref(dY, X=None, lowp=False, kappa=KAPPA):
    """drn_outer_wgrad: dW = dY^T X (lowp: both operands rounded to bf16 first), db = column sums of dY (exact fp32 sums)."""
    M = dY.shape[0]
    out = {}
    if X is not None:
        dy, x = dY.double(), X.double()
        if lowp:
            dy, x = dY.to(torch.bfloat16).double(), X.to(torch.bfloat16).double()
        r, s = dy.t() @ x, dy.abs().t() @ x.abs()
        out["dW"] = Expect("dW", r, elem_bound(r, s, M, U_F32, kappa), REL_L2[torch.float32], lambda i: "n=%d, k=%d" % i)
    d = dY.double()
    r, s = d.sum(0), d.abs().sum(0)
    out["db"] = Expect("db", r, elem_bound(r, s, M, U_F32, kappa), REL_L2[torch.float32], lambda i: "n=%d" % i)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------------------------------
class LaunchMismatch(AssertionError):
    pass


def compare(tag, expect, got):
    """Check one output against its Expect: every element finite and within its bound, relative L2 error within the limit.
    -> (max err / bound, rel-L2).  Raises LaunchMismatch naming the launch, the worst element, got, ref and bound."""
    ref, bound = expect.ref, expect.bound
    g = got.double().reshape(ref.shape)
    finite = torch.isfinite(g)
    err = (g - ref).abs()
    err = torch.where(finite, err, torch.full_like(err, float("inf")))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    worst = int(ratio.reshape(-1).argmax())
    mx = float(ratio.reshape(-1)[worst])
    nref = float(ref.norm())
    diff = torch.where(finite, g - ref, torch.zeros_like(g))
    rel = float(diff.norm()) / nref if nref > 0 else float(diff.norm())
    nonfinite = int((~finite).sum())
    if nonfinite or mx > 1.0 or rel > expect.rel_l2:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ref.shape))
        at = expect.where(idx) if expect.where is not None else str(idx)
        raise LaunchMismatch("%s: %s: %d non-finite, max err/bound %.3g, rel-L2 %.3g (limit %.3g); worst at %s: got %r ref %r bound %.3g"
                             % (tag, expect.name, nonfinite, mx, rel, expect.rel_l2, at, float(g.reshape(-1)[worst]),
                                float(ref.reshape(-1)[worst]), float(bound.reshape(-1)[worst])))
    return mx, rel


def compare_all(tag, expects, gots):
    """expects / gots: {name: ...}.  -> (worst err/bound, worst rel-L2) over the outputs."""
    mx = rel = 0.0
    for name, e in expects.items():
        a, b = compare(tag, e, gots[name])
        mx, rel = max(mx, a), max(rel, b)
    return mx, rel
