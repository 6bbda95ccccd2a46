"""tests/launch_ref.py -- the float64 model of the GEMM launch contracts and its comparator -- on the CPU: the model agrees with
torch's own convolution / linear / autograd, the comparator accepts a legitimate fp32 implementation that sums in another order,
and it rejects the kinds of kernel fault a loose whole-model tolerance would let through."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import launch_ref as LR

F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def wide(rows, cols, extra, dtype=F64, seed=0, scale=1.0):
    """(rows, cols) view of a (rows, cols + extra) buffer: a row stride wider than the data."""
    buf = torch.randn(rows, cols + extra, generator=gen(seed), dtype=F64) * scale
    return buf.to(dtype)[:, :cols]


def to_cl(x):
    """(B, C, L) -> channels-last rows (B*L, C)."""
    return x.permute(0, 2, 1).reshape(-1, x.shape[1])


def close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the reference against torch
# ---------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [  # (B, L, Cin, Cout, k, stride)
    (2, 16, 8, 12, 3, 1), (3, 15, 5, 7, 3, 2), (2, 9, 6, 4, 1, 1), (3, 10, 4, 6, 1, 2), (1, 7, 3, 5, 3, 2), (5, 13, 9, 11, 3, 1)]


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_forward_mode0_matches_conv1d(shape):
    B, L, Cin, Cout, k, stride = shape
    pad = (k - 1) // 2
    x = torch.randn(B, Cin, L, generator=gen(1), dtype=F64)
    w = torch.randn(Cout, Cin, k, generator=gen(2), dtype=F64)
    y = F.conv1d(x, w, stride=stride, padding=pad)
    Lo = y.shape[2]
    M = B * Lo
    A = torch.zeros(B * L, Cin + 3, dtype=F64)                       # lda = Cin + 3
    A[:, :Cin] = to_cl(x)
    Bm = torch.zeros(Cout, k * Cin + 5, dtype=F64)                   # ldb = k*Cin + 5
    Bm[:, :k * Cin] = w.permute(0, 2, 1).reshape(Cout, k * Cin)
    e = LR.gemm_nt_ref(A, Bm, M, Cout, Cin, taps=k, stride=stride, pad=pad, mode=0, Lout=Lo, Lsrc=L, out_dtype=torch.float32)
    close(e["C"].ref, to_cl(y))


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_data_gradient_mode1_matches_autograd(shape):
    B, L, Cin, Cout, k, stride = shape
    pad = (k - 1) // 2
    x = torch.randn(B, Cin, L, generator=gen(3), dtype=F64, requires_grad=True)
    w = torch.randn(Cout, Cin, k, generator=gen(4), dtype=F64)
    y = F.conv1d(x, w, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=gen(5), dtype=F64)
    dx, = torch.autograd.grad(y, x, dy)
    Lo = y.shape[2]
    A = wide(B * Lo, Cout, 2)
    A.copy_(to_cl(dy))
    Bm = w.permute(1, 2, 0).reshape(Cin, k * Cout)                   # [Cin][k][Cout]
    e = LR.gemm_nt_ref(A, Bm, B * L, Cin, Cout, taps=k, stride=stride, pad=pad, mode=1, Lout=L, Lsrc=Lo, out_dtype=torch.float32)
    close(e["C"].ref, to_cl(dx))


@pytest.mark.parametrize("shape", CONV_SHAPES)
@pytest.mark.parametrize("w_layout", [0, 1])
def test_weight_gradient_matches_autograd(shape, w_layout):
    B, L, Cin, Cout, k, stride = shape
    pad = (k - 1) // 2
    x = torch.randn(B, Cin, L, generator=gen(6), dtype=F64)
    w = torch.randn(Cout, Cin, k, generator=gen(7), dtype=F64, requires_grad=True)
    y = F.conv1d(x, w, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=gen(8), dtype=F64)
    dw, = torch.autograd.grad(y, w, dy)
    Lo = y.shape[2]
    X = wide(B * L, Cin, 4)
    X.copy_(to_cl(x))
    dY = wide(B * Lo, Cout, 1)
    dY.copy_(to_cl(dy))
    old = torch.randn(dw.shape, generator=gen(9), dtype=F64)
    for acc in (None, old if w_layout == 1 else old.permute(0, 2, 1)):
        e = LR.wgrad_ref([dict(dY=dY, X=X, M=B * Lo, Lout=Lo, Lsrc=L)], Cout, Cin, taps=k, stride=stride, pad=pad, w_layout=w_layout,
                         dW_old=acc)
        want = dw if w_layout == 1 else dw.permute(0, 2, 1)
        close(e.ref, want + (0 if acc is None else acc))


def test_weight_gradient_groups_and_per_problem_cin():
    """Groups accumulate into one dW (shared-weight heads); gemm_wgrad_multi problems have their own Cin."""
    k, Cout = 3, 6
    parts, want = [], 0
    w = torch.randn(Cout, 5, k, generator=gen(10), dtype=F64, requires_grad=True)
    for i, (B, L) in enumerate([(2, 8), (2, 4), (3, 2)]):
        x = torch.randn(B, 5, L, generator=gen(20 + i), dtype=F64)
        y = F.conv1d(x, w, padding=1)
        dy = torch.randn(y.shape, generator=gen(30 + i), dtype=F64)
        want = want + torch.autograd.grad(y, w, dy)[0]
        parts.append(dict(dY=to_cl(dy), X=to_cl(x), M=B * L, Lout=L, Lsrc=L))
    close(LR.wgrad_ref(parts, Cout, 5, taps=3, pad=1, w_layout=1).ref, want)
    for Cin in (3, 8):                                                # the FPN laterals: one N, different Cin
        x = torch.randn(2, Cin, 6, generator=gen(Cin), dtype=F64)
        wl = torch.randn(Cout, Cin, 1, generator=gen(Cin + 1), dtype=F64, requires_grad=True)
        dy = torch.randn(2, Cout, 6, generator=gen(Cin + 2), dtype=F64)
        dw, = torch.autograd.grad(F.conv1d(x, wl), wl, dy)
        close(LR.wgrad_ref([dict(dY=to_cl(dy), X=to_cl(x), M=12, Lout=6, Lsrc=6)], Cout, Cin, taps=1, w_layout=1).ref, dw)


def test_linear_epilogue_fields_match_torch():
    """bias, gate, C2, accumulate, row strides lda / ldb / ldc / ldg, stats with a short last slab, ragged M."""
    B, T, D, N = 3, 50, 24, 20                                        # M = 150: slabs of 128 + 22
    M = B * T
    x = wide(M, D, 8, seed=11)
    W = wide(N, D, 3, seed=12)
    bias = torch.randn(N, generator=gen(13), dtype=F64)
    gate = wide(B, N, 5, seed=14)
    C_old = wide(M, N, 2, seed=15)
    lin = F.linear(x, W, bias)
    e = LR.gemm_nt_ref(x, W, M, N, D, Lout=T, bias=bias, gate=gate, C_old=C_old, C2=True, out_dtype=torch.float32)
    close(e["C2"].ref, lin)
    close(e["C"].ref, lin * gate.repeat_interleave(T, 0) + C_old)
    e = LR.gemm_nt_ref(x, W, M, N, D, Lout=T, stats=True, out_dtype=torch.float32)
    acc = F.linear(x, W)
    for j, (lo, hi) in enumerate([(0, 128), (128, 150)]):
        close(e["stats"].ref[j, 0], acc[lo:hi].sum(0))
        close(e["stats"].ref[j, 1], acc[lo:hi].var(0, unbiased=False) * (hi - lo))


def test_gate_backward_epilogue_matches_definition():
    """gb_dct[c][m] = dtype(g * gate), gb_dgate = sum_t g * act, gb_dsum = sum_t g * gate with g = the product rounded to the dtype."""
    B, T, C, Cout = 2, 32, 16, 8
    dy = torch.randn(B * T, Cout, generator=gen(16), dtype=F64).to(torch.bfloat16)
    Wd = torch.randn(C, 3 * Cout, generator=gen(17), dtype=F64).to(torch.bfloat16)
    gate = torch.rand(B, C, generator=gen(18), dtype=F64).float()
    act = torch.randn(B * T, C, generator=gen(19), dtype=F64).to(torch.bfloat16)
    e = LR.gemm_nt_ref(dy, Wd, B * T, C, Cout, taps=3, pad=1, mode=1, Lout=T, Lsrc=T, gate=gate, gb_act=act)
    dx = LR.gemm_nt_ref(dy, Wd, B * T, C, Cout, taps=3, pad=1, mode=1, Lout=T, Lsrc=T, out_dtype=torch.float32)["C"].ref
    g = dx.float().to(torch.bfloat16).double()
    gt = gate.double().repeat_interleave(T, 0)
    close(e["gb_dct"].ref, (dx * gt).t())
    close(e["gb_dgate"].ref, (g * act.double()).view(B, T, C).sum(1))
    close(e["gb_dsum"].ref, (g * gt).view(B, T, C).sum(1))


def test_skinny_and_outer_match_torch():
    X = wide(40, 32, 4, seed=21)
    W = torch.randn(24, 32, generator=gen(22), dtype=F64)
    b = torch.randn(24, generator=gen(23), dtype=F64)
    mask = torch.randn(40, 24, generator=gen(24), dtype=F64)
    e = LR.skinny_ref(X, W, bias=b, mask=mask, relu=True)
    close(e.ref, torch.relu(F.linear(X, W, b)) * (mask > 0))
    Xb = X.to(torch.bfloat16)                                         # bf16 rows: the weights are rounded too
    close(LR.skinny_ref(Xb, W).ref, F.linear(Xb.double(), W.to(torch.bfloat16).double()))
    dY = torch.randn(40, 24, generator=gen(25), dtype=F64)
    o = LR.outer_ref(dY, X)
    close(o["dW"].ref, dY.t() @ X)
    close(o["db"].ref, dY.sum(0))
    o = LR.outer_ref(dY, X, lowp=True)
    close(o["dW"].ref, dY.to(torch.bfloat16).double().t() @ X.to(torch.bfloat16).double())
    close(o["db"].ref, dY.sum(0))


def test_w4_block_order_is_a_permutation():
    for M, N in [(4096, 4096), (512, 768), (8192, 256)]:
        tiles = LR.w4_block_tiles(M, N)
        assert sorted(tiles) == [(a, b) for a in range(M // 256) for b in range(N // 256)]


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 implementation of the contract with its own summation order: what the comparator must accept
# ---------------------------------------------------------------------------------------------------------------------
def fp32_conv(A, Bm, M, N, Cin, taps, pad, Lout, Lsrc, splits=5, mode=0, stride=1, drop=None, tapfix=None):
    """C' = A' B^T accumulated in fp32: the K loop split `splits` ways, the partials added in REVERSE order.
    drop: (k0, k1) columns of K skipped (a lost K-step); tapfix(tap, row, ok) -> (row, ok): a faulty addressing."""
    K = taps * Cin
    cols = []
    for tap in range(taps):
        row, ok = LR.src_rows(M, Lout, Lsrc, stride, pad, tap, mode, A.device)
        if tapfix is not None:
            row, ok = tapfix(tap, row, ok)
        cols.append(A[:, :Cin][row].float() * ok.unsqueeze(1).float())
    Ap = torch.cat(cols, 1)
    Bf = Bm[:N, :K].float()
    if drop is not None:
        Ap[:, drop[0]:drop[1]] = 0
    edges = [K * i // splits for i in range(splits + 1)]
    parts = [Ap[:, a:b] @ Bf[:, a:b].t() for a, b in zip(edges, edges[1:])]
    acc = torch.zeros(M, N)
    for p in reversed(parts):
        acc = acc + p
    return acc


def conv0_like(seed=0, B=4, Lout=64, Cin=4352, N=128):
    """conv0's reduction (k = 3 over 4096 + 256 channels: K = 13056) on a few clips, bf16 operands at the model's scale."""
    A = (torch.rand(B * Lout, Cin, generator=gen(seed)) - 0.3).to(torch.bfloat16)
    Bm = (torch.randn(N, 3 * Cin, generator=gen(seed + 1)) / (3 * Cin) ** 0.5).to(torch.bfloat16)
    return A, Bm, B * Lout, N, Cin, Lout


def check(e, got, tag="t"):
    return LR.compare(tag, e, got)


def test_fp32_reordered_conv0_is_accepted():
    A, Bm, M, N, Cin, Lout = conv0_like()
    bias = torch.randn(N, generator=gen(40)) * 0.1
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout, bias=bias.double(), stats=True, C2=True)
    acc = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout)
    mx, rel = check(e["C"], (acc + bias).to(torch.bfloat16))
    assert mx < 1 and rel < 2 ** -8
    check(e["C2"], (acc + bias).to(torch.bfloat16))
    check(e["stats"], fp32_stats(acc))
    # another split count, no bias, fp32 output (parity mode): accepted at the fp32 bound too
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout, out_dtype=torch.float32)
    check(e["C"], fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout, splits=17))


def fp32_stats(acc, shift=0):
    """(sum, M2) per 128-row slab in fp32, the slab boundaries optionally shifted by `shift` rows (a fault)."""
    M, N = acc.shape
    out = torch.zeros((M + 127) // 128, 2, N)
    for j in range(out.shape[0]):
        x = acc[max(0, 128 * j + shift):128 * (j + 1) + shift]
        out[j, 0] = x.sum(0)
        out[j, 1] = ((x - x.mean(0)) ** 2).sum(0)
    return out


def test_fp32_reordered_gate_backward_and_sumsq_are_accepted():
    # gate backward (conv0's data gradient: k = 3, K = 3 * 512, Lout = 256)
    B, T, C, Cout = 2, 256, 64, 512
    dy = (torch.randn(B * T, Cout, generator=gen(41)) * 0.05).to(torch.bfloat16)
    Wd = (torch.randn(C, 3 * Cout, generator=gen(42)) / 40).to(torch.bfloat16)
    gate = torch.rand(B, C, generator=gen(43))
    act = torch.randn(B * T, C, generator=gen(44)).to(torch.bfloat16)
    e = LR.gemm_nt_ref(dy, Wd, B * T, C, Cout, taps=3, pad=1, mode=1, Lout=T, Lsrc=T, gate=gate, gb_act=act)
    g = fp32_conv(dy, Wd, B * T, C, Cout, 3, 1, T, T, mode=1, splits=3).to(torch.bfloat16).float()
    gt = gate.repeat_interleave(T, 0)
    check(e["gb_dct"], (g * gt).to(torch.bfloat16).t())
    check(e["gb_dgate"], (g * act.float()).view(B, T, C).flip(1).sum(1))
    check(e["gb_dsum"], g.view(B, T, C).sum(1) * gate)
    # prop_fc's weight gradient as an NT product with per-tile squared sums (K = B*T = 8192)
    M = N = 512
    Kr = 8192
    a = (torch.randn(M, Kr, generator=gen(45)) * 0.01).to(torch.bfloat16)
    b = torch.rand(N, Kr, generator=gen(46)).to(torch.bfloat16)
    e = LR.gemm_nt_ref(a, b, M, N, Kr, out_dtype=torch.float32, sumsq=True)
    c = fp32_conv(a, b, M, N, Kr, 1, 0, M, M, splits=11)
    check(e["C"], c)
    check(e["sumsq"], fp32_sumsq(c))


def fp32_sumsq(c):
    M, N = c.shape
    t = (c * c).view(M // 256, 256, N // 256, 256).sum((1, 3))
    return torch.stack([t[a, b] for a, b in LR.w4_block_tiles(M, N)])


def fp32_wgrad(dY, X, M, N, Cin, Lout, nsplit=8, skip=None):
    """dW [N][3][Cin] (k = 3, pad 1) in fp32 from `nsplit` row splits added in order; skip: one split's partial left out."""
    parts = []
    edges = [M * i // nsplit for i in range(nsplit + 1)]
    for i, (a, b) in enumerate(zip(edges, edges[1:])):
        p = torch.zeros(N, 3, Cin)
        for tap in range(3):
            row, ok = LR.src_rows(M, Lout, Lout, 1, 1, tap, 0, X.device)
            x = X[row].float() * ok.unsqueeze(1).float()
            p[:, tap] = dY[a:b].float().t() @ x[a:b]
        if i != skip:
            parts.append(p)
    out = torch.zeros(N, 3, Cin)
    for p in parts:
        out = out + p
    return out


def wgrad_case():
    M, Lout, N, Cin = 8192, 256, 64, 32
    dY = (torch.randn(M, N, generator=gen(50)) * 0.01).to(torch.bfloat16)
    X = torch.rand(M, Cin, generator=gen(51)).to(torch.bfloat16)
    e = LR.wgrad_ref([dict(dY=dY, X=X, M=M, Lout=Lout, Lsrc=Lout)], N, Cin, taps=3, pad=1)
    return dY, X, M, N, Cin, Lout, e


def test_fp32_reordered_wgrad_and_query_side_are_accepted():
    dY, X, M, N, Cin, Lout, e = wgrad_case()
    check(e, fp32_wgrad(dY, X, M, N, Cin, Lout))
    Xq = torch.randn(64, 1024, generator=gen(52))
    Wq = torch.randn(768, 1024, generator=gen(53)) / 32
    check(LR.skinny_ref(Xq, Wq, relu=True), torch.relu((Xq[:, 512:] @ Wq[:, 512:].t()) + (Xq[:, :512] @ Wq[:, :512].t())))
    o = LR.outer_ref(Wq[:64].t().contiguous(), Xq.t()[:, :48].contiguous(), lowp=True)
    dYb, Xb = Wq[:64].t().to(torch.bfloat16).float(), Xq.t()[:, :48].to(torch.bfloat16).float()
    check(o["dW"], dYb[512:].t() @ Xb[512:] + dYb[:512].t() @ Xb[:512])
    check(o["db"], Wq[:64].t().flip(0).sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# mutations: each a plausible kernel fault; the comparator must reject every one at realistic K
# ---------------------------------------------------------------------------------------------------------------------
def rejected(e, got):
    with pytest.raises(LR.LaunchMismatch):
        LR.compare("mutant", e, got)


def test_rejects_a_dropped_k_step():
    A, Bm, M, N, Cin, Lout = conv0_like(seed=3)
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout)
    ok = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout)
    check(e["C"], ok.to(torch.bfloat16))
    for k0 in (0, 64 * 100, 13056 - 64):                             # first, a middle and the last K-step
        bad = ok.clone()
        bad[:, :] = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout, drop=(k0, k0 + 64))
        rejected(e["C"], bad.to(torch.bfloat16))
    # a K-step lost by ONE 128x128 tile only (a hazard inside one workgroup): still caught
    bad = ok.clone()
    bad[128:256, :] = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout, drop=(6400, 6464))[128:256]
    rejected(e["C"], bad.to(torch.bfloat16))


def test_rejects_padding_row_read_from_the_neighbouring_clip():
    A, Bm, M, N, Cin, Lout = conv0_like(seed=5)
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout)

    def leak(tap, row, ok):                                           # t = 0, tap 0 reads the previous clip's last row
        m = torch.arange(row.shape[0])
        edge = (tap == 0) & (m % Lout == 0) & (m >= Lout)
        return torch.where(edge, m - 1, row), ok | edge
    rejected(e["C"], fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout, tapfix=leak).to(torch.bfloat16))


def test_rejects_a_tap_offset_by_one():
    A, Bm, M, N, Cin, Lout = conv0_like(seed=7)
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout)

    def shifted(tap, row, ok):
        if tap != 2:
            return row, ok
        r2, ok2 = LR.src_rows(row.shape[0], Lout, Lout, 1, 1, 3, 0, row.device)      # tap 2 reads tap 3's rows
        return r2, ok2
    rejected(e["C"], fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout, tapfix=shifted).to(torch.bfloat16))


def test_rejects_one_scaled_16x16_block():
    A, Bm, M, N, Cin, Lout = conv0_like(seed=9)
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout)
    bad = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout)
    bad[48:64, 96:112] *= 1.01
    rejected(e["C"], bad.to(torch.bfloat16))


def test_rejects_one_unwritten_element():
    A, Bm, M, N, Cin, Lout = conv0_like(seed=11)
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout)
    bad = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout).to(torch.bfloat16)
    bad[M - 1, N - 1] = float("nan")
    rejected(e["C"], bad)
    dY, X, M, N, Cin, Lout, ew = wgrad_case()
    badw = fp32_wgrad(dY, X, M, N, Cin, Lout)
    badw[3, 1, 7] = float("nan")
    rejected(ew, badw)


def test_rejects_a_stats_slab_shifted_by_one_row():
    A, Bm, M, N, Cin, Lout = conv0_like(seed=13, B=5)                 # M = 320: slabs 128, 128, 64
    e = LR.gemm_nt_ref(A, Bm, M, N, Cin, taps=3, pad=1, Lout=Lout, stats=True)
    acc = fp32_conv(A, Bm, M, N, Cin, 3, 1, Lout, Lout)
    check(e["stats"], fp32_stats(acc))
    rejected(e["stats"], fp32_stats(acc, shift=1))
    bad = fp32_stats(acc)
    bad[1] = fp32_stats(acc, shift=1)[1]                              # one slab only
    rejected(e["stats"], bad)


def test_rejects_a_weight_gradient_missing_one_split():
    dY, X, M, N, Cin, Lout, e = wgrad_case()
    for skip in (0, 5, 7):
        rejected(e, fp32_wgrad(dY, X, M, N, Cin, Lout, skip=skip))


def test_rejects_gate_backward_and_sumsq_faults():
    B, T, C, Cout = 2, 256, 64, 512
    dy = (torch.randn(B * T, Cout, generator=gen(60)) * 0.05).to(torch.bfloat16)
    Wd = (torch.randn(C, 3 * Cout, generator=gen(61)) / 40).to(torch.bfloat16)
    gate = torch.rand(B, C, generator=gen(62)) + 0.5
    act = torch.randn(B * T, C, generator=gen(63)).to(torch.bfloat16)
    e = LR.gemm_nt_ref(dy, Wd, B * T, C, Cout, taps=3, pad=1, mode=1, Lout=T, Lsrc=T, gate=gate, gb_act=act)
    g = fp32_conv(dy, Wd, B * T, C, Cout, 3, 1, T, T, mode=1).to(torch.bfloat16).float()
    gd = (g * act.float()).view(B, T, C)
    check(e["gb_dgate"], gd.sum(1))
    rejected(e["gb_dgate"], gd[:, 1:].sum(1))                         # one row of the clip left out
    gl = fp32_conv(dy, Wd, B * T, C, Cout, 3, 1, T, T, mode=1, drop=(512, 576)).to(torch.bfloat16).float()
    rejected(e["gb_dct"], (gl * gate.repeat_interleave(T, 0)).to(torch.bfloat16).t())
    M = N = 512
    a = (torch.randn(M, 8192, generator=gen(64)) * 0.01).to(torch.bfloat16)
    b = torch.rand(N, 8192, generator=gen(65)).to(torch.bfloat16)
    e = LR.gemm_nt_ref(a, b, M, N, 8192, out_dtype=torch.float32, sumsq=True)
    c = fp32_conv(a, b, M, N, 8192, 1, 0, M, M)
    s = fp32_sumsq(c)
    rejected(e["sumsq"], s.flip(0))                                   # the tiles in another order
    c[0:16, 0:16] *= 1.01
    rejected(e["sumsq"], fp32_sumsq(c))


# ---------------------------------------------------------------------------------------------------------------------
# the shadow step wraps drn_amd.ops functions: every call site must go through the module attribute
# ---------------------------------------------------------------------------------------------------------------------
WRAPPED = ("gemm_desc", "wgrad_desc", "gemm_nt", "gemm_wgrad", "gemm_wgrad_multi", "wgrad_reduce_pending", "skinny_group",
           "outer_wgrad", "conv_bn_train")


def test_gemm_entry_points_are_reached_through_the_ops_module():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "drn_amd")
    direct = re.compile(r"from\s+\.+(ops)?\s+import\s+[^\n]*\b(%s)\b" % "|".join(WRAPPED))
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not direct.search(src), "%s imports a GEMM entry point by name (the shadow step could not see it)" % f
                if f != "ops.py":
                    for name in WRAPPED:
                        for m in re.finditer(r"(?<![\w.])%s\s*\(" % name, src):
                            raise AssertionError("%s calls %s without the ops. prefix" % (f, name))
