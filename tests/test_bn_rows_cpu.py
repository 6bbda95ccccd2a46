"""tests/bn_ref.py checked without a GPU: the variance bound holds for a torch emulation of the slab scheme (fp32 slab sum, fp32 slab
mean, centred fp32 second pass, bn_merge_cols' double merge with its n_last handling) on every column kind, a naive fp32
E[x^2] - E[x]^2 on the same data breaks it by more than 10x on the `offset` columns -- which is what makes the GPU test
(tests/test_bn_rows_gpu.py) worth having --, exact_gemm_case is exact, and the mirrored launcher thresholds sit where csrc/bn.hip
puts them."""
import pytest
import torch

import bn_ref as R

ROWS = [8192, 8193, 8321, 16500]          # 64 slabs; 65 with a one-row last slab; the issue's emulation size; 129 slabs, ragged


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def emu(request):
    """{M: (x, exact stats, slab-scheme (mean, var), naive (mean, var))} on bn_ref.columns, computed once."""
    dt = request.param
    out = {}
    for M in ROWS:
        x = R.columns(M, 128, dt, seed=M)
        out[M] = (x, R.exact_stats(x), R.merge_slabs(R.slab_stats_fp32(x), M), R.merge_naive(R.slab_stats_naive_fp32(x), M))
    return dt, out


def test_slab_scheme_stays_inside_the_variance_bound_on_every_column_kind(emu):
    dt, cases = emu
    worst = 0.0
    for M, (x, (mean, var, varb, xmax), (m_s, v_s), _) in cases.items():
        bound = R.var_bound(var, varb, xmax)
        ratio = ((v_s - var).abs() / bound.clamp_min(1e-300))
        ratio[(v_s == var)] = 0.0
        assert float(ratio.max()) <= 1.0, (M, int(ratio.argmax()), float(ratio.max()))
        assert bool(((m_s - mean).abs() <= R.delta_of(xmax)).all()), M
        worst = max(worst, float(ratio.max()))
        for kind in R.KINDS:                                      # every kind is present in every tile, and is what it says
            assert len(R.kind_index(128, kind)) == 2
        c = R.kind_index(128, "offset")
        want = R.OFFSET[dt][0] / R.OFFSET[dt][1]
        assert bool(((mean[c].abs() / var[c].sqrt()) / want - 1).abs().max() < 0.15)
        assert bool((var[R.kind_index(128, "const")] == 0).all())
        assert bool((var[R.kind_index(128, "tiny")] < 0.01 * R.EPS).all())
        assert bool((xmax[R.kind_index(128, "outlier")] == R.OUTLIER[dt]).all())
    print("slab scheme, %s: largest |var - var_ref| / bound = %.3g" % (dt, worst))
    # not slack beyond use either: the emulation reaches a thousandth of it somewhere
    assert worst >= 1e-3


def test_naive_variance_breaks_the_bound_tenfold_on_the_offset_columns(emu):
    """fp32 data at |mean| / std = 16384.  (The bf16 columns cannot show it: bf16 values of one binade are multiples of one quantum with
    8-bit factors, so 128 of them, and 128 of their squares, sum EXACTLY in fp32 -- a naive epilogue is exact on them.  The ratio there
    is limited to ~128 by the format, |mean| 2^-7 <= std; it is fp32 accumulators the epilogues see.)"""
    dt, cases = emu
    if dt == torch.bfloat16:
        for M, (x, (mean, var, varb, xmax), _, (m_n, v_n)) in cases.items():
            c = R.kind_index(128, "offset")
            assert bool(((v_n - var).abs()[c] <= R.var_bound(var, varb, xmax)[c]).all())       # exact slab sums: nothing to break
        return
    for M, (x, (mean, var, varb, xmax), (m_s, v_s), (m_n, v_n)) in cases.items():
        c = R.kind_index(128, "offset")
        bound = R.var_bound(var, varb, xmax)[c]
        naive = (v_n - var).abs()[c]
        slab = (v_s - var).abs()[c]
        print("M = %d: offset columns, naive / bound = %s, slab scheme / bound = %s, bound / var = %s"
              % (M, (naive / bound).tolist(), (slab / bound).tolist(), (bound / var[c]).tolist()))
        assert bool((naive >= 10.0 * bound).all()), (M, (naive / bound).tolist())
        assert bool((slab <= bound).all())


def test_bound_constants_are_the_derived_ones():
    assert R.A_VAR == R.gamma_n(130) and 7.7e-6 < R.A_VAR < 7.8e-6
    assert R.delta_of(1.0) == R.gamma_n(128) and abs(R.delta_of(1.0) / (128 * R.U) - 1) < 1e-5
    # a column of one value: the bound is the square of the slab-mean error alone
    z = torch.zeros(1, dtype=torch.float64)
    assert float(R.var_bound(z, z, torch.tensor([0.7], dtype=torch.float64))) == pytest.approx(2 * (128 * R.U * 0.7) ** 2, rel=1e-4)


def test_merge_handles_the_ragged_last_slab_like_the_definition():
    """merge_slabs against the definition on exact (float64) slab pairs: M = 1 .. a few slabs, a last slab of 1, 127 and 128 rows."""
    for M in (1, 127, 128, 129, 255, 256, 257, 8193):
        x = torch.randn(M, 3, generator=torch.Generator().manual_seed(M), dtype=torch.float64) + 5.0
        pairs = []
        for r0 in range(0, M, 128):
            blk = x[r0:r0 + 128]
            pairs.append(torch.stack([blk.sum(0), ((blk - blk.mean(0)) ** 2).sum(0)]))
        mean, var = R.merge_slabs(torch.stack(pairs), M)
        assert torch.allclose(mean, x.mean(0), rtol=1e-13, atol=0)
        assert torch.allclose(var, x.var(0, unbiased=False), rtol=1e-11, atol=1e-15)


@pytest.mark.parametrize("taps,Cin,N,L", [(1, 64, 192, None), (1, 128, 128, None), (3, 64, 256, 128)])
def test_exact_gemm_case_is_exact_in_fp32_under_two_summation_orders(taps, Cin, N, L):
    M = 8320 + 57 if taps == 1 else 1024
    A, W, P = R.exact_gemm_case(M, Cin, N, taps=taps, L=L)
    assert A.dtype == W.dtype == torch.bfloat16 and P.dtype == torch.float64
    Af, Wf = A.float(), W.float().reshape(N, taps, Cin)
    if taps == 3:                                                     # im2col with the zero rows at the sequence edges
        x = Af.reshape(M // L, L, Cin)
        z = torch.zeros(M // L, 1, Cin)
        Af = torch.cat([torch.cat([z, x[:, :-1]], 1), x, torch.cat([x[:, 1:], z], 1)], 2).reshape(M, 3 * Cin)
    Wf = Wf.reshape(N, taps * Cin)
    K = taps * Cin
    fwd = torch.zeros(M, N)
    for k in range(K):                                                # one term at a time, first to last ...
        fwd += Af[:, k:k + 1] * Wf[:, k][None, :]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(1))
    halves = [torch.zeros(M, N), torch.zeros(M, N)]
    for i, k in enumerate(perm.tolist()):                             # ... and shuffled, in two partial sums added at the end
        halves[i % 2] += Af[:, k:k + 1] * Wf[:, k][None, :]
    other = halves[0] + halves[1]
    assert torch.equal(fwd.double(), P) and torch.equal(other.double(), P)
    assert torch.equal((Af @ Wf.t()).double(), P)                     # and whatever order the BLAS takes
    # the column kinds arrive through the weights
    mean, var, _, xmax = R.exact_stats(P)
    off = R.kind_index(N, "offset")
    assert bool((mean[off].abs() / var[off].sqrt() > 100).all())
    assert bool((var[R.kind_index(N, "const")] == 0).all()) and bool((P[:, R.kind_index(N, "const")] == 2.375).all())
    assert bool((var[R.kind_index(N, "tiny")] < 0.01 * R.EPS).all()) and bool((var[R.kind_index(N, "tiny")] > 0).all())
    assert bool((var[R.kind_index(N, "big")].sqrt() > 500).all())
    assert bool((xmax[R.kind_index(N, "outlier")] == 9984.0).all())
    assert bool((P[:, R.kind_index(N, "relu_off")] == 0).all())


def test_slab_bounds_hold_for_the_emulated_epilogue_on_exact_accumulators():
    A, W, P = R.exact_gemm_case(8377, 64, 128)
    st = R.slab_stats_fp32(P.float())                                  # P is exact in fp32
    assert torch.equal(P.float().double(), P)
    s, ds, m2, dm2 = R.slab_bounds(P)
    assert bool(((st[:, 0].double() - s).abs() <= ds).all())
    assert bool(((st[:, 1].double() - m2).abs() <= dm2).all())
    mean, var, varb, xmax = R.exact_stats(P)
    m_s, v_s = R.merge_slabs(st, 8377)
    assert bool(((v_s - var).abs() <= R.var_bound(var, varb, xmax)).all())
    m_n, v_n = R.merge_naive(R.slab_stats_naive_fp32(P.float()), 8377)
    off = R.kind_index(128, "offset")
    assert bool(((v_n - var).abs()[off] >= 10 * R.var_bound(var, varb, xmax)[off]).all())


def test_forward_ref_is_batchnorm1d_with_relu_upsample_and_gate():
    B, L, C = 3, 8, 5
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(B * L, C, generator=g, dtype=torch.float64) * 2 + 1
    up = torch.randn(B * L // 2, C, generator=g, dtype=torch.float64)
    gate = torch.randn(B, C, generator=g, dtype=torch.float64)
    gamma, beta, cb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    r = R.forward_ref(raw, gamma, beta, 1e-5, cb, rm, rv, 0.1, True, up=up, gate=gate, L=L)
    bn = torch.nn.BatchNorm1d(C, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    y = torch.relu(bn(raw + cb.double()))                              # the conv bias shifts the mean only
    out = y.reshape(B, L, C) + up.reshape(B, L // 2, C).repeat_interleave(2, dim=1)
    assert torch.allclose(r["out"].reshape(B, L, C), out, rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["gated"].reshape(B, L, C), out * gate[:, None, :], rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["running_mean"], bn.running_mean, rtol=1e-12) and torch.allclose(r["running_var"], bn.running_var, rtol=1e-12)
    assert torch.allclose(r["invstd"], 1 / torch.sqrt(raw.var(0, unbiased=False) + 1e-5), rtol=1e-12)


def test_mirrored_thresholds_sit_where_the_launchers_put_them():
    f32, bf16 = torch.float32, torch.bfloat16
    # bn_merge_cols: registers up to 64 slabs
    assert [R.slabs(M) for M in (8192, 8193, 8320, 16500)] == [64, 65, 65, 129]
    assert R.merge_is_cached(8192) and not R.merge_is_cached(8193)
    assert (16500 - 128 * 128, [len(range(j, 129, 4)) for j in range(4)]) == (116, [33, 32, 32, 32])   # ragged, uneven over the lanes
    # drn_bn_train_apply: one trip of 4*RP rows up to 4096 workgroups
    assert R.rows_per_pass(f32) == 16 and R.rows_per_pass(bf16) == 32
    assert R.train_apply_rows_wg([131072], 128, f32) == 64 and R.train_apply_rows_wg([131074], 128, f32) == 128
    assert R.train_apply_rows_wg([262144], 128, bf16) == 128 and R.train_apply_rows_wg([262146], 128, bf16) == 256
    assert R.train_apply_rows_wg([8192 * 33], 1024, bf16) == 128 * 9
    # bn_bwd_launch64: at most 64 reduce blocks per level; apply blocks of 8*RP rows beyond 4096 workgroups
    lv, arows = R.bwd64_rrows_arows([32768, 16384, 8192], 256, f32)
    assert lv == [(512, 64, True), (448, 37, False), (448, 19, False)] and arows == 64
    lv, arows = R.bwd64_rrows_arows([32768, 16384, 8192], 256, bf16)
    assert lv == [(512, 64, False), (512, 32, False), (512, 16, False)] and arows == 128
    assert R.bwd64_rrows_arows([8193], 64, f32) == ([(192, 43, True)], 64)
    assert R.bwd64_rrows_arows([262144], 64, f32)[1] == 64 and R.bwd64_rrows_arows([262209], 64, f32) == ([(4160, 64, True)], 128)
    # bn_bwd_one_plan: at most 64 row blocks of 16*RP rows per level and 512 workgroups
    assert R.bwd_one_fits([8193], 64, f32) and R.bwd_one_fits([16384], 128, f32) and not R.bwd_one_fits([16385], 128, f32)
    assert R.bwd_one_fits([32768, 16384, 8192], 256, bf16) and not R.bwd_one_fits([32768, 16384, 8192], 256, f32)
    assert not R.bwd_one_fits([40000], 1024, bf16) and not R.bwd_one_fits([8192, 4096, 2048], 1024, f32)     # (tests/test_bn_bwd_one_gpu.py)
    # row_grid: ~4 rows per thread, a multiple of nvec / gcd(nvec, 256) blocks, at most 4096 (+ rounding)
    assert R.row_grid_blocks(3, 9) == (9, 1, False) and R.row_grid_blocks(70001, 9) == (621, 4, False)
    assert R.row_grid_blocks(466033, 9)[2] is False and R.row_grid_blocks(466034, 9) == (4104, 4, True)
    assert R.row_grid_blocks(8192, 128) == (1024, 4, False)
    # three-launch backward: partial-sum row blocks
    assert [R.bwd3_nblk([M], 72, bf16)[0] for M in (3, 300, 4096, 70001)] == [1, 18, 256, 256]
    assert [R.bwd3_nblk([M], 36, f32)[0] for M in (3, 300, 4096, 70001)] == [1, 18, 256, 256]
