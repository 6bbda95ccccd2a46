"""The BatchNorm kernels past 64 row slabs and on ill-conditioned columns (csrc/bn.hip, csrc/bn_merge.h, the statistics part of the GEMM
epilogues), called through drn_amd.ops at the smallest shapes that cross each threshold of the launchers, against the float64 model
and the derived bounds of tests/bn_ref.py (checked without a GPU by tests/test_bn_rows_cpu.py):

  1. the statistics merge and the apply pass (ops.bn_train_apply): 64 / 65 / 129 slabs, ragged last slabs, levels sharing a module, the
     top-down chain in one launch, and the multi-trip row loop beyond 4096 workgroups;
  2. the epilogue statistics of every GEMM kernel that writes them, on accumulators that are exact whatever the summation order, and
     the tagged merge of the one-launch conv -> BN kernel above 64 slabs;
  3. the backward (ops.bn_bwd_multi), one launch and two: enlarged reduce blocks, 8*RP apply blocks, the plan that declines, the gate
     backward inside the launch, in place;
  4. the three-launch backward and row_grid (C % 64 != 0): ragged block counts, the finalize loop's tail, the 4096-block cap.

Every case asserts through bn_ref's mirrored launcher arithmetic which side of its threshold it is on.  No tolerance comes from a
kernel's output: each is a bound derived in bn_ref.py or a formula the suite already uses (named where used).  With -s every test
prints its largest err / bound; the module prints the largest per group when it is done (DESIGN.md quotes one MI355X run)."""
import numpy as np
import pytest
import torch

import bn_ref as R
from test_bn_bwd_one_gpu import _run
from test_gemm_gpu import _restore_tuning, tune          # noqa: F401  (the fixture restores what tune() changed)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DTS = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("\n[bn-rows] %-44s largest err / bound = %.3g" % (k, RATIOS[k]), end="")
    print()


def code_of(dt):
    from drn_amd import ops
    return ops.BF16 if dt == BF16 else ops.F32


def check(group, what, got, ref, bound):
    """|got - ref| <= bound elementwise (bound 0: equal); records the largest err / bound of the group."""
    assert bool(torch.isfinite(got.float()).all()), "%s: %s holds a NaN / Inf (an element nobody wrote?)" % (group, what)
    err = (got.double() - ref.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    assert bool(torch.isfinite(err).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), \
        "%s / %s: the reference or the bound is not finite" % (group, what)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[group] = max(RATIOS.get(group, 0.0), worst)
    print("[bn-rows] %s / %s: err / bound = %.3g" % (group, what, worst))
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = [int(j) for j in np.unravel_index(i, tuple(err.shape))]
        raise AssertionError("%s / %s: err %.6g > bound %.6g at %s (got %.9g, want %.9g)"
                             % (group, what, float(err.flatten()[i]), float(bound.flatten()[i]), idx, float(got.flatten()[i]),
                                float(ref.flatten()[i])))


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. statistics merge + apply
# ---------------------------------------------------------------------------------------------------------------------------------
def train_level(M, C, dt, seed, L, ld_extra=0, up=False, gate=False, module=None, raw=None, stats=None):
    """One level of an ops.bn_train_apply launch on bn_ref.columns: statistics made on the host per slab from the stored values (as
    test_top_down_chain_in_one_batchnorm_launch does), outputs pre-filled with NaN, every buffer `ld_extra` columns wider than C."""
    ld = C + ld_extra
    if raw is None:
        raw = R.columns(M, C, dt, seed, ld=ld, fill=7.0).to(DEV)
    x = raw[:, :C]
    if stats is None:
        stats = R.slab_stats_fp32(x)
    B = M // L
    if module is None:
        gamma, beta = R.affine(C, seed + 1)
        module = dict(gamma=gamma.to(DEV), beta=beta.to(DEV), conv_bias=rnd(C, seed=seed + 2, scale=0.2).to(DEV),
                      running_mean=rnd(C, seed=seed + 3, scale=0.5).to(DEV), running_var=(rnd(C, seed=seed + 4).abs() + 0.5).to(DEV))
    lv = dict(module)
    lv.update(raw=x, ld_raw=ld, M=M, L=L, stats=stats, tiles=stats.shape[0], momentum=0.1, eps=R.EPS,
              ss=torch.full((2, C), float("nan"), device=DEV), save=torch.full((2, C), float("nan"), device=DEV),
              out_full=torch.full((M, ld), float("nan"), device=DEV, dtype=dt), ld_out=ld)
    lv["out"] = lv["out_full"][:, :C]
    if up:
        lv["up_full"] = torch.cat([rnd(M // 2, C, seed=seed + 5), torch.full((M // 2, ld_extra), 7.0)], 1).to(DEV, dt)
        lv["up"], lv["ld_up"] = lv["up_full"][:, :C], ld
    if gate:
        lv["gate_full"] = torch.cat([rnd(B, C, seed=seed + 6, scale=0.5) + 1.0, torch.full((B, ld_extra), 7.0)], 1).to(DEV)
        lv["gate"] = lv["gate_full"][:, :C]                       # (ops passes gate.stride(0))
        lv["gated_full"] = torch.full((M, ld), float("nan"), device=DEV, dtype=dt)
        lv["gated"], lv["ld_gated"] = lv["gated_full"][:, :C], ld
    return lv


def verify_train_level(lv, C, dt, rm0, rv0, group, relu=True, stats_of=None):
    """save / ss / running statistics against forward_ref within bn_ref.stat_bounds, out / gated within apply_bound (the kernel's own
    scale / shift) and out_bound (the model's), nothing written past C."""
    x, M, L = lv["raw"], lv["M"], lv["L"]
    up, gate = lv.get("up"), lv.get("gate")
    r = R.forward_ref(x, lv["gamma"], lv["beta"], R.EPS, lv["conv_bias"], rm0, rv0, 0.1, relu, up=up, gate=gate, L=L, stats_of=stats_of)
    sb = R.stat_bounds(r, lv["gamma"], lv["beta"], R.EPS, M, lv["conv_bias"], rm0, rv0, 0.1)
    check(group + " stats", "save mean", lv["save"][0], r["mean"], sb["mean"])
    check(group + " stats", "save invstd", lv["save"][1], r["invstd"], sb["invstd"])
    # the variance itself, back out of the stored invstd (whose fp32 rounding moves var + eps by 2 u relative: 3 u allowed), all columns
    # and the offset columns alone -- where the bound is widest, so that its slack there shows in the report
    var_k = 1.0 / lv["save"][1].double() ** 2 - R.EPS
    var_b = sb["var"] + 3 * R.U * (r["var"] + R.EPS)
    ofs = R.kind_index(C, "offset").to(DEV)
    check(group + " variance", "var", var_k, r["var"], var_b)
    check(group + " variance, offset columns", "var", var_k[ofs], r["var"][ofs], var_b[ofs])
    check(group + " stats", "scale", lv["ss"][0], r["scale"], sb["scale"])
    check(group + " stats", "shift", lv["ss"][1], r["shift"], sb["shift"])
    check(group + " stats", "running_mean", lv["running_mean"], r["running_mean"], sb["running_mean"])
    check(group + " stats", "running_var", lv["running_var"], r["running_var"], sb["running_var"])
    k = R.forward_ref(x, lv["gamma"], lv["beta"], R.EPS, None, None, None, 0.1, relu, up=up, gate=gate, L=L, scale_shift=(lv["ss"][0], lv["ss"][1]))
    up2 = R.upsample2(up, M // L, L) if up is not None else None
    g2 = gate.repeat_interleave(L, dim=0) if gate is not None else None
    check(group + " apply", "out", lv["out"], k["out"], R.apply_bound(x, lv["ss"][0], lv["ss"][1], k["out"], dt, up=up2))
    if gate is not None:
        check(group + " apply", "gated", lv["gated"], k["gated"], R.apply_bound(x, lv["ss"][0], lv["ss"][1], k["gated"], dt, up=up2, gate=g2))
    check(group + " end to end", "out", lv["out"], r["out"], R.out_bound(r, sb, x, dt, up=up2))
    if gate is not None:
        check(group + " end to end", "gated", lv["gated"], r["gated"], R.out_bound(r, sb, x, dt, up=up2, gate=g2))
    for name in ("out_full", "gated_full"):
        if name in lv and lv[name].shape[1] > C:
            assert bool(torch.isnan(lv[name][:, C:].float()).all()), "%s: columns past C were written" % name
    if relu:                                                     # the ReLU columns are what they say, and the kernel agrees exactly
        off, on = R.kind_index(C, "relu_off").to(DEV), R.kind_index(C, "relu_on").to(DEV)
        assert bool((r["y"][:, off] == 0).all()) and bool((r["y"][:, on] > 1).all())
        want_off = up2[:, off].double() if up2 is not None else torch.zeros_like(r["y"][:, off])
        assert torch.equal(lv["out"][:, off].double(), want_off.to(dt).double())


# M, L, extra row stride, upsample add (needs an even L)
MERGE_CASES = [(8192, 256, 0, True),       # 64 slabs: the last launch whose merge keeps its pairs in registers
               (8193, 3, 0, False),        # 65 slabs, a last slab of ONE row
               (8320, 128, 64, True),      # 65 full slabs; every buffer with a row stride above C
               (16500, 500, 0, True)]      # 129 slabs, a ragged last slab (116 rows), 33 / 32 / 32 / 32 slabs on the four slab lanes


@DTS
@pytest.mark.parametrize("M,L,ld_extra,up", MERGE_CASES)
def test_merge_and_apply_across_the_64_slab_threshold(dt, M, L, ld_extra, up):
    from drn_amd import ops
    C = 128                                                       # two channel tiles, two updater workgroups
    assert R.merge_is_cached(M) == (M == 8192) and R.slabs(M) == {8192: 64, 8193: 65, 8320: 65, 16500: 129}[M]
    assert R.train_apply_rows_wg([M], C, dt) == 4 * R.rows_per_pass(dt)          # one trip of the row loop
    lv = train_level(M, C, dt, seed=M, L=L, ld_extra=ld_extra, up=up, gate=True)
    rm0, rv0 = lv["running_mean"].clone(), lv["running_var"].clone()
    ops.bn_train_apply([lv], C, code_of(dt))
    torch.cuda.synchronize()
    verify_train_level(lv, C, dt, rm0, rv0, "1 merge+apply")


@DTS
def test_two_levels_sharing_one_module_update_its_running_statistics_in_order(dt):
    from drn_amd import ops
    C, Ms, Ls = 128, (8320, 4160), (128, 64)
    assert not R.merge_is_cached(Ms[0]) and R.merge_is_cached(Ms[1])
    a = train_level(Ms[0], C, dt, seed=11, L=Ls[0], gate=True)
    module = {k: a[k] for k in ("gamma", "beta", "conv_bias", "running_mean", "running_var")}
    b = train_level(Ms[1], C, dt, seed=12, L=Ls[1], module=module)
    rm0, rv0 = a["running_mean"].clone(), a["running_var"].clone()
    ops.bn_train_apply([a, b], C, code_of(dt))
    torch.cuda.synchronize()
    # the running statistics after BOTH updates: forward_ref twice, the first update's bound carried through the second
    ra = R.forward_ref(a["raw"], a["gamma"], a["beta"], R.EPS, a["conv_bias"], rm0, rv0, 0.1, True)
    sa = R.stat_bounds(ra, a["gamma"], a["beta"], R.EPS, Ms[0], a["conv_bias"], rm0, rv0, 0.1)
    rb = R.forward_ref(b["raw"], b["gamma"], b["beta"], R.EPS, b["conv_bias"], ra["running_mean"], ra["running_var"], 0.1, True)
    sb = R.stat_bounds(rb, b["gamma"], b["beta"], R.EPS, Ms[1], b["conv_bias"], ra["running_mean"], ra["running_var"], 0.1)
    check("1 shared module stats", "running_mean", a["running_mean"], rb["running_mean"], sb["running_mean"] + 0.9 * sa["running_mean"])
    check("1 shared module stats", "running_var", a["running_var"], rb["running_var"], sb["running_var"] + 0.9 * sa["running_var"])
    # everything else per level (a level's own running-statistics update is not observable: the module's buffers hold both)
    for lv in (a, b):
        r = R.forward_ref(lv["raw"], lv["gamma"], lv["beta"], R.EPS, None, None, None, 0.1, True, gate=lv.get("gate"), L=lv["L"])
        s = R.stat_bounds(r, lv["gamma"], lv["beta"], R.EPS, lv["M"])
        for what, got, key in (("save mean", lv["save"][0], "mean"), ("save invstd", lv["save"][1], "invstd"), ("scale", lv["ss"][0], "scale"),
                               ("shift", lv["ss"][1], "shift")):
            check("1 shared module stats", what, got, r[key], s[key])
        check("1 shared module end to end", "out", lv["out"], r["out"], R.out_bound(r, s, lv["raw"], dt))


@DTS
def test_top_down_chain_in_one_launch_with_66_33_and_16_5_slabs(dt):
    """B = 33, L = (256, 128, 64): the whole chain in ONE launch against float64 and, bit for bit, against one launch per level."""
    from drn_amd import ops
    B, Ls, C = 33, (256, 128, 64), 128
    assert [B * L / 128 for L in Ls] == [66, 33, 16.5] and not R.merge_is_cached(B * Ls[0]) and R.merge_is_cached(B * Ls[1])

    def run(one_launch):
        lvs = [train_level(B * L, C, dt, seed=20 + i, L=L) for i, L in enumerate(Ls)]
        for l in range(2):
            lvs[l]["up"], lvs[l]["ld_up"] = lvs[l + 1]["out"], C
        if one_launch:
            ops.bn_train_apply(lvs, C, code_of(dt))
        else:
            for l in (2, 1, 0):
                ops.bn_train_apply([lvs[l]], C, code_of(dt))
        torch.cuda.synchronize()
        return lvs
    one, per = run(True), run(False)
    for l in range(3):
        for k in ("out_full", "ss", "save", "running_mean", "running_var"):
            assert torch.equal(one[l][k], per[l][k]), "level %d: %s differs from the one-launch-per-level result" % (l, k)
    # float64, coarse to fine, with the kernel's own scale / shift; every level rounds its output once and adds the coarser one's
    ref_up, bnd_up = None, None
    for l in (2, 1, 0):
        lv = one[l]
        x, M, L = lv["raw"], lv["M"], lv["L"]
        y = (x.double() * lv["ss"][0].double() + lv["ss"][1].double()).clamp_min(0.0)
        ref = y if ref_up is None else y + R.upsample2(ref_up, B, L)
        bnd = R.apply_bound(x, lv["ss"][0], lv["ss"][1], ref, dt, up=None if ref_up is None else R.upsample2(ref_up, B, L))
        if bnd_up is not None:
            bnd = bnd + R.upsample2(bnd_up, B, L)
        check("1 chain apply", "out level %d" % l, lv["out"], ref, bnd)
        ref_up, bnd_up = ref, bnd
        r = R.forward_ref(x, lv["gamma"], lv["beta"], R.EPS, None, None, None, 0.1, True)
        s = R.stat_bounds(r, lv["gamma"], lv["beta"], R.EPS, M)
        check("1 chain stats", "scale level %d" % l, lv["ss"][0], r["scale"], s["scale"])
        check("1 chain stats", "shift level %d" % l, lv["ss"][1], r["shift"], s["shift"])


@DTS
def test_row_loop_of_more_than_one_trip_beyond_4096_workgroups(dt):
    """The smallest M * C that crosses 4096 workgroups at C = 128: rows_wg = 8 * RP, the `for (mb ...)` loop runs twice and calls
    load_batch again; M is ragged against rows_wg (two rows over)."""
    from drn_amd import ops
    C = 128
    M = 131074 if dt == F32 else 262146
    rp4 = 4 * R.rows_per_pass(dt)
    assert R.train_apply_rows_wg([M - 2], C, dt) == rp4 and R.train_apply_rows_wg([M], C, dt) == 2 * rp4 and M % (2 * rp4) == 2
    lv = train_level(M, C, dt, seed=31, L=2, up=True, gate=True)
    rm0, rv0 = lv["running_mean"].clone(), lv["running_var"].clone()
    ops.bn_train_apply([lv], C, code_of(dt))
    torch.cuda.synchronize()
    verify_train_level(lv, C, dt, rm0, rv0, "1 multi-trip")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. epilogue statistics on exact accumulators
# ---------------------------------------------------------------------------------------------------------------------------------
# kernel, dtype, M, N, Cin, taps, L, tuning.  M = 8320 + 57 (66 slabs, a last slab of 57 rows) where the kernel takes it; the 4-wave
# kernels want M % 256 == 0 (drn_nt_w4c_eligible / drn_nt_w4h_eligible), so they get the smallest such M above 64 slabs, 8448 = 66 slabs.
# The 128 x 128 tile writes into a buffer whose rows are 8 elements longer than N (and N = 192 / 320 end inside a tile).
EPI_CASES = [("tile128", F32, 8377, 192, 64, 1, None, {"nt_w4h": 0, "nt_w4c": 0}),
             ("tile128", BF16, 8377, 192, 64, 1, None, {"nt_w4h": 0, "nt_w4c": 0}),
             ("tile256", F32, 8377, 320, 64, 1, None, {"exp0": 1}),
             ("tile256", BF16, 8377, 320, 64, 1, None, {"exp0": 1}),
             ("w4c", BF16, 8448, 256, 64, 3, 128, {"exp0": 1, "nt_w4c": 1}),
             ("w4h", BF16, 8448, 128, 128, 1, None, {"nt_w4h": 1})]


@pytest.mark.parametrize("kernel,dt,M,N,Cin,taps,L,tuning", EPI_CASES, ids=["%s-%s" % (c[0], "f32" if c[1] == F32 else "bf16") for c in EPI_CASES])
def test_epilogue_statistics_on_exact_accumulators(monkeypatch, kernel, dt, M, N, Cin, taps, L, tuning):
    from drn_amd import ops
    assert R.slabs(M) == 66 and not R.merge_is_cached(M)
    A, W, P = R.exact_gemm_case(M, Cin, N, taps=taps, L=L)
    Ad, Wd, Pd = A.to(DEV, dt), W.to(DEV, dt), P.to(DEV)
    for k, v in tuning.items():
        tune(monkeypatch, k, v)
    ld_extra = 8 if kernel == "tile128" else 0
    Cfull = torch.full((M, N + ld_extra), float("nan"), device=DEV, dtype=dt)
    Cout = Cfull[:, :N]
    stats = torch.full((R.slabs(M), 2, N), float("nan"), device=DEV)
    d = ops.gemm_desc(Ad, Wd, Cout, M, N, Cin, taps=taps, pad=taps // 2, Lout=M if L is None else L, Lsrc=M if L is None else L, stats=stats,
                      ldc=N + ld_extra)
    want_kind = {"tile128": ops.NT_KIND_TILE128, "tile256": ops.NT_KIND_TILE256, "w4c": ops.NT_KIND_W4C, "w4h": ops.NT_KIND_W4H}[kernel]
    assert ops.gemm_nt_plan([d], code_of(dt)) == want_kind
    ops.gemm_nt([d], code_of(dt))
    torch.cuda.synchronize()
    # the accumulators are exact: the stored product is the float64 product (rounded once to bf16 where that is the type)
    assert torch.equal(Cout.double(), Pd.to(dt).double()), "the product is not exact: max |d| = %g" % float((Cout.double() - Pd).abs().max())
    assert bool(torch.isnan(Cfull[:, N:].float()).all()), "columns past N were written"
    s, ds, m2, dm2 = R.slab_bounds(Pd)
    check("2 slab pairs", "%s sum" % kernel, stats[:, 0], s, ds)
    check("2 slab pairs", "%s M2" % kernel, stats[:, 1], m2, dm2)
    # ... and merged by drn_bn_train_apply (statistics OF the accumulators, applied to the stored rows)
    lv = train_level(M, N, dt, seed=41, L=M, ld_extra=ld_extra, raw=Cfull, stats=stats)
    rm0, rv0 = lv["running_mean"].clone(), lv["running_var"].clone()
    ops.bn_train_apply([lv], N, code_of(dt))
    torch.cuda.synchronize()
    verify_train_level(lv, N, dt, rm0, rv0, "2 merged", stats_of=Pd)


@DTS
def test_tagged_merge_of_the_one_launch_conv_bn_kernel_above_64_slabs(monkeypatch, dt):
    """ops.conv_bn_train with BN_FUSE on, 66 slabs: the wait loop on tagged pairs that bn_merge_cols takes when a thread's pairs no
    longer fit its registers -- bit-identical to drn_gemm_nt + drn_bn_train_apply (as tests/test_conv_bn_gpu.py holds it below 64
    slabs), no watchdog, and within the float64 bounds."""
    from drn_amd import ops
    B, L, N, Cin = 66, 128, 128, 64
    M = B * L
    assert R.slabs(M) == 66 and not R.merge_is_cached(M)
    A, W, P = R.exact_gemm_case(M, Cin, N, taps=3, L=L)
    Ad, Wd, Pd = A.to(DEV, dt), W.to(DEV, dt), P.to(DEV)
    tune(monkeypatch, "nt_w4h", 0)             # the two-launch side on the general tile, whose statistics order the fused kernel shares
    tune(monkeypatch, "nt_w4c", 0)
    ops.conv_bn_train_timeouts()

    def run(fused):
        Cout = torch.full((M, N), float("nan"), device=DEV, dtype=dt)
        stats = torch.full((R.slabs(M), 2, N), float("nan"), device=DEV)
        lv = train_level(M, N, dt, seed=51, L=L, gate=True, raw=Cout, stats=stats)
        d = ops.gemm_desc(Ad, Wd, Cout, M, N, Cin, taps=3, pad=1, Lout=L, Lsrc=L, stats=None if fused else stats)
        launched = True
        if fused:
            monkeypatch.setattr(ops, "BN_FUSE", True)
            launched = ops.conv_bn_train([d], [lv], code_of(dt), relu=True)
            monkeypatch.setattr(ops, "BN_FUSE", False)
        else:
            ops.gemm_nt([d], code_of(dt))
            ops.bn_train_apply([lv], N, code_of(dt))
        torch.cuda.synchronize()
        return launched, Cout, lv
    init = train_level(M, N, dt, seed=51, L=L, raw=torch.zeros(M, N, device=DEV, dtype=dt), stats=torch.zeros(66, 2, N, device=DEV))
    rm0, rv0 = init["running_mean"], init["running_var"]              # (the same seed: what both runs start from)
    ok, Cf, f = run(True)
    _, Cp, p = run(False)
    assert ops.conv_bn_train_timeouts() == 0
    assert torch.equal(Cp.double(), Pd.to(dt).double())
    verify_train_level(p, N, dt, rm0, rv0, "2 conv+bn two launches", stats_of=Pd)
    # 66 workgroups of the 128 x 128 tile, one K-split: the launcher takes this launch on an MI355X (a decline would leave the tagged
    # wait loop above 64 slabs unrun, so it is a failure here, with the library's reason)
    from drn_amd import _lib
    assert ok, "drn_conv_bn_train declined: %s" % _lib.lib().drn_last_error().decode()
    assert torch.equal(Cf, Cp), "raw conv output differs"
    for k in ("out_full", "gated_full", "ss", "save", "running_mean", "running_var"):
        assert torch.equal(f[k], p[k]), "%s differs from the two-launch result" % k
    verify_train_level(f, N, dt, rm0, rv0, "2 conv+bn one launch", stats_of=Pd)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. backward, C % 64 == 0
# ---------------------------------------------------------------------------------------------------------------------------------
def bwd_levels(Ms, C, dt, seed, ld_extra=0, shared=True):
    """tests/test_bn_bwd_one_gpu.py's _levels on bn_ref.columns: scale_shift and save computed in float64 from the stored values."""
    gamma, beta = R.affine(C, seed + 90)
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    lv = []
    for i, M in enumerate(Ms):
        ld = C + ld_extra
        raw = R.columns(M, C, dt, seed + i, ld=ld, fill=7.0).to(DEV)
        dout = torch.cat([rnd(M, C, seed=seed + 40 + i), torch.full((M, ld_extra), 7.0)], 1).to(DEV, dt)
        x = raw[:, :C].double()
        mean, var = x.mean(0), x.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + R.EPS)
        g = gamma if shared or i == 0 else (R.affine(C, seed + 95 + i)[0]).to(DEV)
        sc = (g.double() * invstd).float()
        sh = (beta.double() - mean * g.double() * invstd).float()
        lv.append(dict(raw=raw, dout=dout, ss=torch.cat([sc, sh]).contiguous(), save=torch.cat([mean.float(), invstd.float()]).contiguous(),
                       gamma=g, M=M, ld=ld))
    return lv


def plan_bytes(Ms, C, dt, gb_L=None):
    """drn_bn_bwd_one_ws_bytes: > 0 when the one-launch plan takes the launch."""
    from drn_amd import _lib
    arr = (_lib.BnBwdDesc * len(Ms))()
    for d, M in zip(arr, Ms):
        d.M = M
        if gb_L:
            d.gb_dg, d.gb_L = 1, gb_L               # (only looked at for being non-null)
    return int(_lib.lib().drn_bn_bwd_one_ws_bytes(arr, len(Ms), C, code_of(dt)))


def one_launches():
    """launches of drn_bn_bwd_one so far: the generation words of its tagged workspaces (one per size and stream) advance by one each."""
    from drn_amd import ops
    torch.cuda.synchronize()
    return sum(int(t[0].item()) for k, t in ops._persistent.items() if isinstance(k[0], tuple) and k[0][0] == "bn_bwd_one")


def verify_backward(lv, C, dt, shared, ld_extra, group, inplace=False, ones=(True, False)):
    """relu = True through the one-launch kernel (where the plan takes it) and the two launches: the suite's tolerance formulas
    (tests/test_bn_bwd_one_gpu.py) against float64 and between the two, bn_ref.draw_bound per element, and the special columns."""
    from drn_amd import ops
    Ms = [v["M"] for v in lv]
    rows = sum(Ms)
    want, dg_l, db_l = R.backward_ref(lv, C, True, False)          # per level: the bound needs these; a shared module sums them
    dg_w, db_w = ([sum(dg_l)], [sum(db_l)]) if shared else (dg_l, db_l)
    fits = plan_bytes(Ms, C, dt) > 0
    runs = {}
    for one in ones:                                               # ... and each run took the path it is named after
        n0 = one_launches()
        runs[one] = _run(lv, C, dt, True, shared, one=one, inplace=inplace)
        assert one_launches() - n0 == (1 if one and fits else 0), "BN_BWD_ONE = %s, plan fits = %s" % (one, fits)
    lin = {one: _run(lv, C, dt, False, shared, one=one) for one in ones}           # relu = False, for the relu_on column
    assert ops.bn_bwd_one_timeouts() == 0
    off, on, ofs = (R.kind_index(C, k).to(DEV) for k in ("relu_off", "relu_on", "offset"))
    tol = 2e-2 if dt == BF16 else 1e-4
    for one, (got, dg, db, full) in runs.items():
        tag = "%s %s" % (group, "one launch" if one else "two launches")
        for i, (a, w) in enumerate(zip(got, want)):
            check(tag + " (suite formula)", "draw level %d" % i, a, w, tol * max(1.0, float(w.abs().max())))
            bound = R.draw_bound(lv[i], C, True, dg_l[i], db_l[i], Ms[i], dt)
            check(tag, "draw level %d" % i, a, w, bound)
            check(tag + " offset columns", "draw level %d" % i, a[:, ofs], w[:, ofs], bound[:, ofs])
            assert bool((a[:, off] == 0).all()), "relu_off: draw must be exactly 0"
            assert torch.equal(a[:, on], lin[one][0][i][:, on]), "relu_on: draw must equal the relu = False result"
        for a, w in zip(dg + db, dg_w + db_w):
            check(tag + " (suite formula)", "dgamma / dbeta", a, w, R.sum_tol(rows) * max(1.0, float(w.abs().max())))
            assert bool((a[off] == 0).all()), "relu_off: dgamma == dbeta == 0"
        for a, b in zip(dg + db, lin[one][1] + lin[one][2]):
            assert torch.equal(a[on], b[on]), "relu_on: dgamma / dbeta must equal the relu = False result"
        if ld_extra:                                  # columns past C belong to somebody else (draw starts as zeros, or as dout in place)
            for f, v in zip(full, lv):
                assert bool((f[:, C:] == (7.0 if inplace else 0.0)).all())
    if len(runs) == 2:                                # the one-launch result against the two-launch result, as the existing test does
        for a, b, w in zip(runs[True][0], runs[False][0], want):
            wmax = float(w.abs().max())
            check(group + " one vs two (suite formula)", "draw", a.float(), b.float(), wmax * 2 ** -7 if dt == BF16 else 1e-5 * max(1.0, wmax))
        for a, b, w in zip(runs[True][1] + runs[True][2], runs[False][1] + runs[False][2], dg_w + db_w):
            check(group + " one vs two (suite formula)", "dgamma / dbeta", a, b, R.sum_tol(rows) * max(1.0, float(w.abs().max())))
    return runs


@DTS
@pytest.mark.parametrize("Ms,C,ld_extra", [((8193,), 64, 0), ((16500,), 128, 64), ((32768, 16384, 8192), 256, 0)])
def test_backward_above_64_slabs(dt, Ms, C, ld_extra):
    lv_plan, arows = R.bwd64_rrows_arows(Ms, C, dt)
    rp4 = 4 * R.rows_per_pass(dt)
    assert arows == rp4 and all(rb <= 64 for _, rb, _ in lv_plan)
    if Ms == (32768, 16384, 8192):                     # 448-row reduce blocks would make 74 of level 0 in fp32: enlarged to 512 rows
        assert [big for _, _, big in lv_plan] == [dt == F32, False, False] and lv_plan[0][:2] == (512, 64)
    elif Ms == (8193,):
        assert lv_plan[0][2] and lv_plan[0][1] == (43 if dt == F32 else 33)
    # the one-launch kernel takes 8193 rows in both types; 16500 and the pyramid only in bf16 (fp32 row blocks end at 256 rows: 65 and
    # 128 of them) -- there BN_BWD_ONE on falls back to the two launches
    fits = R.bwd_one_fits(Ms, C, dt)
    assert fits == (dt == BF16 or Ms == (8193,)) and (plan_bytes(Ms, C, dt) > 0) == fits
    lv = bwd_levels(Ms, C, dt, seed=7, ld_extra=ld_extra)
    verify_backward(lv, C, dt, True, ld_extra, "3 backward")


@DTS
def test_backward_in_place_above_64_slabs(dt):
    Ms, C = (16500,), 128
    lv = bwd_levels(Ms, C, dt, seed=9, ld_extra=64)
    a = verify_backward(lv, C, dt, True, 64, "3 backward in place", inplace=True)
    for one in (True, False):
        b = _run(lv, C, dt, True, True, one=one)
        for x, y in zip(a[one][0] + a[one][1] + a[one][2], b[0] + b[1] + b[2]):
            assert torch.equal(x, y), "in place differs from out of place"


def test_backward_apply_blocks_of_8_rp_rows_and_the_plan_that_declines():
    """The smallest m_all * (C / 64) / (4 * RP) above 4096 (fp32, C = 64): arows = 8 * RP, M ragged against it, 64 enlarged reduce
    blocks -- and more row blocks than the one-launch plan takes, so ops.bn_bwd_multi falls back with BN_BWD_ONE on."""
    dt, C, M = F32, 64, 262209
    lv_plan, arows = R.bwd64_rrows_arows([M], C, dt)
    assert R.bwd64_rrows_arows([M - 65], C, dt)[1] == 64 and arows == 128 and M % arows == 65 and lv_plan == [(4160, 64, True)]
    assert plan_bytes([M], C, dt) == 0
    lv = bwd_levels((M,), C, dt, seed=13)
    runs = verify_backward(lv, C, dt, True, 0, "3 backward 8*RP")
    for x, y in zip(runs[True][0] + runs[True][1] + runs[True][2], runs[False][0] + runs[False][1] + runs[False][2]):
        assert torch.equal(x, y)                        # both are the two launches


@DTS
def test_gate_backward_inside_the_launch_at_66_clips(dt, monkeypatch):
    """DrnBnBwdDesc::gb_* at B = 66, L = 128, C = 256 (8448 rows, 66 slabs), handed to ops.bn_bwd_multi inside the level (`gb`) and as
    a drn_gate_bwd launch of the caller's own, each with BN_BWD_ONE on and off -- four runs, three kernels paths:
      gb, on:   bf16: the GATED one-launch kernel (256-row blocks).  fp32: its plan declines (66 blocks of 128 rows are too many and
                256 rows are more passes than the gated variant holds), ops runs drn_gate_bwd itself and asks again without gb_*:
                the PLAIN one-launch kernel takes it (33 blocks of 256 rows)
      gb, off:  drn_gate_bwd from ops + the two launches (drn_bn_bwd_multi)
      separate, on / off: drn_gate_bwd from here + the plain one-launch kernel / the two launches
    Which path a run took is asserted (both plans, and the one-launch generation count); every run against float64 with the
    suite's formulas (tests/test_bn_bwd_one_gpu.py), and against the others."""
    from drn_amd import ops
    B, L, C = 66, 128, 256
    M = B * L
    code = code_of(dt)
    gated_fits, plain_fits = plan_bytes([M], C, dt, gb_L=L) > 0, plan_bytes([M], C, dt) > 0
    assert R.slabs(M) == 66 and gated_fits == (dt == BF16) and plain_fits and R.bwd_one_fits([M], C, dt)
    v = bwd_levels((M,), C, dt, seed=11)[0]
    raw, ss, save, gamma = v["raw"], v["ss"], v["save"], v["gamma"]
    dG = rnd(M, C, seed=21).to(DEV, dt)
    add = rnd(M, C, seed=22).to(DEV, dt)
    gate = (rnd(B, C, seed=23) * 0.5 + 1.0).to(DEV)
    act = torch.empty((M, C), device=DEV, dtype=dt)
    ops.bn_apply(raw, C, ss, act, C, M, C, L, code, relu=True)

    def run(inside, one):
        dgate = torch.full((B, C), float("nan"), device=DEV)
        dgamma, dbeta = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        draw = torch.full((M, C), float("nan"), device=DEV, dtype=dt)
        level = dict(dout=add, ld_dout=C, raw=raw, ld_raw=C, ss=ss, save=save, gamma=gamma, draw=draw, ld_draw=C, dgamma=dgamma, dbeta=dbeta,
                     accumulate=False, M=M)
        if inside:
            level["gb"] = dict(dg=dG, ld_dg=C, gate=gate, ldg=C, dgate=dgate, L=L, act=act, ld_act=C)
        else:
            d = torch.empty((M, C), device=DEV, dtype=dt)
            ops.gate_bwd(dG, C, act, C, gate, d, C, add, C, dgate, B, L, C, code)
            level["dout"] = d
        monkeypatch.setattr(ops, "BN_BWD_ONE", one)
        n0 = one_launches()
        ops.bn_bwd_multi([level], C, code, relu=True)
        assert one_launches() - n0 == (1 if one else 0), "inside = %s, BN_BWD_ONE = %s" % (inside, one)
        # (ops.bn_bwd_multi replaces `gb` by the gradient drn_gate_bwd wrote when it had to run that launch itself)
        assert (level.get("gb") is not None) == (inside and one and gated_fits)
        return draw, dgate, dgamma, dbeta
    runs = {(inside, one): run(inside, one) for inside in (True, False) for one in (True, False)}
    assert ops.bn_bwd_one_timeouts() == 0
    # float64: dout_eff = T(add + dG * gate[clip]) -- every path rounds it to the storage type before the BatchNorm backward reads it --,
    # dgate = sum_t dG * act; then the BatchNorm backward of dout_eff
    eff = (add.double() + dG.double() * gate.double().repeat_interleave(L, dim=0)).to(dt)
    want, dg_w, db_w = R.backward_ref([dict(v, dout=eff)], C, True, True)
    ref_gate = (dG.double() * act.double()).view(B, L, C).sum(1)
    tol = 2e-2 if dt == BF16 else 1e-4
    for (inside, one), r in runs.items():
        tag = "%s, BN_BWD_ONE %s" % ("gb" if inside else "separate", "on" if one else "off")
        check("3 gate backward (suite formula)", "draw " + tag, r[0], want[0], tol * max(1.0, float(want[0].abs().max())))
        check("3 gate backward (suite formula)", "dgate " + tag, r[1], ref_gate, 3e-5 * max(1.0, float(ref_gate.abs().max())) * max(1.0, L ** 0.5 / 4))
        for x, w in zip(r[2:], dg_w + db_w):
            check("3 gate backward (suite formula)", "dgamma / dbeta " + tag, x, w, R.sum_tol(M) * max(1.0, float(w.abs().max())))
    base = runs[(False, False)]                        # the caller's drn_gate_bwd + the two launches: the others against it
    scale = max(1.0, float(base[0].float().abs().max()))
    for key, r in runs.items():
        if key == (False, False):
            continue
        tag = "%s / %s vs separate / off" % ("gb" if key[0] else "separate", "on" if key[1] else "off")
        check("3 gate backward, path vs path (suite formula)", "draw " + tag, r[0].float(), base[0].float(), (2.0 ** -7 if dt == BF16 else 2e-5) * scale)
        check("3 gate backward, path vs path (suite formula)", "dgate " + tag, r[1], base[1],
              3e-5 * max(1.0, float(ref_gate.abs().max())) * max(1.0, L ** 0.5 / 4))
        for x, y in zip(r[2:], base[2:]):
            check("3 gate backward, path vs path (suite formula)", "dgamma / dbeta " + tag, x, y, R.sum_tol(M) * max(1.0, float(y.abs().max())))
    # the same kernels on the same inputs: the same bits (drn_gate_bwd from ops or from here, then the two launches)
    for x, y in zip(runs[(True, False)], runs[(False, False)]):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. C % 64 != 0: the three-launch backward and row_grid
# ---------------------------------------------------------------------------------------------------------------------------------
ODD_C = {F32: 36, BF16: 72}                             # nine 16-byte vectors per row either way: row_grid's unit is 9 blocks


@DTS
@pytest.mark.parametrize("M", [3, 300, 4096, 70001])
def test_three_launch_backward_with_ragged_block_counts(dt, M):
    """ops.bn_bwd where C % 64 != 0 (today only the query encoder's (B, C) BatchNorm gets here): 1, 18 and 256 partial-sum blocks --
    the finalize kernel's unrolled loop (four blocks per lane and trip) and its tail --, rows that do not fill the last block, and
    at 70001 rows four passes of the apply kernel's stride loop."""
    from drn_amd import ops
    C = ODD_C[dt]
    nvec = C // (8 if dt == BF16 else 4)
    assert C % 64 != 0 and nvec == 9
    assert R.bwd3_nblk([M], C, dt)[0] == {3: 1, 300: 18, 4096: 256, 70001: 256}[M]
    assert R.row_grid_blocks(M, nvec)[1] == {3: 1, 300: 2, 4096: 4, 70001: 4}[M] and not R.row_grid_blocks(M, nvec)[2]
    ld = C + 8
    v = bwd_levels((M,), C, dt, seed=17, ld_extra=8)[0]
    want, dg_w, db_w = R.backward_ref([v], C, True, True)
    lin_w, _, _ = R.backward_ref([v], C, False, True)
    outs = {}
    for relu in (True, False):
        draw = torch.full((M, ld), float("nan"), device=DEV, dtype=dt)
        dgamma, dbeta = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
        ops.bn_bwd(v["dout"][:, :C], ld, v["raw"][:, :C], ld, v["ss"], v["save"], v["gamma"], draw[:, :C], ld, dgamma, dbeta, False, M, C,
                   code_of(dt), relu=relu)
        torch.cuda.synchronize()
        assert bool(torch.isnan(draw[:, C:].float()).all()), "columns past C were written"
        outs[relu] = (draw[:, :C], dgamma, dbeta)
    got, dgamma, dbeta = outs[True]
    tol = 2e-2 if dt == BF16 else 1e-4
    check("4 backward (suite formula)", "draw", got, want[0], tol * max(1.0, float(want[0].abs().max())))
    check("4 backward", "draw", got, want[0], R.draw_bound(v, C, True, dg_w[0], db_w[0], M, dt))
    check("4 backward (suite formula)", "draw, relu off", outs[False][0], lin_w[0], tol * max(1.0, float(lin_w[0].abs().max())))
    for a, w in ((dgamma, dg_w[0]), (dbeta, db_w[0])):
        check("4 backward (suite formula)", "dgamma / dbeta", a, w, R.sum_tol(M) * max(1.0, float(w.abs().max())))
    off, on = R.kind_index(C, "relu_off").to(DEV), R.kind_index(C, "relu_on").to(DEV)
    assert bool((got[:, off] == 0).all()) and bool((dgamma[off] == 0).all()) and bool((dbeta[off] == 0).all())
    assert torch.equal(got[:, on], outs[False][0][:, on]) and torch.equal(dgamma[on], outs[False][1][on]) and torch.equal(dbeta[on], outs[False][2][on])
    # accumulate = True adds to what is there
    base = rnd(C, seed=3).to(DEV)
    dg2, db2 = base.clone(), base.clone()
    draw = torch.empty((M, ld), device=DEV, dtype=dt)
    ops.bn_bwd(v["dout"][:, :C], ld, v["raw"][:, :C], ld, v["ss"], v["save"], v["gamma"], draw[:, :C], ld, dg2, db2, True, M, C, code_of(dt))
    torch.cuda.synchronize()
    assert torch.equal(dg2, base + dgamma) and torch.equal(db2, base + dbeta)


def apply_level(M, L, C, dt, seed, ld_extra=8):
    """One level of ops.bn_apply / bn_apply_multi on bn_ref.columns with the upsample add and the gate; scale_shift in float64 from the data."""
    ld = C + ld_extra
    v = bwd_levels((M,), C, dt, seed=seed, ld_extra=ld_extra)[0]
    B = M // L
    lv = dict(raw=v["raw"][:, :C], ld_raw=ld, ss=v["ss"], M=M, L=L, ld_out=ld, ld_up=ld, ld_gated=ld,
              out_full=torch.full((M, ld), float("nan"), device=DEV, dtype=dt), gated_full=torch.full((M, ld), float("nan"), device=DEV, dtype=dt),
              up=torch.cat([rnd(M // 2, C, seed=seed + 5), torch.full((M // 2, ld_extra), 7.0)], 1).to(DEV, dt)[:, :C],
              gate=torch.cat([rnd(B, C, seed=seed + 6, scale=0.5) + 1.0, torch.full((B, 4), 7.0)], 1).to(DEV)[:, :C])
    lv["out"], lv["gated"] = lv["out_full"][:, :C], lv["gated_full"][:, :C]
    return lv


def verify_apply_level(lv, C, dt, group):
    x, M, L = lv["raw"], lv["M"], lv["L"]
    sc, sh = lv["ss"][:C], lv["ss"][C:]
    k = R.forward_ref(x, sc, sh, R.EPS, None, None, None, 0.1, True, up=lv["up"], gate=lv["gate"], L=L, scale_shift=(sc, sh))
    up2, g2 = R.upsample2(lv["up"], M // L, L), lv["gate"].repeat_interleave(L, dim=0)
    check(group, "out", lv["out"], k["out"], R.apply_bound(x, sc, sh, k["out"], dt, up=up2))
    check(group, "gated", lv["gated"], k["gated"], R.apply_bound(x, sc, sh, k["gated"], dt, up=up2, gate=g2))
    for name in ("out_full", "gated_full"):
        assert bool(torch.isnan(lv[name][:, C:].float()).all()), "%s: columns past C were written" % name


@DTS
@pytest.mark.parametrize("M,L", [(300, 20), (4096, 64), (70002, 6), (466034, 2)])
def test_apply_with_odd_channel_counts_up_to_the_block_cap(dt, M, L):
    """ops.bn_apply at C % 64 != 0 with the upsample add and the gate, against forward_ref fed the same scale_shift; 466034 rows of
    nine vectors are the fewest that want more than 4096 blocks (row_grid caps the grid; the stride loop makes up for it)."""
    from drn_amd import ops
    C = ODD_C[dt]
    blocks, passes, capped = R.row_grid_blocks(M, 9)
    assert capped == (M == 466034) and not R.row_grid_blocks(466033, 9)[2] and (blocks, passes) == {300: (9, 2), 4096: (36, 4), 70002: (621, 4),
                                                                                                  466034: (4104, 4)}[M]
    lv = apply_level(M, L, C, dt, seed=61)
    ops.bn_apply(lv["raw"], lv["ld_raw"], lv["ss"], lv["out"], lv["ld_out"], M, C, L, code_of(dt), up=lv["up"], ld_up=lv["ld_up"], gate=lv["gate"],
                 gated=lv["gated"], ld_gated=lv["ld_gated"], relu=True)
    torch.cuda.synchronize()
    verify_apply_level(lv, C, dt, "4 apply")


@DTS
@pytest.mark.parametrize("shapes", [[(4096, 64), (2048, 32), (300, 20)], [(466034, 2), (300, 20)]], ids=["three-levels", "capped"])
def test_apply_multi_with_odd_channel_counts(dt, shapes):
    """ops.bn_apply_multi: several levels in one launch, each with its own block range; one launch whose first level hits the cap."""
    from drn_amd import ops
    C = ODD_C[dt]
    assert R.row_grid_blocks(shapes[0][0], 9)[2] == (shapes[0][0] == 466034)
    lvs = [apply_level(M, L, C, dt, seed=71 + i) for i, (M, L) in enumerate(shapes)]
    ops.bn_apply_multi(lvs, C, code_of(dt), relu=True)
    torch.cuda.synchronize()
    for lv in lvs:
        verify_apply_level(lv, C, dt, "4 apply")
