"""tests/heads_ref.py checked without a GPU: the float64 model against nn.Conv1d + torch.exp autograd, the exactness of the data
under fp32 accumulation in any order, and the sensitivity of every geometry to the single faults it is listed for (heads_ref.FAULTS):
what tests/test_heads_gpu.py asserts would change if a kernel made that mistake."""
import functools

import pytest
import torch
import torch.nn.functional as F

import heads_ref as H

F32, BF16 = torch.float32, torch.bfloat16
NAMES = list(H.GEOMETRIES)


def test_geometry_table():
    """the row counts and block counts the table of heads_ref.GEOMETRIES promises"""
    rows = {n: H.total_rows(*H.geometry(n)) for n in NAMES}
    assert rows == {"one_run": 8, "short_tail": 11, "wrap": 24, "unit": 9, "ragged3": 264, "four": 60, "many_blocks": 4470}
    assert H.level_starts(*H.geometry("ragged3")) == [0, 150, 225]
    assert -(-rows["many_blocks"] // H.ROWS_PER_W_WG) == 70 and rows["many_blocks"] % H.ROWS_PER_W_WG != 0
    assert all(len(H.geometry(n)[1]) <= H.MAX_GROUPS for n in NAMES)
    assert sorted(len(H.geometry(n)[1]) for n in ("one_run", "ragged3", "four")) == [1, 3, 4]


@pytest.mark.parametrize("exp", [False, True], ids=["linear", "exp"])
@pytest.mark.parametrize("taps", [1, 3])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_conv1d_autograd(name, N, taps, exp):
    """forward_ref / backward_ref against nn.Conv1d (+ torch.exp) autograd in float64, level by level, 1e-12 relative"""
    c = H.exact_case(name, 8, N, taps, exp, F32, seed=1)
    B, Ls = c["B"], c["Ls"]
    xs = [x.clone().requires_grad_() for x in c["xs"]]
    W, bias = c["W"].clone().requires_grad_(), c["bias"].clone().requires_grad_()
    sc = c["scales"].clone().requires_grad_() if exp else None
    zs = [F.conv1d(x.permute(0, 2, 1), W, bias, padding=(taps - 1) // 2).permute(0, 2, 1) for x in xs]       # (B, L, N)
    outs = [torch.exp(sc[l] * z) if exp else z for l, z in enumerate(zs)]
    (H.flat(outs) * c["dout"]).sum().backward()
    f = H.forward_ref(c["xs"], c["W"], c["bias"], c["scales"])
    b = H.backward_ref(c["xs"], c["W"], c["dout"], out=f["out"], z=f["z"], scales=c["scales"])

    def close(got, want, what):
        tol = 1e-12 * max(float(want.abs().max()), 1.0)
        assert got.shape == want.shape and float((got - want).abs().max()) <= tol, what
    close(f["z"], H.flat(zs).detach(), "z")
    close(f["out"], H.flat(outs).detach(), "out")
    for l in range(len(Ls)):
        close(b["dX"][l], xs[l].grad, "dX level %d" % l)
    close(b["dW"], W.grad, "dW")
    close(b["dbias"], bias.grad, "dbias")
    if exp:
        close(b["dscale"], sc.grad, "dscale")
    # the sums of absolute terms bound their sums, and the old values of the accumulate modes are plain further terms
    assert bool((f["z_abs"] >= f["z"].abs()).all()) and bool((b["dW_abs"] >= b["dW"].abs()).all())
    a = H.backward_ref(c["xs"], c["W"], c["dout"], out=f["out"], z=f["z"], scales=c["scales"], dx0=c["dx0"], dW0=c["dW0"],
                       db0=c["db0"], ds0=c["ds0"])
    for l in range(len(Ls)):
        close(a["dX"][l], b["dX"][l] + c["dx0"][l], "dX + dx0")
    close(a["dW"], b["dW"] + c["dW0"], "dW + dW0")
    close(a["dbias"], b["dbias"] + c["db0"], "dbias + db0")
    if exp:
        close(a["dscale"], b["dscale"] + c["ds0"], "dscale + ds0")


@pytest.mark.parametrize("name,C", [("ragged3", 520), ("many_blocks", 64)])
def test_fp32_sums_are_exact_in_any_order(name, C):
    """The linear-mode data: z, dX, dW and dbias accumulated in float32, term by term in three random orders, equal the float64 model
    bit for bit (ragged3 at the widest C of the GPU tests; many_blocks at their largest row count)."""
    c = H.exact_case(name, C, 2, 3, False, BF16, seed=2)
    X, W, dout = H.flat(c["xs"]), c["W"], c["dout"]
    f = H.forward_ref(c["xs"], W, c["bias"])
    b = H.backward_ref(c["xs"], W, dout, dx0=c["dx0"], dW0=c["dW0"], db0=c["db0"])
    pairs = H.tap_pairs(c["B"], c["Ls"], 3)
    R = c["R"]
    rows = [0, 149, 150, R - 1]                          # z: a few rows, every term (channel x tap) on its own
    for seed in range(3):
        for r in rows:
            terms = [c["bias"][None, :]]
            for tap, (dst, src) in enumerate(pairs):
                hit = (dst == r).nonzero()
                if hit.numel():
                    terms.append(X[src[hit[0, 0]], :, None] * W[:, :, tap].t())           # (C, N)
            got = H.fp32_sum_any_order(torch.cat(terms), seed)
            assert torch.equal(got.double(), f["z"][r]), "z row %d" % r
        # dW[n, c, tap], channels 0..7: one term per row, plus the old value
        for tap, (dst, src) in enumerate(pairs):
            terms = torch.cat([dout[dst][:, :, None] * X[src][:, None, :8], c["dW0"][None, :, :8, tap]])     # (rows + 1, N, 8)
            assert torch.equal(H.fp32_sum_any_order(terms, seed).double(), b["dW"][:, :8, tap]), "dW tap %d" % tap
        got = H.fp32_sum_any_order(torch.cat([dout, c["db0"][None]]), seed)
        assert torch.equal(got.double(), b["dbias"])
        # dX of a few rows, channels 0..7: N x taps terms plus the old value
        dX, dx0 = H.flat(b["dX"]), H.flat(c["dx0"])
        for r in rows:
            terms = [dx0[r, None, :8]]
            for tap, (dst, src) in enumerate(pairs):
                for d in dst[src == r].tolist():
                    terms.append(dout[d][:, None] * W[:, :8, tap])
            assert torch.equal(H.fp32_sum_any_order(torch.cat(terms), seed).double(), dX[r, :8]), "dX row %d" % r


@functools.lru_cache(maxsize=None)
def _sens_case(name, C, N, taps, exp):
    c = H.exact_case(name, C, N, taps, exp, F32, seed=3)
    f = H.forward_ref(c["xs"], c["W"], c["bias"], c["scales"])
    b = H.backward_ref(c["xs"], c["W"], c["dout"], out=f["out"], z=f["z"], scales=c["scales"], dx0=c["dx0"])
    return c, f, b


def _changed(name, fault, C, N, taps, exp):
    """the asserted outputs (as test_heads_gpu.py compares them: exactly in linear mode, beyond their bounds in exp mode) that the
    single-fault variant of the model moves"""
    c, f, b = _sens_case(name, C, N, taps, exp)
    ff = H.forward_ref(c["xs"], c["W"], c["bias"], c["scales"], fault=fault)
    fb = H.backward_ref(c["xs"], c["W"], c["dout"], out=ff["out"], z=ff["z"], scales=c["scales"], dx0=c["dx0"], fault=fault)
    R, nl = c["R"], len(c["Ls"])
    bounds = dict(z=0.0, out=0.0, dX=0.0, dW=0.0, dbias=0.0, dscale=0.0)
    if exp:
        bounds = dict(z=0.0, out=H.out_bound(f["sz"]), dX=H.dx_bound(H.flat(b["dX_abs"]), H.flat(b["dX"]), N, taps, F32),
                      dW=H.sum_bound(b["dW_abs"], R + 2), dbias=H.sum_bound(b["dbias_abs"], R + 1),
                      dscale=torch.stack([H.sum_bound(b["dscale_abs"][l], N * c["B"] * c["Ls"][l] + 2) for l in range(nl)]))
    changed = []
    for k in ("z", "out"):
        if H.differs(ff[k], f[k], bounds[k]):
            changed.append(k)
    for k in ("dX", "dW", "dbias") + (("dscale",) if exp else ()):
        got, want = (H.flat(fb[k]), H.flat(b[k])) if k == "dX" else (fb[k], b[k])
        if H.differs(got, want, bounds[k]):
            changed.append(k)
    return changed


SENS = [(fault, name) for fault in H.FAULTS for name in H.FAULTS[fault]]


@pytest.mark.parametrize("fault,name", SENS, ids=["%s-%s" % s for s in SENS])
def test_single_faults_show(fault, name):
    """Every single-fault variant of the model moves at least one asserted output on every geometry listed as reaching that path --
    and the outputs one would expect: both directions for the masks, the sums for the dropped row blocks."""
    N, taps = 2, 3
    C = 260 if fault == "chan64" else 8                      # 65 fp32 vectors: one lane of the second pass
    for exp in ((True,) if fault == "scale0" else (False, True)):
        ch = _changed(name, fault, C, N, taps, exp)
        assert ch, "%s on %s (%s) changes nothing a test asserts" % (fault, name, "exp" if exp else "linear")
        if fault in ("noclip", "nolevel", "chan64", "swap"):
            assert "out" in ch and "dX" in ch and "dW" in ch, ch
        elif fault == "lastrow":
            assert "out" in ch and "dX" in ch, ch
        elif fault == "blk64":
            assert "dW" in ch and "dbias" in ch and "out" not in ch and "dX" not in ch and (not exp or "dscale" in ch), ch
        elif fault == "scale0":
            assert "out" in ch and "z" not in ch, ch
        elif fault == "dx0":
            assert ch == ["dX"], ch


@pytest.mark.parametrize("fault", ["noclip", "nolevel", "blk64", "scale0"])
def test_faults_are_silent_elsewhere(fault):
    """...and the table is not padded: a fault is invisible on the geometries NOT listed for it (no clip boundary with one clip, no
    level boundary with one level, no row block past 64 below 4097 rows)."""
    for name in NAMES:
        if name in H.FAULTS[fault] or name == "many_blocks":
            continue
        assert _changed(name, fault, 8, 2, 3, True) == [], (fault, name)


def test_taps1_head_ignores_clip_faults():
    """a 1-tap head (iou_scores) has no neighbours: the mask faults cannot show there, the others do"""
    assert _changed("ragged3", "noclip", 8, 1, 1, False) == []
    assert _changed("ragged3", "lastrow", 8, 1, 1, False)
