"""tests/optim_ref.py checked without a GPU: the float64 model is clip_grad_norm_ + torch.optim.Adam, a step-by-step fp32 evaluation
of the kernels' formula sits inside the derived bound on every row of the case table while nine subtly wrong ones each leave it --
which is what makes tests/test_optim_kernels_gpu.py worth having --, and the bucket layout, tiled items and skip ranges of that file
reach every code path of drn_amd/csrc/optim.hip, with the predicates' thresholds read from its source text."""
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as R

N_CASE = 3000


def test_model_is_clip_grad_norm_and_torch_adam_in_float64():
    """6 steps from zero state on float64 CPU tensors; the gradient scale moves by 100 x so that clipping is active on some steps and
    idle on others.  m, v and p agree to 1e-12 of each tensor's largest magnitude."""
    rng = np.random.default_rng(0)
    shapes = [(37, 5), (11,), (1,), (4, 3, 3)]
    lr, b1, b2, eps, max_norm = R.f32(1e-2), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(2.0)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    state = [(np.zeros(s), np.zeros(s), p.detach().numpy().copy()) for s, p in zip(shapes, params)]
    clipped = []
    for t, scale in enumerate([1.0, 0.01, 1.0, 0.01, 0.05, 3.0], start=1):
        grads = [scale * rng.standard_normal(s) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        total = sum(float((g ** 2).sum()) for g in grads)
        tn = torch.nn.utils.clip_grad_norm_(params, max_norm)
        assert float(tn) == pytest.approx(np.sqrt(total), rel=1e-14)
        clipped.append(np.sqrt(total) > max_norm)
        opt.step()
        new = []
        for p, g, (m0, v0, p0) in zip(params, grads, state):
            m, v, pn = R.adam_model(g, m0, v0, p0, total, t, lr, b1, b2, eps, max_norm, 1.0)
            st = opt.state[p]
            for got, want in ((st["exp_avg"], m), (st["exp_avg_sq"], v), (p.detach(), pn)):
                got = got.numpy()
                assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max()), t
            new.append((m, v, pn))
        state = new
    assert any(clipped) and not all(clipped), clipped


def test_grad_scale_is_the_gradient_divided_before_everything_else():
    """adam_model(g, grad_scale = 1/8, norm of g / 8) is adam_model(g / 8, grad_scale = 1) exactly: 1/8 is a power of two."""
    (g, m0, v0, p0), kw = R.case_arrays(R.CASES[1], 500)
    assert kw["grad_scale"] == 0.125
    a = R.adam_model(g, m0, v0, p0, **kw)
    b = R.adam_model(g * np.float32(0.125), m0, v0, p0, **dict(kw, grad_scale=1.0))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def table():
    """{row: (arrays, kwargs, model, bound)} on N_CASE elements, computed once."""
    out = {}
    for row in R.CASES:
        arrays, kw = R.case_arrays(row, N_CASE)
        out[row] = (arrays, kw, R.adam_model(*arrays, **kw), R.adam_bound(*arrays, **kw))
    return out


def test_case_table_covers_what_it_says(table):
    assert sorted(set(r[0] for r in R.CASES)) == [1, 2, 10, 1000, 100000]
    assert set(r[1] for r in R.CASES) == {"off", "idle", "active"} and set(r[2] for r in R.CASES) == {1.0, 0.125}
    assert set(r[3] for r in R.CASES) == {"ordinary", "wide", "tiny", "zeros"}
    tiny = np.finfo(np.float32).tiny
    for row, ((g, m0, v0, p0), kw, (m, v, p), _) in table.items():
        t, clipping, gs, regime = row
        norm = np.sqrt(kw["total_sumsq"])
        coef = kw["max_norm"] / (norm + 1e-6) if kw["max_norm"] > 0 else None
        assert {"off": coef is None, "idle": coef is not None and coef > 1.5, "active": coef is not None and coef < 0.5}[clipping] \
            or regime == "zeros", row
        # every non-zero intermediate is a normal fp32 number: the smallest is (1 - beta2) * gh * gh
        gh = np.abs(g.astype(np.float64)) * gs * (min(1.0, coef) if coef is not None else 1.0)
        for x in (gh, (1 - R.f32(0.999)) * gh * gh, np.abs(m), v, 0.9 * np.abs(m0.astype(np.float64)), np.abs(p0 - p)):
            nz = x[x != 0]
            assert nz.size == 0 or float(nz.min()) >= tiny, row
        if regime == "tiny":                                      # eps decides: sqrt(v) is of its size or far below
            assert float(np.median(np.sqrt(v))) < 100 * kw["eps"]
        if regime == "zeros":
            assert np.array_equal(p, p0.astype(np.float64)) and not m.any() and not v.any()


def test_emulation_is_inside_the_bound_on_every_row(table):
    for row, (arrays, kw, (m, v, p), (dm, dv, dp)) in table.items():
        em, ev, ep = R.emulate_fp32(*arrays, **kw)
        ratios = [R.inside(em, m, dm), R.inside(ev, v, dv), R.inside(ep, p, dp)]
        print("emulation, %s: |err| / bound  m %.3g  v %.3g  p %.3g" % ((R.case_id(row),) + tuple(ratios)))
        assert max(ratios) <= 1.0, (row, ratios)
        if row[3] == "zeros":
            assert np.array_equal(ep, arrays[3]) and np.isfinite(ep).all()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_leaves_the_bound_on_some_row(table, mutant):
    caught = []
    for row, (arrays, kw, (m, v, p), (dm, dv, dp)) in table.items():
        em, ev, ep = R.emulate_fp32(*arrays, mutant=mutant, **kw)
        worst = max(R.inside(em, m, dm), R.inside(ev, v, dv), R.inside(ep, p, dp))
        if worst > 1.0:
            caught.append((R.case_id(row), worst))
    print("%s: outside the bound on %d of %d rows: %s" % (mutant, len(caught), len(R.CASES), ", ".join("%s (%.3g x)" % c for c in caught)))
    assert caught, mutant


def test_bound_carries_the_conditioning_of_the_bias_corrections():
    """At t = 1 the bound on p is dominated by POW_ULPS ulps of powf(beta2, 1) amplified by beta2 / (1 - beta2) ~ 1000 (halved by the
    square root); at t = 100000 the term is gone and the final subtraction's |p| U is what is left for a zero update."""
    assert R.pow_cond(0.999, 1) == pytest.approx(999.0, rel=1e-4) and R.pow_cond(0.9, 1) == pytest.approx(9.0, rel=1e-6)
    assert R.pow_cond(0.999, 100000) < 1e-40 and R.pow_cond(0.9, 100000) == 0.0
    g, m0, v0, p0 = (np.array([x], dtype=np.float32) for x in (1.0, 0.0, 0.0, 0.0))
    kw = dict(R.HYPER, total_sumsq=1.0, max_norm=0.0, grad_scale=1.0)
    m, v, p = R.adam_model(g, m0, v0, p0, t=1, **kw)
    assert float(p[0]) == pytest.approx(-R.f32(1e-3), rel=1e-6)                 # step 1 from zero state: lr * sign(g)
    dp1 = float(R.adam_bound(g, m0, v0, p0, t=1, **kw)[2][0]) / abs(float(p[0]))
    want = (2 * R.POW_ULPS * (9.0 + 999.0 / 2)) * R.U
    assert want < dp1 < want + 40 * R.U
    z = np.zeros(1, dtype=np.float32)
    dp = R.adam_bound(z, z, z, np.array([3.0], dtype=np.float32), t=100000, **kw)[2]
    assert float(dp[0]) == pytest.approx(3.0 * R.U * (1 + R.SECOND_ORDER), rel=1e-12)


# ---- the thresholds of the predicates against the source text ----------------------------------------------------------------------
def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, name)).read()


def test_thresholds_are_the_ones_in_the_source():
    src, hdr = _source("drn_amd/csrc/optim.hip"), _source("include/drn_hip.h")
    define = lambda txt, name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    assert define(src, "OPT_ELEMS_PER_BLOCK") == R.BLOCK and define(src, "OPT_THREADS") == R.THREADS
    assert define(hdr, "DRN_SUMSQ_MAX_SKIP") == R.MAX_SKIP and define(hdr, "DRN_SUMSQ_MAX_EXT") == R.MAX_EXT
    assert define(_source("drn_amd/csrc/common.h"), "DRN_BF16") == R.BF16
    k = define(src, "TILED_MAXK")
    assert k == 3 and max(it["k"] for it in R.tiled_items()) == k
    assert re.search(r"__shared__ float tile\[(\d+)\]\[(\d+) \* TILED_MAXK \+ 1\]", src).groups() == (str(R.TILE), str(R.TILE))
    assert int(re.search(r"constexpr int tcw = (\d+);", src).group(1)) == R.TILE
    assert len(re.findall(r"r0 = \(t / it\.tiles_c\) \* 64", src)) == 1 and len(re.findall(r"min\(64, it\.R - r0\)", src)) == 1
    assert re.search(r"constexpr int VEC = 16 / \(int\)sizeof\(T\);", src) and (R.vec_of(R.F32), R.vec_of(R.BF16)) == (16 // 4, 16 // 2)
    assert len(re.findall(r"<<<1, 1024, 0", src)) == 2 and len(re.findall(r"i \+= 1024\)", src)) == 3          # finalize_chain's 1024
    assert R.PARTIAL_CHAIN == 28 and R.finalize_chain(1025, (1500, 1)) == 2 + 2 + 1 + 14
    # the alignment tests of the update paths
    assert len(re.findall(r"& 15\) == 0", src)) == 5
    assert "const bool vec4 = (ts % 4 == 0) && (S % 4 == 0) && ((((uintptr_t)it.p) & 15) == 0) && (it.off % 4 == 0);" in src
    assert "const bool vec = (nc % VEC == 0) && (it.ld1 % VEC == 0) && ((((uintptr_t)out) & 15) == 0);" in src
    assert "const bool vec = (nr % VEC == 0) && (it.ld2 % VEC == 0) && ((((uintptr_t)out) & 15) == 0);" in src


# ---- every named path is reached ---------------------------------------------------------------------------------------------------
def test_bucket_layout_reaches_every_path_of_the_linear_kernel():
    segs, n, p_bytes, m_bytes = R.bucket_layout()
    assert n % 4 != 0 and all(s["start"] % 4 == 0 for s in segs if s["kind"] != "pad")
    seg_start = [s["start"] for s in segs] + [segs[-1]["end"]]
    assert seg_start[-1] > n > segs[-1]["start"]                                            # the last tensor is cut by n
    addr, mirror = [s["addr"] for s in segs], [s["mirror"] or 0 for s in segs]
    rec = R.bucket_paths(seg_start, addr, n, mirror)
    name = lambda r: segs[r[3]]["name"]
    kinds = set((r[2], r[4]) for r in rec)
    # the three update paths, each with a mirror and with a NULL entry of the mirror table
    for path in ("fast", "quad"):
        assert (path, True) in kinds and (path, False) in kinds, path
    assert any(r[2].startswith("scalar") and r[4] for r in rec) and any(r[2].startswith("scalar") and not r[4] for r in rec)
    fast = sorted((r[0], name(r)) for r in rec if r[2] == "fast")
    assert fast == [(0, "fast2"), (1, "fast2"), (5, "mid"), (7, "last")], fast
    # a misaligned parameter inside one tensor: the whole block is scalar
    blk2 = [r for r in rec if r[0] == 2]
    assert len(blk2) == R.BLOCK // 4 and all(r[2] == "scalar:misaligned" and name(r) == "misaligned" for r in blk2)
    # tails of 10, 1 and 5002 elements; the bucket's own end
    tails = sorted(name(r) for r in rec if r[2] == "scalar:tail")
    assert tails == ["mid", "one", "ten"], tails
    assert [name(r) for r in rec if r[2] == "scalar:n"] == ["last"] and rec[-1][2] == "scalar:n"
    # NULL pointers: a padding segment that holds a whole quad, and the tensor taken out (a whole block of it among them)
    nulls = set(name(r) for r in rec if r[2] == "null")
    assert nulls == {"pad1", "taken_out"}, nulls
    assert sum(1 for r in rec if r[0] == 4 and r[2] == "null") > R.BLOCK // 8
    assert any(s["kind"] == "pad" for s in segs) and sum(s["end"] - s["start"] for s in segs if s["kind"] == "out") > R.BLOCK
    # quads, then a fast block, then a partial last quad, all in `mid`
    mid = [r for r in rec if name(r) == "mid"]
    assert [r[2] for r in mid if r[0] == 4] == ["quad"] * 225 and [r[2] for r in mid if r[0] == 6] == ["quad", "scalar:tail"]
    # the table FusedAdam builds is what the kernel's binary search finds, and it is not the identity
    tab = R.blk_seg_table(seg_start, n)
    for b in range(R.nblocks(n)):
        lo, hi = 0, len(addr) - 1
        while lo < hi:
            mid_ = (lo + hi + 1) >> 1
            if seg_start[mid_] <= b * R.BLOCK:
                lo = mid_
            else:
                hi = mid_ - 1
        assert tab[b] == lo
    assert tab.tolist() == [0, 0, 1, 2, 6, 7, 7, 9, 9]
    # no parameter overlaps another, and the arena leaves a gap behind each
    spans = sorted((s["addr"], s["addr"] + 4 * (s["end"] - s["start"])) for s in segs if s["addr"])
    assert all(a[1] + 200 <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= p_bytes
    assert sorted(s["addr"] % 16 for s in segs if s["addr"]) == [0, 0, 0, 0, 0, 4]


def test_tiled_items_reach_every_path_of_the_tiled_kernel():
    seen, shapes = set(), set()
    for it in R.tiled_items():
        c1 = None if it["c1"] is None else (it["c1"][0], it["c1"][1], it["c1"][2])
        c2 = None if it["c2"] is None else (it["c2"][0], it["c2"][1], it["c2"][2])
        rec = R.tiled_paths(it["R"], it["C"], it["k"], it["off_mis"], it["p_mis"], c1, c2)
        tiles_r, tiles_c = -(-it["R"] // 64), -(-it["C"] // 64)
        assert len(rec) == tiles_r * tiles_c
        assert it["R"] in (1, 63, 64, 65, 130) and it["C"] in (1, 7, 64, 65, 72, 136) and it["k"] in (1, 2, 3)
        for c, ext in ((it["c1"], it["C"]), (it["c2"], it["R"])):
            if c is not None:
                assert c[1] >= ext
                seen.add("ld:" + ("extent" if c[1] == ext else "vec" if c[1] % R.vec_of(c[0]) == 0 else "odd"))
        shapes.add("copies:" + ("both" if c1 and c2 else "m1" if c1 else "m2"))
        if c1 and c2:
            shapes.add("codes:" + ("mixed" if c1[0] != c2[0] else "same"))
        shapes.add("k%d" % it["k"])
        if it["R"] == 1:
            shapes.add("1d")
        for r in rec:
            seen.add("update:" + r["update"])
            for which, c in ((1, c1), (2, c2)):
                if c is not None:
                    seen.add("flush%d:%s:%s" % (which, "bf16" if c[0] == R.BF16 else "f32", r["flush%d" % which]))
            if tiles_r > 1:
                seen.add("row_tiles:%d" % tiles_r)
            if tiles_r > 1 and tiles_c > 1 and r["nr"] < 64 and r["nc"] < 64:
                seen.add("corner:" + r["update"])
            if 1 in r["divisors"]:
                seen.add("divisor1")
    want = {"update:vec4", "update:elem", "row_tiles:2", "row_tiles:3", "corner:vec4", "corner:elem", "divisor1",
            "ld:extent", "ld:vec", "ld:odd"}
    want |= {"flush%d:%s:%s" % (w, c, v) for w in (1, 2) for c in ("bf16", "f32") for v in ("vec", "elem")}
    assert want <= seen, sorted(want - seen)
    assert shapes >= {"copies:both", "copies:m1", "copies:m2", "codes:mixed", "codes:same", "k1", "k2", "k3", "1d"}, shapes
    # the conditions one at a time
    P = lambda *a, **k: R.tiled_paths(*a, **k)[0]
    assert P(64, 64, 1, 0, 0)["update"] == "vec4" and P(64, 64, 1, 2, 0)["update"] == "elem" and P(64, 64, 1, 0, 4)["update"] == "elem"
    assert P(64, 65, 1, 0, 0)["update"] == "elem" and R.tiled_paths(64, 66, 2, 0, 0)[1]["update"] == "vec4"
    assert P(64, 64, 1, 0, 0, (R.BF16, 64, 0))["flush1"] == "vec" and P(64, 64, 1, 0, 0, (R.BF16, 68, 0))["flush1"] == "elem"
    assert P(64, 64, 1, 0, 0, (R.F32, 68, 0))["flush1"] == "vec" and P(64, 64, 1, 0, 0, (R.F32, 68, 4))["flush1"] == "elem"
    assert P(60, 64, 1, 0, 0, None, (R.F32, 60, 0))["flush2"] == "vec" and P(60, 64, 1, 0, 0, None, (R.BF16, 64, 0))["flush2"] == "elem"


def test_skip_cases_reach_every_path_of_the_skip_kernel():
    n = R.SKIP_N
    assert R.nblocks(n) == 4 and n % R.BLOCK == 5
    paths = {k: R.skip_paths(n, v) for k, v in R.SKIP_CASES.items()}
    assert paths["four_in_one_block"] == ["extra", "clear", "clear", "clear"]
    assert len(R.SKIP_CASES["sixteen"]) == R.MAX_SKIP and "extra" in paths["sixteen"]
    assert paths["block_edge_and_n"] == ["boundary", "boundary", "clear", "boundary"]   # (the last block has 5 elements, 3 of them left out)
    assert paths["everything"] == ["inside"] * 4 and paths["whole_blocks"] == ["clear", "inside", "inside", "clear"]
    assert any(lo == hi for lo, hi in R.SKIP_CASES["empty"]) and paths["empty"] == ["boundary", "boundary", "clear", "clear"]
    for k, v in R.SKIP_CASES.items():
        assert all(0 <= lo <= hi <= n for lo, hi in v) and len(v) <= R.MAX_SKIP, k
        srt = sorted(v)
        assert all(a[1] <= b[0] for a, b in zip(srt, srt[1:])), k
    assert any(hi % R.BLOCK == 0 and lo % R.BLOCK != 0 for lo, hi in R.SKIP_CASES["block_edge_and_n"])
    assert any(hi == n for lo, hi in R.SKIP_CASES["block_edge_and_n"])


def test_sumsq_model_and_chain_bound_on_an_fp32_emulation():
    """Partials summed in fp32 by a chain no longer than the kernel's (16 in a row, then a tree) stay inside gamma(28) of the model."""
    rng = np.random.default_rng(3)
    n = R.SKIP_N
    g = rng.standard_normal(n).astype(np.float32)
    ranges = R.SKIP_CASES["block_edge_and_n"]
    part, total = R.sumsq_model(g, ranges, ext=[np.array([2.0, 3.0])], grad_scale=0.125)
    keep = np.ones(n, dtype=bool)
    for lo, hi in ranges:
        keep[lo:hi] = False
    assert float(part.sum()) == pytest.approx(float((g[keep].astype(np.float64) ** 2).sum()), rel=1e-13)
    assert total == pytest.approx((part.sum() + 5.0) / 64, rel=1e-15)
    pad = np.zeros(R.nblocks(n) * R.BLOCK, dtype=np.float32)
    pad[:n] = np.where(keep, g, 0)
    lanes = np.zeros((R.nblocks(n), R.THREADS), dtype=np.float32)
    for i in range(R.BLOCK // R.THREADS):
        x = pad.reshape(-1, R.BLOCK // R.THREADS, R.THREADS)[:, i]
        lanes = (lanes.astype(np.float64) + x.astype(np.float64) ** 2).astype(np.float32)      # one fmaf: one rounding
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    assert R.inside(lanes[:, 0], part, R.sumsq_bound(part, R.PARTIAL_CHAIN)) <= 1.0
