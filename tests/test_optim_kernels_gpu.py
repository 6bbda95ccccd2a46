"""The clip + Adam kernels of drn_amd/csrc/optim.hip called directly through their C entries, against the float64 model and the
derived error bound of tests/optim_ref.py, on every code path (tests/test_optim_ref_cpu.py shows that the layouts below reach them and
that a subtly wrong kernel leaves the bound).  Every buffer lives in an arena pre-filled with a NaN bit pattern: what a kernel is not
documented to write must come back bit-unchanged, and a read of what it must not read shows in the result.  `-s` prints, per kernel and
case, the worst observed error as a fraction of the bound."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

NAN32, NAN16 = 0x7FC0BEEF, 0x7FC1          # quiet NaNs with a payload: fp32 / bf16 canaries
GUARD = 64                                  # elements in front of and behind every flat buffer (256 bytes: alignment is kept)
WORST = {}                                  # (kernel, t) -> worst |err| / bound seen, for the report at the end


def _dev():
    return torch.device("cuda:0")


def _L():
    from drn_amd import _lib
    return _lib, _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def arena32(nelem):
    return np.full(nelem, NAN32, dtype=np.uint32)


def arena16(nelem):
    return np.full(nelem, NAN16, dtype=np.uint16)


def up(a):
    """A host arena (uint32 / uint16 / int) on the device, as the same-sized signed integer type."""
    t = torch.from_numpy(a.view({4: np.int32, 2: np.int16, 8: np.int64}[a.dtype.itemsize]).copy()).to(_dev())
    assert t.data_ptr() % 256 == 0
    return t


def down(t):
    return t.cpu().numpy().view({4: np.uint32, 2: np.uint16}[t.element_size()])


def bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def note(kernel, t, *ratios):
    WORST[(kernel, t)] = max(WORST.get((kernel, t), 0.0), *ratios)


def scalars(kw):
    """total_sumsq and the step counter on the device, each between two canaries."""
    tot = arena32(3)
    tot.view(np.float32)[1] = kw["total_sumsq"]
    cnt = np.array([-77, kw["t"], -78], dtype=np.int32)
    return up(tot), up(cnt)


def hyper_args(kw):
    return [ctypes.c_float(kw[k]) for k in ("lr", "beta1", "beta2", "eps", "max_norm", "grad_scale")]


def check_update(kernel, row, kw, got, arrays, mask):
    """got = (m, v, p) fp32 arrays of the kernel on the elements of `mask`; arrays = the inputs on the same elements."""
    want, bound = R.adam_model(*arrays, **kw), R.adam_bound(*arrays, **kw)
    ratios = [R.inside(g_, w_, b_) for g_, w_, b_ in zip(got, want, bound)]
    used = R.pow_allowance_used(got[2], want[2], bound[2], R.adam_bound(*arrays, pow_ulps=0, **kw)[2])
    print("%s, %s: |err| / bound  m %.3g  v %.3g  p %.3g; share of powf's %d ulps needed %.3g"
          % ((kernel, R.case_id(row)) + tuple(ratios) + (R.POW_ULPS, used)))
    note(kernel, kw["t"], *ratios)
    note(kernel + ", powf share", kw["t"], used)
    assert max(ratios) <= 1.0, (kernel, row, ratios)
    if row[3] == "zeros":
        assert np.array_equal(got[2], arrays[3]) and np.isfinite(got[2]).all() and not got[0].any() and not got[1].any()


# ---- drn_adam_bucket ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.CASES, ids=R.case_id)
def test_adam_bucket_every_path_against_the_model(row):
    lib_mod, L = _L()
    segs, n, p_bytes, m_bytes = R.bucket_layout()
    (g, m0, v0, p0), kw = R.case_arrays(row, n)
    nseg = len(segs)
    seg_start = [s["start"] for s in segs] + [segs[-1]["end"]]
    live = np.zeros(n, dtype=bool)                                   # elements the kernel updates
    for s in segs:
        if s["kind"] == "tensor":
            live[s["start"]:min(s["end"], n)] = True
    # flat buffers: NaN in the guards and in the m / v / g of padding and taken-out ranges
    flat = []
    for x in (g, m0, v0):
        a = arena32(n + 2 * GUARD)
        a.view(np.float32)[GUARD:GUARD + n][live] = x[live]
        flat.append(a)
    # parameters and mirrors in their arenas
    pa, ma = arena32(p_bytes // 4), arena16(m_bytes // 2)
    p_live, m_live = np.zeros(pa.size, dtype=bool), np.zeros(ma.size, dtype=bool)
    for s in segs:
        if s["kind"] == "tensor":
            cnt, o = min(s["end"], n) - s["start"], s["addr"] // 4
            pa.view(np.float32)[o:o + cnt] = p0[s["start"]:s["start"] + cnt]
            p_live[o:o + cnt] = True
            if s["mirror"] is not None:
                m_live[s["mirror"] // 2:s["mirror"] // 2 + cnt] = True
    G = up(flat[0])
    tot, cnt = scalars(kw)
    tab_seg = up(np.asarray(seg_start, dtype=np.int64))
    blk_seg = up(R.blk_seg_table(seg_start, n))
    results = []
    for use_tab in (True, False):
        Mo, Vo, Pa, Ma = up(flat[1]), up(flat[2]), up(pa), up(ma)
        p_addr = [Pa.data_ptr() + s["addr"] if s["kind"] == "tensor" else 0 for s in segs]
        m_addr = [Ma.data_ptr() + s["mirror"] if s["mirror"] is not None else 0 for s in segs]
        # the paths the predicates promise are the paths of the real addresses
        assert R.bucket_paths(seg_start, p_addr, n, m_addr) == \
            R.bucket_paths(seg_start, [s["addr"] for s in segs], n, [s["mirror"] or 0 for s in segs])
        tab_p, tab_m = up(np.asarray(p_addr, dtype=np.int64)), up(np.asarray(m_addr, dtype=np.int64))
        base = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
        lib_mod.check(L.drn_adam_bucket(base(G), base(Mo), base(Vo), ctypes.c_int64(n), P(tab_seg), P(tab_p), nseg,
                                        P(blk_seg) if use_tab else None, P(tab_m), ctypes.c_void_p(tot.data_ptr() + 4),
                                        ctypes.c_void_p(cnt.data_ptr() + 4), *(hyper_args(kw) + [_stream()])), "drn_adam_bucket")
        torch.cuda.synchronize()
        results.append([down(t) for t in (Mo, Vo, Pa, Ma)])
    for a, b in zip(*results):
        assert np.array_equal(a, b)                                  # block table and binary search: bit-identical
    Mn, Vn, Pn, Man = results[0]
    # nothing but the documented outputs changed
    assert np.array_equal(down(G), flat[0]) and np.array_equal(down(tot), down(scalars(kw)[0])) and cnt.tolist() == [-77, kw["t"], -78]
    keep = np.ones(n + 2 * GUARD, dtype=bool)
    keep[GUARD:GUARD + n] = ~live
    assert np.array_equal(Mn[keep], flat[1][keep]) and np.array_equal(Vn[keep], flat[2][keep])
    assert np.array_equal(Pn[~p_live], pa[~p_live]) and np.array_equal(Man[~m_live], ma[~m_live])
    # the update, gathered back into flat order
    p_new = np.zeros(n, dtype=np.float32)
    for s in segs:
        if s["kind"] == "tensor":
            c_, o = min(s["end"], n) - s["start"], s["addr"] // 4
            p_new[s["start"]:s["start"] + c_] = Pn.view(np.float32)[o:o + c_]
            if s["mirror"] is not None:
                assert np.array_equal(Man[s["mirror"] // 2:s["mirror"] // 2 + c_], bf16_bits(p_new[s["start"]:s["start"] + c_])), s["name"]
    got = (Mn.view(np.float32)[GUARD:GUARD + n][live], Vn.view(np.float32)[GUARD:GUARD + n][live], p_new[live])
    check_update("adam_bucket", row, kw, got, (g[live], m0[live], v0[live], p0[live]), live)
    if row[3] == "zeros":
        assert np.array_equal(Pn, pa)


# ---- drn_adam_tiled ----------------------------------------------------------------------------------------------------------------
def _tiled_plan():
    """Offsets of every item of optim_ref.tiled_items() inside shared arenas: flat (elements, other items and NaN gaps between), parameter
    arena (bytes), and one copy arena per dtype (bytes)."""
    items, flat, pb, cb = [], GUARD, 256, {R.F32: 64, R.BF16: 64}
    for it in R.tiled_items():
        d = dict(it)
        n = it["R"] * it["C"] * it["k"]
        d["n"] = n
        d["off"] = (flat + 3) // 4 * 4 + it["off_mis"]
        flat = d["off"] + n + 9
        d["p"] = pb + it["p_mis"]
        pb += (4 * n + it["p_mis"] + 255) // 256 * 256 + 256
        for key, rows in (("c1", it["R"]), ("c2", it["C"])):
            if it[key] is not None:
                code, ld, mis = it[key]
                size = rows * it["k"] * ld * (2 if code == R.BF16 else 4)
                d[key] = (code, ld, cb[code] + mis, rows)
                cb[code] += (size + mis + 63) // 64 * 64 + 64
        items.append(d)
    return items, flat + GUARD, pb, cb


@pytest.mark.parametrize("row", R.CASES, ids=R.case_id)
def test_adam_tiled_every_path_against_the_model(row):
    lib_mod, L = _L()
    items, nflat, p_bytes, c_bytes = _tiled_plan()
    total = sum(d["n"] for d in items)
    (g, m0, v0, p0), kw = R.case_arrays(row, total, seed=1)
    flat = [arena32(nflat) for _ in range(3)]
    pa = arena32(p_bytes // 4)
    ca = {R.F32: arena32(c_bytes[R.F32] // 4), R.BF16: arena16(c_bytes[R.BF16] // 2)}
    live, p_live, o = np.zeros(nflat, dtype=bool), np.zeros(pa.size, dtype=bool), 0
    for d in items:
        d["src"] = slice(o, o + d["n"])
        for a, x in zip(flat, (g, m0, v0)):
            a.view(np.float32)[d["off"]:d["off"] + d["n"]] = x[d["src"]]
        live[d["off"]:d["off"] + d["n"]] = True
        pa.view(np.float32)[d["p"] // 4:d["p"] // 4 + d["n"]] = p0[d["src"]]
        p_live[d["p"] // 4:d["p"] // 4 + d["n"]] = True
        o += d["n"]
    assert np.count_nonzero(~live) >= 2 * GUARD + 9 * len(items)             # NaN gaps between the items
    G, Mo, Vo, Pa = up(flat[0]), up(flat[1]), up(flat[2]), up(pa)
    Ca = {c: up(a) for c, a in ca.items()}
    tot, cnt = scalars(kw)
    arr = (lib_mod.AdamTiledItem * len(items))()
    blocks = []
    for i, d in enumerate(items):
        it = arr[i]
        it.p, it.off, it.R, it.C, it.k, it.tiles_c = Pa.data_ptr() + d["p"], d["off"], d["R"], d["C"], d["k"], (d["C"] + 63) // 64
        real = {}
        for key, f_m, f_ld, f_code in (("c1", "m1", "ld1", "code1"), ("c2", "m2", "ld2", "code2")):
            if d[key] is not None:
                code, ld, byte, rows = d[key]
                real[key] = (code, ld, Ca[code].data_ptr() + byte)
                setattr(it, f_m, real[key][2]); setattr(it, f_ld, ld); setattr(it, f_code, code)
        ntiles = ((d["R"] + 63) // 64) * it.tiles_c
        blocks += [(i, t) for t in range(ntiles)]
        src = R.tiled_items()[i]
        assert R.tiled_paths(d["R"], d["C"], d["k"], d["off"], it.p, real.get("c1"), real.get("c2")) == \
            R.tiled_paths(d["R"], d["C"], d["k"], src["off_mis"], src["p_mis"], src["c1"], src["c2"])
    order = np.random.default_rng(5).permutation(len(blocks))                 # several items in one launch, tiles in shuffled order
    blk_item = up(np.asarray([blocks[j][0] for j in order], dtype=np.int32))
    blk_tile = up(np.asarray([blocks[j][1] for j in order], dtype=np.int32))
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(_dev())
    lib_mod.check(L.drn_adam_tiled(P(G), P(Mo), P(Vo), P(raw), P(blk_item), P(blk_tile), len(blocks), ctypes.c_void_p(tot.data_ptr() + 4),
                                   ctypes.c_void_p(cnt.data_ptr() + 4), *(hyper_args(kw) + [_stream()])), "drn_adam_tiled")
    torch.cuda.synchronize()
    Mn, Vn, Pn = down(Mo), down(Vo), down(Pa)
    assert np.array_equal(down(G), flat[0]) and cnt.tolist() == [-77, kw["t"], -78]
    assert np.array_equal(Mn[~live], flat[1][~live]) and np.array_equal(Vn[~live], flat[2][~live]) and np.array_equal(Pn[~p_live], pa[~p_live])
    # every copy: permute + cast of the kernel's own result, everything else in the copy arenas (padding columns, gaps) untouched
    want = {c: a.copy() for c, a in ca.items()}
    got_p = np.zeros(total, dtype=np.float32)
    for d in items:
        pn = Pn.view(np.float32)[d["p"] // 4:d["p"] // 4 + d["n"]]
        got_p[d["src"]] = pn
        p3 = pn.reshape(d["R"], d["C"], d["k"])
        for key, perm, ext in (("c1", (0, 2, 1), d["C"]), ("c2", (1, 2, 0), d["R"])):
            if d[key] is not None:
                code, ld, byte, rows = d[key]
                val = np.ascontiguousarray(p3.transpose(perm))
                bits = bf16_bits(val).reshape(val.shape) if code == R.BF16 else val.view(np.uint32)
                es = 2 if code == R.BF16 else 4
                want[code][byte // es:byte // es + rows * d["k"] * ld].reshape(rows, d["k"], ld)[:, :, :ext] = bits
    for c in ca:
        assert np.array_equal(down(Ca[c]), want[c]), "copies of dtype code %d" % c
    got = (Mn.view(np.float32)[live], Vn.view(np.float32)[live], got_p)
    # (the flat order of `live` is the order of the items: offsets grow with the item index)
    check_update("adam_tiled", row, kw, got, (g, m0, v0, p0), live)
    if row[3] == "zeros":
        assert np.array_equal(Pn, pa)


# ---- the norm passes ---------------------------------------------------------------------------------------------------------------
def _partials_call(g_host, skip, use_cls, counter):
    """Runs the pass on g (fp32 host array, NaN where skipped) between guards; returns (partials incl. guards, nb)."""
    lib_mod, L = _L()
    n = g_host.size
    nb = R.nblocks(n)
    assert int(L.drn_opt_nblocks(ctypes.c_int64(n))) == nb
    ga = arena32(n + 2 * GUARD)
    ga.view(np.float32)[GUARD:GUARD + n] = g_host
    G, part = up(ga), up(arena32(nb + 2))
    gp, pp = ctypes.c_void_p(G.data_ptr() + 4 * GUARD), ctypes.c_void_p(part.data_ptr() + 4)
    cp = ctypes.c_void_p(counter.data_ptr() + 4) if counter is not None else None
    if skip is None:
        lib_mod.check(L.drn_sumsq_partials(gp, ctypes.c_int64(n), pp, cp, _stream()), "drn_sumsq_partials")
    else:
        lo = (ctypes.c_int64 * len(skip))(*[r[0] for r in skip])
        hi = (ctypes.c_int64 * len(skip))(*[r[1] for r in skip])
        cls = None
        if use_cls:
            host = (ctypes.c_ubyte * nb)()
            lib_mod.check(L.drn_sumsq_block_classes(ctypes.c_int64(n), lo, hi, len(skip), host), "drn_sumsq_block_classes")
            want = [{"clear": 0, "inside": 1}.get(x, 2) for x in R.skip_paths(n, skip)]
            assert list(host) == want
            cls = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(_dev())
        lib_mod.check(L.drn_sumsq_partials_skip(gp, ctypes.c_int64(n), pp, cp, lo, hi, len(skip), P(cls), _stream()), "drn_sumsq_partials_skip")
    torch.cuda.synchronize()
    assert np.array_equal(down(G), ga)
    return down(part), nb


def _finalize(partials_f32, ext, grad_scale, two):
    """drn_sumsq_finalize (two = False, no ext) or drn_sumsq_finalize2 on host fp32 arrays; returns the fp32 total."""
    lib_mod, L = _L()
    pa = arena32(partials_f32.size + 2)
    pa.view(np.float32)[1:-1] = partials_f32
    Pt, out = up(pa), up(arena32(3))
    pp, op = ctypes.c_void_p(Pt.data_ptr() + 4), ctypes.c_void_p(out.data_ptr() + 4)
    if not two:
        assert not ext
        lib_mod.check(L.drn_sumsq_finalize(pp, partials_f32.size, op, ctypes.c_float(grad_scale), _stream()), "drn_sumsq_finalize")
    else:
        devs = []
        for e in ext:
            a = arena32(e.size + 2)
            a.view(np.float32)[1:-1] = e
            devs.append(up(a))
        ptrs = (ctypes.c_void_p * max(1, len(ext)))(*[t.data_ptr() + 4 for t in devs])
        lens = (ctypes.c_int32 * max(1, len(ext)))(*[e.size for e in ext])
        lib_mod.check(L.drn_sumsq_finalize2(pp, partials_f32.size, ptrs if ext else None, lens if ext else None, len(ext), op,
                                            ctypes.c_float(grad_scale), _stream()), "drn_sumsq_finalize2")
    torch.cuda.synchronize()
    o = down(out)
    assert o[0] == NAN32 and o[2] == NAN32 and np.array_equal(down(Pt), pa)
    return o.view(np.float32)[1]


@pytest.mark.parametrize("n", [1, 3, 4095, 4096, 4097, 3 * 4096 + 5])
def test_sumsq_partials_and_total(n):
    g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    counter = up(np.array([-5, 41, -6], dtype=np.int32))
    part, nb = _partials_call(g, None, False, counter)
    assert counter.tolist() == [-5, 42, -6]
    part2, _ = _partials_call(g, None, False, counter)
    assert counter.tolist() == [-5, 43, -6] and np.array_equal(part, part2)
    part3, _ = _partials_call(g, None, False, None)                                      # NULL: no counter is touched
    assert counter.tolist() == [-5, 43, -6] and np.array_equal(part, part3)
    assert part[0] == NAN32 and part[-1] == NAN32                                        # exactly nb values written, all of them
    got = part.view(np.float32)[1:-1]
    want, total = R.sumsq_model(g, grad_scale=0.125)
    r = R.inside(got, want, R.sumsq_bound(want, R.PARTIAL_CHAIN))
    tot = _finalize(got, [], 0.125, False)
    rt = R.inside(tot, total, R.sumsq_bound(total, R.PARTIAL_CHAIN + R.finalize_chain(nb)))
    print("sumsq_partials n = %d: |err| / bound  partials %.3g  total %.3g" % (n, r, rt))
    note("sumsq_partials", 0, r)
    note("sumsq_finalize", 0, rt)
    assert r <= 1.0 and rt <= 1.0


@pytest.mark.parametrize("case", sorted(R.SKIP_CASES))
def test_sumsq_partials_skip(case):
    n, ranges = R.SKIP_N, R.SKIP_CASES[case]
    g = np.random.default_rng(len(case)).standard_normal(n).astype(np.float32)
    exact = g.copy()
    for lo, hi in ranges:
        g[lo:hi] = np.nan                                                                 # a read of a skipped element shows
    counter = up(np.array([-5, 7, -6], dtype=np.int32))
    part, nb = _partials_call(g, ranges, False, counter)
    part_cls, _ = _partials_call(g, ranges, True, None)
    assert counter.tolist() == [-5, 8, -6]
    assert np.array_equal(part, part_cls)                                                 # host block classes or the in-kernel walk
    assert part[0] == NAN32 and part[-1] == NAN32
    got = part.view(np.float32)[1:-1]
    want, _ = R.sumsq_model(exact, ranges)
    r = R.inside(got, want, R.sumsq_bound(want, R.PARTIAL_CHAIN))
    print("sumsq_partials_skip %s (%s): |err| / bound %.3g" % (case, ",".join(R.skip_paths(n, ranges)), r))
    note("sumsq_partials_skip", 0, r)
    assert r <= 1.0
    for b, path in enumerate(R.skip_paths(n, ranges)):
        if path == "inside":
            assert got[b] == 0.0


@pytest.mark.parametrize("npartials", [1, 1023, 1024, 1025, 3000])
@pytest.mark.parametrize("ext_lens", [(), (1,), (1500,), (1, 1500, 1, 1500, 1500, 1, 1, 1500)], ids=["ext0", "ext1x1", "ext1x1500", "ext8"])
def test_sumsq_finalize(npartials, ext_lens):
    rng = np.random.default_rng(npartials + len(ext_lens))
    part = (rng.standard_normal(npartials) ** 2 * 4096).astype(np.float32)
    ext = [(rng.standard_normal(ne) ** 2 * 300).astype(np.float32) for ne in ext_lens]
    exact = 0.125 ** 2 * (float(part.astype(np.float64).sum()) + sum(float(e.astype(np.float64).sum()) for e in ext))
    bound = R.sumsq_bound(exact, R.finalize_chain(npartials, ext_lens))
    got2 = _finalize(part, ext, 0.125, True)
    r = R.inside(got2, exact, bound)
    if not ext:
        got1 = _finalize(part, [], 0.125, False)
        r = max(r, R.inside(got1, exact, bound))
    print("sumsq_finalize npartials = %d, ext %s: |err| / bound %.3g" % (npartials, list(ext_lens), r))
    note("sumsq_finalize", 0, r)
    assert r <= 1.0


# ---- FusedAdam: the Python-side tables at multi-tile shapes ------------------------------------------------------------------------
def test_fused_adam_steps_against_the_model_with_tiled_multi_tile_parameters():
    """(130, 72, 3) with both packed copies and (65, 136) with a transposed stack go through drn_adam_tiled with more than one row tile,
    (7,) and (4100,) through drn_adam_bucket.  5 steps, the gradient scale moving by 100 x so that clipping switches on and off; after
    every step p and the m / v slices are inside adam_bound of adam_model fed with the kernel's own previous state and the total_sumsq
    the norm pass produced, and the copies are the permuted casts of p, bit for bit."""
    from drn_amd import functional as DF
    from drn_amd import ops
    from drn_amd.dist import GradReducer
    from drn_amd.optim import FusedAdam
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    shapes = [(130, 72, 3), (65, 136), (7,), (4100,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
    c1, c2 = DF.packed(params[0], (0, 2, 1), ops.BF16), DF.packed(params[0], (1, 2, 0), ops.BF16)
    st_t = DF.stacked_t([params[1]])
    ptrs = (c1.data_ptr(), c2.data_ptr(), st_t.data_ptr())
    hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=20.0, grad_scale=1.0)
    red = GradReducer(params, world_size=1)
    opt = FusedAdam(red, lr=hyper["lr"], max_norm=hyper["max_norm"])
    where = {}
    for bi, b in enumerate(red.buckets):
        for p, off in zip(b.params, b.offsets):
            where[p.data_ptr()] = (bi, off)
    state = {p.data_ptr(): (np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32), p.detach().cpu().numpy().ravel().copy())
             for p in params}
    clipped = []
    for t, scale in enumerate([1.0, 0.01, 1.0, 0.01, 0.5], start=1):
        red.zero()
        for p in params:
            p.grad = (torch.randn(p.shape, generator=gen) * scale).to(dev)
        red.finish()
        opt.step()
        torch.cuda.synchronize()
        assert int(opt.step_counter) == t
        total = float(opt.total_sumsq)
        # the norm the kernels produced, against the model of the flat buffers
        exact = sum(R.sumsq_model(b.flat.cpu().numpy())[1] for b in red.buckets)
        nparts = opt.partials.numel()
        rt = R.inside(total, exact, R.sumsq_bound(exact, R.PARTIAL_CHAIN + R.finalize_chain(nparts)))
        assert rt <= 1.0, (t, total, exact)
        clipped.append(np.sqrt(total) > hyper["max_norm"])
        ratios = [rt]
        for p in params:
            bi, off = where[p.data_ptr()]
            n = p.numel()
            g = red.buckets[bi].flat[off:off + n].cpu().numpy()
            got = (opt.state[bi]["m"][off:off + n].cpu().numpy(), opt.state[bi]["v"][off:off + n].cpu().numpy(),
                   p.detach().cpu().numpy().ravel().copy())
            m0, v0, p0 = state[p.data_ptr()]
            kw = dict(hyper, total_sumsq=total, t=t)
            want, bound = R.adam_model(g, m0, v0, p0, **kw), R.adam_bound(g, m0, v0, p0, **kw)
            rs = [R.inside(a, w, b_) for a, w, b_ in zip(got, want, bound)]
            assert max(rs) <= 1.0, (t, tuple(p.shape), rs)
            ratios += rs
            note("fused_adam, powf share", t, R.pow_allowance_used(got[2], want[2], bound[2], R.adam_bound(g, m0, v0, p0, pow_ulps=0, **kw)[2]))
            state[p.data_ptr()] = got
        note("fused_adam", t, *ratios)
        print("FusedAdam step %d (clip %s): worst |err| / bound %.3g" % (t, "active" if clipped[-1] else "idle", max(ratios)))
        # the re-laid copies: refreshed in place by the tiled kernel, bit for bit the permuted cast of the parameter
        w = params[0].detach()
        for perm, ptr in (((0, 2, 1), ptrs[0]), ((1, 2, 0), ptrs[1])):
            again = DF.packed(params[0], perm, ops.BF16)
            assert again.data_ptr() == ptr and torch.equal(again, w.permute(*perm).contiguous().to(torch.bfloat16))
        again = DF.stacked_t([params[1]])
        assert again.data_ptr() == ptrs[2] and torch.equal(again, params[1].detach().t().contiguous())
    assert any(clipped) and not all(clipped), clipped
    tiled = [st["tiled"] for st in opt.state if st.get("tiled") is not None]
    assert sum(tl[3] for tl in tiled) == 3 * 2 + 2 * 3                           # both in 64 x 64 tiles, three and two row tiles
    red.remove()


def test_report_worst_ratio_per_kernel_and_step():
    """Not a check of its own: prints what the tests above recorded (run the file with -s)."""
    for (kernel, t), r in sorted(WORST.items()):
        print("worst |err| / bound: %-20s %s %.3g" % (kernel, "t = %d" % t if t else "", r))
    assert all(r <= 1.0 for k, r in WORST.items() if "powf share" not in k[0])
