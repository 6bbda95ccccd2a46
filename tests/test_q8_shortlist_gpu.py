"""The shortlist over a block-scaled FP8 table on the device: drn_shortlist_topn_q8 and drn_shortlist_segments_topn_q8
(Shortlister(quantize="mxfp8"), Shortlister.from_mx8) bit for bit against the plain kernels over the dequantised rows, against the float64
definitions on exact data, the quantising and its size, the lossy bound against the ORIGINAL table, and what the quantised path shares
with the plain one: independence of the other sentences and of the table's size, a NaN query, out= buffers inside a guard band, graph
replay, and its ids as Grounder.search's device candidates.
tests/test_q8_shortlist_cpu.py holds the refusals, the sizes, the C boundary and the compiler's notes."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import offsets_of
from test_shortlist_gpu import world

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])

# name -> the run lengths of the videos: runs cycling 1 / 3 / 0 / 17 (several blocks, empty videos), a video of 300 rows (two passes of
# its block), 257 one-row videos (one past a block's video cap)
LAYOUTS = {"cycle": [1, 3, 0, 17] * 30, "long": [2, 300, 1, 0, 4], "ones257": [1] * 257}


def same_lists(got, want, what=""):
    assert type(got) is type(want), what
    for f in got._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


@functools.lru_cache(maxsize=None)
def random_table(R, E, dtype, seed=0):
    """A random table whose blocks of 32 columns differ in size (so that their scale bytes do), and 17 queries; shared, changed by no
    test."""
    g = torch.Generator().manual_seed(seed + 1000 * R + E)
    emb = torch.randn(R, E, generator=g) * torch.exp2(torch.randint(-3, 4, (R, E // 32), generator=g).float()).repeat_interleave(32, dim=1)
    q = torch.randn(17, E, generator=g)
    return emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous()


# -- 1. bit for bit the plain kernels over the dequantised rows ------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantised_shortlist_is_the_plain_shortlist_of_the_dequantised_rows(dtype, E):
    """V = 1 / 63 / 65 / 257 (257: a second workgroup), E = 32 (one scale block) / 96 (the block index advances against both step
    widths, an odd number of blocks) / 512, S = 1 / 17, n = 1 / 5 / 128: every field torch.equal to dequantized().shortlist()."""
    from drn_amd import Shortlist, Shortlister
    from drn_amd.index import mx8_dequantize
    for V in (1, 63, 65, 257):
        emb, q17 = random_table(V, E, dtype)
        sl = Shortlister(emb, quantize="mxfp8")
        oracle = sl.dequantized()
        assert sl.embeddings is None and oracle.quantize is None and len(sl) == len(oracle) == V and sl.dtype == oracle.dtype == dtype
        assert torch.equal(oracle.embeddings, mx8_dequantize(sl.codes, sl.scales, dtype))
        for S_ in (1, 17):
            q = q17[:S_].contiguous()
            for n in (1, 5, 128):
                got = sl.shortlist(q, n)
                assert isinstance(got, Shortlist) and int(got.n.min()) == min(n, V)
                same_lists(got, oracle.shortlist(q, n), (V, S_, n))


@DTYPES
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantised_segment_shortlist_is_the_plain_one_of_the_dequantised_rows(dtype, E):
    from drn_amd import SegmentShortlist, Shortlister
    for layout, lens in LAYOUTS.items():
        off = offsets_of(lens)
        emb, q17 = random_table(int(off[-1]), E, dtype, seed=5)
        sl = Shortlister(emb, offsets=off, quantize="mxfp8")
        oracle = sl.dequantized()
        assert len(sl) == len(oracle) == len(lens) and torch.equal(sl.offsets, oracle.offsets)
        for S_ in (1, 17):
            q = q17[:S_].contiguous()
            for n in (1, 5, 128):
                got = sl.shortlist(q, n)
                assert isinstance(got, SegmentShortlist)
                same_lists(got, oracle.shortlist(q, n), (layout, S_, n))


# -- 2. the float64 definition on exact data -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_tables(lens, E, seed=0):
    """codes / scales written DIRECTLY: integer code values in -8 .. 8 (exact e4m3fn codes), per-block exponents in -2 .. 3 that differ
    between neighbouring blocks (block b of a row has exponent (5 b + start) % 6 - 2 with a random start per row), integer queries in
    -4 .. 4.  Planted ties: the last row of every video repeats its first (inside a video) and the first row of every third video that
    owns rows repeats the first row of video 0 or 1 (between videos and blocks).

    Why every partial sum is exact in fp32: a table value is k * 2^e with |k| <= 8 and -2 <= e <= 3, a multiple of 2^-2 of magnitude at
    most 64 (four significant bits: exact in bf16 too); a product with a query in -4 .. 4 is a multiple of 2^-2 of magnitude at most 256,
    and any sum of at most E = 512 of them is a multiple of 2^-2 of magnitude at most 2^17: 20 bits, inside fp32's 24, in ANY order.
    So the device's scores equal the float64 definition's, rounded to float32, exactly.  -> (codes, scales, q, offsets) on the device."""
    off = offsets_of(list(lens))
    R, V = int(off[-1]), len(off) - 1
    g = torch.Generator().manual_seed(seed + 1000 * R + E)
    codes = torch.randint(-8, 9, (R, E), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
    start = torch.randint(0, 6, (R, 1), generator=g)
    scales = ((5 * torch.arange(E // 32)[None, :] + start) % 6 - 2 + 127).to(torch.uint8)
    if E > 32:
        assert bool((scales[:, 1:] != scales[:, :-1]).all())
    q = torch.randint(-4, 5, (17, E), generator=g).float()
    owners = [v for v in range(V) if off[v + 1] > off[v]]
    for i, v in enumerate(owners):
        for t in (codes, scales):
            if off[v + 1] - off[v] > 1:
                t[off[v + 1] - 1] = t[off[v]]
            if i >= 2 and i % 3 == 2:
                t[off[v]] = t[off[owners[i % 2]]]
    return codes.to(DEV).contiguous(), scales.to(DEV).contiguous(), q.to(DEV), off


@DTYPES
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantised_shortlists_equal_the_float64_definitions_on_exact_data(dtype, E):
    from drn_amd import Shortlister, segment_shortlist_reference, shortlist_reference
    from drn_amd.index import mx8_dequantize
    for layout, lens in LAYOUTS.items():
        codes, scales, q32, off = exact_tables(tuple(lens), E)
        table = mx8_dequantize(codes, scales)                                  # (float32: every value exact)
        assert float(table.abs().max()) <= 64 and bool((table * 4 == (table * 4).round()).all())
        q17 = q32.to(dtype).contiguous()
        plain = Shortlister.from_mx8(codes, scales, dtype)
        seg = Shortlister.from_mx8(codes, scales, dtype, offsets=off)
        assert plain.codes is codes and plain.scales is scales and plain.dtype == dtype and plain.E == E and len(seg) == len(lens)
        for n in (1, 5, 128):
            want_p, want_s = shortlist_reference(table, q32, n), segment_shortlist_reference(table, off, q32, n)
            if n == 128:
                for w in (want_p, want_s):
                    assert bool(((w.scores[:, 1:] == w.scores[:, :-1]) & (w.ids[:, 1:] > w.ids[:, :-1]) & (w.ids[:, 1:] >= 0)).any()), "no tie"
            for S_ in (1, 17):
                q = q17[:S_].contiguous()
                same_lists(plain.shortlist(q, n), type(want_p)(*(t[:S_] for t in want_p)), (layout, "plain", S_, n))
                same_lists(seg.shortlist(q, n), type(want_s)(*(t[:S_] for t in want_s)), (layout, "segments", S_, n))


# -- 3. the quantising and its size ---------------------------------------------------------------------------------------------------------

@DTYPES
def test_quantize_writes_mx8_quantize_byte_for_byte_and_the_bytes_are_bytes_of(dtype):
    from drn_amd import Shortlister
    from drn_amd.index import mx8_quantize
    lens = LAYOUTS["cycle"]
    off = offsets_of(lens)
    R, E = int(off[-1]), 96
    emb, q17 = random_table(R, E, dtype, seed=2)
    emb = emb.clone()
    emb[3, 32:64] = 0                                                           # a zero block: exponent -110
    emb[5, 0] = 1e-30                                                           # a value far below its block's scale: a zero code
    codes, scales = mx8_quantize(emb)
    for kw in ({}, {"offsets": off}):
        sl = Shortlister(emb, quantize="mxfp8", **kw)
        assert sl.quantize == "mxfp8" and sl.embeddings is None and sl.dtype == dtype and sl.E == E
        assert sl.codes.dtype == sl.scales.dtype == torch.uint8 and sl.codes.shape == (R, E) and sl.scales.shape == (R, E // 32)
        assert torch.equal(sl.codes, codes) and torch.equal(sl.scales, scales)
        assert sl.nbytes == Shortlister.bytes_of(R, E, dtype, "mxfp8") == R * (E + E // 32) == sl.codes.numel() + sl.scales.numel()
        wide = sl.dequantized()
        assert wide.nbytes == Shortlister.bytes_of(R, E, dtype) == R * E * emb.element_size()
        again = Shortlister.from_mx8(sl.codes, sl.scales, dtype, **kw)
        assert again.nbytes == sl.nbytes and len(again) == len(sl)
        for n in (5, 128):
            same_lists(again.shortlist(q17, n), sl.shortlist(q17, n), n)
    plain = Shortlister(emb)
    assert plain.quantize is None and plain.codes is None and plain.scales is None and plain.embeddings is emb and plain.dtype == dtype
    assert plain.nbytes == Shortlister.bytes_of(R, E, dtype)


def test_from_mx8_refuses_tables_that_are_not_the_format():
    from drn_amd import Shortlister, _lib
    codes, scales, _, off = exact_tables(tuple(LAYOUTS["cycle"]), 96)
    for bad_code in (0x7f, 0xff):
        c = codes.clone()
        c[7, 40] = bad_code
        for kw in ({}, {"offsets": off}):
            with pytest.raises(_lib.DrnError, match="NaN code"):
                Shortlister.from_mx8(c, scales, torch.bfloat16, **kw)
    for bad_scale in (255, 16, 0):
        s = scales.clone()
        s[600, 2] = bad_scale
        with pytest.raises(_lib.DrnError, match="scale byte outside"):
            Shortlister.from_mx8(codes, s, torch.float32)
    big_c, big_s = codes.clone(), scales.clone()
    big_c[1, :32], big_s[1, 0] = 0x08, 254                                      # 2^-6 * 2^127: finite, the top of the scale range
    big_c[1, 0] = 0x7e                                                          # 448 * 2^127 is not
    with pytest.raises(_lib.DrnError, match="not finite"):
        Shortlister.from_mx8(big_c, big_s, torch.float32)
    big_c[1, 0] = 0x08
    assert len(Shortlister.from_mx8(big_c, big_s, torch.float32)) == codes.shape[0]


# -- 4. lossy against the ORIGINAL table -------------------------------------------------------------------------------------------------

def lossy_ratio(emb, q, sl, got, off=None):
    """-> the largest |quantised score - float64 score of the ORIGINAL table| / bound over what is listed (quantized_score_bound; a video's
    bound is the largest among its rows)."""
    from drn_amd.retrieve import quantized_score_bound
    ref, tol = q.double() @ emb.double().t(), quantized_score_bound(emb, sl.scales, q)
    if off is not None:
        lens = torch.as_tensor(np.diff(off), device=emb.device)
        video = torch.repeat_interleave(torch.arange(len(off) - 1, device=emb.device), lens)[None].expand(q.shape[0], -1)
        full = lambda fill: torch.full((q.shape[0], len(off) - 1), fill, dtype=torch.float64, device=emb.device)
        ref, tol = full(float("-inf")).scatter_reduce(1, video, ref, "amax"), full(0.0).scatter_reduce(1, video, tol, "amax")
    listed = got.ids >= 0
    assert int(listed.sum()) == int(got.n.sum()) > 0
    ids = got.ids.clamp(min=0).long()
    ratio = (got.scores.double() - torch.gather(ref, 1, ids)).abs() / torch.gather(tol, 1, ids)
    return float(ratio[listed].max())


def test_quantised_scores_are_within_the_formats_bound_of_the_original_table():
    """Random bf16 data, E = 512: every listed quantised score within sum_e |q_e| * max(|x_e| / 16, 2^e_block / 1024) + E * 2^-23 *
    sum |q . x| of the float64 score on the table BEFORE quantising; the largest fraction is printed as tolerance_ratio."""
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    off = offsets_of(lens)
    emb, q17 = random_table(int(off[-1]), 512, torch.bfloat16, seed=4)
    q = q17[:5].contiguous()
    plain, seg = Shortlister(emb, quantize="mxfp8"), Shortlister(emb, offsets=off, quantize="mxfp8")
    ratios = [lossy_ratio(emb, q, plain, plain.shortlist(q, n)) for n in (16, 128)]
    ratios += [lossy_ratio(emb, q, seg, seg.shortlist(q, n), off) for n in (16, 128)]
    print("tolerance_ratio: %.4f" % max(ratios))
    assert 0 < max(ratios) <= 1.0


# -- 5. what the quantised path shares with the plain one --------------------------------------------------------------------------------

@DTYPES
def test_a_sentence_alone_and_a_prefix_of_the_table_give_the_same_bits(dtype):
    from drn_amd import Shortlister
    V, E = 600, 96
    emb, q = random_table(V, E, dtype, seed=8)
    sl = Shortlister(emb, quantize="mxfp8")
    full = sl.shortlist(q, 128)
    assert int(full.n.min()) == 128
    for s in (0, 5, 16):
        alone = sl.shortlist(q[s:s + 1].contiguous(), 128)
        for f in full._fields:
            assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]), (s, f)
    # every row's score from tables of 100 rows (all of them listed at n = 128), where the row has another place in another grid: the
    # whole table and a prefix of 300 rows (another last workgroup) list the same bits
    per = torch.full((17, V), float("nan"), device=DEV)
    for lo in range(0, V, 100):
        got = Shortlister.from_mx8(sl.codes[lo:lo + 100].contiguous(), sl.scales[lo:lo + 100].contiguous(), dtype).shortlist(q, 128)
        assert int(got.n.min()) == 100
        per.scatter_(1, got.ids[:, :100].long() + lo, got.scores[:, :100])
    assert not bool(torch.isnan(per).any())
    prefix = Shortlister.from_mx8(sl.codes[:300].contiguous(), sl.scales[:300].contiguous(), dtype).shortlist(q, 128)
    for got in (full, prefix):
        assert torch.equal(torch.gather(per, 1, got.ids.long()), got.scores)
    assert not torch.equal(prefix.ids, full.ids)
    seg =Shortlister(emb, offsets=offsets_of([1, 3, 0, 17] * 28 + [12]), quantize="mxfp8")
    both = seg.shortlist(q, 128)
    for s in (0, 16):
        alone = seg.shortlist(q[s:s + 1].contiguous(), 128)
        for f in both._fields:
            assert torch.equal(getattr(alone, f)[0], getattr(both, f)[s]), (s, f)


def test_a_nan_query_row_lists_nothing_and_leaves_the_others_alone():
    from drn_amd import Shortlister
    off = offsets_of(LAYOUTS["cycle"])
    emb, q = random_table(int(off[-1]), 96, torch.bfloat16, seed=3)
    bad = q.clone()
    bad[2, 7], bad[16, 0] = float("nan"), float("inf")                          # (inf * x sums to NaN or +-inf: nothing finite)
    keep = [s for s in range(17) if s not in (2, 16)]
    for sl in (Shortlister(emb, quantize="mxfp8"), Shortlister(emb, offsets=off, quantize="mxfp8")):
        clean, got = sl.shortlist(q, 9), sl.shortlist(bad, 9)
        same_lists(got, sl.dequantized().shortlist(bad, 9))
        for s in (2, 16):
            assert int(got.n[s]) == 0 and bool((got.ids[s] == -1).all()) and bool((got.scores[s] == 0).all())
        for f in got._fields:
            assert torch.equal(getattr(got, f)[keep], getattr(clean, f)[keep]), f


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_out_buffers_are_written_in_place_and_a_captured_quantised_shortlist_replays(ragged):
    from drn_amd import Shortlister
    from drn_amd.graph import capture_graph
    off = offsets_of(LAYOUTS["cycle"])
    emb, q17 = random_table(int(off[-1]), 96, torch.bfloat16, seed=3)
    _, q17b = random_table(int(off[-1]), 96, torch.bfloat16, seed=6)
    q, q2 = q17[:5].contiguous(), q17b[:5].contiguous()
    kw = {"offsets": off} if ragged else {}
    sl = Shortlister(emb, quantize="mxfp8", **kw)
    oracle = sl.dequantized()
    n, GUARD = 100, 64                                                          # (n above a sentence's 64-lane stride, below the cap)
    shapes = ((5, n), (5, n), (5,), (5, n))[:4 if ragged else 3]
    dtypes = (torch.int32, torch.float32, torch.int32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = tuple(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes))

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)
    got = sl.shortlist(q, n, out=out)
    assert all(a is b for a, b in zip(got, out)) and guards_hold()
    same_lists(got, oracle.shortlist(q, n), "every element")
    small = Shortlister.from_mx8(sl.codes[:4].contiguous(), sl.scales[:4].contiguous(), torch.bfloat16, **({"offsets": [0, 1, 1, 4]} if ragged else {}))
    for t in out:
        t.fill_(77)
    same_lists(small.shortlist(q, n, out=out), small.dequantized().shortlist(q, n), "the tail past the list")
    assert guards_hold()
    # capture on one stream, then replay on other queries written into the captured buffer
    qbuf = q.clone()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist(qbuf, n, out=out)                                          # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sl.shortlist(qbuf, n, out=out)
    for queries in (q2, q):
        qbuf.copy_(queries)
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_lists(type(got)(*out), oracle.shortlist(queries, n), "replay == the dequantised table")
    assert guards_hold()


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_quantised_ids_are_device_candidates_of_the_search(ragged):
    """search(candidates=short.ids) with short from a quantised table == the Hits of the dequantised table's ids; between the queries and
    the Hits the host reads nothing (torch raises on a synchronising call meanwhile) and the shortlist is one tagged entry."""
    from drn_amd import Grounder, Shortlister, ops
    m, store, index, kw = world("plain")
    lens = [3, 1, 0, 17, 2, 5, 1] if ragged else [1] * NV
    assert len(lens) == NV
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(12)
    emb = (torch.randint(-4, 5, (int(off[-1]), 32), generator=g).float() * 0.25).to(DEV).contiguous()
    emb[off[4]] = emb[off[1]]                                                   # a tie between videos the shortlist breaks by position
    sl = Shortlister(emb, names=store.names, offsets=off if ragged else None, quantize="mxfp8")
    sl.check(store), sl.check(index)
    oracle = sl.dequantized()
    assert oracle.names == sl.names
    qe = torch.randint(-4, 5, (S, 32), generator=g).float().to(DEV)
    qe[1] = float("nan")                                                        # a sentence whose shortlist is empty: ids all -1
    grounder = Grounder(m, top_k=5, **kw)
    tok, qlen = sentences(7)
    n = 4
    sl.shortlist(qe, n), grounder.search(tok, qlen, index, per_video=2, candidates=sl.shortlist(qe, n).ids)      # (warm)
    torch.cuda.synchronize()
    ops.kernel_timer = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                         # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        short = sl.shortlist(qe, n)
        tags = [t[0] for t in ops.kernel_timer]
        got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    assert tags == ["shortlist_segments_topn_q8" if ragged else "shortlist_topn_q8"]
    want = oracle.shortlist(qe, n)
    same_lists(short, want)
    assert short.n.tolist() == [n, 0, n]
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=want.ids), "two stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0
