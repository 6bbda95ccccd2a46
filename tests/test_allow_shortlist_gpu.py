"""Filtered shortlists on the device: Shortlister.shortlist(allow=) on all four tables against shortlist_reference(..., allow=) and
segment_shortlist_reference(..., allow=) (exact data: torch.equal on every field), the independence of a score's bits from the mask,
the quantised tables against their dequantised oracle, pack_allow against pack_allow_reference inside a guard band, in-place buffers
and graph replay with the mask's contents changed between replays, and the two stages end to end.
tests/test_allow_shortlist_cpu.py holds the definitions, the refusals and the compiler's resource notes."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import exact_case, offsets_of
from test_shortlist_gpu import BLOCK, exact_data, world

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
# (table, E): the plain kernels at a width below one K-step, at one that is no multiple of it and at 512; the FP8 format needs E % 32 == 0:
# one scale block, and three (an odd number, the block index moving against both step widths)
TABLES = [("plain", 8), ("plain", 40), ("plain", 512), ("mxfp8", 32), ("mxfp8", 96)]
EMPTY, SHORT, LONE = 2, 5, 3                                # rows of a per-sentence mask: all zero; three bits; the one that lights block 1


def same_lists(got, want, what=""):
    assert type(got) is type(want), what
    for f in got._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


def rows_of(want, S_):
    return type(want)(*(t[:S_] for t in want))


@functools.lru_cache(maxsize=None)
def bool_masks(V, empty_video=None):
    """-> (shared (V,), per sentence (17, V)) bool tensors on the host; shared is row 0.  Random halves with video 0 dropped and its
    twin 1 kept in every row but these two: row EMPTY all zero, row SHORT three bits anywhere (fewer when V < 3); `empty_video`
    allowed in every other row.
    At V = 775 block 1 (videos 256..511) is dark for every sentence but LONE and block 2 (512..767) for all."""
    g = torch.Generator().manual_seed(77 + V)
    per = torch.rand(17, V, generator=g) < 0.5
    per[:, 0] = False
    if V > 1:
        per[:, 1] = True
    if empty_video is not None:
        per[:, empty_video] = True
    if V == 3 * BLOCK + 7:
        per[:, BLOCK:3 * BLOCK] = False
        per[LONE, BLOCK + 44], per[LONE, 2 * BLOCK - 1] = True, True
    per[EMPTY] = False
    per[SHORT] = False
    pool = torch.arange(V) if V != 3 * BLOCK + 7 else torch.cat([torch.arange(BLOCK), torch.arange(3 * BLOCK, V)])
    per[SHORT, pool[torch.randperm(len(pool), generator=g)[:3]]] = True
    return per[0].clone(), per


def packed(mask):
    """pack_allow_reference of a host bool mask, on the device, with EVERY bit past V set in the last word: the kernels must ignore them."""
    from drn_amd import pack_allow_reference
    V = int(mask.shape[-1])
    words = pack_allow_reference(mask).copy().view(np.uint32)
    assert V % 32, "the test's tables end inside a word"
    junk = np.uint32((0xffffffff << (V % 32)) & 0xffffffff)
    words[..., -1] |= junk
    assert bool(((words[..., -1] & junk) == junk).all()) and words.shape[-1] == -(-V // 32)
    return torch.from_numpy(words.view(np.int32)).to(DEV).contiguous()


def build(emb, table, **kw):
    """A Shortlister over emb, plain or quantised; a quantised one of the tests' exact data holds exactly emb."""
    from drn_amd import Shortlister
    sl = Shortlister(emb, quantize=None if table == "plain" else table, **kw)
    if table != "plain":
        assert torch.equal(sl.dequantized().embeddings, emb), "the exact data is not exact in FP8"
    return sl


# -- 1. the definition, one row per video -------------------------------------------------------------------------------------------------

def test_the_masks_hold_what_the_tests_are_about():
    for V in (1, 33, 65, BLOCK + 1, 3 * BLOCK + 7):
        shared, per = bool_masks(V)
        others = [s for s in range(17) if s not in (EMPTY, SHORT)]
        assert not bool(per[others, 0].any()) and not bool(shared[0]) and not bool(per[EMPTY].any())
        assert int(per[SHORT].sum()) == min(3, V) < 5
        if V > 1:
            assert bool(shared[1]) and bool(per[others, 1].all())
        for m in (shared, per):
            w = packed(m).cpu().numpy().view(np.uint32)
            assert bool((w[..., -1] >> (V % 32) == (0xffffffff >> (V % 32))).all())
    shared, per = bool_masks(3 * BLOCK + 7)
    lit = per[:, BLOCK:2 * BLOCK].any(dim=1)
    assert lit.tolist() == [s == LONE for s in range(17)] and not bool(per[:, 2 * BLOCK:3 * BLOCK].any())
    assert not bool(shared[BLOCK:3 * BLOCK].any()) and bool(shared[:BLOCK].any()) and bool(per[:, 3 * BLOCK:].any(dim=1)[0])


@DTYPES
@pytest.mark.parametrize("table,E", TABLES, ids=["%s-%d" % t for t in TABLES])
def test_masked_shortlist_equals_the_reference_exactly(table, E, dtype):
    """V = 1, 33, 65, 257, 775 x S = 1, 16, 17 x n = 1, 5, 128 x a shared and a per-sentence mask: ids, scores and n equal to the float64
    definition, bit for bit.  The twins 0 and 1 tie, 0 is dropped: the tie is split.  At V = 775 block 2 is dark in both tiles and block
    1 in the second tile (the dark-block exit), and in the first tile one sentence alone lights block 1."""
    from drn_amd import Shortlist, shortlist_reference
    for V in (1, 33, 65, BLOCK + 1, 3 * BLOCK + 7):
        emb, q17 = exact_data(V, E, 17, dtype)
        if V > 1:
            assert torch.equal(emb[0], emb[1])
        sl = build(emb, table)
        for kind, mask in zip(("shared", "per sentence"), bool_masks(V)):
            words = packed(mask)
            for n in (1, 5, 128):
                want = shortlist_reference(emb, q17, n, allow=mask.to(DEV))
                rows, cols = torch.nonzero(want.ids >= 0, as_tuple=True)
                assert bool(mask.to(DEV).expand(17, V)[rows, want.ids[rows, cols].long()].all()), "the definition lists a dropped video"
                if mask.dim() == 2 and n > 1:
                    assert int(want.n[EMPTY]) == 0 and int(want.n[SHORT]) == min(3, V) < n, "no list shorter than n"
                for S_ in (1, 16, 17):
                    ws = words if mask.dim() == 1 else words[:S_].contiguous()
                    got = sl.shortlist(q17[:S_].contiguous(), n, allow=ws)
                    assert isinstance(got, Shortlist)
                    same_lists(got, rows_of(want, S_), (V, kind, S_, n))


# -- 2. the definition, ragged tables -------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("table,E", TABLES, ids=["%s-%d" % t for t in TABLES])
def test_masked_segment_shortlist_equals_the_reference_exactly(table, E, dtype):
    """Run lengths cycling 1 / 3 / 0 / 17 (blocks that start inside a mask word), a video of 300 rows, 257 one-row videos: ids, scores,
    n and rows equal to the float64 definition with the mask over VIDEOS.  An empty video whose bit is set is still not listed."""
    from drn_amd import SegmentShortlist, segment_shortlist_reference
    for layout, empty in (("cycle", 2), ("long", 3), ("ones257", None)):
        emb, q17, off = exact_case(layout, E, dtype)
        V = len(off) - 1
        if empty is not None:
            assert off[empty + 1] == off[empty]
        sl = build(emb, table, offsets=off)
        for kind, mask in zip(("shared", "per sentence"), bool_masks(V, empty)):
            words = packed(mask)
            if empty is not None:
                assert bool(mask[..., empty].reshape(-1)[0])
            for n in (1, 5, 128):
                want = segment_shortlist_reference(emb, off, q17, n, allow=mask.to(DEV))
                assert empty is None or not bool((want.ids == empty).any())
                for S_ in (1, 16, 17):
                    ws = words if mask.dim() == 1 else words[:S_].contiguous()
                    got = sl.shortlist(q17[:S_].contiguous(), n, allow=ws)
                    assert isinstance(got, SegmentShortlist)
                    same_lists(got, rows_of(want, S_), (layout, kind, S_, n))


# -- 3. a score's bits do not depend on the mask ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_table(R, E, dtype, seed=0):
    """A random table whose blocks of 32 columns differ in size (so that their scale bytes do), and 17 queries; changed by no test."""
    g = torch.Generator().manual_seed(seed + 1000 * R + E)
    emb = torch.randn(R, E, generator=g) * torch.exp2(torch.randint(-3, 4, (R, E // 32), generator=g).float()).repeat_interleave(32, dim=1)
    q = torch.randn(17, E, generator=g)
    return emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous()


@DTYPES
def test_a_masked_list_is_the_unmasked_list_of_the_kept_rows_bit_for_bit(dtype):
    """Random data, where a changed summation order would show: V = 775, at most 128 bits a sentence, so the masked n = 128 list holds
    every allowed video -- and equals the UNMASKED n = 128 list over emb[keep], ids mapped back, in ids and in the scores' bits."""
    from drn_amd import Shortlister
    V = 3 * BLOCK + 7
    emb, q17 = random_table(V, 224, dtype, seed=1)
    g = torch.Generator().manual_seed(3)
    per = torch.zeros(17, V, dtype=torch.bool)
    for s in range(17):
        per[s, torch.randperm(V, generator=g)[:(128, 100, 1, 37)[s % 4]]] = True
    sl = Shortlister(emb)

    def sub_table(s, keep):
        keep = torch.nonzero(keep)[:, 0].to(DEV)
        sub = Shortlister(emb[keep].contiguous()).shortlist(q17[s:s + 1].contiguous(), 128)
        ids = torch.where(sub.ids >= 0, keep[sub.ids.clamp(min=0).long()].to(torch.int32), sub.ids)
        return ids[0], sub.scores[0], sub.n[0]
    got = sl.shortlist(q17, 128, allow=packed(per))
    assert got.n.tolist() == per.sum(dim=1).tolist()
    for s in (0, 1, 2, 3, 16):
        for a, b in zip((got.ids[s], got.scores[s], got.n[s]), sub_table(s, per[s])):
            assert torch.equal(a, b), s
    shared = sl.shortlist(q17, 128, allow=packed(per[1]))
    for s in (0, 16):
        for a, b in zip((shared.ids[s], shared.scores[s], shared.n[s]), sub_table(s, per[1])):
            assert torch.equal(a, b), s


@DTYPES
@pytest.mark.parametrize("table", ["plain", "mxfp8"])
def test_the_all_ones_mask_is_the_unmasked_shortlist(table, dtype):
    from drn_amd import Shortlister
    off = offsets_of([1, 3, 0, 17] * 30 + [300, 2])
    emb, q17 = random_table(int(off[-1]), 96, dtype, seed=2)
    quantize = None if table == "plain" else table
    for sl in (Shortlister(emb, quantize=quantize), Shortlister(emb, offsets=off, quantize=quantize)):
        V = len(sl)
        ones = torch.ones(17, V, dtype=torch.bool)
        for n in (5, 128):
            want = sl.shortlist(q17, n)
            same_lists(sl.shortlist(q17, n, allow=packed(ones[0])), want, (V, n, "shared"))
            same_lists(sl.shortlist(q17, n, allow=packed(ones)), want, (V, n, "per sentence"))


# -- 4. the quantised tables against their oracle ------------------------------------------------------------------------------------------

@DTYPES
def test_masked_quantised_shortlists_are_those_of_the_dequantised_rows(dtype):
    from drn_amd import Shortlister
    off = offsets_of([1, 3, 0, 17] * 30 + [300, 2])
    emb, q17 = random_table(int(off[-1]), 96, dtype, seed=4)
    for kw in ({}, {"offsets": off}):
        sl = Shortlister(emb, quantize="mxfp8", **kw)
        oracle = sl.dequantized()
        for mask in bool_masks(len(sl)):
            words = packed(mask)
            for n in (5, 128):
                got = sl.shortlist(q17, n, allow=words)
                same_lists(got, oracle.shortlist(q17, n, allow=words), (len(sl), mask.dim(), n))
                assert int(got.n.max()) > 0


# -- 5. pack_allow -----------------------------------------------------------------------------------------------------------------------------

def test_pack_allow_equals_its_definition_and_writes_nothing_outside_its_words():
    from drn_amd import pack_allow, pack_allow_reference
    GUARD = 64
    g = torch.Generator().manual_seed(8)
    for V in (1, 31, 32, 33, 3 * BLOCK + 7):
        W = -(-V // 32)
        for S_ in (1, 17):
            host = torch.rand(S_, V, generator=g) < 0.5
            host[0, V - 1] = True
            for mask in ((host[0], host) if S_ == 1 else (host,)):
                want = torch.from_numpy(pack_allow_reference(mask)).to(DEV)
                dev = mask.to(DEV).contiguous()
                got = pack_allow(dev)
                assert got.dtype == torch.int32 and got.shape == want.shape == mask.shape[:-1] + (W,) and torch.equal(got, want), (V, S_)
                # out=: a stale buffer with every bit set, inside a guard band
                flat = torch.full((want.numel() + 2 * GUARD,), -1, dtype=torch.int32, device=DEV)
                out = flat[GUARD:GUARD + want.numel()].view(want.shape)
                assert pack_allow(dev, out=out) is out and torch.equal(out, want), (V, S_, "out=")
                assert bool((flat[:GUARD] == -1).all()) and bool((flat[GUARD + want.numel():] == -1).all())
                if V % 32:
                    assert bool((out.reshape(-1, W)[:, -1].contiguous().cpu().numpy().view(np.uint32) >> (V % 32) == 0).all()), "stale bits past V"


# -- 6. in-place buffers, graph replay, NaN rows -------------------------------------------------------------------------------------------

FOUR = pytest.mark.parametrize("table,ragged", [("plain", False), ("plain", True), ("mxfp8", False), ("mxfp8", True)],
                               ids=["plain", "segments", "q8", "q8-segments"])


@FOUR
def test_out_buffers_in_place_and_a_replay_follows_the_mask_written_in_place(table, ragged):
    from drn_amd import Shortlister, pack_allow
    from drn_amd.graph import capture_graph
    off = offsets_of([1, 3, 0, 17] * 30)
    emb, q17 = random_table(int(off[-1]), 96, torch.bfloat16, seed=3)
    q = q17[:5].contiguous()
    sl = Shortlister(emb, quantize=None if table == "plain" else table, **({"offsets": off} if ragged else {}))
    oracle = sl.dequantized()
    V = len(sl)
    shared, per = bool_masks(V)
    masks = [per[:5].contiguous(), torch.flip(per[:5], dims=(0, 1)).contiguous(), torch.zeros(5, V, dtype=torch.bool)]
    n, GUARD = 100, 64
    shapes = ((5, n), (5, n), (5,), (5, n))[:4 if ragged else 3]
    dtypes = (torch.int32, torch.float32, torch.int32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = tuple(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes))

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)
    words = packed(masks[0])
    got = sl.shortlist(q, n, out=out, allow=words)
    assert all(a is b for a, b in zip(got, out)) and guards_hold()
    reference = lambda m: oracle.shortlist(q, n, allow=packed(m))
    same_lists(got, reference(masks[0]), "every element")
    # capture mask packing + shortlist on one stream; replay after the BOOL mask, and so the packed words, changed in place
    mbuf = masks[0].to(DEV).contiguous()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        pack_allow(mbuf, out=words)
        sl.shortlist(q, n, out=out, allow=words)                               # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        pack_allow(mbuf, out=words)
        sl.shortlist(q, n, out=out, allow=words)
    for m in (masks[1], masks[2], masks[0]):
        mbuf.copy_(m)
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_lists(type(got)(*out), reference(m), "replay == eager on the new mask")
    assert int(out[2].max()) > 0 and guards_hold()
    # and with the words themselves overwritten, no packing in the graph
    graph2 = torch.cuda.CUDAGraph()
    with capture_graph(graph2, stream):
        sl.shortlist(q, n, out=out, allow=words)
    words.copy_(packed(masks[1]))
    graph2.replay()
    torch.cuda.synchronize()
    same_lists(type(got)(*out), reference(masks[1]), "replay == eager on the overwritten words")
    assert guards_hold()


@FOUR
def test_a_nan_query_row_lists_nothing_under_a_mask(table, ragged):
    from drn_amd import Shortlister
    off = offsets_of([1, 3, 0, 17] * 30)
    emb, q = random_table(int(off[-1]), 96, torch.bfloat16, seed=3)
    sl = Shortlister(emb, quantize=None if table == "plain" else table, **({"offsets": off} if ragged else {}))
    bad = q.clone()
    bad[1, 7], bad[16, 0] = float("nan"), float("inf")                          # (inf * x sums to NaN or +-inf: nothing finite)
    keep = [s for s in range(17) if s not in (1, 16)]
    for mask in bool_masks(len(sl)):
        words = packed(mask)
        clean, got = sl.shortlist(q, 9, allow=words), sl.shortlist(bad, 9, allow=words)
        for s in (1, 16):
            assert int(got.n[s]) == 0 and bool((got.ids[s] == -1).all()) and bool((got.scores[s] == 0).all())
        for f in got._fields:
            assert torch.equal(getattr(got, f)[keep], getattr(clean, f)[keep]), f
        assert int(clean.n[1]) > 0


# -- 7. the two stages end to end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_a_masked_shortlist_feeds_the_search_and_names_no_dropped_video(ragged):
    """search(candidates=masked.ids) == the search given the same rows as host lists, eagerly and by graph replay; no Hit names a
    dropped video; between the queries and the ids the host reads nothing (torch raises on a synchronising call meanwhile) and the
    shortlist is one tagged entry."""
    from drn_amd import Grounder, Shortlister, ops
    m, store, index, kw = world("plain")
    lens = [3, 1, 0, 17, 2, 5, 1] if ragged else [1] * NV
    assert len(lens) == NV
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (int(off[-1]), 16), generator=g).float().to(DEV).contiguous()
    sl = Shortlister(emb, names=store.names, offsets=off if ragged else None)
    sl.check(store), sl.check(index)
    qe = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    dropped = ["vid3", 5]
    allow = sl.allow_of(drop=dropped)
    assert allow.is_cuda and allow.dtype == torch.int32 and tuple(allow.shape) == (1,) and int(allow[0]) == 0x7f & ~(1 << 3) & ~(1 << 5)
    tok, qlen = sentences(7)
    n = 4
    for grounder in (Grounder(m, top_k=6, **kw), Grounder(m, top_k=6, graph=True, **kw)):
        sl.shortlist(qe, n, allow=allow), grounder.search(tok, qlen, index, per_video=2, candidates=sl.shortlist(qe, n, allow=allow).ids)  # (warm)
        torch.cuda.synchronize()
        ops.kernel_timer = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                     # (torch says that the mode is a prototype)
            torch.cuda.set_sync_debug_mode("error")
        try:
            short = sl.shortlist(qe, n, allow=allow)
            tags = [t[0] for t in ops.kernel_timer]
        finally:
            torch.cuda.set_sync_debug_mode("default")
            ops.kernel_timer = None
        got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
        assert tags == ["shortlist_segments_topn_allow" if ragged else "shortlist_topn_allow"]
        lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
        assert all(len(l) == n and 3 not in l and 5 not in l and (not ragged or 2 not in l) for l in lists)
        same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "two stages")
        named = [h[0] for hits in got.tolist(names=store.names) for h in hits]
        assert len(named) > 0 and "vid3" not in named and "vid5" not in named
