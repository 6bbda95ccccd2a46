"""Deep shortlists on the device: Shortlister.shortlist_deep (drn_shortlist_deep: the masked phase one, then shortlist_merge_deep_kernel
of csrc/retrieve_deep.hip) against the float64 definitions on exact data -- torch.equal on every field -- at the shapes where the merge
can go wrong: n above and below V, m = n that is no power of two, m = 256 < n, every CAP and every CAP folding, staircase tables that
set the fold count; on ragged and quantised tables, under masks, against shortlist() where both answer, into guarded buffers, by graph
replay, and as the first stage of rerank, Grounder.search and evaluate_cascade.
tests/test_deep_shortlist_cpu.py holds the definition, the refusals, the C boundary and the compiler's resource notes."""
import warnings

import numpy as np
import pytest
import torch

from test_allow_shortlist_gpu import EMPTY, bool_masks, build, packed, same_lists
from test_grounding_engine_gpu import DEV
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import offsets_of
from test_shortlist_gpu import BLOCK, exact_data, random_case_ratio, world

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
FOUR = pytest.mark.parametrize("table,ragged", [("plain", False), ("plain", True), ("mxfp8", False), ("mxfp8", True)],
                               ids=["plain", "segments", "q8", "q8-segments"])
DEPTHS = (1, 128, 129, 256, 257, 512, 513, 1000, 1024)


def rows_of(want, S_):
    return type(want)(*(t[:S_] for t in want))


def cut(deep, k):
    """The first k columns of a list, as the list of n = k."""
    return type(deep)(*(t[:, :k].contiguous() if t.dim() == 2 else t.clamp(max=k) for t in deep))


def ragged_lens():
    """Runs cycling 1 / 3 / 0 / 17 over five blocks' worth of videos, with one video of 300 rows in the middle: alone in its block
    of the plan, so that block's list is shorter than m."""
    lens = [1, 3, 0, 17] * (5 * BLOCK // 4)
    lens.insert(2 * BLOCK + 2, 300)
    return lens


def ragged_exact(E, dtype, seed=0):
    """Integer-valued rows and 17 queries in [-4, 4] over ragged_lens(); the first row of every third video repeats the first row of
    video 0 or 1: equal best scores across videos and blocks.  -> (emb, q, offsets)"""
    lens = ragged_lens()
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(seed + E)
    emb = torch.randint(-4, 5, (int(off[-1]), E), generator=g).float()
    for v in range(4, len(lens), 3):
        if lens[v]:
            emb[off[v]] = emb[off[v % 2]]
    q = torch.randint(-4, 5, (17, E), generator=g).float()
    return emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous(), off


# -- 1. the definition, one row per video -----------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [8, 40])
def test_deep_shortlist_equals_the_reference_exactly(dtype, E):
    """V: one video; a block's half + 1; one block + 1; three blocks + 7; six blocks + 7; eleven blocks + 7 (three rounds of four
    lists, the last of three with a 7-video tail).  n: both ends, around 128 / 256 / 512 (m = n no power of two, m = 256 < n, each CAP
    from below and above), 1000 and the cap.  S = 17 is a second sentence tile of one row.  Every field equal to the float64
    definition, bit for bit; where every video is listed the planted twins are among them; where V >= n the list is full."""
    from drn_amd import Shortlist, Shortlister, _lib, shortlist_reference
    assert BLOCK == _lib.SHORTLIST_BLOCK and _lib.SHORTLIST_DEEP_MAX == 1024 and 11 * BLOCK + 7 == 2823
    for V in (1, 129, 257, 775, 1543, 2823):
        emb, q17 = exact_data(V, E, 17, dtype)
        sl = Shortlister(emb)
        for n in DEPTHS:
            want17 = shortlist_reference(emb, q17, n)
            if 1 < V <= n:
                assert bool(((want17.scores[:, 1:] == want17.scores[:, :-1]) & (want17.ids[:, 1:] > want17.ids[:, :-1])
                             & (want17.ids[:, 1:] >= 0)).any()), "no tie in the data"
            for S_ in (1, 16, 17):
                got = sl.shortlist_deep(q17[:S_].contiguous(), n)
                assert isinstance(got, Shortlist) and tuple(got.ids.shape) == (S_, n)
                same_lists(got, rows_of(want17, S_), (V, S_, n))
                if V >= n:
                    assert bool((got.n == n).all()) and bool((got.ids >= 0).all())


@DTYPES
def test_staircase_tables_set_the_fold_count(dtype):
    """emb[v] = (s // 32, s % 32) with s = v // 3 and the query (32, 1): score s, exact in bf16, tied in threes.  ASCENDING in v every
    later list lies wholly above the threshold -- the most folds a table of its size can ask for; DESCENDING nothing after the first
    lists enters.  The second query, (-32, -1), walks each table the other way.  n = 1024 (CAP = 1024 full) and 513."""
    from drn_amd import Shortlister, shortlist_reference
    V = 2823
    s = torch.arange(V) // 3
    up = torch.stack([s // 32, s % 32], dim=1).float()
    q = torch.tensor([[32.0, 1.0], [-32.0, -1.0]]).to(DEV, dtype).contiguous()
    for name, emb in (("ascending", up), ("descending", torch.flip(up, dims=(0,)))):
        emb = emb.to(DEV, dtype).contiguous()
        sl = Shortlister(emb)
        for n in (1024, 513):
            want = shortlist_reference(emb, q, n)
            same_lists(sl.shortlist_deep(q, n), want, (name, n))
            assert bool((want.n == n).all())
            assert want.scores[0, :6].tolist() == [940.0] * 3 + [939.0] * 3 and want.scores[1, :6].tolist() == [0.0] * 3 + [-1.0] * 3
        first = int(shortlist_reference(emb, q, 1).ids[0, 0])
        assert first == (V - 3 if name == "ascending" else 0)                   # (the lowest position of the best three)


# -- 2. ragged and quantised tables ------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [8, 40])
def test_deep_segment_shortlist_equals_the_reference_exactly(dtype, E):
    from drn_amd import SegmentShortlist, Shortlister, segment_shortlist_reference
    emb, q17, off = ragged_exact(E, dtype)
    sl = Shortlister(emb, offsets=off)
    lone = 2 * BLOCK + 2
    assert len(sl) == 5 * BLOCK + 1 and int(off[lone + 1] - off[lone]) == 300
    b = int(sl.plan.vid_blk[lone])
    assert int(sl.plan.blk_vid[b]) == lone and int(sl.plan.blk_vid[b + 1]) == lone + 1, "the long video is not alone in its block"
    for n in (129, 256, 257, 1024):
        want17 = segment_shortlist_reference(emb, off, q17, n)
        assert bool((want17.ids == lone).any()) and int(want17.n.max()) == min(n, 3 * 5 * BLOCK // 4 + 1)
        assert bool(((want17.scores[:, 1:] == want17.scores[:, :-1]) & (want17.ids[:, 1:] > want17.ids[:, :-1]) & (want17.ids[:, 1:] >= 0)).any())
        for S_ in (1, 17):
            got = sl.shortlist_deep(q17[:S_].contiguous(), n)
            assert isinstance(got, SegmentShortlist)
            same_lists(got, rows_of(want17, S_), (S_, n))


@DTYPES
@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_deep_quantised_shortlists_are_those_of_the_dequantised_rows(dtype, ragged):
    from drn_amd import segment_shortlist_reference, shortlist_reference
    from drn_amd.index import mx8_dequantize
    if ragged:
        emb, q, off = ragged_exact(64, dtype)
        sl = build(emb, "mxfp8", offsets=off)
    else:
        emb, q = exact_data(1543, 64, 17, dtype)
        sl = build(emb, "mxfp8")
    table = mx8_dequantize(sl.codes, sl.scales, dtype)
    oracle = sl.dequantized()
    for n in (129, 300, 1024):
        got = sl.shortlist_deep(q, n)
        same_lists(got, oracle.shortlist_deep(q, n), n)
        same_lists(got, segment_shortlist_reference(table, off, q, n) if ragged else shortlist_reference(table, q, n), n)


# -- 3. masks ---------------------------------------------------------------------------------------------------------------------------

@FOUR
def test_deep_shortlists_under_masks_equal_the_masked_reference(table, ragged):
    """allow=None is the explicit all-ones mask; a shared mask; per-sentence masks with an all-zero row, which lists nothing; at
    V = 775 block 1 is dark for every sentence but one and block 2 for all.  Each against the reference's allow=."""
    from drn_amd import segment_shortlist_reference, shortlist_reference
    if ragged:
        emb, q, off = ragged_exact(64, torch.bfloat16)
        sl = build(emb, table, offsets=off)
        reference = lambda n, mask: segment_shortlist_reference(emb, off, q, n, allow=None if mask is None else mask.to(DEV))
    else:
        emb, q = exact_data(3 * BLOCK + 7, 64, 17, torch.bfloat16)
        sl = build(emb, table)
        reference = lambda n, mask: shortlist_reference(emb, q, n, allow=None if mask is None else mask.to(DEV))
    V = len(sl)
    shared, per = bool_masks(V)
    ones = torch.ones(V, dtype=torch.bool)
    for n in (129, 1024):
        plain = sl.shortlist_deep(q, n)
        same_lists(plain, reference(n, None), ("no mask", n))
        same_lists(sl.shortlist_deep(q, n, allow=packed(ones)), plain, ("all ones", n))
        same_lists(sl.shortlist_deep(q, n, allow=packed(ones[None, :].expand(17, V).contiguous())), plain, ("all ones a sentence", n))
        same_lists(sl.shortlist_deep(q, n, allow=packed(shared)), reference(n, shared), ("shared", n))
        got = sl.shortlist_deep(q, n, allow=packed(per))
        same_lists(got, reference(n, per), ("per sentence", n))
        assert int(got.n[EMPTY]) == 0 and bool((got.ids[EMPTY] == -1).all()) and bool((got.scores[EMPTY] == 0).all())
        assert int(got.n.max()) > 100
    if not ragged:
        assert int(per[:, BLOCK:2 * BLOCK].any(dim=1).sum()) == 1 and not bool(per[:, 2 * BLOCK:3 * BLOCK].any()), "no dark block"


# -- 4. ties to what exists -----------------------------------------------------------------------------------------------------------------

@FOUR
def test_a_deep_list_agrees_with_shortlist_with_its_own_prefixes_and_with_rerank(table, ragged):
    """Random data, where a changed chain would show in the bits: shortlist_deep(q, n) == shortlist(q, n) field for field at n = 1 / 64
    / 128; the first k columns of shortlist_deep(q, 1024) are shortlist_deep(q, k), and its first 128 shortlist(q, 128); reranking
    its ids to 128 gives shortlist(q, 128) again."""
    from drn_amd import Shortlister
    from test_allow_shortlist_gpu import random_table
    off = offsets_of(ragged_lens()) if ragged else None
    emb, q = random_table(int(off[-1]) if ragged else 1543, 96, torch.bfloat16, seed=5)
    sl = Shortlister(emb, quantize=None if table == "plain" else table, offsets=off)
    for n in (1, 64, 128):
        same_lists(sl.shortlist_deep(q, n), sl.shortlist(q, n), n)
    deep = sl.shortlist_deep(q, 1024)
    assert int(deep.n.min()) == (961 if ragged else 1024)
    for k in (129, 256, 512):
        same_lists(cut(deep, k), sl.shortlist_deep(q, k), k)
    short = sl.shortlist(q, 128)
    same_lists(cut(deep, 128), short, "the first 128 columns")
    again = sl.rerank(deep.ids, q, n=128)
    for f in ("ids", "scores", "n"):
        assert torch.equal(getattr(again, f), getattr(short, f)), f


def test_deep_shortlist_on_random_bf16_data_is_within_the_derived_bound():
    from drn_amd import Shortlister
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(2823, 512, generator=g).to(DEV, torch.bfloat16).contiguous()
    q = torch.randn(3, 512, generator=g).to(DEV, torch.bfloat16).contiguous()
    ratio = random_case_ratio(emb, q, Shortlister(emb).shortlist_deep(q, 1024))
    print("largest error / tol: %.4f" % ratio)
    assert ratio <= 1.0


# -- 5. NaN, buffers, graphs ----------------------------------------------------------------------------------------------------------------

def test_a_nan_query_row_lists_nothing_and_leaves_the_others_alone():
    from drn_amd import Shortlister, shortlist_reference
    emb, q = exact_data(3 * BLOCK + 7, 40, 17, torch.bfloat16)
    sl = Shortlister(emb)
    clean = sl.shortlist_deep(q, 600)
    bad = q.clone()
    bad[2, 7], bad[16, 0] = float("nan"), float("inf")                  # (inf * 0 is NaN somewhere, +-inf elsewhere: nothing finite)
    got = sl.shortlist_deep(bad, 600)
    same_lists(got, shortlist_reference(emb, bad, 600))
    assert int(got.n[2]) == 0 and bool((got.ids[2] == -1).all()) and bool((got.scores[2] == 0).all()) and int(got.n[16]) < 600
    keep = [s for s in range(17) if s not in (2, 16)]
    for f in got._fields:
        assert torch.equal(getattr(got, f)[keep], getattr(clean, f)[keep]), f


@FOUR
def test_out_buffers_in_place_and_a_replay_follows_queries_and_mask_written_in_place(table, ragged):
    """out= inside guard bands: every element written, nothing outside them -- also where the table is shorter than n.  One captured
    graph, replayed with the queries and the mask's words changed in place, equals eager and the dequantised table's list."""
    from drn_amd import Shortlister
    from drn_amd.graph import capture_graph
    from test_allow_shortlist_gpu import random_table
    off = offsets_of([1, 3, 0, 17] * 90)
    emb, q17 = random_table(int(off[-1]), 96, torch.bfloat16, seed=3)
    sl = Shortlister(emb, quantize=None if table == "plain" else table, **({"offsets": off} if ragged else {}))
    oracle = sl.dequantized()
    V = len(sl)
    shared, per = bool_masks(V)
    q, q2 = q17[:5].contiguous(), q17[5:10].contiguous()
    n, GUARD = 300, 64
    shapes = ((5, n), (5, n), (5,), (5, n))[:4 if ragged else 3]
    dtypes = (torch.int32, torch.float32, torch.int32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = tuple(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes))

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)
    got = sl.shortlist_deep(q, n, out=out)
    assert all(a is b for a, b in zip(got, out)) and guards_hold()
    same_lists(got, oracle.shortlist_deep(q, n), "every element")
    assert int(got.n.min()) == (n if not ragged else min(n, 270)) and (ragged or bool((got.ids >= 0).all()))
    words = packed(per[:5].contiguous())
    qbuf = q.clone()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist_deep(qbuf, n, out=out, allow=words)                        # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sl.shortlist_deep(qbuf, n, out=out, allow=words)
    for queries, mask in ((q2, torch.flip(per[:5], dims=(0, 1)).contiguous()), (q, torch.zeros(5, V, dtype=torch.bool)), (q2, per[:5].contiguous())):
        qbuf.copy_(queries)
        words.copy_(packed(mask))
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_lists(type(got)(*out), oracle.shortlist_deep(queries, n, allow=packed(mask)), "replay == eager on new queries and a new mask")
        assert guards_hold()
    assert int(out[2].max()) > 0


# -- 6. the stages end to end ---------------------------------------------------------------------------------------------------------------

def test_a_deep_list_feeds_the_search_like_the_same_set_from_shortlist():
    """The store has NV videos: a deep list names them all, padded with -1 to its width, and the search over its ids gives the Hits of
    the same set passed from shortlist(); one shortlist_deep tag per call."""
    from drn_amd import Grounder, Shortlister, ops
    m, store, index, kw = world("plain")
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (NV, 16), generator=g).float()
    emb[4] = emb[1]
    sl = Shortlister(emb.to(DEV).contiguous(), names=store.names)
    sl.check(index)
    qe = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    qe[1] = float("nan")                                                  # a sentence whose list is empty: ids all -1
    tok, qlen = sentences(7)
    ops.kernel_timer = []
    try:
        deep = sl.shortlist_deep(qe, 300)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags == ["shortlist_deep"]
    short = sl.shortlist(qe, 16)
    assert torch.equal(deep.ids[:, :16], short.ids) and bool((deep.ids[:, 16:] == -1).all()) and deep.n.tolist() == [NV, 0, NV]
    grounder = Grounder(m, top_k=5, **kw)
    got = grounder.search(tok, qlen, index, per_video=2, candidates=deep.ids)
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=short.ids), "deep ids == shortlist ids")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0


def test_evaluate_cascade_deep_ranks_are_the_full_ranks_under_the_coarse_mask_cut_at_128():
    """deep=True, depth = 300: ranks == fine.rank(..., allow=pack_allow(candidates_mask(coarse deep ids))) clipped to -1 at
    SHORTLIST_MAX = 128, the length the fine stage reranks to; a topk above it saturates."""
    from drn_amd import ShortlistRecall, Shortlister, _lib, candidates_mask, evaluate_cascade, metrics, pack_allow
    from test_allow_shortlist_gpu import random_table
    lens = [1, 3, 0, 17] * 150 + [40, 2]
    V, off = len(lens), offsets_of(lens)
    names = ["v%d" % v for v in range(V)]
    emb, q17 = random_table(int(sum(lens)), 96, torch.bfloat16, seed=70)
    g = torch.Generator().manual_seed(4)
    coarse = Shortlister(torch.randn(V, 32, generator=g).to(DEV, torch.bfloat16).contiguous(), names=names, quantize="mxfp8")
    fine = Shortlister(emb, names=names, offsets=off)
    depth, topks = 300, (1, 10, 128, 300)
    batches = []
    for S_ in (17, 6):
        cq = torch.randn(S_, 32, generator=g).to(DEV, torch.bfloat16).contiguous()
        targets = torch.randint(0, V, (S_,), generator=g).tolist()
        batches.append(([names[t] for t in targets], cq, q17[:S_].contiguous()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = evaluate_cascade(coarse, fine, iter(batches), depth, topks=topks, deep=True)
    assert isinstance(got, ShortlistRecall) and got.n == 23 and got.topks == list(topks)
    want = []
    for bnames, cq, fq in batches:
        listed = coarse.shortlist_deep(cq, depth)
        assert bool((listed.n == depth).all())
        words = pack_allow(candidates_mask(listed.ids, V))
        targets = torch.tensor([names.index(x) for x in bnames], dtype=torch.int32, device=DEV)
        r = fine.rank(fq, targets, allow=words).rank
        want.append(torch.where(r < _lib.SHORTLIST_MAX, r, torch.full_like(r, -1)))
    want = torch.cat(want).cpu().numpy()
    assert got.ranks.dtype == np.int32 and np.array_equal(got.ranks, want)
    assert (want >= 0).any() and (want < 0).any()
    assert got.recall == metrics.recall_from_ranks(want, list(topks)) and got.recall[3] == got.recall[2]
    # the default path is untouched: the same call without deep=True still refuses the depth
    with pytest.raises(_lib.DrnError, match=r"depth = 300 outside \[1, 128\]"):
        evaluate_cascade(coarse, fine, iter(batches), depth)
