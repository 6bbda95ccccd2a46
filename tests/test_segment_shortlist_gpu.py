"""The segmented shortlist on the device: drn_shortlist_segments_topn (Shortlister(offsets=)) against segment_shortlist_reference on exact
data (torch.equal on ids, scores, n and rows), against the plain shortlist's bits with one row per video and under three segmentations
of one table, its independence of the other sentences and of the cut, random bf16 data against a derived bound, a NaN query, out=
buffers inside a guard band, graph replay, and its ids as Grounder.search's device candidates.
tests/test_segment_shortlist_cpu.py holds the definition, the block plan, the refusals and the compiler's notes."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_search_gpu import NV, S, same_hits, sentences
from test_shortlist_gpu import world

pytestmark = pytest.mark.gpu
FIELDS = ("ids", "scores", "n", "rows")
LONG = [2, 300, 1, 0, 600, 4, 7]                           # a 300-row and a 600-row video among short ones: blocks of two and three passes

# name -> the run lengths of the videos (a block of the plan closes at 256 videos or 256 rows)
LAYOUTS = {
    "one": [1],                                            # R = V = 1
    "ones": [1] * 70,
    "cycle": [1, 3, 0, 17] * 30,                           # empty videos inside, R = 630: several blocks
    "straddle": [5, 260, 3, 0],                            # a video across the pass edge at its block's row 256, an empty video last
    "long": LONG,
    "ones257": [1] * 257,                                  # one past the video cap: a second block of one video
    "target": [0, 100, 100, 56, 1, 255, 2],                # two blocks that close exactly at the row target, an empty video first
}


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same_lists(got, want, what=""):
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


@functools.lru_cache(maxsize=None)
def exact_case(layout, E, dtype, seed=0):
    """Integer-valued rows and 17 queries in [-4, 4] (exact in bf16, every dot product exact in fp32) over LAYOUTS[layout], with planted
    ties: the last row of every video repeats its first (inside a video), the first row of every third video repeats the first row of
    video 0 or 1 (across videos and blocks), and in "long" the best possible row for sentence 0 stands twice in each long video, once
    in its first pass and once in its last.  -> (emb, q, offsets); shared, changed by no test."""
    off = offsets_of(LAYOUTS[layout])
    R, V = int(off[-1]), len(off) - 1
    g = torch.Generator().manual_seed(seed + 1000 * R + E)
    emb = torch.randint(-4, 5, (R, E), generator=g).float()
    q = torch.randint(-4, 5, (17, E), generator=g).float()
    owners = [v for v in range(V) if off[v + 1] > off[v]]
    for i, v in enumerate(owners):
        if off[v + 1] - off[v] > 1:
            emb[off[v + 1] - 1] = emb[off[v]]
        if i >= 2 and i % 3 == 2:
            emb[off[v]] = emb[off[owners[i % 2]]]
    if layout == "long":
        best = 4 * torch.sign(q[0])
        for v, first, last in ((1, 3, 290), (4, 10, 590)):
            emb[off[v] + first], emb[off[v] + last] = best, best
    return emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous(), off


# -- 1. exact data -------------------------------------------------------------------------------------------------------------------------

def test_the_layouts_cover_the_edges_of_the_plan():
    from drn_amd import _lib, plan_segment_blocks
    assert _lib.SHORTLIST_SEG_BLOCK == 256
    blocks = {k: plan_segment_blocks(offsets_of(v)).blk_vid.tolist() for k, v in LAYOUTS.items()}
    assert blocks["one"] == [0, 1] and blocks["ones"] == [0, 70] and blocks["ones257"] == [0, 256, 257]
    assert blocks["straddle"] == [0, 1, 2, 4] and blocks["long"] == [0, 1, 2, 4, 5, 7]
    assert blocks["target"] == [0, 4, 6, 7] and len(blocks["cycle"]) > 3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("E", [8, 40, 512])
def test_segment_shortlist_equals_the_reference_exactly(dtype, E):
    """Every layout at S = 1, 16, 17 and n = 1, 5, 128: ids, scores, n and rows equal to the float64 definition, bit for bit, with
    ties between videos and between the rows of a video in the data."""
    from drn_amd import Shortlister, segment_shortlist_reference
    for layout in LAYOUTS:
        emb, q17, off = exact_case(layout, E, dtype)
        sl = Shortlister(emb, offsets=off)
        assert len(sl) == len(off) - 1
        want = {n: segment_shortlist_reference(emb, off, q17, n) for n in (1, 5, 128)}
        if layout not in ("one", "ones", "ones257"):
            dot = q17.double() @ emb.double().t()
            video = torch.repeat_interleave(torch.arange(len(off) - 1), torch.as_tensor(np.diff(off))).to(DEV)
            top = torch.full((17, len(off) - 1), float("-inf"), dtype=torch.float64, device=DEV).scatter_reduce(
                1, video[None].expand(17, -1), dot, "amax")
            reached = torch.zeros_like(top).scatter_add(1, video[None].expand(17, -1), (dot == top[:, video]).double())
            assert bool((reached > 1).any()), "no tie inside a video"
        if layout not in ("one", "straddle"):                         # (straddle: three owners, a tie between them is not certain)
            w = want[128]
            assert bool(((w.scores[:, 1:] == w.scores[:, :-1]) & (w.ids[:, 1:] > w.ids[:, :-1]) & (w.ids[:, 1:] >= 0)).any()), "no tie"
        if layout == "long":
            w, peak = want[128], float(4 * q17[0].float().abs().sum())
            for v, first in ((1, 3), (4, 10)):
                at = w.ids[0].tolist().index(v)
                assert float(w.scores[0, at]) == peak and int(w.rows[0, at]) == first
        for S_ in (1, 16, 17):
            q = q17[:S_].contiguous()
            for n in (1, 5, 128):
                got = sl.shortlist(q, n)
                same_lists(got, type(got)(*(t[:S_] for t in want[n])), (layout, S_, n))


def test_segment_shortlist_with_odd_widths_reads_no_vector_past_a_row():
    """E = 5 (bf16 rows are not 16-byte aligned: the element-wise loader) and E = 36 (aligned rows, a partial last step)."""
    from drn_amd import Shortlister, segment_shortlist_reference
    for E in (5, 36):
        for dtype in (torch.bfloat16, torch.float32):
            for layout in ("cycle", "long"):
                emb, q17, off = exact_case(layout, E, dtype)
                q = q17[:3].contiguous()
                same_lists(Shortlister(emb, offsets=off).shortlist(q, 7), segment_shortlist_reference(emb, off, q, 7), (E, dtype, layout))


# -- 2. random data: the plain kernel's bits ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_table(R, E, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(R, E, generator=g).to(DEV, dtype).contiguous()
    q = torch.randn(17, E, generator=g).to(DEV, dtype).contiguous()
    return emb, q


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_one_row_per_video_is_the_plain_shortlist(dtype):
    from drn_amd import Shortlister
    V = 3 * 256 + 7
    emb, q = random_table(V, 200, dtype, 9)
    plain, seg = Shortlister(emb), Shortlister(emb, offsets=torch.arange(V + 1, device=DEV))
    for n in (1, 16, 128):
        a, b = plain.shortlist(q, n), seg.shortlist(q, n)
        for f in ("ids", "scores", "n"):
            assert torch.equal(getattr(a, f), getattr(b, f)), (n, f)
        assert bool((b.rows == 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_a_rows_score_does_not_depend_on_the_segmentation(dtype):
    """One table of 128 rows under three offset tables: every listed video's score is the maximum over its rows of the PLAIN kernel's
    scores of those rows, bit for bit, and rows names the lowest row that reaches it."""
    from drn_amd import Shortlister
    R = 128
    emb, q17 = random_table(R, 200, dtype, 21)
    q = q17[:5].contiguous()
    plain = Shortlister(emb).shortlist(q, R)
    assert int(plain.n.min()) == R
    per_row = torch.empty((5, R), dtype=torch.float32, device=DEV).scatter_(1, plain.ids.long(), plain.scores).cpu()
    for lens in ([128], [1, 3, 0, 17] * 6 + [2], [5, 0, 59, 36, 28, 0]):
        off = offsets_of(lens)
        assert off[-1] == R
        got = Shortlister(emb, offsets=off.tolist()).shortlist(q, R)
        owners = [v for v in range(len(lens)) if lens[v]]
        ids, scores, rows = got.ids.cpu(), got.scores.cpu(), got.rows.cpu()
        for s in range(5):
            assert int(got.n[s]) == len(owners) and sorted(ids[s, :len(owners)].tolist()) == owners
            for i in range(len(owners)):
                v = int(ids[s, i])
                mine = per_row[s, off[v]:off[v + 1]]
                assert float(scores[s, i]) == float(mine.max()) and int(rows[s, i]) == int((mine == mine.max()).nonzero()[0]), (lens, s, v)


def test_a_sentence_alone_and_a_shorter_cut_give_the_same_rows():
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 60 + [300]
    emb, q = random_table(int(sum(lens)), 200, torch.bfloat16, 33)
    sl = Shortlister(emb, offsets=offsets_of(lens))
    full = sl.shortlist(q, 128)
    assert int(full.n.min()) == 128
    for s in (0, 5, 16):
        alone = sl.shortlist(q[s:s + 1].contiguous(), 128)
        for f in FIELDS:
            assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]), (s, f)
    cut = sl.shortlist(q, 16)
    for f in ("ids", "scores", "rows"):
        assert torch.equal(getattr(cut, f), getattr(full, f)[:, :16]), f
    assert cut.n.tolist() == [16] * 17


def segment_case_ratio(emb, q, off, got):
    """The checks of random data -> the largest |error| / tol.  tol[s, v] = the maximum over v's rows of E * 2^-23 * sum_e |q[s, e] *
    emb[r, e]| (tests/test_shortlist_gpu.py derives the bound of one row; the error of a maximum is at most the largest error of its
    terms).  The returned score is within tol of the video's float64 maximum, so is the float64 score of the returned row, the list is
    sorted on the returned scores, and nobody left out is better than the last one listed by more than both tolerances."""
    E, V = int(emb.shape[1]), len(off) - 1
    lens = torch.as_tensor(np.diff(off), device=emb.device)
    toff = torch.as_tensor(off, device=emb.device)
    video = torch.repeat_interleave(torch.arange(V, device=emb.device), lens)[None].expand(q.shape[0], -1)
    dot = q.double() @ emb.double().t()
    tol_row = E * 2.0 ** -23 * (q.double().abs() @ emb.double().abs().t())
    ref = torch.full((q.shape[0], V), float("-inf"), dtype=torch.float64, device=emb.device).scatter_reduce(1, video, dot, "amax")
    tol = torch.zeros_like(ref).scatter_reduce(1, video, tol_row, "amax")
    worst = 0.0
    for s in range(q.shape[0]):
        n = int(got.n[s])
        ids, sc, rows = got.ids[s, :n].long(), got.scores[s, :n].double(), got.rows[s, :n].long()
        assert n == got.ids.shape[1] and len(set(ids.tolist())) == n and bool((lens[ids] > rows).all()) and bool((rows >= 0).all())
        err = (sc - ref[s, ids]).abs()
        assert bool((err <= tol[s, ids]).all()), s
        assert bool(((dot[s, toff[ids] + rows] - ref[s, ids]).abs() <= tol[s, ids]).all()), s
        worst = max(worst, float((err / tol[s, ids]).max()))
        assert bool(((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:-1] < ids[1:]))).all()), s
        out = lens > 0
        out[ids] = False
        last = ids[-1]
        assert bool((ref[s][out] <= ref[s, last] + tol[s][out] + tol[s, last]).all()), s
    return worst


def test_segment_shortlist_on_random_bf16_data_is_within_the_derived_bound():
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    emb, q17 = random_table(int(sum(lens)), 512, torch.bfloat16, 4)
    q, off = q17[:5].contiguous(), offsets_of(lens)
    ratio = segment_case_ratio(emb, q, off, Shortlister(emb, offsets=off).shortlist(q, 16))
    print("largest error / tol: %.4f" % ratio)
    assert ratio <= 1.0


# -- 3. a NaN query, buffers, graphs ---------------------------------------------------------------------------------------------------------

def test_a_nan_query_row_lists_nothing_and_leaves_the_others_alone():
    from drn_amd import Shortlister, segment_shortlist_reference
    emb, q, off = exact_case("cycle", 40, torch.bfloat16)
    sl = Shortlister(emb, offsets=off)
    clean = sl.shortlist(q, 9)
    bad = q.clone()
    bad[2, 7], bad[16, 0] = float("nan"), float("inf")                  # (inf * 0 is NaN somewhere, +-inf elsewhere: nothing finite)
    got = sl.shortlist(bad, 9)
    same_lists(got, segment_shortlist_reference(emb, off, bad, 9))
    assert int(got.n[2]) == 0 and bool((got.ids[2] == -1).all()) and bool((got.scores[2] == 0).all()) and bool((got.rows[2] == -1).all())
    keep = [s for s in range(17) if s not in (2, 16)]
    for f in FIELDS:
        assert torch.equal(getattr(got, f)[keep], getattr(clean, f)[keep]), f


def test_out_buffers_are_written_in_place_and_a_captured_segment_shortlist_replays():
    from drn_amd import SegmentShortlist, Shortlister, segment_shortlist_reference
    from drn_amd.graph import capture_graph
    emb, q17, off = exact_case("cycle", 40, torch.bfloat16)
    emb2, q17b, _ = exact_case("cycle", 40, torch.bfloat16, seed=7)
    q, q2 = q17[:5].contiguous(), q17b[:5].contiguous()
    sl = Shortlister(emb, offsets=off)
    n, GUARD = 100, 64                                                   # (n above a sentence's 64-lane stride, below the cap)
    shapes = ((5, n), (5, n), (5,), (5, n))
    dtypes = (torch.int32, torch.float32, torch.int32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = SegmentShortlist(*(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes)))

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)
    got = sl.shortlist(q, n, out=out)
    assert all(a is b for a, b in zip(got, out)) and guards_hold()
    same_lists(out, segment_shortlist_reference(emb, off, q, n), "every element")
    small = Shortlister(emb[:4].contiguous(), offsets=[0, 1, 1, 4])
    for t in out:
        t.fill_(77)
    same_lists(small.shortlist(q, n, out=out), segment_shortlist_reference(emb[:4], [0, 1, 1, 4], q, n), "the tail past the list")
    assert guards_hold()
    # capture on one stream, then replay on other queries written into the captured buffer
    qbuf = q.clone()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist(qbuf, n, out=out)                                   # (warm: the workspace of this shape exists)
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
        same_lists(out, sl.shortlist(queries, n), "replay == eager")
        same_lists(out, segment_shortlist_reference(emb, off, queries, n), "replay == reference")
    assert guards_hold()


# -- 4. the two stages -----------------------------------------------------------------------------------------------------------------------

def test_segment_ids_are_device_candidates_of_the_search():
    """search(candidates=seg.ids) on a plain index == the same rows passed as host lists at the same T; between the queries and the Hits
    the host reads nothing (torch raises on a synchronising call meanwhile) and the shortlist is one tagged entry."""
    from drn_amd import Grounder, Shortlister, ops
    m, store, index, kw = world("plain")
    lens = [3, 1, 0, 17, 2, 5, 1]
    assert len(lens) == NV
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (int(off[-1]), 16), generator=g).float()
    emb[off[4]] = emb[off[1]]                                             # a tie between videos the shortlist breaks by position
    sl = Shortlister(emb.to(DEV).contiguous(), names=store.names, offsets=off)
    sl.check(store), sl.check(index)
    qe = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    qe[1] = float("nan")                                                  # a sentence whose shortlist is empty: ids all -1
    grounder = Grounder(m, top_k=5, **kw)
    tok, qlen = sentences(7)
    n = 4
    sl.shortlist(qe, n), grounder.search(tok, qlen, index, per_video=2, candidates=sl.shortlist(qe, n).ids)     # (warm)
    torch.cuda.synchronize()
    ops.kernel_timer = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        short = sl.shortlist(qe, n)
        tags = [t[0] for t in ops.kernel_timer]
        got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    assert tags == ["shortlist_segments_topn"]
    lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
    assert [len(l) for l in lists] == [n, 0, n] and all(2 not in l for l in lists)
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "two stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0
