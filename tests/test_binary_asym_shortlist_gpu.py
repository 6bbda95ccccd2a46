"""Asymmetric binary shortlists on the device: BinaryShortlister.shortlist_asym and the asymmetric() view (drn_shortlist_bin_asym,
csrc/retrieve_bin_asym.hip: the plain shortlist's MFMA chain with its table operand built from the code bits, then the merges and the
segment look-up of the other shortlists).  The launch IS the plain shortlist over the +-1 table the codes stand for, so every field is
compared with torch.equal to dequantized().shortlist_deep(q, n, allow) -- on any data -- and, on EXACT data (integer queries in [-8, 8]:
every sum is an integer of at most 8 * 512 = 4096, exact in fp32 whatever the order of the additions), to
binary_asym_shortlist_reference computed on the host.  Rows repeated and rows negated make ties: the total order (score descending,
position ascending, lowest segment) is what is tested.
tests/test_binary_asym_shortlist_cpu.py holds the definition, the refusals and the C boundary."""
import warnings

import numpy as np
import pytest
import torch

from drn_amd.binary import binary_asym_shortlist_reference  # noqa: F401  (without the definition nothing below can run)
from test_binary_shortlist_gpu import masks_of, on_device, packed, rows_of, same_lists

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
# W = 1 with 24 pad bits (one tail step, zeros past E on both sides); W = 1; W = 2 with pad bits (a whole step and a tail step); W = 3
# (word loads); W = 16 (16-byte loads)
WIDTHS = pytest.mark.parametrize("E", [8, 32, 40, 96, 512])
DEPTHS = (1, 5, 128, 300, 1024)
CYCLING = [1, 3, 0, 17] * 75


def exact_table_and_queries(V, E, dtype, seed=0):
    """V rows of random +-1 with whole rows repeated (equal scores at different positions, across blocks) and rows negated, and 17
    query rows of integers in [-8, 8] -> on the device.  Every score is an integer of magnitude at most 8 E."""
    g = torch.Generator().manual_seed(seed + 1000 * V + E)
    emb = torch.where(torch.rand(V, E, generator=g) < 0.5, -1.0, 1.0)
    for a, b in ((1, 0), (V - 1, 0), (V // 2, V // 3), (256, 0), (261, 70), (70, 5)):
        if 0 <= a < V and 0 <= b < V:
            emb[a] = emb[b]
    for a, b in ((2, 0), (V - 2, 3), (257, 5)):
        if 0 <= a < V and 0 <= b < V:
            emb[a] = -emb[b]
    q = torch.randint(-8, 9, (17, E), generator=g).float()
    return emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous()


def random_table_and_queries(V, E, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * V + E)
    return torch.randn(V, E, generator=g).to(DEV, dtype).contiguous(), torch.randn(17, E, generator=g).to(DEV, dtype).contiguous()


def check(sl, oracle, q17, n, S_, mask=None, what=""):
    """One call on EXACT data against the oracle on the device and the definition from the host -> the result."""
    q = q17[:S_].contiguous()
    allow = None if mask is None else packed(mask if mask.dim() == 1 else mask[:S_].contiguous())
    got = sl.shortlist_asym(q, n, allow=allow)
    same_lists(got, oracle.shortlist_deep(q, n, allow=allow), (what, "oracle", n, S_))
    want = binary_asym_shortlist_reference(sl.codes.cpu(), sl.E, q.cpu(), n, offsets=None if sl.offsets is None else sl.offsets.cpu(),
                                           allow=None if mask is None else (mask if mask.dim() == 1 else mask[:S_]))
    same_lists(got, on_device(want), (what, "definition", n, S_))
    return got


def has_a_tie(lists):
    return bool(((lists.scores[:, 1:] == lists.scores[:, :-1]) & (lists.ids[:, 1:] > lists.ids[:, :-1]) & (lists.ids[:, 1:] >= 0)).any())


# -- 1. one row per video ---------------------------------------------------------------------------------------------------------------

@DTYPES
@WIDTHS
def test_asymmetric_shortlist_equals_the_oracle_and_the_definition(dtype, E):
    """V: one video; a block's quarter less one, exactly, plus one; one block + 1; three blocks + 7.  n: both ends, around 128 / 300,
    the cap; n > V is padding.  S = 17 is a second sentence tile of one row.  Through the method and through the view."""
    from drn_amd import BinaryShortlister, Shortlist
    for V in (1, 63, 64, 65, 257, 775):
        emb, q17 = exact_table_and_queries(V, E, dtype)
        sl = BinaryShortlister(emb)
        oracle, view = sl.dequantized(), sl.asymmetric()
        assert len(sl) == V and oracle.embeddings.dtype == dtype and torch.equal(oracle.embeddings, emb)
        for n in DEPTHS:
            want17 = on_device(binary_asym_shortlist_reference(sl.codes.cpu(), E, q17.cpu(), n))
            if 2 < V <= n:
                assert has_a_tie(want17), "no tie in the data"
            for S_ in (1, 16, 17):
                q = q17[:S_].contiguous()
                got = sl.shortlist_asym(q, n)
                assert isinstance(got, Shortlist) and tuple(got.ids.shape) == (S_, n)
                same_lists(got, rows_of(want17, S_), (V, n, S_, "definition"))
                same_lists(got, oracle.shortlist_deep(q, n), (V, n, S_, "oracle"))
                assert bool((got.n == min(n, V)).all())
            same_lists(view.shortlist(q17, n), got, (V, n, "view.shortlist"))
            same_lists(view.shortlist_deep(q17, n), got, (V, n, "view.shortlist_deep"))


@DTYPES
@pytest.mark.parametrize("E", [8, 40, 96, 512])
def test_random_data_lists_equal_the_oracle_and_scores_are_within_the_bound_of_the_definition(dtype, E):
    """On random data the lists are the oracle Shortlister's, field for field, and every listed score is within the project's bound for
    an fp32 dot product, E * 2^-23 * sum_e |q_e| |x_e| with |x_e| = 1, of the float64 score of the same pair."""
    from drn_amd import BinaryShortlister
    off = np.concatenate([[0], np.cumsum(CYCLING)])
    worst = 0.0
    for kw, V in (({}, 775), ({"offsets": off}, int(off[-1]))):
        emb, q17 = random_table_and_queries(V, E, dtype, seed=12)
        sl = BinaryShortlister(emb, **kw)
        oracle = sl.dequantized()
        for n in (5, 300):
            got = sl.shortlist_asym(q17, n)
            same_lists(got, oracle.shortlist_deep(q17, n), (E, n, bool(kw)))
            assert int(got.n.min()) == min(n, 775 if not kw else 225)
            wide = oracle.embeddings.double()
            listed = got.ids >= 0
            row = got.ids.long().clamp(min=0)
            if kw:
                row = sl.offsets.to(DEV).long()[row] + got.rows.long().clamp(min=0)
            exact = (q17.double()[:, None, :] * wide[row]).sum(dim=2)
            bound = (E * 2.0 ** -23 * q17.double().abs().sum(dim=1))[:, None].expand_as(exact)
            err = (got.scores.double() - exact).abs()
            worst = max(worst, float((err / bound)[listed].max()))
            print("E = %d %s n = %d ragged = %s: the largest |error| / bound is %.4f" % (E, dtype, n, bool(kw), float((err / bound)[listed].max())))
            assert bool((err <= bound)[listed].all())
    assert worst <= 1.0


def test_one_tag_a_call_and_the_hamming_shortlist_is_unchanged_afterwards():
    from drn_amd import BinaryShortlister, binary_shortlist_reference, ops
    off = np.concatenate([[0], np.cumsum(CYCLING)])
    for kw, V in (({}, 300), ({"offsets": off}, int(off[-1]))):
        emb, q17 = exact_table_and_queries(V, 96, torch.bfloat16)
        sl = BinaryShortlister(emb, **kw)
        ops.kernel_timer = []
        try:
            sl.shortlist_asym(q17, 16)
            sl.asymmetric().shortlist_deep(q17, 300)
            tags = [t[0] for t in ops.kernel_timer]
        finally:
            ops.kernel_timer = None
        assert tags == ["shortlist_bin_asym", "shortlist_bin_asym"]
        for n in (16, 300):                                                      # (the workspaces of (17, 16) and (17, 300) are shared)
            want = binary_shortlist_reference(sl.codes.cpu(), 96, q17.cpu(), n, offsets=None if sl.offsets is None else sl.offsets.cpu())
            same_lists(sl.shortlist(q17, n), on_device(want), ("Hamming afterwards", n))


# -- 2. ragged tables ---------------------------------------------------------------------------------------------------------------------

@DTYPES
@WIDTHS
def test_asymmetric_segment_shortlist_equals_the_oracle_and_the_definition(dtype, E):
    """R = V = 1; run lengths cycling 1 / 3 / 0 / 17 over 300 videos (several blocks of the plan, videos without rows); 257 videos of
    one row (two blocks), which must answer like the plain table with rows = 0."""
    from drn_amd import BinaryShortlister, SegmentShortlist
    emb, q17 = exact_table_and_queries(1, E, dtype, seed=1)
    sl = BinaryShortlister(emb, offsets=[0, 1])
    for n in (1, 300):
        got = check(sl, sl.dequantized(), q17, n, 17, what="R = V = 1")
        assert bool((got.n == 1).all()) and bool((got.ids[:, 0] == 0).all()) and bool((got.rows[:, 0] == 0).all())
    off = np.concatenate([[0], np.cumsum(CYCLING)])
    emb, q17 = exact_table_and_queries(int(off[-1]), E, dtype, seed=1)
    sl = BinaryShortlister(emb, offsets=off)
    oracle = sl.dequantized()
    assert len(sl) == 300 and len(sl.plan.blk_vid) - 1 > 4
    for n in DEPTHS:
        for S_ in (1, 17):
            got = check(sl, oracle, q17, n, S_, what="cycling")
            assert isinstance(got, SegmentShortlist) and bool((got.n == min(n, 225)).all())
    emb, q17 = exact_table_and_queries(257, E, dtype, seed=2)
    sl, plain = BinaryShortlister(emb, offsets=np.arange(258)), BinaryShortlister(emb)
    oracle = sl.dequantized()
    assert len(sl.plan.blk_vid) - 1 == 2
    for n in (5, 300):
        got = check(sl, oracle, q17, n, 17, what="one row a video")
        flat = plain.shortlist_asym(q17, n)
        for f in flat._fields:
            assert torch.equal(getattr(got, f), getattr(flat, f)), (n, f)
        assert bool((got.rows[got.ids >= 0] == 0).all()) and bool((got.rows[got.ids < 0] == -1).all())


@DTYPES
@pytest.mark.parametrize("E", [40, 512])
def test_long_videos_are_walked_in_passes_and_rows_names_the_lowest_tied_segment(dtype, E):
    """Videos of 300 and 600 rows -- two and three passes of 256 rows, each alone in its block.  The best score there is, sum_e |q_e|
    (the row of the query's own signs), is planted in the first pass and again in the last (sentence 0, video 1: segments 5 and 299;
    sentence 2, video 3: segments 10 and 590): the lowest wins.  Planted in the last pass alone (sentence 1, video 3: segment 599) it
    is found there."""
    from drn_amd import BinaryShortlister
    lens = [2, 300, 1, 600, 3]
    off = np.concatenate([[0], np.cumsum(lens)])
    emb, q17 = exact_table_and_queries(int(off[-1]), E, dtype, seed=3)
    q17[:3] = torch.where(q17[:3] == 0, torch.ones_like(q17[:3]), q17[:3])       # (no zero: the best row is the only one of its score)
    for s, v, segments in ((0, 1, (5, 299)), (2, 3, (10, 590)), (1, 3, (599,))):
        for j in segments:
            emb[int(off[v]) + j] = torch.where(q17[s] < 0, -1.0, 1.0).to(dtype)
    sl = BinaryShortlister(emb, offsets=off)
    oracle = sl.dequantized()
    for v in (1, 3):
        b = int(sl.plan.vid_blk[v])
        assert int(sl.plan.blk_vid[b]) == v and int(sl.plan.blk_vid[b + 1]) == v + 1, "the long video is not alone in its block"
    for n in (1, 5, 300):
        got = check(sl, oracle, q17, n, 17, what="long videos")
        for s, v, seg in ((0, 1, 5), (2, 3, 10), (1, 3, 599)):
            best = float(q17[s].float().abs().sum())
            assert int(got.ids[s, 0]) == v and float(got.scores[s, 0]) == best and int(got.rows[s, 0]) == seg, (n, s)
    same_lists(check(sl, oracle, q17, 5, 1), rows_of(sl.shortlist_asym(q17, 5), 1), "sentence 0 alone")


# -- 3. masks -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
@pytest.mark.parametrize("E", [40, 512])
def test_asymmetric_shortlists_under_masks_equal_the_masked_definition(ragged, E):
    """A shared mask with one whole block dark; a mask per sentence with an all-zero row (lists nothing), a one-bit row and the dark
    block; every bit past V set in the packed words; the all-ones mask -- shared and per sentence -- is allow=None."""
    from drn_amd import BinaryShortlister
    if ragged:
        off = np.concatenate([[0], np.cumsum(CYCLING + [5])])
        emb, q17 = exact_table_and_queries(int(off[-1]), E, torch.bfloat16, seed=4)
        sl = BinaryShortlister(emb, offsets=off)
        dark = slice(int(sl.plan.blk_vid[1]), int(sl.plan.blk_vid[2]))
    else:
        emb, q17 = exact_table_and_queries(775, E, torch.bfloat16, seed=4)
        sl = BinaryShortlister(emb)
        dark = slice(256, 512)
    oracle, V = sl.dequantized(), len(sl)
    assert V % 32 and dark.stop > dark.start
    shared, per = masks_of(V)
    shared[dark] = False
    per[:, dark] = False
    ones = torch.ones(V, dtype=torch.bool)
    for n in (5, 128, 1024):
        plain = check(sl, oracle, q17, n, 17)
        same_lists(check(sl, oracle, q17, n, 17, mask=ones), plain, ("all ones", n))
        same_lists(check(sl, oracle, q17, n, 17, mask=ones[None, :].expand(17, V).contiguous()), plain, ("all ones a sentence", n))
        got = check(sl, oracle, q17, n, 17, mask=shared, what="shared")
        assert not bool(((got.ids >= dark.start) & (got.ids < dark.stop)).any())
        got = check(sl, oracle, q17, n, 17, mask=per, what="per sentence")
        assert int(got.n[2]) == 0 and bool((got.ids[2] == -1).all()) and bool((got.scores[2] == 0).all())
        assert got.n[5].item() == 1 and got.ids[5, 0].item() == V - 1
        check(sl, oracle, q17, n, 1, mask=per, what="one sentence of a mask per sentence")
    assert int(got.n.max()) > 50


# -- 4. what a score depends on -----------------------------------------------------------------------------------------------------------

@DTYPES
def test_a_query_row_that_is_not_finite_lists_nothing_and_leaves_the_others_alone(dtype):
    from drn_amd import BinaryShortlister
    for kw in ({}, {"offsets": np.concatenate([[0], np.cumsum([1, 3, 0, 17] * 37)])}):
        emb, q17 = exact_table_and_queries(777, 96, dtype, seed=6)
        sl = BinaryShortlister(emb, **kw)
        oracle = sl.dequantized()
        clean = sl.shortlist_asym(q17, 300)
        bad = q17.clone()
        bad[2, 95], bad[16, 0], bad[7, 40] = float("nan"), float("inf"), float("-inf")
        got = check(sl, oracle, bad, 300, 17)
        for s in (2, 16, 7):
            assert int(got.n[s]) == 0 and bool((got.ids[s] == -1).all()) and bool((got.scores[s] == 0).all())
        keep = [s for s in range(17) if s not in (2, 16, 7)]
        for f in got._fields:
            assert torch.equal(getattr(got, f)[keep], getattr(clean, f)[keep]), f
        assert int(got.n[keep].min()) > 0


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_a_sentence_alone_and_a_prefix_of_the_table_give_the_same_bits(ragged):
    """Random bf16 data: the bits of a score depend on its own (sentence, row) pair alone."""
    from drn_amd import BinaryShortlister
    off = np.concatenate([[0], np.cumsum(CYCLING)])
    emb, q17 = random_table_and_queries(int(off[-1]) if ragged else 775, 512, torch.bfloat16, seed=8)
    sl = BinaryShortlister(emb, **({"offsets": off} if ragged else {}))
    full = sl.shortlist_asym(q17, 1024)
    for s in (0, 9, 16):
        alone = sl.shortlist_asym(q17[s:s + 1].contiguous(), 1024)
        for f in full._fields:
            assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]), (s, f)
    # the first K videos as a table of their own == the full table under the mask of the first K
    K = 130
    first = BinaryShortlister(emb[:int(off[K])].contiguous(), offsets=off[:K + 1]) if ragged else BinaryShortlister(emb[:K].contiguous())
    mask = torch.zeros(len(sl), dtype=torch.bool)
    mask[:K] = True
    same_lists(first.shortlist_asym(q17, 1024), sl.shortlist_asym(q17, 1024, allow=packed(mask)), "a prefix")


# -- 5. buffers and graphs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_out_buffers_in_place_and_a_replay_follows_queries_and_mask_written_in_place(ragged):
    """out= inside guard bands: every element written, nothing outside them -- also where the table is shorter than n.  One captured
    graph, replayed with the queries and the mask's words changed in place, equals eager; one tag is recorded a call."""
    from drn_amd import BinaryShortlister, ops
    from drn_amd.graph import capture_graph
    off = np.concatenate([[0], np.cumsum([1, 3, 0, 17] * 90)])
    emb, q17 = exact_table_and_queries(int(off[-1]), 96, torch.bfloat16, seed=9)
    sl = BinaryShortlister(emb, **({"offsets": off} if ragged else {}))
    oracle = sl.dequantized()
    V = len(sl)
    _, per = masks_of(V, seed=1)
    q, q2 = q17[:5].contiguous(), q17[5:10].contiguous()
    n, GUARD = 300, 64
    shapes = ((5, n), (5, n), (5,), (5, n))[:4 if ragged else 3]
    dtypes = (torch.int32, torch.float32, torch.int32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = tuple(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes))

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)
    ops.kernel_timer = []
    try:
        got = sl.shortlist_asym(q, n, out=out)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags == ["shortlist_bin_asym"]
    assert all(a is b for a, b in zip(got, out)) and guards_hold()
    same_lists(got, oracle.shortlist_deep(q, n), "every element")
    assert int(got.n.min()) == (n if not ragged else min(n, 270))
    words = packed(per[:5].contiguous())
    qbuf = q.clone()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist_asym(qbuf, n, out=out, allow=words)                        # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sl.shortlist_asym(qbuf, n, out=out, allow=words)
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


# -- 6. the cascade ----------------------------------------------------------------------------------------------------------------------

def test_evaluate_cascade_takes_the_asymmetric_view_and_ranks_like_the_cascade_by_hand():
    """coarse: the asymmetric view of the sign codes of the fine table's rows, depth 300; fine: rerank to 128.  The ranks are the
    target's place in the reranked list, -1 where the coarse stage missed it.  Sentences 0..7 of a batch ARE a table row, their target
    (no row scores higher against it than its own signs: listed); the others' target is the first video their coarse list lacks."""
    from drn_amd import BinaryShortlister, ShortlistRecall, Shortlister, evaluate_cascade, metrics
    V = 775
    names = ["v%d" % v for v in range(V)]
    emb, q17 = random_table_and_queries(V, 96, torch.bfloat16, seed=10)
    binary, fine = BinaryShortlister(emb, names=names), Shortlister(emb, names=names)
    coarse = binary.asymmetric()
    depth, topks = 300, (1, 10, 128)
    batches = []
    for S_ in (17, 11):
        q = q17[:S_].clone()
        targets = [10 + 3 * s + S_ for s in range(8)]
        q[:8] = emb[targets]
        lists = binary.shortlist_asym(q, depth).ids.cpu().tolist()
        targets += [min(set(range(V)) - set(lists[s])) for s in range(8, S_)]
        batches.append(([names[t] for t in targets], q, q))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = evaluate_cascade(coarse, fine, iter(batches), depth, topks=topks, deep=True)
    assert isinstance(got, ShortlistRecall) and got.n == 28
    want = []
    for bnames, cq, fq in batches:
        listed = binary.shortlist_asym(cq, depth)
        assert bool((listed.n == depth).all())
        reranked = fine.rerank(listed.ids, fq, n=128).ids.cpu()
        for s, name in enumerate(bnames):
            place = (reranked[s] == names.index(name)).nonzero()
            want.append(int(place[0, 0]) if len(place) else -1)
    want = np.asarray(want, dtype=np.int32)
    assert got.ranks.dtype == np.int32 and np.array_equal(got.ranks, want)
    assert (want >= 0).any() and (want < 0).any()
    assert got.recall == metrics.recall_from_ranks(want, list(topks))
