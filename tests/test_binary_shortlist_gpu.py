"""Binary shortlists on the device: BinaryShortlister.shortlist / shortlist_deep (drn_shortlist_bin, csrc/retrieve_bin.hip: XOR and
popcount, then the merges and the segment look-up of the other shortlists).  Scores are integers, so every field is compared with
torch.equal -- to dequantized().shortlist_deep(binary_signs(q), n, allow), the plain Shortlister over the +-1 table the codes stand
for, and to binary_shortlist_reference computed on the host and brought to the device -- and ties are everywhere: the total order
(score descending, position ascending, lowest segment) is what is tested.
tests/test_binary_shortlist_cpu.py holds the format, the definition, the refusals and the C boundary."""
import warnings

import numpy as np
import pytest
import torch

from drn_amd.binary import BinaryShortlister  # noqa: F401  (without the module nothing below can run)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
WIDTHS = pytest.mark.parametrize("E", [32, 40, 96, 512])    # W = 1; W = 2 with pad bits; W = 3 (word loads); W = 16 (16-byte loads)
DEPTHS = (1, 5, 128, 300, 1024)


def same_lists(got, want, what=""):
    assert type(got) is type(want), what
    for f in got._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


def rows_of(want, S_):
    return type(want)(*(t[:S_].contiguous() for t in want))


def on_device(lists):
    return type(lists)(*(t.to(DEV) for t in lists))


def signed(rows, E, seed):
    """Random values with both zeros sprinkled in (+0 and -0 are bit 1) -- on the host, float32."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + E)
    x = torch.randn(rows, E, generator=g)
    z = torch.rand(rows, E, generator=g)
    x[z < 0.05] = 0.0
    x[z > 0.95] = -0.0
    return x


def table_and_queries(V, E, dtype, seed=0):
    """V rows with whole rows repeated (equal scores at different positions, across blocks) and 17 queries -> on the device."""
    emb = signed(V, E, seed)
    for a, b in ((1, 0), (V - 1, 0), (V // 2, V // 3), (256, 0), (261, 70), (70, 5)):
        if 0 <= a < V and 0 <= b < V:
            emb[a] = emb[b]
    return emb.to(DEV, dtype).contiguous(), signed(17, E, seed + 7).to(DEV, dtype).contiguous()


def packed(mask):
    """pack_allow_reference of a host bool mask, on the device, with EVERY bit past V set: the kernels must ignore them."""
    from drn_amd import pack_allow_reference
    V = int(mask.shape[-1])
    words = pack_allow_reference(mask).copy().view(np.uint32)
    if V % 32:
        words[..., -1] |= np.uint32((0xffffffff << (V % 32)) & 0xffffffff)
    return torch.from_numpy(words.view(np.int32)).to(DEV).contiguous()


def masks_of(V, seed=0):
    """-> (shared (V,), per sentence (17, V)) on the host: random halves, row 2 all zero, row 5 a single bit (the last video)."""
    g = torch.Generator().manual_seed(seed + V)
    per = torch.rand(17, V, generator=g) < 0.5
    per[2] = False
    per[5] = False
    per[5, V - 1] = True
    return per[0].clone(), per


def check(sl, oracle, q17, n, S_, mask=None, what=""):
    """One call against the oracle on the device and the definition from the host -> the result."""
    from drn_amd import binary_shortlist_reference, binary_signs
    q = q17[:S_].contiguous()
    allow = None if mask is None else packed(mask if mask.dim() == 1 else mask[:S_].contiguous())
    got = sl.shortlist(q, n, allow=allow)
    same_lists(got, oracle.shortlist_deep(binary_signs(q), n, allow=allow), (what, "oracle", n, S_))
    want = binary_shortlist_reference(sl.codes.cpu(), sl.E, q.cpu(), n, offsets=None if sl.offsets is None else sl.offsets.cpu(),
                                      allow=None if mask is None else (mask if mask.dim() == 1 else mask[:S_]))
    same_lists(got, on_device(want), (what, "definition", n, S_))
    return got


# -- 1. one row per video ---------------------------------------------------------------------------------------------------------------

@DTYPES
@WIDTHS
def test_binary_shortlist_equals_the_oracle_and_the_definition(dtype, E):
    """V: one video; a block's quarter less one, exactly, plus one; one block + 1; three blocks + 7.  n: both ends, around the two
    merges' border (128 / 300), the cap; n > V is padding.  S = 17 is a second sentence tile of one row.  Under both names."""
    from drn_amd import BinaryShortlister, Shortlist, binary_shortlist_reference, binary_signs
    for V in (1, 63, 64, 65, 257, 775):
        emb, q17 = table_and_queries(V, E, dtype)
        sl = BinaryShortlister(emb)
        oracle = sl.dequantized()
        assert len(sl) == V and sl.nbytes == V * 4 * -(-E // 32) and oracle.embeddings.dtype == dtype
        for n in DEPTHS:
            want17 = on_device(binary_shortlist_reference(sl.codes.cpu(), E, q17.cpu(), n))
            if 1 < V <= n:
                assert bool(((want17.scores[:, 1:] == want17.scores[:, :-1]) & (want17.ids[:, 1:] > want17.ids[:, :-1])
                             & (want17.ids[:, 1:] >= 0)).any()), "no tie in the data"
            for S_ in (1, 16, 17):
                q = q17[:S_].contiguous()
                got = sl.shortlist(q, n)
                assert isinstance(got, Shortlist) and tuple(got.ids.shape) == (S_, n)
                same_lists(got, rows_of(want17, S_), (V, n, S_, "definition"))
                same_lists(got, oracle.shortlist_deep(binary_signs(q), n), (V, n, S_, "oracle"))
                same_lists(sl.shortlist_deep(q, n), got, (V, n, S_, "shortlist_deep == shortlist"))
                assert bool((got.n == min(n, V)).all())
                assert bool((got.scores == got.scores.round()).all()) and float(got.scores.abs().max()) <= E
                assert bool(((got.scores.int() - E) % 2 == 0)[got.ids >= 0].all()), "a score is E - 2 h"


def test_one_tag_a_call_and_the_ops_wrapper_is_the_entry():
    from drn_amd import BinaryShortlister, ops
    emb, q17 = table_and_queries(300, 96, torch.bfloat16)
    sl = BinaryShortlister(emb)
    ops.kernel_timer = []
    try:
        sl.shortlist(q17, 16)
        sl.shortlist_deep(q17, 300)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags == ["shortlist_bin", "shortlist_bin"]


# -- 2. ragged tables ---------------------------------------------------------------------------------------------------------------------

@DTYPES
@WIDTHS
def test_binary_segment_shortlist_equals_the_oracle_and_the_definition(dtype, E):
    """Run lengths cycling 1 / 3 / 0 / 17 over 300 videos (several blocks of the plan, videos without rows); 257 videos of one row
    (two blocks), which must answer like the plain table with rows = 0."""
    from drn_amd import BinaryShortlister, SegmentShortlist
    lens = [1, 3, 0, 17] * 75
    off = np.concatenate([[0], np.cumsum(lens)])
    emb, q17 = table_and_queries(int(off[-1]), E, dtype, seed=1)
    sl = BinaryShortlister(emb, offsets=off)
    oracle = sl.dequantized()
    assert len(sl) == 300 and len(sl.plan.blk_vid) - 1 > 4
    for n in DEPTHS:
        for S_ in (1, 17):
            got = check(sl, oracle, q17, n, S_, what="cycling")
            assert isinstance(got, SegmentShortlist) and bool((got.n == min(n, 225)).all())
    emb, q17 = table_and_queries(257, E, dtype, seed=2)
    sl, plain = BinaryShortlister(emb, offsets=np.arange(258)), BinaryShortlister(emb)
    oracle = sl.dequantized()
    assert len(sl.plan.blk_vid) - 1 == 2
    for n in (5, 300):
        got = check(sl, oracle, q17, n, 17, what="one row a video")
        flat = plain.shortlist(q17, n)
        for f in flat._fields:
            assert torch.equal(getattr(got, f), getattr(flat, f)), (n, f)
        assert bool((got.rows[got.ids >= 0] == 0).all()) and bool((got.rows[got.ids < 0] == -1).all())


@DTYPES
@pytest.mark.parametrize("E", [40, 512])
def test_long_videos_are_walked_in_passes_and_rows_names_the_lowest_tied_segment(dtype, E):
    """Videos of 300 and 600 rows -- two and three passes of 256 rows, each alone in its block.  The best score, E, is planted in the
    first pass and again in the last (sentence 0, video 1: segments 5 and 299; sentence 2, video 3: segments 10 and 590): the lowest
    wins.  Planted in the last pass alone (sentence 1, video 3: segment 599) it is found there."""
    from drn_amd import BinaryShortlister
    lens = [2, 300, 1, 600, 3]
    off = np.concatenate([[0], np.cumsum(lens)])
    emb, q17 = table_and_queries(int(off[-1]), E, dtype, seed=3)
    for s, v, segments in ((0, 1, (5, 299)), (2, 3, (10, 590)), (1, 3, (599,))):
        for j in segments:
            emb[int(off[v]) + j] = q17[s]
    sl = BinaryShortlister(emb, offsets=off)
    oracle = sl.dequantized()
    for v in (1, 3):
        b = int(sl.plan.vid_blk[v])
        assert int(sl.plan.blk_vid[b]) == v and int(sl.plan.blk_vid[b + 1]) == v + 1, "the long video is not alone in its block"
    for n in (1, 5, 300):
        got = check(sl, oracle, q17, n, 17, what="long videos")
        for s, v, seg in ((0, 1, 5), (2, 3, 10), (1, 3, 599)):
            assert int(got.ids[s, 0]) == v and float(got.scores[s, 0]) == E and int(got.rows[s, 0]) == seg, (n, s)
    same_lists(check(sl, oracle, q17, 5, 1), rows_of(sl.shortlist(q17, 5), 1), "sentence 0 alone")


# -- 3. masks -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
@pytest.mark.parametrize("E", [40, 512])
def test_binary_shortlists_under_masks_equal_the_masked_definition(ragged, E):
    """A shared mask; a mask per sentence with an all-zero row (lists nothing) and a one-bit row; every bit past V set in the packed
    words; the all-ones mask -- shared and per sentence -- is allow=None."""
    from drn_amd import BinaryShortlister
    if ragged:
        lens = [1, 3, 0, 17] * 75 + [5]
        off = np.concatenate([[0], np.cumsum(lens)])
        emb, q17 = table_and_queries(int(off[-1]), E, torch.bfloat16, seed=4)
        sl = BinaryShortlister(emb, offsets=off)
    else:
        emb, q17 = table_and_queries(775, E, torch.bfloat16, seed=4)
        sl = BinaryShortlister(emb)
    oracle, V = sl.dequantized(), len(sl)
    assert V % 32
    shared, per = masks_of(V)
    ones = torch.ones(V, dtype=torch.bool)
    for n in (5, 128, 1024):
        plain = check(sl, oracle, q17, n, 17)
        same_lists(check(sl, oracle, q17, n, 17, mask=ones), plain, ("all ones", n))
        same_lists(check(sl, oracle, q17, n, 17, mask=ones[None, :].expand(17, V).contiguous()), plain, ("all ones a sentence", n))
        check(sl, oracle, q17, n, 17, mask=shared, what="shared")
        got = check(sl, oracle, q17, n, 17, mask=per, what="per sentence")
        assert int(got.n[2]) == 0 and bool((got.ids[2] == -1).all()) and bool((got.scores[2] == 0).all())
        assert got.n[5].item() == 1 and got.ids[5, 0].item() == V - 1
        check(sl, oracle, q17, n, 1, mask=per, what="one sentence of a mask per sentence")
    assert int(got.n.max()) > 100


# -- 4. the codes -------------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [40, 96, 512])
def test_codes_built_on_the_device_equal_the_definition_across_a_chunk_boundary(dtype, E, monkeypatch):
    """23 rows packed 5 at a time (the last chunk is short), both zeros among the values; the wide table is not kept."""
    from drn_amd import BinaryShortlister, binary, binary_quantize_reference
    emb = signed(23, E, 11).to(DEV, dtype).contiguous()
    assert bool((emb == 0).any()) and bool(torch.signbit(emb[emb == 0]).any())
    want = binary_quantize_reference(emb.cpu())
    whole = BinaryShortlister(emb)
    monkeypatch.setattr(binary, "BINARY_PACK_ELEMS", 5 * E + 3)
    for sl in (whole, BinaryShortlister(emb), BinaryShortlister(emb, offsets=[0, 20, 23])):
        assert sl.codes.dtype == torch.int32 and sl.codes.is_contiguous() and torch.equal(sl.codes.cpu(), want)
        assert sl.codes.cpu().numpy().tobytes() == want.numpy().tobytes()
        assert all(v is not emb for v in vars(sl).values()), "a reference to the wide table is kept"
        assert sl.dtype == dtype and sl.E == E and sl.device == emb.device
    assert torch.equal(binary_quantize_reference(emb).cpu(), want)              # (a device tensor in, the same words on the device)


def test_from_codes_takes_a_table_and_refuses_a_set_pad_bit():
    from drn_amd import BinaryShortlister, _lib
    emb, q17 = table_and_queries(300, 40, torch.bfloat16, seed=5)
    sl = BinaryShortlister(emb, names=["v%d" % v for v in range(300)])
    again = BinaryShortlister.from_codes(sl.codes.clone(), 40, torch.bfloat16, names=sl.names)
    same_lists(again.shortlist(q17, 300), sl.shortlist(q17, 300))
    assert again.names == sl.names and again.nbytes == sl.nbytes == 300 * 8
    for bit in (8, 31):
        dirty = sl.codes.clone()
        dirty[299, 1] |= int(np.array([1 << bit], dtype=np.uint32).view(np.int32)[0])
        for kw in ({}, {"offsets": [0, 100, 300]}):
            with pytest.raises(_lib.DrnError, match="the codes have a set bit at or past E = 40"):
                BinaryShortlister.from_codes(dirty, 40, torch.bfloat16, **kw)
    with pytest.raises(_lib.DrnError, match="the embeddings hold values that are not finite"):
        bad = emb.clone()
        bad[7, 3] = float("nan")
        BinaryShortlister(bad)


# -- 5. what a score depends on -----------------------------------------------------------------------------------------------------------

@DTYPES
def test_a_query_row_that_is_not_finite_lists_nothing_and_leaves_the_others_alone(dtype):
    from drn_amd import BinaryShortlister
    for kw in ({}, {"offsets": np.concatenate([[0], np.cumsum([1, 3, 0, 17] * 37)])}):
        emb, q17 = table_and_queries(777, 96, dtype, seed=6)
        sl = BinaryShortlister(emb, **kw)
        oracle = sl.dequantized()
        clean = sl.shortlist(q17, 300)
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
    from drn_amd import BinaryShortlister
    lens = [1, 3, 0, 17] * 75
    off = np.concatenate([[0], np.cumsum(lens)])
    emb, q17 = table_and_queries(int(off[-1]) if ragged else 775, 512, torch.bfloat16, seed=8)
    sl = BinaryShortlister(emb, **({"offsets": off} if ragged else {}))
    full = sl.shortlist(q17, 1024)
    for s in (0, 9, 16):
        alone = sl.shortlist(q17[s:s + 1].contiguous(), 1024)
        for f in full._fields:
            assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]), (s, f)
    # the first K videos as a table of their own == the full table under the mask of the first K
    K = 130
    first = BinaryShortlister(emb[:int(off[K])].contiguous(), offsets=off[:K + 1]) if ragged else BinaryShortlister(emb[:K].contiguous())
    mask = torch.zeros(len(sl), dtype=torch.bool)
    mask[:K] = True
    same_lists(first.shortlist(q17, 1024), sl.shortlist(q17, 1024, allow=packed(mask)), "a prefix")


# -- 6. buffers and graphs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_out_buffers_in_place_and_a_replay_follows_queries_and_mask_written_in_place(ragged):
    """out= inside guard bands: every element written, nothing outside them -- also where the table is shorter than n.  One captured
    graph, replayed with the queries and the mask's words changed in place, equals eager."""
    from drn_amd import BinaryShortlister, binary_signs
    from drn_amd.graph import capture_graph
    off = np.concatenate([[0], np.cumsum([1, 3, 0, 17] * 90)])
    emb, q17 = table_and_queries(int(off[-1]), 96, torch.bfloat16, seed=9)
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
    got = sl.shortlist(q, n, out=out)
    assert all(a is b for a, b in zip(got, out)) and guards_hold()
    same_lists(got, oracle.shortlist_deep(binary_signs(q), n), "every element")
    assert int(got.n.min()) == (n if not ragged else min(n, 270))
    words = packed(per[:5].contiguous())
    qbuf = q.clone()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist(qbuf, n, out=out, allow=words)                             # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sl.shortlist(qbuf, n, out=out, allow=words)
    for queries, mask in ((q2, torch.flip(per[:5], dims=(0, 1)).contiguous()), (q, torch.zeros(5, V, dtype=torch.bool)), (q2, per[:5].contiguous())):
        qbuf.copy_(queries)
        words.copy_(packed(mask))
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_lists(type(got)(*out), oracle.shortlist_deep(binary_signs(queries), n, allow=packed(mask)), "replay == eager on new queries and a new mask")
        assert guards_hold()
    assert int(out[2].max()) > 0


# -- 7. the cascade ----------------------------------------------------------------------------------------------------------------------

def test_evaluate_cascade_takes_a_binary_coarse_table_and_ranks_like_the_cascade_by_hand():
    """coarse: the sign codes of the fine table's rows, depth 300; fine: rerank to 128.  The ranks are the target's place in the
    reranked list, -1 where the coarse stage missed it.  Sentences 0..7 of a batch ARE a table row, their target (its code is at
    distance 0: listed); the others' target is the first video their coarse list lacks."""
    from drn_amd import BinaryShortlister, ShortlistRecall, Shortlister, evaluate_cascade, metrics
    V = 775
    names = ["v%d" % v for v in range(V)]
    emb, q17 = table_and_queries(V, 96, torch.bfloat16, seed=10)
    coarse, fine = BinaryShortlister(emb, names=names), Shortlister(emb, names=names)
    depth, topks = 300, (1, 10, 128)
    batches = []
    for S_ in (17, 11):
        q = q17[:S_].clone()
        targets = [10 + 3 * s + S_ for s in range(8)]
        q[:8] = emb[targets]
        lists = coarse.shortlist_deep(q, depth).ids.cpu().tolist()
        targets += [min(set(range(V)) - set(lists[s])) for s in range(8, S_)]
        batches.append(([names[t] for t in targets], q, q))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = evaluate_cascade(coarse, fine, iter(batches), depth, topks=topks, deep=True)
    assert isinstance(got, ShortlistRecall) and got.n == 28
    want = []
    for bnames, cq, fq in batches:
        listed = coarse.shortlist_deep(cq, depth)
        assert bool((listed.n == depth).all())
        reranked = fine.rerank(listed.ids, fq, n=128).ids.cpu()
        for s, name in enumerate(bnames):
            place = (reranked[s] == names.index(name)).nonzero()
            want.append(int(place[0, 0]) if len(place) else -1)
    want = np.asarray(want, dtype=np.int32)
    assert got.ranks.dtype == np.int32 and np.array_equal(got.ranks, want)
    assert (want >= 0).any() and (want < 0).any()
    assert got.recall == metrics.recall_from_ranks(want, list(topks))
