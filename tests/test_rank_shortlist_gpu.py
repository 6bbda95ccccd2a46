"""The rank of a target video in the full shortlist order on the device: drn_shortlist_rank / _segments_rank / _late_rank
(Shortlister.rank, rank_late) against the float64 definitions on exact data with planted ties, against the lists the shortlist kernels
give, against an integer count over the kernels' own scores on random data, under allow masks, on block-scaled FP8 tables, and what an
answer may depend on; out= buffers and a workspace inside guard bands, graph replay with queries, targets and mask overwritten in
place, and evaluate_shortlist.  torch.equal throughout: ranks and totals are integers, scores are compared as bits.
tests/test_rank_shortlist_cpu.py holds the definitions, the refusals, the C boundary and the compiler's notes."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_late_shortlist_gpu import exact_tokens, lengths_of, tokens_for
from test_q8_shortlist_gpu import exact_tables
from test_segment_shortlist_gpu import exact_case, offsets_of
from test_shortlist_gpu import BLOCK, exact_data

pytestmark = pytest.mark.gpu
FIELDS = ("rank", "score", "total")
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def tgt(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=DEV)


def bits(x):
    return (x + 0.0).view(torch.int32)                                       # (-0 + 0 = +0: the kernels' keys fold the two zeros too)


def same_rank(got, want, what=""):
    assert torch.equal(got.rank, want.rank), (what, "rank", got.rank.tolist(), want.rank.tolist())
    assert torch.equal(bits(got.score), bits(want.score)), (what, "score")
    assert torch.equal(got.total, want.total), (what, "total", got.total.tolist(), want.total.tolist())


def plain_targets(V, k):
    """17 targets: the rows tests/test_shortlist_gpu.py exact_data duplicates -- 0 has its twins at higher positions (1, V - 1 and, a
    block away, 256), V - 1 and 256 have theirs at lower ones, 261 / 515 and 774 / 255 are twins in different blocks -- and the values
    that mean "no target"; what is not below V is one of those, too."""
    pool = [0, 1, V - 1, BLOCK, 70, 5, V // 2, V // 3, BLOCK + 5, 2 * BLOCK + 3, 3 * BLOCK + 6, BLOCK - 1, -1, V, INT_MIN, INT_MAX, V + 5]
    return tgt(pool[(s + k) % len(pool)] for s in range(17))


def spread_targets(V, k, S_=17):
    """S_ targets walking over -1 .. V (both ends mean "no target"), a different walk for every k."""
    return tgt((k + 5 * s) % (V + 2) - 1 for s in range(S_))


# -- 1. exact data against the definitions -------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [8, 40, 512])
def test_rank_equals_the_reference_exactly(dtype, E):
    """V: one video, one short of / exactly / one past a 64-video wave tile, one block + 1, three blocks + 7; S = 1 / 16 / 17; targets
    with twins before and after them, in their block and in another, and -1, V, INT_MIN and INT_MAX; a NaN query row."""
    from drn_amd import Shortlister, TargetRank, rank_reference
    for V in (1, 63, 64, 65, BLOCK + 1, 3 * BLOCK + 7):
        emb, q17 = exact_data(V, E, 17, dtype)
        q17 = q17.clone()
        q17[3, E // 2] = float("nan")
        sl = Shortlister(emb)
        for k in (0, 6, 12):
            t17 = plain_targets(V, k)
            want = rank_reference(emb, q17, t17)
            assert int(want.total[3]) == 0 and int(want.rank[3]) == -1 and int(want.total[0]) == V
            for S_ in (1, 16, 17):
                got = sl.rank(q17[:S_].contiguous(), t17[:S_].contiguous())
                assert isinstance(got, TargetRank)
                same_rank(got, TargetRank(*(f[:S_] for f in want)), (V, k, S_))
        if V == 3 * BLOCK + 7:
            # one sentence five times: row 0 and its twins 1 and 256, row 255 and its twin 774 -- a twin's rank counts those before it
            # (and whatever else reaches that score in between)
            r = sl.rank(q17[:1].expand(5, E).contiguous(), tgt([0, 1, BLOCK, BLOCK - 1, V - 1])).rank.tolist()
            assert 0 <= r[0] < r[1] < r[2] and 0 <= r[3] < r[4], r


def test_rank_with_odd_widths_reads_no_vector_past_a_row():
    """E = 1 and 5 (bf16 rows are not 16-byte aligned: the element-wise loader) and E = 36 (aligned rows, a partial last step)."""
    from drn_amd import Shortlister, rank_reference, segment_rank_reference
    for E in (1, 5, 36):
        for dtype in (torch.bfloat16, torch.float32):
            emb, q = exact_data(BLOCK + 9, E, 3, dtype)
            t = tgt([BLOCK + 8, 0, 77])
            same_rank(Shortlister(emb).rank(q, t), rank_reference(emb, q, t), (E, dtype))
            off = offsets_of([3, 0, 1] * 66 + [BLOCK + 9 - 4 * 66])
            t = tgt([198, 1, 0])
            same_rank(Shortlister(emb, offsets=off).rank(q, t), segment_rank_reference(emb, off, q, t), (E, dtype, "ragged"))


@DTYPES
@pytest.mark.parametrize("E", [8, 40, 512])
def test_segment_rank_equals_the_reference_exactly(dtype, E):
    """Runs cycling 1 / 3 / 0 / 17 (rowless targets among them), the 300- and the 600-row video with the best row planted in the first
    and in the last pass, a block edge inside a video, 257 one-row videos and R = V = 1."""
    from drn_amd import Shortlister, TargetRank, segment_rank_reference
    for layout in ("cycle", "long", "straddle", "ones257", "one"):
        emb, q17, off = exact_case(layout, E, dtype)
        V = len(off) - 1
        sl = Shortlister(emb, offsets=off)
        sets = [spread_targets(V, k) for k in range(0, V + 2, max(1, (V + 2) // 6))]
        if layout == "long":
            sets += [tgt([v] * 17) for v in range(V)]                        # every video for every sentence, 1 and 4 (the long ones) too
            best = segment_rank_reference(emb, off, q17, [4] * 17)
            assert int(best.rank[0]) == 1 and int(segment_rank_reference(emb, off, q17, [1] * 17).rank[0]) == 0   # (a tie: by position)
        if layout == "cycle":
            sets.append(tgt([2, 6, 10] * 5 + [0, 3]))                        # videos without rows
        for i, t17 in enumerate(sets):
            want = segment_rank_reference(emb, off, q17, t17)
            for S_ in ((17, 1) if i % 3 == 0 else (17,)):
                same_rank(sl.rank(q17[:S_].contiguous(), t17[:S_].contiguous()), TargetRank(*(f[:S_] for f in want)), (layout, i, S_))
        if layout == "cycle":
            assert want.rank.tolist()[:3] == [-1] * 3 and int(want.total[0]) == 90


@DTYPES
@pytest.mark.parametrize("E", [8, 512])
def test_late_rank_equals_the_reference_exactly(dtype, E):
    """L = 1 / 5 / 16 / 17 / 33 / 64 with lengths mixing 0, 1, 16, 17 and L (and values the device clamps), over the same layouts."""
    from drn_amd import Shortlister, TargetRank, late_rank_reference
    for layout in ("cycle", "long", "ones257", "one"):
        emb, tok, off = tokens_for(layout, E, dtype)
        V = len(off) - 1
        sl = Shortlister(emb, offsets=off)
        for L in (1, 5, 16, 17, 33, 64):
            q, lengths = tok[:, :L].contiguous(), lengths_of(L)
            for k in ((0, 3) if layout != "one" else (0, 1, 2)):
                t17 = spread_targets(V, 7 * k + L) if layout != "long" else tgt([(s + k + L) % (V + 1) for s in range(17)])
                want = late_rank_reference(emb, off, q, lengths, t17)
                assert int(want.total[1]) == 0 and int(want.rank[1]) == -1   # (lengths[1] = 0)
                for S_ in ((17, 3) if k == 0 else (17,)):
                    got = sl.rank_late(q[:S_].contiguous(), lengths[:S_].contiguous(), t17[:S_].contiguous())
                    same_rank(got, TargetRank(*(f[:S_] for f in want)), (layout, L, k, S_))


@DTYPES
def test_equal_sums_from_different_token_splits_rank_by_position(dtype):
    """The table of tests/test_late_shortlist_gpu.py: videos 1, 2 and 4 reach 8 by different splits, 6 is ahead with 16."""
    from drn_amd import Shortlister, late_rank_reference
    E = 8
    rows = {1: [[3, 0], [0, 5]], 2: [[4, 4]], 4: [[5, 0], [0, 3]], 5: [[1, 1]], 6: [[8, 0], [0, 8], [-8, -8]], 7: [[2, 5]]}
    lens = [len(rows.get(v, [])) for v in range(9)]
    emb = torch.zeros(sum(lens), E)
    emb[:, :2] = torch.tensor([r for v in sorted(rows) for r in rows[v]], dtype=torch.float32)
    q = torch.zeros(9, 3, E)
    q[:, 0, 0] = q[:, 1, 1] = 1
    lengths = torch.tensor([2] * 8 + [3], dtype=torch.int32, device=DEV)
    emb, q, off = emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous(), offsets_of(lens)
    t = tgt(range(9))
    want = late_rank_reference(emb, off, q, lengths, t)
    assert want.rank.tolist() == [-1, 1, 2, -1, 3, 5, 0, 4, -1] and want.score.tolist() == [0., 8., 8., 0., 8., 2., 16., 7., 0.]
    same_rank(Shortlister(emb, offsets=off).rank_late(q, lengths, t), want)


@DTYPES
def test_one_token_per_sentence_is_rank(dtype):
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    g = torch.Generator().manual_seed(19)
    emb = torch.randn(int(sum(lens)), 200, generator=g).to(DEV, dtype).contiguous()
    tok = torch.randn(17, 7, 200, generator=g).to(DEV, dtype).contiguous()
    sl = Shortlister(emb, offsets=offsets_of(lens))
    ones = torch.ones(17, dtype=torch.int32, device=DEV)
    for k in (0, 9, 40):
        t = spread_targets(len(lens), k)
        a = sl.rank(tok[:, 0].contiguous(), t)
        same_rank(sl.rank_late(tok[:, :1].contiguous(), ones, t), a, k)
        same_rank(sl.rank_late(tok, ones, t), a, (k, "padded"))              # ... and with the token first among padding
    assert int(a.total[0]) == sum(1 for x in lens if x) and int((a.rank >= 0).sum()) > 8


# -- 2. agreement with the lists ---------------------------------------------------------------------------------------------------------

def agrees_with_list(r, short, targets, n):
    """rank < n: the list holds the target at that place with the score's bits; otherwise the target is not in the list."""
    ranks, ids, t = r.rank.tolist(), short.ids.tolist(), targets.tolist()
    mine, theirs = bits(r.score).tolist(), bits(short.scores).tolist()
    hit = 0
    for s, k in enumerate(ranks):
        if 0 <= k < n:
            assert ids[s][k] == t[s] and mine[s] == theirs[s][k], (s, k, n)
            hit += 1
        else:
            assert t[s] < 0 or t[s] not in ids[s], (s, k, n)             # (a list's padding is -1, which names no video)
    return hit


@functools.lru_cache(maxsize=None)
def random_case(R, E, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(R, E, generator=g).to(DEV, dtype).contiguous()
    tok = torch.randn(17, 17, E, generator=g).to(DEV, dtype).contiguous()
    return emb, tok


@DTYPES
def test_rank_agrees_with_the_lists_of_the_shortlist_kernels(dtype):
    """n = 1 / 5 / 128 on random data, the three rankings: targets taken from assorted places of the n = 128 list, from past it and from
    outside the table."""
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 70 + [300, 2]                                     # V = 282, R = 1772
    emb, tok = random_case(int(sum(lens)), 96, dtype, 5)
    lengths = lengths_of(17)
    places = [0, 1, 4, 5, 127, 126, 0, 3, 64, 2, 0, 1, 4, 5, 100, 0, 77]
    for kind in ("plain", "ragged", "late"):
        sl = Shortlister(emb) if kind == "plain" else Shortlister(emb, offsets=offsets_of(lens))
        q = tok if kind == "late" else tok[:, 0].contiguous()
        lists = {n: sl.shortlist_late(q, lengths, n) if kind == "late" else sl.shortlist(q, n) for n in (1, 5, 128)}
        full = lists[128].ids.tolist()
        inside = tgt(full[s][places[s]] for s in range(17))                  # (-1 where the sentence lists nothing: lengths 0)
        hits = 0
        for targets in (inside, spread_targets(len(sl), 3), spread_targets(len(sl), 50)):
            r = sl.rank_late(q, lengths, targets) if kind == "late" else sl.rank(q, targets)
            for n in (1, 5, 128):
                hits += agrees_with_list(r, lists[n], targets, n)
        assert hits >= 20, (kind, hits)


@DTYPES
def test_every_video_of_a_small_table_ranks_where_the_full_list_has_it(dtype):
    """At most 128 candidates: every video in turn as the target of all 17 sentences.  Its rank is its index in the n = 128 list (-1 when
    it is not there), and total == Shortlist.n."""
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 25                                                # V = 100, 75 owners
    emb, tok = random_case(int(sum(lens)), 96, dtype, 6)
    emb = emb.clone()
    emb[21:25] = emb[0]                                                      # equal scores, certain
    lengths = lengths_of(17)
    for kind in ("plain", "ragged", "late"):
        sl = Shortlister(emb[:100].contiguous()) if kind == "plain" else Shortlister(emb, offsets=offsets_of(lens))
        q = tok if kind == "late" else tok[:, 0].contiguous()
        short = sl.shortlist_late(q, lengths, 128) if kind == "late" else sl.shortlist(q, 128)
        for v in range(100):
            t = tgt([v] * 17)
            r = sl.rank_late(q, lengths, t) if kind == "late" else sl.rank(q, t)
            at = short.ids == v
            want = torch.where(at.any(dim=1), at.int().argmax(dim=1).to(torch.int32), torch.full((17,), -1, dtype=torch.int32, device=DEV))
            assert torch.equal(r.rank, want) and torch.equal(r.total, short.n), (kind, v)
            listed = torch.where(at, short.scores, torch.zeros_like(short.scores)).sum(dim=1)
            assert torch.equal(bits(r.score), bits(listed)), (kind, v)


def test_rank_on_random_bf16_data_is_the_integer_count_over_the_kernels_own_scores():
    """V = 775, E = 512, random bf16: no float64 comparison (near-ties may legitimately flip).  The kernel's own (S, V) score matrix is
    rebuilt from shortlists of 128-row slices (a slice keeps the bits), and rank is the count of the videos ahead under the key order."""
    from drn_amd import Shortlister
    V, E = 3 * BLOCK + 7, 512
    emb, tok = random_case(V, E, torch.bfloat16, 7)
    emb = emb.clone()
    emb[300], emb[700], emb[11] = emb[10], emb[10], emb[10]                   # twins of row 10 before and after block edges
    q = tok[:, 0].contiguous()
    dense = torch.empty((17, V), dtype=torch.float32, device=DEV)
    for a in range(0, V, 128):
        part = Shortlister(emb[a:a + 128].contiguous()).shortlist(q, 128)
        assert int(part.n.min()) == min(128, V - a)
        dense[:, a:a + 128].scatter_(1, part.ids[:, :min(128, V - a)].long(), part.scores[:, :min(128, V - a)])
    sl = Shortlister(emb)
    where = torch.arange(V, device=DEV)[None, :]
    for targets in (tgt([10, 11, 300, 700] * 4 + [774]), spread_targets(V, 123), spread_targets(V, 400)):
        got = sl.rank(q, targets)
        tc = targets.clamp(0, V - 1).long()[:, None]
        ts = torch.gather(dense, 1, tc)
        count = ((dense > ts) | ((dense == ts) & (where < tc))).sum(dim=1).to(torch.int32)
        ok = (targets >= 0) & (targets < V)
        assert torch.equal(got.rank, torch.where(ok, count, torch.full_like(count, -1)))
        assert torch.equal(bits(got.score), bits(torch.where(ok, ts[:, 0], torch.zeros_like(ts[:, 0]))))
        assert got.total.tolist() == [V] * 17
    r = sl.rank(q[:4].contiguous(), tgt([10, 11, 300, 700])).rank
    again = sl.rank(q[:1].expand(4, E).contiguous(), tgt([10, 11, 300, 700])).rank.tolist()
    assert 0 <= again[0] < again[1] < again[2] < again[3] and int(r[0]) >= 0      # (the twins of row 10, in position order)


# -- 3. masks ----------------------------------------------------------------------------------------------------------------------------

def test_masks_all_ones_dark_blocks_a_sub_table_and_bits_past_the_table():
    from drn_amd import Shortlister, pack_allow
    lens = [1, 3, 0, 17] * 190 + [300, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]   # V = 775
    V = len(lens)
    assert V == 3 * BLOCK + 7
    emb, tok = random_case(int(sum(lens)), 96, torch.bfloat16, 41)
    lengths = lengths_of(17)
    g = torch.Generator().manual_seed(3)
    for kind in ("plain", "ragged", "late"):
        sl = Shortlister(emb[:V].contiguous()) if kind == "plain" else Shortlister(emb, offsets=offsets_of(lens))
        q = tok if kind == "late" else tok[:, 0].contiguous()
        rank = (lambda t, **kw: sl.rank_late(q, lengths, t, **kw)) if kind == "late" else (lambda t, **kw: sl.rank(q, t, **kw))
        targets = tgt((47 * s + 30) % (V + 2) - 1 for s in range(17))         # 29, 76, ... 734, 4: some inside the block masked below
        full = rank(targets)
        ones = pack_allow(torch.ones(V, dtype=torch.bool, device=DEV))
        same_rank(rank(targets, allow=ones), full, (kind, "all ones, shared"))
        same_rank(rank(targets, allow=ones.repeat(17, 1).contiguous()), full, (kind, "all ones, per sentence"))
        stuffed = ones.clone()
        stuffed[-1] = -1                                                     # (V = 775: the last word's bits 7 .. 31 lie past the table)
        assert int(stuffed[-1]) != int(ones[-1])
        same_rank(rank(targets, allow=stuffed), full, (kind, "bits at or past V"))
        # the masked rank over `keep` == the unmasked rank on the table of those videos alone; a target outside keep gives -1
        keep = torch.sort(torch.randperm(V, generator=g)[:300]).values
        keep = torch.unique(torch.cat([keep, torch.tensor([V - 15]), targets[:6].cpu().clamp(0, V - 1).long()]))
        mask = torch.zeros(V, dtype=torch.bool)
        mask[keep] = True
        if kind == "plain":
            sub = Shortlister(emb[keep.to(DEV)].contiguous())
        else:
            off = offsets_of(lens)
            rows = torch.cat([torch.arange(int(off[v]), int(off[v + 1])) for v in keep.tolist()])
            sub = Shortlister(emb[rows.to(DEV)].contiguous(), offsets=offsets_of([lens[v] for v in keep.tolist()]))
        at = torch.searchsorted(keep, targets.cpu().long().clamp(0, V - 1))
        inside = (targets.cpu() >= 0) & (targets.cpu() < V) & mask[targets.cpu().long().clamp(0, V - 1)]
        mapped = tgt(torch.where(inside, at, torch.full_like(at, -1)).tolist())
        want = sub.rank_late(q, lengths, mapped) if kind == "late" else sub.rank(q, mapped)
        got = rank(targets, allow=pack_allow(mask.to(DEV)))
        same_rank(got, want, (kind, "sub-table"))
        assert int((got.rank >= 0).sum()) >= 3 and int((got.rank[~inside.to(DEV)] == -1).all())
        # dark blocks: the videos of one whole block (plain) or of several (ragged) masked for everyone, and others for one sentence alone
        dark = torch.ones(17, V, dtype=torch.bool)
        dark[:, BLOCK:2 * BLOCK] = False
        dark[5, :2 * BLOCK + 100] = False
        dark[7] = False
        got = rank(targets, allow=pack_allow(dark.to(DEV)))
        sub_mask = torch.ones(V, dtype=torch.bool)
        sub_mask[BLOCK:2 * BLOCK] = False
        shared = rank(targets, allow=pack_allow(sub_mask.to(DEV)))
        others = [s for s in range(17) if s not in (5, 7)]
        for f in FIELDS:
            assert torch.equal(getattr(got, f)[others], getattr(shared, f)[others]), (kind, f)
        assert int(got.total[7]) == 0 and int(got.rank[7]) == -1 and float(got.score[7]) == 0.0
        t = targets.cpu()
        hidden = (t >= BLOCK) & (t < 2 * BLOCK)
        assert bool(hidden.any()) and bool((shared.rank.cpu()[hidden] == -1).all())
        if kind == "plain":
            assert shared.total.tolist() == [V - BLOCK] * 17 and int(got.total[5]) == V - 2 * BLOCK - 100


@DTYPES
def test_shared_and_per_sentence_masks_equal_the_references_on_exact_data(dtype):
    from drn_amd import Shortlister, late_rank_reference, pack_allow, rank_reference, segment_rank_reference
    V = 3 * BLOCK + 7
    emb, q17 = exact_data(V, 40, 17, dtype)
    g = torch.Generator().manual_seed(V)
    sl = Shortlister(emb)
    for shape in ((V,), (17, V)):
        mask = (torch.rand(shape, generator=g) < 0.4).to(DEV)
        for k in (0, 6):
            t = plain_targets(V, k)
            same_rank(sl.rank(q17, t, allow=pack_allow(mask)), rank_reference(emb, q17, t, allow=mask), ("plain", shape, k))
    for layout in ("cycle", "long", "ones257"):
        emb, tok, off = tokens_for(layout, 40, dtype)
        V = len(off) - 1
        sl = Shortlister(emb, offsets=off)
        q3, lengths = tok[:, :17].contiguous(), lengths_of(17)
        q = tok[:, 0].contiguous()
        for shape in ((V,), (17, V)):
            mask = (torch.rand(shape, generator=g) < 0.4).to(DEV)
            for k in (1, V // 2):
                t = spread_targets(V, k)
                same_rank(sl.rank(q, t, allow=pack_allow(mask)), segment_rank_reference(emb, off, q, t, allow=mask), (layout, shape, k))
                same_rank(sl.rank_late(q3, lengths, t, allow=pack_allow(mask)), late_rank_reference(emb, off, q3, lengths, t, allow=mask),
                          (layout, shape, k, "late"))


# -- 4. block-scaled FP8 tables --------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantised_ranks_are_the_dequantised_ones_and_the_references(dtype, E):
    """Exact tables (tests/test_q8_shortlist_gpu.py exact_tables says why every partial sum is exact): every field equals
    dequantized().rank() / rank_late() and the float64 definition over the dequantised table, masked and not; a random table, where
    nothing is exact, still equals dequantized() bit for bit."""
    from drn_amd import Shortlister, late_rank_reference, pack_allow, rank_reference, segment_rank_reference
    from drn_amd.index import mx8_dequantize
    codes, scales, q, _ = exact_tables(tuple([1] * (2 * BLOCK + 9)), E)
    V = int(codes.shape[0])
    table, q = mx8_dequantize(codes, scales), q.to(dtype)
    sl = Shortlister.from_mx8(codes, scales, dtype)
    oracle = sl.dequantized()
    mask = torch.arange(V, device=DEV) % 3 != 1
    for k in (0, 100):
        t = spread_targets(V, k)
        got = sl.rank(q, t)
        same_rank(got, oracle.rank(q, t), (k, "dequantized"))
        same_rank(got, rank_reference(table, q, t), (k, "reference"))
        same_rank(sl.rank(q, t, allow=pack_allow(mask)), rank_reference(table, q, t, allow=mask), (k, "masked"))
    for lens in ([1, 3, 0, 17] * 30, [2, 300, 1, 0, 4], [1] * 257):
        codes, scales, q, off = exact_tables(tuple(lens), E)
        V = len(lens)
        table, q = mx8_dequantize(codes, scales), q.to(dtype)
        sl = Shortlister.from_mx8(codes, scales, dtype, offsets=off)
        oracle = sl.dequantized()
        mask = torch.arange(V, device=DEV) % 3 != 1
        tok, lengths = exact_tokens(E, dtype)[:, :16].contiguous(), lengths_of(16)
        for k in (0, 3):
            t = spread_targets(V, k)
            got = sl.rank(q, t)
            same_rank(got, oracle.rank(q, t), (len(lens), k, "dequantized"))
            same_rank(got, segment_rank_reference(table, off, q, t), (len(lens), k, "reference"))
            same_rank(sl.rank(q, t, allow=pack_allow(mask)), segment_rank_reference(table, off, q, t, allow=mask), (len(lens), k, "masked"))
            got = sl.rank_late(tok, lengths, t)
            same_rank(got, oracle.rank_late(tok, lengths, t), (len(lens), k, "late, dequantized"))
            same_rank(got, late_rank_reference(table, off, tok, lengths, t), (len(lens), k, "late, reference"))
            same_rank(sl.rank_late(tok, lengths, t, allow=pack_allow(mask)), late_rank_reference(table, off, tok, lengths, t, allow=mask),
                      (len(lens), k, "late, masked"))
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    g = torch.Generator().manual_seed(E)
    R = int(sum(lens))
    emb = (torch.randn(R, E, generator=g)
           * torch.exp2(torch.randint(-3, 4, (R, E // 32), generator=g).float()).repeat_interleave(32, dim=1)).to(DEV, dtype).contiguous()
    tok = torch.randn(17, 33, E, generator=g).to(DEV, dtype).contiguous()
    t = spread_targets(len(lens), 11)
    ragged = Shortlister(emb, offsets=offsets_of(lens), quantize="mxfp8")
    same_rank(ragged.rank_late(tok, lengths_of(33), t), ragged.dequantized().rank_late(tok, lengths_of(33), t), "random, late")
    same_rank(ragged.rank(tok[:, 0].contiguous(), t), ragged.dequantized().rank(tok[:, 0].contiguous(), t), "random, ragged")
    plain = Shortlister(emb, quantize="mxfp8")
    t = spread_targets(R, 200)
    same_rank(plain.rank(tok[:, 0].contiguous(), t), plain.dequantized().rank(tok[:, 0].contiguous(), t), "random, plain")


# -- 5. what an answer depends on ------------------------------------------------------------------------------------------------------------

def test_an_answer_depends_on_its_sentence_its_target_and_the_table_alone():
    """A sentence alone and among 17; the other sentences' targets changed; a longer table whose extra videos all score lower: rank and
    score unchanged, total larger by their number."""
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 60 + [300, 2]                                     # V = 242
    V, off = len(lens), offsets_of(lens)
    emb, tok = random_case(int(sum(lens)), 200, torch.bfloat16, 33)
    lengths = lengths_of(17)
    for kind in ("plain", "ragged", "late"):
        sl = Shortlister(emb[:V].contiguous()) if kind == "plain" else Shortlister(emb, offsets=off)
        q = tok if kind == "late" else tok[:, 0].contiguous()
        rank = (lambda q_, l_, t_, on=sl: on.rank_late(q_, l_, t_)) if kind == "late" else (lambda q_, l_, t_, on=sl: on.rank(q_, t_))
        targets = tgt([(37 * s + 5) % V for s in range(17)])
        full = rank(q, lengths, targets)
        assert int((full.rank >= 0).sum()) >= 8
        for s in (0, 3, 5, 16):
            alone = rank(q[s:s + 1].contiguous(), lengths[s:s + 1].contiguous(), targets[s:s + 1].contiguous())
            other = spread_targets(V, 11 * s)
            other[s] = targets[s]
            among = rank(q, lengths, other)
            for f in FIELDS:
                assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]) and torch.equal(getattr(among, f)[s], getattr(full, f)[s]), (kind, s, f)
    # exact data, one sentence at a time: 20 more videos (a block edge among them) that hold the lowest score there is
    emb, q17 = exact_data(250, 40, 17, torch.bfloat16)
    for s in (0, 8):
        q = q17[s:s + 1].contiguous()
        low = (-4 * torch.sign(q.float())).to(torch.bfloat16).expand(20, 40)
        longer = torch.cat([emb, low]).contiguous()
        for t in (0, 100, 249):
            a, b = Shortlister(emb).rank(q, tgt([t])), Shortlister(longer).rank(q, tgt([t]))
            assert torch.equal(a.rank, b.rank) and torch.equal(bits(a.score), bits(b.score)) and int(b.total) == int(a.total) + 20 == 270
        lens_a, lens_b = [2] * 125, [2] * 125 + [2] * 10
        a = Shortlister(emb, offsets=offsets_of(lens_a)).rank(q, tgt([60]))
        b = Shortlister(longer, offsets=offsets_of(lens_b)).rank(q, tgt([60]))
        assert torch.equal(a.rank, b.rank) and torch.equal(bits(a.score), bits(b.score)) and int(b.total) == int(a.total) + 10 == 135
        one = torch.ones(1, dtype=torch.int32, device=DEV)
        a = Shortlister(emb, offsets=offsets_of(lens_a)).rank_late(q[:, None].contiguous(), one, tgt([60]))
        b = Shortlister(longer, offsets=offsets_of(lens_b)).rank_late(q[:, None].contiguous(), one, tgt([60]))
        assert torch.equal(a.rank, b.rank) and torch.equal(bits(a.score), bits(b.score)) and int(b.total) == int(a.total) + 10 == 135


# -- 6. buffers, graphs ------------------------------------------------------------------------------------------------------------------------

def armed():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")


@pytest.mark.parametrize("kind", ["plain", "ragged", "late", "mxfp8"])
def test_out_buffers_and_the_workspace_stay_inside_their_guards_and_a_captured_call_replays(kind):
    """out= written in place; guard bands around the three outputs AND the workspace untouched; a captured call replays after queries,
    targets, lengths and the mask were overwritten in place; eager calls and the replay run with torch's synchronisation check armed."""
    from drn_amd import Shortlister, TargetRank, late_rank_reference, ops, pack_allow, rank_reference, segment_rank_reference
    from drn_amd.graph import capture_graph
    from drn_amd.index import mx8_dequantize
    S_, L, GUARD = 5, 17, 64
    if kind == "mxfp8":
        codes, scales, q17, _ = exact_tables(tuple([1] * (2 * BLOCK + 9)), 96)
        emb, off = mx8_dequantize(codes, scales), None
        sl, V = Shortlister.from_mx8(codes, scales, torch.bfloat16), int(codes.shape[0])
        tok = q17.to(torch.bfloat16)[:, None].contiguous()
    elif kind == "plain":
        emb, q17 = exact_data(2 * BLOCK + 9, 40, 17, torch.bfloat16)
        sl, V, off, tok = Shortlister(emb), int(emb.shape[0]), None, q17[:, None].contiguous()
    else:
        emb, tok, off = tokens_for("cycle", 40, torch.bfloat16)
        sl, V = Shortlister(emb, offsets=off), len(off) - 1
    late = kind == "late"
    q, q2 = (tok[:S_, :L].contiguous(), tok[5:5 + S_, 3:3 + L].contiguous()) if late else (tok[:S_, 0].contiguous(), tok[5:5 + S_, 0].contiguous())
    lengths, lengths2 = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in ([17, 0, 1, 16, 5], [2, 17, 30, 0, 16]))
    t1, t2 = tgt([0, V - 1, 7, -1, V // 2]), tgt([V, 3, 1, 4, V - 2])
    g = torch.Generator().manual_seed(8)
    mask, mask2 = ((torch.rand((S_, V), generator=g) < p).to(DEV) for p in (0.5, 0.8))

    def reference(queries, lens_, targets, m):
        if late:
            return late_rank_reference(emb, off, queries, lens_, targets, allow=m)
        if off is not None:
            return segment_rank_reference(emb, off, queries, targets, allow=m)
        return rank_reference(emb, queries, targets, allow=m)

    def run(queries, lens_, targets, **kw):
        return sl.rank_late(queries, lens_, targets, **kw) if late else sl.rank(queries, targets, **kw)
    dtypes = (torch.int32, torch.float32, torch.int32)
    flat = [torch.full((S_ + 2 * GUARD,), 77, dtype=dt, device=DEV) for dt in dtypes]
    out = TargetRank(*(f[GUARD:GUARD + S_] for f in flat))
    nblocks = -(-V // BLOCK) if off is None else len(sl.plan.blk_vid) - 1
    words8 = ops.shortlist_rank_ws_bytes(nblocks, S_) // 8
    wsflat = torch.full((words8 + 2 * GUARD,), 77, dtype=torch.int64, device=DEV)
    key = ("rank_late", S_) if late else ("rank", S_)
    sl._ws[key] = wsflat[GUARD:GUARD + words8]

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat + [wsflat])
    qbuf, lbuf, tbuf, words = q.clone(), lengths.clone(), t1.clone(), pack_allow(mask)
    armed()
    try:
        got = run(qbuf, lbuf, tbuf, out=out, allow=words)
        bare = run(qbuf, lbuf, tbuf)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(a is b for a, b in zip(got, out)) and guards_hold() and sl._ws[key].data_ptr() == wsflat[GUARD:].data_ptr()
    assert bool((wsflat[GUARD:GUARD + words8] != 77).all())                   # (every word of the workspace is written)
    same_rank(out, reference(q, lengths, t1, mask), "every element")
    same_rank(bare, reference(q, lengths, t1, None), "no mask")
    # capture on one stream, then replay on other queries, lengths, targets and mask written into the captured buffers
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(qbuf, lbuf, tbuf, out=out, allow=words)                          # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        run(qbuf, lbuf, tbuf, out=out, allow=words)
    for queries, lens_, targets, m in ((q2, lengths2, t2, mask2), (q, lengths, t1, mask)):
        qbuf.copy_(queries), lbuf.copy_(lens_), tbuf.copy_(targets), pack_allow(m, out=words)
        for t in out:
            t.fill_(77)
        armed()
        try:
            graph.replay()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        same_rank(out, reference(queries, lens_, targets, m), "replay == reference")
    assert guards_hold()


# -- 7. recall -------------------------------------------------------------------------------------------------------------------------------

def test_evaluate_shortlist_is_recall_from_ranks_of_the_batches_ranks():
    from drn_amd import ShortlistRecall, Shortlister, _lib, evaluate_shortlist, metrics, ops
    V = 3 * BLOCK + 7
    emb, tok = random_case(V, 96, torch.bfloat16, 51)
    names = ["v%04d" % v for v in range(V)]
    sl = Shortlister(emb, names=names)
    q = (emb[torch.arange(17, device=DEV) * 40].float() + 2.0 * tok[:, 0].float()).to(torch.bfloat16).contiguous()   # a target's row plus noise
    ta, tb = [40 * s for s in range(9)], [40 * s for s in range(9, 17)]
    batches = [([names[v] for v in ta], q[:9].contiguous()), ([names[v] for v in tb], q[9:].contiguous())]
    qa, qb, dev_a, dev_b = q[:9].contiguous(), q[9:].contiguous(), tgt(ta), tgt(tb)
    ops.kernel_timer = []
    armed()
    try:
        ranks = [sl.rank(qa, dev_a).rank, sl.rank(qb, dev_b).rank]
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    assert tags == ["shortlist_rank"] * 2                                    # (one tagged entry a call)
    mine = torch.cat(ranks).cpu().numpy()
    got = evaluate_shortlist(sl, batches)
    assert isinstance(got, ShortlistRecall) and got.n == 17 and got.topks == [1, 10, 100, 1000]
    assert got.ranks.dtype == np.int32 and got.ranks.tolist() == mine.tolist() and bool((mine >= 0).all())
    assert got.recall == metrics.recall_from_ranks(mine, (1, 10, 100, 1000)) and got.recall[-1] == 1.0
    assert got.mrr == metrics.mrr_from_ranks(mine) and got.median_rank == metrics.median_rank_from_ranks(mine)
    # a shared mask reaches every batch: without the targets' own videos nothing is found
    none = evaluate_shortlist(sl, batches, topks=(5,), allow=sl.allow_of(drop=ta + tb))
    assert none.ranks.tolist() == [-1] * 17 and none.recall == [0.0] and none.mrr == 0.0 and none.median_rank == float("inf")
    # an unknown name raises before anything of its batch is launched
    ops.kernel_timer = []
    try:
        with pytest.raises(_lib.DrnError, match="no video named nobody"):
            evaluate_shortlist(sl, [(["v0001", "nobody"], q[:2].contiguous())])
        assert ops.kernel_timer == []
    finally:
        ops.kernel_timer = None
    # late=True goes through rank_late
    lens = [1, 3, 0, 17] * 25
    emb2, tok2 = random_case(int(sum(lens)), 96, torch.bfloat16, 6)
    rag = Shortlister(emb2, names=["w%d" % v for v in range(100)], offsets=offsets_of(lens))
    lengths = lengths_of(17)
    want = rag.rank_late(tok2, lengths, tgt(range(17))).rank.tolist()
    late = evaluate_shortlist(rag, [(["w%d" % v for v in range(17)], tok2, lengths)], topks=(1, 50), late=True)
    assert late.ranks.tolist() == want and late.recall == metrics.recall_from_ranks(want, (1, 50))
