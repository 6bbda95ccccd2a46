"""The shortlist by late interaction on the device: drn_shortlist_late_topn (Shortlister.shortlist_late) against
late_shortlist_reference on exact data with planted ties (torch.equal on ids, scores and n), its links to the shipped kernels (one token
per sentence is shortlist(); the sums are fp32 sums of shortlist()'s scores), what a score may depend on, allow masks, block-scaled FP8
tables, random bf16 data against a derived bound, out= buffers and a workspace inside guard bands, graph replay with queries, lengths and
mask overwritten in place, and its ids as Grounder.search's device candidates.
tests/test_late_shortlist_cpu.py holds the definition, the refusals, the C boundary and the compiler's notes."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_q8_shortlist_gpu import exact_tables
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import exact_case, offsets_of
from test_shortlist_gpu import world

pytestmark = pytest.mark.gpu
FIELDS = ("ids", "scores", "n")
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
# the live tokens of 17 sentences, where L stands for "all of them": 0, 1, 16, 17 and L inside one call, a tile boundary on either side,
# values past L (and L itself, where it is smaller) that the device clamps, and a negative one
LENGTHS = ["L", 0, 1, 16, 17, "L", 5, 33, 64, 70, -2, 2, 15, 32, 31, 48, "L"]


def lengths_of(L, S_=17):
    return torch.tensor([L if x == "L" else x for x in LENGTHS[:S_]], dtype=torch.int32, device=DEV)


def same_lists(got, want, what=""):
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


def head(short, S_, n):
    """The first S_ sentences of a list cut to n: what the definition gives for them (a shorter cut is a prefix)."""
    from drn_amd import Shortlist
    return Shortlist(short.ids[:S_, :n].contiguous(), short.scores[:S_, :n].contiguous(), short.n[:S_].clamp(max=n))


def dense(short, V):
    """A complete list (n >= the videos listed) -> (S, V) float32, NaN where a video is not listed."""
    out = torch.full((short.ids.shape[0], V + 1), float("nan"), dtype=torch.float32, device=short.ids.device)
    at = torch.where(short.ids >= 0, short.ids.long(), torch.full_like(short.ids, V).long())
    return out.scatter_(1, at, short.scores)[:, :V]


@functools.lru_cache(maxsize=None)
def exact_tokens(E, dtype, seed=0):
    """(17, 64, E) integer tokens in [-4, 4]: with integer rows in [-4, 4] a dot product is an integer of magnitude at most 16 E <= 2^13
    and a sum of 64 of them stays below 2^19 -- L |dot| < 2^24, every partial sum exact in fp32 in any order.  Shared, changed by no
    test."""
    g = torch.Generator().manual_seed(77 + seed + E)
    return torch.randint(-4, 5, (17, 64, E), generator=g).float().to(DEV, dtype).contiguous()


def tokens_for(layout, E, dtype):
    """exact_tokens with exact_case's queries as every sentence's first token, so that what that case plants for its queries (in "long":
    the best row for sentence 0, in the first and again in the last pass of each long video) is planted for token 0."""
    emb, q17, off = exact_case(layout, E, dtype)
    tok = exact_tokens(E, dtype).clone()
    tok[:, 0] = q17
    return emb, tok, off


# -- 1. exact data -------------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [8, 40, 512])
def test_late_shortlist_equals_the_reference_exactly(dtype, E):
    """Runs cycling 1 / 3 / 0 / 17, a 300- and a 600-row video, 257 one-row videos and R = V = 1, at L = 1 / 5 / 16 / 17 / 33 / 64 with
    lengths mixing 0, 1, 16, 17 and L, S = 1 / 3 / 17 and n = 1 / 5 / 128: ids, scores and n equal to the float64 definition."""
    from drn_amd import Shortlist, Shortlister, late_shortlist_reference
    for layout in ("cycle", "long", "ones257", "one"):
        emb, tok, off = tokens_for(layout, E, dtype)
        sl = Shortlister(emb, offsets=off)
        if layout == "long":
            # token 0 of sentence 0 finds its best possible row in the first and again in the last pass of videos 1 and 4
            assert set(late_shortlist_reference(emb, off, tok[:1, :1].contiguous(), [1], 2).ids[0].tolist()) == {1, 4}
        for L in (1, 5, 16, 17, 33, 64):
            q, lengths = tok[:, :L].contiguous(), lengths_of(L)
            want = late_shortlist_reference(emb, off, q, lengths, 128)
            assert int(want.n[1]) == 0 and int(want.n[10]) == 0 and int(want.n[0]) > 0
            for S_, n in ((17, 128), (17, 1), (3, 5), (1, 1), (1, 128)):
                got = sl.shortlist_late(q[:S_].contiguous(), lengths[:S_].contiguous(), n)
                assert isinstance(got, Shortlist)
                same_lists(got, head(want, S_, n), (layout, L, S_, n))


@DTYPES
def test_equal_sums_from_different_token_splits_go_by_position(dtype):
    """Tokens along the axes; video 1 reaches 8 as 3 + 5 in two rows, video 2 as 4 + 4 in one, video 4 as 5 + 3; video 6 is ahead of
    them with 8 + 8 and the others stay below; a third token of zeros adds 0 to every sum.  The list is the reference's: ties by
    position, whatever made the sum."""
    from drn_amd import Shortlister, late_shortlist_reference
    E = 8
    rows = {1: [[3, 0], [0, 5]], 2: [[4, 4]], 4: [[5, 0], [0, 3]], 5: [[1, 1]], 6: [[8, 0], [0, 8], [-8, -8]], 7: [[2, 5]]}
    lens = [len(rows.get(v, [])) for v in range(9)]
    emb = torch.zeros(sum(lens), E)
    emb[:, :2] = torch.tensor([r for v in sorted(rows) for r in rows[v]], dtype=torch.float32)
    q = torch.zeros(3, 3, E)
    q[0, 0, 0] = q[0, 1, 1] = 1                                              # two tokens: e0, e1
    q[1, 0, 1] = q[1, 1, 0] = 1                                              # the same two the other way round
    q[2, 0, 0] = q[2, 1, 1] = 1                                              # three tokens: e0, e1, 0
    lengths = torch.tensor([2, 2, 3], dtype=torch.int32, device=DEV)
    emb, q, off = emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous(), offsets_of(lens)
    want = late_shortlist_reference(emb, off, q, lengths, 9)
    assert want.ids[0].tolist() == [6, 1, 2, 4, 7, 5, -1, -1, -1] and want.scores[0].tolist() == [16., 8., 8., 8., 7., 2., 0., 0., 0.]
    same_lists(Shortlister(emb, offsets=off).shortlist_late(q, lengths, 9), want)


# -- 2. links to the shipped kernels --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_case(R, E, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(R, E, generator=g).to(DEV, dtype).contiguous()
    tok = torch.randn(17, 64, E, generator=g).to(DEV, dtype).contiguous()
    return emb, tok


@DTYPES
def test_one_token_per_sentence_is_the_segment_shortlist(dtype):
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    emb, tok = random_case(int(sum(lens)), 200, dtype, 9)
    sl = Shortlister(emb, offsets=offsets_of(lens))
    ones = torch.ones(17, dtype=torch.int32, device=DEV)
    for n in (1, 16, 128):
        a, b = sl.shortlist(tok[:, 0].contiguous(), n), sl.shortlist_late(tok[:, :1].contiguous(), ones, n)
        same_lists(b, a, n)
        # ... and with the token first among padding
        same_lists(sl.shortlist_late(tok[:, :7].contiguous(), ones, n), a, (n, "padded"))


def summed(sl, q, lengths, V):
    """What the issue defines the sums by: shortlist() of the flattened tokens with n = V, scattered to a dense (S L, V), added over
    the live tokens in ascending order with fp32 torch adds -> (S, V) float32, NaN for a video that is never listed."""
    S_, L = int(q.shape[0]), int(q.shape[1])
    sim = dense(sl.shortlist(q.reshape(S_ * L, -1).contiguous(), V), V).reshape(S_, L, V)
    acc = torch.zeros((S_, V), dtype=torch.float32, device=q.device)
    for t in range(L):
        acc = torch.where((lengths > t)[:, None], acc + sim[:, t], acc)
    return acc


@DTYPES
def test_the_sums_are_fp32_sums_of_the_segment_shortlists_scores_in_token_order(dtype):
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 5 + [40, 2, 9] + [1] * 60                        # V = 83 <= 128, five of them without rows, R = 216
    V = len(lens)
    emb, tok = random_case(int(sum(lens)), 200, dtype, 21)
    sl = Shortlister(emb, offsets=offsets_of(lens))
    owners = torch.tensor([x > 0 for x in lens], device=DEV)
    for L in (5, 17, 33):
        q = tok[:, :L].contiguous()
        lengths = lengths_of(L).clamp(1, L)
        want = summed(sl, q, lengths, V)
        assert bool((torch.isnan(want) == ~owners[None]).all())
        got = sl.shortlist_late(q, lengths, V)
        assert got.n.tolist() == [int(owners.sum())] * 17
        mine = dense(got, V)
        assert torch.equal(torch.isnan(mine), torch.isnan(want)) and torch.equal(mine[:, owners], want[:, owners]), L
        # the list is the stable descending sort of those sums
        order = torch.sort(torch.where(owners[None], want, torch.full_like(want, float("-inf"))), dim=1, descending=True, stable=True).indices
        k = int(owners.sum())
        assert torch.equal(got.ids[:, :k].long(), order[:, :k]), L


# -- 3. what a score depends on -------------------------------------------------------------------------------------------------------------

def test_a_score_depends_on_its_sentence_and_its_video_alone():
    """Bit for bit: a sentence alone and among 17; L = 16 and the same live tokens padded to L = 64 with NaN; a prefix of the table and
    the full table on the prefix's videos; one video's rows under two segmentations of the other videos."""
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 5 + [40, 2, 9] + [1] * 60 + [300]                # V = 84, R = 516
    V, off = len(lens), offsets_of(lens)
    emb, tok = random_case(int(sum(lens)), 200, torch.bfloat16, 33)
    sl = Shortlister(emb, offsets=off)
    q16, lengths = tok[:, :16].contiguous(), lengths_of(16).clamp(max=16)   # (clamped here: the same lengths serve L = 64 below)
    full = sl.shortlist_late(q16, lengths, 128)
    assert int(full.n[0]) == sum(1 for x in lens if x) and int(full.n[1]) == 0
    for s in (0, 2, 3, 16):
        alone = sl.shortlist_late(q16[s:s + 1].contiguous(), lengths[s:s + 1].contiguous(), 128)
        for f in FIELDS:
            assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]), (s, f)
    cut = sl.shortlist_late(q16, lengths, 7)
    same_lists(cut, head(full, 17, 7), "a shorter cut")
    padded = torch.full((17, 64, 200), float("nan"), dtype=torch.bfloat16, device=DEV)
    for s, k in enumerate(lengths.clamp(min=0).tolist()):
        padded[s, :k] = q16[s, :k]                                           # (what q16 holds past a sentence's length becomes NaN too)
    same_lists(sl.shortlist_late(padded, lengths, 128), full, "NaN padding to L = 64")
    k = 23                                                                   # the prefix: the first 23 videos, the blocks cut elsewhere
    pre = Shortlister(emb[:off[k]].contiguous(), offsets=off[:k + 1]).shortlist_late(q16, lengths, 128)
    a, b = dense(pre, k), dense(full, V)[:, :k]
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))
    # video 20 (40 rows) while the rows around it are cut into other videos
    v, lo, hi, R = 20, int(off[20]), int(off[21]), int(off[-1])
    assert hi - lo == 40
    other = list(range(0, lo, 7)) + [lo, hi] + list(range(hi + 50, R, 111)) + [R]
    at = other.index(lo)
    again = dense(Shortlister(emb, offsets=other).shortlist_late(q16, lengths, 128), len(other) - 1)[:, at]
    mine = dense(full, V)[:, v]
    assert torch.equal(torch.isnan(again), torch.isnan(mine)) and torch.equal(again.nan_to_num(7.0), mine.nan_to_num(7.0))
    assert int(torch.isfinite(mine).sum()) == int((full.n > 0).sum())


# -- 4. allow ---------------------------------------------------------------------------------------------------------------------------------

def test_masks_all_ones_a_sub_table_an_empty_row_and_bits_past_the_table():
    from drn_amd import Shortlister, pack_allow
    lens = [1, 3, 0, 17] * 75 + [300]                                        # V = 301, several blocks
    V, off = len(lens), offsets_of(lens)
    emb, tok = random_case(int(sum(lens)), 96, torch.bfloat16, 41)
    sl = Shortlister(emb, offsets=off)
    q, lengths = tok[:, :17].contiguous(), lengths_of(17)
    full = sl.shortlist_late(q, lengths, 128)
    ones = pack_allow(torch.ones(V, dtype=torch.bool, device=DEV))
    same_lists(sl.shortlist_late(q, lengths, 128, allow=ones), full, "all ones, shared")
    same_lists(sl.shortlist_late(q, lengths, 128, allow=ones.repeat(17, 1).contiguous()), full, "all ones, per sentence")
    stuffed = ones.clone()
    stuffed[-1] = -1                                                         # (V = 301: the last word's bits 13 .. 31 lie past the table)
    assert int(stuffed[-1]) != int(ones[-1])
    same_lists(sl.shortlist_late(q, lengths, 128, allow=stuffed), full, "bits at or past V")
    # at most 128 allowed videos == the unmasked list over the table of those videos alone, ids mapped back
    g = torch.Generator().manual_seed(3)
    keep = torch.sort(torch.randperm(V, generator=g)[:100]).values
    keep = torch.unique(torch.cat([keep, torch.tensor([V - 1])]))            # (the long video among them)
    mask = torch.zeros(V, dtype=torch.bool)
    mask[keep] = True
    rows = torch.cat([torch.arange(int(off[v]), int(off[v + 1])) for v in keep.tolist()])
    sub = Shortlister(emb[rows.to(DEV)].contiguous(), offsets=offsets_of([lens[v] for v in keep.tolist()]))
    want = sub.shortlist_late(q, lengths, 128)
    got = sl.shortlist_late(q, lengths, 128, allow=pack_allow(mask.to(DEV)))
    back = torch.where(want.ids >= 0, keep.to(DEV)[want.ids.clamp(min=0).long()].to(torch.int32), want.ids)
    assert torch.equal(got.ids, back) and torch.equal(got.scores, want.scores) and torch.equal(got.n, want.n)
    assert int(got.n[0]) == sum(1 for v in keep.tolist() if lens[v])
    # an all-zero row lists nothing, the other rows are untouched
    per = ones.repeat(17, 1).contiguous()
    per[4] = 0
    got = sl.shortlist_late(q, lengths, 128, allow=per)
    assert int(got.n[4]) == 0 and bool((got.ids[4] == -1).all()) and bool((got.scores[4] == 0).all()) and int(full.n[4]) == 128
    keep_rows = [s for s in range(17) if s != 4]
    for f in FIELDS:
        assert torch.equal(getattr(got, f)[keep_rows], getattr(full, f)[keep_rows]), f


@DTYPES
def test_shared_and_per_sentence_masks_equal_the_reference_on_exact_data(dtype):
    from drn_amd import Shortlister, late_shortlist_reference, pack_allow
    for layout in ("cycle", "long", "ones257"):
        emb, tok, off = tokens_for(layout, 40, dtype)
        V = len(off) - 1
        sl = Shortlister(emb, offsets=off)
        q, lengths = tok[:, :17].contiguous(), lengths_of(17)
        g = torch.Generator().manual_seed(V)
        for shape in ((V,), (17, V)):
            mask = (torch.rand(shape, generator=g) < 0.4).to(DEV)
            for n in (5, 128):
                same_lists(sl.shortlist_late(q, lengths, n, allow=pack_allow(mask)), late_shortlist_reference(emb, off, q, lengths, n, allow=mask),
                           (layout, shape, n))


# -- 5. block-scaled FP8 tables ----------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantised_late_shortlist_is_the_dequantised_one_and_the_reference(dtype, E):
    """Exact tables (values k 2^e, multiples of 2^-2 of magnitude at most 64) and integer tokens in [-4, 4]: a dot product is a multiple
    of 2^-2 of magnitude at most 2^17 at E = 512, and a sum of 16 of them one of magnitude at most 2^21 -- 23 bits, exact in fp32.  Every
    field equals dequantized().shortlist_late() and the float64 definition over the dequantised table; a random table at L = 33, where
    nothing is exact, still equals dequantized() bit for bit."""
    from drn_amd import Shortlister, late_shortlist_reference, pack_allow
    from drn_amd.index import mx8_dequantize
    for lens in ([1, 3, 0, 17] * 30, [2, 300, 1, 0, 4], [1] * 257):
        codes, scales, _, off = exact_tables(tuple(lens), E)
        table = mx8_dequantize(codes, scales)
        sl = Shortlister.from_mx8(codes, scales, dtype, offsets=off)
        oracle = sl.dequantized()
        mask = torch.arange(len(lens), device=DEV) % 3 != 1
        for L in (5, 16):
            q, lengths = exact_tokens(E, dtype)[:, :L].contiguous(), lengths_of(L)
            for n in (5, 128):
                got = sl.shortlist_late(q, lengths, n)
                same_lists(got, oracle.shortlist_late(q, lengths, n), (len(lens), L, n))
                same_lists(got, late_shortlist_reference(table, off, q, lengths, n), (len(lens), L, n, "reference"))
            same_lists(sl.shortlist_late(q, lengths, 128, allow=pack_allow(mask)),
                       late_shortlist_reference(table, off, q, lengths, 128, allow=mask), (len(lens), L, "masked"))
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    g = torch.Generator().manual_seed(E)
    emb = (torch.randn(int(sum(lens)), E, generator=g)
           * torch.exp2(torch.randint(-3, 4, (int(sum(lens)), E // 32), generator=g).float()).repeat_interleave(32, dim=1)).to(DEV, dtype)
    tok = torch.randn(17, 33, E, generator=g).to(DEV, dtype).contiguous()
    sl = Shortlister(emb.contiguous(), offsets=offsets_of(lens), quantize="mxfp8")
    same_lists(sl.shortlist_late(tok, lengths_of(33), 128), sl.dequantized().shortlist_late(tok, lengths_of(33), 128), "random")


# -- 6. random data against float64 ------------------------------------------------------------------------------------------------------------

def late_case_ratio(emb, q, lengths, off, got):
    """The checks of random data -> the largest |error| / tol.  tol[s, v] = sum over the live t of max over v's rows of E 2^-23 sum_e
    |q[s, t, e] emb[r, e]| -- the bound of one dot product that tests/test_shortlist_gpu.py derives, taken at the worst row since |max a
    - max b| <= max |a - b| -- plus L 2^-23 sum over the live t of |sim[s, t, v]|, the fp32 running sum of L terms.  A returned score
    is within tol of the float64 score, the list is sorted on the returned scores, and nobody left out is better than the last one
    listed by more than both tolerances (the comparison of tests/test_segment_shortlist_gpu.py)."""
    S_, L, E = (int(x) for x in q.shape)
    V = len(off) - 1
    lens = torch.as_tensor(np.diff(off), device=emb.device)
    video = torch.repeat_interleave(torch.arange(V, device=emb.device), lens)[None].expand(S_ * L, -1)
    flat = q.double().reshape(S_ * L, E)
    dot = flat @ emb.double().t()
    tol_row = E * 2.0 ** -23 * (flat.abs() @ emb.double().abs().t())
    sim = torch.full((S_ * L, V), float("-inf"), dtype=torch.float64, device=emb.device).scatter_reduce(1, video, dot, "amax").reshape(S_, L, V)
    tol_dot = torch.zeros((S_ * L, V), dtype=torch.float64, device=emb.device).scatter_reduce(1, video, tol_row, "amax").reshape(S_, L, V)
    live = (torch.arange(L, device=emb.device)[None] < lengths.clamp(0, L)[:, None])[:, :, None]
    owners = lens > 0
    sim = torch.where(live & owners[None, None], sim, torch.zeros_like(sim))
    ref = sim.sum(dim=1)
    tol = torch.where(live, tol_dot, torch.zeros_like(tol_dot)).sum(dim=1) + L * 2.0 ** -23 * sim.abs().sum(dim=1)
    worst = 0.0
    for s in range(S_):
        n = int(got.n[s])
        ids, sc = got.ids[s, :n].long(), got.scores[s, :n].double()
        assert n == got.ids.shape[1] and len(set(ids.tolist())) == n and bool(owners[ids].all())
        err = (sc - ref[s, ids]).abs()
        assert bool((err <= tol[s, ids]).all()), s
        worst = max(worst, float((err / tol[s, ids]).max()))
        assert bool(((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:-1] < ids[1:]))).all()), s
        out = owners.clone()
        out[ids] = False
        last = ids[-1]
        assert bool((ref[s][out] <= ref[s, last] + tol[s][out] + tol[s, last]).all()), s
    return worst


def test_late_shortlist_on_random_bf16_data_is_within_the_derived_bound():
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    emb, tok = random_case(int(sum(lens)), 512, torch.bfloat16, 4)
    off = offsets_of(lens)
    q = tok[:5, :33].contiguous()
    lengths = torch.tensor([33, 1, 16, 17, 20], dtype=torch.int32, device=DEV)
    ratio = late_case_ratio(emb, q, lengths, off, Shortlister(emb, offsets=off).shortlist_late(q, lengths, 16))
    print("largest error / tol: %.4f" % ratio)
    assert ratio <= 1.0


# -- 7. buffers, graphs ------------------------------------------------------------------------------------------------------------------------

def test_out_buffers_and_the_workspace_stay_inside_their_guards_and_a_captured_call_replays():
    """out= written in place, every element; guard bands around the three outputs AND the workspace untouched; a captured call replays
    after queries, lengths and the mask were overwritten in place; the whole call, masked and not, runs with torch's synchronisation
    check armed."""
    from drn_amd import Shortlist, Shortlister, late_shortlist_reference, ops, pack_allow
    from drn_amd.graph import capture_graph
    emb, tok, off = tokens_for("cycle", 40, torch.bfloat16)
    V = len(off) - 1
    sl = Shortlister(emb, offsets=off)
    S_, L, n, GUARD = 5, 17, 100, 64
    q, lengths = tok[:S_, :L].contiguous(), torch.tensor([17, 0, 1, 16, 5], dtype=torch.int32, device=DEV)
    q2, lengths2 = tok[5:5 + S_, 3:3 + L].contiguous(), torch.tensor([2, 17, 30, 0, 16], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(8)
    mask, mask2 = ((torch.rand((S_, V), generator=g) < p).to(DEV) for p in (0.5, 0.8))
    shapes = ((S_, n), (S_, n), (S_,))
    dtypes = (torch.int32, torch.float32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = Shortlist(*(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes)))
    keys = ops.shortlist_late_ws_keys(len(sl.plan.blk_vid) - 1, S_, n)
    wsflat = torch.full((keys + 2 * GUARD,), 77, dtype=torch.int64, device=DEV)
    sl._ws[("late", S_, n)] = wsflat[GUARD:GUARD + keys]

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat + [wsflat])
    qbuf, lbuf, words = q.clone(), lengths.clone(), pack_allow(mask)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = sl.shortlist_late(qbuf, lbuf, n, out=out, allow=words)
        bare = sl.shortlist_late(qbuf, lbuf, n, out=None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(a is b for a, b in zip(got, out)) and guards_hold() and sl._ws[("late", S_, n)].data_ptr() == wsflat[GUARD:].data_ptr()
    same_lists(out, late_shortlist_reference(emb, off, q, lengths, n, allow=mask), "every element")
    same_lists(bare, late_shortlist_reference(emb, off, q, lengths, n), "no mask")
    small = Shortlister(emb[:4].contiguous(), offsets=[0, 1, 1, 4])
    for t in out:
        t.fill_(77)
    same_lists(small.shortlist_late(q, lengths, n, out=out), late_shortlist_reference(emb[:4], [0, 1, 1, 4], q, lengths, n), "the tail past the list")
    assert guards_hold()
    # capture on one stream, then replay on other queries, lengths and mask written into the captured buffers
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist_late(qbuf, lbuf, n, out=out, allow=words)            # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sl.shortlist_late(qbuf, lbuf, n, out=out, allow=words)
    for queries, lens_, m in ((q2, lengths2, mask2), (q, lengths, mask)):
        qbuf.copy_(queries), lbuf.copy_(lens_), pack_allow(m, out=words)
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_lists(out, late_shortlist_reference(emb, off, queries, lens_, n, allow=m), "replay == reference")
    assert guards_hold()


# -- 8. the two stages -------------------------------------------------------------------------------------------------------------------------

def test_late_ids_are_device_candidates_of_the_graphed_search():
    """Grounder(graph=True).search(candidates=short.ids) on a small index == the same rows passed as host lists, field for field; the shortlist
    reads nothing on the host (torch raises on a synchronising call meanwhile) and is one tagged entry."""
    from drn_amd import Grounder, Shortlister, ops
    m, store, index, kw = world("plain")
    lens = [3, 1, 0, 17, 2, 5, 1]
    assert len(lens) == NV
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (int(off[-1]), 16), generator=g).float()
    emb[off[4]:off[5]] = emb[off[1]]                                       # a tie between videos the shortlist breaks by position
    sl = Shortlister(emb.to(DEV).contiguous(), names=store.names, offsets=off)
    sl.check(store), sl.check(index)
    qe = torch.randint(-4, 5, (S, 6, 16), generator=g).float().to(DEV)
    lengths = torch.tensor([6, 0, 3], dtype=torch.int32, device=DEV)      # a sentence whose shortlist is empty: ids all -1
    grounder = Grounder(m, top_k=5, graph=True, **kw)
    tok, qlen = sentences(7)
    n = 4
    grounder.search(tok, qlen, index, per_video=2, candidates=sl.shortlist_late(qe, lengths, n).ids)     # (warm, and the capture)
    torch.cuda.synchronize()
    ops.kernel_timer = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        short = sl.shortlist_late(qe, lengths, n)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    assert tags == ["shortlist_late_topn"]
    lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
    assert [len(l) for l in lists] == [n, 0, n] and all(2 not in l for l in lists)
    same_hits(got, Grounder(m, top_k=5, **kw).search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "two stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0
