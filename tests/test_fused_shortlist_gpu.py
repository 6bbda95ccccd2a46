"""Dense scores and fused shortlists on the device (csrc/retrieve_fuse.hip): Shortlister.scores / scores_late against scores_reference
on exact data and against the kernels' own lists and ranks on random data; under masks, into strided and guarded buffers, over shards;
shortlist_scores against shortlist() and shortlist_deep(); FusedShortlister.shortlist and rank against the fold of the tables' own
scores() -- bit for bit, since the references fold the same fp32 inputs in the same stated order.
Every comparison is torch.equal, scores as int32 bits, except the one derived bound that is named.
No product and no partial sum of a fused score is subnormal here: the exact tables hold integers and the weights are dyadic, and on
the random tables a score is a sum of E >= 8 products of magnitude around 1, a weight is at least 2^-3 in magnitude or exactly 0, and a
difference of two fp32 numbers of magnitude above 2^-100 is 0 or at least 2^-124.
tests/test_fused_shortlist_cpu.py holds the definitions, the refusals and the C boundary."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_allow_shortlist_gpu import EMPTY, bool_masks, build, packed, random_table
from test_grounding_engine_gpu import DEV
from test_late_shortlist_gpu import exact_tokens, lengths_of
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import exact_case, offsets_of
from test_shortlist_gpu import BLOCK, exact_data, world

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
FOUR = pytest.mark.parametrize("table,ragged", [("plain", False), ("plain", True), ("mxfp8", False), ("mxfp8", True)],
                               ids=["plain", "segments", "q8", "q8-segments"])
NINF = float("-inf")


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    if not torch.equal(bits(got), bits(want)):
        bad = (bits(got) != bits(want)).nonzero()
        i = tuple(int(x) for x in bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, bad.shape[0], got.numel(), i, float(got[i]), float(want[i])))


def same_fields(got, want, what="", fields=("ids", "scores", "n")):
    for f in fields:
        a, b = getattr(got, f), getattr(want, f)
        assert torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b), (what, f)


def same_ranks(got, want, what=""):
    same_fields(got, want, what, ("rank", "score", "total"))


def cycle_lens(V, seed=0):
    """V run lengths cycling 1 / 3 / 0 / 17, started at `seed`."""
    return [(1, 3, 0, 17)[(v + seed) % 4] for v in range(V)]


# -- 1. scores against the definitions, exact data ---------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [5, 8, 40, 512])
def test_plain_scores_equal_the_reference_exactly(dtype, E):
    """V: one video; one short of, exactly and one past a 64-video wave tile; a block + 1; three blocks + 7.  E = 5 and 40 take the
    tail loads.  S = 17 is a second sentence tile of one row.  A row of the matrix depends on its sentence alone."""
    from drn_amd import Shortlister, scores_reference
    for V in (1, 63, 64, 65, 257, 775):
        emb, q17 = exact_data(V, E, 17, dtype)
        want17 = scores_reference(emb, q17)
        assert bool(torch.isfinite(want17).all())
        sl = Shortlister(emb)
        for S_ in (1, 16, 17):
            got = sl.scores(q17[:S_].contiguous())
            assert tuple(got.shape) == (S_, V) and got.is_contiguous()
            same_bits(got, want17[:S_], (V, S_))


@DTYPES
@pytest.mark.parametrize("E", [32, 64, 512])
def test_quantised_scores_are_those_of_the_dequantised_rows(dtype, E):
    from drn_amd import scores_reference
    for V in (1, 65, 775):
        emb, q17 = exact_data(V, E, 17, dtype)
        sl = build(emb, "mxfp8")
        for S_ in (1, 17):
            q = q17[:S_].contiguous()
            got = sl.scores(q)
            same_bits(got, sl.dequantized().scores(q), (V, S_))
            same_bits(got, scores_reference(emb, q), (V, S_))
    for layout in ("cycle", "long", "ones257"):
        emb, q17, off = exact_case(layout, E, dtype)
        sl = build(emb, "mxfp8", offsets=off)
        got = sl.scores(q17)
        same_bits(got, sl.dequantized().scores(q17), layout)
        same_bits(got, scores_reference(emb, q17, offsets=off), layout)
        tok, lengths = exact_tokens(E, dtype)[:, :17].contiguous(), lengths_of(17)
        got = sl.scores_late(tok, lengths)
        same_bits(got, sl.dequantized().scores_late(tok, lengths), layout)
        same_bits(got, scores_reference(emb, tok, offsets=off, lengths=lengths), layout)


@DTYPES
@pytest.mark.parametrize("E", [8, 40])
def test_ragged_and_late_scores_equal_the_reference_exactly(dtype, E):
    """Runs cycling 1 / 3 / 0 / 17 (videos without rows: -inf), a 300- and a 600-row video (several passes), 257 one-row videos (a second
    block of one video) and R = V = 1; late at L = 1 / 16 / 17 with lengths that mix 0, 1, L and values outside [0, L]."""
    from drn_amd import Shortlister, scores_reference
    for layout in ("cycle", "long", "ones257", "one"):
        emb, q17, off = exact_case(layout, E, dtype)
        V = len(off) - 1
        empty = torch.from_numpy(np.diff(off) == 0).to(DEV)
        sl = Shortlister(emb, offsets=off)
        want17 = scores_reference(emb, q17, offsets=off)
        assert bool((want17[:, empty] == NINF).all()) and bool(torch.isfinite(want17[:, ~empty]).all())
        for S_ in (1, 16, 17):
            same_bits(sl.scores(q17[:S_].contiguous()), want17[:S_], (layout, S_))
        for L in (1, 16, 17):
            tok, lengths = exact_tokens(E, dtype)[:, :L].contiguous(), lengths_of(L)
            want = scores_reference(emb, tok, offsets=off, lengths=lengths)
            assert bool((want[1] == NINF).all()) and bool((want[10] == NINF).all()) and bool(torch.isfinite(want[0, ~empty]).all())
            for S_ in (1, 3, 17):
                got = sl.scores_late(tok[:S_].contiguous(), lengths[:S_].contiguous())
                assert tuple(got.shape) == (S_, V)
                same_bits(got, want[:S_], (layout, L, S_))


# -- 2. scores against the kernels' own lists and ranks, random data ---------------------------------------------------------------------------

def dense_rank(sc, targets):
    """TargetRank's three fields by integer counting over a dense score matrix (finite <=> candidate)."""
    S_, V = sc.shape
    t = targets.long()
    inside = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)[:, None]
    ts = torch.gather(sc, 1, tc)
    finite = torch.isfinite(sc)
    found = inside & torch.isfinite(ts[:, 0])
    before = finite & ((sc > ts) | ((sc == ts) & (torch.arange(V, device=sc.device)[None, :] < tc)))
    rank = torch.where(found, before.sum(dim=1), torch.full_like(t, -1)).to(torch.int32)
    return rank, torch.where(found, ts[:, 0], torch.zeros_like(ts[:, 0])), finite.sum(dim=1).to(torch.int32)


@FOUR
def test_a_dense_score_has_the_bits_of_the_listed_score_and_counts_to_the_rank(table, ragged):
    """Random bf16 data at E = 512, where another summation order would show in the bits: scores()[s, ids[s, k]] has the bits of
    shortlist(q, 128).scores[s, k]; rank()'s three fields are the integer counts over the dense matrix; the same by late interaction."""
    from drn_amd import Shortlister
    V = 3 * BLOCK + 7
    off = offsets_of(cycle_lens(V)) if ragged else None
    emb, q17 = random_table(int(off[-1]) if ragged else V, 512, torch.bfloat16, seed=21)
    sl = Shortlister(emb, quantize=None if table == "plain" else table, offsets=off)
    g = torch.Generator().manual_seed(2)
    targets = torch.randint(0, V, (17,), generator=g).to(torch.int32)
    targets[3], targets[4], targets[5] = -1, V, 2                              # (no target twice; video 2 owns no row on the ragged table)
    targets = targets.to(DEV)

    def check(sc, short, rk, what):
        assert bool((short.n == 128).all())
        same_bits(torch.gather(sc, 1, short.ids.long()), short.scores, what)
        rank, score, total = dense_rank(sc, targets)
        assert torch.equal(rk.rank, rank) and torch.equal(bits(rk.score), bits(score)) and torch.equal(rk.total, total), what
        assert not bool(torch.isnan(sc).any()) and int(rk.rank.max()) >= 0 and int(rk.rank[3]) == int(rk.rank[4]) == -1
    sc = sl.scores(q17)
    check(sc, sl.shortlist(q17, 128), sl.rank(q17, targets), "one vector a sentence")
    if ragged:
        assert int(sl.rank(q17, targets).rank[5]) == -1 and bool((sc[:, 2] == NINF).all())
        tok = torch.randn(17, 5, 512, generator=g).to(DEV, torch.bfloat16)
        lengths = torch.tensor([5, 1, 3, 5, 2, 4, 5, 5, 1, 2, 3, 4, 5, 5, 5, 1, 5], dtype=torch.int32, device=DEV)
        check(sl.scores_late(tok, lengths), sl.shortlist_late(tok, lengths, 128), sl.rank_late(tok, lengths, targets), "late")


def test_random_bf16_scores_are_within_the_derived_bound_of_float64():
    """Every finite entry within E * 2^-23 * sum_e |q_e * emb_e| of the float64 score: the bound tests/test_shortlist_gpu.py derives."""
    from drn_amd import Shortlister
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(775, 512, generator=g).to(DEV, torch.bfloat16).contiguous()
    q = torch.randn(17, 512, generator=g).to(DEV, torch.bfloat16).contiguous()
    got = Shortlister(emb).scores(q)
    assert bool(torch.isfinite(got).all())
    ref = q.double() @ emb.double().t()
    tol = 512 * 2.0 ** -23 * (q.double().abs() @ emb.double().abs().t())
    ratio = float(((got.double() - ref).abs() / tol).max())
    print("largest error / tol: %.4f" % ratio)
    assert ratio <= 1.0


# -- 3. masks and views ------------------------------------------------------------------------------------------------------------------------

@FOUR
def test_scores_under_masks_into_strided_and_guarded_buffers(table, ragged):
    """A shared mask; per-sentence masks with an all-zero row (a row of -inf) and, on the plain table, block 1 dark for every sentence
    but one and block 2 for all; a NaN query row is a row of -inf and leaves the others alone; a sentence alone has the bits it has
    among 17; out= a column slice of a wider buffer: the columns outside it and the guard bands around the buffer stay untouched."""
    from drn_amd import scores_reference
    V = 3 * BLOCK + 7
    off = offsets_of(cycle_lens(V)) if ragged else None
    emb, q = exact_data(int(off[-1]) if ragged else V, 64, 17, torch.bfloat16)
    sl = build(emb, table, **({"offsets": off} if ragged else {}))
    shared, per = bool_masks(V)
    if not ragged:
        assert int(per[:, BLOCK:2 * BLOCK].any(dim=1).sum()) == 1 and not bool(per[:, 2 * BLOCK:3 * BLOCK].any()), "no dark block"
    free = sl.scores(q)
    same_bits(free, scores_reference(emb, q, offsets=off), "no mask")
    for what, mask in (("shared", shared), ("per sentence", per)):
        got = sl.scores(q, allow=packed(mask))
        same_bits(got, scores_reference(emb, q, offsets=off, allow=mask.to(DEV)), what)
        # a masked entry is the unmasked one or -inf
        same_bits(got, torch.where(mask.to(DEV).expand(17, V), free, torch.full_like(free, NINF)), what)
    assert bool((got[EMPTY] == NINF).all()) and bool(torch.isfinite(got).any())
    bad = q.clone()
    bad[2, 7], bad[16, 0] = float("nan"), float("inf")
    got = sl.scores(bad)
    keep = [s for s in range(17) if s not in (2, 16)]
    assert bool((got[2] == NINF).all()) and not bool(torch.isnan(got).any())
    same_bits(got[keep].contiguous(), free[keep].contiguous(), "the other sentences")
    for s in (0, 16):
        same_bits(sl.scores(q[s:s + 1].contiguous(), allow=packed(per[s:s + 1].contiguous())),
                  sl.scores(q, allow=packed(per))[s:s + 1].contiguous(), "a sentence alone")
    GUARD, LEFT, WIDE = 64, 13, V + 40
    flat = torch.full((17 * WIDE + 2 * GUARD,), 77.0, dtype=torch.float32, device=DEV)
    wide = flat[GUARD:GUARD + 17 * WIDE].view(17, WIDE)
    out = wide[:, LEFT:LEFT + V]
    assert sl.scores(q, out=out, allow=packed(per)) is out
    same_bits(out.contiguous(), scores_reference(emb, q, offsets=off, allow=per.to(DEV)), "a column slice")
    assert bool((wide[:, :LEFT] == 77).all()) and bool((wide[:, LEFT + V:] == 77).all())
    assert bool((flat[:GUARD] == 77).all()) and bool((flat[GUARD + 17 * WIDE:] == 77).all())
    if ragged:
        tok, lengths = exact_tokens(64, torch.bfloat16)[:, :5].contiguous(), lengths_of(5)
        wide.fill_(77.0)
        assert sl.scores_late(tok, lengths, out=out, allow=packed(per)) is out
        same_bits(out.contiguous(), scores_reference(emb, tok, offsets=off, lengths=lengths, allow=per.to(DEV)), "late, a column slice")
        assert bool((wide[:, :LEFT] == 77).all()) and bool((wide[:, LEFT + V:] == 77).all())
        assert bool((flat[:GUARD] == 77).all()) and bool((flat[GUARD + 17 * WIDE:] == 77).all())


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_sharded_scores_are_the_single_tables(ragged):
    """Three shards, plain and FP8 mixed, of 300 + 7 + 468 videos: every column is bit for bit what ONE table over the concatenated
    (dequantised) rows writes, with and without a mask over the corpus, also by late interaction."""
    from drn_amd import ShardedShortlister, Shortlister
    sizes = (300, 7, 468)
    V = sum(sizes)
    lens = cycle_lens(V) if ragged else [1] * V
    off = offsets_of(lens)
    emb, q17 = random_table(int(off[-1]), 96, torch.bfloat16, seed=9)
    shards, a = [], 0
    for k, size in enumerate(sizes):
        r0, r1 = int(off[a]), int(off[a + size])
        kw = {"offsets": off[a:a + size + 1] - off[a]} if ragged else {}
        shards.append(Shortlister(emb[r0:r1].contiguous(), quantize="mxfp8" if k == 1 else None, **kw))
        a += size
    corpus = ShardedShortlister(shards)
    rows = torch.cat([s.dequantized().embeddings for s in shards]).contiguous()
    one = Shortlister(rows, **({"offsets": off} if ragged else {}))
    shared, per = bool_masks(V)
    same_bits(corpus.scores(q17), one.scores(q17), "no mask")
    for mask in (shared, per):
        same_bits(corpus.scores(q17, allow=packed(mask)), one.scores(q17, allow=packed(mask)), "masked")
    if ragged:
        g = torch.Generator().manual_seed(1)
        tok, lengths = torch.randn(17, 5, 96, generator=g).to(DEV, torch.bfloat16), lengths_of(5)
        same_bits(corpus.scores_late(tok, lengths, allow=packed(per)), one.scores_late(tok, lengths, allow=packed(per)), "late")


# -- 4. shortlist_scores -----------------------------------------------------------------------------------------------------------------------

@FOUR
def test_ranking_a_tables_own_scores_gives_its_shortlists(table, ragged):
    """shortlist_scores(scores(q), n) == shortlist(q, n) at n = 1 / 5 / 128 and shortlist_deep(q, n) at n = 300 / 1024, on ids, scores
    and n: exact data with planted ties, V = six blocks + 7."""
    from drn_amd import Shortlist, shortlist_scores
    V = 6 * BLOCK + 7
    off = offsets_of(cycle_lens(V)) if ragged else None
    emb, q = exact_data(int(off[-1]) if ragged else V, 64, 17, torch.bfloat16)
    sl = build(emb, table, **({"offsets": off} if ragged else {}))
    sc = sl.scores(q)
    shared, per = bool_masks(V)
    for n in (1, 5, 128, 300, 1024):
        want = sl.shortlist(q, n) if n <= 128 else sl.shortlist_deep(q, n)
        got = shortlist_scores(sc, n)
        assert isinstance(got, Shortlist)
        same_fields(got, want, n)
        same_fields(shortlist_scores(sc, n, allow=packed(per)),
                    sl.shortlist(q, n, allow=packed(per)) if n <= 128 else sl.shortlist_deep(q, n, allow=packed(per)), ("masked", n))
    assert bool(((got.scores[:, 1:] == got.scores[:, :-1]) & (got.ids[:, 1:] > got.ids[:, :-1]) & (got.ids[:, 1:] >= 0)).any()), "no tie"


def test_shortlist_scores_ranks_any_matrix_under_the_total_order():
    """Planted ties across a 256-video block edge; entries that are not finite; a matrix of all -inf; lists shorter than n; a row-strided
    matrix; out= inside guard bands -- against fused_shortlist_reference with one table of weight one."""
    from drn_amd import Shortlist, fused_shortlist_reference, shortlist_scores
    g = torch.Generator().manual_seed(6)
    V = 2 * BLOCK + 9
    x = torch.randn(5, V, generator=g)
    x[:, 10], x[:, BLOCK - 1], x[:, BLOCK], x[:, 2 * BLOCK + 8] = 9.0, 9.0, 9.0, 9.0
    x[1, 7], x[1, 8], x[1, 9], x[1, 11] = NINF, float("nan"), float("inf"), -0.0
    x[2] = NINF
    x[3, 40:] = NINF                                                             # a list of 40
    x = x.to(DEV)
    for n in (1, 5, 128, 129, 600, 1024):
        got = shortlist_scores(x, n)
        same_fields(got, fused_shortlist_reference(x[None], None, n), n)
        if n >= 4:
            assert got.ids[0, :4].tolist() == [10, BLOCK - 1, BLOCK, 2 * BLOCK + 8]
        assert int(got.n[2]) == 0 and bool((got.ids[2] == -1).all()) and bool((got.scores[2] == 0).all())
        assert int(got.n[3]) == min(n, 40) and int(got.n[1]) == min(n, V - 3)
    wide = torch.full((5, V + 30), 123.0, device=DEV)
    wide[:, 11:11 + V] = x
    n, GUARD = 300, 64
    shapes, dtypes = ((5, n), (5, n), (5,)), (torch.int32, torch.float32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = Shortlist(*(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes)))
    got = shortlist_scores(wide[:, 11:11 + V], n, out=out)
    assert all(a is b for a, b in zip(got, out))
    same_fields(got, fused_shortlist_reference(x[None], None, n), "strided in, guarded out")
    assert all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)


# -- 5. fused ----------------------------------------------------------------------------------------------------------------------------------

VF = 2 * BLOCK + 88                                          # 600 videos: three blocks, the last of 88
WEIGHTS = [1.0, -0.5, 0.0, 0.125, 2.0, 1.0, -1.0, 0.25]      # a negative one, a zero and 2^-3 among them


@functools.lru_cache(maxsize=None)
def fused_world(exact):
    """Four ways to score the same VF videos -> (tables, items, references' inputs): a plain bf16 table (E = 40), a ragged fp32 table
    (E = 8; runs cycling 1 / 3 / 0 / 17: every fourth video owns no row), an FP8 ragged table with OTHER offsets (E = 64; runs cycling
    0 / 17 / 1 / 3) and that table again by late interaction (L = 5).  exact: integers in [-4, 4]; else random values.  Shared, changed
    by no test."""
    from drn_amd import Shortlister
    g = torch.Generator().manual_seed(31 if exact else 32)
    draw = (lambda *sh: torch.randint(-4, 5, sh, generator=g).float()) if exact else (lambda *sh: torch.randn(*sh, generator=g))
    off_b, off_c = offsets_of(cycle_lens(VF)), offsets_of(cycle_lens(VF, seed=2))
    names = ["v%d" % v for v in range(VF)]
    ea = draw(VF, 40).to(DEV, torch.bfloat16).contiguous()
    eb = draw(int(off_b[-1]), 8).to(DEV).contiguous()
    ec = draw(int(off_c[-1]), 64).to(DEV, torch.bfloat16).contiguous()
    a, b = Shortlister(ea, names=names), Shortlister(eb, offsets=off_b)
    c = Shortlister(ec, names=names, offsets=off_c, quantize="mxfp8")
    qa, qb = draw(17, 40).to(DEV, torch.bfloat16).contiguous(), draw(17, 8).to(DEV).contiguous()
    qc, tok = draw(17, 64).to(DEV, torch.bfloat16).contiguous(), draw(17, 5, 64).to(DEV, torch.bfloat16).contiguous()
    lengths = torch.tensor([5, 1, 0, 3, 5, 2, 4, 5, 5, 1, 2, 3, 4, 5, 5, 1, 5], dtype=torch.int32, device=DEV)
    tables, items = [a, b, c, c], [qa, qb, qc, (tok, lengths)]
    dq = c.dequantized().embeddings
    defs = [(ea, qa, None, None), (eb, qb, off_b, None), (dq, qc, off_c, None), (dq, tok, off_c, lengths)]
    return tables, items, defs


def own_scores(tables, items):
    return torch.stack([t.scores_late(*i) if isinstance(i, tuple) else t.scores(i) for t, i in zip(tables, items)])


def pick(world_, M):
    """The first M of the four ways, cycled: M = 8 uses each twice."""
    tables, items, defs = world_
    idx = [m % 4 for m in range(M)]
    return [tables[i] for i in idx], [items[i] for i in idx], [defs[i] for i in idx]


@pytest.mark.parametrize("missing", ["drop", "skip"])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_fused_lists_and_ranks_equal_the_fold_of_the_tables_own_scores(exact, M, missing):
    """shortlist and rank == fused_shortlist_reference / fused_rank_reference of the stacked scores() outputs, bit for bit on random data
    too; on exact data also == the fold of scores_reference.  rank[s] = k exactly when ids[s, k] is the target, n = 5 / 128 / 1024.
    The videos that own no row in the ragged tables are dropped under "drop" and kept under "skip"."""
    from drn_amd import FusedShortlister, Shortlist, TargetRank, fused_rank_reference, fused_shortlist_reference, scores_reference
    tables, items, defs = pick(fused_world(exact), M)
    w = WEIGHTS[:M]
    fused = FusedShortlister(tables, weights=w, missing=missing)
    assert len(fused) == VF and fused.names == ["v%d" % v for v in range(VF)]
    stack = own_scores(tables, items)
    if exact:
        ref = torch.stack([scores_reference(e, q, offsets=o, lengths=l) for e, q, o, l in defs])
        same_bits(stack, ref, "the tables' scores are the definition's")
    g = torch.Generator().manual_seed(M)
    targets = torch.randint(0, VF, (17,), generator=g).to(torch.int32)
    targets[0], targets[1], targets[6] = -1, VF, 2                              # (video 2 owns no row in table 1)
    targets = targets.to(DEV)
    rk = fused.rank(items, targets)
    assert isinstance(rk, TargetRank)
    same_ranks(rk, fused_rank_reference(stack, w, targets, missing), "rank")
    total = int(rk.total.max())
    if M == 1:
        assert total == VF
    elif missing == "drop":
        assert 0 < total <= VF - VF // 4 and int(rk.rank[6]) == -1              # (every fourth video owns no row in table 1)
    else:
        assert total == VF and int(rk.total[2]) == VF                           # (the sentence without a live token skips the late table)
    for n in (5, 128, 1024):
        got = fused.shortlist(items, n)
        assert isinstance(got, Shortlist) and tuple(got.ids.shape) == (17, n)
        same_fields(got, fused_shortlist_reference(stack, w, n, missing), n)
        at = (got.ids == targets[:, None]) & (targets[:, None] >= 0)
        place = torch.where(at.any(dim=1), at.int().argmax(dim=1), torch.full((17,), -1, device=DEV))
        inside = (rk.rank >= 0) & (rk.rank < n)
        assert torch.equal(torch.where(inside, rk.rank.long(), torch.full_like(place, -1)), place), n
        assert torch.equal(bits(torch.gather(got.scores, 1, place.clamp(min=0)[:, None])[:, 0][inside]), bits(rk.score[inside])), n
    assert bool((rk.rank >= 0).any())


def test_fused_masks_apply_after_fusion_and_sharded_tables_fuse_too():
    """allow= reaches the ranking launch alone: the stacked buffer holds the UNMASKED scores whatever the mask; the list and the rank are
    the references' under allow=.  A ShardedShortlister among the tables answers as the single table does."""
    from drn_amd import FusedShortlister, ShardedShortlister, Shortlister, fused_rank_reference, fused_shortlist_reference
    tables, items, _ = pick(fused_world(False), 3)
    w = [1.0, 0.25, -0.5]
    stack = own_scores(tables, items)
    shared, per = bool_masks(VF)
    targets = torch.arange(17, dtype=torch.int32, device=DEV) * 31
    for missing in ("drop", "skip"):
        fused = FusedShortlister(tables, weights=w, missing=missing)
        for mask in (shared, per):
            got = fused.shortlist(items, 300, allow=packed(mask))
            same_fields(got, fused_shortlist_reference(stack, w, 300, missing, allow=mask.to(DEV)), missing)
            same_bits(fused._bufs[("scores", 17)], stack, "the stacked buffer is unmasked")
            same_ranks(fused.rank(items, targets, allow=packed(mask)), fused_rank_reference(stack, w, targets, missing, allow=mask.to(DEV)))
        assert int(got.n[EMPTY]) == 0 and bool((got.ids[EMPTY] == -1).all())
    plain = tables[0]
    parts = ShardedShortlister([Shortlister(plain.embeddings[:300].contiguous()), Shortlister(plain.embeddings[300:].contiguous(), quantize=None)])
    a = FusedShortlister([parts, tables[1], tables[2]], weights=w, missing="skip")
    b = FusedShortlister(tables, weights=w, missing="skip")
    same_fields(a.shortlist(items, 128), b.shortlist(items, 128), "a sharded table")
    same_ranks(a.rank(items, targets), b.rank(items, targets), "a sharded table")


def test_fused_buffers_stay_inside_their_guards_and_a_captured_call_replays():
    """Guard bands around the workspace, the stacked score buffer and the outputs; the whole call with torch's synchronisation check
    armed; one captured graph replayed after queries, lengths, weights and mask were overwritten in place."""
    from drn_amd import FusedShortlister, Shortlist, TargetRank, fused_rank_reference, fused_shortlist_reference, ops
    from drn_amd.graph import capture_graph
    tables, items, _ = pick(fused_world(False), 4)
    S_, n, GUARD, M = 5, 300, 64, 4
    head = lambda its, a: [(i[0][a:a + S_].contiguous(), i[1][a:a + S_].contiguous()) if isinstance(i, tuple) else i[a:a + S_].contiguous() for i in its]
    first, second = head(items, 0), head(items, 7)
    wdev = torch.tensor(WEIGHTS[:M], dtype=torch.float32, device=DEV)
    fused = FusedShortlister(tables, weights=wdev, missing="skip")
    assert fused.weights is wdev
    shapes = ((S_, n), (S_, n), (S_,), (S_,), (S_,), (S_,))
    dtypes = (torch.int32, torch.float32, torch.int32, torch.int32, torch.float32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    bufs = [f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes)]
    out, rout = Shortlist(*bufs[:3]), TargetRank(*bufs[3:])
    keys = ops.shortlist_ws_keys(VF, S_, n)
    wsflat = torch.full((keys + 2 * GUARD,), 77, dtype=torch.int64, device=DEV)
    scflat = torch.full((M * S_ * VF + 2 * GUARD,), 77.0, dtype=torch.float32, device=DEV)
    fused._bufs[("ws", S_, n)] = wsflat[GUARD:GUARD + keys]
    fused._bufs[("scores", S_)] = scflat[GUARD:GUARD + M * S_ * VF].view(M, S_, VF)

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat + [wsflat, scflat])
    shared, per = bool_masks(VF)
    words = packed(per[:S_].contiguous())
    targets = torch.tensor([3, 599, -1, 77, 300], dtype=torch.int32, device=DEV)
    live = [(i[0].clone(), i[1].clone()) if isinstance(i, tuple) else i.clone() for i in first]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = fused.shortlist(live, n, out=out, allow=words)
        rk = fused.rank(live, targets, out=rout, allow=words)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(a is b for a, b in zip(got, out)) and all(a is b for a, b in zip(rk, rout)) and guards_hold()
    stack = own_scores(tables, first)
    same_bits(fused._bufs[("scores", S_)], stack, "the stacked buffer")
    same_fields(got, fused_shortlist_reference(stack, wdev, n, "skip", allow=per[:S_].to(DEV)), "eager")
    same_ranks(rk, fused_rank_reference(stack, wdev, targets, "skip", allow=per[:S_].to(DEV)), "eager")
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fused.shortlist(live, n, out=out, allow=words)                         # (warm: the buffers of this shape exist)
        fused.rank(live, targets, out=rout, allow=words)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        fused.shortlist(live, n, out=out, allow=words)
        fused.rank(live, targets, out=rout, allow=words)
    for its, weights, mask in ((second, [0.5, 2.0, -1.0, 0.125], torch.flip(per[:S_], dims=(0, 1)).contiguous()),
                               (first, [1.0, 0.0, 0.0, -2.0], torch.zeros(S_, VF, dtype=torch.bool)),
                               (second, WEIGHTS[:M], per[:S_].contiguous())):
        for dst, src in zip(live, its):
            if isinstance(dst, tuple):
                dst[0].copy_(src[0]), dst[1].copy_(src[1])
            else:
                dst.copy_(src)
        wdev.copy_(torch.tensor(weights, dtype=torch.float32))
        words.copy_(packed(mask))
        for t in bufs:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        stack = own_scores(tables, its)
        same_fields(out, fused_shortlist_reference(stack, weights, n, "skip", allow=mask.to(DEV)), "replay")
        same_ranks(rout, fused_rank_reference(stack, weights, targets, "skip", allow=mask.to(DEV)), "replay")
        assert guards_hold()
    assert int(out.n.max()) > 0


# -- 6. the stages end to end ------------------------------------------------------------------------------------------------------------------

def test_a_fused_list_feeds_the_search_and_the_evaluation():
    """Two tables over the store's NV videos: the fused shortlist's ids go into Grounder.search(candidates=) unchanged and give the
    Hits of the same set passed as host lists' device twin; evaluate_shortlist(fused, batches) reads rank() by duck typing."""
    from drn_amd import FusedShortlister, Grounder, ShortlistRecall, Shortlister, evaluate_shortlist, fused_shortlist_reference, metrics, ops
    m, store, index, kw = world("plain")
    g = torch.Generator().manual_seed(12)
    vis = Shortlister(torch.randint(-4, 5, (NV, 16), generator=g).float().to(DEV).contiguous(), names=store.names)
    off = offsets_of([2, 0, 3, 1, 1, 4, 2])
    sub = Shortlister(torch.randint(-4, 5, (int(off[-1]), 32), generator=g).float().to(DEV, torch.bfloat16).contiguous(), names=store.names,
                      offsets=off)
    assert len(off) - 1 == NV
    fused = FusedShortlister([vis, sub], weights=[1.0, 0.5], missing="skip")
    vis.check(index)
    qv = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    qs = torch.randint(-4, 5, (S, 32), generator=g).float().to(DEV, torch.bfloat16)
    qv[1] = float("nan")                                                  # a sentence the visual table cannot score: subtitles alone
    ops.kernel_timer = []
    try:
        short = fused.shortlist([qv, qs], 4)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags == ["shortlist_scores", "shortlist_scores", "shortlist_fuse_topn"]
    stack = torch.stack([vis.scores(qv), sub.scores(qs)])
    same_fields(short, fused_shortlist_reference(stack, [1.0, 0.5], 4, "skip"))
    assert short.n.tolist() == [4, 4, 4] and 1 not in short.ids[1].tolist()  # (video 1 has no subtitles)
    tok, qlen = sentences(7)
    grounder = Grounder(m, top_k=5, **kw)
    got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=short.ids.clone()), "the ids as they are")
    assert int(got.n[0]) > 0 and set(got.video[0, :int(got.n[0])].tolist()) <= set(short.ids[0].tolist())
    names = [store.names[int(short.ids[s, 0])] for s in range(S)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec = evaluate_shortlist(fused, iter([(names, [qv, qs])]), topks=(1, 3))
    assert isinstance(rec, ShortlistRecall) and rec.n == S and rec.ranks.tolist() == [0, 0, 0] and rec.recall == metrics.recall_from_ranks(rec.ranks, [1, 3])
