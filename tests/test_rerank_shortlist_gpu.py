"""Reranking a candidate list on the device: drn_shortlist_rerank (Shortlister.rerank / rerank_late) against the rerank references on
exact data with planted ties (torch.equal on ids, scores and n), bit for bit against the full filtered shortlists on random data, what
an answer may depend on (not the list's order, padding, repeats, width, S or the other sentences), allow masks, block-scaled FP8 tables,
out= buffers and a workspace inside guard bands, the cascade coarse shortlist -> rerank_late in ONE captured graph with its ids as
Grounder.search's device candidates, and evaluate_cascade.
tests/test_rerank_shortlist_cpu.py holds the definition, the refusals and the C boundary."""
import functools
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_late_shortlist_gpu import exact_tokens, head, lengths_of, random_case, same_lists, tokens_for
from test_q8_shortlist_gpu import exact_tables
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import LAYOUTS, exact_case, offsets_of
from test_shortlist_gpu import world

pytestmark = pytest.mark.gpu
FIELDS = ("ids", "scores", "n")
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
RAGGED = ("cycle", "straddle", "long", "ones257", "one")
CUTS = ((17, 128), (3, 5), (1, 1))                                           # (S, n)


# -- the candidate lists: deterministic, per sentence, interleaved with padding; built once on the host and uploaded -------------------------

def _padded(rows):
    C = max(len(r) for r in rows)
    return torch.tensor([list(r) + [-1] * (C - len(r)) for r in rows], dtype=torch.int32).to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def cands(kind, layout, S_=17, C=None):
    """(S_, C) int32 on the device over LAYOUTS[layout].  "all": a shuffled permutation of range(V) with a -1 after every fifth entry;
    "sparse": every third video, shuffled, a -1 between entries; "dirty": C = 48 -- a repeat inside one group of 16 (slots 2 and 9), one
    across groups (slots 1 and 40), the ids -1, -7, V, V + 5 and 2^31 - 1 scattered in, a video without rows listed where the layout has
    one, and sentence 2's row all -1; "width": C random positions, one in seven a -1 (repeats wherever C > V)."""
    lens = LAYOUTS[layout]
    V = len(lens)
    g = torch.Generator().manual_seed(1000 * V + 7 * S_ + (C or 0) + len(kind))
    rows = []
    for s in range(S_):
        if kind == "all":
            row = []
            for i, v in enumerate(torch.randperm(V, generator=g).tolist()):
                row += [v, -1] if i % 5 == 4 else [v]
        elif kind == "sparse":
            third = torch.arange(V)[s % 3::3]
            row = []
            for v in third[torch.randperm(len(third), generator=g)].tolist():
                row += [v, -1]
        elif kind == "dirty":
            row = torch.randint(0, V, (48,), generator=g).tolist()
            row[9], row[40] = row[2], row[1]
            for at, v in zip((5, 12, 20, 33, 44), (-1, -7, V, V + 5, 2 ** 31 - 1)):
                row[at] = v
            if 0 in lens:
                row[7] = lens.index(0)
            if s == 2:
                row = [-1] * 48
        else:
            row = [-1 if x else v for v, x in zip(torch.randint(0, V, (C,), generator=g).tolist(),
                                                  (torch.randint(0, 7, (C,), generator=g) == 0).tolist())]
        rows.append(row)
    out = _padded(rows)
    assert out.shape[1] <= 1024 and (C is None or out.shape[1] == C)
    return out


def firsts(got, S_):
    return type(got)(*(getattr(got, f)[:S_] for f in FIELDS))


# -- 1. equality to the definition on exact data -----------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [8, 40, 512])
def test_rerank_equals_the_reference_exactly_on_plain_and_ragged_tables(dtype, E):
    """rerank on every layout as a ragged table (a video scores by its best row) and, where every video owns one row, as a plain
    table: the lists "all", "sparse" and "dirty", S = 17 / 3 / 1, n = 128 / 5 / 1: ids, scores and n equal to the float64 definition."""
    from drn_amd import Shortlist, Shortlister, rerank_reference, segment_rerank_reference
    for layout in RAGGED:
        emb, q17, off = exact_case(layout, E, dtype)
        tables = [(Shortlister(emb, offsets=off), lambda c, q, n: segment_rerank_reference(emb, off, c, q, n))]
        if set(LAYOUTS[layout]) == {1}:
            tables.append((Shortlister(emb), lambda c, q, n: rerank_reference(emb, c, q, n)))
        for sl, reference in tables:
            for kind in ("all", "sparse", "dirty"):
                c = cands(kind, layout)
                want = reference(c, q17, 128)
                if kind == "dirty":
                    assert int(want.n[2]) == 0                                # the row of -1 lists nothing
                for S_, n in CUTS:
                    got = sl.rerank(c[:S_].contiguous(), q17[:S_].contiguous(), n)
                    assert isinstance(got, Shortlist)
                    same_lists(got, head(want, S_, n), (layout, kind, S_, n))
            # n = None is min(C, 128)
            c = cands("dirty", layout)
            assert sl.rerank(c, q17).ids.shape == (17, 48) and sl.rerank(cands("all", layout), q17).ids.shape[1] == min(128, cands("all", layout).shape[1])


@DTYPES
@pytest.mark.parametrize("E", [8, 40, 512])
def test_rerank_late_equals_the_reference_exactly(dtype, E):
    """L = 1 / 5 / 16 / 17 / 64 with lengths mixing 0, 1, 16, 17 and L (and values the device clamps), on every layout and list."""
    from drn_amd import Shortlist, Shortlister, late_rerank_reference
    for layout in RAGGED:
        emb, tok, off = tokens_for(layout, E, dtype)
        sl = Shortlister(emb, offsets=off)
        for L in (1, 5, 16, 17, 64):
            q, lengths = tok[:, :L].contiguous(), lengths_of(L)
            for kind in ("all", "sparse", "dirty"):
                c = cands(kind, layout)
                want = late_rerank_reference(emb, off, c, q, lengths, 128)
                assert int(want.n[1]) == 0 and int(want.n[10]) == 0          # no live token
                assert int(want.n[0]) > 0 or layout == "one"
                for S_, n in CUTS:
                    got = sl.rerank_late(c[:S_].contiguous(), q[:S_].contiguous(), lengths[:S_].contiguous(), n)
                    assert isinstance(got, Shortlist)
                    same_lists(got, head(want, S_, n), (layout, L, kind, S_, n))


@DTYPES
def test_the_widths_at_the_group_edges_and_the_widest_list(dtype):
    """C = 1, 15, 16, 17, 33 and 257 on "cycle", C = 1024 on "ones257": the group of 16 slots half full, full, and one slot over."""
    from drn_amd import Shortlister, late_rerank_reference, segment_rerank_reference
    for layout, widths in (("cycle", (1, 15, 16, 17, 33, 257)), ("ones257", (1024,))):
        emb, tok, off = tokens_for(layout, 40, dtype)
        sl = Shortlister(emb, offsets=off)
        q, lengths = tok[:, :17].contiguous(), lengths_of(17)
        for C in widths:
            c = cands("width", layout, 17, C)
            for n in (5, 128):
                same_lists(sl.rerank(c, tok[:, 0].contiguous(), n), segment_rerank_reference(emb, off, c, tok[:, 0].contiguous(), n), (layout, C, n))
                same_lists(sl.rerank_late(c, q, lengths, n), late_rerank_reference(emb, off, c, q, lengths, n), (layout, C, n, "late"))


@DTYPES
def test_nan_in_dead_tokens_is_ignored_and_a_nan_query_row_lists_nothing(dtype):
    from drn_amd import Shortlister, late_rerank_reference, segment_rerank_reference
    emb, tok, off = tokens_for("cycle", 40, dtype)
    sl = Shortlister(emb, offsets=off)
    c = cands("all", "cycle")
    L = 17
    q, lengths = tok[:, :L].contiguous(), lengths_of(L)
    clean = sl.rerank_late(c, q, lengths, 128)
    dead = q.clone()
    for s, k in enumerate(lengths.clamp(0, L).tolist()):
        dead[s, k:] = float("nan")
    same_lists(sl.rerank_late(c, dead, lengths, 128), clean, "NaN in dead tokens")
    same_lists(clean, late_rerank_reference(emb, off, c, dead, lengths, 128), "the reference ignores them too")
    live = q.clone()
    live[0, 3, 5] = float("nan")                                             # a live token of sentence 0 (17 live)
    got = sl.rerank_late(c, live, lengths, 128)
    assert int(got.n[0]) == 0 and bool((got.ids[0] == -1).all()) and bool((got.scores[0] == 0).all())
    same_lists(got, late_rerank_reference(emb, off, c, live, lengths, 128), "a NaN token")
    q1 = tok[:, 0].clone()
    q1[4, 0] = float("nan")
    got = sl.rerank(c, q1, 128)
    assert int(got.n[4]) == 0 and int(got.n[3]) > 0
    same_lists(got, segment_rerank_reference(emb, off, c, q1, 128), "a NaN query row")


# -- 2. bit equality to the full filtered shortlists on random data -----------------------------------------------------------------------------

RANDOM_LENS = [1, 3, 0, 17] * 20 + [300, 2]                                  # V = 82, R = 722: several groups, a video across passes


@functools.lru_cache(maxsize=None)
def random_lists(V, S_=17, seed=5):
    """Per sentence 40 distinct random positions, a repeat and padding between them: C = 64."""
    g = torch.Generator().manual_seed(seed + V)
    rows = []
    for s in range(S_):
        keep = torch.randperm(V, generator=g)[:40].tolist()
        row = []
        for i, v in enumerate(keep):
            row += [v, -1] if i % 2 else [v]
        rows.append(row + [keep[3], keep[0], V, -1])
    return _padded(rows)


@DTYPES
@pytest.mark.parametrize("E", [512, 40])
def test_rerank_is_bit_for_bit_the_full_filtered_shortlist_on_random_data(dtype, E):
    """Non-exact sums.  rerank == shortlist(allow=pack_allow(candidates_mask)) without rows on a plain and a ragged table, rerank_late ==
    shortlist_late(allow=...), rerank(shortlist(q, n).ids, q, n) == shortlist(q, n), and rerank_late with one token == rerank.  The
    error of those scores against float64 is bounded by the tests of the full shortlists: no new tolerance here."""
    from drn_amd import Shortlister, candidates_mask, pack_allow
    V = len(RANDOM_LENS)
    emb, tok = random_case(int(sum(RANDOM_LENS)), E, dtype, 90 + E)
    ragged, plain = Shortlister(emb, offsets=offsets_of(RANDOM_LENS)), Shortlister(emb[:300].contiguous())
    q = tok[:, 0].contiguous()
    ones = torch.ones(17, dtype=torch.int32, device=DEV)
    for sl in (ragged, plain):
        c = random_lists(len(sl))
        words = pack_allow(candidates_mask(c, len(sl)))
        for n in (1, 16, 128):
            want = sl.shortlist(q, n, allow=words)
            got = sl.rerank(c, q, n)
            same_lists(got, want, (len(sl), n))
            assert int(got.n[0]) == min(n, int(want.n[0])) > 0
            full = sl.shortlist(q, n)
            same_lists(sl.rerank(full.ids, q, n), full, (len(sl), n, "its own list"))
            same_lists(sl.rerank(full.ids.flip(1).contiguous(), q), full, (len(sl), n, "its own list, reversed, n = None"))
    c = random_lists(V)
    words = pack_allow(candidates_mask(c, V))
    for L in (5, 17, 33):
        tq, lengths = tok[:, :L].contiguous(), lengths_of(L)
        for n in (16, 128):
            same_lists(ragged.rerank_late(c, tq, lengths, n), ragged.shortlist_late(tq, lengths, n, allow=words), (L, n))
    for n in (1, 128):
        same_lists(ragged.rerank_late(c, tok[:, :1].contiguous(), ones, n), ragged.rerank(c, q, n), (n, "one token"))
        same_lists(ragged.rerank_late(c, tok[:, :7].contiguous(), ones, n), ragged.rerank(c, q, n), (n, "one token among padding"))


# -- 3. what an answer depends on ---------------------------------------------------------------------------------------------------------------

@DTYPES
def test_an_answer_depends_on_the_sentence_and_the_set_of_its_candidates_alone(dtype):
    """Shuffling each row, adding repeats and padding, widening C, running a sentence alone or changing the other sentences' lists
    changes no bit of a sentence's answer, on random data (late, L = 17) and on the planted ties of exact data."""
    from drn_amd import Shortlister
    V = len(RANDOM_LENS)
    emb, tok = random_case(int(sum(RANDOM_LENS)), 200, dtype, 61)
    sl = Shortlister(emb, offsets=offsets_of(RANDOM_LENS))
    q, lengths = tok[:, :17].contiguous(), lengths_of(17)
    c = random_lists(V)
    base = sl.rerank_late(c, q, lengths, 128)
    # every sentence with a live token lists the videos of its row that own rows: 40 distinct positions, some of them empty videos
    owning = [len({v for v in row if 0 <= v < V and RANDOM_LENS[v]}) for row in c.tolist()]
    assert base.n.tolist() == [k if t > 0 else 0 for k, t in zip(owning, lengths.tolist())] and 20 < owning[0] <= 40
    g = torch.Generator().manual_seed(2)
    host = c.cpu()
    shuffled = torch.stack([row[torch.randperm(len(row), generator=g)] for row in host]).to(DEV).contiguous()
    same_lists(sl.rerank_late(shuffled, q, lengths, 128), base, "shuffled")
    wide = torch.cat([torch.full((17, 9), -1, dtype=torch.int32), host.flip(1), host[:, :20], torch.full((17, 3), V + 1, dtype=torch.int32),
                      host], dim=1).to(DEV).contiguous()
    assert wide.shape[1] == 9 + 64 + 20 + 3 + 64
    same_lists(sl.rerank_late(wide, q, lengths, 128), base, "repeats, padding, a wider list")
    same_lists(sl.rerank_late(wide, q, lengths, 7), head(base, 17, 7), "a shorter cut")
    for s in (0, 2, 16):
        alone = sl.rerank_late(shuffled[s:s + 1].contiguous(), q[s:s + 1].contiguous(), lengths[s:s + 1].contiguous(), 128)
        for f in FIELDS:
            assert torch.equal(getattr(alone, f)[0], getattr(base, f)[s]), (s, f)
    others = c.clone()
    others[1:] = random_lists(V, seed=6)[1:]
    assert not torch.equal(others, c)
    got = sl.rerank_late(others, q, lengths, 128)
    for f in FIELDS:
        assert torch.equal(getattr(got, f)[0], getattr(base, f)[0]), f
    # planted ties: equal scores among candidates fall by store position, whatever their order in the list
    for layout in ("cycle", "ones257"):
        emb, q17, off = exact_case(layout, 40, dtype)
        sl = Shortlister(emb, offsets=off)
        c = cands("all", layout)
        up, down = sl.rerank(c, q17, 128), sl.rerank(c.flip(1).contiguous(), q17, 128)
        same_lists(down, up, (layout, "reversed"))
        ties = 0
        for s in range(17):
            k = int(up.n[s])
            sc, ids = up.scores[s, :k], up.ids[s, :k]
            same = sc[:-1] == sc[1:]
            ties += int(same.sum())
            assert bool(((sc[:-1] > sc[1:]) | (same & (ids[:-1] < ids[1:]))).all()), (layout, s)
        assert ties > 0


# -- 4. masks -----------------------------------------------------------------------------------------------------------------------------------

@DTYPES
def test_masks_combine_with_the_list(dtype):
    """allow=, shared and per sentence, is candidates_mask & allow: equal to the references on exact data; a listed but masked video is no
    candidate; bits at or past V are ignored."""
    from drn_amd import Shortlister, candidates_mask, late_rerank_reference, pack_allow, rerank_reference, segment_rerank_reference
    for layout in ("cycle", "long", "ones257"):
        emb, tok, off = tokens_for(layout, 40, dtype)
        V = len(off) - 1
        sl = Shortlister(emb, offsets=off)
        q, lengths, q1 = tok[:, :17].contiguous(), lengths_of(17), tok[:, 0].contiguous()
        g = torch.Generator().manual_seed(V)
        for kind in ("all", "dirty"):
            c = cands(kind, layout)
            for shape in ((V,), (17, V)):
                mask = (torch.rand(shape, generator=g) < 0.5).to(DEV)
                words = pack_allow(mask)
                for n in (5, 128):
                    got = sl.rerank_late(c, q, lengths, n, allow=words)
                    same_lists(got, late_rerank_reference(emb, off, c, q, lengths, n, allow=mask), (layout, kind, shape, n))
                    same_lists(sl.rerank(c, q1, n, allow=words), segment_rerank_reference(emb, off, c, q1, n, allow=mask), (layout, kind, shape, n))
                both = candidates_mask(c, V) & mask
                listed = torch.zeros((17, V + 1), dtype=torch.bool, device=DEV)
                listed.scatter_(1, torch.where(got.ids >= 0, got.ids.long(), torch.full_like(got.ids, V).long()), torch.ones_like(got.ids, dtype=torch.bool))
                assert not bool((listed[:, :V] & ~both).any())
        if layout == "ones257":
            plain = Shortlister(emb)
            mask = (torch.rand((17, V), generator=g) < 0.5).to(DEV)
            c = cands("dirty", layout)
            same_lists(plain.rerank(c, q1, 128, allow=pack_allow(mask)), rerank_reference(emb, c, q1, 128, allow=mask), "plain")
            ones = pack_allow(torch.ones(V, dtype=torch.bool, device=DEV))
            stuffed = ones.clone()
            stuffed[-1] = -1                                                 # (V = 257: the last word's bits 1 .. 31 lie past the table)
            assert int(stuffed[-1]) != int(ones[-1])
            bare = sl.rerank_late(c, q, lengths, 128)
            same_lists(sl.rerank_late(c, q, lengths, 128, allow=ones), bare, "all ones")
            same_lists(sl.rerank_late(c, q, lengths, 128, allow=stuffed), bare, "bits at or past V")
            same_lists(sl.rerank_late(c, q, lengths, 128, allow=stuffed.repeat(17, 1).contiguous()), bare, "per sentence")


# -- 5. block-scaled FP8 tables -------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [32, 96, 512])
def test_quantised_rerank_is_the_dequantised_one_and_the_reference(dtype, E):
    """from_mx8 on exact tables, ragged and plain: every field equals dequantized().rerank / rerank_late and the float64 definition over
    the dequantised table (exact_tables and exact_tokens say why every sum is exact); Shortlister(quantize="mxfp8") on a random table,
    where nothing is exact, still equals dequantized() bit for bit."""
    from drn_amd import Shortlister, late_rerank_reference, pack_allow, rerank_reference, segment_rerank_reference
    from drn_amd.index import mx8_dequantize
    for layout in ("cycle", "long", "ones257"):
        lens = LAYOUTS[layout]
        codes, scales, q17, off = exact_tables(tuple(lens), E)
        q17 = q17.to(DEV, dtype).contiguous()
        table = mx8_dequantize(codes, scales)
        sl = Shortlister.from_mx8(codes, scales, dtype, offsets=off)
        oracle = sl.dequantized()
        mask = torch.arange(len(lens), device=DEV) % 3 != 1
        for kind in ("all", "dirty"):
            c = cands(kind, layout)
            for n in (5, 128):
                got = sl.rerank(c, q17, n)
                same_lists(got, oracle.rerank(c, q17, n), (layout, kind, n))
                same_lists(got, segment_rerank_reference(table, off, c, q17, n), (layout, kind, n, "reference"))
                for L in (5, 16):
                    q, lengths = exact_tokens(E, dtype)[:, :L].contiguous(), lengths_of(L)
                    got = sl.rerank_late(c, q, lengths, n)
                    same_lists(got, oracle.rerank_late(c, q, lengths, n), (layout, kind, L, n))
                    same_lists(got, late_rerank_reference(table, off, c, q, lengths, n), (layout, kind, L, n, "reference"))
            same_lists(sl.rerank(c, q17, 128, allow=pack_allow(mask)), segment_rerank_reference(table, off, c, q17, 128, allow=mask), (layout, kind, "masked"))
        if layout == "ones257":
            plain = Shortlister.from_mx8(codes, scales, dtype)
            c = cands("dirty", layout)
            for n in (5, 128):
                got = plain.rerank(c, q17, n)
                same_lists(got, plain.dequantized().rerank(c, q17, n), ("plain", n))
                same_lists(got, rerank_reference(table, c, q17, n), ("plain", n, "reference"))
    g = torch.Generator().manual_seed(E)
    R = int(sum(RANDOM_LENS))
    emb = (torch.randn(R, E, generator=g) * torch.exp2(torch.randint(-3, 4, (R, E // 32), generator=g).float()).repeat_interleave(32, dim=1)).to(DEV, dtype)
    tok = torch.randn(17, 33, E, generator=g).to(DEV, dtype).contiguous()
    c = random_lists(len(RANDOM_LENS))
    sl = Shortlister(emb.contiguous(), offsets=offsets_of(RANDOM_LENS), quantize="mxfp8")
    same_lists(sl.rerank_late(c, tok, lengths_of(33), 128), sl.dequantized().rerank_late(c, tok, lengths_of(33), 128), "random, late")
    plain = Shortlister(emb[:300].contiguous(), quantize="mxfp8")
    c = random_lists(300)
    same_lists(plain.rerank(c, tok[:, 0].contiguous(), 128), plain.dequantized().rerank(c, tok[:, 0].contiguous(), 128), "random, plain")


# -- 6. buffers ---------------------------------------------------------------------------------------------------------------------------------

def test_out_buffers_and_the_workspace_stay_inside_their_guards():
    """out= written in place, every element; guard bands around the three outputs AND the workspace untouched; the whole call, masked
    and not, runs with torch's synchronisation check armed and is one tagged entry."""
    from drn_amd import Shortlist, Shortlister, late_rerank_reference, ops, pack_allow, segment_rerank_reference
    emb, tok, off = tokens_for("cycle", 40, torch.bfloat16)
    V = len(off) - 1
    sl = Shortlister(emb, offsets=off)
    S_, L, n, GUARD = 5, 17, 100, 64
    c = cands("dirty", "cycle")[:S_].contiguous()
    C = int(c.shape[1])
    q, lengths = tok[:S_, :L].contiguous(), torch.tensor([17, 0, 1, 16, 5], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(8)
    mask = (torch.rand((S_, V), generator=g) < 0.5).to(DEV)
    shapes = ((S_, n), (S_, n), (S_,))
    dtypes = (torch.int32, torch.float32, torch.int32)
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    out = Shortlist(*(f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes)))
    keys = ops.shortlist_rerank_ws_keys(C, S_, n)
    assert keys == S_ * 3 * 16
    wsflat = torch.full((keys + 2 * GUARD,), 77, dtype=torch.int64, device=DEV)
    sl._ws[("rerank", S_, C, n)] = wsflat[GUARD:GUARD + keys]

    def guards_hold():
        return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat + [wsflat])
    words = pack_allow(mask)
    ops.kernel_timer = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = sl.rerank_late(c, q, lengths, n, out=out, allow=words)
        bare = sl.rerank_late(c, q, lengths, n)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    assert tags == ["shortlist_rerank", "shortlist_rerank"]
    assert all(a is b for a, b in zip(got, out)) and guards_hold() and sl._ws[("rerank", S_, C, n)].data_ptr() == wsflat[GUARD:].data_ptr()
    assert bool((wsflat[GUARD:GUARD + keys] != 77).all())                   # every key of the workspace is written
    same_lists(out, late_rerank_reference(emb, off, c, q, lengths, n, allow=mask), "every element")
    same_lists(bare, late_rerank_reference(emb, off, c, q, lengths, n), "no mask")
    for t in out:
        t.fill_(77)
    same_lists(sl.rerank(c, q[:, 0].contiguous(), n, out=out), segment_rerank_reference(emb, off, c, q[:, 0].contiguous(), n), "rerank, the tail past the list")
    assert guards_hold()


# -- 7. the cascade in ONE captured graph --------------------------------------------------------------------------------------------------------

def test_the_cascade_is_one_captured_graph_and_its_ids_are_device_candidates_of_the_search():
    """coarse.shortlist(out=) on a quantised one-row-per-video table, then fine.rerank_late(coarse ids, out=) on a bf16 ragged table,
    captured together; replayed after queries, lengths and the mask were overwritten in place == the eager calls, field for field.  The
    reranked ids are then Grounder(graph=True).search's device candidates on a small index == the same rows as host lists."""
    from drn_amd import Grounder, Shortlist, Shortlister, late_rerank_reference, pack_allow
    from drn_amd.graph import capture_graph
    m, store, index, kw = world("plain")
    lens = [3, 1, 0, 17, 2, 5, 1]
    assert len(lens) == NV
    off = offsets_of(lens)
    g = torch.Generator().manual_seed(12)
    fine_emb = torch.randint(-4, 5, (int(off[-1]), 32), generator=g).float()
    fine_emb[off[4]:off[5]] = fine_emb[off[1]]                             # a tie between videos the rerank breaks by position
    fine_emb = fine_emb.to(DEV, torch.bfloat16).contiguous()
    coarse_emb = torch.randint(-4, 5, (NV, 32), generator=g).float().to(DEV, torch.bfloat16).contiguous()
    coarse = Shortlister(coarse_emb, names=store.names, quantize="mxfp8")
    fine = Shortlister(fine_emb, names=store.names, offsets=off)
    fine.check(store), fine.check(index)
    depth, n = 5, 4
    make = lambda: (torch.randint(-4, 5, (S, 32), generator=g).float().to(DEV, torch.bfloat16),
                    torch.randint(-4, 5, (S, 6, 32), generator=g).float().to(DEV, torch.bfloat16))
    (cq, fq), (cq2, fq2) = make(), make()
    lengths, lengths2 = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in ([6, 0, 3], [2, 6, 9]))
    mask, mask2 = (torch.tensor(x, dtype=torch.bool, device=DEV) for x in ([True] * NV, [True, False, True, True, True, True, False]))
    cbuf, fbuf, lbuf, words = cq.clone(), fq.clone(), lengths.clone(), pack_allow(mask)
    first = Shortlist(torch.empty((S, depth), dtype=torch.int32, device=DEV), torch.empty((S, depth), dtype=torch.float32, device=DEV),
                      torch.empty((S,), dtype=torch.int32, device=DEV))
    out = Shortlist(torch.empty((S, n), dtype=torch.int32, device=DEV), torch.empty((S, n), dtype=torch.float32, device=DEV),
                    torch.empty((S,), dtype=torch.int32, device=DEV))

    def cascade():
        coarse.shortlist(cbuf, depth, out=first, allow=words)
        fine.rerank_late(first.ids, fbuf, lbuf, n, out=out, allow=words)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        cascade()                                                         # (warm: the workspaces of these shapes exist)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        cascade()
    for a, b, c_, d in ((cq2, fq2, lengths2, mask2), (cq, fq, lengths, mask)):
        cbuf.copy_(a), fbuf.copy_(b), lbuf.copy_(c_), pack_allow(d, out=words)
        for t in tuple(first) + tuple(out):
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        w = pack_allow(d)
        eager_first = coarse.shortlist(a, depth, allow=w)
        same_lists(first, eager_first, "the coarse stage, replayed")
        same_lists(out, fine.rerank_late(eager_first.ids, b, c_, n, allow=w), "the cascade, replayed == eager")
        same_lists(out, late_rerank_reference(fine_emb, off, eager_first.ids, b, c_, n, allow=d), "== the definition")
    # the last replay holds (cq, fq, lengths, all allowed): sentence 1 has no live token, its ids are all -1
    short = Shortlist(*(t.clone() for t in out))
    lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
    assert [len(l) for l in lists] == [n, 0, n] and all(2 not in l for l in lists)
    grounder = Grounder(m, top_k=5, graph=True, **kw)
    tok, qlen = sentences(7)
    got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    same_hits(got, Grounder(m, top_k=5, **kw).search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "three stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0


# -- 8. evaluate_cascade --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [False, True], ids=["rerank", "rerank_late"])
def test_evaluate_cascade_ranks_are_the_full_ranks_under_the_coarse_mask_cut_at_depth(late):
    """ranks == fine.rank / rank_late(..., allow=pack_allow(candidates_mask(coarse ids))) clipped to -1 at depth, on two batches; the
    recalls are metrics.recall_from_ranks of them, a topk > depth saturating."""
    from drn_amd import ShortlistRecall, Shortlister, candidates_mask, evaluate_cascade, metrics, pack_allow
    lens = [1, 3, 0, 17] * 10 + [40, 2]
    V, off = len(lens), offsets_of(lens)
    names = ["v%d" % v for v in range(V)]
    emb, tok = random_case(int(sum(lens)), 96, torch.bfloat16, 70)
    g = torch.Generator().manual_seed(4)
    coarse_emb = torch.randn(V, 32, generator=g).to(DEV, torch.bfloat16).contiguous()
    coarse = Shortlister(coarse_emb, names=names, quantize="mxfp8")
    fine = Shortlister(emb, names=names, offsets=off)
    depth, topks = 12, (1, 5, 12, 100)
    batches = []
    for b, S_ in enumerate((17, 6)):
        cq = torch.randn(S_, 32, generator=g).to(DEV, torch.bfloat16).contiguous()
        targets = torch.randint(0, V, (S_,), generator=g).tolist()
        fq = tok[:S_, 8 * b:8 * b + 8].contiguous()
        batches.append(([names[t] for t in targets], cq, fq if late else fq[:, 0].contiguous(), lengths_of(8, S_).clamp(min=1)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = evaluate_cascade(coarse, fine, iter(batches), depth, topks=topks, late=late)
    assert isinstance(got, ShortlistRecall) and got.n == 23 and got.topks == list(topks)
    want = []
    for bnames, cq, fq, lengths in batches:
        words = pack_allow(candidates_mask(coarse.shortlist(cq, depth).ids, V))
        targets = torch.tensor([names.index(x) for x in bnames], dtype=torch.int32, device=DEV)
        r = fine.rank_late(fq, lengths, targets, allow=words).rank if late else fine.rank(fq, targets, allow=words).rank
        want.append(torch.where(r < depth, r, torch.full_like(r, -1)))
    want = torch.cat(want).cpu().numpy()
    assert got.ranks.dtype == np.int32 and np.array_equal(got.ranks, want)
    assert (want >= 0).any() and (want < 0).any()
    assert got.recall == metrics.recall_from_ranks(want, list(topks)) and got.recall[3] == got.recall[2]
    assert got.mrr == metrics.mrr_from_ranks(want) and got.median_rank == metrics.median_rank_from_ranks(want)
    empty = evaluate_cascade(coarse, fine, iter(()), depth)
    assert empty.n == 0 and empty.ranks.shape == (0,)
