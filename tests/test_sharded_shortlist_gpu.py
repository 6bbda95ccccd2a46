"""Sharded shortlist tables on the device: drn_shortlist_merge_lists against merge_shortlists_reference on hand-built lists (more lists
than are kept in flight, every width edge, ties across shards, empty lists, a staging half that folds twice, junk past the counts, rows
carried and absent, outputs inside guard bands), drn_allow_slices against slice_allow_reference, and ShardedShortlister against ONE
Shortlister over the same rows, bit for bit in every field: plain, ragged, late, mixed FP8 / plain shards, masks, append, out=, one
captured graph, and its ids as Grounder.search's device candidates.
tests/test_sharded_shortlist_cpu.py holds the definitions, the refusals and the C boundary."""
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_late_shortlist_gpu import lengths_of, random_case, tokens_for
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import LAYOUTS, exact_case, offsets_of
from test_shortlist_gpu import exact_data, world

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
V = 775
CUTS = ([0, V], [0, 321, V], [0, 1, 64, 321, V])                             # 1 / 2 / 4 shards, a shard of one video among them
GUARD = 64
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def same(got, want, what=""):
    assert type(got) is type(want), what
    for f in want._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


def guarded(shape, dtype):
    """-> (a contiguous view of `shape` in the middle of a buffer of sentinels, the buffer)."""
    flat = torch.full((int(np.prod(shape)) + 2 * GUARD,), 77, dtype=dtype, device=DEV)
    return flat[GUARD:flat.numel() - GUARD].view(shape), flat


def guards_hold(flats):
    return all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flats)


# -- 1. the merge alone ------------------------------------------------------------------------------------------------------------------------

def run_merge(parts, bases, n, what):
    """Host lists of one width -> ops.shortlist_merge_lists on their stack, junk written past every count, outputs inside guard bands,
    against merge_shortlists_reference of the SAME host lists; with rows when the parts have them."""
    from drn_amd import SegmentShortlist, Shortlist, merge_shortlists_reference, ops
    ragged = len(parts[0]) == 4
    stack = [torch.stack([p[i] for p in parts]).clone() for i in range(len(parts[0]))]
    n_in = int(stack[0].shape[2])
    past = torch.arange(n_in)[None, None, :] >= stack[2].clamp(max=n_in)[:, :, None]
    junk_ids = torch.tensor([INT_MAX, INT_MIN, 0, 5], dtype=torch.int32)[torch.arange(n_in) % 4].expand_as(stack[0])
    junk_scores = torch.tensor([float("nan"), 1e30, float("inf"), 9.0])[(torch.arange(n_in) // 2) % 4].expand_as(stack[1])
    stack[0], stack[1] = torch.where(past, junk_ids, stack[0]), torch.where(past, junk_scores, stack[1])
    dirty = [type(parts[0])(*(t[k] for t in stack)) for k in range(len(parts))]
    want = merge_shortlists_reference(dirty, bases, n)
    same(want, merge_shortlists_reference(parts, bases, n), (what, "the reference ignores the junk"))
    S_ = int(stack[0].shape[1])
    outs, flats = zip(*(guarded(sh, dt) for sh, dt in (((S_, n), torch.int32), ((S_, n), torch.float32), ((S_,), torch.int32), ((S_, n), torch.int32))))
    dev = [t.to(DEV).contiguous() for t in stack]
    dbases = torch.tensor(bases, dtype=torch.int32, device=DEV)
    if ragged:
        got = SegmentShortlist(*ops.shortlist_merge_lists(dev[0], dev[1], dev[2], dev[3], dbases, n, outs[0], outs[1], outs[2], rows=outs[3]))
    else:
        got = Shortlist(*ops.shortlist_merge_lists(dev[0], dev[1], dev[2], None, dbases, n, outs[0], outs[1], outs[2]))
        assert bool((flats[3] == 77).all())                                   # rows absent: nothing of that buffer is touched
    assert guards_hold(flats), what
    same(type(want)(*(t.cpu() for t in got)), want, what)
    return want


def scored_parts(sizes, n_in, S_=3, seed=0, ragged=False):
    """Per-shard reference lists of width n_in over small integer scores (E = 4, values in [-2, 2]: ties everywhere, across shards
    too); with ragged, every entry gets a row number that depends on its shard and id."""
    from drn_amd import SegmentShortlist, shortlist_reference
    bases = [0] + np.cumsum(sizes).tolist()
    g = torch.Generator().manual_seed(seed + len(sizes))
    emb = torch.randint(-2, 3, (bases[-1], 4), generator=g).float()
    q = torch.randint(-2, 3, (S_, 4), generator=g).float()
    parts = [shortlist_reference(emb[a:b], q, n_in) for a, b in zip(bases[:-1], bases[1:])]
    if ragged:
        parts = [SegmentShortlist(*p, torch.where(p.ids >= 0, (p.ids * 7 + k) % 11, p.ids)) for k, p in enumerate(parts)]
    return parts, bases


@pytest.mark.parametrize("K", [1, 2, 3, 9, 64])
def test_the_merge_equals_its_reference_at_every_width(K):
    """K = 9 is more lists than are kept in flight, 64 the cap; shards of 1, 130, 37, 200 and 5 videos; n_in = n = 1, 5, 64, 65, 128, a
    wide input cut short (128 -> 5) and a narrow one padded (5 -> 16); with rows and without."""
    sizes = [(1, 130, 37, 200, 5)[k % 5] for k in range(K)]
    for n_in, n in ((1, 1), (5, 5), (64, 64), (65, 65), (128, 128), (128, 5), (5, 16)):
        for ragged in (False, True):
            parts, bases = scored_parts(sizes, n_in, ragged=ragged)
            want = run_merge(parts, bases, n, (K, n_in, n, ragged))
            assert want.n.tolist() == [min(n, sum(min(n_in, v) for v in sizes))] * 3
    if K == 2:                                                               # the narrow lists leave padding: 1 + 5 entries in 16 places
        assert want.n.tolist() == [6] * 3 and want.ids[0, 6:].tolist() == [-1] * 10 and want.rows[0, 6:].tolist() == [-1] * 10


def test_the_merge_on_hand_built_lists():
    """A tie between the last entry of shard 0 and the first of shard 1 (the lower corpus position wins); a shard whose list is empty
    for some sentences; a shard of one video; ids out of range inside a count, which never become positions."""
    from drn_amd import SegmentShortlist, Shortlist
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    a = Shortlist(i32([[2, 0, -1], [1, -1, -1]]), torch.tensor([[5., 3., 0.], [2., 0., 0.]]), i32([2, 1]))
    b = Shortlist(i32([[1, 3, 0], [-1, -1, -1]]), torch.tensor([[3., 3., 1.], [0., 0., 0.]]), i32([3, 0]))      # nothing for sentence 1
    c = Shortlist(i32([[0, -1, -1], [0, -1, -1]]), torch.tensor([[3., 0., 0.], [2., 0., 0.]]), i32([1, 1]))     # one video
    want = run_merge([a, b, c], [0, 3, 7, 8], 8, "hand")
    assert want.ids.tolist() == [[2, 0, 4, 6, 7, 3, -1, -1], [1, 7, -1, -1, -1, -1, -1, -1]] and want.n.tolist() == [6, 2]
    assert want.scores[0].tolist() == [5., 3., 3., 3., 3., 1., 0., 0.]
    assert run_merge([a, b, c], [0, 3, 7, 8], 2, "hand, cut inside the tie").ids.tolist() == [[2, 0], [1, 7]]
    # inside the count: an id equal to the shard's size, a negative one and INT_MAX are no candidates; so is a score that is not finite
    d = Shortlist(i32([[3, 1, -5], [INT_MAX, 2, 0]]), torch.tensor([[9., 4., 8.], [7., float("inf"), 1.]]), i32([3, 3]))
    want = run_merge([d, b], [0, 3, 7], 4, "out of range")
    assert want.ids.tolist() == [[1, 4, 6, 3], [0, -1, -1, -1]] and want.n.tolist() == [4, 1]
    rows = lambda p, r: SegmentShortlist(*p, i32(r))
    want = run_merge([rows(a, [[10, 11, -1], [12, -1, -1]]), rows(b, [[20, 21, 22], [-1, -1, -1]]), rows(c, [[30, -1, -1], [31, -1, -1]])],
                     [0, 3, 7, 8], 5, "hand, rows")
    assert want.rows.tolist() == [[10, 11, 20, 21, 30], [12, 31, -1, -1, -1]]


def test_rising_scores_stage_every_list_and_fold_the_staging_half_twice():
    """Three shards of 130 videos at n = 128 whose scores grow with the corpus position: every key of every list lies above the n-th
    best so far, so each list is staged whole and the staging half overflows and folds before the second and the third."""
    from drn_amd import SegmentShortlist
    ids = torch.arange(129, 1, -1, dtype=torch.int32)[None].expand(2, 128).contiguous()
    parts = [SegmentShortlist(ids, (130.0 * k + ids).float(), torch.full((2,), 128, dtype=torch.int32), 129 - ids) for k in range(3)]
    want = run_merge(parts, [0, 130, 260, 390], 128, "rising")
    assert want.ids[0].tolist() == list(range(389, 261, -1)) and want.rows[1].tolist() == list(range(128))
    falling = [SegmentShortlist(p.ids, -p.scores, p.n, p.rows) for p in parts]
    falling = [SegmentShortlist(p.ids.flip(1).contiguous() - 2, p.scores.flip(1).contiguous(), p.n, p.rows.flip(1).contiguous()) for p in falling]
    want = run_merge(falling, [0, 130, 260, 390], 128, "falling: only the first list is staged")
    assert want.ids[0].tolist() == list(range(128))


# -- 2. mask slices ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [0, 1, 17], ids=["shared", "one-row", "S17"])
def test_mask_slices_equal_the_reference_inside_guard_bands(rows):
    """V = 775 at the bases 0 / 1 / 64 / 321, at multiples of 32 and as one piece; a shared (W,) mask, one row and 17 rows; bits at or
    past V set in the input never reach a piece; every word of every piece is compared and the buffer lies inside guard bands."""
    from drn_amd import ops, pack_allow, pack_allow_reference, slice_allow_reference
    g = torch.Generator().manual_seed(rows)
    mask = torch.rand((V,) if rows == 0 else (rows, V), generator=g) < 0.5
    words = pack_allow(mask.to(DEV))
    assert np.array_equal(words.cpu().numpy(), pack_allow_reference(mask))
    stuffed = words.clone()
    stuffed[..., -1] |= -1 << (V % 32)
    nrows = max(rows, 1)
    for bases in ([0, 1, 64, 321, V], [0, 32, 64, 320, V], [0, V], [0, 31, 33, 96, 97, 774, V]):
        total = ops.allow_slice_words(bases)
        dbases = torch.tensor(bases, dtype=torch.int32, device=DEV)
        for w in (words, stuffed):
            out, flat = guarded((nrows * total,), torch.int32)
            assert ops.allow_slices(w, dbases, bases, out) is out and guards_hold([flat])
            host, at = out.cpu().numpy(), 0
            for a, b in zip(bases[:-1], bases[1:]):
                Wk = -(-(b - a) // 32)
                piece = host[at:at + nrows * Wk].reshape((Wk,) if rows == 0 else (nrows, Wk))
                assert np.array_equal(piece, slice_allow_reference(words.cpu(), V, a, b)), (bases, a, b)
                assert np.array_equal(piece, pack_allow_reference(mask[..., a:b])), (bases, a, b)
                at += nrows * Wk
            assert at == nrows * total


# -- 3. sharded = whole, bit for bit, every field ----------------------------------------------------------------------------------------------

def shards_of(emb, bases, offsets=None, quantize=None):
    """Shortlisters over CLONED slices of the table (a row slice is generally not 16-byte aligned); bases count videos."""
    from drn_amd import Shortlister
    out = []
    for a, b in zip(bases[:-1], bases[1:]):
        if offsets is None:
            out.append(Shortlister(emb[a:b].clone(), quantize=quantize))
        else:
            out.append(Shortlister(emb[int(offsets[a]):int(offsets[b])].clone(), offsets=offsets[a:b + 1] - offsets[a], quantize=quantize))
    return out


@DTYPES
@pytest.mark.parametrize("E", [8, 40, 512])
def test_a_sharded_plain_table_is_the_whole_table(dtype, E):
    from drn_amd import ShardedShortlister, Shortlist, Shortlister
    emb, q17 = exact_data(V, E, 17, dtype)
    whole = Shortlister(emb)
    want = {(S_, n): whole.shortlist(q17[:S_].contiguous(), n) for S_ in (1, 17) for n in (1, 5, 128)}
    assert bool((want[(17, 128)].scores[:, 1:] == want[(17, 128)].scores[:, :-1]).any())      # ties in the data
    for bases in CUTS:
        sh = ShardedShortlister(shards_of(emb, bases))
        assert len(sh) == V and sh.bases == bases and sh.bases_device.tolist() == bases and sh.nbytes == whole.nbytes
        for (S_, n), w in want.items():
            got = sh.shortlist(q17[:S_].contiguous(), n)
            assert isinstance(got, Shortlist)
            same(got, w, (bases, S_, n))


@DTYPES
def test_a_sharded_ragged_table_is_the_whole_table_rows_included(dtype):
    """Layouts cut on video boundaries: next to a video without rows ("cycle" at 3 and 70, "long" at 4, "straddle" at 2), a shard whose
    last video is empty, a shard of one video ("target" 4 .. 5)."""
    from drn_amd import SegmentShortlist, ShardedShortlister, Shortlister
    for layout, bases in (("cycle", [0, 3, 70, 120]), ("straddle", [0, 2, 4]), ("long", [0, 4, 7]), ("target", [0, 2, 4, 5, 7]), ("ones257", [0, 256, 257])):
        emb, q17, off = exact_case(layout, 40, dtype)
        assert bases[-1] == len(LAYOUTS[layout])
        whole = Shortlister(emb, offsets=off)
        sh = ShardedShortlister(shards_of(emb, bases, off))
        for S_ in (1, 17):
            for n in (1, 5, 128):
                got = sh.shortlist(q17[:S_].contiguous(), n)
                assert isinstance(got, SegmentShortlist)
                same(got, whole.shortlist(q17[:S_].contiguous(), n), (layout, S_, n))


@DTYPES
def test_a_sharded_late_shortlist_is_the_whole_table(dtype):
    """L = 3 tokens, lengths 3, 0, 1 and values the device clamps, on "cycle" and "long"."""
    from drn_amd import ShardedShortlister, Shortlist, Shortlister
    for layout, bases in (("cycle", [0, 3, 70, 120]), ("long", [0, 4, 7])):
        emb, tok, off = tokens_for(layout, 40, dtype)
        q, lengths = tok[:, :3].contiguous(), lengths_of(3)
        assert 0 in lengths.tolist()
        whole = Shortlister(emb, offsets=off)
        sh = ShardedShortlister(shards_of(emb, bases, off))
        for n in (1, 5, 128):
            got = sh.shortlist_late(q, lengths, n)
            assert isinstance(got, Shortlist)
            same(got, whole.shortlist_late(q, lengths, n), (layout, n))
            assert int(got.n[1]) == 0 and int(got.n[0]) > 0


@DTYPES
def test_a_quantised_shard_beside_a_plain_one_is_the_plain_table_over_the_dequantised_rows(dtype):
    """Random data, where nothing is exact: one quantize="mxfp8" shard, one plain -- a plain table and a ragged one -- against ONE plain
    Shortlister over the concatenation of dequantized() rows."""
    from drn_amd import ShardedShortlister, Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    off = offsets_of(lens)
    emb, tok = random_case(int(off[-1]), 64, dtype, 21)
    q = tok[:, 0].contiguous()
    cold, hot = Shortlister(emb[:300].clone(), quantize="mxfp8"), Shortlister(emb[300:].clone())
    assert cold.quantize == "mxfp8" and hot.quantize is None and len(cold) + len(hot) == int(off[-1])
    sh = ShardedShortlister([cold, hot])
    whole = Shortlister(torch.cat([cold.dequantized().embeddings, hot.embeddings]).contiguous())
    assert sh.nbytes == cold.nbytes + hot.nbytes < whole.nbytes
    for n in (5, 128):
        same(sh.shortlist(q, n), whole.shortlist(q, n), ("plain", n))
    cut = 41                                                                  # videos; rows off[41]
    cold = Shortlister(emb[:int(off[cut])].clone(), offsets=off[:cut + 1], quantize="mxfp8")
    hot = Shortlister(emb[int(off[cut]):].clone(), offsets=off[cut:] - off[cut])
    sh = ShardedShortlister([cold, hot])
    whole = Shortlister(torch.cat([cold.dequantized().embeddings, hot.embeddings]).contiguous(), offsets=off)
    lengths = lengths_of(5)
    for n in (5, 128):
        same(sh.shortlist(q, n), whole.shortlist(q, n), ("ragged", n))
        same(sh.shortlist_late(tok[:, :5].contiguous(), lengths, n), whole.shortlist_late(tok[:, :5].contiguous(), lengths, n), ("late", n))


# -- 4. masks, append, out=, graph ---------------------------------------------------------------------------------------------------------------

@DTYPES
def test_a_mask_over_the_corpus_is_the_single_tables_mask(dtype):
    """A shared (W,) mask and one row per sentence, with a shard wholly masked (for every sentence; for one sentence), on a plain and a
    ragged table, shortlist and shortlist_late; allow_of's mask over corpus positions."""
    from drn_amd import ShardedShortlister, Shortlister, pack_allow
    emb, q17 = exact_data(V, 40, 17, dtype)
    whole, sh = Shortlister(emb), ShardedShortlister(shards_of(emb, CUTS[2]))
    g = torch.Generator().manual_seed(6)
    shared = torch.rand((V,), generator=g) < 0.5
    shared[1:64] = False                                                      # shard 1 wholly masked
    per = torch.rand((17, V), generator=g) < 0.5
    per[3, 64:321], per[5] = False, False
    for mask in (shared, per):
        words = pack_allow(mask.to(DEV))
        for n in (5, 128):
            got = sh.shortlist(q17, n, allow=words)
            same(got, whole.shortlist(q17, n, allow=words), (tuple(mask.shape), n))
        assert not bool(((got.ids >= 1) & (got.ids < 64)).any()) or mask.dim() == 2
    assert int(got.n[5]) == 0
    drop = [0, 1, 63, 64, 320, 321, 774]
    same(sh.shortlist(q17, 128, allow=sh.allow_of(drop=drop)), whole.shortlist(q17, 128, allow=whole.allow_of(drop=drop)), "allow_of")
    emb, tok, off = tokens_for("cycle", 40, dtype)
    q, lengths = tok[:, :3].contiguous(), lengths_of(3)
    whole, sh = Shortlister(emb, offsets=off), ShardedShortlister(shards_of(emb, [0, 3, 70, 120], off))
    shared = torch.rand((120,), generator=g) < 0.5
    shared[:3] = False
    per = torch.rand((17, 120), generator=g) < 0.5
    per[0, 3:70] = False
    for mask in (shared, per):
        words = pack_allow(mask.to(DEV))
        same(sh.shortlist(tok[:, 0].contiguous(), 128, allow=words), whole.shortlist(tok[:, 0].contiguous(), 128, allow=words), "ragged")
        same(sh.shortlist_late(q, lengths, 128, allow=words), whole.shortlist_late(q, lengths, 128, allow=words), "late")


def test_append_after_a_first_call_gives_the_bits_of_a_fresh_object():
    from drn_amd import ShardedShortlister, Shortlister, _lib
    emb, q17 = exact_data(V, 40, 17, torch.bfloat16)
    parts = shards_of(emb, CUTS[2])
    sh = ShardedShortlister(parts[:2])
    first = sh.shortlist(q17, 128)
    same(first, Shortlister(emb[:64].contiguous()).shortlist(q17, 128), "before")
    assert (2, 17, 128) in sh._bufs
    resident = [p.embeddings.data_ptr() for p in parts[:2]]
    assert sh.append(parts[2]).append(parts[3]) is sh and sh._bufs == {} and sh.bases == CUTS[2] and sh.bases_device.tolist() == CUTS[2]
    assert [p.embeddings.data_ptr() for p in sh.shards[:2]] == resident      # kept by reference, not copied
    got = sh.shortlist(q17, 128)
    same(got, ShardedShortlister(parts).shortlist(q17, 128), "a fresh object")
    same(got, Shortlister(emb).shortlist(q17, 128), "the whole table")
    with pytest.raises(_lib.DrnError, match="shard 4 has E = 8 columns, the others 40"):
        sh.append(Shortlister(exact_data(5, 8, 1, torch.bfloat16)[0]))
    same(sh.shortlist(q17, 128), got, "a refused shard changes nothing")


def test_out_buffers_are_written_in_place():
    from drn_amd import SegmentShortlist, ShardedShortlister, Shortlist, Shortlister
    emb, q17, off = exact_case("cycle", 40, torch.bfloat16)
    q = q17[:5].contiguous()
    whole, sh = Shortlister(emb, offsets=off), ShardedShortlister(shards_of(emb, [0, 3, 70, 120], off))
    n = 100
    outs, flats = zip(*(guarded(sh_, dt) for sh_, dt in (((5, n), torch.int32), ((5, n), torch.float32), ((5,), torch.int32), ((5, n), torch.int32))))
    got = sh.shortlist(q, n, out=SegmentShortlist(*outs))
    assert all(a is b for a, b in zip(got, outs)) and guards_hold(flats)
    same(got, whole.shortlist(q, n), "every element")
    small = ShardedShortlister(shards_of(emb, [0, 1, 2], off))                # two videos: the tail past the list is written too
    for t in outs:
        t.fill_(77)
    same(small.shortlist(q, n, out=outs), Shortlister(emb[:4].contiguous(), offsets=off[:3]).shortlist(q, n), "the tail past the list")
    tok, lengths = tokens_for("cycle", 40, torch.bfloat16)[1][:5, :3].contiguous(), lengths_of(3, 5)
    for t in outs:
        t.fill_(77)
    got = sh.shortlist_late(tok, lengths, n, out=Shortlist(*outs[:3]))
    assert all(a is b for a, b in zip(got, outs)) and guards_hold(flats) and bool((outs[3] == 77).all())
    same(got, whole.shortlist_late(tok, lengths, n), "late")


def test_one_captured_graph_of_three_shards_replays_after_queries_and_mask_change_in_place():
    from drn_amd import ShardedShortlister, Shortlist, Shortlister, pack_allow
    from drn_amd.graph import capture_graph
    emb, q17 = exact_data(V, 40, 17, torch.bfloat16)
    _, other = exact_data(V, 40, 17, torch.bfloat16, seed=7)
    whole, sh = Shortlister(emb), ShardedShortlister(shards_of(emb, [0, 64, 321, V]))
    g = torch.Generator().manual_seed(2)
    mask, mask2 = (torch.rand((17, V), generator=g) < 0.5).to(DEV), (torch.rand((17, V), generator=g) < 0.5).to(DEV)
    mask2[:, 64:321] = False
    n = 16
    qbuf, words = q17.clone(), pack_allow(mask)
    out = Shortlist(torch.empty((17, n), dtype=torch.int32, device=DEV), torch.empty((17, n), dtype=torch.float32, device=DEV),
                    torch.empty((17,), dtype=torch.int32, device=DEV))
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sh.shortlist(qbuf, n, out=out, allow=words)                           # (warm: the buffers and workspaces of this shape exist)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sh.shortlist(qbuf, n, out=out, allow=words)
    for queries, m in ((other, mask2), (q17, mask)):
        qbuf.copy_(queries), pack_allow(m, out=words)
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        w = pack_allow(m)
        same(out, sh.shortlist(queries, n, allow=w), "replay == eager")
        same(out, whole.shortlist(queries, n, allow=w), "replay == the whole table")


# -- 5. the two stages ---------------------------------------------------------------------------------------------------------------------------

def test_sharded_ids_are_device_candidates_of_the_search():
    """search(candidates=sharded.ids) on a plain index == the same rows passed as host lists; between the queries and the Hits the host
    reads nothing (torch raises on a synchronising call meanwhile): each shard's entry, then ONE merge."""
    from drn_amd import Grounder, ShardedShortlister, Shortlister, ops
    m, store, index, kw = world("plain")
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (NV, 16), generator=g).float()
    emb[4] = emb[1]                                                           # a tie across the shards, broken by corpus position
    emb = emb.to(DEV).contiguous()
    sh = ShardedShortlister([Shortlister(emb[:3].clone(), names=store.names[:3]), Shortlister(emb[3:].clone(), names=store.names[3:])])
    sh.check(store), sh.check(index)
    qe = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    qe[1] = float("nan")                                                      # a sentence whose shortlist is empty: ids all -1
    grounder = Grounder(m, top_k=5, **kw)
    tok, qlen = sentences(7)
    n = 4
    sh.shortlist(qe, n), grounder.search(tok, qlen, index, per_video=2, candidates=sh.shortlist(qe, n).ids)     # (warm)
    torch.cuda.synchronize()
    ops.kernel_timer = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        short = sh.shortlist(qe, n)
        tags = [t[0] for t in ops.kernel_timer]
        got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    assert tags == ["shortlist_topn", "shortlist_topn", "shortlist_merge_lists"]
    same(short, Shortlister(emb).shortlist(qe, n), "the whole table")
    lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
    assert [len(l) for l in lists] == [n, 0, n]
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "two stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0
