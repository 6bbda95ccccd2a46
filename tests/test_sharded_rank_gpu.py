"""Rank and rerank over a sharded corpus on the device: drn_shard_positions against shard_positions_reference inside guard bands,
drn_shortlist_rank_thresholds and drn_shortlist_rank_reduce_shards on hand-built keys and counts, and ShardedShortlister.rank /
rank_late / rerank / rerank_late against ONE Shortlister over the same rows, torch.equal in every field: plain, ragged, late, a
quantised shard beside a plain one, masks, ties across the cuts with both twins as targets, the ends of every shard, K = 64, out=,
append, captured graphs, the launch tags of one call, and the two evaluators.  There is no tolerance anywhere in this file.
tests/test_sharded_rank_cpu.py holds the definitions, the refusals and the C boundary."""
import struct
import warnings

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_late_shortlist_gpu import lengths_of, random_case, tokens_for
from test_search_gpu import NV, S, same_hits, sentences
from test_segment_shortlist_gpu import LAYOUTS, exact_case, offsets_of
from test_sharded_shortlist_gpu import CUTS, INT_MAX, INT_MIN, V, guarded, guards_hold, same, shards_of
from test_shortlist_gpu import exact_data, world

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
# video cuts of the ragged layouts: next to a video without rows, a shard of one video, a shard that is one 600-row video's neighbour
RAGGED_CUTS = {"one": [0, 1], "ones": [0, 33, 70], "cycle": [0, 3, 70, 120], "straddle": [0, 2, 4], "long": [0, 4, 7], "ones257": [0, 256, 257],
               "target": [0, 2, 4, 5, 7]}
ONES = 0xffffffffffffffff


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def targets_for(bases, S_=17):
    """-1, V, INT_MIN, INT_MAX, the first and the last position of every shard, then positions striding through the corpus."""
    t = [-1, bases[-1], INT_MIN, INT_MAX]
    for a, b in zip(bases[:-1], bases[1:]):
        t += [a, b - 1]
    i = 0
    while len(t) < S_:
        t.append((5 * i + 2) % bases[-1])
        i += 1
    return i32(t[:S_])


def key_of(score, position):
    """sl_key of csrc/shortlist.h on the host, for a finite score."""
    b = struct.unpack("<I", struct.pack("<f", score + 0.0))[0]
    word = (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)
    return (word << 32) | (~position & 0xffffffff)


def u64(rows):
    """Python integers below 2^64 -> a torch.int64 tensor on the device that holds their bits."""
    return torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)).to(DEV)


def bits(t):
    return t.cpu().numpy().view(np.uint64).tolist()


# -- 1. the kernels alone ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [None, 5, 1024], ids=["targets", "C5", "C1024"])
def test_shard_positions_equal_the_reference_inside_guard_bands(C):
    """(S,) targets and (S, C) lists with -1, V, INT_MIN, INT_MAX and both ends of every shard among random positions; one shard, four
    (one of a single video) and 64 shards; every word compared."""
    from drn_amd import ops, shard_positions_reference
    g = torch.Generator().manual_seed(C or 1)
    for bases in ([0, V], [0, 1, 64, 321, V], list(range(0, 64 * 12, 12)) + [V]):
        shape = (23,) if C is None else (3, C)
        pos = torch.randint(-3, V + 3, shape, generator=g, dtype=torch.int32)
        edge = torch.tensor([-1, V, INT_MIN, INT_MAX] + [x for a, b in zip(bases[:-1], bases[1:]) for x in (a, b - 1)], dtype=torch.int32)
        edge = edge[:pos.numel()]                                             # (the four values outside first, then both ends of every shard)
        pos.view(-1)[:edge.numel()] = edge
        want = shard_positions_reference(pos, bases)
        out, flat = guarded((len(bases) - 1,) + shape, torch.int32)
        assert ops.shard_positions(pos.to(DEV), i32(bases), out) is out and guards_hold([flat])
        assert torch.equal(out.cpu(), want), (C, bases)
        assert int((want >= 0).sum()) == int(((pos >= 0) & (pos < V)).sum())    # a position inside the corpus lands in exactly one shard


def test_thresholds_on_hand_built_keys():
    """A target in the first, a middle and the last shard, in none, and -- what the host's bases rule out -- in two: the lowest wins."""
    from drn_amd import ops, rank_thresholds_reference
    a, b, c = key_of(3.0, 5), key_of(-2.5, 0), key_of(0.0, 700)
    keys = [[a, 0, 0, 0, 0], [0, b, 0, 0, b], [0, 0, c, 0, a]]
    dev = u64(keys)
    (thr, tflat), (key, kflat) = guarded((3, 5), torch.int64), guarded((5,), torch.int64)
    ops.shortlist_rank_thresholds(dev, thr, key)
    assert guards_hold([tflat, kflat])
    top = lambda k: (k >> 32) << 32
    assert bits(key) == [a, b, c, 0, b]
    assert bits(thr) == [[a, top(b) - 1, top(c) - 1, ONES, top(b) - 1], [top(a) | 0xffffffff, b, top(c) - 1, ONES, b],
                         [top(a) | 0xffffffff, top(b) | 0xffffffff, c, ONES, top(b) | 0xffffffff]]
    want_thr, want_key = rank_thresholds_reference(dev[:, :4].contiguous())
    assert torch.equal(thr[:, :4], want_thr) and torch.equal(key[:4], want_key)
    for K in (1, 64):                                                         # one shard; every lane a shard, the target in the last
        rows = [[0, 0]] * (K - 1) + [[a, 0]]
        thr, key = torch.empty((K, 2), dtype=torch.int64, device=DEV), torch.empty((2,), dtype=torch.int64, device=DEV)
        ops.shortlist_rank_thresholds(u64(rows), thr, key)
        want_thr, want_key = rank_thresholds_reference(u64(rows))
        assert torch.equal(thr, want_thr) and torch.equal(key, want_key) and bits(key) == [a, 0]
        assert bits(thr[:, 1]) == [ONES] * K and bits(thr[:, 0]) == [top(a) - 1] * (K - 1) + [a]


@pytest.mark.parametrize("blocks", [[1, 2, 1], [69, 1], [1] * 64], ids=["small", "70-blocks", "K64"])
def test_the_reduce_sums_the_regions_of_hand_built_counts(blocks):
    from drn_amd import ops
    S_, K = 5, len(blocks)
    off = [0] + np.cumsum(blocks).tolist()
    g = torch.Generator().manual_seed(K)
    regions = [torch.randint(0, 257, (S_, nb, 2), generator=g, dtype=torch.int32) for nb in blocks]
    cnt = torch.cat([r.reshape(-1) for r in regions]).contiguous().view(torch.int64).to(DEV)
    scores = [3.0, -0.0, -17.25, 1e-30]
    key = u64([key_of(x, 9) for x in scores] + [0])
    outs, flats = zip(*(guarded((S_,), dt) for dt in (torch.int32, torch.float32, torch.int32)))
    ops.shortlist_rank_reduce_shards(key, cnt, i32(off), off[-1], *outs)
    assert guards_hold(flats)
    above, total = sum(r[:, :, 0].sum(dim=1) for r in regions), sum(r[:, :, 1].sum(dim=1) for r in regions)
    assert outs[0].tolist() == above[:4].tolist() + [-1] and outs[2].tolist() == total.tolist()
    assert torch.equal(outs[1].cpu(), torch.tensor([3.0, 0.0, -17.25, 1e-30, 0.0]))


# -- 2. rank: sharded = whole, bit for bit, every field ------------------------------------------------------------------------------------------

@DTYPES
def test_a_sharded_rank_is_the_whole_tables_rank_on_a_plain_table(dtype):
    """V = 775 cut into 1 / 2 / 4 shards -- one of a single video, one of 454 videos (two counting blocks) -- with targets at both ends
    of every shard and outside the corpus; then the twins the data plants on either side of every cut, both of each pair as targets."""
    from drn_amd import ShardedShortlister, Shortlister, TargetRank
    for E in (8, 40):
        emb, q17 = exact_data(V, E, 17, dtype)
        whole = Shortlister(emb)
        twins = i32([1, 0, 70, 5, 387, 258, 256, 0, 774, 255, 63, 64, 320, 321, 1, 774, 256])
        assert all(torch.equal(emb[a], emb[b]) for a, b in ((1, 0), (70, 5), (387, 258), (256, 0), (774, 255)))
        for bases in CUTS:
            sh = ShardedShortlister(shards_of(emb, bases))
            for targets in (targets_for(bases), twins):
                for S_ in (1, 17):
                    got = sh.rank(q17[:S_].contiguous(), targets[:S_].contiguous())
                    assert isinstance(got, TargetRank)
                    same(got, whole.rank(q17[:S_].contiguous(), targets[:S_].contiguous()), (E, bases, S_))
                if targets is not twins:
                    assert got.rank[:4].tolist() == [-1] * 4 and bool((got.rank[4:] >= 0).all()) and got.total.tolist() == [V] * 17


@DTYPES
def test_a_sharded_rank_is_the_whole_tables_rank_on_every_ragged_layout(dtype):
    """Every layout: videos without rows as targets ("cycle" 2, "long" 3, "target" 0), a 600-row video (three passes) as a shard's
    first, 257 one-row videos cut at 256."""
    from drn_amd import ShardedShortlister, Shortlister
    for layout, bases in RAGGED_CUTS.items():
        emb, q17, off = exact_case(layout, 40, dtype)
        assert bases[-1] == len(LAYOUTS[layout])
        whole, sh = Shortlister(emb, offsets=off), ShardedShortlister(shards_of(emb, bases, off))
        targets = targets_for(bases)
        got = sh.rank(q17, targets)
        same(got, whole.rank(q17, targets), layout)
        rowless = [s for s, t in enumerate(targets.tolist()) if 0 <= t < bases[-1] and LAYOUTS[layout][t] == 0]
        assert all(int(got.rank[s]) == -1 for s in rowless) and (rowless or layout not in ("cycle", "long", "target"))


@DTYPES
@pytest.mark.parametrize("L", [3, 17])
def test_a_sharded_late_rank_is_the_whole_tables(dtype, L):
    """L = 17 is two token tiles; lengths hold 0, values the device clamps and a negative one."""
    from drn_amd import ShardedShortlister, Shortlister
    for layout in ("cycle", "long"):
        bases = RAGGED_CUTS[layout]
        emb, tok, off = tokens_for(layout, 40, dtype)
        q, lengths = tok[:, :L].contiguous(), lengths_of(L)
        assert 0 in lengths.tolist()
        whole, sh = Shortlister(emb, offsets=off), ShardedShortlister(shards_of(emb, bases, off))
        targets = targets_for(bases)
        targets[1] = bases[1]                                                 # (the sentence without a live token names a real video)
        got = sh.rank_late(q, lengths, targets)
        same(got, whole.rank_late(q, lengths, targets), (layout, L))
        assert int(got.rank[1]) == -1 and int(got.total[1]) == 0 and int(got.total[0]) > 0


@DTYPES
def test_a_quantised_shard_beside_a_plain_one_ranks_like_the_dequantised_concatenation(dtype):
    from drn_amd import ShardedShortlister, Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    off = offsets_of(lens)
    emb, tok = random_case(int(off[-1]), 64, dtype, 21)
    q = tok[:, 0].contiguous()
    cold, hot = Shortlister(emb[:300].clone(), quantize="mxfp8"), Shortlister(emb[300:].clone())
    sh = ShardedShortlister([cold, hot])
    whole = Shortlister(torch.cat([cold.dequantized().embeddings, hot.embeddings]).contiguous())
    targets = targets_for([0, 300, int(off[-1])])
    same(sh.rank(q, targets), whole.rank(q, targets), "plain")
    cut = 41
    cold = Shortlister(emb[:int(off[cut])].clone(), offsets=off[:cut + 1], quantize="mxfp8")
    hot = Shortlister(emb[int(off[cut]):].clone(), offsets=off[cut:] - off[cut])
    sh = ShardedShortlister([cold, hot])
    whole = Shortlister(torch.cat([cold.dequantized().embeddings, hot.embeddings]).contiguous(), offsets=off)
    targets, lengths = targets_for([0, cut, len(lens)]), lengths_of(5)
    same(sh.rank(q, targets), whole.rank(q, targets), "ragged")
    same(sh.rank_late(tok[:, :5].contiguous(), lengths, targets), whole.rank_late(tok[:, :5].contiguous(), lengths, targets), "late")
    cands = sh.shortlist(q, 40).ids
    same(sh.rerank(cands, q, 16), whole.rerank(cands, q, 16), "rerank")
    same(sh.rerank_late(cands, tok[:, :5].contiguous(), lengths), whole.rerank_late(cands, tok[:, :5].contiguous(), lengths), "rerank_late")


@DTYPES
def test_masks_over_the_corpus_shared_and_per_sentence_with_a_shard_wholly_masked(dtype):
    from drn_amd import ShardedShortlister, Shortlister, pack_allow
    emb, q17 = exact_data(V, 40, 17, dtype)
    whole, sh = Shortlister(emb), ShardedShortlister(shards_of(emb, CUTS[2]))
    g = torch.Generator().manual_seed(6)
    shared = torch.rand((V,), generator=g) < 0.5
    shared[1:64] = False                                                      # shard 1 wholly masked
    per = torch.rand((17, V), generator=g) < 0.5
    per[3, 64:321], per[5] = False, False
    targets = targets_for(CUTS[2])
    cands = torch.randint(-2, V + 2, (17, 37), generator=g, dtype=torch.int32).to(DEV)
    for mask in (shared, per):
        words = pack_allow(mask.to(DEV))
        got = sh.rank(q17, targets, allow=words)
        same(got, whole.rank(q17, targets, allow=words), tuple(mask.shape))
        same(sh.rerank(cands, q17, 16, allow=words), whole.rerank(cands, q17, 16, allow=words), ("rerank", tuple(mask.shape)))
    assert int(got.total[5]) == 0 and got.rank[5].item() == -1 and bool((got.rank >= 0).any())
    emb, tok, off = tokens_for("cycle", 40, dtype)
    bases = RAGGED_CUTS["cycle"]
    q, lengths = tok[:, :3].contiguous(), lengths_of(3)
    whole, sh = Shortlister(emb, offsets=off), ShardedShortlister(shards_of(emb, bases, off))
    shared = torch.rand((120,), generator=g) < 0.5
    shared[:3] = False
    per = torch.rand((17, 120), generator=g) < 0.5
    per[0, 3:70] = False
    targets = targets_for(bases)
    cands = torch.randint(-2, 122, (17, 37), generator=g, dtype=torch.int32).to(DEV)
    for mask in (shared, per):
        words = pack_allow(mask.to(DEV))
        same(sh.rank(tok[:, 0].contiguous(), targets, allow=words), whole.rank(tok[:, 0].contiguous(), targets, allow=words), "ragged")
        same(sh.rank_late(q, lengths, targets, allow=words), whole.rank_late(q, lengths, targets, allow=words), "late")
        same(sh.rerank_late(cands, q, lengths, 16, allow=words), whole.rerank_late(cands, q, lengths, 16, allow=words), "rerank_late")


def test_sixty_four_shards_rank_and_rerank_like_the_whole_table():
    from drn_amd import ShardedShortlister, Shortlister
    sizes = [(1, 130, 37, 200, 5)[k % 5] for k in range(64)]
    bases = [0] + np.cumsum(sizes).tolist()
    emb, q17 = exact_data(bases[-1], 8, 17, torch.float32)
    whole, sh = Shortlister(emb), ShardedShortlister(shards_of(emb, bases))
    g = torch.Generator().manual_seed(64)
    targets = torch.cat([i32([-1, bases[-1], 0, bases[-1] - 1, bases[63]]), torch.randint(0, bases[-1], (12,), generator=g, dtype=torch.int32).to(DEV)])
    same(sh.rank(q17, targets), whole.rank(q17, targets), "K = 64")
    cands = whole.shortlist(q17, 128).ids
    same(sh.rerank(cands, q17, 128), whole.rerank(cands, q17, 128), "K = 64, rerank")


def test_out_buffers_append_and_the_place_in_the_shortlist():
    """out= is written in place inside guard bands; append() drops the buffers and the same call then ranks over the longer corpus;
    rank[s] == k exactly when the sharded shortlist holds the target at place k."""
    from drn_amd import ShardedShortlister, Shortlister, TargetRank
    emb, q17 = exact_data(V, 40, 17, torch.bfloat16)
    parts = shards_of(emb, CUTS[2])
    sh = ShardedShortlister(parts[:2])
    targets = targets_for(CUTS[2])
    same(sh.rank(q17, targets), Shortlister(emb[:64].contiguous()).rank(q17, targets), "before")
    assert ("rank", 2, 17) in sh._bufs
    assert sh.append(parts[2]).append(parts[3]) is sh and sh._bufs == {} and sh.blk_off == [0, 1, 2, 4, 6] and sh.blk_off_device.tolist() == sh.blk_off
    whole = Shortlister(emb)
    outs, flats = zip(*(guarded((17,), dt) for dt in (torch.int32, torch.float32, torch.int32)))
    got = sh.rank(q17, targets, out=TargetRank(*outs))
    assert all(a is b for a, b in zip(got, outs)) and guards_hold(flats)
    same(got, whole.rank(q17, targets), "after append, out=")
    n = 128
    short = sh.shortlist(q17, n)
    listed = short.ids == targets[:, None]
    place = torch.where(listed.any(dim=1), listed.int().argmax(dim=1), torch.full((17,), -1, device=DEV)).to(torch.int32)
    inside = (got.rank >= 0) & (got.rank < n)
    assert bool(inside.any()) and torch.equal(torch.where(inside, got.rank, torch.full_like(got.rank, -1)), place)
    assert torch.equal(short.scores[listed], got.score[listed.any(dim=1)])
    # rerank with out=
    louts, lflats = zip(*(guarded(sh_, dt) for sh_, dt in (((17, 20), torch.int32), ((17, 20), torch.float32), ((17,), torch.int32))))
    got = sh.rerank(short.ids, q17, 20, out=louts)
    assert all(a is b for a, b in zip(got, louts)) and guards_hold(lflats)
    same(got, whole.rerank(short.ids, q17, 20), "rerank, out=")


# -- 3. rerank -----------------------------------------------------------------------------------------------------------------------------

@DTYPES
def test_a_sharded_rerank_is_the_whole_tables_rerank(dtype):
    """The sharded shortlist's own ids as they are; shuffled rows with repeats and junk; n = None, n < C and n > C; and rerank of a
    shortlist's ids gives the shortlist back."""
    from drn_amd import ShardedShortlister, Shortlist, Shortlister
    emb, q17 = exact_data(V, 40, 17, dtype)
    whole = Shortlister(emb)
    g = torch.Generator().manual_seed(8)
    junk = torch.randint(-3, V + 3, (17, 50), generator=g, dtype=torch.int32)
    junk[:, 7], junk[:, 8], junk[:, 9], junk[:, 10] = junk[:, 3], INT_MIN, INT_MAX, -1
    junk[:, 11:17] = torch.tensor([0, 1, 63, 64, 320, 321], dtype=torch.int32)  # both sides of every cut; 0 | 1 are twins
    junk = junk.to(DEV)
    for bases in CUTS:
        sh = ShardedShortlister(shards_of(emb, bases))
        short = sh.shortlist(q17, 24)
        for cands in (short.ids, junk):
            C = int(cands.shape[1])
            for n in (None, 5, C + 9):
                got = sh.rerank(cands, q17, n)
                assert isinstance(got, Shortlist) and got.ids.shape[1] == (C if n is None else n)
                same(got, whole.rerank(cands, q17, n), (bases, C, n))
        same(sh.rerank(short.ids, q17, 24), short, "rerank(shortlist) == shortlist")
    emb, tok, off = tokens_for("cycle", 40, dtype)
    bases = RAGGED_CUTS["cycle"]
    whole, sh = Shortlister(emb, offsets=off), ShardedShortlister(shards_of(emb, bases, off))
    q, tokens, lengths = tok[:, 0].contiguous(), tok[:, :17].contiguous(), lengths_of(17)
    short = sh.shortlist(q, 24)
    junk = torch.randint(-3, 123, (17, 50), generator=g, dtype=torch.int32).to(DEV)
    for cands in (short.ids, junk):
        for n in (None, 5, 70):
            same(sh.rerank(cands, q, n), whole.rerank(cands, q, n), ("ragged", n))
            same(sh.rerank_late(cands, tokens, lengths, n), whole.rerank_late(cands, tokens, lengths, n), ("late", n))
    same(sh.rerank(short.ids, q, 24), Shortlist(short.ids, short.scores, short.n), "ragged: the shortlist without its rows")
    late = sh.shortlist_late(tokens, lengths, 24)
    same(sh.rerank_late(late.ids, tokens, lengths, 24), late, "late: rerank(shortlist) == shortlist")


# -- 4. graphs, tags ---------------------------------------------------------------------------------------------------------------------------

def captured(call):
    from drn_amd.graph import capture_graph
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()                                                                # (warm: the buffers and workspaces of this shape exist)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        call()
    return graph


def test_captured_rank_and_rerank_replay_after_their_inputs_changed_in_place():
    from drn_amd import ShardedShortlister, Shortlist, Shortlister, TargetRank, pack_allow
    emb, q17 = exact_data(V, 40, 17, torch.bfloat16)
    _, other = exact_data(V, 40, 17, torch.bfloat16, seed=7)
    whole, sh = Shortlister(emb), ShardedShortlister(shards_of(emb, [0, 64, 321, V]))
    g = torch.Generator().manual_seed(2)
    mask, mask2 = (torch.rand((17, V), generator=g) < 0.5).to(DEV), (torch.rand((17, V), generator=g) < 0.5).to(DEV)
    mask2[:, 64:321] = False
    t1, t2 = targets_for([0, 64, 321, V]), torch.randint(0, V, (17,), generator=g, dtype=torch.int32).to(DEV)
    c1, c2 = (torch.randint(-2, V + 2, (17, 40), generator=g, dtype=torch.int32).to(DEV) for _ in range(2))
    qbuf, tbuf, cbuf, words = q17.clone(), t1.clone(), c1.clone(), pack_allow(mask)
    rout = TargetRank(torch.empty((17,), dtype=torch.int32, device=DEV), torch.empty((17,), dtype=torch.float32, device=DEV),
                      torch.empty((17,), dtype=torch.int32, device=DEV))
    n = 16
    lout = Shortlist(torch.empty((17, n), dtype=torch.int32, device=DEV), torch.empty((17, n), dtype=torch.float32, device=DEV),
                     torch.empty((17,), dtype=torch.int32, device=DEV))
    rank_graph = captured(lambda: sh.rank(qbuf, tbuf, out=rout, allow=words))
    rerank_graph = captured(lambda: sh.rerank(cbuf, qbuf, n, out=lout, allow=words))
    for queries, targets, cands, m in ((other, t2, c2, mask2), (q17, t1, c1, mask)):
        qbuf.copy_(queries), tbuf.copy_(targets), cbuf.copy_(cands), pack_allow(m, out=words)
        for t in tuple(rout) + tuple(lout):
            t.fill_(77)
        rank_graph.replay(), rerank_graph.replay()
        torch.cuda.synchronize()
        w = pack_allow(m)
        same(rout, whole.rank(queries, targets, allow=w), "rank: replay == the whole table, eager")
        same(lout, whole.rerank(cands, queries, n, allow=w), "rerank: replay == the whole table, eager")


def test_the_launch_tags_of_one_call_and_nothing_waits_for_the_device():
    from drn_amd import ShardedShortlister, ops, pack_allow
    emb, q17 = exact_data(V, 40, 17, torch.bfloat16)
    emb2, tok, off = tokens_for("cycle", 40, torch.bfloat16)
    sh, rg = ShardedShortlister(shards_of(emb, [0, 321, V])), ShardedShortlister(shards_of(emb2, [0, 3, 70, 120], off))
    words = pack_allow((torch.rand((V,)) < 0.5).to(DEV))
    targets, cands = targets_for([0, 321, V]), sh.shortlist(q17, 8).ids
    q, lengths, t2 = tok[:, :3].contiguous(), lengths_of(3), targets_for([0, 3, 70, 120])
    calls = (lambda: sh.rank(q17, targets), lambda: sh.rank(q17, targets, allow=words), lambda: rg.rank(q[:, 0].contiguous(), t2),
             lambda: rg.rank_late(q, lengths, t2), lambda: sh.rerank(cands, q17, 8), lambda: sh.rerank(cands, q17, 8, allow=words))
    for call in calls:
        call()                                                                # (warm)
    torch.cuda.synchronize()
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # (torch says that the mode is a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        for call in calls:
            ops.kernel_timer = []
            call()
            seen.append([t[0] for t in ops.kernel_timer])
    finally:
        torch.cuda.set_sync_debug_mode("default")
        ops.kernel_timer = None
    group = lambda K, tag: ["shard_positions"] + [tag] * K + ["shortlist_rank_thresholds"] + [tag] * K + ["shortlist_rank_reduce_shards"]
    assert seen[0] == group(2, "shortlist_rank_phase")
    assert seen[1] == seen[0][:1] + ["allow_slices"] + seen[0][1:] and len(seen[1]) == 2 * 2 + 4
    assert seen[2] == group(3, "shortlist_segments_rank_phase") and seen[3] == group(3, "shortlist_late_rank_phase")
    assert seen[4] == ["shard_positions", "shortlist_rerank", "shortlist_rerank", "shortlist_merge_lists"]
    assert seen[5] == ["shard_positions", "allow_slices", "shortlist_rerank", "shortlist_rerank", "shortlist_merge_lists"]


# -- 5. the evaluators ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [False, True], ids=["one-vector", "late"])
def test_the_evaluators_take_a_sharded_table_in_either_place(late):
    from drn_amd import ShardedShortlister, Shortlister, evaluate_cascade, evaluate_shortlist
    lens = [1, 3, 0, 17] * 10 + [40, 2]
    Vv, off = len(lens), offsets_of(lens)
    names = ["v%d" % v for v in range(Vv)]
    emb, tok = random_case(int(sum(lens)), 96, torch.bfloat16, 70)
    g = torch.Generator().manual_seed(4)
    coarse_emb = torch.randn(Vv, 32, generator=g).to(DEV, torch.bfloat16).contiguous()
    coarse, fine = Shortlister(coarse_emb, names=names, quantize="mxfp8"), Shortlister(emb, names=names, offsets=off)
    cut = 13
    coarse_sh = ShardedShortlister([Shortlister(coarse_emb[:cut].clone(), names=names[:cut], quantize="mxfp8"),
                                    Shortlister(coarse_emb[cut:].clone(), names=names[cut:], quantize="mxfp8")])
    fine_sh = ShardedShortlister([Shortlister(emb[:int(off[cut])].clone(), names=names[:cut], offsets=off[:cut + 1]),
                                  Shortlister(emb[int(off[cut]):].clone(), names=names[cut:], offsets=off[cut:] - off[cut])])
    batches, ranked = [], []
    for b, S_ in enumerate((17, 6)):
        cq = torch.randn(S_, 32, generator=g).to(DEV, torch.bfloat16).contiguous()
        picked = [names[t] for t in torch.randint(0, Vv, (S_,), generator=g).tolist()]
        fq = tok[:S_, 8 * b:8 * b + 8].contiguous()
        lengths = lengths_of(8, S_).clamp(min=1)
        batches.append((picked, cq, fq if late else fq[:, 0].contiguous(), lengths))
        ranked.append((picked, fq, lengths) if late else (picked, fq[:, 0].contiguous()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = evaluate_shortlist(fine, iter(ranked), topks=(1, 10, 100), late=late)
        got = evaluate_shortlist(fine_sh, iter(ranked), topks=(1, 10, 100), late=late)
        assert got.n == 23 and np.array_equal(got.ranks, want.ranks) and got.recall == want.recall and (want.ranks >= 0).any()
        want = evaluate_cascade(coarse, fine, iter(batches), 12, late=late)
        for a, b in ((coarse_sh, fine), (coarse, fine_sh), (coarse_sh, fine_sh)):
            got = evaluate_cascade(a, b, iter(batches), 12, late=late)
            assert np.array_equal(got.ranks, want.ranks) and got.recall == want.recall
    assert (want.ranks >= 0).any() and (want.ranks < 0).any()


def test_reranked_ids_of_a_sharded_table_are_device_candidates_of_the_search():
    from drn_amd import Grounder, ShardedShortlister, Shortlister
    m, store, index, kw = world("plain")
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (NV, 16), generator=g).float()
    emb[4] = emb[1]                                                           # a tie across the shards, broken by corpus position
    emb = emb.to(DEV).contiguous()
    sh = ShardedShortlister([Shortlister(emb[:3].clone(), names=store.names[:3]), Shortlister(emb[3:].clone(), names=store.names[3:])])
    qe = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    qe[1] = float("nan")                                                      # a sentence whose lists are empty: ids all -1
    grounder = Grounder(m, top_k=5, **kw)
    tok, qlen = sentences(7)
    short = sh.rerank(sh.shortlist(qe, 6).ids, qe, 4)
    same(short, Shortlister(emb).shortlist(qe, 4), "the whole table")
    got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
    assert [len(l) for l in lists] == [4, 0, 4]
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "two stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0
