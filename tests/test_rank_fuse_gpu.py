"""Rank fusion on the device: rank_fuse / rank_fuse_rank (drn_rank_fuse_topn / _rank, csrc/retrieve_rrf.hip) against
rank_fuse_reference / rank_fuse_rank_reference evaluated on the host over the same lists -- every sort length the entry picks, rows of
junk, of one id repeated everywhere and of nothing, a full 8192-word row of disjoint lists, masks, out= buffers inside guard bands, a
device weights tensor changed in place -- then RankFusedShortlister against rank_fuse over the tables' own lists, evaluate_shortlist on a
planted corpus, and one graph capture replayed after lists, weights and mask were overwritten.
Every comparison is torch.equal, scores as int32 bits.  No vote and no partial sum is subnormal here: a weight is 0 or at least 2^-3 in
magnitude, a denominator at most 1084, and a difference of two fp32 numbers above 2^-14 in magnitude is 0 or at least 2^-38.
tests/test_rank_fuse_cpu.py holds the definition, the refusals and the C boundary."""
import warnings

import numpy as np
import pytest
import torch

from test_allow_shortlist_gpu import EMPTY, bool_masks, packed
from test_fused_rerank_gpu import INT_MAX, INT_MIN, listed
from test_fused_shortlist_gpu import VF, WEIGHTS, fused_world, pick, same_fields, same_ranks
from test_grounding_engine_gpu import DEV
from test_segment_shortlist_gpu import offsets_of
from test_shortlist_gpu import exact_data

pytestmark = pytest.mark.gpu
V40 = 40                                                     # heavy overlap, many ties
WEIGHT_SETS = ([1.0] * 8, [1.0, 0.5, 2.0, 0.25, 4.0, 0.125, 3.0, 1.5], [1.0, 0.0, 2.0, 0.0, 1.0, 1.0, 0.0, 1.0],
               [1.0, -0.5, 2.0, -1.0, 0.25, 1.0, -2.0, 1.0])  # ones, distinct, with zeros, with negatives
K0S = (0.0, 0.5, 60.0)
DEPTHS = (1, 128, 129, 1024)


def host_reference(lists, V, n, w, k0, missing, allow=None):
    """rank_fuse_reference over host copies of the lists (IEEE float32 on the CPU) -> Shortlist on the device."""
    from drn_amd import Shortlist, rank_fuse_reference
    got = rank_fuse_reference([c.cpu() for c in lists], V, n, weights=w, k0=k0, missing=missing, allow=allow)
    return Shortlist(*(t.to(DEV) for t in got))


def host_rank_reference(lists, V, targets, w, k0, missing, allow=None):
    from drn_amd import TargetRank, rank_fuse_rank_reference
    got = rank_fuse_rank_reference([c.cpu() for c in lists], V, targets.cpu(), weights=w, k0=k0, missing=missing, allow=allow)
    return TargetRank(*(t.to(DEV) for t in got))


def targets_of(V, S_, k=0):
    """S_ targets walking over [0, V) with -1, V, INT_MIN and INT_MAX among them."""
    t = [(7 * s + k) % V for s in range(S_)]
    for s, junk in zip(range(1, S_, 4), (-1, V, INT_MIN, INT_MAX)):
        t[s] = junk
    return torch.tensor(t, dtype=torch.int32, device=DEV)


def lists_of(M, C, S_, V=V40):
    """M lists (S_, C): the junk and repeat pattern of listed(), a different draw per list; list 1 is a real shortlist's ids over
    exact data (equal scores, -1 padding at the end where C > V)."""
    from drn_amd import Shortlister
    out = [listed(V, C, S_=S_, seed=m) for m in range(M)]
    if M > 1:
        emb, q = exact_data(V, 8, S_, torch.float32)
        sl = Shortlister(emb)
        out[1] = (sl.shortlist(q, C) if C <= 128 else sl.shortlist_deep(q, C)).ids
    return out


# -- 1. the kernel against the definition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("missing", ["skip", "drop"])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_fused_lists_and_ranks_equal_the_reference(M, missing):
    """M x C = 1 .. 8192 entries a sentence: every sort length from 256 to 8192 words.  V = 40: every list holds most videos, equal
    sums are common and fall by position.  n, k0 and the weights cycle, so every value meets every C."""
    from drn_amd import Shortlist, TargetRank, rank_fuse, rank_fuse_rank
    case = 0
    for C in (1, 5, 128, 1024):
        for S_ in (1, 17):
            lists = lists_of(M, C, S_)
            stacked = torch.stack(lists)
            for n in DEPTHS:
                w, k0 = WEIGHT_SETS[case % 4][:M], K0S[case % 3]
                case += 1
                got = rank_fuse(stacked if case % 2 else lists, V40, n, weights=w, k0=k0, missing=missing)
                assert isinstance(got, Shortlist) and tuple(got.ids.shape) == (S_, n)
                same_fields(got, host_reference(lists, V40, n, w, k0, missing), (C, S_, n, k0))
            targets = targets_of(V40, S_, k=C)
            rk = rank_fuse_rank(lists, V40, targets, weights=w, k0=k0, missing=missing)
            assert isinstance(rk, TargetRank)
            same_ranks(rk, host_rank_reference(lists, V40, targets, w, k0, missing), (C, S_))
            # rank = k exactly when ids[s, k] is the target (n = 1024 holds every candidate of 40 videos)
            at = (got.ids == targets[:, None]) & (targets[:, None] >= 0)
            place = torch.where(at.any(dim=1), at.int().argmax(dim=1), torch.full((S_,), -1, device=DEV))
            assert torch.equal(rk.rank.long(), place) and torch.equal(rk.total, got.n)
    if missing == "skip":
        assert int(got.n.max()) > 30                               # (C = 1024 over 40 videos lists nearly all of them)


def test_unequal_widths_are_padded_with_what_means_nothing():
    """A sequence of lists of 5, 128, 1 and 300 columns: the stacked buffer is padded with -1, and the answer is the definition's over
    the lists as they were given."""
    from drn_amd import rank_fuse, rank_fuse_rank
    lists = [listed(V40, C, seed=m) for m, C in enumerate((5, 128, 1, 300))]
    w = [1.0, 0.5, 2.0, -1.0]
    targets = targets_of(V40, 17)
    for missing in ("skip", "drop"):
        for n in (7, 129):
            same_fields(rank_fuse(lists, V40, n, weights=w, missing=missing), host_reference(lists, V40, n, w, 60.0, missing), (missing, n))
        same_ranks(rank_fuse_rank(lists, V40, targets, weights=w, missing=missing), host_rank_reference(lists, V40, targets, w, 60.0, missing))


def test_eight_disjoint_lists_of_1024_fill_the_row():
    """V = 9000, list m a permutation of [1024 m, 1024 m + 1024): the union is exactly 8192 videos, every word of LDS is an owner, and
    at equal weights the eight videos of one rank tie.  Under "drop" nothing is a candidate."""
    from drn_amd import rank_fuse, rank_fuse_rank
    V, S_ = 9000, 3
    g = torch.Generator().manual_seed(8)
    lists = [torch.stack([1024 * m + torch.randperm(1024, generator=g) for _ in range(S_)]).to(torch.int32).to(DEV) for m in range(8)]
    targets = torch.tensor([int(lists[5][0, 1023]), 8999, int(lists[0][2, 0])], dtype=torch.int32, device=DEV)
    for w in (WEIGHT_SETS[0], WEIGHT_SETS[1]):
        got = rank_fuse(lists, V, 1024, weights=w, k0=0.5)
        same_fields(got, host_reference(lists, V, 1024, w, 0.5, "skip"), "full row")
        rk = rank_fuse_rank(lists, V, targets, weights=w, k0=0.5)
        same_ranks(rk, host_rank_reference(lists, V, targets, w, 0.5, "skip"), "full row")
        assert rk.total.tolist() == [8192] * 3 and int(rk.rank[1]) == -1 and int(rk.rank[0]) > 1024
    assert got.n.tolist() == [1024] * 3
    none = rank_fuse(lists, V, 5, missing="drop")
    assert none.n.tolist() == [0] * 3 and bool((none.ids == -1).all()) and bool((none.scores == 0).all())
    assert rank_fuse_rank(lists, V, targets, missing="drop").total.tolist() == [0] * 3


def test_rows_of_one_id_of_nothing_and_of_junk():
    """8 x 1024 entries: sentence 0 holds video 7 in every entry (8192 repeats: one owner, ranks 0), sentence 1 only -1, sentence 2 only
    values outside [0, V), sentence 3 the ordinary pattern."""
    from drn_amd import rank_fuse, rank_fuse_rank
    lists = [listed(V40, 1024, S_=4, seed=m) for m in range(8)]
    for m, c in enumerate(lists):
        c[0], c[1] = 7, -1
        c[2] = torch.tensor([V40, INT_MIN, INT_MAX, -1], dtype=torch.int32, device=DEV).repeat(256)
    targets = torch.tensor([7, 7, 0, 3], dtype=torch.int32, device=DEV)
    for missing in ("skip", "drop"):
        got = rank_fuse(lists, V40, 128, missing=missing, k0=0.0)
        same_fields(got, host_reference(lists, V40, 128, None, 0.0, missing), missing)
        assert got.n.tolist()[:3] == [1, 0, 0] and got.ids[0, :2].tolist() == [7, -1] and float(got.scores[0, 0]) == 8.0
        rk = rank_fuse_rank(lists, V40, targets, missing=missing, k0=0.0)
        same_ranks(rk, host_rank_reference(lists, V40, targets, None, 0.0, missing), missing)
        assert rk.rank.tolist()[:3] == [0, -1, -1] and rk.total.tolist()[:3] == [1, 0, 0]


def test_masks_out_buffers_and_device_weights():
    """A shared and a per-sentence mask (bits past V set in the last word); out= buffers between guard bands; a device weights tensor
    kept by reference and changed in place between calls; torch's synchronisation check armed around the calls."""
    from drn_amd import Shortlist, TargetRank, rank_fuse, rank_fuse_rank
    M, C, S_, n, GUARD = 3, 128, 17, 20, 64
    lists = lists_of(M, C, S_)
    stacked = torch.stack(lists)
    shared, per = bool_masks(V40)
    targets = targets_of(V40, S_)
    wdev = torch.tensor(WEIGHT_SETS[1][:M], dtype=torch.float32, device=DEV)
    shapes, dtypes = ((S_, n), (S_, n), (S_,), (S_,), (S_,), (S_,)), (torch.int32, torch.float32, torch.int32) * 2
    flat = [torch.full((int(np.prod(sh)) + 2 * GUARD,), 77, dtype=dt, device=DEV) for sh, dt in zip(shapes, dtypes)]
    bufs = [f[GUARD:f.numel() - GUARD].view(sh) for f, sh in zip(flat, shapes)]
    out, rout = Shortlist(*bufs[:3]), TargetRank(*bufs[3:])
    words = {id(shared): packed(shared), id(per): packed(per)}
    rank_fuse(stacked, V40, n), rank_fuse_rank(stacked, V40, targets)           # (warm: host weights of ones are uploaded once)
    for weights in (WEIGHT_SETS[1][:M], WEIGHT_SETS[3][:M], WEIGHT_SETS[2][:M]):
        wdev.copy_(torch.tensor(weights, dtype=torch.float32))
        for mask in (shared, per):
            for missing in ("skip", "drop"):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                       # (torch says that the mode is a prototype)
                    torch.cuda.set_sync_debug_mode("error")
                try:
                    got = rank_fuse(stacked, V40, n, weights=wdev, k0=0.5, missing=missing, allow=words[id(mask)], out=out)
                    rk = rank_fuse_rank(stacked, V40, targets, weights=wdev, k0=0.5, missing=missing, allow=words[id(mask)], out=rout)
                    plain = rank_fuse(lists, V40, n, missing=missing, allow=words[id(mask)])
                finally:
                    torch.cuda.set_sync_debug_mode("default")
                assert all(a is b for a, b in zip(got, out)) and all(a is b for a, b in zip(rk, rout))
                same_fields(got, host_reference(lists, V40, n, weights, 0.5, missing, allow=mask), (weights, missing))
                same_ranks(rk, host_rank_reference(lists, V40, targets, weights, 0.5, missing, allow=mask), (weights, missing))
                same_fields(plain, host_reference(lists, V40, n, None, 60.0, missing, allow=mask), "a sequence, weights of ones")
                assert all(bool((f[:GUARD] == 77).all()) and bool((f[f.numel() - GUARD:] == 77).all()) for f in flat)
        assert int(got.n[EMPTY]) == 0 and int(rk.rank[EMPTY]) == -1 and int(rk.total[EMPTY]) == 0


# -- 2. the class ------------------------------------------------------------------------------------------------------------------------------

def own_lists(tables, items, depth, allow=None):
    """Each table's own list of `depth`: shortlist, shortlist_deep beyond 128, shortlist_late for a pair."""
    out = []
    for t, i in zip(tables, items):
        if isinstance(i, tuple):
            out.append(t.shortlist_late(i[0], i[1], depth, allow=allow).ids)
        else:
            out.append((t.shortlist if depth <= 128 else t.shortlist_deep)(i, depth, allow=allow).ids)
    return out


def sharded_world():
    """fused_world's four ways to score VF videos -- a plain bf16 table, a ragged fp32 one, a ragged FP8 one, that one by late
    interaction -- and the plain table again as two shards."""
    from drn_amd import ShardedShortlister, Shortlister
    tables, items, _ = pick(fused_world(False), 4)
    plain = tables[0]
    parts = ShardedShortlister([Shortlister(plain.embeddings[:300].contiguous()), Shortlister(plain.embeddings[300:].contiguous())])
    return tables + [parts], items + [items[0]]


@pytest.mark.parametrize("missing", ["skip", "drop"])
def test_the_class_is_rank_fuse_over_the_tables_own_lists(missing):
    """A plain table, a ragged one, a ragged FP8 one, a late item and a sharded table, at depth 128 and 20; with and without a mask, which
    goes to the tables: a masked video takes no rank.  rank agrees with shortlist."""
    from drn_amd import RankFusedShortlister, Shortlist, rank_fuse, rank_fuse_rank
    tables, items = sharded_world()
    w = [1.0, 0.5, 2.0, -0.25, 1.0]
    shared, per = bool_masks(VF)
    targets = targets_of(VF, 17, k=3)
    for depth in (128, 20):
        rf = RankFusedShortlister(tables, weights=w, k0=0.5, depth=depth, missing=missing)
        assert len(rf) == VF and rf.names == ["v%d" % v for v in range(VF)] and rf.device == tables[0].device
        for mask in (None, shared, per):
            words = None if mask is None else packed(mask)
            lists = own_lists(tables, items, depth, allow=words)
            for n in (5, 300):
                got = rf.shortlist(items, n, allow=words)
                assert isinstance(got, Shortlist) and tuple(got.ids.shape) == (17, n)
                same_fields(got, rank_fuse(lists, VF, n, weights=w, k0=0.5, missing=missing), (depth, n))
                same_fields(got, host_reference(lists, VF, n, w, 0.5, missing), (depth, n))
            rk = rf.rank(items, targets, allow=words)
            same_ranks(rk, rank_fuse_rank(lists, VF, targets, weights=w, k0=0.5, missing=missing), depth)
            full = rf.shortlist(items, 1024, allow=words)
            at = (full.ids == targets[:, None]) & (targets[:, None] >= 0)
            place = torch.where(at.any(dim=1), at.int().argmax(dim=1), torch.full((17,), -1, device=DEV))
            assert torch.equal(rk.rank.long(), place) and torch.equal(rk.total, full.n)
            if mask is not None:
                listed_ = full.ids.clamp(min=0).long()
                ok = torch.gather((mask if mask.dim() == 2 else mask[None].expand(17, VF)).to(DEV), 1, listed_) | (full.ids < 0)
                assert bool(ok.all()), "a masked video is listed"
    assert int(full.n[EMPTY]) == 0


def test_depth_300_goes_through_the_deep_shortlists():
    from drn_amd import RankFusedShortlister, rank_fuse
    tables, items, _ = pick(fused_world(False), 3)
    rf = RankFusedShortlister(tables, depth=300)
    lists = own_lists(tables, items, 300)
    assert all(tuple(c.shape) == (17, 300) for c in lists) and int((lists[0][:, 299] >= 0).sum()) == 17
    for n in (128, 1024):
        got = rf.shortlist(items, n)
        same_fields(got, rank_fuse(lists, VF, n), n)
        same_fields(got, host_reference(lists, VF, n, None, 60.0, "skip"), n)
    out = tuple(torch.empty_like(t) for t in got)
    assert all(a is b for a, b in zip(rf.shortlist(items, 1024, out=out), out))
    same_fields(rf.shortlist(items, 1024, out=out), got, "out=")


def test_evaluate_shortlist_takes_a_rank_fused_table_as_it_stands():
    """A planted corpus: every sentence's queries are rows of its own video, so both tables list the target first, its fused vote is
    the largest there is and its rank is 0; a sentence whose target no list holds ranks -1."""
    from drn_amd import RankFusedShortlister, ShortlistRecall, Shortlister, evaluate_shortlist, metrics
    lens = [1, 3, 2, 17] * 10 + [40, 2]
    V, off = len(lens), offsets_of(lens)
    names = ["v%d" % v for v in range(V)]
    g = torch.Generator().manual_seed(15)
    win, tit = torch.randn(int(off[-1]), 96, generator=g), torch.randn(V, 128, generator=g)   # (wide: a row's best match is itself)
    windows = Shortlister(win.to(DEV, torch.bfloat16).contiguous(), names=names, offsets=off)
    titles = Shortlister(tit.to(DEV).contiguous())
    rf = RankFusedShortlister([windows, titles], depth=4)
    batches, want = [], []
    for S_ in (17, 6):
        targets = torch.randint(0, V, (S_,), generator=g)
        qw = win[torch.from_numpy(off[:-1])[targets]].to(DEV, torch.bfloat16).contiguous()
        qt = tit[targets].clone()
        qw[0], qt[0] = -qw[0], -qt[0]                                     # (sentence 0 points away from its video: outside both lists)
        batches.append(([names[t] for t in targets.tolist()], [qw, qt.to(DEV).contiguous()]))
        want += [-1] + [0] * (S_ - 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = evaluate_shortlist(rf, iter(batches), topks=(1, 10))
    assert isinstance(got, ShortlistRecall) and got.n == 23
    assert got.ranks.dtype == np.int32 and got.ranks.tolist() == want
    assert got.recall == metrics.recall_from_ranks(np.array(want, dtype=np.int32), [1, 10]) and abs(got.recall[0] - 21 / 23) < 1e-6


# -- 3. graph replay ---------------------------------------------------------------------------------------------------------------------------

def test_a_captured_fusion_replays_after_lists_weights_and_mask_changed_in_place():
    from drn_amd import Shortlist, rank_fuse
    from drn_amd.graph import capture_graph
    M, C, S_, n = 3, 128, 5, 40
    pool = [torch.stack(lists_of(M, C, 17))[:, a:a + S_].contiguous() for a in (0, 6, 12)]
    _, per = bool_masks(V40)
    live, wdev, words = pool[0].clone(), torch.tensor(WEIGHT_SETS[0][:M], dtype=torch.float32, device=DEV), packed(per[:S_].contiguous())
    out = Shortlist(torch.empty((S_, n), dtype=torch.int32, device=DEV), torch.empty((S_, n), dtype=torch.float32, device=DEV),
                    torch.empty((S_,), dtype=torch.int32, device=DEV))
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        rank_fuse(live, V40, n, weights=wdev, k0=0.5, allow=words, out=out)      # (warm)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        rank_fuse(live, V40, n, weights=wdev, k0=0.5, allow=words, out=out)
    for lists, weights, mask in ((pool[1], WEIGHT_SETS[1][:M], torch.flip(per[:S_], dims=(0, 1)).contiguous()),
                                 (pool[2], WEIGHT_SETS[3][:M], torch.zeros(S_, V40, dtype=torch.bool)),
                                 (pool[0], WEIGHT_SETS[2][:M], per[:S_].contiguous())):
        live.copy_(lists)
        wdev.copy_(torch.tensor(weights, dtype=torch.float32))
        words.copy_(packed(mask))
        for t in out:
            t.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_fields(out, host_reference(list(lists), V40, n, weights, 0.5, "skip", allow=mask), "replay")
    assert int(out.n.max()) > 0
