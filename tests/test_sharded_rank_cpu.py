"""Rank and rerank over a sharded corpus, the host side: per-part counts under rank_thresholds_reference, summed, EQUAL the rank
references of the whole table (plain, ragged, late) on integer data with equal scores on both sides of every cut;
shard_positions_reference on hand-built rows; per-part rerank references merged by merge_shortlists_reference equal the whole table's;
every refusal of ShardedShortlister.rank / rank_late / rerank / rerank_late that needs no GPU; the six new C entries at ABI 9 with their
argument checks; the compiler's notes on the new kernels, and the notes of the existing rank kernels against the values recorded before
their entries were opened into phases (tests/golden/rank_kernel_notes.json).
tests/test_sharded_rank_gpu.py holds the kernels."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_late_shortlist_cpu import Resident, _no_library
from test_sharded_shortlist_cpu import CUTS, V, _stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
TWINS = ((1, 0), (63, 64), (320, 321), (321, 0), (774, 5), (400, 64))         # equal scores on both sides of every cut of CUTS
PHASES = ("drn_shortlist_rank_phase", "drn_shortlist_segments_rank_phase", "drn_shortlist_late_rank_phase")
SHARD = ("drn_shard_positions", "drn_shortlist_rank_thresholds", "drn_shortlist_rank_reduce_shards")


def same(got, want, what):
    assert type(got) is type(want), what
    for f in want._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


# -- the device's keys and counts, restated on the host ----------------------------------------------------------------------------------------

def keys_of(score, candidate):
    """sl_key of csrc/shortlist.h for every (sentence, LOCAL position): score (S, V) float64 holding float32 values, candidate (S, V)
    bool -> (S, V) numpy uint64, 0 where the video is no candidate."""
    b = (score.float() + 0.0).numpy().view(np.uint32).astype(np.uint64)
    word = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xffffffff), b | np.uint64(0x80000000))
    pos = ~np.arange(score.shape[1], dtype=np.uint64) & np.uint64(0xffffffff)
    return np.where(candidate.numpy(), (word << np.uint64(32)) | pos[None, :], np.uint64(0)).astype(np.uint64)


def score_of(key):
    """sl_score of csrc/shortlist.h -> float32 numpy, 0 where the key is 0."""
    o = (key >> np.uint64(32)).astype(np.uint32)
    raw = np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o).astype(np.uint32)
    return np.where(key != 0, raw.view(np.float32), np.float32(0))


def summed_over_parts(parts, bases, targets):
    """What ShardedShortlister.rank computes, with integer keys on the host: parts = [(score, candidate)] per shard over LOCAL
    positions -> TargetRank.  Target keys from shard_positions_reference, thresholds from rank_thresholds_reference, per-part counts
    of keys > threshold and of keys != 0, summed."""
    from drn_amd import TargetRank, rank_thresholds_reference, shard_positions_reference
    local = shard_positions_reference(targets, bases).numpy()
    keys = [keys_of(*p) for p in parts]
    S = keys[0].shape[0]
    tkeys = np.stack([np.where(local[k] >= 0, keys[k][np.arange(S), np.clip(local[k], 0, keys[k].shape[1] - 1)], np.uint64(0)) for k in range(len(parts))])
    thr, key = rank_thresholds_reference(tkeys.astype(np.uint64))
    above = sum((keys[k] > thr[k][:, None]).sum(axis=1) for k in range(len(parts)))
    total = sum((keys[k] != 0).sum(axis=1) for k in range(len(parts)))
    rank = np.where(key != 0, above, -1)
    return TargetRank(torch.from_numpy(rank.astype(np.int32)), torch.from_numpy(score_of(key).astype(np.float32)), torch.from_numpy(total.astype(np.int32)))


def plain_case():
    """test_sharded_shortlist_cpu.plain_case's table and twins with a sentence per target: both twins of every pair, -1, V, INT_MIN,
    INT_MAX, a target the per-sentence mask excludes, and a NaN query row."""
    g = torch.Generator().manual_seed(3)
    emb = torch.randint(-4, 5, (V, 8), generator=g).float()
    for a, b in TWINS:
        emb[a] = emb[b]
    targets = [t for pair in TWINS for t in pair] + [-1, V, INT_MIN, INT_MAX, 200, 500]
    S = len(targets)
    q = torch.randint(-4, 5, (S, 8), generator=g).float()
    q[S - 1] = float("nan")                                                   # a sentence without candidates
    mask = torch.rand((S, V), generator=g) < 0.5
    mask[2, :64] = False                                                      # a part wholly masked for one sentence (its target 63 too)
    mask[S - 2, 200] = False                                                  # a masked target
    for s, t in enumerate(targets[:12]):
        if s != 2:
            mask[s, t] = True
    return emb, q, mask, torch.tensor(targets, dtype=torch.int32)


def test_counts_under_the_thresholds_sum_to_the_rank_of_the_whole_plain_table():
    from drn_amd import rank_reference
    from drn_amd.retrieve import _plain_scores
    emb, q, mask, targets = plain_case()
    shared = mask[0] | mask[1]
    seen = set()
    for bases in CUTS:
        for allow in (None, mask, shared):
            want = rank_reference(emb, q, targets, allow=allow)
            cut = lambda a, b: None if allow is None else allow[..., a:b]
            parts = [_plain_scores(emb[a:b], q, cut(a, b)) for a, b in zip(bases[:-1], bases[1:])]
            same(summed_over_parts(parts, bases, targets), want, (bases, allow is not None))
            seen.update(want.rank.tolist())
    want = rank_reference(emb, q, targets)
    assert want.rank[12:16].tolist() == [-1] * 4 and want.rank[-1].item() == -1 and want.total[-1].item() == 0 and want.total[0].item() == V
    # with ONE query the later twin of a pair follows the earlier one, and only videos of the same score stand between them
    assert sum(torch.equal(emb[a], emb[b]) for a, b in TWINS) == 5               # (321 was overwritten by row 0 after 320 copied it)
    for a, b in (t for t in TWINS if torch.equal(emb[t[0]], emb[t[1]])):
        pair = rank_reference(emb, q[:1].expand(2, 8), torch.tensor(sorted((a, b)), dtype=torch.int32))
        between = int(((emb @ q[0]) == float(pair.score[0]))[min(a, b) + 1:max(a, b)].sum())
        assert pair.score[0] == pair.score[1] and int(pair.rank[1]) == int(pair.rank[0]) + 1 + between, (a, b)
    masked = rank_reference(emb, q, targets, allow=mask)
    assert masked.rank[2].item() == -1 and masked.rank[-2].item() == -1 and -1 in seen and max(seen) > 100


def ragged_case():
    lens = [1, 3, 0, 17] * 20                                                 # V = 80; video 2 owns no row: the cut at 3 lies next to it
    off = np.concatenate([[0], np.cumsum(lens)])
    g = torch.Generator().manual_seed(5)
    emb = torch.randint(-4, 5, (int(off[-1]), 8), generator=g).float()
    emb[off[70]], emb[off[3]] = emb[off[0]], emb[off[1]]                     # equal scores across the cuts (row off[70] is video 71's first)
    targets = [0, 71, 1, 3, 2, 69, 79, -1, 80, INT_MIN, INT_MAX, 40, 41]
    S = len(targets)
    tok = torch.randint(-4, 5, (S, 3, 8), generator=g).float()
    tok[S - 1, 0, 1] = float("nan")
    lengths = [3, 1, 2, 3, 3, 1, 2, 3, 3, 3, 3, 0, 3]                         # sentence 11 has no live token
    mask = torch.rand((S, 80), generator=g) < 0.6
    mask[0, 0], mask[1, 71], mask[5, 3:70] = True, True, False
    return emb, off, tok, lengths, mask, torch.tensor(targets, dtype=torch.int32)


def test_counts_under_the_thresholds_sum_to_the_rank_of_the_whole_ragged_table():
    from drn_amd import late_rank_reference, segment_rank_reference
    from drn_amd.retrieve import _late_scores, _segment_scores
    emb, off, tok, lengths, mask, targets = ragged_case()
    bases = [0, 3, 70, 80]
    part = lambda a, b: (emb[off[a]:off[b]], off[a:b + 1] - off[a])
    for allow in (None, mask, mask[3]):
        cut = lambda a, b: None if allow is None else allow[..., a:b]
        want = segment_rank_reference(emb, off, tok[:, 0], targets, allow=allow)
        parts = [_segment_scores(*part(a, b), tok[:, 0], cut(a, b)) for a, b in zip(bases[:-1], bases[1:])]
        same(summed_over_parts([(p[0], p[2]) for p in parts], bases, targets), want, ("segments", allow is not None))
        assert want.rank[4].item() == -1 and want.rank[7:11].tolist() == [-1] * 4 and want.rank[-1].item() == -1      # rowless, outside, NaN
        want = late_rank_reference(emb, off, tok, lengths, targets, allow=allow)
        parts = [_late_scores(*part(a, b), tok, lengths, cut(a, b)) for a, b in zip(bases[:-1], bases[1:])]
        same(summed_over_parts(parts, bases, targets), want, ("late", allow is not None))
        assert want.rank[11].item() == -1 and want.total[11].item() == 0 and want.total[0].item() > 0
    want = segment_rank_reference(emb, off, tok[:, 0], targets)
    assert want.rank[0].item() >= 0 and want.rank[1].item() >= 0 and want.rank[6].item() >= 0


def test_the_thresholds_reference_by_hand():
    from drn_amd import _lib, rank_thresholds_reference
    ones = 0xffffffffffffffff
    tk = (5 << 32) | 7
    keys = np.zeros((3, 4), dtype=np.uint64)
    keys[0, 0], keys[1, 1], keys[2, 2] = tk, tk, tk
    thr, key = rank_thresholds_reference(keys)
    assert thr.dtype == key.dtype == np.uint64 and key.tolist() == [tk, tk, tk, 0]
    below, above = (5 << 32) - 1, (5 << 32) | 0xffffffff
    assert thr.tolist() == [[tk, below, below, ones], [above, tk, below, ones], [above, above, tk, ones]]
    t = torch.from_numpy(keys.view(np.int64))
    thr2, key2 = rank_thresholds_reference(t)
    assert thr2.dtype == torch.int64 and np.array_equal(thr2.numpy().view(np.uint64), thr) and np.array_equal(key2.numpy().view(np.uint64), key)
    high = np.array([[0], [(0xfffffffe << 32) | 1]], dtype=np.uint64)        # a word with the top bit set survives the int64 round trip
    assert rank_thresholds_reference(high)[0].tolist() == [[(0xfffffffe << 32) - 1], [int(high[1, 0])]]
    keys[1, 0] = tk
    with pytest.raises(_lib.DrnError, match="sentence 0 has a target key in more than one shard"):
        rank_thresholds_reference(keys)
    for bad in (keys.astype(np.int64), keys[0], torch.zeros((2, 2), dtype=torch.int32)):
        with pytest.raises(_lib.DrnError, match="rank_thresholds_reference: keys must be"):
            rank_thresholds_reference(bad)


def test_shard_positions_reference_on_hand_built_rows():
    from drn_amd import _lib, shard_positions_reference
    bases = [0, 1, 64, 321, V]
    row = [0, 1, 63, 64, 320, 321, 774, -1, V, INT_MIN, INT_MAX]            # both ends of every shard, then the four outside
    got = shard_positions_reference(torch.tensor(row, dtype=torch.int32), bases)
    n = -1
    assert got.dtype == torch.int32 and got.tolist() == [[0, n, n, n, n, n, n, n, n, n, n], [n, 0, 62, n, n, n, n, n, n, n, n],
                                                         [n, n, n, 0, 256, n, n, n, n, n, n], [n, n, n, n, n, 0, 453, n, n, n, n]]
    lists = torch.tensor([row[:6], row[5:]], dtype=torch.int64)
    got = shard_positions_reference(lists, bases)
    assert got.shape == (4, 2, 6) and got[3].tolist() == [[n] * 5 + [0], [0, 453, n, n, n, n]] and got[0].tolist() == [[0] + [n] * 5, [n] * 6]
    assert shard_positions_reference(torch.tensor([5, INT_MAX], dtype=torch.int32), [0, INT_MAX]).tolist() == [[5, -1]]
    for bad in ([1, 2], torch.zeros(3), torch.zeros((1, 2, 3), dtype=torch.int32), torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(_lib.DrnError, match="positions must be an integer tensor"):
            shard_positions_reference(bad, bases)
    with pytest.raises(_lib.DrnError, match="K \\+ 1 bases"):
        shard_positions_reference(torch.zeros(3, dtype=torch.int32), [0])


def test_reranking_the_parts_and_merging_is_the_rerank_of_the_whole_table():
    from drn_amd import (late_rerank_reference, merge_shortlists_reference, rerank_reference, segment_rerank_reference,
                         shard_positions_reference)
    emb, q, mask, _ = plain_case()
    S = int(q.shape[0])
    g = torch.Generator().manual_seed(11)
    cands = torch.randint(-3, V + 3, (S, 40), generator=g, dtype=torch.int32)
    cands[:, 5], cands[:, 6], cands[:, 7], cands[:, 8] = cands[:, 2], -1, INT_MIN, INT_MAX          # a repeat, padding, junk
    cands[:, 9:21] = torch.tensor([t for pair in TWINS for t in pair], dtype=torch.int32)            # ties across every cut
    for bases in CUTS:
        local = shard_positions_reference(cands, bases)
        for n in (5, 40, 49):                                                 # n > C = 40 pads
            for allow in (None, mask):
                want = rerank_reference(emb, cands, q, n, allow=allow)
                parts = [rerank_reference(emb[a:b], local[k], q, n, allow=None if allow is None else allow[:, a:b])
                         for k, (a, b) in enumerate(zip(bases[:-1], bases[1:]))]
                same(merge_shortlists_reference(parts, bases, n), want, (bases, n, allow is not None))
    assert int(want.n[0]) > 5 and int(want.n[-1]) == 0
    emb, off, tok, lengths, mask, _ = ragged_case()
    S, bases = int(tok.shape[0]), [0, 3, 70, 80]
    cands = torch.randint(-3, 83, (S, 30), generator=g, dtype=torch.int32)
    cands[:, :6] = torch.tensor([0, 71, 1, 3, 2, -1], dtype=torch.int32)
    local = shard_positions_reference(cands, bases)
    part = lambda a, b: (emb[off[a]:off[b]], off[a:b + 1] - off[a])
    for n in (5, 37):
        for allow in (None, mask):
            cut = lambda a, b: None if allow is None else allow[:, a:b]
            spans = list(enumerate(zip(bases[:-1], bases[1:])))
            want = segment_rerank_reference(emb, off, cands, tok[:, 0], n, allow=allow)
            got = merge_shortlists_reference([segment_rerank_reference(*part(a, b), local[k], tok[:, 0], n, allow=cut(a, b)) for k, (a, b) in spans], bases, n)
            same(got, want, ("segments", n, allow is not None))
            want = late_rerank_reference(emb, off, cands, tok, lengths, n, allow=allow)
            got = merge_shortlists_reference([late_rerank_reference(*part(a, b), local[k], tok, lengths, n, allow=cut(a, b)) for k, (a, b) in spans], bases, n)
            same(got, want, ("late", n, allow is not None))
            assert int(want.n[11]) == 0 and int(want.n[0]) > 0


# -- refusals, before the library is reached ---------------------------------------------------------------------------------------------------

def test_rank_and_rerank_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import ShardedShortlister, _lib
    _no_library(monkeypatch)
    res = lambda t: t.as_subclass(Resident)
    i32 = lambda *shape: res(torch.zeros(shape, dtype=torch.int32))
    q, tok, lengths = res(torch.zeros(2, 32, dtype=torch.bfloat16)), res(torch.zeros(2, 3, 32, dtype=torch.bfloat16)), i32(2)
    for ragged in (False, True):
        sh = ShardedShortlister([_stand_in(3, ragged), _stand_in(70, ragged, quantize="mxfp8")])       # V = 73: W = 3
        assert sh.blk_off == [0, 1, 2] and sh.blk_off_device.tolist() == [0, 1, 2] and sh.device == torch.device("cpu")
        calls = [("rank", lambda queries=q, targets=i32(2), **kw: sh.rank(queries, targets, **kw)),
                 ("rerank", lambda queries=q, candidates=i32(2, 5), **kw: sh.rerank(candidates, queries, **kw))]
        if ragged:
            calls += [("rank_late", lambda queries=tok, targets=i32(2), **kw: sh.rank_late(queries, lengths, targets, **kw)),
                      ("rerank_late", lambda queries=tok, candidates=i32(2, 5), **kw: sh.rerank_late(candidates, queries, lengths, **kw))]
        for name, call in calls:
            late = name.endswith("late")
            with pytest.raises(_lib.DrnError, match="Shortlister.%s: the queries must be a tensor" % name):
                call(queries=[[0.0] * 32])
            with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
                call(queries=res(torch.zeros((2, 3, 32) if late else (2, 32))))
            with pytest.raises(_lib.DrnError, match="on the table's device"):
                call(queries=torch.zeros((2, 3, 32) if late else (2, 32), dtype=torch.bfloat16))
            for bad, match in ((torch.ones(73, dtype=torch.bool), "pack it first"), (res(torch.zeros(3, dtype=torch.int64)), "torch.int32 packed words"),
                               (torch.zeros(3, dtype=torch.int32), "on the table's device"),
                               (i32(1), r"must be \(3,\) -- one mask for all sentences -- or \(2, 3\).*V = 73")):
                with pytest.raises(_lib.DrnError, match=match):
                    call(allow=bad)
            if name.startswith("rank"):
                for bad in (i32(3), res(torch.zeros(2, dtype=torch.int64)), [0, 1], i32(2, 2)[:, 0]):
                    with pytest.raises(_lib.DrnError, match=r"targets must be a contiguous \(2,\) torch.int32 tensor"):
                        call(targets=bad)
                with pytest.raises(_lib.DrnError, match="targets must be on the table's device"):
                    call(targets=torch.zeros(2, dtype=torch.int32))
                with pytest.raises(_lib.DrnError, match="three buffers of a TargetRank"):
                    call(out=[None] * 2)
                with pytest.raises(_lib.DrnError, match="out.score must be a contiguous"):
                    call(out=[i32(2), i32(2), i32(2)])
            else:
                with pytest.raises(_lib.DrnError, match="the table must be on the GPU"):
                    ShardedShortlister([_stand_in(3, ragged, resident=False)]).__getattribute__(name)(*((i32(2, 5), tok, lengths) if late else (i32(2, 5), q)))
                for bad, match in (([[1]], "candidates must be a tensor"), (res(torch.zeros((2, 5), dtype=torch.int64)), "torch.int32 store positions"),
                                   (i32(2), r"must be \(S, C\)"), (i32(2, 1025), r"C = 1025 candidates a sentence outside \[1, 1024\]"),
                                   (torch.zeros((2, 5), dtype=torch.int32), "candidates must be on the table's device"),
                                   (i32(2, 10)[:, ::2], "candidates must be contiguous")):
                    with pytest.raises(_lib.DrnError, match=match):
                        call(candidates=bad)
                for n in (0, 129):
                    with pytest.raises(_lib.DrnError, match=r"n = %d outside \[1, 128\]" % n):
                        call(n=n)
                with pytest.raises(_lib.DrnError, match="%d sentences|a row per row of candidates" % 2):
                    call(candidates=i32(3, 5))
                with pytest.raises(_lib.DrnError, match="three buffers of a Shortlist"):
                    call(out=[None] * 4)
                with pytest.raises(_lib.DrnError, match="out.ids must be a contiguous"):
                    call(n=4, out=[i32(2, 5), res(torch.zeros(2, 4)), i32(2)])
        if ragged:
            with pytest.raises(_lib.DrnError, match=r"L = 65 tokens outside \[1, 64\]"):
                sh.rank_late(res(torch.zeros(2, 65, 32, dtype=torch.bfloat16)), lengths, i32(2))
            with pytest.raises(_lib.DrnError, match="never read on the host"):
                sh.rerank_late(i32(2, 5), tok, torch.zeros(2, dtype=torch.int32))
            with pytest.raises(_lib.DrnError, match="lengths must be a contiguous"):
                sh.rank_late(tok, None, i32(2))
        else:
            with pytest.raises(_lib.DrnError, match=r"rank_late: these tables have one row per video.*call rank\(\)"):
                sh.rank_late(tok, lengths, i32(2))
            with pytest.raises(_lib.DrnError, match=r"rerank_late: these tables have one row per video.*call rerank\(\)"):
                sh.rerank_late(i32(2, 5), tok, lengths)
    # with every argument in order the first launch is what fails: the library is not there
    sh = ShardedShortlister([_stand_in(3), _stand_in(70)])
    for call in (lambda: sh.rank(q, i32(2)), lambda: sh.rerank(i32(2, 5), q)):
        with pytest.raises(_lib.DrnError, match="GPU only|not found"):
            call()


def test_the_wrappers_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops
    _no_library(monkeypatch)
    res = lambda t: t.as_subclass(Resident)
    i32 = lambda *shape: res(torch.zeros(shape, dtype=torch.int32))
    i64 = lambda *shape: res(torch.zeros(shape, dtype=torch.int64))
    assert ops.shortlist_sharded_rank_ws_keys([1, 2, 1], 5) == 5 * (2 * 3 + 4) and ops.shortlist_sharded_rank_ws_keys([7], 1) == 9
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.shard_positions(torch.zeros(3, dtype=torch.int32), i32(3), i32(2, 3))
    for bad in (i64(3), i32(2, 1025), i32(2, 3, 4), i32(4, 2)[:, 0]):
        with pytest.raises(_lib.DrnError, match=r"positions must be a contiguous torch.int32 tensor \(S,\) or \(S, C\)"):
            ops.shard_positions(bad, i32(3), i32(2, 3))
    for bad in (i32(1), i32(66), i64(3)):
        with pytest.raises(_lib.DrnError, match=r"bases must be a contiguous \(K \+ 1,\) torch.int32 tensor with 1 <= K <= 64"):
            ops.shard_positions(i32(3), bad, i32(2, 3))
    with pytest.raises(_lib.DrnError, match=r"out must be a contiguous \(2, 3, 4\) torch.int32 tensor"):
        ops.shard_positions(i32(3, 4), i32(3), i32(2, 3))
    for bad in (i64(65, 2), i64(4), i32(2, 2)):
        with pytest.raises(_lib.DrnError, match=r"keys must be a contiguous \(K, S\) torch.int64 tensor with 1 <= K <= 64"):
            ops.shortlist_rank_thresholds(bad, i64(2, 2), i64(2))
    with pytest.raises(_lib.DrnError, match="thresholds must be a contiguous"):
        ops.shortlist_rank_thresholds(i64(2, 3), i64(3, 2), i64(3))
    with pytest.raises(_lib.DrnError, match="key must be a contiguous"):
        ops.shortlist_rank_thresholds(i64(2, 3), i64(2, 3), i64(2))
    good = lambda: dict(key=i64(5), cnt=i64(20), blk_off=i32(4), blocks=4, rank=i32(5), score=res(torch.zeros(5)), total=i32(5))
    for change, match in ((dict(key=i32(5)), "key must be"), (dict(blk_off=i32(1)), "blk_off must be"), (dict(cnt=i64(19)), "at least 20 elements"),
                          (dict(blocks=2), "blocks = 2 >= K = 3"), (dict(score=i32(5)), "score must be"), (dict(total=i32(4)), "total must be")):
        with pytest.raises(_lib.DrnError, match=match):
            ops.shortlist_rank_reduce_shards(**dict(good(), **change))
    emb, q = res(torch.zeros(300, 32)), res(torch.zeros(2, 32))
    for phase in (0, 3):
        with pytest.raises(_lib.DrnError, match="phase = %d is neither 1" % phase):
            ops.shortlist_rank_phase(emb, q, phase, i32(2), i64(2), None)
    with pytest.raises(_lib.DrnError, match="phase 1 takes targets"):
        ops.shortlist_rank_phase(emb, q, 1, None, i64(2), None)
    with pytest.raises(_lib.DrnError, match="phase 1 takes targets"):
        ops.shortlist_rank_phase(emb, q, 1, i32(2), i64(2), i64(4))
    with pytest.raises(_lib.DrnError, match=r"phase 2 takes cnt, a contiguous torch.int64 tensor of at least 4 elements"):
        ops.shortlist_rank_phase(emb, q, 2, None, i64(2), i64(3))
    with pytest.raises(_lib.DrnError, match=r"keys must be a contiguous \(2,\) torch.int64"):
        ops.shortlist_rank_phase(emb, q, 1, i32(2), i64(3), None)
    with pytest.raises(_lib.DrnError, match=r"queries must be a contiguous \(S, L, E\)"):
        ops.shortlist_late_rank_phase(emb, q, i32(2), i32(11), i32(2), 1, i32(2), i64(2), None)


def test_the_evaluators_take_a_sharded_table_up_to_the_first_launch(monkeypatch):
    """No _table() is asked of a ShardedShortlister: names are resolved over the corpus and the first thing that fails is a launch."""
    from drn_amd import ShardedShortlister, _lib, evaluate_cascade, evaluate_shortlist, search_eval
    _no_library(monkeypatch)
    monkeypatch.setattr(search_eval, "_upload", lambda t, dev: t.as_subclass(Resident))
    res = lambda t: t.as_subclass(Resident)
    sh = ShardedShortlister([_stand_in(3), _stand_in(70)])
    sh.names = ["a%d" % v for v in range(73)]
    q = res(torch.zeros(2, 32, dtype=torch.bfloat16))
    with pytest.raises(_lib.DrnError, match="no video named zzz"):
        evaluate_shortlist(sh, [(["zzz", "a1"], q)])
    with pytest.raises(_lib.DrnError, match="GPU only|not found"):
        evaluate_shortlist(sh, [(["a72", "a1"], q)])
    coarse = _stand_in(73)                                                    # (a single table: its first launch is what fails)
    coarse.names = list(sh.names)
    with pytest.raises(_lib.DrnError, match="no video named zzz"):
        evaluate_cascade(coarse, sh, [(["zzz", "a1"], q, q)], 4)
    with pytest.raises(_lib.DrnError, match="GPU only|not found"):
        evaluate_cascade(coarse, sh, [(["a72", "a1"], q, q)], 4)
    coarse.names = coarse.names[::-1]
    for pair in ((coarse, sh), (sh, coarse)):
        with pytest.raises(_lib.DrnError, match="must carry the same names"):
            evaluate_cascade(pair[0], pair[1], [(["a72", "a1"], q, q)], 4)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_six_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name, count in zip(PHASES + SHARD, (15, 19, 21, 7, 6, 11)):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
        assert callable(getattr(ops, name[4:]))
    for public in ("shard_positions_reference", "rank_thresholds_reference"):
        assert hasattr(drn_amd, public), public
    for method in ("rank", "rank_late", "rerank", "rerank_late"):
        assert callable(getattr(drn_amd.ShardedShortlister, method))
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_shard_rank.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shard_positions_kernel", "rank_thresholds_kernel", "rank_reduce_shards_kernel"]
    assert not re.search(r"atomic\w*\s*\(", src)


def test_the_new_entries_check_their_arguments_before_anything_is_launched():
    lib = built_lib()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def positions(K=4, S=2, C=5, ptrs=(p, p, p)):
        return lib.drn_shard_positions(ptrs[0], ptrs[1], K, S, C, ptrs[2], None)
    for i in range(3):
        assert positions(ptrs=[None if j == i else p for j in range(3)]) != 0 and b"null pointer" in lib.drn_last_error(), i
        assert positions(ptrs=[ctypes.c_void_p(0x1002) if j == i else p for j in range(3)]) != 0 and b"4-byte aligned" in lib.drn_last_error(), i
    for K in (0, -1, 65):
        assert positions(K=K) != 0 and b"shards outside [1, 64]" in lib.drn_last_error(), K
    assert positions(S=0) != 0 and b"bad args" in lib.drn_last_error()
    for C in (0, 1025):
        assert positions(C=C) != 0 and b"outside [1, 1024]" in lib.drn_last_error(), C
    assert positions(K=64, S=1 << 20, C=1024) != 0 and b"more than 2^31 words" in lib.drn_last_error()

    def thresholds(K=4, S=2, ptrs=(p, p, p)):
        return lib.drn_shortlist_rank_thresholds(ptrs[0], K, S, ptrs[1], ptrs[2], None)
    for i in range(3):
        assert thresholds(ptrs=[None if j == i else p for j in range(3)]) != 0 and b"null pointer" in lib.drn_last_error(), i
        assert thresholds(ptrs=[odd if j == i else p for j in range(3)]) != 0 and b"8-byte aligned" in lib.drn_last_error(), i
    for K in (0, 65):
        assert thresholds(K=K) != 0 and b"shards outside [1, 64]" in lib.drn_last_error(), K
    assert thresholds(S=0) != 0 and b"bad args" in lib.drn_last_error()

    def reduce(K=3, S=2, blocks=4, nbytes=64, ptrs=None):
        a = [p] * 6 if ptrs is None else ptrs                                 # key cnt blk_off | rank score total
        return lib.drn_shortlist_rank_reduce_shards(a[0], a[1], nbytes, a[2], K, S, blocks, a[3], a[4], a[5], None)
    for i in range(6):
        assert reduce(ptrs=[None if j == i else p for j in range(6)]) != 0 and b"null pointer" in lib.drn_last_error(), i
    for i in (0, 1):
        assert reduce(ptrs=[odd if j == i else p for j in range(6)]) != 0 and b"8-byte aligned" in lib.drn_last_error(), i
    for i in (2, 3, 4, 5):
        assert reduce(ptrs=[ctypes.c_void_p(0x1002) if j == i else p for j in range(6)]) != 0 and b"4-byte aligned" in lib.drn_last_error(), i
    for K in (0, 65):
        assert reduce(K=K, blocks=70) != 0 and b"shards outside [1, 64]" in lib.drn_last_error(), K
    assert reduce(S=0) != 0 and b"bad args" in lib.drn_last_error()
    assert reduce(blocks=2) != 0 and b"2 blocks for K = 3 shards" in lib.drn_last_error()
    assert reduce(nbytes=63) != 0 and b"64 are needed" in lib.drn_last_error()
    assert reduce(S=1 << 20, blocks=1 << 20, nbytes=0x7fffffff) != 0 and b"are needed" in lib.drn_last_error()      # (no int overflow)

    # the phases: the checks of the whole entries (tests/test_rank_shortlist_cpu.py) with keys / cnt in the place of ws and the results
    def plain(V=300, E=64, S=2, dtype=1, phase=2, nbytes=1 << 20, stride=0, ptrs=None, **_):
        a = [p] * 7 if ptrs is None else ptrs                                # table scales queries targets allow | keys cnt
        return lib.drn_shortlist_rank_phase(a[0], a[1], a[2], a[3], a[4], stride, V, E, S, dtype, phase, a[5], a[6], nbytes, None)

    def ragged(R=900, V=300, nblocks=2, E=64, S=2, dtype=1, phase=2, nbytes=1 << 20, stride=0, ptrs=None, **_):
        a = [p] * 9 if ptrs is None else ptrs                                # table scales queries offsets blk_vid targets allow | keys cnt
        return lib.drn_shortlist_segments_rank_phase(a[0], a[1], a[2], a[3], a[4], a[5], a[6], stride, R, V, nblocks, E, S, dtype, phase,
                                                     a[7], a[8], nbytes, None)

    def late(R=900, V=300, nblocks=2, E=64, S=2, L=4, dtype=1, phase=2, nbytes=1 << 20, stride=0, ptrs=None):
        a = [p] * 10 if ptrs is None else ptrs                               # table scales queries lengths offsets blk_vid targets allow | ...
        return lib.drn_shortlist_late_rank_phase(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], stride, R, V, nblocks, E, S, L, dtype, phase,
                                                 a[8], a[9], nbytes, None)
    for fn, nptr, mask_at in ((plain, 7, 4), (ragged, 9, 6), (late, 10, 7)):
        for phase in (0, 3, -1):
            assert fn(phase=phase) != 0 and b"is neither 1 (the target keys) nor 2 (the block counts)" in lib.drn_last_error(), phase
        for phase, optional in ((1, (1, mask_at, nptr - 1)), (2, (1, mask_at, mask_at - 1))):       # phase 1 needs no cnt, phase 2 no targets
            for i in range(nptr):
                rc = fn(phase=phase, ptrs=[None if j == i else p for j in range(nptr)])
                if i in optional:
                    assert b"null pointer" not in lib.drn_last_error() or rc == 0, (fn.__name__, phase, i)
                else:
                    assert rc != 0 and b"null pointer" in lib.drn_last_error(), (fn.__name__, phase, i)
        assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in lib.drn_last_error()
        assert fn(dtype=2) != 0 and b"dtype" in lib.drn_last_error()
        for at in (0, 2):
            assert fn(ptrs=[ctypes.c_void_p(0x1008) if j == at else p for j in range(nptr)]) != 0 and b"16-byte aligned" in lib.drn_last_error()
        for at in (nptr - 2, nptr - 1):                                       # keys, cnt
            assert fn(ptrs=[odd if j == at else p for j in range(nptr)]) != 0 and b"8-byte aligned" in lib.drn_last_error()
        assert fn(E=48) != 0 and b"not a multiple of the block of 32 columns" in lib.drn_last_error()
        assert fn(stride=9) != 0 and b"neither 0" in lib.drn_last_error()
        assert fn(nbytes=8 * 2 * 2 - 1) != 0 and b"the counts hold 31 bytes, 32 are needed" in lib.drn_last_error()    # (two blocks either way)
        assert fn(V=1 << 30, nblocks=1 << 22, S=1 << 10, nbytes=0x7fffffff) != 0 and b"are needed" in lib.drn_last_error()
    for fn in (ragged, late):
        for nblocks in (0, 1, 301):
            assert fn(nblocks=nblocks) != 0 and b"blocks outside" in lib.drn_last_error(), nblocks
    assert late(L=65) != 0 and b"tokens outside [1, 64]" in lib.drn_last_error()


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def _notes(tmp_path, source):
    hipcc, readelf = "/opt/rocm/bin/hipcc", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), source.replace(".hip", ".co"))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, source], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = {"vgpr": get("vgpr_count"), "agpr": int(blk.split()[0]), "sgpr": get("sgpr_count"), "lds": get("group_segment_fixed_size"),
                      "scratch": get("private_segment_fixed_size"), "spills": get("vgpr_spill_count") + get("sgpr_spill_count")}
    return seen


def test_the_new_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_shard_rank.hip compiled for gfx950 on its own: three kernels, no scratch, no spilled register; static LDS is the
    DRN_SHARDS_MAX + 1 words of bases / blk_off (none in the thresholds kernel); VGPRs at or below 64, so eight wavefronts a SIMD."""
    from drn_amd import _lib
    seen = _notes(tmp_path, "retrieve_shard_rank.hip")
    table = (_lib.SHARDS_MAX + 1) * 4
    claims = {"shard_positions_kernel": table, "rank_thresholds_kernel": 0, "rank_reduce_shards_kernel": table}
    assert len(seen) == len(claims), sorted(seen)
    for name, got in seen.items():
        claim = [v for k, v in claims.items() if k in name]
        assert len(claim) == 1, name
        assert got["scratch"] == 0 and got["spills"] == 0, (name, got)
        assert got["lds"] == claim[0] and got["vgpr"] + got["agpr"] <= 64, (name, got)


def test_the_rank_kernels_keep_the_resources_they_had_before_the_phases(tmp_path):
    """The phases are host code: csrc/retrieve_rank.hip still holds the same 21 kernels, and each has the VGPRs, AGPRs, SGPRs, LDS
    and (no) scratch recorded from the commit before the *_phase entries (tests/golden/rank_kernel_notes.json)."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "rank_kernel_notes.json")))
    seen = _notes(tmp_path, "retrieve_rank.hip")
    assert len(want) == 21 and sorted(seen) == sorted(want)
    for name, got in seen.items():
        assert got["spills"] == 0 and {k: got[k] for k in want[name]} == want[name], (name, got, want[name])
