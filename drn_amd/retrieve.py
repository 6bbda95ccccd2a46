"""The first stage of a two-stage search, on the device: each sentence's best n videos by the dot product of CALLER-SUPPLIED embeddings.

The project has no video-level embedding of its own (DRN has none) and this module invents none: the (V, E) table and the (S, E)
queries come from any dual encoder.  What it supplies is the ranking -- under a TOTAL order (score descending, then store position
ascending), so that equal scores fall the same way in every run and every build, which torch.topk does not promise -- and a result
that never leaves the device: Shortlist.ids is what Grounder.search(candidates=) takes as a device tensor.

shortlist_reference is the definition, in plain torch; Shortlister.shortlist is drn_shortlist_topn (csrc/retrieve.hip).

A dual encoder hands out one embedding per clip, shot or window rather than one per video.  Shortlister(offsets=) takes such a RAGGED
table -- R segment rows, video v owning the rows offsets[v] .. offsets[v + 1] - 1, the FeatureStore's seg_off layout -- scores a video
by its BEST segment and lists distinct videos, with the winning segment beside each: segment_shortlist_reference is that definition,
drn_shortlist_segments_topn (csrc/retrieve_seg.hip) the launch, plan_segment_blocks its host-side block plan.

Shortlister(quantize="mxfp8") and Shortlister.from_mx8 keep either table in block-scaled FP8 (the index's MX layout, drn_amd.index.mx8_quantize:
E + E / 32 bytes a row instead of 2 E or 4 E) and rank it with drn_shortlist_topn_q8 / drn_shortlist_segments_topn_q8
(csrc/retrieve_q8.hip).  A dequantised value is exact in bfloat16 and float32, so no new definition is needed: the quantised shortlist IS
shortlist_reference(mx8_dequantize(codes, scales), queries, n) -- with offsets, segment_shortlist_reference of the same dequantised
table -- and the kernels answer bit for bit like shortlister.dequantized(), a plain Shortlister over those rows.  Quantising the table
is lossy against the ORIGINAL embeddings (|dq - x| <= max(|x| / 16, 2^e / 1024) per element); the ranking of what the table holds is not.

shortlist(allow=) FILTERS any of the four tables on the device: a packed mask -- ceil(V / 32) int32 words, one row for all sentences or
one per sentence, made by pack_allow from a bool tensor or by Shortlister.allow_of from host names or positions -- says which videos a
sentence may list (a metadata filter, deleted videos, per-user visibility).  A video whose bit is clear is no candidate, exactly like
one whose score is not finite: shortlist_reference(..., allow=) and segment_shortlist_reference(..., allow=) are the definition, the
four *_allow entries (csrc/retrieve_allow.hip) the launches, and a listed score has the bits the unfiltered shortlist gives it.

Shortlister.shortlist_late takes the QUERY side multi-vector too (late interaction, as token-level dual encoders score): queries
(S, L, E), one vector per token, lengths (S,) on the device saying how many are live, and a video's score is the sum over the live
tokens of the token's best row of the video.  late_shortlist_reference is the definition, drn_shortlist_late_topn
(csrc/retrieve_late.hip) the launch, on a ragged table plain or quantised, with or without a mask.

Shortlister.shortlist_deep is shortlist() up to SHORTLIST_DEEP_MAX = 1024 videos a sentence -- the width rerank and
Grounder.search(candidates=) take -- on all four tables, with or without a mask: the same definitions, drn_shortlist_deep the one
entry (the masked phase one, then the merge of csrc/retrieve_deep.hip).

Shortlister.rank and rank_late answer what a list of at most SHORTLIST_MAX cannot: the place of a NAMED video in the FULL order -- how
many candidates precede targets[s], over the whole table, with its score and the number of candidates -- from the kernels' own scores
and total order, without a list, a sort or a host read.  rank_reference, segment_rank_reference and late_rank_reference are the
definitions, drn_shortlist_rank / _segments_rank / _late_rank (csrc/retrieve_rank.hip) the launches, on all the tables above, with or
without a mask; drn_amd.search_eval.evaluate_shortlist turns the ranks of annotated sentences into recall at any depth.

Shortlister.rerank and rerank_late are the SECOND stage of a cascade: they take another shortlist's ids as they lie on the device --
candidates_mask defines what such a tensor means: a set per sentence, -1 and out-of-range entries meaning nothing, repeats counting
once -- and score only the listed (sentence, video) pairs, with the bits and the total order of the full filtered shortlists.
rerank_reference, segment_rerank_reference and late_rerank_reference are the definitions (the existing ones under the mask "listed, and
allowed"), drn_shortlist_rerank (csrc/retrieve_rerank.hip) the one launch, on all the tables above; a coarse table, a fine rerank and
Grounder.search(candidates=) never leave the device, and drn_amd.search_eval.evaluate_cascade says what depth the coarse stage needs.

ShardedShortlister keeps a corpus as SEVERAL Shortlisters -- appended without a rebuild, plain and quantised side by side -- at the
corpus positions bases[k] + position in shard k.  Each shard ranks itself with its own entry; drn_shortlist_merge_lists
(csrc/retrieve_shard.hip) merges the per-shard lists under the one total order and drn_allow_slices cuts a mask over the corpus into
the shards' own.  A score's bits do not depend on the table that holds the video and the best n of a set are among the best n of each
part, so the answer is the single table's, bit for bit: merge_shortlists_reference and slice_allow_reference are the definitions.

ShardedShortlister.rank / rank_late / rerank / rerank_late answer over the shards what the single table's methods answer over the
concatenated rows, bit for bit, and need NO new definition of the answer: rank_reference, segment_rank_reference, late_rank_reference and
the three *_rerank_reference functions over the concatenated rows are it.  drn_shard_positions turns corpus positions into each shard's
local ones (shard_positions_reference).  A rank runs each shard's target kernel, turns the one key that is not 0 into a threshold per
shard (rank_thresholds_reference, drn_shortlist_rank_thresholds: an equal score precedes the target in an earlier shard and follows it
in a later one), runs each shard's counting kernel against its threshold and sums the counts (drn_shortlist_rank_reduce_shards).  A
rerank is each shard's rerank of the candidates that fall inside it, merged by drn_shortlist_merge_lists.

ShardedShortlister.compact is the third verb of a corpus that changes, beside append() and allow_of(drop=): ONE new table over the
videos a packed mask keeps, in corpus order, the dropped ones gone, with the map from old positions to new ones.  compact_reference is
the definition.  drn_compact_plan (csrc/retrieve_compact.hip), once per shard, scans the mask -- and a ragged shard's offsets -- into
new positions and new offsets with a carry that runs from shard to shard; after ONE synchronise (the carry, the mask words for the
names, the new offsets for the block plan: no table data) drn_compact_rows, once per shard, moves the kept rows: plain rows and FP8
codes and scales as they are, FP8 rows dequantised exactly where the target is plain; plain rows on their way to FP8 cross a bounded
staging buffer into ops.quantize_rows_mx8, the one quantiser.  Where nothing is quantised the new table answers every method bit for
bit as the shards do under allow=keep, positions mapped.

Shortlister.pooled and ShardedShortlister.pooled are the fourth verb: a CHEAPER table over the same videos, made on the device from the
ragged table the caller owns -- one row a video (group=None) or one row per g rows of a video (group=g), the mean or the maximum, from a
plain or an FP8 table into either format.  pool_segments_reference is the definition, bit for bit: an fp32 sum in ascending row order,
one IEEE division, one rounding; drn_pool_segments (csrc/retrieve_pool.hip) the launch, one wavefront per pooled row and column slab.
Store positions and names are unchanged, so the pooled table is the `coarse` of evaluate_cascade beside its source as `fine`; with
group=None a video without rows is a row of zeros and table.nonempty the mask that keeps it off the lists.

Shortlister.scores / scores_late (and ShardedShortlister's) hand out the DENSE score matrix the lists are cut from: float32 (S, V), a
written score with the bits the list would show, -inf where the video is no candidate (scores_reference; drn_shortlist_scores,
csrc/retrieve_fuse.hip, one launch).  shortlist_scores ranks any such matrix under the total order, and FusedShortlister ranks SEVERAL
tables over the same videos as one -- w_0 * best window + w_1 * best subtitle line, each table taking its own maximum over its own rows
-- by a fold whose order is stated (fuse_scores_reference: acc = acc + (w_m * s_m), m ascending, fp32, two roundings a term;
fused_shortlist_reference and fused_rank_reference cut the list and take the rank; drn_shortlist_fuse_topn / _rank the launches).

Shortlister.rerank_scores / rerank_scores_late (and ShardedShortlister's) are the listed-pairs counterpart of scores(): float32 (S, C),
column j the score rerank() would list for the pair (s, candidates[s, j]) and -inf where the slot is no candidate
(rerank_scores_reference; drn_shortlist_rerank_scores, csrc/retrieve_rerank.hip: the rerank kernel up to its sums, one launch), and
fused_rerank(fused, candidates, queries, n) is the fused SECOND stage of a cascade: M such matrices, unmasked, then one ranking of
candidate slots under the fold and the total order above (fused_rerank_reference: the fused shortlist under the mask "listed, and
allowed"; drn_shortlist_fuse_rerank, csrc/retrieve_fuse.hip).  Only the listed videos' rows of every table are read.

rank_fuse / rank_fuse_rank and RankFusedShortlister fuse BY RANK, for tables whose scores share no scale (a dot product against a sum
over 64 tokens): reciprocal-rank fusion of M finished id lists -- list m votes w[m] / (k0 + rank + 1) for each video it holds, the rank
being the column of the video's first occurrence, the votes added in fp32 in list order, the sums ranked under the total order, which
decides the constant ties of reciprocal ranks the same way in every run.  rank_fuse_reference and rank_fuse_rank_reference are the
definitions, drn_rank_fuse_topn / _rank (csrc/retrieve_rrf.hip) the launches: one workgroup a sentence sorts the M * C <= 8192 entries
in LDS, folds and sorts again; no dense buffer, no second read of any table."""
import collections
import numbers

import numpy as np
import torch

from . import ops
from ._lib import (FUSE_MAX_TABLES, FUSE_MODES, LATE_MAX_TOKENS, RANK_FUSE_MAX_LISTS, RERANK_MAX_CANDIDATES, SHARDS_MAX, SHORTLIST_BLOCK, SHORTLIST_DEEP_MAX, SHORTLIST_MAX, SHORTLIST_SEG_BLOCK,
                   DrnError)      # SHORTLIST_MAX = 128 and SHARDS_MAX = 64 are CHOICES, not measurements (see _lib.py, include/drn_hip.h)
from .index import MX8_BLOCK, MX8_EMIN, QUANTIZE, mx8_dequantize, mx8_quantize

Shortlist = collections.namedtuple("Shortlist", "ids scores n")
Shortlist.__doc__ = """ids (S, n) int32 store positions, best first, -1 past the list; scores (S, n) float32, 0 past the list; n (S,) int32 the
length of each sentence's list.  All on the device."""


def _allowed(allow, S, V, device):
    """A reference's allow= -> a bool tensor that broadcasts against (S, V): (V,) is shared by all sentences, (S, V) has a row each."""
    if not torch.is_tensor(allow) or allow.dtype != torch.bool or tuple(allow.shape) not in ((V,), (S, V)):
        raise DrnError("allow must be a bool tensor (%d,) or (%d, %d): one entry per video, shared or per sentence" % (V, S, V))
    return allow.to(device)


def shortlist_reference(embeddings, queries, n, allow=None):
    """THE DEFINITION of a shortlist, in float64 (usable on the CPU): score[s, v] = sum_e queries[s, e] * embeddings[v, e]; sentence s
    lists the videos whose score is finite, ordered by higher score, then lower position, cut to n.  Past the list ids = -1 and
    scores = 0; n[s] is its length (a NaN query row lists nothing).  allow: a bool tensor (V,), shared by all sentences, or (S, V), one
    row per sentence: a video with allow == False is no candidate for that sentence, exactly like one whose score is not finite (its
    score, NaN or the best, changes nothing for the others).  -> Shortlist on the inputs' device, scores rounded to float32."""
    score, finite = _plain_scores(embeddings, queries, allow)
    ids, scores, count, _ = _listed(score, finite, int(n))
    return Shortlist(ids, scores, count)


def _plain_scores(embeddings, queries, allow):
    """What shortlist_reference and rank_reference share -> score (S, V) float64 and candidate (S, V) bool: the score is finite and the
    video allowed."""
    emb, q = embeddings.double(), queries.double()
    V, S = int(emb.shape[0]), int(q.shape[0])
    score = q @ emb.t()
    finite = torch.isfinite(score)
    if allow is not None:
        finite = finite & _allowed(allow, S, V, emb.device)
    return score, finite


def _listed(score, finite, n):
    """The list every reference cuts from its scores (S, V) and candidates -> ids, scores (S, n), count (S,) int32 and the (S, m)
    positions listed, m = min(n, V), with the bool (S, m) that says which of them lie inside the list."""
    S, V = (int(x) for x in score.shape)
    dev = score.device
    key = torch.where(finite, score, torch.full_like(score, float("-inf")))
    # a stable sort by descending score keeps equal scores in position order
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    count = finite.sum(dim=1).clamp(max=n)
    ids = torch.full((S, n), -1, dtype=torch.int32, device=dev)
    scores = torch.zeros((S, n), dtype=torch.float32, device=dev)
    m = min(n, V)
    listed = torch.arange(m, device=dev)[None, :] < count[:, None]
    ids[:, :m] = torch.where(listed, order[:, :m].to(torch.int32), ids[:, :m])
    scores[:, :m] = torch.where(listed, torch.gather(score, 1, order[:, :m]).float(), scores[:, :m])
    return ids, scores, count.to(torch.int32), (order[:, :m], listed)


TargetRank = collections.namedtuple("TargetRank", "rank score total")
TargetRank.__doc__ = """rank (S,) int32: how many candidates precede the sentence's target video in the FULL shortlist order (score
descending, then position ascending), -1 where the target is no candidate; score (S,) float32: the target's score, 0 beside -1; total
(S,) int32: the sentence's candidates, the length of its list were n unbounded.  All on the device."""


def _ranked(score, finite, targets):
    """The rank every rank reference takes from its scores (S, V) and candidates -> TargetRank."""
    S, V = (int(x) for x in score.shape)
    dev = score.device
    t = torch.as_tensor(targets, device=dev).to(torch.int64).reshape(-1)
    if int(t.shape[0]) != S:
        raise DrnError("rank reference: %d targets for %d sentences" % (int(t.shape[0]), S))
    tc = t.clamp(0, V - 1)[:, None]
    ts = torch.gather(score, 1, tc)                                                # (S, 1) the target's score
    found = ((t >= 0) & (t < V))[:, None] & torch.gather(finite, 1, tc)
    before = finite & ((score > ts) | ((score == ts) & (torch.arange(V, device=dev)[None, :] < tc)))
    rank = torch.where(found[:, 0], before.sum(dim=1), torch.full((S,), -1, dtype=torch.int64, device=dev))
    value = torch.where(found[:, 0], ts[:, 0], torch.zeros_like(ts[:, 0]))
    return TargetRank(rank.to(torch.int32), value.float(), finite.sum(dim=1).to(torch.int32))


def rank_reference(embeddings, queries, targets, allow=None):
    """THE DEFINITION of a target's rank, in float64 (usable on the CPU).  Scores and candidates are shortlist_reference's: a video is
    a candidate of sentence s when its score is finite and allow does not exclude it.  targets: S integers (a sequence or a tensor);
    with t = targets[s], total[s] = the candidates of s; where 0 <= t < V and t is a candidate, rank[s] = the candidates u with
    score[s, u] > score[s, t], or score[s, u] == score[s, t] and u < t, and score[s] = t's score rounded to float32; otherwise
    rank[s] = -1 and score[s] = 0 (a value outside [0, V) is legal and means "no target").  So rank[s] = k >= 0 exactly when
    shortlist_reference(..., n).ids[s, k] == t for every n > k.  Over the concatenated (dequantised) rows of its shards this IS the
    definition of ShardedShortlister.rank too; so are segment_rank_reference and late_rank_reference with the offsets of each shard
    shifted by the running row count.  -> TargetRank on the inputs' device."""
    return _ranked(*_plain_scores(embeddings, queries, allow), targets)


def segment_rank_reference(embeddings, offsets, queries, targets, allow=None):
    """rank_reference with the scores and candidates of segment_shortlist_reference: a video scores by its best row and is a candidate
    when it owns a row, its score is finite and allow (over VIDEOS) does not exclude it.  -> TargetRank."""
    score, _, finite = _segment_scores(embeddings, offsets, queries, allow)
    return _ranked(score, finite, targets)


def late_rank_reference(embeddings, offsets, queries, lengths, targets, allow=None):
    """rank_reference with the scores and candidates of late_shortlist_reference: queries (S, L, E), lengths (S,); a video scores by
    the sum over the live tokens of its best row and is a candidate when it owns a row, the sum is finite, allow does not exclude it
    and the sentence has a live token (one without has total = 0 and rank = -1).  -> TargetRank."""
    return _ranked(*_late_scores(embeddings, offsets, queries, lengths, allow), targets)


def scores_reference(embeddings, queries, offsets=None, lengths=None, allow=None):
    """THE DEFINITION of Shortlister.scores / scores_late (usable on the CPU): the WHOLE score matrix the shortlist references cut
    their lists from -> float32 (S, V) on the inputs' device.  Without offsets: shortlist_reference's scores (_plain_scores); with
    offsets: segment_shortlist_reference's, a video's best row (_segment_scores); with offsets and lengths: late_shortlist_reference's,
    queries (S, L, E) (_late_scores) -- computed in float64 and rounded to float32, a -0 returned as +0.  Where the video is NO
    CANDIDATE of the sentence -- it owns no row, its score is not finite (in float32), allow excludes it or (late) the sentence has no
    live token -- the entry is -inf: finite <=> candidate, and no NaN is ever returned.  No arithmetic of its own."""
    if lengths is not None:
        if offsets is None:
            raise DrnError("scores_reference: lengths (late interaction) need offsets: a ragged table")
        score, finite = _late_scores(embeddings, offsets, queries, lengths, allow)
    elif offsets is not None:
        score, _, finite = _segment_scores(embeddings, offsets, queries, allow)
    else:
        score, finite = _plain_scores(embeddings, queries, allow)
    value = torch.where(finite, score, torch.zeros_like(score)).float() + 0.0      # (-0 + 0 = +0)
    return torch.where(finite & torch.isfinite(value), value, torch.full_like(value, float("-inf")))


def _fuse_inputs(what, scores, weights, missing):
    """What the fuse references take -> (scores (M, S, V) float32 ON THE HOST, weights (M,) float32 on the host, the scores' device)."""
    if missing not in FUSE_MODES:
        raise DrnError("%s: missing must be \"drop\" or \"skip\", not %r" % (what, missing))
    if not torch.is_tensor(scores):
        try:
            scores = torch.stack(list(scores))
        except Exception:
            raise DrnError("%s: scores must be an (M, S, V) float32 tensor or a sequence of M (S, V) float32 tensors" % what)
    if scores.dim() != 3 or scores.dtype != torch.float32 or not 1 <= scores.shape[0] <= FUSE_MAX_TABLES or scores.shape[1] < 1 \
            or scores.shape[2] < 1:
        raise DrnError("%s: scores must be (M, S, V) float32 with 1 <= M <= %d, S >= 1 and V >= 1, not %s %s"
                       % (what, FUSE_MAX_TABLES, scores.dtype, tuple(scores.shape)))
    M = int(scores.shape[0])
    w = torch.ones(M, dtype=torch.float32) if weights is None else torch.as_tensor(weights).detach().cpu()
    if tuple(w.shape) != (M,) or w.dtype == torch.bool or w.is_complex():
        raise DrnError("%s: weights must be %d numbers, one per score matrix, not %s %s" % (what, M, w.dtype, tuple(w.shape)))
    return scores.detach().cpu(), w.to(torch.float32), scores.device


def fuse_scores_reference(scores, weights, missing="drop"):
    """THE DEFINITION of the fused score, EVALUATED ON THE HOST in float32 whatever device the inputs live on -> (fused (S, V) float32,
    candidate (S, V) bool) on the scores' device.  scores: (M, S, V) float32, or a sequence of M (S, V) matrices, 1 <= M <=
    FUSE_MAX_TABLES -- what Shortlister.scores returns: an entry that is not finite says the video is MISSING from that table;
    weights: M numbers (None: all ones), rounded to float32.  The order is FIXED, one float32 multiply and one float32 add a term,
    each rounded on its own (not an FMA, and not a sum whose order nobody states):
        acc = +0;  for m = 0 .. M - 1 ascending:  present = isfinite(scores[m]);
            missing="drop":  acc = acc + (w[m] * scores[m]);      missing="skip":  acc = where(present, acc + (w[m] * scores[m]), acc)
        candidate = isfinite(acc) and (drop: every m present | skip: some m present).
    Under "drop" a video missing from any table is missing from the answer; under "skip" a modality the video lacks adds nothing.
    With M = 1 and w = 1 the candidates are the finite entries and the fused score is the entry (0 + 1 * s, exact; a -0 becomes +0)."""
    sc, w, dev = _fuse_inputs("fuse_scores_reference", scores, weights, missing)
    M = int(sc.shape[0])
    acc = torch.zeros(tuple(sc.shape[1:]), dtype=torch.float32)
    every, some = torch.ones(tuple(sc.shape[1:]), dtype=torch.bool), torch.zeros(tuple(sc.shape[1:]), dtype=torch.bool)
    for m in range(M):
        present = torch.isfinite(sc[m])
        term = w[m] * sc[m]                                  # (one rounding)
        added = acc + term                                   # (one more)
        acc = added if missing == "drop" else torch.where(present, added, acc)
        every, some = every & present, some | present
    candidate = torch.isfinite(acc) & (every if missing == "drop" else some)
    return acc.to(dev), candidate.to(dev)


def fused_shortlist_reference(scores, weights, n, missing="drop", allow=None):
    """THE DEFINITION of FusedShortlister.shortlist and of shortlist_scores (M = 1, w = 1): the list every reference cuts, from
    fuse_scores_reference's fused scores and candidates -- a candidate that allow (a bool tensor (V,) or (S, V)) excludes is none --
    ordered by higher fused score, then lower position, cut to n; -1 / 0 past the list.  -> Shortlist on the scores' device."""
    fused, candidate = fuse_scores_reference(scores, weights, missing)
    if allow is not None:
        candidate = candidate & _allowed(allow, int(fused.shape[0]), int(fused.shape[1]), fused.device)
    ids, listed, count, _ = _listed(fused.double(), candidate, int(n))
    return Shortlist(ids, listed, count)


def fused_rank_reference(scores, weights, targets, missing="drop", allow=None):
    """THE DEFINITION of FusedShortlister.rank: rank_reference's answer (_ranked) from fuse_scores_reference's fused scores and
    candidates, allow applied as in fused_shortlist_reference.  -> TargetRank on the scores' device."""
    fused, candidate = fuse_scores_reference(scores, weights, missing)
    if allow is not None:
        candidate = candidate & _allowed(allow, int(fused.shape[0]), int(fused.shape[1]), fused.device)
    return _ranked(fused.double(), candidate, targets)


def candidates_mask(candidates, V):
    """THE DEFINITION of what a candidates tensor means (usable on the CPU): candidates (S, C) integers, row s = the SET of store
    positions sentence s may list -> bool (S, V) on its device, mask[s, v] true iff some column of row s equals v.  An entry outside
    [0, V) means nothing -- the -1 padding of a Shortlist is one -- and a position listed twice counts once; the order of a row means
    nothing.  This is the meaning Grounder.search gives a device candidates tensor."""
    if not torch.is_tensor(candidates) or candidates.dim() != 2 or candidates.is_floating_point() or candidates.is_complex() \
            or candidates.dtype == torch.bool:
        raise DrnError("candidates_mask: candidates must be an integer tensor (S, C), a row of store positions per sentence")
    V = int(V)
    c = candidates.to(torch.int64)
    S = int(c.shape[0])
    valid = (c >= 0) & (c < V)
    mask = torch.zeros((S, V + 1), dtype=torch.bool, device=c.device)            # (column V collects what means nothing)
    mask.scatter_(1, torch.where(valid, c, torch.full_like(c, V)), torch.ones_like(valid))
    return mask[:, :V].contiguous()


def _listed_and_allowed(candidates, S, V, allow, device):
    """candidates_mask(candidates, V) & allow, the mask of a rerank reference -> bool (S, V)."""
    mask = candidates_mask(candidates, V).to(device)
    if int(mask.shape[0]) != S:
        raise DrnError("rerank reference: %d rows of candidates for %d sentences" % (int(mask.shape[0]), S))
    return mask if allow is None else mask & _allowed(allow, S, V, device)


def rerank_reference(embeddings, candidates, queries, n, allow=None):
    """THE DEFINITION of a reranked list on a table of one row per video, in float64 (usable on the CPU): shortlist_reference with
    allow replaced by candidates_mask(candidates, V) & allow.  Score, candidate-hood (finite score, listed, allowed) and the total
    order (score descending, then store position ascending) are shortlist_reference's: the order of the input list means nothing, and
    ties fall by store position, not by place in the list.  n > C is legal: past the list ids = -1 and scores = 0.  Over the
    concatenated (dequantised) rows of its shards, with CORPUS positions in candidates, this IS the definition of
    ShardedShortlister.rerank too; so are segment_rerank_reference and late_rerank_reference with the offsets of each shard shifted
    by the running row count.  -> Shortlist."""
    V, S = int(embeddings.shape[0]), int(queries.shape[0])
    return shortlist_reference(embeddings, queries, n, allow=_listed_and_allowed(candidates, S, V, allow, embeddings.device))


def segment_rerank_reference(embeddings, offsets, candidates, queries, n, allow=None):
    """rerank_reference on a RAGGED table: segment_shortlist_reference with allow replaced by candidates_mask(candidates, V) & allow,
    without its rows -- a listed video scores by its best row and is a candidate when it owns one.  -> Shortlist."""
    V, S = len(offsets) - 1, int(queries.shape[0])
    out = segment_shortlist_reference(embeddings, offsets, queries, n, allow=_listed_and_allowed(candidates, S, V, allow, embeddings.device))
    return Shortlist(out.ids, out.scores, out.n)


def late_rerank_reference(embeddings, offsets, candidates, queries, lengths, n, allow=None):
    """rerank_reference by LATE INTERACTION: late_shortlist_reference with allow replaced by candidates_mask(candidates, V) & allow
    (queries (S, L, E), lengths (S,); a sentence without a live token lists nothing).  -> Shortlist."""
    V, S = len(offsets) - 1, int(queries.shape[0])
    return late_shortlist_reference(embeddings, offsets, queries, lengths, n,
                                    allow=_listed_and_allowed(candidates, S, V, allow, embeddings.device))


def _first_occurrences(what, candidates, S, V):
    """candidates (S, C) integers -> (positions (S, C) int64, first (S, C) bool): slot j of a row is a FIRST OCCURRENCE when its id lies
    in [0, V) and no earlier slot of the row holds the same id -- the slots whose set candidates_mask describes."""
    if not torch.is_tensor(candidates) or candidates.dim() != 2 or candidates.is_floating_point() or candidates.is_complex() \
            or candidates.dtype == torch.bool:
        raise DrnError("%s: candidates must be an integer tensor (S, C), a row of store positions per sentence" % what)
    if int(candidates.shape[0]) != S:
        raise DrnError("%s: %d rows of candidates for %d sentences" % (what, int(candidates.shape[0]), S))
    c = candidates.to(torch.int64)
    C = int(c.shape[1])
    earlier = torch.ones((C, C), dtype=torch.bool, device=c.device).tril(-1)      # [j, i]: i < j
    repeat = ((c[:, :, None] == c[:, None, :]) & earlier[None]).any(dim=2)
    return c, (c >= 0) & (c < V) & ~repeat


def rerank_scores_reference(embeddings, candidates, queries, offsets=None, lengths=None, allow=None):
    """THE DEFINITION of Shortlister.rerank_scores / rerank_scores_late (usable on the CPU) -> float32 (S, C) on the inputs' device:
    scores_reference(embeddings, queries, offsets, lengths, allow=allow) gathered at each slot's id, with -inf where the id lies
    outside [0, V) and -inf where the id occurred EARLIER in the row (of a repeated position the first slot carries the score).  So a
    slot is finite exactly when it is the first occurrence of a candidate of the sentence, and the finite slots of a row are the
    scores of the set candidates_mask describes.  No arithmetic of its own."""
    full = scores_reference(embeddings, queries, offsets=offsets, lengths=lengths, allow=allow)
    S, V = (int(x) for x in full.shape)
    c, first = _first_occurrences("rerank_scores_reference", candidates, S, V)
    c, first = c.to(full.device), first.to(full.device)
    return torch.where(first, torch.gather(full, 1, c.clamp(0, V - 1)), torch.full_like(full[:, :1], float("-inf")).expand(S, int(c.shape[1])))


def fused_rerank_reference(scores, weights, candidates, V, n, missing="drop", allow=None):
    """THE DEFINITION of fused_rerank (evaluated on the host, as fuse_scores_reference is): scores (M, S, C) float32 -- or a
    sequence of M (S, C) matrices -- column j of row s belonging to the video candidates[s, j], what rerank_scores returns.  Each row's
    FIRST OCCURRENCES (an id in [0, V) that no earlier slot of the row holds) are scattered into an (M, S, V) stack filled with -inf,
    and the answer is fused_shortlist_reference(stack, weights, n, missing, allow): the fused rerank IS the fused shortlist under the
    mask "listed, and allowed", so ties fall by store position and the place of a video in the list means nothing.  What a slot that
    is no first occurrence holds is ignored.  -> Shortlist on the scores' device."""
    what = "fused_rerank_reference"
    sc, w, dev = _fuse_inputs(what, scores, weights, missing)
    M, S, C = (int(x) for x in sc.shape)
    V = int(V)
    if V < 1:
        raise DrnError("%s: V = %d videos, at least one is needed" % (what, V))
    if torch.is_tensor(candidates) and candidates.dim() == 2 and int(candidates.shape[1]) != C:
        raise DrnError("%s: candidates has %d columns, the score matrices %d" % (what, int(candidates.shape[1]), C))
    c, first = _first_occurrences(what, candidates.detach().cpu() if torch.is_tensor(candidates) else candidates, S, V)
    stack = torch.full((M, S, V + 1), float("-inf"), dtype=torch.float32)        # (column V collects what is not listed)
    where = torch.where(first, c, torch.full_like(c, V))
    stack.scatter_(2, where[None].expand(M, S, C), sc)
    return fused_shortlist_reference(stack[:, :, :V].contiguous().to(dev), w, n, missing=missing, allow=allow)


def _check_k0(what, k0):
    """k0 of a rank fusion: a host number, rounded to float32, finite and >= 0 -> the rounded value as a Python float."""
    if isinstance(k0, bool) or not isinstance(k0, numbers.Real):
        raise DrnError("%s: k0 must be a host number, not %s" % (what, type(k0).__name__))
    with np.errstate(over="ignore"):
        k0 = float(np.float32(k0))
    if not 0.0 <= k0 < float("inf"):
        raise DrnError("%s: k0 = %r is not a finite number >= 0 (in float32)" % (what, k0))
    return k0


def _rank_fuse_lists(what, lists, V):
    """What the rank-fusion functions take as lists -> (a list of M (S, C_m) integer tensors on one device, S, V)."""
    V = int(V)
    if V < 1:
        raise DrnError("%s: V = %d videos, at least one is needed" % (what, V))
    if torch.is_tensor(lists):
        if lists.dim() != 3:
            raise DrnError("%s: a lists tensor must be (M, S, C), not %s" % (what, tuple(lists.shape)))
        lists = list(lists.unbind(0))
    else:
        try:
            lists = list(lists)
        except TypeError:
            raise DrnError("%s: lists must be an (M, S, C) tensor or a sequence of (S, C_m) tensors" % what)
    if not 1 <= len(lists) <= RANK_FUSE_MAX_LISTS:
        raise DrnError("%s: %d lists outside [1, %d]" % (what, len(lists), RANK_FUSE_MAX_LISTS))
    for m, t in enumerate(lists):
        if not torch.is_tensor(t) or t.dim() != 2 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise DrnError("%s: list %d must be an integer tensor (S, C), a row of store positions per sentence" % (what, m))
        if int(t.shape[0]) != int(lists[0].shape[0]) or t.shape[0] < 1:
            raise DrnError("%s: list %d holds %d sentences, list 0 holds %d" % (what, m, int(t.shape[0]), int(lists[0].shape[0])))
        if not 1 <= int(t.shape[1]) <= SHORTLIST_DEEP_MAX:
            raise DrnError("%s: list %d has C = %d entries a sentence outside [1, %d]" % (what, m, int(t.shape[1]), SHORTLIST_DEEP_MAX))
        if t.device != lists[0].device:
            raise DrnError("%s: list %d is on %s, list 0 on %s" % (what, m, t.device, lists[0].device))
    return lists, int(lists[0].shape[0]), V


def _rank_fuse_scores(what, lists, V, weights, k0, missing, allow):
    """What the two rank-fusion references share -> (fused (S, V) float32, candidate (S, V) bool) on the lists' device, by tensor
    operations alone: nothing is read on the host."""
    if missing not in FUSE_MODES:
        raise DrnError("%s: missing must be \"drop\" or \"skip\", not %r" % (what, missing))
    lists, S, V = _rank_fuse_lists(what, lists, V)
    M, dev = len(lists), lists[0].device
    k0 = torch.full((), _check_k0(what, k0), dtype=torch.float32, device=dev)
    if weights is None:
        w = torch.ones(M, dtype=torch.float32, device=dev)
    elif torch.is_tensor(weights):
        w = weights.to(dev)
    else:
        try:
            w = torch.tensor([float(x) for x in weights], dtype=torch.float32).to(dev)
        except (TypeError, ValueError):
            raise DrnError("%s: weights must be None, %d numbers or a float32 (%d,) tensor" % (what, M, M))
    if tuple(w.shape) != (M,) or w.dtype != torch.float32:
        raise DrnError("%s: weights must be %d float32 numbers, one per list, not %s %s" % (what, M, w.dtype, tuple(w.shape)))
    acc = torch.zeros((S, V), dtype=torch.float32, device=dev)
    held = torch.zeros((S, V), dtype=torch.int32, device=dev)
    for m, c in enumerate(lists):
        c = c.to(torch.int64)
        C = int(c.shape[1])
        valid = (c >= 0) & (c < V)
        # the column of the FIRST occurrence of every video: the minimum over the columns that hold it (column V collects the junk)
        first = torch.full((S, V + 1), C, dtype=torch.int64, device=dev)
        first.scatter_reduce_(1, torch.where(valid, c, torch.full_like(c, V)), torch.arange(C, device=dev)[None, :].expand(S, C), "amin")
        j = first[:, :V]
        holds = j < C
        term = w[m] / (k0 + (j + 1).to(torch.float32))          # (one add, one division: each rounded to float32 on its own)
        acc = torch.where(holds, acc + term, acc)
        held = held + holds.to(torch.int32)
    candidate = torch.isfinite(acc) & (held == M if missing == "drop" else held > 0)
    if allow is not None:
        candidate = candidate & _allowed(allow, S, V, dev)
    return acc + 0.0, candidate


def rank_fuse_reference(lists, V, n, weights=None, k0=60.0, missing="skip", allow=None):
    """THE DEFINITION of rank_fuse: reciprocal-rank fusion (RRF) of M id lists over the same V videos, in float32 (usable on the CPU,
    and on any device without a host synchronisation) -> Shortlist on the lists' device.  lists: an (M, S, C) integer tensor or a
    sequence of M (S, C_m) integer tensors, 1 <= M <= RANK_FUSE_MAX_LISTS, 1 <= C_m <= SHORTLIST_DEEP_MAX -- other shortlists' ids as
    they lie on the device.  The entries mean what candidates_mask says: a value outside [0, V) means nothing (-1, V, INT_MIN,
    INT_MAX), and of a position repeated in one row the first occurrence counts.  THE RANK of video v in list m is the column j of
    its first occurrence: for any list a shortlist produces that is its place in the list, because the padding sits at the end.
    weights: M numbers (None: all ones) or a float32 (M,) tensor; k0: a host number rounded to float32, finite and >= 0 (anything else
    is refused).  The order is FIXED, every operation rounded to float32 on its own:
        acc = +0;  for m = 0 .. M - 1 ascending, where list m holds v at rank j:  acc = acc + w[m] / (k0 + float(j + 1))
    missing="skip" (standard RRF): a list that does not hold v adds nothing, and v is a candidate when any list holds it;
    missing="drop": every list must hold v.  A video whose acc is not finite is no candidate (the weights may hold anything), nor is
    one that allow (a bool tensor (V,) or (S, V)) excludes.  The candidates are listed by higher acc, then lower position, cut to n;
    -1 / 0 past the list.  With M = 1 and w = 1 the ids are the list's distinct valid entries in order.
    What this is NOT: a fusion of scores -- the votes depend on the lists alone and so on the DEPTH they were cut at: a video just
    past a list's end gets nothing from it.  Subnormal terms follow IEEE here; the kernels are tested away from them."""
    fused, candidate = _rank_fuse_scores("rank_fuse_reference", lists, V, weights, k0, missing, allow)
    ids, listed, count, _ = _listed(fused.double(), candidate, _check_depth("rank_fuse_reference", n))
    return Shortlist(ids, listed, count)


def rank_fuse_rank_reference(lists, V, targets, weights=None, k0=60.0, missing="skip", allow=None):
    """THE DEFINITION of rank_fuse_rank: rank_reference's answer (_ranked) from rank_fuse_reference's fused scores and candidates, so
    rank[s] = k >= 0 exactly when rank_fuse_reference(..., n).ids[s, k] is the target for every n > k; total is the number of fused
    candidates.  -> TargetRank on the lists' device."""
    fused, candidate = _rank_fuse_scores("rank_fuse_rank_reference", lists, V, weights, k0, missing, allow)
    return _ranked(fused.double(), candidate, targets)


SegmentShortlist = collections.namedtuple("SegmentShortlist", "ids scores n rows")
SegmentShortlist.__doc__ = """ids, scores, n as in Shortlist (a video's score is its best segment's); rows (S, n) int32: the lowest segment number of
the video (table row - offsets[video]) that reaches that score, -1 past the list.  All on the device."""

SegmentPlan = collections.namedtuple("SegmentPlan", "blk_vid vid_blk")
SegmentPlan.__doc__ = """blk_vid (nblocks + 1,) int32: block b holds the videos blk_vid[b] .. blk_vid[b + 1] - 1; vid_blk (V,) int32: a video's block.
numpy arrays."""

SEGMENT_ROW_TARGET = 256  # rows a block of the plan aims at: a CHOICE (one pass of the ranking workgroup), not a measurement


def check_segment_offsets(offsets, R, names=None):
    """offsets (a sequence, a numpy array or a HOST tensor) for a table of R rows -> an int64 numpy array of V + 1 entries; raises
    unless they are integers, start at 0, never decrease, end at R, V >= 1 and 1 <= R < 2^31, and names (when given) has V entries."""
    R = int(R)
    if torch.is_tensor(offsets):
        if offsets.is_floating_point() or offsets.is_complex() or offsets.dtype == torch.bool:
            raise DrnError("Shortlister: the offsets must be integers, not %s" % offsets.dtype)
        offsets = offsets.detach().cpu().numpy()
    try:
        off = np.asarray(offsets)
    except Exception:
        raise DrnError("Shortlister: the offsets must be a sequence of V + 1 integers")
    if off.dtype.kind not in "iu":
        raise DrnError("Shortlister: the offsets must be integers, not %s" % off.dtype)
    if off.ndim != 1 or off.shape[0] < 2:
        raise DrnError("Shortlister: the offsets must be V + 1 integers with V >= 1, not %s" % (tuple(off.shape),))
    if not 1 <= R < 2 ** 31:
        raise DrnError("Shortlister: R = %d rows outside [1, 2^31)" % R)
    off = off.astype(np.int64)
    if int(off[0]) != 0 or int(off[-1]) != R:
        raise DrnError("Shortlister: the offsets must start at 0 and end at R = %d, not run from %d to %d" % (R, int(off[0]), int(off[-1])))
    if bool((np.diff(off) < 0).any()):
        raise DrnError("Shortlister: the offsets decrease at video %d" % int(np.argmax(np.diff(off) < 0)))
    if names is not None and len(names) != off.shape[0] - 1:
        raise DrnError("Shortlister: %d names for %d videos (the offsets have V + 1 entries)" % (len(names), off.shape[0] - 1))
    return off


def plan_segment_blocks(offsets, max_videos=SHORTLIST_SEG_BLOCK, row_target=SEGMENT_ROW_TARGET):
    """The block plan of a segmented shortlist, from host offsets (V + 1 non-decreasing integers) -> SegmentPlan.  The videos are walked
    in order; a block is closed when the next video would bring it over max_videos videos or over row_target rows, and a single video
    larger than row_target is a block of its own.  Every video lies whole inside exactly one block, so the merge never sees a video
    twice; max_videos may not exceed what one ranking workgroup sorts (SHORTLIST_SEG_BLOCK)."""
    if not 1 <= int(max_videos) <= SHORTLIST_SEG_BLOCK or int(row_target) < 1:
        raise DrnError("plan_segment_blocks: max_videos = %d outside [1, %d] or row_target = %d below 1"
                       % (int(max_videos), SHORTLIST_SEG_BLOCK, int(row_target)))
    lens = np.diff(np.asarray(offsets, dtype=np.int64)).tolist()
    starts, videos, rows = [0], 0, 0
    for v, length in enumerate(lens):
        if videos and (videos + 1 > max_videos or rows + length > row_target):
            starts.append(v)
            videos = rows = 0
        videos, rows = videos + 1, rows + length
    starts.append(len(lens))
    blk_vid = np.asarray(starts, dtype=np.int32)
    vid_blk = np.repeat(np.arange(len(starts) - 1, dtype=np.int32), np.diff(blk_vid))
    return SegmentPlan(blk_vid, vid_blk)


def segment_shortlist_reference(embeddings, offsets, queries, n, allow=None):
    """THE DEFINITION of a segmented shortlist, in float64 (usable on the CPU).  embeddings (R, E), queries (S, E); offsets: V + 1
    non-decreasing integers from 0 to R, video v owning the rows offsets[v] .. offsets[v + 1] - 1, row r being segment r - offsets[v]
    of its video.  score[s, v] = the maximum over v's rows of sum_e queries[s, e] * embeddings[r, e] (a NaN among them makes it NaN);
    rows[s, v] = the lowest segment number that reaches it.  Sentence s lists the videos that own a row and whose score is finite,
    ordered by higher score, then lower position, cut to n.  Past the list ids = -1, scores = 0 and rows = -1; n[s] is its length (a NaN
    query row lists nothing).  allow: as in shortlist_reference, a bool tensor (V,) or (S, V) over VIDEOS, not rows: a video with
    allow == False is no candidate for that sentence.  -> SegmentShortlist on the inputs' device, scores rounded to float32."""
    score, rows, finite = _segment_scores(embeddings, offsets, queries, allow)
    ids, scores, count, (order, listed) = _listed(score, finite, int(n))
    segs = torch.full(tuple(ids.shape), -1, dtype=torch.int32, device=ids.device)
    m = int(order.shape[1])
    segs[:, :m] = torch.where(listed, torch.gather(rows, 1, order).to(torch.int32), segs[:, :m])
    return SegmentShortlist(ids, scores, count, segs)


def _segment_scores(embeddings, offsets, queries, allow):
    """What segment_shortlist_reference and segment_rank_reference share -> score (S, V) float64, rows (S, V) int64 (the lowest
    segment that reaches it) and candidate (S, V) bool: the video owns a row, its score is finite and it is allowed."""
    emb, q = embeddings.double(), queries.double()
    dev = emb.device
    R, S = int(emb.shape[0]), int(q.shape[0])
    off = torch.as_tensor(check_segment_offsets(offsets, R), device=dev)
    V = int(off.shape[0]) - 1
    lens = off[1:] - off[:-1]
    video = torch.repeat_interleave(torch.arange(V, device=dev), lens)             # (R,) the video of a row
    segment = torch.arange(R, device=dev) - off[video]
    index = video[None, :].expand(S, R)
    dot = q @ emb.t()                                                               # (S, R)
    nan = torch.isnan(dot)
    clean = torch.where(nan, torch.full_like(dot, float("-inf")), dot)
    score = torch.full((S, V), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(1, index, clean, "amax", include_self=True)
    any_nan = torch.zeros((S, V), dtype=torch.float64, device=dev).scatter_add(1, index, nan.double()) > 0
    score = torch.where(any_nan, torch.full_like(score, float("nan")), score)
    reaches = clean == torch.gather(score, 1, index)
    rows = torch.full((S, V), R, dtype=torch.int64, device=dev).scatter_reduce(
        1, index, torch.where(reaches, segment[None, :].expand(S, R), torch.full_like(index, R)), "amin", include_self=True)
    finite = torch.isfinite(score) & (lens > 0)[None, :]
    if allow is not None:
        finite = finite & _allowed(allow, S, V, dev)
    return score, rows, finite


def late_shortlist_reference(embeddings, offsets, queries, lengths, n, allow=None):
    """THE DEFINITION of a shortlist by late interaction, in float64 (usable on the CPU).  embeddings (R, E) and offsets as in
    segment_shortlist_reference; queries (S, L, E), one vector per token; lengths (S,) integers, clamped into [0, L]: token t of sentence
    s is live iff t < lengths[s], and the contents of a token that is not live are ignored, NaN included.  sim[s, t, v] = the maximum
    over v's rows of sum_e queries[s, t, e] * embeddings[r, e] (a NaN among them makes it NaN); score[s, v] = the sum of sim[s, t, v]
    over the live tokens.  Sentence s lists the videos that own a row, that allow (a bool tensor (V,) or (S, V), as in the other
    references) does not exclude and whose score is finite, ordered by higher score, then lower position, cut to n; a sentence without a
    live token lists nothing.  Past the list ids = -1 and scores = 0; n[s] is its length.  With one token per sentence this is
    segment_shortlist_reference without its rows.  -> Shortlist on the inputs' device, scores rounded to float32."""
    ids, scores, count, _ = _listed(*_late_scores(embeddings, offsets, queries, lengths, allow), int(n))
    return Shortlist(ids, scores, count)


def _late_scores(embeddings, offsets, queries, lengths, allow):
    """What late_shortlist_reference and late_rank_reference share -> score (S, V) float64 and candidate (S, V) bool: the video owns a
    row, the sum is finite, the video is allowed and the sentence has a live token."""
    emb, q = embeddings.double(), queries.double()
    dev = emb.device
    R = int(emb.shape[0])
    S, L = int(q.shape[0]), int(q.shape[1])
    off = torch.as_tensor(check_segment_offsets(offsets, R), device=dev)
    V = int(off.shape[0]) - 1
    lens = off[1:] - off[:-1]
    live = torch.arange(L, device=dev)[None, :] < torch.as_tensor(lengths, device=dev).to(torch.int64).clamp(0, L)[:, None]      # (S, L)
    q = torch.where(live[:, :, None], q, torch.zeros_like(q))                       # (what a dead token holds never reaches a product)
    video = torch.repeat_interleave(torch.arange(V, device=dev), lens)             # (R,) the video of a row
    index = video[None, :].expand(S * L, R)
    dot = q.reshape(S * L, -1) @ emb.t()                                            # (S L, R)
    nan = torch.isnan(dot)
    clean = torch.where(nan, torch.full_like(dot, float("-inf")), dot)
    sim = torch.full((S * L, V), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(1, index, clean, "amax", include_self=True)
    any_nan = torch.zeros((S * L, V), dtype=torch.float64, device=dev).scatter_add(1, index, nan.double()) > 0
    sim = torch.where(any_nan, torch.full_like(sim, float("nan")), sim).reshape(S, L, V)
    score = torch.where(live[:, :, None], sim, torch.zeros_like(sim)).sum(dim=1)    # (S, V)
    finite = torch.isfinite(score) & (lens > 0)[None, :] & live.any(dim=1)[:, None]
    if allow is not None:
        finite = finite & _allowed(allow, S, V, dev)
    return score, finite


def pack_allow_reference(mask):
    """THE DEFINITION of a packed allow mask, in numpy: mask (V,) or (S, V) of booleans (an array, a sequence or a host tensor) -> int32
    words (W,) or (S, W), W = ceil(V / 32): bit v & 31 of word v >> 5 is mask[..., v], the bits at or past V are zero."""
    m = np.asarray(mask.detach().cpu().numpy() if torch.is_tensor(mask) else mask)
    if m.dtype != np.bool_ or m.ndim not in (1, 2) or m.shape[-1] < 1 or m.shape[0] < 1:
        raise DrnError("pack_allow_reference: the mask must be booleans (V,) or (S, V) with V >= 1 and S >= 1, not %s %s" % (m.dtype, m.shape))
    V = m.shape[-1]
    W = ops.allow_words(V)
    padded = np.zeros(m.shape[:-1] + (32 * W,), dtype=np.bool_)
    padded[..., :V] = m
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u4").astype(np.uint32).view(np.int32)


def pack_allow(mask, out=None):
    """mask: a contiguous bool tensor (V,) or (S, V) ON THE DEVICE -> the packed mask shortlist(allow=) takes, int32 (W,) or (S, W) with
    W = ceil(V / 32), on the device (pack_allow_reference defines it).  ONE launch on the current stream, no host synchronisation, and
    it can be captured in a graph: a filter computed on the device never leaves it.  out: written in place, every word, with zero bits
    past V, and returned."""
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise DrnError("pack_allow: the mask must be a tensor on the GPU; there is no CPU fallback (Shortlister.allow_of packs host lists)")
    if mask.dtype != torch.bool or mask.dim() not in (1, 2) or mask.shape[-1] < 1 or mask.shape[0] < 1 or not mask.is_contiguous():
        raise DrnError("pack_allow: the mask must be a contiguous bool tensor (V,) or (S, V) with V >= 1 and S >= 1, not %s %s"
                       % (mask.dtype, tuple(mask.shape)))
    shape = tuple(mask.shape[:-1]) + (ops.allow_words(mask.shape[-1]),)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=mask.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.device != mask.device or out.dtype != torch.int32 or tuple(out.shape) != shape \
            or not out.is_contiguous():
        raise DrnError("pack_allow: out must be a contiguous %s torch.int32 tensor on the mask's device" % (shape,))
    return ops.pack_allow(mask, out)


def slice_allow_reference(words, V, start, stop):
    """THE DEFINITION of a shard's piece of a packed mask, in numpy: words (W,) or (S, W) int32, W = ceil(V / 32) (an array or a host
    tensor), a packed mask over V videos -> pack_allow_reference of its unpacked bits [start, stop), 0 <= start < stop <= V: bit j of the
    result is bit start + j of the input, and the bits at or past stop - start are zero."""
    w = np.ascontiguousarray(words.detach().cpu().numpy() if torch.is_tensor(words) else words)
    V, start, stop = int(V), int(start), int(stop)
    if w.dtype != np.int32 or w.ndim not in (1, 2) or w.shape[-1] != ops.allow_words(V) or not 0 <= start < stop <= V:
        raise DrnError("slice_allow_reference: words must be int32 (W,) or (S, W) with W = ceil(V / 32) = %d and 0 <= start < stop <= V, "
                       "not %s %s with [%d, %d)" % (ops.allow_words(V), w.dtype, w.shape, start, stop))
    bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little").astype(np.bool_)
    return pack_allow_reference(bits[..., start:stop])


def merge_shortlists_reference(lists, bases, n):
    """THE DEFINITION of the merge of per-shard lists, in plain torch (usable on the CPU).  lists: K Shortlist or K SegmentShortlist
    tuples over the same S sentences (widths may differ); bases: K + 1 integers, shard k holding the corpus positions bases[k] ..
    bases[k + 1] - 1.  Entry (k, s, i) is a candidate iff i < min(lists[k].n[s], width of list k), 0 <= ids[s, i] < bases[k + 1] -
    bases[k] and its score is finite; sentence s lists its candidates by higher score, then lower corpus position bases[k] + id, cut to
    n.  Past the list ids = -1, scores = 0 (and rows = -1); rows travel with their entry.  When every input is a shard's list of width
    >= n this is the list of the concatenated table (the best n of a set are among the best n of each part).  -> Shortlist, or
    SegmentShortlist when the inputs are, on their device."""
    lists, n = list(lists), int(n)
    bases = [int(b) for b in bases]
    if not lists or len(bases) != len(lists) + 1:
        raise DrnError("merge_shortlists_reference: %d lists need %d bases, not %d" % (len(lists), len(lists) + 1, len(bases)))
    ragged = len(lists[0]) == 4
    dev = lists[0][0].device
    S = int(lists[0][0].shape[0])
    pos, score, valid, rows = [], [], [], []
    for k, item in enumerate(lists):
        if (len(item) == 4) != ragged:
            raise DrnError("merge_shortlists_reference: the lists must all be Shortlists or all be SegmentShortlists")
        ids, sc, count = item[0].to(torch.int64), item[1].double(), item[2].to(torch.int64)
        width = int(ids.shape[1])
        ok = (torch.arange(width, device=dev)[None, :] < count.clamp(max=width)[:, None]) & (ids >= 0) & (ids < bases[k + 1] - bases[k])
        ok = ok & torch.isfinite(sc)
        pos.append(ids + bases[k]), score.append(sc), valid.append(ok)
        if ragged:
            rows.append(item[3].to(torch.int64))
    pos, score, valid = torch.cat(pos, dim=1), torch.cat(score, dim=1), torch.cat(valid, dim=1)
    # by corpus position first, so that the stable sort by score in _listed keeps equal scores in position order
    order = torch.sort(torch.where(valid, pos, torch.full_like(pos, 2 ** 62)), dim=1, stable=True).indices
    pos, score, valid = torch.gather(pos, 1, order), torch.gather(score, 1, order), torch.gather(valid, 1, order)
    _, scores, count, (at, listed) = _listed(score, valid, n)
    m = int(at.shape[1])
    ids = torch.full((S, n), -1, dtype=torch.int32, device=dev)
    ids[:, :m] = torch.where(listed, torch.gather(pos, 1, at).to(torch.int32), ids[:, :m])
    if not ragged:
        return Shortlist(ids, scores, count)
    segs = torch.full((S, n), -1, dtype=torch.int32, device=dev)
    segs[:, :m] = torch.where(listed, torch.gather(torch.gather(torch.cat(rows, dim=1), 1, order), 1, at).to(torch.int32), segs[:, :m])
    return SegmentShortlist(ids, scores, count, segs)


def shard_positions_reference(positions, bases):
    """THE DEFINITION of a shard's local positions, in plain torch (usable on the CPU): positions, an integer tensor (S,) or (S, C) of
    CORPUS positions (targets; candidate lists), and bases, K + 1 integers, shard k holding the corpus positions bases[k] ..
    bases[k + 1] - 1 -> int32 (K, S) / (K, S, C) on its device: out[k] = positions - bases[k] where bases[k] <= positions <
    bases[k + 1], else -1.  Computed in 64 bits, without wrap-around: INT_MIN, INT_MAX, -1 and V land in no shard.  Slice [k] is what
    shard k's rank and rerank take, where -1 means "no target" / "no candidate"."""
    if not torch.is_tensor(positions) or positions.dim() not in (1, 2) or positions.is_floating_point() or positions.is_complex() \
            or positions.dtype == torch.bool:
        raise DrnError("shard_positions_reference: positions must be an integer tensor (S,) or (S, C)")
    bases = [int(b) for b in bases]
    if len(bases) < 2:
        raise DrnError("shard_positions_reference: K + 1 bases with K >= 1, not %d" % len(bases))
    p = positions.to(torch.int64)
    return torch.stack([torch.where((p >= a) & (p < b), p - a, torch.full_like(p, -1)) for a, b in zip(bases[:-1], bases[1:])]).to(torch.int32)


def rank_thresholds_reference(keys):
    """THE DEFINITION of the per-shard counting thresholds of a rank over K shards, in numpy (usable on the CPU).  keys (K, S): each
    shard's 64-bit key of sentence s's target at its LOCAL position -- (word of the score << 32) | ~position, 0 where the shard does
    not hold a candidate target -- as integers that hold 64 bits: a numpy uint64 array, or a torch.int64 tensor holding the same bits;
    at most one key per column is not 0 (refused otherwise).  -> (thresholds (K, S), key (S,)) of the input's kind.  With kt the shard
    whose key tk is not 0 and tw = tk >> 32 (>= 1: a finite score's word is never 0): thresholds[k, s] = (tw << 32) - 1 for k < kt --
    an equal score in an earlier shard lies at a lower corpus position, so it precedes: every key of word >= tw counts --, tk for
    k == kt, (tw << 32) | 0xffffffff for k > kt -- an equal score in a later shard follows: only the words > tw count --, and
    key[s] = tk.  Where every key of the column is 0, thresholds = all ones (nothing counts as above) and key[s] = 0.  The rank of
    the target over the concatenated table is then the sum over the shards of their keys > thresholds[k, s]: rank_reference,
    segment_rank_reference and late_rank_reference over the concatenated rows stay THE definition of the answer."""
    tensor = torch.is_tensor(keys)
    if tensor:
        if keys.dtype != torch.int64 or keys.dim() != 2:
            raise DrnError("rank_thresholds_reference: keys must be (K, S) torch.int64 (or a numpy uint64 array), not %s %s"
                           % (keys.dtype, tuple(keys.shape)))
        k = keys.detach().cpu().contiguous().numpy().view(np.uint64)
    else:
        k = np.ascontiguousarray(keys)
        if k.dtype != np.uint64 or k.ndim != 2:
            raise DrnError("rank_thresholds_reference: keys must be a (K, S) numpy uint64 array (or a torch.int64 tensor), not %s %s"
                           % (k.dtype, k.shape))
    K, S = k.shape
    if K < 1:
        raise DrnError("rank_thresholds_reference: K >= 1 rows of keys, not %d" % K)
    nz = k != 0
    if bool((nz.sum(axis=0) > 1).any()):
        raise DrnError("rank_thresholds_reference: sentence %d has a target key in more than one shard" % int(np.argmax(nz.sum(axis=0) > 1)))
    has, kt = nz.any(axis=0), nz.argmax(axis=0)
    tk = k[kt, np.arange(S)]
    top = (tk >> np.uint64(32)) << np.uint64(32)
    at = np.arange(K)[:, None]
    ones = np.uint64(0xffffffffffffffff)
    thr = np.where(at < kt[None, :], (top - np.uint64(1))[None, :], np.where(at == kt[None, :], tk[None, :], (top | np.uint64(0xffffffff))[None, :]))
    thr = np.where(has[None, :], thr, ones).astype(np.uint64)
    key = np.where(has, tk, np.uint64(0)).astype(np.uint64)
    if tensor:
        return torch.from_numpy(thr.view(np.int64).copy()).to(keys.device), torch.from_numpy(key.view(np.int64).copy()).to(keys.device)
    return thr, key


def _allow_of(what, names, V, dev, keep, drop):
    """Shortlister.allow_of and ShardedShortlister.allow_of: HOST names or positions of a table of V videos -> a packed mask on dev."""
    if (keep is None) == (drop is None):
        raise DrnError("%s: exactly one of keep= and drop= must be given" % what)
    mask = np.zeros(V, dtype=np.bool_) if drop is None else np.ones(V, dtype=np.bool_)
    where = None
    for item in (keep if drop is None else drop):
        if isinstance(item, str):
            if names is None:
                raise DrnError("%s: %r is a name and this table has no names" % (what, item))
            if where is None:
                where = {name: v for v, name in enumerate(names)}
            if item not in where:
                raise DrnError("%s: no video named %r in this table" % (what, item))
            v = where[item]
        elif isinstance(item, (numbers.Integral, np.integer)) and not isinstance(item, (bool, np.bool_)):
            v = int(item)
            if not 0 <= v < V:
                raise DrnError("%s: position %d outside [0, %d)" % (what, v, V))
        else:
            raise DrnError("%s: an entry must be a name or a position, not %r" % (what, item))
        mask[v] = drop is None
    return _mask_words(mask, dev)


def _mask_words(mask, dev):
    """A HOST bool mask over the videos -> its packed words on dev: packed on the host (pack_allow_reference), ONE upload from pinned
    memory.  The tail of allow_of, and how pooled() makes nonempty from the offsets it holds on the host."""
    words = torch.from_numpy(pack_allow_reference(mask))
    if dev.type != "cuda":                    # (a table that is not on a GPU can be asked for its mask, never for a shortlist)
        return words
    return words.pin_memory().to(dev, non_blocking=True)


def _check_packed_allow(allow, S, V, dev):
    """The refusals of shortlist(allow=) over V videos on dev, before the library is reached."""
    W = ops.allow_words(V)
    if not torch.is_tensor(allow):
        raise DrnError("Shortlister.shortlist: allow must be a packed mask, a tensor (pack_allow or allow_of makes one)")
    if allow.dtype == torch.bool:
        raise DrnError("Shortlister.shortlist: allow is a bool tensor; pack it first -- allow=pack_allow(mask) -- into ceil(V / 32) "
                       "int32 words a row")
    if allow.dtype != torch.int32:
        raise DrnError("Shortlister.shortlist: allow must be torch.int32 packed words (pack_allow makes them), not %s" % allow.dtype)
    if not allow.is_cuda or allow.device != dev:
        raise DrnError("Shortlister.shortlist: allow must be on the table's device %s, not %s" % (dev, allow.device))
    if tuple(allow.shape) not in ((W,), (S, W)):
        raise DrnError("Shortlister.shortlist: allow must be (%d,) -- one mask for all sentences -- or (%d, %d), ceil(V / 32) words a "
                       "row for V = %d videos, not %s" % (W, S, W, V, tuple(allow.shape)))
    if not allow.is_contiguous():
        raise DrnError("Shortlister.shortlist: allow must be contiguous")


def _check_list_out(what, out, S, n, rows=False):
    """out= of a method that returns a Shortlist -- with rows, a SegmentShortlist: the buffers of its shapes and dtypes."""
    if rows and len(out) != 4:
        raise DrnError("%s: out must hold the four buffers of a SegmentShortlist (ids, scores, n, rows), not %d" % (what, len(out)))
    if not rows and len(out) != 3:
        raise DrnError("%s: out must hold the three buffers of a Shortlist (ids, scores, n), not %d" % (what, len(out)))
    for name, t, dt, shape in zip(SegmentShortlist._fields, out, (torch.int32, torch.float32, torch.int32, torch.int32),
                                  ((S, n), (S, n), (S,), (S, n))):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise DrnError("%s: out.%s must be a contiguous %s %s tensor on the GPU" % (what, name, shape, dt))


def _check_scores_out(what, out, S, V, dev):
    """out= of scores() / scores_late(): a float32 (S, V) tensor on dev whose rows are contiguous -- last stride 1, row stride >= V."""
    if not torch.is_tensor(out) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (S, V):
        raise DrnError("%s: out must be a (%d, %d) torch.float32 tensor on the table's device %s" % (what, S, V, dev))
    if (V > 1 and out.stride(1) != 1) or (S > 1 and out.stride(0) < V):
        raise DrnError("%s: out must have last stride 1 and row stride >= %d (a contiguous matrix, or a column slice of a wider one), "
                       "not strides %s" % (what, V, tuple(out.stride())))


def _list_buffers(dev, S, n, rows=False):
    """The result buffers (ids, scores, n[, rows]) of lists of n a sentence, made on dev."""
    out = (torch.empty((S, n), dtype=torch.int32, device=dev), torch.empty((S, n), dtype=torch.float32, device=dev),
           torch.empty((S,), dtype=torch.int32, device=dev))
    return out + (torch.empty((S, n), dtype=torch.int32, device=dev),) if rows else out


def _check_targets(what, S, targets, dev):
    """What every rank refuses about targets on dev, before the library is reached."""
    if not torch.is_tensor(targets) or targets.dtype != torch.int32 or tuple(targets.shape) != (S,) or not targets.is_contiguous():
        raise DrnError("%s: targets must be a contiguous (%d,) torch.int32 tensor, the store position of each sentence's video" % (what, S))
    if not targets.is_cuda or targets.device != dev:
        raise DrnError("%s: targets must be on the table's device %s (they are never read on the host)" % (what, dev))


def _check_rank_out(what, S, out):
    """out= of a method that returns a TargetRank: None, or the three buffers of its shapes and dtypes."""
    if out is not None:
        if len(out) != 3:
            raise DrnError("%s: out must hold the three buffers of a TargetRank (rank, score, total), not %d" % (what, len(out)))
        for name, t, dt in zip(TargetRank._fields, out, (torch.int32, torch.float32, torch.int32)):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != (S,) or not t.is_contiguous():
                raise DrnError("%s: out.%s must be a contiguous (%d,) %s tensor on the GPU" % (what, name, S, dt))


def _rank_buffers(dev, S):
    """The result buffers (rank, score, total) of S sentences, made on dev."""
    return (torch.empty((S,), dtype=torch.int32, device=dev), torch.empty((S,), dtype=torch.float32, device=dev),
            torch.empty((S,), dtype=torch.int32, device=dev))


def _refuse_late(what, instead, whose="this table has"):
    """The refusal of late interaction over one row per video; `instead` is the method that answers there."""
    raise DrnError("%s: %s one row per video (no offsets=), where late interaction is no new ranking -- sum_t q_t . emb_v = "
                   "(sum_t q_t) . emb_v: add each sentence's live token vectors and call %s()" % (what, whose, instead))


def quantized_score_bound(embeddings, scales, queries):
    """How far a quantised table's score may lie from the float64 score of the ORIGINAL table -> (S, rows) float64.  embeddings (rows,
    E) is the table before quantising and scales (rows, E / 32) the scale bytes mx8_quantize gave it.  The format rounds an element to
    within max(|x| / 16, 2^e / 1024) of itself (e4m3fn keeps four significant bits of a normal code, and its subnormal codes are 2^-9
    apart; e = scale - 127), so |q . dq - q . x| <= sum_e |q_e| * max(|x_e| / 16, 2^e_block / 1024); the fp32 accumulation of E products
    adds at most E * 2^-23 * sum_e |q_e * x_e| (tests/test_shortlist_gpu.py derives that term).  A best-segment score moves by no more
    than the largest bound among the video's rows."""
    x, q = embeddings.double(), queries.double()
    rows, E = (int(v) for v in x.shape)
    ulp = torch.ldexp(torch.ones((), dtype=torch.float64, device=x.device), scales.to(x.device).to(torch.int32) - 127 - 10)
    per = torch.maximum(x.abs() / 16, ulp.repeat_interleave(MX8_BLOCK, dim=1))
    return q.abs() @ per.t() + E * 2.0 ** -23 * (q.abs() @ x.abs().t())


Pooled = collections.namedtuple("Pooled", "rows offsets")
Pooled.__doc__ = """rows (R', E): the pooled rows in the table's dtype, on the HOST; offsets: None with group=None (row v is video v), else the pooled
table's own offsets, V + 1 int64 in a numpy array."""

def pool_offsets(offsets, group):
    """The offsets of a pooled table from the source's host offsets (V + 1 integers): a video of len_v rows keeps ceil(len_v / group)
    -> V + 1 int64 (a video without rows keeps none); group=None -> None: the pooled table has one row a video and no offsets."""
    if group is None:
        return None
    lens = np.diff(np.asarray(offsets, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(-(-lens // int(group)))]).astype(np.int64)


def pool_segments_reference(embeddings_or_shortlister, offsets=None, how="mean", group=None):
    """THE DEFINITION of Shortlister.pooled, in plain torch and numpy, EVALUATED ON THE HOST whatever device the inputs live on (so that
    every add and the division are IEEE fp32, whatever a device's kernels do) -> Pooled(rows, offsets).  embeddings_or_shortlister: the
    (R, E) segment rows, float32 or bfloat16, with offsets (V + 1 non-decreasing integers from 0 to R); or a ragged Shortlister -- or
    an object that stands in for one --, whose offsets are taken when offsets is None and whose values are its embeddings or, on a
    quantised table, mx8_dequantize(codes, scales, dtype), which is exact.

    The rows: a video of len_v = offsets[v + 1] - offsets[v] rows becomes ceil(len_v / group) rows, row j of video v pooling the source
    rows offsets[v] + j * group .. min(offsets[v] + (j + 1) * group, offsets[v + 1]) - 1; a video without rows keeps none, and the
    result's offsets are the running sums.  group=None pools a whole video into ONE row and gives a plain (V, E) table without
    offsets; row v of a video without rows is all +0.

    how="mean": an fp32 accumulator that starts at +0; the group's rows added in ASCENDING row order, one plain fp32 add a row --
    ((0 + r0) + r1) + ... --; ONE IEEE fp32 division by float(count); ONE rounding to the table's dtype, to nearest even.  The order
    holds by construction: step i adds row i of every group that has one (a masked add), for i below the longest group -- there is no
    torch.sum and no torch.mean here, whose order nobody states.
    how="max": acc = the group's first row, then, in ascending row order, acc = where(row > acc, row, acc): the element-wise
    maximum, exact in any order -- and of two zeros of different sign, which compare equal, the EARLIER row's (a block-scaled FP8
    table holds both).  Only finite inputs are defined; tables hold no others.
    (So group=1 returns the source's values: bit for bit under "max"; under "mean" bit for bit EXCEPT a -0, which comes back as
    0 + -0 = +0 -- an FP8 table holds such zeros as a matter of course, and a plain table may: its constructor asks for finite values
    only.)"""
    what = "pool_segments_reference"
    group = ops.pool_args(what, how, group)
    src = embeddings_or_shortlister
    if torch.is_tensor(src):
        x = src
        if offsets is None:
            raise DrnError("%s: rows need their offsets" % what)
    else:
        if getattr(src, "_seg", None) is None:
            raise DrnError("%s: the table has no offsets: it is one row a video already" % what)
        x = src.embeddings if src.quantize is None else mx8_dequantize(src.codes.detach().cpu(), src.scales.detach().cpu(), src.dtype)
        if offsets is None:
            offsets = src._seg[0]
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() != 2:
        raise DrnError("%s: the rows must be a (R, E) bfloat16 or float32 tensor, not %s %s" % (what, x.dtype, tuple(x.shape)))
    dtype = x.dtype
    vals = x.detach().cpu().float()                         # (exact)
    R, E = (int(n) for n in vals.shape)
    off = check_segment_offsets(offsets.detach().cpu() if torch.is_tensor(offsets) else offsets, R)
    lens = np.diff(off)
    if group is None:
        out_off, starts, counts = None, off[:-1].copy(), lens.copy()
    else:
        out_off = pool_offsets(off, group)
        per = np.diff(out_off)
        within = np.arange(int(out_off[-1]), dtype=np.int64) - np.repeat(out_off[:-1], per)
        starts = np.repeat(off[:-1], per) + within * group
        counts = np.minimum(group, np.repeat(off[1:], per) - starts)
    acc = torch.zeros((len(starts), E), dtype=torch.float32)
    for i in range(int(counts.max()) if len(counts) else 0):
        live = torch.from_numpy(np.nonzero(counts > i)[0])
        row = vals[torch.from_numpy(starts[counts > i] + i)]
        if how == "mean":
            acc[live] = acc[live] + row
        elif i == 0:
            acc[live] = row
        else:
            old = acc[live]
            acc[live] = torch.where(row > old, row, old)
    if how == "mean":
        live = torch.from_numpy(np.nonzero(counts > 0)[0])
        acc[live] = acc[live] / torch.from_numpy(counts[counts > 0]).to(torch.float32)[:, None]
    return Pooled(acc.to(dtype), out_off)


class Shortlister(object):
    """Shortlister(embeddings, names=None, offsets=None, quantize=None): a (V, E) table of video embeddings, row v belonging to store position v -- a
    contiguous CUDA tensor, bfloat16 or float32, V >= 1 and E >= 1, kept by reference.  Non-finite embeddings are refused here (ONE
    synchronise, once).  names: kept when given; check(store) raises unless they are the store's, before any launch.

    offsets (a sequence, a numpy array or a tensor on any device) makes the table RAGGED: (R, E) segment embeddings, video v -- store
    position v -- owning the rows offsets[v] .. offsets[v + 1] - 1, V + 1 non-decreasing integers from 0 to R with V >= 1 and
    1 <= R < 2^31 (a video may own no row: it is never listed).  They are checked on the host here, in the same one synchronise as the
    embeddings, and the block plan (plan_segment_blocks) is made and put on the device once.  len() is V and names has V entries;
    shortlist() scores a video by its best segment and returns a SegmentShortlist.  Beside a FeatureStore, whose windows are such
    runs, the intended use is Shortlister(window_embeddings, names=store.names, offsets=store.seg_off).

    quantize="mxfp8" keeps the table -- plain or ragged -- in block-scaled FP8 instead: codes (rows, E) uint8 and scales (rows, E / 32)
    uint8, byte for byte drn_amd.index.mx8_quantize of the embeddings (written by ops.quantize_rows_mx8), E + E / 32 bytes a row.  E must
    be a multiple of 32.  Every check above is made as without it, in the same one synchronise, and NO reference to `embeddings` is
    kept: the caller may drop the wide table.  Shortlister.from_mx8 takes tables quantised elsewhere.  shortlist() then returns, bit for
    bit, what dequantized() -- a plain Shortlister over mx8_dequantize(codes, scales, dtype) -- returns; against the ORIGINAL embeddings
    the table is lossy (the format's bound per element), and what that does to recall this module does not say.

    Attributes a caller may rely on: quantize (None or "mxfp8"); dtype (of the table's values and of the queries shortlist() takes) and
    E; embeddings (the table, None on a quantised object); codes and scales (None on a plain one); names; offsets and plan on a ragged
    table; nbytes, the bytes of the table held (= bytes_of(rows, E, dtype, quantize))."""

    quantize = codes = scales = _dtype = _seg = None     # (what a plain table has; also for an object made without the constructor)
    _off_host = None                                     # (a ragged table's offsets as the constructor's check left them on the host)
    nonempty = None                                      # (pooled(group=None) sets it on its result: the mask of the videos that own a row)
    _owners = None                                       # (the same on the host, a bool array (V,); None: every video owns a row)

    def __init__(self, embeddings, names=None, offsets=None, quantize=None):
        if quantize not in QUANTIZE:
            raise DrnError("Shortlister: quantize must be one of %s, not %r" % (QUANTIZE, quantize))
        if not torch.is_tensor(embeddings) or not embeddings.is_cuda:
            raise DrnError("Shortlister: the embeddings must be a tensor on the GPU; there is no CPU fallback")
        if embeddings.dtype not in (torch.bfloat16, torch.float32):
            raise DrnError("Shortlister: the embeddings must be bfloat16 or float32, not %s" % embeddings.dtype)
        if embeddings.dim() != 2 or embeddings.shape[0] < 1 or embeddings.shape[1] < 1 or not embeddings.is_contiguous():
            raise DrnError("Shortlister: the embeddings must be a contiguous (V, E) tensor with V >= 1 and E >= 1, not %s"
                           % (tuple(embeddings.shape),))
        rows, E = (int(x) for x in embeddings.shape)
        if quantize is not None and E % MX8_BLOCK:
            raise DrnError("Shortlister: quantize=%r needs E to be a multiple of %d (one scale per %d columns, and the kernels have no "
                           "tail), not E = %d" % (quantize, MX8_BLOCK, MX8_BLOCK, E))
        self._init_table(rows, embeddings.device, names, offsets, lambda: torch.isfinite(embeddings).all(),
                         "the embeddings hold values that are not finite")
        if quantize is None:
            self.embeddings = embeddings
            return
        self.embeddings, self.quantize, self._dtype = None, quantize, embeddings.dtype
        self.codes = torch.empty((rows, E), dtype=torch.uint8, device=embeddings.device)
        self.scales = torch.empty((rows, E // MX8_BLOCK), dtype=torch.uint8, device=embeddings.device)
        step = max(1, (1 << 30) // E)             # (a launch quantises at most 2^30 elements: one launch up to 2 M rows of 512)
        for a in range(0, rows, step):
            ops.quantize_rows_mx8(embeddings[a:a + step], self.codes[a:a + step], self.scales[a:a + step])

    @classmethod
    def from_mx8(cls, codes, scales, dtype, names=None, offsets=None):
        """A quantised Shortlister on tables the caller quantised: codes (rows, E) and scales (rows, E / 32), contiguous uint8 CUDA
        tensors, E % 32 == 0, kept by reference -- ops.quantize_rows_mx8(x_chunk, codes[a:b], scales[a:b]) fills row slices, so the wide
        table never has to exist.  dtype (torch.bfloat16 or torch.float32) is that of the queries and fixes which MFMA chain scores.
        Raises unless the tables are the format's: no code an e4m3fn NaN (0x7f / 0xff), every scale byte in [17, 254] (2^-110 .. 2^127,
        the range mx8_quantize writes: below it a value could be subnormal, which is not exact in bfloat16) and every dequantised value
        finite in dtype -- checked in row chunks, without materialising the dequantised table, in the ONE synchronise that also
        serves the offsets.  names and offsets as in the constructor."""
        if not torch.is_tensor(codes) or not torch.is_tensor(scales) or not codes.is_cuda or not scales.is_cuda:
            raise DrnError("Shortlister.from_mx8: codes and scales must be tensors on the GPU; there is no CPU fallback")
        if codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise DrnError("Shortlister.from_mx8: codes and scales must be uint8, not %s and %s" % (codes.dtype, scales.dtype))
        if codes.dim() != 2 or codes.shape[0] < 1 or codes.shape[1] < 1 or not codes.is_contiguous():
            raise DrnError("Shortlister.from_mx8: codes must be a contiguous (V, E) tensor with V >= 1 and E >= 1, not %s" % (tuple(codes.shape),))
        rows, E = (int(x) for x in codes.shape)
        if E % MX8_BLOCK:
            raise DrnError("Shortlister.from_mx8: E must be a multiple of %d (one scale per %d columns, and the kernels have no tail), "
                           "not E = %d" % (MX8_BLOCK, MX8_BLOCK, E))
        if tuple(scales.shape) != (rows, E // MX8_BLOCK) or not scales.is_contiguous():
            raise DrnError("Shortlister.from_mx8: scales must be a contiguous (%d, %d) tensor beside codes %s, not %s"
                           % (rows, E // MX8_BLOCK, tuple(codes.shape), tuple(scales.shape)))
        if dtype not in (torch.bfloat16, torch.float32):
            raise DrnError("Shortlister.from_mx8: dtype (of the queries) must be bfloat16 or float32, not %s" % (dtype,))

        def sound():
            ok = (scales >= MX8_EMIN + 127).all() & (scales <= 254).all()
            step = max(1, (1 << 22) // E)         # (a chunk's dequantised rows and the table look-up's indices: 4 M elements)
            for a in range(0, rows, step):
                c = codes[a:a + step]
                ok = ok & ((c & 0x7f) != 0x7f).all() & torch.isfinite(mx8_dequantize(c, scales[a:a + step], dtype)).all()
            return ok
        self = cls.__new__(cls)
        self._init_table(rows, codes.device, names, offsets, sound,
                         "the tables are not block-scaled FP8 with finite values (a NaN code 0x7f / 0xff, a scale byte outside "
                         "[17, 254], or a value that is not finite in %s)" % (dtype,))
        self.embeddings, self.quantize, self._dtype, self.codes, self.scales = None, "mxfp8", dtype, codes, scales
        return self

    def _init_table(self, rows, dev, names, offsets, sound, unsound):
        """What every way of building shares: names, offsets and the block plan, and the ONE synchronise that brings sound() -- a
        device boolean, launched here after the host-side refusals -- to the host."""
        self.names = None if names is None else list(names)
        self._ws = {}
        if offsets is not None:
            self._init_segments(rows, dev, offsets, sound, unsound)
        else:
            if self.names is not None and len(self.names) != rows:
                raise DrnError("Shortlister: %d names for %d embeddings" % (len(self.names), rows))
            if not bool(sound()):
                raise DrnError("Shortlister: " + unsound)

    def _init_segments(self, R, dev, offsets, sound, unsound):
        """The ragged table's checks and its device tables.  Offsets that live on the device come to the host in the one transfer
        that brings the table's soundness (its finiteness)."""
        finite = sound()
        if torch.is_tensor(offsets) and offsets.is_cuda:
            if offsets.is_floating_point() or offsets.is_complex() or offsets.dtype == torch.bool:
                raise DrnError("Shortlister: the offsets must be integers, not %s" % offsets.dtype)
            if offsets.dim() != 1:
                raise DrnError("Shortlister: the offsets must be V + 1 integers with V >= 1, not %s" % (tuple(offsets.shape),))
            both = torch.cat([offsets.to(device=dev, dtype=torch.int64), finite.to(torch.int64).reshape(1)]).cpu()
            offsets, finite = both[:-1], bool(both[-1])
        off = check_segment_offsets(offsets, R, self.names)
        if not bool(finite):
            raise DrnError("Shortlister: " + unsound)
        plan = plan_segment_blocks(off)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.plan = plan
        self._seg = (put(off), put(plan.blk_vid), put(plan.vid_blk))
        self.offsets = self._seg[0]
        self._off_host = off

    def _table(self):
        """The tensor that has the table's rows, columns and device: the embeddings, or the codes of a quantised table."""
        return self.embeddings if self.quantize is None else self.codes

    def _operand(self):
        """The table as the ops wrappers take it: the embeddings, or the pair (codes, scales) of a quantised table."""
        return self.embeddings if self.quantize is None else (self.codes, self.scales)

    def _nblocks(self):
        """The blocks a sentence's first launch ranks: ceil(V / SHORTLIST_BLOCK) on a plain table, the plan's on a ragged one."""
        return -(-len(self) // SHORTLIST_BLOCK) if self._seg is None else int(self._seg[1].shape[0]) - 1

    def _workspace(self, key, keys):
        """The int64 workspace kept as self._ws[key]; keys() is its size in elements, asked for when it has to be made."""
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(keys(), dtype=torch.int64, device=self._table().device)
        return ws

    @property
    def device(self):
        """The device of the table (ShardedShortlister.device is the same accessor)."""
        return self._table().device

    @property
    def dtype(self):
        """The dtype of the table's values and of the queries shortlist() takes."""
        return self.embeddings.dtype if self.quantize is None else self._dtype

    @property
    def E(self):
        return int(self._table().shape[1])

    @staticmethod
    def bytes_of(rows, E, dtype, quantize=None):
        """The bytes of a table of `rows` rows of E columns: rows * E * itemsize(dtype) as given, rows * (E + E / 32) with
        quantize="mxfp8" whatever the dtype (528 against 1024 in bfloat16 and 2048 in float32 at E = 512)."""
        rows, E = int(rows), int(E)
        if quantize not in QUANTIZE:
            raise DrnError("Shortlister.bytes_of: quantize must be one of %s, not %r" % (QUANTIZE, quantize))
        if quantize is None:
            return rows * E * torch.empty((), dtype=dtype).element_size()
        if E % MX8_BLOCK:
            raise DrnError("Shortlister.bytes_of: quantize=%r needs E to be a multiple of %d, not E = %d" % (quantize, MX8_BLOCK, E))
        return rows * (E + E // MX8_BLOCK)

    @property
    def nbytes(self):
        """The bytes of the table this object holds (the offsets, the plan and the workspaces are not counted)."""
        if self.quantize is None:
            return self.embeddings.numel() * self.embeddings.element_size()
        return self.codes.numel() + self.scales.numel()

    def dequantized(self):
        """A plain Shortlister over mx8_dequantize(codes, scales, dtype) with the same names and offsets: what the quantised table
        really holds, and the oracle shortlist() answers bit for bit like.  (On a plain table: itself.)"""
        if self.quantize is None:
            return self
        return Shortlister(mx8_dequantize(self.codes, self.scales, self._dtype), names=self.names,
                           offsets=None if self._seg is None else self._seg[0])

    def _host_offsets(self):
        """A ragged table's offsets on the host, V + 1 int64: what the constructor's check left there; an object made without the
        constructor reads them back from the device once (a synchronise) and keeps them."""
        if self._off_host is None:
            self._off_host = self._seg[0].detach().cpu().numpy().astype(np.int64)
        return self._off_host

    def pooled(self, how="mean", group=None, quantize="same", stage_elems=None):
        """POOL this ragged table's segments into a COARSE table over the same videos, on the device -> a new Shortlister;
        pool_segments_reference is the definition, byte for byte.  The cheap first stage of a cascade, made from the one table the
        caller owns: coarse = fine.pooled(); evaluate_cascade(coarse, fine, ..., allow=coarse.nonempty).

        group=None pools every video into ONE row: the result is a plain (V, E) table WITHOUT offsets (shortlist() returns a
        Shortlist).  group=g >= 1 pools every g consecutive rows of a video (the last group of a video may be shorter): the result is
        ragged, a video of len_v rows owning ceil(len_v / g) -- its offsets are pool_offsets(self offsets, g), a video without rows
        keeps none -- and pooled row r of video v starts at source row offsets_src[v] + (r - offsets_pooled[v]) * g: that is the map
        back from the `rows` of its SegmentShortlist (segment j of the pooled video covers the source segments j * g .. j * g + g - 1).
        how="mean": fp32 sum in ascending row order, one division, one rounding; how="max": the element-wise maximum.  The rows are
        NOT normalised.  names are carried over and len() is unchanged: store positions are the source's, so the result is a legal
        `coarse` beside this table as `fine`.  This table is not modified and the result owns its memory.

        A VIDEO WITHOUT ROWS, with group=None, becomes a row of ZEROS.  A zero row scores 0 against every query and IS A CANDIDATE: it
        is listed, ahead of every video with a negative score, unless the caller passes allow=table.nonempty.  nonempty is the packed
        (W,) allow mask of the videos that own a row, on the device (what allow_of(keep=those videos) returns, made the same way from
        the host offsets), and None when every video owns one -- so allow=table.nonempty is always right.  With group=g the videos
        without rows own none in the result either and are never listed; nonempty is None.

        quantize: the format of the result -- "same" (the default) keeps this table's, None gives plain rows in self.dtype, "mxfp8"
        block-scaled FP8 (E % 32 == 0, refused otherwise).  The kernel always writes PLAIN rows (a quantised source is dequantised in
        registers, exactly); an FP8 result is those rows run through ops.quantize_rows_mx8, the one quantiser, crossing a staging
        buffer of at most stage_elems elements (COMPACT_STAGE_ELEMS when None) in chunks of stage_elems // E rows: the result is
        mx8_quantize(pool_segments_reference(...).rows) byte for byte, whatever the chunks.

        One drn_pool_segments launch (per chunk, beside one quantiser launch, for an FP8 result); the new offsets and block plan are
        made on the host from the offsets the constructor already checked there.  It synchronises ONCE, at the end, for the result's
        finiteness -- an fp32 sum can overflow, and a table that is not finite raises here as the constructor would -- and cannot be
        captured in a graph.  A plain table (no offsets=) is refused: it is one row a video already."""
        what = "Shortlister.pooled"
        group = ops.pool_args(what, how, group)
        if self._seg is None:
            raise DrnError("%s: this table has no offsets=: it is one row a video already, and there is nothing to pool" % what)
        target = _compact_target(what, [self], quantize, self.E)
        return self._pooled(what, how, group, target, stage_elems)

    def _pooled(self, what, how, group, target, stage_elems):
        """pooled() behind its refusals of how, group and quantize (ShardedShortlister.pooled pools its shards through it)."""
        table, E, dtype = self._table(), self.E, self.dtype
        if not table.is_cuda:
            raise DrnError("%s: the table must be on the GPU; there is no CPU fallback (pool_segments_reference is the definition)" % what)
        stage_elems = COMPACT_STAGE_ELEMS if stage_elems is None else int(stage_elems)
        if stage_elems < 1:
            raise DrnError("%s: stage_elems = %d below 1" % (what, stage_elems))
        dev = table.device
        off = self._host_offsets()
        lens = np.diff(off)
        out_off = pool_offsets(off, group)
        rows = len(lens) if group is None else int(out_off[-1])
        out_off_dev = None
        if out_off is not None:
            out_off_dev = torch.from_numpy(out_off.astype(np.int32))
            if dev.type == "cuda":
                out_off_dev = out_off_dev.pin_memory().to(dev, non_blocking=True)
        if target is None:
            dst = torch.empty((rows, E), dtype=dtype, device=dev)
            ops.pool_segments(self._operand(), self._seg[0], dst, how, group, out_off_dev)
            finite = torch.isfinite(dst).all()
        else:
            dst = (torch.empty((rows, E), dtype=torch.uint8, device=dev), torch.empty((rows, E // MX8_BLOCK), dtype=torch.uint8, device=dev))
            step = max(1, stage_elems // E)
            stage = torch.empty((min(step, rows), E), dtype=dtype, device=dev)
            finite = torch.ones((), dtype=torch.bool, device=dev)
            for r0 in range(0, rows, step):
                r1 = min(r0 + step, rows)
                ops.pool_segments(self._operand(), self._seg[0], stage[:r1 - r0], how, group, out_off_dev, out_row0=r0)
                finite = finite & torch.isfinite(stage[:r1 - r0]).all()
                ops.quantize_rows_mx8(stage[:r1 - r0], dst[0][r0:r1], dst[1][r0:r1])
        owners = lens > 0 if group is None and bool((lens == 0).any()) else None
        nonempty = None if owners is None else _mask_words(owners, dev)
        if not bool(finite):                          # THE one synchronise
            raise DrnError("%s: the pooled rows hold values that are not finite (an fp32 sum overflowed)" % what)
        out = _trusted_table(dst, dtype, None if self.names is None else list(self.names), out_off)
        out.nonempty, out._owners = nonempty, owners
        return out

    def __len__(self):
        return int(self._table().shape[0]) if self._seg is None else int(self._seg[0].shape[0]) - 1

    def check(self, store):
        """Raises unless this table's names are the store's (a FeatureStore or a SearchIndex), position by position."""
        if self.names is None or self.names != list(store.names):
            raise DrnError("Shortlister: the table's names are not the store's (row v must belong to store position v)")

    def allow_of(self, keep=None, drop=None):
        """HOST names or store positions -> a packed mask on the table's device, (W,) int32, shared by all sentences: what
        shortlist(allow=) takes.  Exactly one of keep / drop is given: keep=[...] allows those videos alone, drop=[...] -- the
        tombstone list of videos deleted since the table was built -- all the others.  An entry is a name, resolved through
        self.names, or a position in [0, V); an unknown name, a position outside the table or an entry that is neither raises.
        Packed on the host (pack_allow_reference) and put on the device in ONE upload from pinned memory."""
        return _allow_of("Shortlister.allow_of", self.names, len(self), self._table().device, keep, drop)

    def _check_allow(self, allow, S):
        """The refusals of shortlist(allow=), before the library is reached."""
        _check_packed_allow(allow, S, len(self), self._table().device)

    def _check_queries(self, what, queries, S=None, n=None, on_table=True, cap=SHORTLIST_MAX):
        """What shortlist, rank and rerank refuse about queries of one vector a sentence and (where given) n -> (S, n).  S: the rows
        they must have (rerank: one per row of candidates), None for any S >= 1.  on_table: rank and rerank ask for the table's
        device, shortlist for the GPU.  cap: the largest n (shortlist_deep: SHORTLIST_DEEP_MAX)."""
        E, dtype = self.E, self.dtype
        if not torch.is_tensor(queries):
            raise DrnError("%s: the queries must be a tensor" % what)
        shape = tuple(queries.shape)
        if len(shape) != 2 or shape[1] != E or (shape[0] < 1 if S is None else shape[0] != S):
            want = "(S, %d)" % E if S is None else "(%d, %d), a row per row of candidates" % (S, E)
            raise DrnError("%s: the queries must be %s, not %s" % (what, want, shape))
        if queries.dtype != dtype:
            raise DrnError("%s: the queries are %s, the table is %s" % (what, queries.dtype, dtype))
        if n is not None:
            n = int(n)
            if not 1 <= n <= cap:
                raise DrnError("%s: n = %d outside [1, %d]" % (what, n, cap))
        if not on_table:
            if not queries.is_cuda:
                raise DrnError("%s: the queries must be on the GPU; there is no CPU fallback" % what)
        elif not queries.is_cuda or queries.device != self._table().device:
            raise DrnError("%s: the queries must be on the table's device %s; there is no CPU fallback" % (what, self._table().device))
        return shape[0], n

    def _check(self, queries, n, out):
        """shortlist's refusals, before the library is reached -> (S, n)."""
        S, n = self._check_queries("Shortlister.shortlist", queries, n=n, on_table=False)
        if out is not None:
            _check_list_out("Shortlister.shortlist", out, S, n, rows=self._seg is not None)
        return S, n

    def shortlist(self, queries, n, out=None, allow=None):
        """queries (S, E) on the device in the table's dtype, 1 <= n <= SHORTLIST_MAX -> Shortlist (shortlist_reference defines it),
        on the device.  out: a Shortlist (or 3-tuple) of buffers written in place, every element, and returned.  Runs on the current
        stream without a host synchronisation and can be captured in a graph (the workspace is kept per (S, n): warm the shape once
        before capturing).  Scores are accumulated in fp32 in an order that is fixed per (sentence, video): the same bits whatever
        V, S or n.

        On a ragged table (offsets=) -> SegmentShortlist (segment_shortlist_reference defines it): distinct videos by their best
        segment, with the winning segment in rows; out takes the four buffers.  A row's score has the same bits whatever the offsets,
        and with one row per video the scores are the plain table's.

        On a quantised table (quantize="mxfp8", from_mx8) the queries have the recorded dtype and the definition is
        shortlist_reference(mx8_dequantize(codes, scales), queries, n) -- with offsets, segment_shortlist_reference of the same
        dequantised table: the result types, the order, the padding, rows, out= and graph capture are unchanged, and every field is
        bit for bit what dequantized().shortlist(queries, n) gives.

        allow: a PACKED MASK on the table's device -- contiguous int32 (W,), shared by all sentences, or (S, W), one row per sentence,
        W = ceil(V / 32), bit v & 31 of word v >> 5 set = video v may be listed, bits at or past V ignored; pack_allow makes one from a
        bool tensor on the device, allow_of from host names or positions (a bool tensor itself is refused).  The list is then the
        definition with allow= applied -- shortlist_reference(..., allow=mask), segment_shortlist_reference(..., allow=mask), over
        videos, not rows -- on all four tables, with out=, without a host synchronisation and under graph capture, where the mask's
        CONTENTS may change in place between replays.  A listed score has the bits the unfiltered shortlist gives it.  allow=None is
        the unfiltered path, entry and bits."""
        S, n = self._check(queries, n, out)
        if allow is not None:
            self._check_allow(allow, S)
        seg = self._seg
        if out is None:
            out = _list_buffers(self._table().device, S, n, rows=seg is not None)
        if seg is None:
            ws = self._workspace((S, n), lambda: ops.shortlist_ws_keys(len(self), S, n))
            ops.shortlist_topn(self._operand(), queries.contiguous(), n, ws, *out, allow=allow)
            return Shortlist(*out)
        ws = self._workspace((S, n), lambda: ops.shortlist_segments_ws_keys(self._nblocks(), S, n))
        ops.shortlist_segments_topn(self._operand(), queries.contiguous(), seg[0], seg[1], seg[2], n, ws, *out, allow=allow)
        return SegmentShortlist(*out)

    def shortlist_deep(self, queries, n, out=None, allow=None):
        """shortlist() at DEPTH: 1 <= n <= SHORTLIST_DEEP_MAX = 1024, the width rerank / rerank_late (RERANK_MAX_CANDIDATES) and
        Grounder.search(candidates=) (CANDIDATES_MAX) take -> Shortlist, or SegmentShortlist on a ragged table, on the device.  It is
        the COARSE stage of a cascade: a pooled or quantised table that needs some hundreds of candidates before a fine rerank
        recovers the recall (drn_amd.search_eval.evaluate_cascade(deep=True) says how many).  No new definition: shortlist_reference and
        segment_shortlist_reference hold for any n, on a quantised table over mx8_dequantize(codes, scales).  Everything else is
        shortlist()'s: queries, every field, the padding (-1 / 0 / -1), the total order, out= written in place, allow=, no host
        synchronisation, graph capture once the shape is warmed (the workspace is kept per (S, n)), and the refusals.  A listed score
        has the bits shortlist() gives it, a shorter deep list is a prefix of a longer one, and at n <= SHORTLIST_MAX every field
        equals shortlist(queries, n)'s.

        ONE entry for the four tables (drn_shortlist_deep): phase one is the masked shortlist's -- with allow=None under an all-ones
        mask made once per table -- and one workgroup per sentence merges the blocks' lists (csrc/retrieve_deep.hip): two launches, three
        on a ragged table.  That workgroup walks a sentence's lists in sequence, so a call of few sentences over many blocks is bound
        by it.

        What this is NOT: there is no shortlist_late at depth, and no ShardedShortlister.shortlist_deep -- a sharded corpus is
        compact()ed into one table first."""
        what = "Shortlister.shortlist_deep"
        S, n = self._check_queries(what, queries, n=n, on_table=False, cap=SHORTLIST_DEEP_MAX)
        seg = self._seg
        if out is not None:
            _check_list_out(what, out, S, n, rows=seg is not None)
        if allow is not None:
            self._check_allow(allow, S)
        else:
            allow = self._all_allowed()
        if out is None:
            out = _list_buffers(self._table().device, S, n, rows=seg is not None)
        if seg is None:
            ws = self._workspace(("deep", S, n), lambda: ops.shortlist_ws_keys(len(self), S, n))
            ops.shortlist_deep(self._operand(), queries.contiguous(), (), n, ws, tuple(out), allow)
            return Shortlist(*out)
        ws = self._workspace(("deep", S, n), lambda: ops.shortlist_segments_ws_keys(self._nblocks(), S, n))
        ops.shortlist_deep(self._operand(), queries.contiguous(), seg, n, ws, tuple(out), allow)
        return SegmentShortlist(*out)

    def _all_allowed(self):
        """The packed mask that allows every video, (W,) int32 of -1 on the table's device, shared by all sentences: made once."""
        ones = self._ws.get("all_allowed")
        if ones is None:
            ones = self._ws["all_allowed"] = torch.full((ops.allow_words(len(self)),), -1, dtype=torch.int32, device=self._table().device)
        return ones

    def shortlist_late(self, queries, lengths, n, out=None, allow=None):
        """The shortlist by LATE INTERACTION (late_shortlist_reference defines it) -> Shortlist, on the device.  queries: contiguous
        (S, L, E) on the table's device in the table's (on a quantised table, the recorded) dtype, one vector per token, 1 <= L <=
        LATE_MAX_TOKENS; lengths: contiguous int32 (S,) on the device, the live tokens of each sentence -- clamped into [0, L] on the
        device and NEVER read on the host; what a token past it holds is ignored, NaN included, and costs nothing.  A video's score is
        the sum over the live tokens, in ascending order in fp32, of the token's best row of the video; each term has the bits
        shortlist() gives that (token, video) pair, and the sum depends on the sentence's live tokens and the video's rows alone -- not
        on S, L, the padding, V, n, the other videos' offsets or the mask.  With one token per sentence the ids, scores and n are
        shortlist()'s.  n, out= (three buffers: ids, scores, n) and allow= as in shortlist(); ONE tagged entry, two launches on the
        current stream, no host synchronisation, and it can be captured in a graph (the workspace is kept per (S, n): warm the shape
        once), where queries, lengths and the mask's contents may change in place between replays.  Works on a ragged table, plain or
        quantised.  A table without offsets is refused: with one row per video the sum over the tokens of q_t . emb_v is (the sum of
        q_t) . emb_v, so the caller adds the live tokens and calls shortlist()."""
        what = "Shortlister.shortlist_late"
        seg = self._seg
        if seg is None:
            _refuse_late(what, "shortlist")
        S, L, n = self._check_late(what, queries, lengths, n)
        if out is not None:
            _check_list_out(what, out, S, n)
        if allow is not None:
            self._check_allow(allow, S)
        if out is None:
            out = _list_buffers(self._table().device, S, n)
        ws = self._workspace(("late", S, n), lambda: ops.shortlist_late_ws_keys(self._nblocks(), S, n))
        ops.shortlist_late_topn(self._operand(), queries, lengths, seg[0], seg[1], n, ws, *out, allow=allow)
        return Shortlist(*out)

    def _check_late(self, what, queries, lengths, n=None):
        """What shortlist_late, rank_late and rerank_late refuse about per-token queries, lengths and (where given) n, before the
        library is reached -> (S, L, n)."""
        E, dtype, dev = self.E, self.dtype, self._table().device
        if not torch.is_tensor(queries):
            raise DrnError("%s: the queries must be a tensor" % what)
        if queries.dim() != 3 or queries.shape[0] < 1 or queries.shape[2] != E:
            raise DrnError("%s: the queries must be (S, L, %d), one vector per token, not %s" % (what, E, tuple(queries.shape)))
        S, L = int(queries.shape[0]), int(queries.shape[1])
        if not 1 <= L <= LATE_MAX_TOKENS:
            raise DrnError("%s: L = %d tokens outside [1, %d]" % (what, L, LATE_MAX_TOKENS))
        if queries.dtype != dtype:
            raise DrnError("%s: the queries are %s, the table is %s" % (what, queries.dtype, dtype))
        if n is not None:
            n = int(n)
            if not 1 <= n <= SHORTLIST_MAX:
                raise DrnError("%s: n = %d outside [1, %d]" % (what, n, SHORTLIST_MAX))
        if not queries.is_cuda or queries.device != dev:
            raise DrnError("%s: the queries must be on the table's device %s; there is no CPU fallback" % (what, dev))
        if not queries.is_contiguous():
            raise DrnError("%s: the queries must be contiguous" % what)
        if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (S,) or not lengths.is_contiguous():
            raise DrnError("%s: lengths must be a contiguous (%d,) torch.int32 tensor, the live tokens of each sentence" % (what, S))
        if not lengths.is_cuda or lengths.device != dev:
            raise DrnError("%s: lengths must be on the table's device %s (they are never read on the host)" % (what, dev))
        return S, L, n

    def _check_candidates(self, what, candidates, n):
        """What rerank and rerank_late refuse about the table's device, the list and n, before the library is reached -> (S, C, n)."""
        dev = self._table().device
        if not self._table().is_cuda:
            raise DrnError("%s: the table must be on the GPU; there is no CPU fallback" % what)
        if not torch.is_tensor(candidates):
            raise DrnError("%s: candidates must be a tensor (the ids of a Shortlist can be passed as they are)" % what)
        if candidates.dtype != torch.int32:
            raise DrnError("%s: candidates must be torch.int32 store positions, not %s" % (what, candidates.dtype))
        if candidates.dim() != 2 or candidates.shape[0] < 1:
            raise DrnError("%s: candidates must be (S, C), a row of store positions per sentence, not %s" % (what, tuple(candidates.shape)))
        S, C = int(candidates.shape[0]), int(candidates.shape[1])
        if not 1 <= C <= RERANK_MAX_CANDIDATES:
            raise DrnError("%s: C = %d candidates a sentence outside [1, %d]" % (what, C, RERANK_MAX_CANDIDATES))
        if not candidates.is_cuda or candidates.device != dev:
            raise DrnError("%s: candidates must be on the table's device %s (they are never read on the host)" % (what, dev))
        if not candidates.is_contiguous():
            raise DrnError("%s: candidates must be contiguous" % what)
        n = min(C, SHORTLIST_MAX) if n is None else int(n)
        if not 1 <= n <= SHORTLIST_MAX:
            raise DrnError("%s: n = %d outside [1, %d]" % (what, n, SHORTLIST_MAX))
        return S, C, n

    def _rerank(self, what, S, C, n, candidates, queries, lengths, out, allow):
        """What rerank and rerank_late share once their tensors are checked: out=, allow=, the workspace and the launch."""
        if out is not None:
            _check_list_out(what, out, S, n)
        if allow is not None:
            self._check_allow(allow, S)
        if out is None:
            out = _list_buffers(self._table().device, S, n)
        ws = self._workspace(("rerank", S, C, n), lambda: ops.shortlist_rerank_ws_keys(C, S, n))
        offsets = None if self._seg is None else self._seg[0]
        ops.shortlist_rerank(self._operand(), queries, lengths, offsets, candidates, n, ws, *out, allow=allow)
        return Shortlist(*out)

    def rerank(self, candidates, queries, n=None, out=None, allow=None):
        """RERANK A CANDIDATE LIST: score only the listed (sentence, video) pairs -> Shortlist, on the device (rerank_reference
        defines it; on a ragged table segment_rerank_reference, a video scoring by its best row).  candidates: contiguous int32 (S, C)
        on the table's device, 1 <= C <= RERANK_MAX_CANDIDATES, row s the SET of store positions sentence s may list
        (candidates_mask defines it): NEVER read on the host; a value outside [0, V) means nothing, a repeat counts once, and the
        order of a row means nothing -- Shortlist.ids and SegmentShortlist.ids of any other Shortlister over the same store positions
        can be passed as they are, -1 padding included.  queries, out= (three buffers: ids, scores, n) and allow= as in shortlist();
        n: None means min(C, SHORTLIST_MAX), otherwise 1 <= n <= SHORTLIST_MAX, and n > C is legal (the rest is padding).

        Every field equals, bit for bit, the filtered call over the whole table, shortlist(queries, n,
        allow=pack_allow(candidates_mask(candidates, V) [& allow])) without its rows -- a score has the bits the full shortlist gives
        that pair, and ties fall by store position, not by place in the list -- but only the rows of the listed videos are read.
        Consequently rerank(shortlist(q, n).ids, q, n) is shortlist(q, n).  An answer depends on the sentence, the SET of its valid
        candidates, the table and the mask alone: not on the list's order, its padding, repeats, C, S, the other sentences' lists or n
        (beyond the cut).  Works on all four tables and returns a Shortlist on every one: the winning segment (rows) of a ragged
        table is NOT reported here.  On a quantised table every field is bit for bit dequantized().rerank(...).  ONE tagged entry, two
        launches on the current stream, no host synchronisation, and it can be captured in a graph (the workspace is kept per
        ("rerank", S, C, n): warm the shape once before capturing), where candidates, the queries and the mask's contents may change
        in place between replays."""
        what = "Shortlister.rerank"
        S, C, n = self._check_candidates(what, candidates, n)
        self._check_queries(what, queries, S)
        return self._rerank(what, S, C, n, candidates, queries.contiguous().view(S, 1, -1), None, out, allow)

    def rerank_late(self, candidates, queries, lengths, n=None, out=None, allow=None):
        """rerank() by LATE INTERACTION -> Shortlist (late_rerank_reference defines it), on the device: candidates and n as in
        rerank(), queries (S, L, E) and lengths (S,) as in shortlist_late(), out= and allow= as there.  Every field equals, bit for
        bit, shortlist_late(queries, lengths, n, allow=pack_allow(candidates_mask(candidates, V) [& allow])), reading the rows of the
        listed videos alone; with one token per sentence this is rerank().  The promises of rerank() hold: the answer depends on the
        sentence, the set of its valid candidates, the table and the mask alone.  Works on a ragged table, plain or quantised (bit
        for bit dequantized().rerank_late(...)); two launches, no host synchronisation, capturable in a graph (the workspace is kept
        per ("rerank", S, C, n)), where candidates, queries, lengths and the mask's contents may change in place between replays.  A
        table without offsets is refused as in shortlist_late()."""
        what = "Shortlister.rerank_late"
        if self._seg is None:
            _refuse_late(what, "rerank")
        S, C, n = self._check_candidates(what, candidates, n)
        Sq, _, _ = self._check_late(what, queries, lengths)
        if Sq != S:
            raise DrnError("%s: the queries hold %d sentences, candidates has %d rows" % (what, Sq, S))
        return self._rerank(what, S, C, n, candidates, queries, lengths, out, allow)

    def _check_rerank_scores(self, what, candidates, queries, lengths):
        """What rerank_scores (lengths=None) and rerank_scores_late refuse about the list and the queries -- rerank's and rerank_late's
        refusals -- before the library is reached -> (S, C, the queries as (S, L, E))."""
        if lengths is not None and self._seg is None:
            _refuse_late(what, "rerank_scores")
        S, C, _ = self._check_candidates(what, candidates, None)
        if lengths is None:
            self._check_queries(what, queries, S)
            return S, C, queries.contiguous().view(S, 1, -1)
        Sq, _, _ = self._check_late(what, queries, lengths)
        if Sq != S:
            raise DrnError("%s: the queries hold %d sentences, candidates has %d rows" % (what, Sq, S))
        return S, C, queries

    def _rerank_scores(self, what, S, C, candidates, queries, lengths, out, allow, inside_only=False):
        """What rerank_scores and rerank_scores_late share once their tensors are checked (queries (S, L, E)): out=, allow= and the one
        launch.  inside_only: ShardedShortlister's shards after the first leave the slots of other shards as they are."""
        dev = self._table().device
        if out is None:
            out = torch.empty((S, C), dtype=torch.float32, device=dev)
        else:
            _check_scores_out(what, out, S, C, dev)
        if allow is not None:
            self._check_allow(allow, S)
        offsets = None if self._seg is None else self._seg[0]
        return ops.shortlist_rerank_scores(self._operand(), queries, lengths, offsets, candidates, out, allow=allow, inside_only=inside_only)

    def rerank_scores(self, candidates, queries, out=None, allow=None):
        """THE SCORES OF THE LISTED PAIRS, the listed-pairs counterpart of scores() -> float32 (S, C) on the device
        (rerank_scores_reference defines it).  candidates and queries as in rerank(): out[s, j] is the score rerank() would list for
        the pair (s, candidates[s, j]) -- the same kernel up to its sums, so the same bits, a -0 written as +0 -- and -inf where the
        slot is NO CANDIDATE: its id lies outside [0, V), an earlier slot of the row holds the same id, allow excludes the video, the
        video owns no row or the score is not finite.  So finite <=> candidate, no NaN is ever written, and
        rerank_scores(c, q)[s, j] == scores(q)[s, c[s, j]] at every first occurrence.  Only the listed videos' rows are read.  Works on
        all four tables; on a quantised one it is bit for bit dequantized().rerank_scores(...).  out: a float32 (S, C) tensor on the
        table's device written in place, EXACTLY those elements; it may be a row-strided view (last stride 1, row stride >= C).
        allow= as in shortlist().  The refusals are rerank()'s.  ONE launch on the current stream (drn_shortlist_rerank_scores), no
        workspace, no host synchronisation, and it can be captured in a graph, where candidates, the queries and the mask's contents
        may change in place between replays.  A distillation target, a calibration set or a learned fuser reads it, and
        fused_rerank folds several."""
        what = "Shortlister.rerank_scores"
        S, C, q = self._check_rerank_scores(what, candidates, queries, None)
        return self._rerank_scores(what, S, C, candidates, q, None, out, allow)

    def rerank_scores_late(self, candidates, queries, lengths, out=None, allow=None):
        """rerank_scores() by LATE INTERACTION -> float32 (S, C): candidates as in rerank(), queries (S, L, E) and lengths (S,) as in
        shortlist_late(); out[s, j] has the bits rerank_late() lists for the pair and is -inf where the slot is no candidate; a
        sentence without a live token is a row of -inf.  out= and allow= as in rerank_scores(), the refusals are rerank_late()'s.  One
        launch, capturable, where candidates, queries, lengths and the mask's contents may change in place between replays.  A table
        without offsets is refused as in shortlist_late()."""
        what = "Shortlister.rerank_scores_late"
        if not torch.is_tensor(lengths):
            raise DrnError("%s: lengths must be a contiguous torch.int32 tensor on the device, the live tokens of each sentence" % what)
        S, C, q = self._check_rerank_scores(what, candidates, queries, lengths)
        return self._rerank_scores(what, S, C, candidates, q, lengths, out, allow)

    def _check_targets(self, what, S, targets):
        """What every rank refuses about targets, before the library is reached."""
        _check_targets(what, S, targets, self._table().device)

    def _check_rank(self, what, S, targets, out, allow):
        """What rank() and rank_late() refuse about targets, out= and allow=, before the library is reached -> out, made where None."""
        self._check_targets(what, S, targets)
        _check_rank_out(what, S, out)
        if allow is not None:
            self._check_allow(allow, S)
        return _rank_buffers(self._table().device, S) if out is None else tuple(out)

    def rank(self, queries, targets, out=None, allow=None):
        """The place of each sentence's TARGET video in its full shortlist order -> TargetRank (rank_reference defines it; on a ragged
        table segment_rank_reference), on the device.  queries as in shortlist(); targets: contiguous int32 (S,) on the table's device,
        the store position of each sentence's video, NEVER read on the host -- a value outside [0, V) is legal and means "no target".
        rank[s] counts the candidates that precede the target over the WHOLE table -- no cap at SHORTLIST_MAX, no list, no sort -- so
        rank[s] = k >= 0 exactly when shortlist(queries, n).ids[s, k] is the target for every n > k, and score[s] has the listed
        score's bits; -1 (and score 0) where the target is no candidate: out of range, without rows, masked, or its score is not
        finite.  total[s] is the number of candidates.  An answer depends on the sentence, its target, the table and the mask alone.
        Works on all four tables; on a quantised one every field is bit for bit dequantized().rank(...).  out: three (S,) buffers
        (rank, score, total) written in place.  allow= as in shortlist().  ONE tagged entry, three launches on the current stream,
        no host synchronisation, and it can be captured in a graph (the workspace is kept per S: warm the shape once), where queries,
        targets and the mask's contents may change in place between replays."""
        what = "Shortlister.rank"
        S, _ = self._check_queries(what, queries)
        out = self._check_rank(what, S, targets, out, allow)
        ws = self._workspace(("rank", S), lambda: ops.shortlist_rank_ws_bytes(self._nblocks(), S) // 8)
        seg = self._seg
        if seg is None:
            ops.shortlist_rank(self._operand(), queries.contiguous(), targets, ws, *out, allow=allow)
        else:
            ops.shortlist_segments_rank(self._operand(), queries.contiguous(), seg[0], seg[1], targets, ws, *out, allow=allow)
        return TargetRank(*out)

    def rank_late(self, queries, lengths, targets, out=None, allow=None):
        """rank() by LATE INTERACTION -> TargetRank (late_rank_reference defines it), on the device: queries (S, L, E) and lengths
        (S,) as in shortlist_late(), targets, out= and allow= as in rank().  rank[s] = k >= 0 exactly when
        shortlist_late(queries, lengths, n).ids[s, k] is the target for every n > k, with the listed score's bits; a sentence without
        a live token has no candidate (rank -1, total 0).  With one token per sentence this is rank().  Works on a ragged table,
        plain or quantised (bit for bit dequantized().rank_late(...)); three launches, no host synchronisation, capturable in a graph
        (the workspace is kept per S), where queries, lengths, targets and the mask's contents may change in place between replays.
        A table without offsets is refused as in shortlist_late()."""
        what = "Shortlister.rank_late"
        seg = self._seg
        if seg is None:
            _refuse_late(what, "rank")
        S, L, _ = self._check_late(what, queries, lengths)
        out = self._check_rank(what, S, targets, out, allow)
        ws = self._workspace(("rank_late", S), lambda: ops.shortlist_rank_ws_bytes(self._nblocks(), S) // 8)
        ops.shortlist_late_rank(self._operand(), queries, lengths, seg[0], seg[1], targets, ws, *out, allow=allow)
        return TargetRank(*out)

    def scores(self, queries, out=None, allow=None):
        """THE WHOLE SCORE MATRIX shortlist() ranks and throws away -> float32 (S, V) on the device (scores_reference defines it).
        queries as in rank(): (S, E) on the table's device in the table's dtype.  out[s, v] is the score shortlist() gives the pair --
        the same MFMA chain and, on a ragged table, the same best row: scores()[s, ids[s, k]] has the bits of shortlist().scores[s, k],
        a -0 written as +0 -- and -inf where the video is NO CANDIDATE: it owns no row, its score is not finite, or allow excludes
        it.  So finite <=> candidate, no NaN is ever written, and an entry depends on the sentence, the video's rows and its mask bit
        alone.  Works on all four tables; on a quantised one it is bit for bit dequantized().scores(...).  out: a float32 (S, V) tensor
        on the table's device written in place, EXACTLY those elements: it may be a row-strided view (last stride 1, row stride >= V),
        such as a column slice buffer[:, a:a + V] of a wider matrix.  allow= as in shortlist().  ONE launch on the current stream
        (drn_shortlist_scores), no workspace, no host synchronisation, and it can be captured in a graph, where the queries and the
        mask's contents may change in place between replays.
        What this costs: 4 * S * V bytes written, where shortlist() writes 12 * S * n; a threshold, a calibration or a distillation
        target reads it, and shortlist_scores() ranks it (or anything made from it) under the project's total order."""
        what = "Shortlister.scores"
        S, _ = self._check_queries(what, queries)
        return self._scores(what, S, queries.contiguous(), None, out, allow)

    def scores_late(self, queries, lengths, out=None, allow=None):
        """scores() by LATE INTERACTION -> float32 (S, V): queries (S, L, E) and lengths (S,) as in shortlist_late(); out[s, v] has
        the bits shortlist_late() lists for the pair -- the fp32 sum over the live tokens, in ascending order, of the token's best row
        -- and is -inf where the video is no candidate; a sentence without a live token is a row of -inf.  out= and allow= as in
        scores().  One launch, capturable, where queries, lengths and the mask's contents may change in place between replays.  A table
        without offsets is refused as in shortlist_late()."""
        what = "Shortlister.scores_late"
        if self._seg is None:
            _refuse_late(what, "scores")
        S, _, _ = self._check_late(what, queries, lengths)
        return self._scores(what, S, queries, lengths, out, allow)

    def _scores(self, what, S, queries, lengths, out, allow):
        """What scores (lengths=None) and scores_late share once their queries are checked: out=, allow= and the one launch."""
        dev, V = self._table().device, len(self)
        if out is None:
            out = torch.empty((S, V), dtype=torch.float32, device=dev)
        else:
            _check_scores_out(what, out, S, V, dev)
        if allow is not None:
            self._check_allow(allow, S)
        seg = self._seg
        return ops.shortlist_scores(self._operand(), queries, lengths, () if seg is None else (seg[0], seg[1]), out, allow=allow)

    def _rank_keys(self, what, queries, lengths, targets, keys, allow=None):
        """PHASE 1 of rank() (lengths=None) or rank_late() alone, for ShardedShortlister: each sentence's target key in THIS table ->
        keys, a contiguous (S,) int64 tensor written in place (0 where the target is no candidate here).  The refusals are the public
        methods', under the name `what`; one launch."""
        self._check_rank_queries(what, queries, lengths)
        self._check_targets(what, int(queries.shape[0]), targets)
        return self._rank_phase(1, queries, lengths, targets, keys, None, allow)

    def _rank_counts(self, what, queries, lengths, thresholds, cnt, allow=None):
        """PHASE 2 of rank() (lengths=None) or rank_late() alone, for ShardedShortlister: the block counts against thresholds, a
        contiguous (S,) int64 tensor read in the place of the target keys -> cnt, a contiguous int64 tensor of S * _nblocks() elements
        written in place.  The refusals are the public methods', under the name `what`; one launch."""
        self._check_rank_queries(what, queries, lengths)
        return self._rank_phase(2, queries, lengths, None, thresholds, cnt, allow)

    def _check_rank_queries(self, what, queries, lengths):
        """rank()'s refusals about queries (lengths=None), rank_late()'s about queries and lengths -> S."""
        if lengths is None:
            return self._check_queries(what, queries)[0]
        if self._seg is None:
            _refuse_late(what, "rank")
        return self._check_late(what, queries, lengths)[0]

    def _rank_phase(self, phase, queries, lengths, targets, keys, cnt, allow):
        """The one launch of _rank_keys / _rank_counts, by the table's shape."""
        if allow is not None:
            self._check_allow(allow, int(queries.shape[0]))
        seg = self._seg
        if seg is None:
            return ops.shortlist_rank_phase(self._operand(), queries.contiguous(), phase, targets, keys, cnt, allow=allow)
        if lengths is None:
            return ops.shortlist_segments_rank_phase(self._operand(), queries.contiguous(), seg[0], seg[1], phase, targets, keys, cnt, allow=allow)
        return ops.shortlist_late_rank_phase(self._operand(), queries, lengths, seg[0], seg[1], phase, targets, keys, cnt, allow=allow)


Compacted = collections.namedtuple("Compacted", "table positions kept")
Compacted.__doc__ = """table: ONE new Shortlister over the surviving videos, in corpus order; positions (V,) int32 on the tables' device: the new
position of corpus position v, -1 where v was dropped (monotone over the survivors: what remaps stored ids, targets and masks); kept:
the host integer V' = len(table)."""

COMPACT_STAGE_ELEMS = 1 << 26   # elements of the staging buffer plain rows cross on their way to FP8 (128 MiB in bfloat16): a CHOICE, not a measurement


def _trusted_table(rows, dtype, names, offsets):
    """A Shortlister over tables that NEED NO CHECK: rows is a plain (R, E) tensor or the pair (codes, scales) in the format, every
    value copied or exactly dequantised from tables whose own constructors checked them (or written by the one quantiser from such
    rows), so nothing is read again for finiteness and nothing synchronises.  offsets: host integers (V + 1) or None; the block plan
    is made here as the constructor makes it."""
    self = Shortlister.__new__(Shortlister)
    self.names, self._ws = names, {}
    if isinstance(rows, tuple):
        self.embeddings, self.quantize, self._dtype, self.codes, self.scales = None, "mxfp8", dtype, rows[0], rows[1]
    else:
        self.embeddings = rows
    if offsets is not None:
        table = self._table()
        off = check_segment_offsets(offsets, int(table.shape[0]), names)
        plan = plan_segment_blocks(off)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(table.device)
        self.plan = plan
        self._seg = (put(off), put(plan.blk_vid), put(plan.vid_blk))
        self.offsets = self._seg[0]
        self._off_host = off
    return self


def _compact_target(what, shards, quantize, E):
    """quantize= of a compaction -> the format of the result, None or "mxfp8"; "same" takes the shards' common one and refuses mixed
    shards: doubling or halving a table's bytes is never silent."""
    if isinstance(quantize, str) and quantize == "same":
        formats = sorted(set(str(shard.quantize) for shard in shards))
        if len(formats) > 1:
            raise DrnError("%s: quantize=\"same\" needs shards of one format and these are mixed (%s): pass quantize=None for a plain "
                           "table or quantize=\"mxfp8\" for block-scaled FP8" % (what, ", ".join(formats)))
        return shards[0].quantize
    if quantize not in QUANTIZE:
        raise DrnError("%s: quantize must be \"same\" or one of %s, not %r" % (what, QUANTIZE, quantize))
    if quantize is not None and E % MX8_BLOCK:
        raise DrnError("%s: quantize=%r needs E to be a multiple of %d, not E = %d" % (what, quantize, MX8_BLOCK, E))
    return quantize


def compact_reference(shards, keep=None, quantize="same"):
    """THE DEFINITION of ShardedShortlister.compact, in plain torch and numpy (usable on the CPU) -> Compacted.  shards: a
    ShardedShortlister or a sequence of Shortlister objects, wherever their tensors live (an object that only stands in for a
    resident table will do: its embeddings or codes and scales, quantize, dtype, names and offsets are all that is read).  keep: None
    -- every video survives -- or a mask over the corpus, a bool (V,) tensor / array or the packed (W,) int32 words of pack_allow.
    quantize: "same", None or "mxfp8", as in compact().

    positions[v] = the number of kept videos before v, -1 where v is dropped; the surviving videos keep their corpus order and
    their rows, in order; names are filtered; on ragged shards the new offsets are the running sums of the survivors' row counts (a
    kept video without rows stays one).  Per row, by source -> target format: plain -> plain the values as they are; mxfp8 -> mxfp8
    codes and scale bytes as they are (NOT requantised); mxfp8 -> plain mx8_dequantize(codes, scales, dtype); plain -> mxfp8
    mx8_quantize(rows).  V' = 0, or R' = 0 on ragged shards, raises.  table is built without the constructor's checks and holds its
    tensors on the shards' device."""
    what = "compact_reference"
    if isinstance(shards, ShardedShortlister):
        sh = shards
    else:
        sh = ShardedShortlister.__new__(ShardedShortlister)
        sh.shards, sh.bases, sh.names = [], [0], []
        for shard in shards:
            sh._admit(shard)
        if not sh.shards:
            raise DrnError("%s: at least one shard" % what)
    V, E, dtype, dev = len(sh), sh.E, sh.dtype, sh.device
    target = _compact_target(what, sh.shards, quantize, E)
    ragged = sh.shards[0]._seg is not None
    if keep is None:
        mask = np.ones(V, dtype=np.bool_)
    else:
        m = np.asarray(keep.detach().cpu().numpy() if torch.is_tensor(keep) else keep)
        if m.dtype == np.bool_ and m.shape == (V,):
            mask = m.copy()
        elif m.dtype == np.int32 and m.shape == (ops.allow_words(V),):
            mask = np.unpackbits(np.ascontiguousarray(m).view(np.uint8), bitorder="little").astype(np.bool_)[:V]
        else:
            raise DrnError("%s: keep must be a bool mask (%d,) or its packed int32 words (%d,), one mask for the corpus, not %s %s"
                           % (what, V, ops.allow_words(V), m.dtype, m.shape))
    kept = int(mask.sum())
    positions = np.where(mask, np.cumsum(mask) - mask, -1).astype(np.int32)
    parts, lens = [], []
    for shard, a, b in zip(sh.shards, sh.bases[:-1], sh.bases[1:]):
        live = torch.from_numpy(mask[a:b])
        if ragged:
            n = (shard._seg[0][1:] - shard._seg[0][:-1]).cpu().to(torch.int64)
            lens.append(n[live])
            live = torch.repeat_interleave(live, n)
        live = live.to(dev)
        if shard.quantize is None:
            rows = shard.embeddings[live]
            parts.append(rows if target is None else mx8_quantize(rows))
        elif target is None:
            parts.append(mx8_dequantize(shard.codes[live], shard.scales[live], dtype))
        else:
            parts.append((shard.codes[live], shard.scales[live]))
    rows = torch.cat(parts).contiguous() if target is None else (torch.cat([p[0] for p in parts]).contiguous(),
                                                                  torch.cat([p[1] for p in parts]).contiguous())
    R = int((rows if target is None else rows[0]).shape[0])
    if kept == 0:
        raise DrnError("%s: the mask keeps no video: a table needs one" % what)
    if R == 0:
        raise DrnError("%s: the %d videos the mask keeps own no row: a table needs one" % (what, kept))
    offsets = np.concatenate([[0], np.cumsum(torch.cat(lens).numpy())]).astype(np.int64) if ragged else None
    names = None if sh.names is None else [name for name, live in zip(sh.names, mask) if live]
    return Compacted(_trusted_table(rows, dtype, names, offsets), torch.from_numpy(positions).to(dev), kept)


class ShardedShortlister(object):
    """ShardedShortlister(shards): a corpus kept as 1 to SHARDS_MAX Shortlister objects, held by reference; the video at position i of
    shard k is the corpus's video bases[k] + i, bases being the running sums of len(shard).  The shards share the device, E, dtype (of
    the queries) and the kind -- all plain or all with offsets=, because the result types differ; quantize may differ from shard to
    shard (yesterday's rows in block-scaled FP8 beside today's in bfloat16), and the corpus holds fewer than 2^31 videos.  Anything
    else is refused before any launch.

    append(shard) is how a video ARRIVES: the new rows become one more shard -- its own constructor checks them, in its own one
    synchronise -- and nothing that is resident is touched, copied or checked again.  (allow_of(drop=) is how a video leaves.)

    shortlist() and shortlist_late() answer, field for field and bit for bit, what ONE Shortlister over the concatenated rows answers:
    a score's bits do not depend on the table that holds the video, every shard cuts its list under the one total order (score
    descending, then position ascending), and the best n of the corpus are among the best n of each shard, so merging the shards'
    lists under the same order with positions shifted by bases (merge_shortlists_reference; drn_shortlist_merge_lists, ONE launch)
    gives the corpus's list.  allow= takes a mask over the corpus, cut into the shards' own by one more launch (slice_allow_reference;
    drn_allow_slices).

    rank() / rank_late() and rerank() / rerank_late() answer likewise, field for field and bit for bit, what ONE Shortlister over the
    concatenated rows answers, with positions and masks over the CORPUS.  A rank: drn_shard_positions gives every shard its local
    target (-1 where it lies elsewhere), each shard's own target kernel makes its key, ONE launch turns the one key that is not 0
    into a counting threshold per shard -- an equal score precedes the target in an earlier shard and follows it in a later one
    (rank_thresholds_reference) --, each shard's own counting kernel counts against its threshold, and ONE launch sums: 2 K + 3
    launches, one more under a mask.  A rerank: drn_shard_positions on the candidate lists, each shard's own rerank of the
    candidates that fall inside it, and the merge of shortlist(): a shard's rerank is its filtered shortlist.

    Attributes a caller may rely on: shards; bases (a host list of K + 1 integers) and bases_device (the same as int32 on the
    device); names (the concatenation when every shard has names, else None); device, E, dtype, nbytes (the sum over the shards).

    NOT here: one grouped launch over all shards in the place of K; the winning segment (rows) from a rerank; shards on several
    devices or ranks (the stacked (K, S, n) lists are laid out so that lists gathered from other GPUs merge through the same entry);
    shards on parallel streams (they run one after the other on the current stream); n above SHORTLIST_MAX.

    compact(keep) is the third verb beside append() and allow_of(drop=): ONE new table over the videos a mask keeps, built on the
    device, for when the shard count or the tombstone list has grown (a single table is the faster one to query)."""

    nonempty = None                              # (the corpus mask of the videos that own a row, over shards made by pooled(group=None): _placed)

    def __init__(self, shards):
        try:
            shards = list(shards)
        except TypeError:
            raise DrnError("ShardedShortlister: the shards must be a sequence of Shortlister objects")
        if not 1 <= len(shards) <= SHARDS_MAX:
            raise DrnError("ShardedShortlister: %d shards outside [1, %d]" % (len(shards), SHARDS_MAX))
        self.shards, self.bases, self.names = [], [0], []
        for shard in shards:
            self._admit(shard)
        self._placed()

    def _admit(self, shard):
        """The checks of one more shard, then its place: nothing is launched."""
        if not isinstance(shard, Shortlister):
            raise DrnError("ShardedShortlister: a shard must be a Shortlister, not %s" % type(shard).__name__)
        if len(self.shards) >= SHARDS_MAX:
            raise DrnError("ShardedShortlister: %d shards outside [1, %d]" % (len(self.shards) + 1, SHARDS_MAX))
        if self.shards:
            first = self.shards[0]
            if shard._table().device != first._table().device:
                raise DrnError("ShardedShortlister: shard %d is on %s, the others on %s" % (len(self.shards), shard._table().device,
                                                                                           first._table().device))
            if shard.E != first.E:
                raise DrnError("ShardedShortlister: shard %d has E = %d columns, the others %d" % (len(self.shards), shard.E, first.E))
            if shard.dtype != first.dtype:
                raise DrnError("ShardedShortlister: shard %d takes %s queries, the others %s" % (len(self.shards), shard.dtype, first.dtype))
            if (shard._seg is None) != (first._seg is None):
                raise DrnError("ShardedShortlister: shard %d is %s, the others are not: the shards must all be plain or all have offsets= "
                               "(the result types differ)" % (len(self.shards), "plain" if shard._seg is None else "ragged"))
        if self.bases[-1] + len(shard) >= 2 ** 31:
            raise DrnError("ShardedShortlister: %d videos with shard %d, outside [1, 2^31)" % (self.bases[-1] + len(shard), len(self.shards)))
        self.shards.append(shard)
        self.bases.append(self.bases[-1] + len(shard))
        if self.names is not None:
            self.names = None if shard.names is None else self.names + list(shard.names)

    def _placed(self):
        """After the shards changed: the buffers kept for the old K are dropped, and bases and blk_off go to the device (uploads from
        pinned memory, no synchronise)."""
        self._bufs = {}
        self.blk_off = [0]                       # the running sums of the shards' counting blocks: where each count region starts
        for shard in self.shards:
            self.blk_off.append(self.blk_off[-1] + shard._nblocks())
        bases, blk_off = torch.tensor(self.bases, dtype=torch.int32), torch.tensor(self.blk_off, dtype=torch.int32)
        dev = self.device
        self.bases_device = bases if dev.type != "cuda" else bases.pin_memory().to(dev, non_blocking=True)
        self.blk_off_device = blk_off if dev.type != "cuda" else blk_off.pin_memory().to(dev, non_blocking=True)
        # nonempty follows the shards: where a shard came from pooled(group=None) with videos that own no row, the corpus's mask is the
        # shards' host masks side by side (a shard without one allows all its videos), made again after every append
        self.nonempty = None
        if any(shard._owners is not None for shard in self.shards):
            owners = [np.ones(len(shard), dtype=np.bool_) if shard._owners is None else shard._owners for shard in self.shards]
            self.nonempty = _mask_words(np.concatenate(owners), dev)

    def append(self, shard):
        """One more shard at the end of the corpus -- the same checks as the constructor, before anything changes -- at the positions
        bases[K] .. bases[K] + len(shard) - 1.  The resident shards are not touched, nothing is copied and nothing synchronises (the
        new shard's own constructor did, once, over its own rows); the stacked buffers kept for the old K are dropped, so warm a
        shape again before capturing it in a graph.  -> self."""
        self._admit(shard)
        self._placed()
        return self

    @property
    def device(self):
        return self.shards[0]._table().device

    @property
    def E(self):
        return self.shards[0].E

    @property
    def dtype(self):
        """The dtype of the queries shortlist() takes (a quantised shard's recorded dtype)."""
        return self.shards[0].dtype

    @property
    def nbytes(self):
        """The bytes of the tables held, the sum over the shards."""
        return sum(shard.nbytes for shard in self.shards)

    def __len__(self):
        return self.bases[-1]

    def check(self, store):
        """Raises unless the corpus's names are the store's (a FeatureStore or a SearchIndex), position by position."""
        if self.names is None or self.names != list(store.names):
            raise DrnError("ShardedShortlister: the corpus's names are not the store's (position v must belong to store position v)")

    def allow_of(self, keep=None, drop=None):
        """Shortlister.allow_of over the CORPUS: names (resolved through self.names) or corpus positions in [0, V) -> a packed mask
        (W,) int32 over all V videos on the shards' device, what shortlist(allow=) takes here."""
        return _allow_of("ShardedShortlister.allow_of", self.names, len(self), self.device, keep, drop)

    def compact(self, keep=None, quantize="same", stage_elems=None):
        """COMPACT the corpus: ONE new Shortlister over the videos `keep` keeps, in corpus order, built on the device -> Compacted(table,
        positions, kept); compact_reference is the definition, field for field and byte for byte.  keep: None -- every video survives,
        the shards are only joined -- or a packed mask over the corpus, contiguous int32 (W,) on the shards' device, W = ceil(V / 32):
        what pack_allow and allow_of(drop=[...]) return (a per-sentence (S, W) mask is refused: a video is in the table or it is
        not).  quantize: the format of the result, None for plain in self.dtype, "mxfp8", or "same" (the default), the shards'
        common format; "same" on mixed shards raises before any launch and says to pass one.

        table is plain or ragged as the shards are and owns its memory (no view of a shard); names are filtered when the corpus has
        names; a ragged result has new offsets and a new block plan, and a kept video that owns no row stays one.  positions (V,) int32
        on the device: the new position of corpus position v, -1 where v was dropped; kept: the host integer V'.  The shards are not
        modified.  V' = 0 raises, and so does a ragged result without a row: a table needs one; nothing half-built is left behind.
        ShardedShortlister([one_table]).compact(keep) drops videos from a single table.

        Per row, by source -> target format: plain -> plain, the values as they are; mxfp8 -> mxfp8, codes and scale bytes COPIED byte
        for byte (a dequantised row is never requantised: mx8_quantize(mx8_dequantize(.)) is not promised to be the identity);
        mxfp8 -> plain, mx8_dequantize(codes, scales, dtype), exact; plain -> mxfp8, mx8_quantize(rows) byte for byte, what
        Shortlister(rows, quantize="mxfp8") writes.  Two consequences:
        1. Where no row goes plain -> mxfp8 (the target is plain, or every shard is FP8 already), table answers shortlist,
           shortlist_late, rank, rank_late, rerank and rerank_late bit for bit as this object does under allow=keep, with ids,
           targets and candidates mapped through positions: a score's bits depend on the sentence and the video's rows alone, and the
           map is monotone, so ties fall the same way.
        2. Where a plain shard is quantised the result equals Shortlister(those rows, quantize="mxfp8"): lossy against the shard,
           exactly as the constructor is.

        The launches, in order: with keep=, drn_allow_slices; K plan launches (drn_compact_plan, one workgroup each, a running carry
        from shard to shard); then the host synchronises ONCE -- one transfer brings the carry (V', R' and each shard's share), the mask
        words for names and, on ragged shards, the new offsets for plan_segment_blocks; no table data crosses to the host --, the
        destination is allocated, and every shard's kept rows are moved by one drn_compact_rows launch.  A plain shard on its way to
        FP8 goes through a staging buffer of at most stage_elems elements (COMPACT_STAGE_ELEMS when None, a choice): per chunk of
        stage_elems // E destination rows one rows launch and one ops.quantize_rows_mx8, the one quantiser, and none where the shard
        keeps no row.  The result is built WITHOUT reading the table again for finiteness: every value is a copy or an exact
        dequantisation of one its shard's constructor checked.  Out of place: peak memory is the sources plus the destination (plus
        the staging buffer).  It synchronises by design and cannot be captured in a graph."""
        what = "ShardedShortlister.compact"
        K, V, E, dev, dtype = len(self.shards), len(self), self.E, self.device, self.dtype
        target = _compact_target(what, self.shards, quantize, E)
        W = ops.allow_words(V)
        if keep is not None:
            if not torch.is_tensor(keep) or keep.dtype != torch.int32:
                raise DrnError("%s: keep must be a packed mask, a torch.int32 tensor (pack_allow or allow_of makes one), not %s"
                               % (what, keep.dtype if torch.is_tensor(keep) else type(keep).__name__))
            if keep.dim() == 2:
                raise DrnError("%s: keep is a per-sentence mask %s; a compaction takes ONE mask (%d,) over the corpus: a video is in the "
                               "table or it is not" % (what, tuple(keep.shape), W))
            if tuple(keep.shape) != (W,) or not keep.is_contiguous():
                raise DrnError("%s: keep must be a contiguous (%d,) tensor, ceil(V / 32) words for V = %d videos, not %s"
                               % (what, W, V, tuple(keep.shape)))
            if not keep.is_cuda or keep.device != dev:
                raise DrnError("%s: keep must be on the shards' device %s, not %s" % (what, dev, keep.device))
        if not self.shards[0]._table().is_cuda:
            raise DrnError("%s: the shards must be on the GPU; there is no CPU fallback (compact_reference is the definition)" % what)
        stage_elems = COMPACT_STAGE_ELEMS if stage_elems is None else int(stage_elems)
        if stage_elems < 1:
            raise DrnError("%s: stage_elems = %d below 1" % (what, stage_elems))
        if sum(int(shard._table().shape[0]) for shard in self.shards) >= 2 ** 31:
            raise DrnError("%s: the shards hold 2^31 rows or more; one table holds fewer" % what)
        ragged = self.shards[0]._seg is not None
        words = keep is not None and self.names is not None
        # ONE buffer for everything the host needs: the carry (K + 1, 2), the mask words (for names), the new offsets (V + 1)
        head = torch.empty(2 * (K + 1) + (W if words else 0) + (V + 1 if ragged else 0), dtype=torch.int32, device=dev)
        carry, at = head[:2 * (K + 1)].view(K + 1, 2), 2 * (K + 1)
        if words:
            head[at:at + W].copy_(keep)
            at += W
        new_off = head[at:] if ragged else None
        positions = torch.empty(V, dtype=torch.int32, device=dev)
        spans = list(zip(self.bases[:-1], self.bases[1:]))
        for k, (shard, piece, (a, b)) in enumerate(zip(self.shards, self._slices(keep), spans)):
            ops.compact_plan(piece, shard._seg[0] if ragged else None, k, carry, positions[a:b], new_off)
        host = head.cpu()                        # THE one synchronise
        cum = host[:2 * (K + 1)].view(K + 1, 2).tolist()
        kept, R = cum[K]
        if kept < 1:
            raise DrnError("%s: the mask keeps no video: a table needs one" % what)
        if R < 1:
            raise DrnError("%s: the %d videos the mask keeps own no row: a table needs one" % (what, kept))
        names = None
        if self.names is not None:
            names = list(self.names)
            if words:
                live = np.unpackbits(host[at - W:at].numpy().view(np.uint8), bitorder="little")[:V]
                names = [name for name, bit in zip(names, live) if bit]
        offsets = host[at:at + kept + 1].numpy().astype(np.int64) if ragged else None
        if target is None:
            dst = torch.empty((R, E), dtype=dtype, device=dev)
        else:
            dst = (torch.empty((R, E), dtype=torch.uint8, device=dev), torch.empty((R, E // MX8_BLOCK), dtype=torch.uint8, device=dev))
        staged = [cum[k + 1][1] - cum[k][1] for k, shard in enumerate(self.shards) if shard.quantize is None and target is not None]
        step = max(1, stage_elems // E)
        stage = torch.empty((min(step, max(staged)), E), dtype=dtype, device=dev) if staged and max(staged) else None
        for k, (shard, (a, b)) in enumerate(zip(self.shards, spans)):
            src, src_off = shard._operand(), shard._seg[0] if ragged else None
            if int(shard._table().shape[0]) == 0:     # (a shard that holds no row -- no constructor makes one -- has none to move)
                continue
            if shard.quantize is None and target is not None:
                for r0 in range(cum[k][1], cum[k + 1][1], step):
                    r1 = min(r0 + step, cum[k + 1][1])
                    ops.compact_rows(src, src_off, positions[a:b], new_off, kept, stage[:r1 - r0], dst_row0=r0)
                    ops.quantize_rows_mx8(stage[:r1 - r0], dst[0][r0:r1], dst[1][r0:r1])
            else:
                ops.compact_rows(src, src_off, positions[a:b], new_off, kept, dst, dtype=dtype)
        return Compacted(_trusted_table(dst, dtype, names, offsets), positions, kept)

    def pooled(self, how="mean", group=None, quantize="same", stage_elems=None):
        """Shortlister.pooled over the CORPUS -> a new ShardedShortlister of the shards' pooled tables, shard by shard: the same
        arguments, definition (pool_segments_reference of each shard; a group never crosses a video, so never a shard), refusals and
        launches, and one synchronise a shard.  The video counts, bases and names are unchanged, so the result is a legal `coarse`
        beside this corpus as `fine`, and it answers shortlist() bit for bit like the pooled() of ONE table over the concatenated
        rows.  quantize="same" keeps every shard's own format and is refused on mixed shards, as compact() refuses it; None or
        "mxfp8" gives every shard that format.  nonempty, with group=None, is the packed (W,) mask OVER THE CORPUS of the videos that
        own a row (what allow_of(keep=those videos) returns), None when every video owns one: a video without rows is a row of
        ZEROS there, scores 0 and IS a candidate unless allow=result.nonempty is passed.  Every shard of the result carries its own
        nonempty over its own videos, and the corpus's is put together from the shards' whenever the shards change: after
        result.append(new_shard.pooled()) it covers the new videos too (a NEW tensor: read result.nonempty again after an append; a
        shard that did not come from pooled() allows all its videos).  The shards must be ragged."""
        what = "ShardedShortlister.pooled"
        group = ops.pool_args(what, how, group)
        if self.shards[0]._seg is None:
            raise DrnError("%s: the shards have no offsets=: they are one row a video already, and there is nothing to pool" % what)
        target = _compact_target(what, self.shards, quantize, self.E)
        return ShardedShortlister([shard._pooled(what, how, group, target, stage_elems) for shard in self.shards])

    def _lists(self, S, n):
        """The stacked per-shard lists of this (K, S, n): slices along dim 0 are contiguous, legal out= buffers of the shards."""
        K = len(self.shards)
        bufs = self._bufs.get((K, S, n))
        if bufs is None:
            dev = self.device
            bufs = (torch.empty((K, S, n), dtype=torch.int32, device=dev), torch.empty((K, S, n), dtype=torch.float32, device=dev),
                    torch.empty((K, S), dtype=torch.int32, device=dev))
            if self.shards[0]._seg is not None:
                bufs += (torch.empty((K, S, n), dtype=torch.int32, device=dev),)
            self._bufs[(K, S, n)] = bufs
        return bufs

    def _slices(self, allow):
        """A mask over the corpus -> the K shards' own masks, views of one buffer kept per (K, rows): ONE launch."""
        if allow is None:
            return [None] * len(self.shards)
        K, rows = len(self.shards), 1 if allow.dim() == 1 else int(allow.shape[0])
        buf = self._bufs.get(("allow", K, rows))
        if buf is None:
            buf = self._bufs[("allow", K, rows)] = torch.empty(rows * ops.allow_slice_words(self.bases), dtype=torch.int32, device=self.device)
        ops.allow_slices(allow, self.bases_device, self.bases, buf)
        pieces, at = [], 0
        for a, b in zip(self.bases[:-1], self.bases[1:]):
            W = ops.allow_words(b - a)
            piece = buf[at:at + rows * W]
            pieces.append(piece if allow.dim() == 1 else piece.view(rows, W))
            at += rows * W
        return pieces

    def shortlist(self, queries, n, out=None, allow=None):
        """Shortlister.shortlist over the corpus -> Shortlist, or SegmentShortlist on ragged shards, with CORPUS positions in ids:
        the arguments, the refusals, the padding (-1 / 0 / -1) and out= of the single table's method, and every field bit for bit what
        one Shortlister over the concatenated rows returns (over the concatenation of dequantized() rows where shards are
        quantised).  allow: a packed mask over the WHOLE corpus, (W,) or (S, W) with W = ceil(V / 32), from pack_allow or allow_of.
        Each shard runs its own entry, unchanged, into slice [k] of buffers kept per (K, S, n); then ONE merge launch; with allow=,
        one slicing launch first.  All on the current stream, without a host synchronisation, and it can be captured in a graph once
        the shape is warmed, where the queries and the mask's contents may change in place between replays."""
        first = self.shards[0]
        S, n = first._check(queries, n, out)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        ragged = first._seg is not None
        if out is None:
            out = _list_buffers(self.device, S, n, rows=ragged)
        lists = self._lists(S, n)
        queries = queries.contiguous()
        for k, (shard, piece) in enumerate(zip(self.shards, self._slices(allow))):
            shard.shortlist(queries, n, out=tuple(t[k] for t in lists), allow=piece)
        if ragged:
            ops.shortlist_merge_lists(lists[0], lists[1], lists[2], lists[3], self.bases_device, n, out[0], out[1], out[2], out[3])
            return SegmentShortlist(*out)
        ops.shortlist_merge_lists(lists[0], lists[1], lists[2], None, self.bases_device, n, out[0], out[1], out[2])
        return Shortlist(*out)

    def shortlist_late(self, queries, lengths, n, out=None, allow=None):
        """Shortlister.shortlist_late over the corpus (ragged shards) -> Shortlist with CORPUS positions: arguments, refusals, padding
        and out= as there, allow= over the whole corpus as in shortlist(), every field bit for bit the single table's.  Each shard
        runs its own entry into slice [k] of the stacked buffers, then ONE merge launch; no host synchronisation, capturable once
        warmed, where queries, lengths and the mask's contents may change in place between replays."""
        what = "Shortlister.shortlist_late"
        first = self.shards[0]
        if first._seg is None:
            _refuse_late(what, "shortlist", whose="these tables have")
        S, L, n = first._check_late(what, queries, lengths, n)
        if out is not None:
            _check_list_out(what, out, S, n)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        if out is None:
            out = _list_buffers(self.device, S, n)
        lists = self._lists(S, n)
        for k, (shard, piece) in enumerate(zip(self.shards, self._slices(allow))):
            shard.shortlist_late(queries, lengths, n, out=tuple(t[k] for t in lists[:3]), allow=piece)
        ops.shortlist_merge_lists(lists[0], lists[1], lists[2], None, self.bases_device, n, out[0], out[1], out[2])
        return Shortlist(*out)

    def _rank(self, what, queries, lengths, targets, out, allow):
        """What rank (lengths=None) and rank_late share: the refusals of the single table's method, then 2 K + 3 launches."""
        first = self.shards[0]
        if lengths is not None and first._seg is None:
            _refuse_late(what, "rank", whose="these tables have")
        S = first._check_rank_queries(what, queries, lengths)
        out = first._check_rank(what, S, targets, out, None)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        if lengths is None:
            queries = queries.contiguous()
        K, blocks = len(self.shards), [b - a for a, b in zip(self.blk_off[:-1], self.blk_off[1:])]
        bufs = self._bufs.get(("rank", K, S))
        if bufs is None:
            dev = self.device
            bufs = self._bufs[("rank", K, S)] = (torch.empty((K, S), dtype=torch.int32, device=dev), torch.empty((S,), dtype=torch.int64, device=dev),
                                                 torch.empty(ops.shortlist_sharded_rank_ws_keys(blocks, S), dtype=torch.int64, device=dev))
        local, key, ws = bufs
        keys, thresholds, cnt = ws[:K * S].view(K, S), ws[K * S:2 * K * S].view(K, S), ws[2 * K * S:]
        ops.shard_positions(targets, self.bases_device, local)
        pieces = self._slices(allow)
        for k, (shard, piece) in enumerate(zip(self.shards, pieces)):
            shard._rank_keys(what, queries, lengths, local[k], keys[k], piece)
        ops.shortlist_rank_thresholds(keys, thresholds, key)
        for k, (shard, piece) in enumerate(zip(self.shards, pieces)):
            shard._rank_counts(what, queries, lengths, thresholds[k], cnt[S * self.blk_off[k]:S * self.blk_off[k + 1]], piece)
        ops.shortlist_rank_reduce_shards(key, cnt, self.blk_off_device, self.blk_off[-1], *out)
        return TargetRank(*out)

    def rank(self, queries, targets, out=None, allow=None):
        """Shortlister.rank over the corpus -> TargetRank: targets are CORPUS positions (a value outside [0, V) means "no target"),
        allow a packed mask over the whole corpus; the arguments, the refusals, out= and every field bit for bit what one Shortlister
        over the concatenated rows returns (rank_reference over them -- segment_rank_reference on ragged shards -- is the
        definition).  The launches, in order: drn_shard_positions; with allow=, drn_allow_slices; K target-key launches, each shard's
        own; one thresholds launch; K counting launches, each shard's own; one reduce.  All on the current stream, without a host
        synchronisation, and capturable in a graph once the shape is warmed (the buffers are kept per (K, S)), where queries, targets
        and the mask's contents may change in place between replays."""
        return self._rank("Shortlister.rank", queries, None, targets, out, allow)

    def rank_late(self, queries, lengths, targets, out=None, allow=None):
        """Shortlister.rank_late over the corpus (ragged shards) -> TargetRank, as rank(): every field bit for bit the single table's
        (late_rank_reference over the concatenated rows is the definition); queries, lengths, targets and the mask's contents may
        change in place between replays of a captured graph.  Shards without offsets are refused as in shortlist_late()."""
        what = "Shortlister.rank_late"
        if not torch.is_tensor(lengths):
            raise DrnError("%s: lengths must be a contiguous torch.int32 tensor on the device, the live tokens of each sentence" % what)
        return self._rank(what, queries, lengths, targets, out, allow)

    def _scores(self, what, S, queries, lengths, out, allow):
        """What scores (lengths=None) and scores_late share once their queries are checked: shard k writes the columns bases[k] ..
        bases[k + 1] - 1 of out through its row stride -- K launches and no merge; with allow=, one slicing launch first."""
        dev, V = self.device, len(self)
        if out is None:
            out = torch.empty((S, V), dtype=torch.float32, device=dev)
        else:
            _check_scores_out(what, out, S, V, dev)
        if allow is not None:
            _check_packed_allow(allow, S, V, dev)
        for shard, piece, a, b in zip(self.shards, self._slices(allow), self.bases[:-1], self.bases[1:]):
            shard._scores(what, S, queries, lengths, out[:, a:b], piece)
        return out

    def scores(self, queries, out=None, allow=None):
        """Shortlister.scores over the corpus -> float32 (S, V), column v the corpus's video v: the arguments, the refusals and out=
        of the single table's method, and every element bit for bit what one Shortlister over the concatenated rows writes (a score's
        bits do not depend on the table that holds the video).  allow: a packed mask over the WHOLE corpus.  Each shard writes its own
        columns of out in place: K launches, one more under a mask, NO merge; no host synchronisation, capturable once the mask's
        slices are warmed."""
        what = "Shortlister.scores"
        S = self.shards[0]._check_rank_queries(what, queries, None)
        return self._scores(what, S, queries.contiguous(), None, out, allow)

    def scores_late(self, queries, lengths, out=None, allow=None):
        """Shortlister.scores_late over the corpus (ragged shards) -> float32 (S, V), as scores().  Shards without offsets are refused
        as in shortlist_late()."""
        what = "Shortlister.scores_late"
        if self.shards[0]._seg is None:
            _refuse_late(what, "scores", whose="these tables have")
        if not torch.is_tensor(lengths):
            raise DrnError("%s: lengths must be a contiguous torch.int32 tensor on the device, the live tokens of each sentence" % what)
        S = self.shards[0]._check_rank_queries(what, queries, lengths)
        return self._scores(what, S, queries, lengths, out, allow)

    def _rerank(self, what, candidates, queries, lengths, n, out, allow):
        """What rerank (lengths=None) and rerank_late share: the refusals of the single table's method, then K + 2 launch groups."""
        first = self.shards[0]
        late = lengths is not None
        if late and first._seg is None:
            _refuse_late(what, "rerank", whose="these tables have")
        S, C, n = first._check_candidates(what, candidates, n)
        if late:
            Sq, _, _ = first._check_late(what, queries, lengths)
            if Sq != S:
                raise DrnError("%s: the queries hold %d sentences, candidates has %d rows" % (what, Sq, S))
        else:
            first._check_queries(what, queries, S)
        if out is not None:
            _check_list_out(what, out, S, n)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        if out is None:
            out = _list_buffers(self.device, S, n)
        K = len(self.shards)
        local = self._bufs.get(("positions", K, S, C))
        if local is None:
            local = self._bufs[("positions", K, S, C)] = torch.empty((K, S, C), dtype=torch.int32, device=self.device)
        ops.shard_positions(candidates, self.bases_device, local)
        lists = self._lists(S, n)[:3]
        for k, (shard, piece) in enumerate(zip(self.shards, self._slices(allow))):
            into = tuple(t[k] for t in lists)
            if late:
                shard.rerank_late(local[k], queries, lengths, n, out=into, allow=piece)
            else:
                shard.rerank(local[k], queries, n, out=into, allow=piece)
        ops.shortlist_merge_lists(lists[0], lists[1], lists[2], None, self.bases_device, n, out[0], out[1], out[2])
        return Shortlist(*out)

    def rerank(self, candidates, queries, n=None, out=None, allow=None):
        """Shortlister.rerank over the corpus -> Shortlist with CORPUS positions: candidates (S, C) hold corpus positions -- the ids
        of any shortlist over the same corpus, sharded or not, as they are --, allow is a packed mask over the whole corpus; the
        arguments, the refusals, the padding and out= of the single table's method, and every field bit for bit what one Shortlister
        over the concatenated rows returns (rerank_reference over them -- segment_rerank_reference on ragged shards -- is the
        definition).  The launches, in order: drn_shard_positions into a (K, S, C) buffer (a candidate that lies in another shard
        becomes -1, which means nothing); with allow=, drn_allow_slices; each shard's own rerank, unchanged, on slice [k] into slice
        [k] of the stacked lists; drn_shortlist_merge_lists.  A shard's rerank of the candidates inside it is its filtered shortlist,
        so the merge is shortlist()'s.  All on the current stream, without a host synchronisation, capturable once warmed (buffers
        per (K, S, C) and (K, S, n)), where candidates, queries and the mask's contents may change in place between replays."""
        return self._rerank("Shortlister.rerank", candidates, queries, None, n, out, allow)

    def rerank_late(self, candidates, queries, lengths, n=None, out=None, allow=None):
        """Shortlister.rerank_late over the corpus (ragged shards) -> Shortlist with CORPUS positions, as rerank(): every field bit
        for bit the single table's (late_rerank_reference over the concatenated rows is the definition).  Shards without offsets are
        refused as in shortlist_late()."""
        what = "Shortlister.rerank_late"
        if not torch.is_tensor(lengths):
            raise DrnError("%s: lengths must be a contiguous torch.int32 tensor on the device, the live tokens of each sentence" % what)
        return self._rerank(what, candidates, queries, lengths, n, out, allow)


    def _rerank_scores(self, what, S, C, candidates, queries, lengths, out, allow, inside_only=False):
        """What rerank_scores and rerank_scores_late share once their tensors are checked (queries (S, L, E), candidates CORPUS
        positions): drn_shard_positions into the (K, S, C) buffer _rerank keeps, the mask's slices, then each shard's own launch into
        the ONE matrix in stream order -- shard 0 writes every slot (-inf where the id lies in no shard, or in another), the shards
        after it only the slots that fall inside them: K + 1 launch groups, one more under a mask."""
        dev, K = self.device, len(self.shards)
        if out is None:
            out = torch.empty((S, C), dtype=torch.float32, device=dev)
        else:
            _check_scores_out(what, out, S, C, dev)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), dev)
        local = self._bufs.get(("positions", K, S, C))
        if local is None:
            local = self._bufs[("positions", K, S, C)] = torch.empty((K, S, C), dtype=torch.int32, device=dev)
        ops.shard_positions(candidates, self.bases_device, local)
        for k, (shard, piece) in enumerate(zip(self.shards, self._slices(allow))):
            shard._rerank_scores(what, S, C, local[k], queries, lengths, out, piece, inside_only=inside_only or k > 0)
        return out

    def rerank_scores(self, candidates, queries, out=None, allow=None):
        """Shortlister.rerank_scores over the corpus -> float32 (S, C): candidates hold CORPUS positions, allow is a packed mask over
        the whole corpus; the arguments, the refusals and out= of the single table's method, and every element bit for bit what one
        Shortlister over the concatenated rows writes (rerank_scores_reference over them is the definition).  The launches, in
        order: drn_shard_positions; with allow=, drn_allow_slices; each shard's own drn_shortlist_rerank_scores on slice [k] into the
        SAME matrix -- shard 0 writes every slot, the others only the slots that fall inside them.  All on the current stream, no
        host synchronisation, capturable once warmed (the positions are kept per (K, S, C))."""
        what = "Shortlister.rerank_scores"
        S, C, q = self.shards[0]._check_rerank_scores(what, candidates, queries, None)
        return self._rerank_scores(what, S, C, candidates, q, None, out, allow)

    def rerank_scores_late(self, candidates, queries, lengths, out=None, allow=None):
        """Shortlister.rerank_scores_late over the corpus (ragged shards) -> float32 (S, C), as rerank_scores().  Shards without
        offsets are refused as in shortlist_late()."""
        what = "Shortlister.rerank_scores_late"
        if self.shards[0]._seg is None:
            _refuse_late(what, "rerank_scores", whose="these tables have")
        if not torch.is_tensor(lengths):
            raise DrnError("%s: lengths must be a contiguous torch.int32 tensor on the device, the live tokens of each sentence" % what)
        S, C, q = self.shards[0]._check_rerank_scores(what, candidates, queries, lengths)
        return self._rerank_scores(what, S, C, candidates, q, lengths, out, allow)


def _check_matrix(what, scores):
    """What shortlist_scores refuses about its matrix, before the library is reached -> (S, V)."""
    if not torch.is_tensor(scores) or not scores.is_cuda:
        raise DrnError("%s: scores must be a tensor on the GPU; there is no CPU fallback (fused_shortlist_reference is the definition)" % what)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise DrnError("%s: scores must be a (S, V) torch.float32 tensor with S >= 1 and V >= 1, not %s %s"
                       % (what, scores.dtype, tuple(scores.shape)))
    S, V = (int(x) for x in scores.shape)
    if (V > 1 and scores.stride(1) != 1) or (S > 1 and scores.stride(0) < V):
        raise DrnError("%s: scores must have last stride 1 and row stride >= %d, not strides %s" % (what, V, tuple(scores.stride())))
    return S, V


def _check_depth(what, n):
    """1 <= n <= SHORTLIST_DEEP_MAX -> n."""
    n = int(n)
    if not 1 <= n <= SHORTLIST_DEEP_MAX:
        raise DrnError("%s: n = %d outside [1, %d]" % (what, n, SHORTLIST_DEEP_MAX))
    return n


def shortlist_scores(scores, n, allow=None, out=None):
    """RANK A SCORE MATRIX the caller already has under the project's total order -> Shortlist, on the device
    (fused_shortlist_reference(scores[None], None, n) defines it).  scores: float32 (S, V) on the GPU, last stride 1 and row stride
    >= V -- what Shortlister.scores returns, or anything computed from it: calibrated, thresholded, distilled.  An entry that is not
    finite (-inf, +inf, NaN) is NO CANDIDATE; the others are listed by higher score, then lower position, cut to 1 <= n <=
    SHORTLIST_DEEP_MAX, with -1 / 0 past the list, and a listed score has the entry's bits (-0 as +0).  So
    shortlist_scores(table.scores(q), n) is table.shortlist(q, n) -- table.shortlist_deep(q, n) above SHORTLIST_MAX -- without its rows.
    allow: a packed mask over the V columns, as in Shortlister.shortlist.  out: the three buffers of a Shortlist, written in place.
    Two launches (drn_shortlist_fuse_topn with one matrix and the weight 1: 0 + 1 * s is exact), no host synchronisation; the
    workspace is allocated per call."""
    what = "shortlist_scores"
    S, V = _check_matrix(what, scores)
    n = _check_depth(what, n)
    if out is not None:
        _check_list_out(what, out, S, n)
    if allow is not None:
        _check_packed_allow(allow, S, V, scores.device)
    if out is None:
        out = _list_buffers(scores.device, S, n)
    ws = torch.empty(ops.shortlist_ws_keys(V, S, n), dtype=torch.int64, device=scores.device)
    one = torch.ones(1, dtype=torch.float32, device=scores.device)
    ops.shortlist_fuse_topn(scores.unsqueeze(0), one, "drop", n, ws, *out, allow=allow)
    return Shortlist(*out)


def _fused_tables(what, tables, missing, cap):
    """What FusedShortlister and RankFusedShortlister refuse about their tables and `missing` -> (the tables as a list, the names of
    the first table that has any): 1 to cap tables over the same videos on one device, equal names position by position."""
    try:
        tables = list(tables)
    except TypeError:
        raise DrnError("%s: the tables must be a sequence of Shortlister / ShardedShortlister objects" % what)
    if not 1 <= len(tables) <= cap:
        raise DrnError("%s: %d tables outside [1, %d]" % (what, len(tables), cap))
    if missing not in FUSE_MODES:
        raise DrnError("%s: missing must be \"drop\" or \"skip\", not %r" % (what, missing))
    names = None
    for m, table in enumerate(tables):
        if not isinstance(table, (Shortlister, ShardedShortlister)):
            raise DrnError("%s: table %d must be a Shortlister or a ShardedShortlister, not %s" % (what, m, type(table).__name__))
        if len(table) != len(tables[0]):
            raise DrnError("%s: table %d holds %d videos, table 0 holds %d: the tables must rank the same videos, position by position"
                           % (what, m, len(table), len(tables[0])))
        if table.device != tables[0].device:
            raise DrnError("%s: table %d is on %s, table 0 on %s" % (what, m, table.device, tables[0].device))
        if table.names is not None:
            if names is not None and list(table.names) != names:
                raise DrnError("%s: the names of table %d are not those of the tables before it (position v must be the same video "
                               "in every table)" % (what, m))
            names = list(table.names)
    return tables, names


def _fused_weights(what, weights, M, dev, things):
    """The weights of a fusion of M `things` ("tables", "lists") on dev -> a float32 (M,) tensor on dev: None is all ones, host numbers
    are rounded to fp32 and uploaded ONCE through pinned memory, a device tensor is checked and kept BY REFERENCE."""
    if weights is None:
        w = torch.ones(M, dtype=torch.float32)
    elif torch.is_tensor(weights):
        if weights.dtype != torch.float32 or tuple(weights.shape) != (M,) or not weights.is_contiguous():
            raise DrnError("%s: a weights tensor must be contiguous (%d,) torch.float32, one weight per %s, not %s %s"
                           % (what, M, things[:-1], weights.dtype, tuple(weights.shape)))
        if weights.device != dev:
            raise DrnError("%s: a weights tensor must be on the %s' device %s (it is kept by reference and never read on the "
                           "host); pass a host sequence to have it uploaded" % (what, things, dev))
        return weights
    else:
        try:
            w = torch.tensor([float(x) for x in weights], dtype=torch.float32)
        except (TypeError, ValueError):
            raise DrnError("%s: weights must be None, %d numbers or a float32 (%d,) tensor on the device" % (what, M, M))
        if tuple(w.shape) != (M,):
            raise DrnError("%s: %d weights for %d %s" % (what, int(w.shape[0]), M, things))
    return w.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else w


def _check_fused_items(what, tables, queries):
    """What FusedShortlister and RankFusedShortlister refuse about the M query items, one per table, ALL before the first launch ->
    (S, [(queries, lengths)] * M)."""
    M = len(tables)
    if not isinstance(queries, (list, tuple)) or len(queries) != M:
        raise DrnError("%s: queries must be a sequence of %d items, one per table: what the table's scores() takes, or a pair "
                       "(queries, lengths) for its scores_late()" % (what, M))
    items, S = [], None
    for m, (table, item) in enumerate(zip(tables, queries)):
        q, lengths = (item[0], item[1]) if isinstance(item, (list, tuple)) and len(item) == 2 else (item, None)
        if isinstance(item, (list, tuple)) and len(item) != 2:
            raise DrnError("%s: item %d must be a queries tensor or a pair (queries, lengths)" % (what, m))
        first = table if isinstance(table, Shortlister) else table.shards[0]
        if lengths is not None and not torch.is_tensor(lengths):
            raise DrnError("%s: the lengths of item %d must be a contiguous torch.int32 tensor on the device" % (what, m))
        Sm = first._check_rank_queries("%s (table %d)" % (what, m), q, lengths)
        if S is not None and Sm != S:
            raise DrnError("%s: item %d holds %d sentences, item 0 holds %d" % (what, m, Sm, S))
        S = Sm
        items.append((q if lengths is not None else q.contiguous(), lengths))
    return S, items


class FusedShortlister(object):
    """FusedShortlister(tables, weights=None, missing="drop"): ONE ranking of several tables over the same videos -- a visual window
    table, a subtitle table, a pooled coarse table, an FP8 copy: score[s, v] = w_0 * score_0[s, v] + w_1 * score_1[s, v] + ..., each
    table scoring the video its own way (its best row over its own offsets, its own E and dtype, its own late interaction), the sum
    folded in a FIXED order in fp32 (fuse_scores_reference defines it: two roundings a term), and the list cut under the one total
    order (fused score descending, then position ascending).  Over ragged tables this is no concatenation: every modality takes its
    own maximum over its own rows.

    tables: 1 to FUSE_MAX_TABLES Shortlister / ShardedShortlister objects over the SAME V videos on one device, held by reference;
    where names are given they must be equal position by position (refused here, before any launch); E, dtype, offsets, quantisation
    and sharding may all differ.  weights: None (all ones), a host sequence of M numbers (rounded to fp32, uploaded ONCE through pinned
    memory) or a contiguous float32 (M,) tensor on the device, kept BY REFERENCE and never read on the host: its contents may change
    between calls and between replays of a captured graph.  missing: "drop" -- a video that is no candidate of ANY table (no row there,
    a score that is not finite) is no candidate of the answer -- or "skip" -- a table the video is missing from adds nothing (a video
    without subtitles), and only a video missing from every table is dropped.

    What this is NOT.  For tables of one row per video and one dtype it is the plain shortlist of the table of concatenated (weighted)
    columns, which is cheaper: one launch group and no dense buffer.  The dense buffers cost 4 * M * S * V bytes, kept per S, and
    the M score launches of shortlist() and rank() read every table whole.  The function fused_rerank(fused, candidates, queries, n) is the fused SECOND stage of a cascade: it scores
    only the listed (sentence, video) pairs -- 4 * M * S * C bytes of buffers, kept per (S, C), and only the listed videos' rows of
    every table are read -- so its cost grows with the list, not with the corpus.  No `rows` come back: a fused score has no single winning
    segment.  Attributes: tables, weights (the device tensor), missing, names (the first table's that has any), device; len() is V."""

    def __init__(self, tables, weights=None, missing="drop"):
        what = "FusedShortlister"
        tables, names = _fused_tables(what, tables, missing, FUSE_MAX_TABLES)
        weights = _fused_weights(what, weights, len(tables), tables[0].device, "tables")
        self.tables, self.weights, self.missing, self.names = tables, weights, missing, names
        self._bufs = {}

    @property
    def device(self):
        return self.tables[0].device

    def __len__(self):
        return len(self.tables[0])

    def _check_items(self, what, queries):
        """What shortlist() and rank() refuse about the M query items, ALL before the first launch -> (S, [(queries, lengths)] * M)."""
        return _check_fused_items(what, self.tables, queries)

    def _stack(self, what, S, items):
        """The M score launch groups (K launches on a sharded table), UNMASKED, into the stacked (M, S, V) buffer kept per S."""
        buf = self._bufs.get(("scores", S))
        if buf is None:
            buf = self._bufs[("scores", S)] = torch.empty((len(self.tables), S, len(self)), dtype=torch.float32, device=self.device)
        for m, (table, (q, lengths)) in enumerate(zip(self.tables, items)):
            table._scores(what, S, q, lengths, buf[m], None)
        return buf

    def shortlist(self, queries, n, out=None, allow=None):
        """Each sentence's best n videos under the fused score -> Shortlist, on the device (fused_shortlist_reference applied to the
        tables' own scores() is the definition, bit for bit).  queries: a sequence of M items, item m what table m's scores() takes --
        (S, E_m) in that table's dtype -- or a pair (queries (S, L, E_m), lengths (S,)) for its scores_late(); every item holds the same
        S sentences.  1 <= n <= SHORTLIST_DEEP_MAX.  out: the three buffers of a Shortlist, written in place.  allow: a packed mask
        over the V videos, as in Shortlister.shortlist; it is applied AFTER fusion, by the ranking launch alone: the score launches run
        unmasked, so a score matrix never depends on the mask.  M score launch groups (K launches on a table of K shards) into a
        stacked buffer kept per S, then drn_shortlist_fuse_topn (two launches); all on the current stream, no host synchronisation,
        and it can be captured in a graph once the shape is warmed (the buffers are kept per S and per (S, n)), where the queries,
        lengths, the weights tensor and the mask's contents may change in place between replays.  No `rows` are returned."""
        what = "FusedShortlister.shortlist"
        S, items = self._check_items(what, queries)
        n = _check_depth(what, n)
        if out is not None:
            _check_list_out(what, out, S, n)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        if out is None:
            out = _list_buffers(self.device, S, n)
        ws = self._bufs.get(("ws", S, n))
        if ws is None:
            ws = self._bufs[("ws", S, n)] = torch.empty(ops.shortlist_ws_keys(len(self), S, n), dtype=torch.int64, device=self.device)
        ops.shortlist_fuse_topn(self._stack(what, S, items), self.weights, self.missing, n, ws, *out, allow=allow)
        return Shortlist(*out)

    def rank(self, queries, targets, out=None, allow=None):
        """The place of each sentence's TARGET video in the full fused order -> TargetRank, on the device (fused_rank_reference
        applied to the tables' own scores() is the definition): queries as in shortlist(), targets, out= and allow= as in
        Shortlister.rank.  rank[s] = k >= 0 exactly when shortlist(queries, n).ids[s, k] is the target for every n > k, and score[s] has
        the listed score's bits.  M score launch groups, then ONE launch (drn_shortlist_fuse_rank); no host synchronisation,
        capturable once the shape is warmed.  evaluate_shortlist(fused, batches) works as it stands, batch[1] being the M items."""
        what = "FusedShortlister.rank"
        S, items = self._check_items(what, queries)
        table = self.tables[0]
        first = table if isinstance(table, Shortlister) else table.shards[0]
        out = first._check_rank(what, S, targets, out, None)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        ops.shortlist_fuse_rank(self._stack(what, S, items), self.weights, self.missing, targets, *out, allow=allow)
        return TargetRank(*out)


def fused_rerank(fused, candidates, queries, n=None, out=None, allow=None):
    """THE FUSED RERANK, a function beside shortlist_scores and NOT a method: FusedShortlister keeps the surface it had (its class has no
    `rerank`, which tests/test_fused_shortlist_cpu.py pins).  fused: a FusedShortlister -> each sentence's best n LISTED videos under
    its fused score, a Shortlist on the device (fused_rerank_reference applied to the tables' own rerank_scores() is the definition,
    bit for bit).  candidates: contiguous int32 (S, C) on the tables' device, 1 <= C <= RERANK_MAX_CANDIDATES, as in Shortlister.rerank
    -- another shortlist's ids as they lie on the device, -1 padding, repeats and out-of-range values included (over sharded tables:
    corpus positions).  queries: the M items of fused.shortlist(), a pair (queries, lengths) selecting that table's late scoring; every
    item holds S sentences.  n: None means C, otherwise 1 <= n <= SHORTLIST_DEEP_MAX (n > C is legal: the rest is padding).  out: the
    three buffers of a Shortlist.  allow: a packed mask over the V videos, applied by the ranking launch alone, as in
    fused.shortlist(): a score matrix never depends on the mask.

    Every field equals, bit for bit, fused.shortlist(queries, n, allow=pack_allow(candidates_mask(candidates, V) [& allow])): a fused
    score has the bits the full fused shortlist gives the pair and ties fall by store position, not by place in the list -- but only
    the listed videos' rows of every table are read, the buffers are 4 * M * S * C bytes and C columns are ranked, not V.
    drn_amd.search_eval.evaluate_cascade calls it where `fine` is a FusedShortlister.  M rerank_scores launch groups (K + 1 on a table of
    K shards), UNMASKED, into a stacked (M, S, C) buffer kept by `fused` per (S, C), then drn_shortlist_fuse_rerank (two launches; the
    workspace is kept per (S, C, n)); all on the current stream, no host synchronisation, and it can be captured in a graph once the
    shape is warmed, where candidates, the queries, lengths, the weights tensor and the mask's contents may change in place between
    replays.  No `rows` are returned."""
    what = "fused_rerank"
    if not isinstance(fused, FusedShortlister):
        raise DrnError("%s: the first argument must be a FusedShortlister, not %s" % (what, type(fused).__name__))
    S, items = fused._check_items(what, queries)
    table = fused.tables[0]
    first = table if isinstance(table, Shortlister) else table.shards[0]
    Sc, C, _ = first._check_candidates(what, candidates, None)
    if Sc != S:
        raise DrnError("%s: the queries hold %d sentences, candidates has %d rows" % (what, S, Sc))
    n = C if n is None else _check_depth(what, n)
    if out is not None:
        _check_list_out(what, out, S, n)
    if allow is not None:
        _check_packed_allow(allow, S, len(fused), fused.device)
    if out is None:
        out = _list_buffers(fused.device, S, n)
    buf = fused._bufs.get(("rerank", S, C))
    if buf is None:
        buf = fused._bufs[("rerank", S, C)] = torch.empty((len(fused.tables), S, C), dtype=torch.float32, device=fused.device)
    ws = fused._bufs.get(("rerank_ws", S, C, n))
    if ws is None:
        ws = fused._bufs[("rerank_ws", S, C, n)] = torch.empty(ops.shortlist_ws_keys(C, S, n), dtype=torch.int64, device=fused.device)
    for m, (table, (q, lengths)) in enumerate(zip(fused.tables, items)):
        table._rerank_scores(what, S, C, candidates, q if lengths is not None else q.view(S, 1, -1), lengths, buf[m], None)
    ops.shortlist_fuse_rerank(buf, fused.weights, fused.missing, candidates, len(fused), n, ws, *out, allow=allow)
    return Shortlist(*out)


_RANK_FUSE_WEIGHTS = {}   # (device, the host weights as a tuple) -> their tensor on the device: host weights are uploaded ONCE
_RANK_FUSE_WEIGHTS_KEPT = 64   # uploads kept before the cache is emptied: a CHOICE (a caller whose weights change passes a device tensor)


def _rank_fuse_weights(what, weights, M, dev):
    """weights= of rank_fuse / rank_fuse_rank -> a float32 (M,) tensor on dev: _fused_weights, host numbers cached by value."""
    if torch.is_tensor(weights):
        return _fused_weights(what, weights, M, dev, "lists")
    try:
        key = (str(dev), tuple(1.0 for _ in range(M)) if weights is None else tuple(float(x) for x in weights))
    except (TypeError, ValueError):
        key = None
    w = _RANK_FUSE_WEIGHTS.get(key)
    if w is None:
        w = _fused_weights(what, weights, M, dev, "lists")       # (raises what a bad sequence deserves)
        if len(_RANK_FUSE_WEIGHTS) >= _RANK_FUSE_WEIGHTS_KEPT:
            _RANK_FUSE_WEIGHTS.clear()
        _RANK_FUSE_WEIGHTS[key] = w
    return w


def _check_rank_fuse(what, lists, V, weights, k0, missing, allow):
    """What rank_fuse and rank_fuse_rank refuse about everything but their results, before the library is reached and before
    anything is launched -> (lists: the (M, S, C) tensor or the checked sequence, S, V, weights on the device, k0)."""
    if missing not in FUSE_MODES:
        raise DrnError("%s: missing must be \"drop\" or \"skip\", not %r" % (what, missing))
    V = int(V)
    if V < 1:
        raise DrnError("%s: V = %d videos, at least one is needed" % (what, V))
    k0 = _check_k0(what, k0)
    if torch.is_tensor(lists):
        seq, dims, shape = [lists], 3, "(M, S, C)"
    else:
        try:
            seq, dims, shape = list(lists), 2, "(S, C)"
        except TypeError:
            raise DrnError("%s: lists must be an (M, S, C) torch.int32 tensor on the device or a sequence of (S, C_m) ones" % what)
        if not 1 <= len(seq) <= RANK_FUSE_MAX_LISTS:
            raise DrnError("%s: %d lists outside [1, %d]" % (what, len(seq), RANK_FUSE_MAX_LISTS))
    for m, t in enumerate(seq):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise DrnError("%s: the lists must be tensors on the GPU; there is no CPU fallback (rank_fuse_reference is the definition)" % what)
        if t.dtype != torch.int32 or t.dim() != dims or not t.is_contiguous() or min(t.shape) < 1:
            raise DrnError("%s: a list must be a contiguous %s torch.int32 tensor -- another shortlist's ids -- not %s %s"
                           % (what, shape, t.dtype, tuple(t.shape)))
        if not 1 <= int(t.shape[-1]) <= SHORTLIST_DEEP_MAX:
            raise DrnError("%s: C = %d entries a sentence outside [1, %d]" % (what, int(t.shape[-1]), SHORTLIST_DEEP_MAX))
        if int(t.shape[-2]) != int(seq[0].shape[-2]):
            raise DrnError("%s: list %d holds %d sentences, list 0 holds %d" % (what, m, int(t.shape[-2]), int(seq[0].shape[-2])))
        if t.device != seq[0].device:
            raise DrnError("%s: list %d is on %s, list 0 on %s" % (what, m, t.device, seq[0].device))
    M = int(lists.shape[0]) if torch.is_tensor(lists) else len(seq)
    if not 1 <= M <= RANK_FUSE_MAX_LISTS:
        raise DrnError("%s: %d lists outside [1, %d]" % (what, M, RANK_FUSE_MAX_LISTS))
    S, dev = int(seq[0].shape[-2]), seq[0].device
    weights = _rank_fuse_weights(what, weights, M, dev)
    if allow is not None:
        _check_packed_allow(allow, S, V, dev)
    return (lists if torch.is_tensor(lists) else seq), S, V, weights, k0


def _stacked_lists(lists):
    """The checked lists of _check_rank_fuse -> one (M, S, C) int32 tensor: a sequence is copied into a buffer padded with -1, which
    means nothing, by M + 1 launches and no host synchronisation."""
    if torch.is_tensor(lists):
        return lists
    S, C = int(lists[0].shape[0]), max(int(t.shape[1]) for t in lists)
    buf = torch.full((len(lists), S, C), -1, dtype=torch.int32, device=lists[0].device)
    for m, t in enumerate(lists):
        buf[m, :, :int(t.shape[1])].copy_(t)
    return buf


def rank_fuse(lists, V, n, weights=None, k0=60.0, missing="skip", allow=None, out=None):
    """RECIPROCAL-RANK FUSION of several shortlists, on the device -> Shortlist (rank_fuse_reference defines it, bit for bit): the
    fusion for tables whose scores share no scale -- a bf16 window table, an FP8 copy, a pooled coarse table, a late-interaction
    subtitle table.  List m votes w[m] / (k0 + rank + 1) for each video it holds, the votes are added in fp32 in list order, and the
    videos are ranked by the sum under the project's total order (sum descending, then position ascending): fused reciprocal ranks
    tie constantly, and the ties fall the same way in every run and build.
    lists: a contiguous (M, S, C) torch.int32 tensor on the device, or a sequence of M contiguous (S, C_m) ones, 1 <= M <=
    RANK_FUSE_MAX_LISTS, 1 <= C_m <= SHORTLIST_DEEP_MAX -- other shortlists' ids as they lie on the device: -1 padding, repeats and
    out-of-range values mean what candidates_mask says, and a video's rank in a list is the column of its first occurrence.  A
    sequence is copied into a stacked buffer padded with -1, which by the definition changes nothing.  V: the videos of the store the
    positions index.  1 <= n <= SHORTLIST_DEEP_MAX.  weights: None (all ones), M host numbers (rounded to fp32 and uploaded ONCE per
    distinct value and device) or a contiguous float32 (M,) tensor on the device, used BY REFERENCE and never read on the host.  k0: a
    host number, finite and >= 0 in fp32.  missing: "skip" -- a list that does not hold the video adds nothing (standard RRF) -- or
    "drop" -- every list must hold it.  allow: a packed mask over the V videos, as in Shortlister.shortlist, applied by the fusing
    launch: the lists are given.  out: the three buffers of a Shortlist, written in place.
    ONE launch (drn_rank_fuse_topn, csrc/retrieve_rrf.hip: one workgroup a sentence sorts the M * C entries in LDS, folds and sorts
    again), after the M + 1 copies of a sequence; no dense buffer, no table read, no host synchronisation, and it can be captured in a
    graph once the shape is warmed, where the lists' contents, the weights tensor and the mask may change in place between replays.
    What this is NOT: the votes depend on the depth the lists were cut at -- see rank_fuse_reference."""
    what = "rank_fuse"
    lists, S, V, weights, k0 = _check_rank_fuse(what, lists, V, weights, k0, missing, allow)
    n = _check_depth(what, n)
    if out is not None:
        _check_list_out(what, out, S, n)
    else:
        out = _list_buffers(weights.device, S, n)
    ops.rank_fuse_topn(_stacked_lists(lists), V, weights, k0, missing, n, *out, allow=allow)
    return Shortlist(*out)


def rank_fuse_rank(lists, V, targets, weights=None, k0=60.0, missing="skip", allow=None, out=None):
    """The place of each sentence's TARGET video in the full order of rank_fuse -> TargetRank, on the device
    (rank_fuse_rank_reference defines it): lists, V, weights, k0, missing and allow as in rank_fuse; targets: contiguous int32 (S,) on
    the lists' device, never read on the host, a value outside [0, V) meaning "no target"; out: three (S,) buffers (rank, score,
    total).  rank[s] = k >= 0 exactly when rank_fuse(lists, V, n).ids[s, k] is the target for every n > k, score[s] has the listed
    score's bits and total[s] counts the fused candidates.  ONE launch (drn_rank_fuse_rank), no host synchronisation, capturable."""
    what = "rank_fuse_rank"
    lists, S, V, weights, k0 = _check_rank_fuse(what, lists, V, weights, k0, missing, allow)
    _check_targets(what, S, targets, weights.device)
    _check_rank_out(what, S, out)
    if out is None:
        out = _rank_buffers(weights.device, S)
    ops.rank_fuse_rank(_stacked_lists(lists), V, weights, k0, missing, targets, *out, allow=allow)
    return TargetRank(*out)


class RankFusedShortlister(object):
    """RankFusedShortlister(tables, weights=None, k0=60.0, depth=SHORTLIST_MAX, missing="skip"): several tables over the same videos
    ranked as one BY RANK -- each table lists its best `depth` videos its own way (its own rows, E, dtype, quantisation, shards, late
    interaction) and the lists are fused by rank_fuse: what FusedShortlister cannot do for tables whose scores share no scale, and
    cheaper -- no dense 4 * M * S * V buffers, M * S * depth ids instead.

    tables: 1 to RANK_FUSE_MAX_LISTS Shortlister / ShardedShortlister objects over the SAME V videos on one device, held by
    reference; names as in FusedShortlister (equal position by position where given, refused here).  weights, k0 and missing as in
    rank_fuse; a device weights tensor is kept by reference.  depth: the length each table's list is cut at, 1 <= depth <=
    SHORTLIST_DEEP_MAX: a Shortlister lists by shortlist() up to SHORTLIST_MAX and by shortlist_deep() beyond it; a ShardedShortlister
    and a late item have no deep entry, so a depth above SHORTLIST_MAX is refused for them -- the table here, the item in the call,
    before any launch.

    What this is NOT: a fusion of scores.  A video outside a table's best `depth` gets no vote from it (under "drop" it is no
    candidate), so the answer depends on depth; rank_fuse_reference over the tables' own shortlist().ids is the definition.
    Attributes: tables, weights (the device tensor), k0, depth, missing, names, device; len() is V."""

    def __init__(self, tables, weights=None, k0=60.0, depth=SHORTLIST_MAX, missing="skip"):
        what = "RankFusedShortlister"
        tables, names = _fused_tables(what, tables, missing, RANK_FUSE_MAX_LISTS)
        k0, depth = _check_k0(what, k0), int(depth)
        if not 1 <= depth <= SHORTLIST_DEEP_MAX:
            raise DrnError("%s: depth = %d outside [1, %d]" % (what, depth, SHORTLIST_DEEP_MAX))
        for m, table in enumerate(tables):
            if depth > SHORTLIST_MAX and isinstance(table, ShardedShortlister):
                raise DrnError("%s: depth = %d above SHORTLIST_MAX = %d needs shortlist_deep, and table %d is a ShardedShortlister, which "
                               "has no deep entry (compact() it into one table first)" % (what, depth, SHORTLIST_MAX, m))
        weights = _fused_weights(what, weights, len(tables), tables[0].device, "tables")
        self.tables, self.weights, self.k0, self.depth, self.missing, self.names = tables, weights, k0, depth, missing, names
        self._bufs = {}

    @property
    def device(self):
        return self.tables[0].device

    def __len__(self):
        return len(self.tables[0])

    def _check_items(self, what, queries, allow):
        """What shortlist() and rank() refuse about the query items and the mask, ALL before the first launch -> (S, items)."""
        S, items = _check_fused_items(what, self.tables, queries)
        for m, (_, lengths) in enumerate(items):
            if lengths is not None and self.depth > SHORTLIST_MAX:
                raise DrnError("%s: depth = %d above SHORTLIST_MAX = %d needs shortlist_deep, and item %d selects late interaction, which "
                               "has no deep entry" % (what, self.depth, SHORTLIST_MAX, m))
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.device)
        return S, items

    def _lists(self, S, items, allow):
        """Each table's own list of `depth` under the mask, its ids into slice [m] of the stacked buffer kept per S -> that buffer."""
        bufs, depth = self._bufs.get(S), self.depth
        if bufs is None:
            bufs = self._bufs[S] = (torch.empty((len(self.tables), S, depth), dtype=torch.int32, device=self.device),) \
                + _list_buffers(self.device, S, depth, rows=True)[1:]
        ids, scores, counts, rows = bufs                          # (scores, counts and rows are scratch: only the ids are fused)
        for m, (table, (q, lengths)) in enumerate(zip(self.tables, items)):
            if lengths is not None:
                table.shortlist_late(q, lengths, depth, out=(ids[m], scores, counts), allow=allow)
                continue
            first = table if isinstance(table, Shortlister) else table.shards[0]
            out = (ids[m], scores, counts) + ((rows,) if first._seg is not None else ())
            (table.shortlist_deep if depth > SHORTLIST_MAX else table.shortlist)(q, depth, out=out, allow=allow)
        return ids

    def shortlist(self, queries, n, out=None, allow=None):
        """Each sentence's best n videos under the fused reciprocal ranks -> Shortlist, on the device: rank_fuse over the tables' own
        shortlist(item, depth, allow=allow).ids, bit for bit.  queries: the M items of FusedShortlister.shortlist, a pair (queries,
        lengths) selecting that table's shortlist_late; every item holds the same S sentences.  1 <= n <= SHORTLIST_DEEP_MAX.  out:
        the three buffers of a Shortlist.  allow: a packed mask over the V videos; it goes to the TABLES' shortlists, so the filter
        comes before the ranking -- a masked video takes no rank in any list -- and the fusing launch runs unmasked.  Each table's
        launches into buffers kept per S, then ONE fusing launch; no host synchronisation, capturable once the shape is warmed,
        where the queries, lengths, the weights tensor and the mask's contents may change in place between replays."""
        what = "RankFusedShortlister.shortlist"
        S, items = self._check_items(what, queries, allow)
        n = _check_depth(what, n)
        if out is not None:
            _check_list_out(what, out, S, n)
        else:
            out = _list_buffers(self.device, S, n)
        ops.rank_fuse_topn(self._lists(S, items, allow), len(self), self.weights, self.k0, self.missing, n, *out)
        return Shortlist(*out)

    def rank(self, queries, targets, out=None, allow=None):
        """The place of each sentence's TARGET video in the full fused order -> TargetRank, on the device (rank_fuse_rank over the
        tables' own lists): queries and allow as in shortlist(), targets and out= as in Shortlister.rank.  rank[s] = k >= 0 exactly
        when shortlist(queries, n).ids[s, k] is the target for every n > k; -1 where no list holds the target (or, under "drop", not
        every list).  evaluate_shortlist(rank_fused, batches) works as it stands, batch[1] being the M items."""
        what = "RankFusedShortlister.rank"
        S, items = self._check_items(what, queries, allow)
        _check_targets(what, S, targets, self.device)
        _check_rank_out(what, S, out)
        if out is None:
            out = _rank_buffers(self.device, S)
        ops.rank_fuse_rank(self._lists(S, items, allow), len(self), self.weights, self.k0, self.missing, targets, *out)
        return TargetRank(*out)
