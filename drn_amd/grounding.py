"""Grounding without a ground truth: "here is a video and some sentences, give me the best moments".

Grounder.ground = mainModel.forward_heads_shared (the query-independent part of the forward -- prop_fc above all -- once per VIDEO,
however many sentences ask about it) -> the device post-processor (drn_postprocess) -> the evaluator's temporal NMS on the device
(drn_select_moments: utils/evaluate_utils.py:91-107,186-212), which hands back the surviving moments themselves, best first.
Nothing crosses to the host until the caller asks (Moments.tolist).

Grounder.search answers "in which video, and where": S sentences against every video of a resident FeatureStore.  The sentences are
encoded ONCE; the store is walked in chunks of equal shape (store.gather with a device index buffer -> forward_heads_shared with the
encoded gates, pair p = (sentence p // Vc, chunk slot p % Vc) -> post-processor -> drn_select_moments), and drn_merge_moments keeps
each sentence's best moments across the chunks on the device (Hits).

Grounder.search(candidates=) looks for each sentence only in that sentence's own list of videos: plan_pairs cuts the ragged list of
(sentence, video) pairs into steps of equal shape, the same fronts and trunk run on a step's pairs, and drn_merge_moments_ragged ranks
them.  With the candidates as a DEVICE tensor (drn_amd.retrieve.Shortlister's ids) nothing is read on the host: the steps come from
the shapes alone (plan_candidate_steps) and one drn_plan_candidates launch fills in their videos.  Grounder.ground_stored is the one-video-per-sentence case without a ranking: ground() on videos that are already resident."""
import collections

import numpy as np
import torch

from . import ops
from ._lib import CANDIDATES_MAX, DrnError


class Moments(object):
    """The best moments of Q queries, on the device: seg (Q, k, 2) [start, end] as fractions of the video, score (Q, k), level (Q, k)
    int32 pyramid level, index (Q, k) int32 position in the query's candidate list, n (Q,) int32 valid entries per query (best
    first; entries past n are 0 / -1).  A query without a candidate has the reference's fallback moment (0, 1), score 1, level -1,
    index -1 (model/inference.py:192-197)."""
    __slots__ = ("seg", "score", "level", "index", "n")

    def __init__(self, seg, score, level, index, n):
        self.seg, self.score, self.level, self.index, self.n = seg, score, level, index, n

    def __len__(self):
        return int(self.n.shape[0])

    def fields(self):
        return self.seg, self.score, self.level, self.index, self.n

    def tolist(self):
        """Per query [[start, end, score], ...], the first n[q] entries: one host copy per field."""
        n, seg, score = self.n.tolist(), self.seg.tolist(), self.score.tolist()
        return [[[seg[q][i][0], seg[q][i][1], score[q][i]] for i in range(n[q])] for q in range(len(n))]


class Hits(object):
    """The best moments of S sentences across the videos of a store, on the device, best first: seg (S, k, 2) [start, end] as fractions
    of the video, score (S, k), video (S, k) int32 position in the store, level (S, k) int32 pyramid level, rank (S, k) int32 position
    of the moment among its (sentence, video) pair's NMS survivors, n (S,) int32 valid entries per sentence (entries past n are
    0 / -1).  Order: score descending, then video position ascending, then rank ascending.  A video in which the model found no
    candidate contributes nothing (the fallback moment of Moments is no hit), so n may be 0."""
    __slots__ = ("seg", "score", "video", "level", "rank", "n")

    def __init__(self, seg, score, video, level, rank, n):
        self.seg, self.score, self.video, self.level, self.rank, self.n = seg, score, video, level, rank, n

    def __len__(self):
        return int(self.n.shape[0])

    def tolist(self, names=None):
        """Per sentence [[video, start, end, score], ...], the first n[s] entries: one host copy per field.  video: the store position,
        or names[position] (names: e.g. store.names)."""
        n, seg, score, video = self.n.tolist(), self.seg.tolist(), self.score.tolist(), self.video.tolist()
        name = (lambda v: v) if names is None else (lambda v: names[v])
        return [[[name(video[s][i]), seg[s][i][0], seg[s][i][1], score[s][i]] for i in range(n[s])] for s in range(len(n))]


def group_by_video(names):
    """Loader batches name one video per query: -> (unique names in order of first appearance, video_index (Q,) int64 host tensor)
    with names[q] == unique[video_index[q]]."""
    slot, unique, index = {}, [], []
    for name in names:
        if name not in slot:
            slot[name] = len(unique)
            unique.append(name)
        index.append(slot[name])
    return unique, torch.tensor(index, dtype=torch.int64)


PairPlan = collections.namedtuple("PairPlan", "vids pair_q pair_v pair_video pair_off")


def _pairs_csr(candidates, num_videos):
    """candidates -> (ids int64, offsets int64 (S + 1,)): sentence s lists ids[offsets[s]:offsets[s + 1]].  Accepted: a sequence of S
    sequences of store positions, or the CSR pair itself as a 2-TUPLE of numpy arrays / host tensors (ids, offsets).  A position
    outside [0, num_videos) raises."""
    is_array = lambda c: isinstance(c, np.ndarray) or torch.is_tensor(c)
    try:
        if isinstance(candidates, tuple) and len(candidates) == 2 and all(is_array(c) for c in candidates):
            ids, off = (np.asarray(c).astype(np.int64).reshape(-1) for c in candidates)
            if off.size < 1 or off[0] != 0 or off[-1] != ids.size or (np.diff(off) < 0).any():
                raise DrnError("plan_pairs: offsets must rise from 0 to the number of ids (%d)" % ids.size)
        else:
            lists = [np.asarray(c if is_array(c) else list(c)).astype(np.int64).reshape(-1) for c in candidates]
            off = np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.int64)
            ids = np.concatenate(lists + [np.zeros(0, np.int64)])
    except (TypeError, ValueError):
        raise DrnError("plan_pairs: candidates must be sequences of store positions (resolve names with ids_of), or (ids, offsets)")
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= int(num_videos)):
        raise DrnError("plan_pairs: video positions outside [0, %d)" % int(num_videos))
    return ids, off


def plan_pairs(candidates, num_videos, pairs, slots, cap):
    """Cut a ragged list of (sentence, video) pairs into chunks of ONE shape -> PairPlan of int32 arrays with a leading chunk axis:
    vids (C, slots) store positions, -1 past the chunk's videos; pair_q (C, pairs) the pair's sentence; pair_v (C, pairs) its slot in
    vids; pair_video (C, pairs) its store position; pair_off (C, S + 1): sentence s owns the pairs [pair_off[s], pair_off[s + 1]) of
    the chunk.  Padded pairs sit after pair_off[S] with pair_video -1, pair_q 0 and pair_v 0 (in range for both fronts: whatever they
    compute there is outside every sentence's range).
    candidates: S sequences of store positions, or the CSR pair (ids, offsets) as a 2-tuple of arrays.  A sentence's list is a SET
    (duplicates are dropped) and may be empty.  The distinct pairs are ordered by (video, sentence) -- a video's pairs lie together, so
    the store path projects each video as few times as possible -- and cut greedily: a new chunk starts when the next pair would make
    it more than `pairs` pairs, more than `slots` distinct videos, or more than `cap` pairs of that pair's sentence.  Within a chunk the
    pairs are then sorted stably by sentence.  No pairs at all: zero chunks.  Pure numpy; deterministic."""
    pairs, slots, cap = int(pairs), int(slots), int(cap)
    if pairs < 1 or slots < 1 or cap < 1:
        raise DrnError("plan_pairs: pairs, slots and cap must be at least 1 (got %d, %d, %d)" % (pairs, slots, cap))
    ids, off = _pairs_csr(candidates, num_videos)
    S = int(off.size) - 1
    if S < 1:
        raise DrnError("plan_pairs: no sentences")
    return _plan(_distinct_pairs(ids, off), S, pairs, slots, cap)


def _distinct_pairs(ids, off):
    """The distinct (sentence, video) pairs of a CSR list as keys video * S + sentence, ascending: ordered by (video, sentence)."""
    S = int(off.size) - 1
    return np.unique(ids * S + np.repeat(np.arange(S, dtype=np.int64), np.diff(off)))


def _plan(key, S, pairs, slots, cap):
    vid, sen = key // S, key % S
    cuts = [0]
    if key.size > pairs or np.unique(vid).size > slots or (key.size and int(np.bincount(sen).max()) > cap):
        n, nv, last, per = 0, 0, -1, {}
        for i, (v, q) in enumerate(zip(vid.tolist(), sen.tolist())):
            if n + 1 > pairs or nv + (v != last) > slots or per.get(q, 0) + 1 > cap:
                cuts.append(i)
                n, nv, last, per = 0, 0, -1, {}
            n, nv, last = n + 1, nv + (v != last), v
            per[q] = per.get(q, 0) + 1
    # (otherwise everything fits one chunk, which is what the greedy walk would find)
    C = len(cuts) if key.size else 0
    cuts.append(int(key.size))
    plan = PairPlan(np.full((C, slots), -1, np.int32), np.zeros((C, pairs), np.int32), np.zeros((C, pairs), np.int32),
                    np.full((C, pairs), -1, np.int32), np.zeros((C, S + 1), np.int32))
    for c in range(C):
        v, q = vid[cuts[c]:cuts[c + 1]], sen[cuts[c]:cuts[c + 1]]
        order = np.argsort(q, kind="stable")
        uniq, slot = np.unique(v, return_inverse=True)
        plan.vids[c, :uniq.size] = uniq
        plan.pair_q[c, :q.size], plan.pair_v[c, :q.size], plan.pair_video[c, :q.size] = q[order], slot.reshape(-1)[order], v[order]
        plan.pair_off[c, 1:] = np.cumsum(np.bincount(q, minlength=S))
    return plan


CandidateSteps = collections.namedtuple("CandidateSteps", "Sc Nc pairs pair_q pair_v pair_off first")
CandidateSteps.__doc__ = """The static half of a search over device candidates (plan_candidate_steps): Sc sentences x Nc columns per step,
`pairs` pair slots per step, and int32 arrays with a leading step axis: pair_q (steps, pairs) the pair's sentence (0 for padding),
pair_v (steps, pairs) = arange(pairs) (one video slot per pair), pair_off (steps, S + 1), first (steps, 1) = 1 for step 0 only."""


def plan_candidate_steps(S, N, pairs=None, cap=None):
    """The steps of a search over a (S, N) table of candidates as a function of the SHAPES alone -- nothing in it depends on the data, so
    the table is never walked on the host -> CandidateSteps.  cap: the pairs of one sentence a ranking step holds,
    (MERGE_MAX_CAND - top_k) // per_video (default: no limit).  pairs: pair slots per step, default min(SEARCH_PAIR_BUDGET, S * N).
    Nc = min(N, cap, pairs) columns and Sc = min(S, pairs // Nc) sentences per step; steps run sentence block outer, column block
    inner: step sb * ceil(N / Nc) + cb, and its pair i = sl * Nc + jl is sentence sb * Sc + sl, column cb * Nc + jl.  pair_off gives
    sentence s of the step's block the pairs [(s - sb * Sc) * Nc, + Nc) and every other sentence an empty range; pairs at or past
    pair_off[S] are padding (pair_q 0).  Which of a step's pairs name a video is the data's half: plan_candidates_reference /
    ops.plan_candidates write -1 for the others, and the ranking skips those.  Pure numpy."""
    S, N = int(S), int(N)
    if S < 1 or N < 1:
        raise DrnError("plan_candidate_steps: S and N must be at least 1 (got %d, %d)" % (S, N))
    pairs = min(Grounder.SEARCH_PAIR_BUDGET, S * N) if pairs is None else int(pairs)
    cap = N if cap is None else int(cap)
    if pairs < 1 or cap < 1:
        raise DrnError("plan_candidate_steps: pairs and cap must be at least 1 (got %d, %d)" % (pairs, cap))
    Nc = min(N, cap, pairs)
    Sc = min(S, pairs // Nc)
    nsb, ncb = -(-S // Sc), -(-N // Nc)
    steps = nsb * ncb
    i = np.arange(pairs)
    sb = np.repeat(np.arange(nsb), ncb)
    sent = sb[:, None] * Sc + (i // Nc)[None, :]
    pair_q = np.where((i[None, :] < Sc * Nc) & (sent < S), sent, 0).astype(np.int32)
    held = np.clip(np.arange(S + 1)[None, :] - sb[:, None] * Sc, 0, np.minimum(Sc, S - sb * Sc)[:, None])
    first = (np.arange(steps) == 0).astype(np.int32).reshape(steps, 1)
    return CandidateSteps(Sc, Nc, pairs, pair_q, np.tile(i.astype(np.int32), (steps, 1)), (held * Nc).astype(np.int32), first)


def plan_candidates_reference(C, num_videos, S, N, pairs=None, cap=None):
    """THE DEFINITION of ops.plan_candidates' table, in numpy: C (S, N) integers -> pair_video (steps, pairs) int32 for the steps of
    plan_candidate_steps(S, N, pairs, cap).  The pair of (sentence s, column j) gets C[s, j] when that is a position in
    [0, num_videos) and no earlier column of row s holds the same position -- the WHOLE row, not only the step's columns -- and -1
    otherwise; pairs of sentences or columns past S or N and pairs past Sc * Nc get -1."""
    C = np.asarray(C).astype(np.int64).reshape(int(S), int(N))
    plan = plan_candidate_steps(S, N, pairs, cap)
    Sc, Nc = plan.Sc, plan.Nc
    ncb = -(-int(N) // Nc)
    table = np.full(plan.pair_q.shape, -1, dtype=np.int32)
    for s in range(int(S)):
        seen = set()
        for j in range(int(N)):
            v = int(C[s, j])
            if 0 <= v < int(num_videos) and v not in seen:
                seen.add(v)
                table[(s // Sc) * ncb + j // Nc, (s % Sc) * Nc + j % Nc] = v
    return table


def check_device_candidates(C, S, store, chunk=None):
    """The refusals of search(candidates= a device tensor) that depend on the tensor, the store and S, before any launch and without
    reading the tensor: a SearchIndex, int32, (S, N) with 1 <= N <= CANDIDATES_MAX -- 1024, a CHOICE, not a measurement:
    ops.plan_candidates holds one row in 4 KiB of LDS to drop its repeats."""
    from .index import SearchIndex
    if not isinstance(store, SearchIndex):
        raise DrnError("Grounder.search: device candidates need a SearchIndex: on a FeatureStore every (sentence, video) pair would "
                       "pool and project its own video -- build an index (SearchIndex.build) or pass host lists")
    if chunk is not None:
        raise DrnError("Grounder.search: chunk= does not apply to device candidates (every pair has a video slot of its own)")
    if S < 1:
        raise DrnError("Grounder.search: no sentences")
    if C.dtype != torch.int32:
        raise DrnError("Grounder.search: device candidates must be int32, not %s" % C.dtype)
    if C.dim() != 2 or int(C.shape[0]) != S or not 1 <= int(C.shape[1]) <= CANDIDATES_MAX:
        raise DrnError("Grounder.search: device candidates must be (%d, N) with 1 <= N <= %d, not %s" % (S, CANDIDATES_MAX, tuple(C.shape)))


class _GroundGraph(object):
    """One captured grounding path: the static inputs, the hipGraph, the static Moments fields and the stamp it was captured under."""
    __slots__ = ("inputs", "graph", "out", "stamp", "stream")


class Grounder(object):
    """Grounder(model, top_k=5, nms_overlap=0.45, fused=False, graph=False, max_graphs=4).ground(query_tokens, query_length,
    props_features, props_start_end, video_index=None) -> Moments.  nms_overlap: the NMS threshold itself; 0.45 is the evaluator's
    0.5 - 0.05 for Recall@IoU 0.5.  The model must be in eval mode; ground() runs under torch.no_grad() and changes no model state.

    fused: the eval conv -> BatchNorm -> ReLU blocks run as one launch each (functional.fused_eval).
    graph: the path from the inputs to drn_select_moments' outputs is captured once per input signature (shapes and dtypes of the five
    inputs, video_index present or not) as ONE linear hipGraph on one stream and replayed afterwards: a call copies its inputs into the
    static buffers (static_inputs(signature) hands them out; an input that already IS the buffer is not copied), replays, and returns
    Moments whose fields are copies of the static outputs.  A host video_index is range-checked on the host first.  At most max_graphs
    signatures are kept, none is evicted, a further one runs eagerly.  The graph holds raw pointers to the re-laid weight copies
    (functional.packed), which are re-made when a parameter's version moves: every graph carries the address and _version of each
    parameter and the WeightCopies epoch, and a call under another stamp captures again.  Running
    statistics changed IN PLACE keep their address and are re-read by the scale/shift launches of every replay.  `captures` counts the captures made.
    search() shares all of this: its per-chunk body is one more signature among the max_graphs, and that of search(candidates=)
    another.  ground_stored() runs eagerly whatever `graph` says.
    conv0="mxfp8": search (cartesian, videos=, candidates=), ground_stored and evaluate_search run conv0 on block-scaled FP8 MFMAs
    straight from a SearchIndex built with quantize="mxfp8" (mainModel.forward_heads_packed(conv0="mxfp8")): no gather launch and no
    (pairs, T, Dp + P) buffer; the sentence gate is folded into conv0's weights, which are quantised to the index's format ONCE per
    search (one launch, outside a captured graph, into the buffer the graph reads).  Lossy: the scores differ from the default path's.
    A store, a plain index or an fp32 model raise before any launch.  ground() is not affected.
    conv0="mxfp8" together with fused=True: conv0, its eval BatchNorm, the ReLU and the level-1 gate are ONE launch on LDS-staged FP8
    tiles (ops.conv0_mx8_bn) that never writes conv0's raw output; without fused it is ops.conv0_mx8 followed by the unfused
    BatchNorm launches.  The two differ in the last bits of their scores (raw is rounded to bf16 only in the unfused mode)."""

    # Pairs (sentence, video) per chunk that search() allows itself by default.  A CHOICE, not a measurement: conv0's input g0 holds
    # T * (D + 256) elements per pair -- 2.1 MiB at T = 256, D = 4096 in bf16 -- so 512 pairs are 1.1 GiB of g0, and the trunk's
    # activations a small multiple of that: a few GiB of a 288 GiB device, beside a store that is meant to fill most of it.
    SEARCH_PAIR_BUDGET = 512

    def __init__(self, model, top_k=5, nms_overlap=0.45, fused=False, graph=False, max_graphs=4, conv0=None):
        if int(top_k) < 1:
            raise DrnError("Grounder: top_k must be at least 1")
        if conv0 not in (None, "mxfp8"):
            raise DrnError("Grounder: conv0 must be None or \"mxfp8\" (got %r)" % (conv0,))
        self.conv0 = conv0
        self.model, self.top_k, self.nms_overlap = model, int(top_k), float(nms_overlap)
        self.fused, self.graph, self.max_graphs = bool(fused), bool(graph), int(max_graphs)
        self._graphs = {}
        self.captures = 0

    @staticmethod
    def signature(query_tokens, query_length, props_features, props_start_end, video_index=None):
        return tuple((tuple(t.shape), t.dtype) for t in (query_tokens, query_length, props_features, props_start_end)) + \
            ((tuple(video_index.shape), torch.int32) if video_index is not None else None,)

    def static_inputs(self, signature):
        """The static input buffers of a captured signature (query_tokens, query_length, props_features, props_start_end, video_index or
        None): fill them in place and pass them to ground() to skip the copies.  None before the signature's first ground() call."""
        ent = self._graphs.get(signature)
        return tuple(ent.inputs) if ent is not None else None

    def _stamp(self):
        """What the captured pointers depend on: functional.packed re-makes a copy when its parameter's (_version, store epoch) moves.
        Buffers are not part of it: the running statistics are read in place by the scale/shift launches of every replay, so an
        in-place change of them needs no new capture (replacing a buffer by another tensor does: call reset_graphs())."""
        from . import functional as DF
        params = list(self.model.parameters())
        return (tuple((id(p), p.data_ptr(), p._version) for p in params), DF.store_of(params).epoch if params else 0)

    def reset_graphs(self):
        """Drop every captured graph; the next ground() call of a signature captures again."""
        self._graphs.clear()

    @torch.no_grad()
    def ground(self, query_tokens, query_length, props_features, props_start_end, video_index=None):
        if not self.graph:
            return self._ground(query_tokens, query_length, props_features, props_start_end, video_index)
        args = [query_tokens, query_length, props_features, props_start_end, video_index]
        if self.model.training or any(t is not None and i != 4 and not t.is_cuda for i, t in enumerate(args)):
            return self._ground(*args)                          # (refused there, as without the graph)
        sig = self.signature(*args)
        if sig not in self._graphs and len(self._graphs) >= self.max_graphs:
            return self._ground(*args)
        if video_index is not None:
            if video_index.dim() != 1 or video_index.is_floating_point():
                return self._ground(*args)                      # (refused there)
            if not video_index.is_cuda and video_index.numel():
                V = int(props_features.shape[0])
                if int(video_index.min()) < 0 or int(video_index.max()) >= V:
                    raise DrnError("Grounder: video_index outside [0, %d)" % V)
        dev = props_features.device
        ent, fresh = self._entry(sig, lambda *a: self._ground(*a).fields(), dev, lambda: [
            None if t is None else (t.to(device=dev, dtype=torch.int32) if i == 4 else t).clone().contiguous() for i, t in enumerate(args)])
        if not fresh:
            for dst, src in zip(ent.inputs, args):
                if dst is not None and src is not dst and src.data_ptr() != dst.data_ptr():
                    dst.copy_(src, non_blocking=src.is_cuda)
            ent.graph.replay()
        return Moments(*[t.clone() for t in ent.out])

    def _entry(self, sig, run, dev, make_inputs):
        """The captured graph of `sig` under today's stamp -> (entry, captured just now): one whose stamp has moved is dropped and
        captured again.  (None, False) when the signature is new and max_graphs are held: the caller runs eagerly."""
        ent = self._graphs.get(sig)
        if ent is None and len(self._graphs) >= self.max_graphs:
            return None, False
        if ent is not None and ent.stamp != self._stamp():
            del self._graphs[sig]
            ent = None
        if ent is not None:
            return ent, False
        ent = self._capture(run, make_inputs(), dev)
        ent.stamp = self._stamp()
        self._graphs[sig] = ent
        return ent, True

    def _capture(self, run, inputs, dev):
        """run(*inputs) -> tuple of tensors, on the static buffers `inputs`: one warm run on the capture stream (lazy module loads,
        weight copies, workspaces), then the capture: everything on ONE stream, so the graph is one linear chain; one replay, so that
        the static outputs hold this call's result."""
        from .graph import capture_graph
        ent = _GroundGraph()
        ent.inputs = inputs
        ent.stream = torch.cuda.Stream(device=dev)
        ent.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(ent.stream):
            run(*ent.inputs)
        torch.cuda.current_stream().wait_stream(ent.stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture_graph(g, ent.stream):
            ent.out = tuple(run(*ent.inputs))
        ent.graph = g
        self.captures += 1
        g.replay()
        return ent

    def _ground(self, query_tokens, query_length, props_features, props_start_end, video_index=None):
        return Moments(*self._select(self.top_k, query_tokens, query_length, props_features, props_start_end, video_index))

    def _select(self, k, *forward_args, **forward_kw):
        """forward_heads_shared(...) -> device post-processor -> ops.select_moments(k): the five Moments fields.  entry=: the name of
        another model method of the same return value (forward_heads_packed)."""
        from . import functional as DF
        model = self.model
        forward = getattr(model, forward_kw.pop("entry", "forward_heads_shared"))
        selector = model.fcos.box_selector_test
        if model.fcos.head.cls_logits.weight.shape[0] != 1:
            raise DrnError("Grounder: the device post-processor serves one foreground channel (fcos_num_class = 2); this model has %d"
                           % model.fcos.head.cls_logits.weight.shape[0])
        was = selector.device_only
        selector.device_only = True
        try:
            with DF.fused_eval(self.fused):
                locations, box_cls, box_reg, iou_scores = forward(*forward_args, **forward_kw)
            dd = selector(locations, box_cls, box_reg, iou_scores)
        finally:
            selector.device_only = was
        if isinstance(dd, list):
            raise DrnError("Grounder: the post-processor has no flat device path for this model (min_size != 0?)")
        return ops.select_moments(dd.det, dd.scores, dd.counts, self.nms_overlap, k)

    # -- search across the videos of a store -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def search(self, query_tokens, query_length, store, top_k=None, per_video=1, videos=None, chunk=None, T=None, candidates=None,
               pairs=None):
        """The best top_k (default: the Grounder's) moments of each of the S sentences across the videos of `store` (a FeatureStore on
        the GPU in the model's compute dtype) -> Hits.  per_video: at most that many moments of one video compete (the first per_video
        survivors of the pair's temporal NMS at nms_overlap).  videos: names or store positions to search, default the whole store.
        T: the padded proposal count, default the largest count among the searched videos (padded proposal positions are treated as
        ground() treats them).  chunk: videos per step.  Its default is the largest value that keeps a step within
        SEARCH_PAIR_BUDGET (sentence, video) pairs and top_k + chunk * per_video within drn_merge_moments' LDS cap -- the pair budget
        is a choice made from the memory of conv0's input at D = 4096, not a measurement.
        The sentences are encoded once.  Every chunk has the same shape (the last one is padded with position -1, whose pairs the
        ranking skips) and runs store.gather -> forward_heads_shared(gates=, query_index=, video_index=) -> post-processor ->
        select_moments -> merge_moments; the chunks' positions are uploaded in one copy before the first.  There is no host
        synchronisation, here or in the loop: only Hits.tolist waits.  A video without a candidate contributes nothing.
        graph=True: that per-chunk body is captured once per (store, S, chunk, T, per_video, top_k) as one linear hipGraph and replayed
        per chunk -- the chunk's positions and the first-chunk word are copied into its static buffers outside the graph -- under
        ground()'s stamp, max_graphs and `captures` rules; Hits' fields are copies of the static state.
        store may be a drn_amd.SearchIndex built from the store for this model: every keyword means what it means above and the Hits
        are the same bit for bit, but a chunk's front is ONE launch (drn_gate_gather_packed reads the projected rows) instead of
        store.gather, the cast, the prop_fc GEMM, the position embedding and the gate pass.  A stale index (index.is_current(model) is
        False) raises before any launch.
        candidates: instead of videos=, EACH sentence's own videos -- S lists of names or store positions, or the CSR pair
        (ids, offsets) as a 2-tuple of arrays; a list is a set and may be empty (that sentence gets n = 0).  Only the listed
        (sentence, video) pairs run the trunk.  plan_pairs cuts them into steps of one shape: at most `pairs` pairs (default
        SEARCH_PAIR_BUDGET, the same choice as above, or the number of distinct pairs when that is smaller), at most `chunk` video slots (default min(pairs, the distinct candidate videos))
        and at most (MERGE_MAX_CAND - top_k) // per_video pairs of one sentence; padded pairs are skipped by the ranking.  T defaults to
        the largest count among all candidate videos.  All steps' arrays and first-chunk words go up in one copy; a step runs the same
        front on its pairs (pair_q, pair_v instead of p // Vc, p % Vc), select_moments and drn_merge_moments_ragged.  The Hits of
        candidates=[all videos] * S are those of the search without candidates.  graph=True: one more signature,
        ("pairs", store, S, pairs, chunk, T, per_video, top_k): other lists that cut to the same shape replay the same graph.
        candidates as a DEVICE tensor: a CUDA int32 tensor (S, N), 1 <= N <= CANDIDATES_MAX (1024, a choice), e.g.
        drn_amd.Shortlister.shortlist(...).ids -- row s is sentence s's set of store positions, an entry < 0 or >= len(store) is no
        candidate, a position repeated in a row counts once (the first occurrence).  The tensor is NEVER read on the host: the steps
        are plan_candidate_steps(S, N, pairs, cap) -- shapes alone, one pinned upload -- one ops.plan_candidates launch per search
        writes their pair_video rows, and each step runs the body above with one video slot per pair (chunk= does not apply).  Needs
        a SearchIndex (plain or quantised; a FeatureStore raises before any launch: every pair would pool and project its own
        video).  T defaults to index.T, because nothing can be read back to find a smaller one: pass T= when the shortlisted videos
        are known to be short.  The Hits are those of the same rows passed as host lists at the same T.  graph=True: one more
        signature, ("cands", store, S, N, pairs, T, per_video, top_k, conv0); the plan launch sits outside the captured body and the
        step's row is copied into its static buffer on the device."""
        from ._lib import MERGE_MAX_CAND
        from .index import SearchIndex
        if candidates is not None and videos is not None:
            raise DrnError("Grounder.search: candidates= and videos= exclude each other")
        if pairs is not None and candidates is None:
            raise DrnError("Grounder.search: pairs= is the step size of a search with candidates=")
        model = self.model
        indexed = isinstance(store, SearchIndex)
        K = self.top_k if top_k is None else int(top_k)
        kv = int(per_video)
        resident = self._check_resident("Grounder.search", query_tokens, query_length, store)
        if kv < 1 or K < 1:
            raise DrnError("Grounder.search: per_video and top_k must be at least 1 (got %d, %d)" % (kv, K))
        if indexed:
            store.check(model, "Grounder.search")
        model.check_conv0(self.conv0, store, "Grounder.search")
        if torch.is_tensor(candidates) and candidates.is_cuda:
            return self._search_device_candidates(query_tokens, query_length, store, K, kv, candidates, chunk, pairs, T, resident.device)
        if candidates is not None:
            return self._search_pairs(query_tokens, query_length, store, K, kv, candidates, chunk, pairs, T, resident.device)
        ids = np.arange(len(store), dtype=np.int32) if videos is None else store.ids_of(videos).numpy()
        if ids.size == 0:
            raise DrnError("Grounder.search: no videos to search")
        if int(ids.min()) < 0 or int(ids.max()) >= len(store):
            raise DrnError("Grounder.search: video positions outside [0, %d)" % len(store))
        S = int(query_tokens.shape[0])
        if S < 1:
            raise DrnError("Grounder.search: no sentences")
        cap = (MERGE_MAX_CAND - K) // kv
        if cap < 1:
            raise DrnError("Grounder.search: top_k + per_video = %d exceeds the %d candidates one ranking step holds" % (K + kv, MERGE_MAX_CAND))
        if chunk is None:
            chunk = min(cap, max(1, self.SEARCH_PAIR_BUDGET // S), int(ids.size))
        Vc = int(chunk)
        if Vc < 1 or Vc > cap:
            raise DrnError("Grounder.search: chunk must be in [1, %d] for top_k = %d, per_video = %d" % (cap, K, kv))
        T = int(store.nprops[ids].max()) if T is None else int(T)
        dev = resident.device
        nchunks = -(-int(ids.size) // Vc)
        # ONE upload for the whole walk: the chunks' store positions, padded with -1, then the first-chunk words 1, 0, 0, ...
        plan = np.full(nchunks * Vc + nchunks, -1, dtype=np.int32)
        plan[:ids.size] = ids
        plan[nchunks * Vc:] = 0
        plan[nchunks * Vc] = 1
        plan = torch.from_numpy(plan).pin_memory().to(dev, non_blocking=True)
        vids, first = plan[:nchunks * Vc].view(nchunks, Vc), plan[nchunks * Vc:].view(nchunks, 1)
        gates = [g.contiguous() for g in model.encode_query(query_tokens, query_length)]
        pair = torch.arange(S * Vc, dtype=torch.int32, device=dev)
        pair_q, pair_v = torch.div(pair, Vc, rounding_mode="floor"), torch.remainder(pair, Vc)

        ng, mx = len(gates), self.conv0 is not None

        def body(vid, flag, pq, pv, seg, score, video, level, rank, n, *g):
            if mx:                                               # g: the gates, then conv0's gated weights (made outside this body)
                mom = self._select(kv, store, vid, pq, pv, list(g[:ng]), T, entry="forward_heads_packed", conv0=self.conv0,
                                   conv0_weights=tuple(g[ng:]))
            elif indexed:
                mom = self._select(kv, store, vid, pq, pv, list(g), T, entry="forward_heads_packed")
            else:
                feats, pse, _ = store.gather(vid, T=T)
                mom = self._select(kv, None, None, feats, pse, video_index=pv, query_index=pq, gates=list(g))
            return ops.merge_moments(mom, vid, len(store), (seg, score, video, level, rank, n), flag)

        ent = None
        if self.graph:
            sig = ("search", store, S, Vc, T, kv, K, self.conv0)  # (the key keeps the store, whose addresses the graph holds, alive)
            ent, fresh = self._entry(sig, body, dev, lambda: [vids[0].clone(), first[0].clone(), pair_q, pair_v]
                                     + list(ops.merge_state(S, K, dev)) + [g.clone() for g in gates] + self._conv0_weights(store, gates))
        if ent is None:
            state = ops.merge_state(S, K, dev)
            wq = tuple(self._conv0_weights(store, gates))
            for c in range(nchunks):
                body(vids[c], first[c], pair_q, pair_v, *(state + tuple(gates) + wq))
            return Hits(*state)
        for dst, src in zip(ent.inputs[10:], gates):
            dst.copy_(src)
        if mx and not fresh:                                     # (a fresh capture made them from these very gates)
            self._conv0_weights(store, gates, out=ent.inputs[10 + ng:])
        for c in range(nchunks):
            ent.inputs[0].copy_(vids[c])
            ent.inputs[1].copy_(first[c])
            ent.graph.replay()
        return Hits(*[t.clone() for t in ent.out])

    def _check_resident(self, what, query_tokens, query_length, store):
        """The refusals search() and ground_stored() share, before anything is read from the device -> the resident tensor."""
        from .index import SearchIndex
        resident = store.resident if isinstance(store, SearchIndex) else store.feats
        if self.model.training:
            raise DrnError("%s is inference only: call model.eval() first" % what)
        for t in (query_tokens, query_length):
            if not t.is_cuda:
                raise DrnError("%s runs on an MI355X only (inputs on %s); no CPU fallback" % (what, t.device))
        if not resident.is_cuda:
            raise DrnError("%s needs a store on the GPU (this one lives on %s); there is no CPU fallback" % (what, store.device))
        if store.dtype != self.model.compute_dtype:
            raise DrnError("%s: the store holds %s, the model computes in %s" % (what, store.dtype, self.model.compute_dtype))
        return resident

    @staticmethod
    def _upload_plan(plan, extra, dev):
        """ONE pinned upload of a PairPlan: row c = vids | pair_q | pair_v | pair_video | pair_off | extra[c] of chunk c -> the (C, width)
        int32 device tensor and split(row) -> the six contiguous views of one row, so that a captured graph's static copy of a chunk is
        filled with one copy."""
        host = np.concatenate(list(plan) + [extra], axis=1).astype(np.int32)
        ends = np.cumsum([a.shape[1] for a in plan] + [extra.shape[1]]).tolist()
        split = lambda row: tuple(row[a:b] for a, b in zip([0] + ends[:-1], ends))
        return torch.from_numpy(np.ascontiguousarray(host)).pin_memory().to(dev, non_blocking=True), split

    def _conv0_weights(self, store, gates, out=None):
        """conv0's gated, quantised weights for this search's sentences as a list (empty without conv0="mxfp8"): ONE launch per search,
        whatever the number of chunks.  out: a captured graph's static copies, written in place."""
        if self.conv0 is None:
            return []
        return list(self.model.conv0_mx8_weights(store, gates[0], out=None if out is None else tuple(out)))

    def _pair_front(self, k, store, T, vid, pq, pv, gates, wq=()):
        """One step's pairs through the front and the trunk -> select_moments(k)'s five fields, one row per pair."""
        from .index import SearchIndex
        if self.conv0 is not None:
            return self._select(k, store, vid, pq, pv, list(gates), T, entry="forward_heads_packed", conv0=self.conv0,
                                conv0_weights=tuple(wq))
        if isinstance(store, SearchIndex):
            return self._select(k, store, vid, pq, pv, list(gates), T, entry="forward_heads_packed")
        feats, pse, _ = store.gather(vid, T=T)
        return self._select(k, None, None, feats, pse, video_index=pv, query_index=pq, gates=list(gates))

    def _search_pairs(self, query_tokens, query_length, store, K, kv, candidates, chunk, pairs, T, dev):
        """search(candidates=) after the refusals both forms share."""
        from ._lib import MERGE_MAX_CAND
        S = int(query_tokens.shape[0])
        if S < 1:
            raise DrnError("Grounder.search: no sentences")
        if not (isinstance(candidates, tuple) and len(candidates) == 2 and all(isinstance(c, np.ndarray) or torch.is_tensor(c) for c in candidates)):
            candidates = [store.ids_of(c).numpy() for c in candidates]            # (names -> positions, list by list)
        ids, off = _pairs_csr(candidates, len(store))
        if off.size - 1 != S:
            raise DrnError("Grounder.search: %d candidate lists for %d sentences" % (off.size - 1, S))
        cap = (MERGE_MAX_CAND - K) // kv
        if cap < 1:
            raise DrnError("Grounder.search: top_k + per_video = %d exceeds the %d candidates one ranking step holds" % (K + kv, MERGE_MAX_CAND))
        distinct, key = np.unique(ids), _distinct_pairs(ids, off)
        # (a short list of pairs is not padded up to the budget)
        pairs = min(self.SEARCH_PAIR_BUDGET, max(1, int(key.size))) if pairs is None else int(pairs)
        slots = min(pairs, max(int(distinct.size), 1)) if chunk is None else int(chunk)
        if pairs < 1 or slots < 1:
            raise DrnError("Grounder.search: pairs and chunk must be at least 1 (got %d, %d)" % (pairs, slots))
        plan = _plan(key, S, pairs, slots, cap)
        C = int(plan.vids.shape[0])
        if C == 0:                                                # nobody listed anything: every sentence's hits are empty
            fill = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)
            return Hits(fill((S, K, 2), torch.float32, 0), fill((S, K), torch.float32, 0), fill((S, K), torch.int32, -1),
                        fill((S, K), torch.int32, -1), fill((S, K), torch.int32, -1), fill((S,), torch.int32, 0))
        T = int(store.nprops[distinct].max()) if T is None else int(T)
        rows, split = self._upload_plan(plan, (np.arange(C) == 0).astype(np.int32).reshape(C, 1), dev)
        gates = [g.contiguous() for g in self.model.encode_query(query_tokens, query_length)]

        ng, mx = len(gates), self.conv0 is not None

        def body(row, seg, score, video, level, rank, n, *g):
            vid, pq, pv, pvideo, poff, flag = split(row)
            mom = self._pair_front(kv, store, T, vid, pq, pv, g[:ng], g[ng:])
            return ops.merge_moments_ragged(mom, pvideo, poff, len(store), (seg, score, video, level, rank, n), flag)

        ent = None
        if self.graph:
            sig = ("pairs", store, S, pairs, slots, T, kv, K, self.conv0)
            ent, fresh = self._entry(sig, body, dev, lambda: [rows[0].clone()] + list(ops.merge_state(S, K, dev)) + [g.clone() for g in gates]
                                     + self._conv0_weights(store, gates))
        if ent is None:
            state = ops.merge_state(S, K, dev)
            wq = tuple(self._conv0_weights(store, gates))
            for c in range(C):
                body(rows[c], *(state + tuple(gates) + wq))
            return Hits(*state)
        for dst, src in zip(ent.inputs[7:], gates):
            dst.copy_(src)
        if mx and not fresh:
            self._conv0_weights(store, gates, out=ent.inputs[7 + ng:])
        for c in range(C):
            ent.inputs[0].copy_(rows[c])
            ent.graph.replay()
        return Hits(*[t.clone() for t in ent.out])

    def _search_device_candidates(self, query_tokens, query_length, store, K, kv, C, chunk, pairs, T, dev):
        """search(candidates= a device tensor) after the refusals every form shares.  C is never read on the host: the steps are
        plan_candidate_steps' (shapes alone, ONE pinned upload), ONE ops.plan_candidates launch writes every step's pair_video row from
        C, and each step is _search_pairs' body with vids = that row and one slot per pair."""
        from ._lib import MERGE_MAX_CAND
        S = int(query_tokens.shape[0])
        check_device_candidates(C, S, store, chunk)
        N = int(C.shape[1])
        cap = (MERGE_MAX_CAND - K) // kv
        if cap < 1:
            raise DrnError("Grounder.search: top_k + per_video = %d exceeds the %d candidates one ranking step holds" % (K + kv, MERGE_MAX_CAND))
        if pairs is not None and int(pairs) < 1:
            raise DrnError("Grounder.search: pairs must be at least 1 (got %d)" % int(pairs))
        plan = plan_candidate_steps(S, N, pairs, cap)
        pairs, steps = plan.pairs, int(plan.pair_q.shape[0])
        T = int(store.T) if T is None else int(T)
        rows, split = self._upload_plan((plan.pair_q, plan.pair_v, plan.pair_off), plan.first, dev)
        table = ops.plan_candidates(C.contiguous(), len(store), plan.Sc, plan.Nc, pairs, steps,
                                    torch.empty((steps, pairs), dtype=torch.int32, device=dev))
        gates = [g.contiguous() for g in self.model.encode_query(query_tokens, query_length)]
        ng, mx = len(gates), self.conv0 is not None

        def body(row, pvideo, seg, score, video, level, rank, n, *g):
            pq, pv, poff, flag = split(row)
            mom = self._pair_front(kv, store, T, pvideo, pq, pv, g[:ng], g[ng:])
            return ops.merge_moments_ragged(mom, pvideo, poff, len(store), (seg, score, video, level, rank, n), flag)

        ent = None
        if self.graph:
            sig = ("cands", store, S, N, pairs, T, kv, K, self.conv0)
            ent, fresh = self._entry(sig, body, dev, lambda: [rows[0].clone(), table[0].clone()] + list(ops.merge_state(S, K, dev))
                                     + [g.clone() for g in gates] + self._conv0_weights(store, gates))
        if ent is None:
            state = ops.merge_state(S, K, dev)
            wq = tuple(self._conv0_weights(store, gates))
            for c in range(steps):
                body(rows[c], table[c], *(state + tuple(gates) + wq))
            return Hits(*state)
        for dst, src in zip(ent.inputs[8:], gates):
            dst.copy_(src)
        if mx and not fresh:
            self._conv0_weights(store, gates, out=ent.inputs[8 + ng:])
        for c in range(steps):
            ent.inputs[0].copy_(rows[c])
            ent.inputs[1].copy_(table[c])
            ent.graph.replay()
        return Hits(*[t.clone() for t in ent.out])

    @torch.no_grad()
    def ground_stored(self, query_tokens, query_length, store, videos, pairs=None, T=None):
        """ground() on videos that are already on the device: sentence q is grounded in videos[q] (Q names or store positions; a video
        may be named by many sentences) of a FeatureStore or a SearchIndex -> Moments, bit for bit those of
        ground(query_tokens, query_length, *store.gather(unique, T)[:2], video_index) with unique, video_index = group_by_video(videos).
        T: the padded proposal count, default the largest count among the named videos.  The sentences are encoded once; the Q pairs
        run in steps of `pairs` (default min(SEARCH_PAIR_BUDGET, Q)) cut by plan_pairs, a step's select_moments(top_k) rows are scattered
        into their sentences' rows of the result, padded pairs' rows are dropped.  No ranking across videos, so a pair without a
        candidate keeps Moments' fallback moment.  No host synchronisation.  Eager only: graph=True does not apply here."""
        from .index import SearchIndex
        resident = self._check_resident("Grounder.ground_stored", query_tokens, query_length, store)
        if isinstance(store, SearchIndex):
            store.check(self.model, "Grounder.ground_stored")
        self.model.check_conv0(self.conv0, store, "Grounder.ground_stored")
        Q = int(query_tokens.shape[0])
        ids = store.ids_of(videos).numpy().astype(np.int64)
        if Q < 1 or ids.size != Q:
            raise DrnError("Grounder.ground_stored: %d videos for %d sentences (one each, at least one)" % (ids.size, Q))
        if int(ids.min()) < 0 or int(ids.max()) >= len(store):
            raise DrnError("Grounder.ground_stored: video positions outside [0, %d)" % len(store))
        pairs = min(self.SEARCH_PAIR_BUDGET, Q) if pairs is None else int(pairs)
        if pairs < 1:
            raise DrnError("Grounder.ground_stored: pairs must be at least 1 (got %d)" % pairs)
        distinct = np.unique(ids)
        plan = plan_pairs((ids, np.arange(Q + 1)), len(store), pairs, min(pairs, int(distinct.size)), pairs)
        T = int(store.nprops[distinct].max()) if T is None else int(T)
        dev, k, C = resident.device, self.top_k, int(plan.vids.shape[0])
        # where a pair's rows go: its sentence's row, or -- a padded pair -- a scratch row of its own past the Q real ones
        real = plan.pair_video >= 0
        dest = np.where(real, plan.pair_q, Q + np.arange(pairs, dtype=np.int32)[None, :])
        rows, split = self._upload_plan(plan, dest, dev)
        gates = [g.contiguous() for g in self.model.encode_query(query_tokens, query_length)]
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        out = (torch.empty((Q + pairs, k, 2), dtype=torch.float32, device=dev), torch.empty((Q + pairs, k), dtype=torch.float32, device=dev),
               i32(Q + pairs, k), i32(Q + pairs, k), i32(Q + pairs))
        wq = self._conv0_weights(store, gates)
        for c in range(C):
            vid, pq, pv, _, _, where = split(rows[c])
            where = where.long()
            for dst, src in zip(out, self._pair_front(k, store, T, vid, pq, pv, gates, wq)):
                dst.index_copy_(0, where, src)
        return Moments(*[t[:Q] for t in out])


def search(model, query_tokens, query_length, store, top_k=5, nms_overlap=0.45, fused=False, conv0=None, **kw):
    """Grounder(model, top_k, nms_overlap, fused, conv0=conv0).search(query_tokens, query_length, store, **kw) for a one-off question;
    keep a Grounder to search by graph replay."""
    return Grounder(model, top_k=top_k, nms_overlap=nms_overlap, fused=fused, conv0=conv0).search(query_tokens, query_length, store, **kw)
