"""Recall@k / temporal-IoU metric of the DRN evaluator (reference: utils/evaluate_utils.py:13-16,91-215,328-354 as driven
by main.py:324-364) -- SURVEY row 8f-2.  Host-side: a few dozen (start, end, score) triples per query.

Input format (main.py:336-348): {video: [{"query": str, "gt": [s, e], "node_predictions": [[s, e, score], ...],
"level": [[l]*n_l, ...]}, ...]}.  Reproduced reference behaviour, quirks included:
  * predictions are sorted by score, descending, STABLE (ties keep their input order);
  * the NMS threshold is iou_thresh - 0.05 and NMS visits candidates from the highest score down, resolving score ties
    in favour of the LATER index (ascending stable sort walked from its end);
  * `calculate_IoU` is not clamped: disjoint segments give a negative value (never >= a positive threshold);
  * "level" is carried along UNSORTED, so the per-pick level recorded for visualisation indexes the original order.
The graph-merging branch (`do_merge=True`) is dead in the reference (it calls a method with a keyword it does not accept,
evaluate_utils.py:336, and reads a hard-coded pickle, :69) and is not provided."""
import json
from copy import deepcopy

import numpy as np


class PostProcessRunner(object):
    def __init__(self, raw_results):
        self.raw_results = raw_results if isinstance(raw_results, dict) else json.load(open(raw_results, "r"))
        self.processed_results = None
        self.viz_processed_results = None

    # -- evaluate_utils.py:91-107
    def _postprocess_raw_results_no_merge(self):
        processed = {}
        for vid, items in self.raw_results.items():
            for it in items:
                preds = sorted(it["node_predictions"], key=lambda x: x[-1], reverse=True)
                processed.setdefault(vid, []).append({"query": it["query"], "gt": it["gt"], "node_predictions": preds,
                                                      "level": it["level"]})
        self.processed_results = processed

    # -- evaluate_utils.py:186-212
    @staticmethod
    def nms_temporal(x1, x2, s, overlap):
        assert len(x1) == len(s) and len(x2) == len(s)
        if len(x1) == 0:
            return []
        x1, x2, s = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64), np.asarray(s, dtype=np.float64)
        length = x2 - x1
        order = list(np.argsort(s, kind="stable"))        # ascending, ties in input order; visited from the end
        pick = []
        while order:
            i = order.pop()
            pick.append(int(i))
            if not order:
                break
            rest = np.asarray(order)
            inter = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]))
            with np.errstate(invalid="ignore", divide="ignore"):      # two empty segments: 0/0 = NaN, "not <= overlap" -> dropped, as in the reference
                o = inter / (length[i] + length[rest] - inter)
            order = [int(j) for j, keep in zip(rest, o <= overlap) if keep]
        return pick

    # -- evaluate_utils.py:228-232 (un-clamped)
    @staticmethod
    def calculate_IoU(i0, i1):
        union = (min(i0[0], i1[0]), max(i0[1], i1[1]))
        inter = (max(i0[0], i1[0]), min(i0[1], i1[1]))
        return 1.0 * (inter[1] - inter[0]) / (union[1] - union[0])

    # -- evaluate_utils.py:131-184
    def compute_IoU_recall_top_n_ours(self, top_n, iou_thresh, nms=False):
        correct, total = 0.0, 0.0
        picked = {}
        for vid, items in self.processed_results.items():
            for it in items:
                total += 1
                gt = it["gt"]
                preds = it["node_predictions"]
                if nms:
                    picks = self.nms_temporal([p[0] for p in preds], [p[1] for p in preds], [p[-1] for p in preds],
                                              iou_thresh - 0.05)
                else:
                    picks = list(range(len(preds)))
                merged_level = np.array([x for lv in it["level"] for x in lv])
                # (an independent record as the reference's deepcopy makes, without copying the predictions NMS drops: the deepcopy
                # of every item for every (IoU, top-k) pair was 70 % of Trainer.evaluate's time)
                rec = {k: deepcopy(v) for k, v in it.items() if k not in ("node_predictions", "level")}
                rec["node_predictions"] = [list(preds[i]) for i in picks] if nms else [list(p) for p in preds]
                rec["level"] = merged_level[picks].tolist()
                picked.setdefault(vid, []).append(rec)
                for i in picks[:top_n] if top_n < len(picks) else picks:
                    if self.calculate_IoU((gt[0], gt[1]), (preds[i][0], preds[i][1])) >= iou_thresh:
                        correct += 1
                        break
        self.viz_processed_results = picked
        return correct, total, correct / total

    # -- evaluate_utils.py:328-354
    def run_evaluate(self, iou_topk_dict, do_merge=False, update_score=False, score_weight=1.0, temporal_nms=False, viz_nms=True,
                     do_viz=""):
        assert isinstance(iou_topk_dict, dict)
        if do_merge:
            raise NotImplementedError("do_merge=True is dead code in the reference (evaluate_utils.py:336 raises TypeError)")
        if do_viz:
            raise NotImplementedError("plotly visualisation (evaluate_utils.py:240-326) is out of scope")
        self._postprocess_raw_results_no_merge()
        accs = []
        for iou_thresh in iou_topk_dict["iou"]:
            for topk in iou_topk_dict["topk"]:
                accs.append(self.compute_IoU_recall_top_n_ours(topk, iou_thresh, temporal_nms)[2])
        return iou_topk_dict["topk"], accs


def select_moments(preds, k, overlap):
    """The first k temporal-NMS survivors of one query's [[start, end, score], ...] predictions, best first: what the evaluator looks
    at (evaluate_utils.py:91-107 stable sort by descending score, then :186-212 nms_temporal at `overlap`; its value there is
    iou - 0.05), as indices into `preds`.  The host twin of drn_select_moments (ops.select_moments), for callers that hold host
    records.  An empty list has no picks (the device path's fallback moment is the post-processor's, inference.py:192-197)."""
    order = sorted(range(len(preds)), key=lambda i: preds[i][-1], reverse=True)
    picks = PostProcessRunner.nms_temporal([preds[i][0] for i in order], [preds[i][1] for i in order], [preds[i][-1] for i in order],
                                           overlap)
    return [order[i] for i in picks[:max(int(k), 0)]]


def merge_moments(per_pair_lists, video_ids, k, state=None):
    """The best k moments of ONE sentence across videos, best first: the host twin of drn_merge_moments (ops.merge_moments, the
    ranking of Grounder.search), for callers that hold host records.
    per_pair_lists[i]: the moments of the (sentence, video video_ids[i]) pair, best first (Moments.tolist()'s rows or select_moments'
    picks): [start, end, score] or [start, end, score, index] records; a moment's rank is its position in that list.
    Dropped: pairs whose video id is None or negative (padding), records that are None (padding), records with index < 0 (the
    fallback moment of a pair without candidates: (0, 1) with score 1 is no hit, and it would top every ranking) and records whose
    score is not finite.  Order: score descending, then video id ascending, then rank ascending -- total, so merging the videos in
    chunks (state = the result of the chunks before) gives the list that merging them at once gives.
    -> [[video, start, end, score, rank], ...], at most k."""
    cand = [list(r) for r in (state or [])]
    for vid, moments in zip(video_ids, per_pair_lists):
        if vid is None or vid < 0:
            continue
        for rank, r in enumerate(moments):
            if r is None or (len(r) > 3 and r[3] < 0) or not np.isfinite(r[2]):
                continue
            cand.append([vid, r[0], r[1], r[2], rank])
    cand.sort(key=lambda c: (-c[3], c[0], c[4]))
    return cand[:max(int(k), 0)]


def recall_from_first_hits(first_hits, ious, topks):
    """accs in run_evaluate's order (for iou: for topk) from the per-query first-hit positions of ops.eval_recall:
    first_hits (n_queries, len(ious)) integer array."""
    fh = np.asarray(first_hits).reshape(-1, len(ious))
    total = max(fh.shape[0], 1)
    return [float((fh[:, q] < k).sum()) / total for q in range(len(ious)) for k in topks]


def recall_from_ranks(ranks, topks):
    """The host twin of evaluate_shortlist's recalls: ranks, one integer per sentence -- the 0-based place of its target video in the
    FULL shortlist order (Shortlister.rank), -1 where the target is no candidate -> the fraction with 0 <= rank < k, one per k of
    topks; -1 counts as a miss at every depth.  No sentences: zeros."""
    r = np.asarray(ranks).reshape(-1)
    total = max(r.shape[0], 1)
    return [float(((r >= 0) & (r < int(k))).sum()) / total for k in topks]


def mrr_from_ranks(ranks):
    """The mean reciprocal rank, 1 / (rank + 1), of the same ranks; -1 is a miss and adds 0.  No sentences: 0."""
    r = np.asarray(ranks).reshape(-1).astype(np.float64)
    return float(np.where(r >= 0, 1.0 / (np.maximum(r, 0) + 1.0), 0.0).sum()) / max(r.shape[0], 1)


def median_rank_from_ranks(ranks):
    """The median 0-based rank of the same ranks; -1 is a miss and counts as infinitely deep (inf where half the sentences or more
    missed).  No sentences: nan."""
    r = np.asarray(ranks).reshape(-1).astype(np.float64)
    if r.shape[0] == 0:
        return float("nan")
    return float(np.median(np.where(r >= 0, r, np.inf)))


def search_first_hits(rows, gt_video, gt, ious, K):
    """Where the right moment of the right video first appears in a search's hits: the host twin of drn_search_recall
    (ops.search_recall), for callers that hold host records.  rows: Hits.tolist()'s, per sentence [[video, start, end, score], ...]
    best first (the first K are read); gt_video[s]: the annotated video as rows name it (a store position; negative: none);
    gt[s]: [start, end] as fractions of the video.  -> (S, len(ious) + 1) int32 array:
      column i < len(ious)  the position of the first row in the right video whose tIoU with gt[s] is >= ious[i] -- calculate_IoU's
                            un-clamped expression in doubles; a disjoint pair is negative, 0/0 and a NaN bound are no hit;
      last column           the number of DISTINCT videos ranked before the first row of the right video: its place in the video
                            ranking, however many moments per video competed;
    K where there is none.  recall_from_first_hits turns columns of either kind into recalls."""
    K, ious = int(K), [float(x) for x in ious]
    out = np.full((len(rows), len(ious) + 1), K, dtype=np.int32)
    for s, hits in enumerate(rows):
        gv, (g0, g1) = int(gt_video[s]), (float(x) for x in gt[s])
        if gv < 0:
            continue
        hits, before = hits[:max(K, 0)], set()
        for p, (v, x1, x2) in enumerate((h[0], float(h[1]), float(h[2])) for h in hits):
            if v != gv:
                before.add(v)
                continue
            if out[s, -1] == K:
                out[s, -1] = len(before)
            if g0 != g0 or g1 != g1 or x1 != x1 or x2 != x2:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):      # (x / 0 as IEEE has it, not ZeroDivisionError)
                iou = float(np.float64(min(g1, x2) - max(g0, x1)) / np.float64(max(g1, x2) - min(g0, x1)))
            for i, thr in enumerate(ious):
                if out[s, i] == K and iou >= thr:
                    out[s, i] = p
    return out


def results_entries(queries, gts, boxes):
    """results_entry for a whole batch with ONE device->host copy per field (all clips' detections / scores concatenated on
    the device first) instead of two per clip."""
    import torch
    dets = [b["detections"].detach().float() for b in boxes]
    scs = [b["scores"].detach().float() for b in boxes]
    if not dets or not dets[0].is_cuda:
        return [results_entry(q, g, b) for q, g, b in zip(queries, gts, boxes)]
    lens = [int(d.shape[0]) for d in dets]
    det = torch.cat(dets).cpu().numpy()
    sc = torch.cat(scs).cpu().numpy()
    out, o = [], 0
    for q, g, b, n in zip(queries, gts, boxes, lens):
        preds = np.concatenate([det[o:o + n], sc[o:o + n, None]], axis=1).tolist()
        out.append({"query": q, "gt": [float(g[0]), float(g[1])], "node_predictions": preds, "edge_predictions": preds,
                    "level": b["level"]})
        o += n
    return out


def results_entry(query, gt, box):
    """One main.py:324-348 record from a post-processor dict (drn_amd.model.inference) and its ground truth."""
    det = box["detections"].detach().float().cpu().numpy()
    sc = box["scores"].detach().float().cpu().numpy()
    preds = np.concatenate([det, sc[:, None]], axis=1).tolist()
    return {"query": query, "gt": [float(gt[0]), float(gt[1])], "node_predictions": preds, "edge_predictions": preds,
            "level": box["level"]}
