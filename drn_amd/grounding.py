"""Grounding without a ground truth: "here is a video and some sentences, give me the best moments".

Grounder.ground = mainModel.forward_heads_shared (the query-independent part of the forward -- prop_fc above all -- once per VIDEO,
however many sentences ask about it) -> the device post-processor (drn_postprocess) -> the evaluator's temporal NMS on the device
(drn_select_moments: utils/evaluate_utils.py:91-107,186-212), which hands back the surviving moments themselves, best first.
Nothing crosses to the host until the caller asks (Moments.tolist)."""
import torch

from . import ops
from ._lib import DrnError


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

    def tolist(self):
        """Per query [[start, end, score], ...], the first n[q] entries: one host copy per field."""
        n, seg, score = self.n.tolist(), self.seg.tolist(), self.score.tolist()
        return [[[seg[q][i][0], seg[q][i][1], score[q][i]] for i in range(n[q])] for q in range(len(n))]


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


class Grounder(object):
    """Grounder(model, top_k=5, nms_overlap=0.45).ground(query_tokens, query_length, props_features, props_start_end,
    video_index=None) -> Moments.  nms_overlap: the NMS threshold itself; 0.45 is the evaluator's 0.5 - 0.05 for Recall@IoU 0.5.
    The model must be in eval mode; ground() runs under torch.no_grad() and changes no model state."""

    def __init__(self, model, top_k=5, nms_overlap=0.45):
        if int(top_k) < 1:
            raise DrnError("Grounder: top_k must be at least 1")
        self.model, self.top_k, self.nms_overlap = model, int(top_k), float(nms_overlap)

    @torch.no_grad()
    def ground(self, query_tokens, query_length, props_features, props_start_end, video_index=None):
        model = self.model
        selector = model.fcos.box_selector_test
        if model.fcos.head.cls_logits.weight.shape[0] != 1:
            raise DrnError("Grounder: the device post-processor serves one foreground channel (fcos_num_class = 2); this model has %d"
                           % model.fcos.head.cls_logits.weight.shape[0])
        was = selector.device_only
        selector.device_only = True
        try:
            locations, box_cls, box_reg, iou_scores = model.forward_heads_shared(query_tokens, query_length, props_features,
                                                                                 props_start_end, video_index)
            dd = selector(locations, box_cls, box_reg, iou_scores)
        finally:
            selector.device_only = was
        if isinstance(dd, list):
            raise DrnError("Grounder: the post-processor has no flat device path for this model (min_size != 0?)")
        return Moments(*ops.select_moments(dd.det, dd.scores, dd.counts, self.nms_overlap, self.top_k))
