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
    statistics changed IN PLACE keep their address and are re-read by the scale/shift launches of every replay.  `captures` counts the captures made."""

    def __init__(self, model, top_k=5, nms_overlap=0.45, fused=False, graph=False, max_graphs=4):
        if int(top_k) < 1:
            raise DrnError("Grounder: top_k must be at least 1")
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
        ent = self._graphs.get(sig)
        if ent is None and len(self._graphs) >= self.max_graphs:
            return self._ground(*args)
        if video_index is not None:
            if video_index.dim() != 1 or video_index.is_floating_point():
                return self._ground(*args)                      # (refused there)
            if not video_index.is_cuda and video_index.numel():
                V = int(props_features.shape[0])
                if int(video_index.min()) < 0 or int(video_index.max()) >= V:
                    raise DrnError("Grounder: video_index outside [0, %d)" % V)
        stamp = self._stamp()
        if ent is not None and ent.stamp != stamp:
            del self._graphs[sig]
            ent = None
        if ent is None:
            ent = self._capture(args, sig)
            ent.stamp = self._stamp()
            self._graphs[sig] = ent
        else:
            for dst, src in zip(ent.inputs, args):
                if dst is not None and src is not dst and src.data_ptr() != dst.data_ptr():
                    dst.copy_(src, non_blocking=src.is_cuda)
            ent.graph.replay()
        return Moments(*[t.clone() for t in ent.out])

    def _capture(self, args, sig):
        """Static buffers <- this call's inputs, one warm run on the capture stream (lazy module loads, weight copies, workspaces), then
        the capture: everything on ONE stream, so the graph is one linear chain."""
        from .graph import capture_graph
        ent = _GroundGraph()
        dev = args[2].device
        ent.inputs = [None if t is None else (t.to(device=dev, dtype=torch.int32) if i == 4 else t).clone().contiguous()
                      for i, t in enumerate(args)]
        ent.stream = torch.cuda.Stream(device=dev)
        ent.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(ent.stream):
            self._ground(*ent.inputs)
        torch.cuda.current_stream().wait_stream(ent.stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture_graph(g, ent.stream):
            mom = self._ground(*ent.inputs)
        ent.graph = g
        ent.out = (mom.seg, mom.score, mom.level, mom.index, mom.n)
        self.captures += 1
        g.replay()
        return ent

    def _ground(self, query_tokens, query_length, props_features, props_start_end, video_index=None):
        from . import functional as DF
        model = self.model
        selector = model.fcos.box_selector_test
        if model.fcos.head.cls_logits.weight.shape[0] != 1:
            raise DrnError("Grounder: the device post-processor serves one foreground channel (fcos_num_class = 2); this model has %d"
                           % model.fcos.head.cls_logits.weight.shape[0])
        was = selector.device_only
        selector.device_only = True
        try:
            with DF.fused_eval(self.fused):
                locations, box_cls, box_reg, iou_scores = model.forward_heads_shared(query_tokens, query_length, props_features,
                                                                                     props_start_end, video_index)
            dd = selector(locations, box_cls, box_reg, iou_scores)
        finally:
            selector.device_only = was
        if isinstance(dd, list):
            raise DrnError("Grounder: the post-processor has no flat device path for this model (min_size != 0?)")
        return Moments(*ops.select_moments(dd.det, dd.scores, dd.counts, self.nms_overlap, self.top_k))
