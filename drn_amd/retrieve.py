"""The first stage of a two-stage search, on the device: each sentence's best n videos by the dot product of CALLER-SUPPLIED embeddings.

The project has no video-level embedding of its own (DRN has none) and this module invents none: the (V, E) table and the (S, E)
queries come from any dual encoder.  What it supplies is the ranking -- under a TOTAL order (score descending, then store position
ascending), so that equal scores fall the same way in every run and every build, which torch.topk does not promise -- and a result
that never leaves the device: Shortlist.ids is what Grounder.search(candidates=) takes as a device tensor.

shortlist_reference is the definition, in plain torch; Shortlister.shortlist is drn_shortlist_topn (csrc/retrieve.hip)."""
import collections

import torch

from . import ops
from ._lib import SHORTLIST_MAX, DrnError      # SHORTLIST_MAX = 128 is a CHOICE, not a measurement (see _lib.py, include/drn_hip.h)

Shortlist = collections.namedtuple("Shortlist", "ids scores n")
Shortlist.__doc__ = """ids (S, n) int32 store positions, best first, -1 past the list; scores (S, n) float32, 0 past the list; n (S,) int32 the
length of each sentence's list.  All on the device."""


def shortlist_reference(embeddings, queries, n):
    """THE DEFINITION of a shortlist, in float64 (usable on the CPU): score[s, v] = sum_e queries[s, e] * embeddings[v, e]; sentence s
    lists the videos whose score is finite, ordered by higher score, then lower position, cut to n.  Past the list ids = -1 and
    scores = 0; n[s] is its length (a NaN query row lists nothing).  -> Shortlist on the inputs' device, scores rounded to float32."""
    n = int(n)
    emb, q = embeddings.double(), queries.double()
    V, S = int(emb.shape[0]), int(q.shape[0])
    score = q @ emb.t()
    finite = torch.isfinite(score)
    key = torch.where(finite, score, torch.full_like(score, float("-inf")))
    # a stable sort by descending score keeps equal scores in position order
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    count = finite.sum(dim=1).clamp(max=n)
    ids = torch.full((S, n), -1, dtype=torch.int32, device=emb.device)
    scores = torch.zeros((S, n), dtype=torch.float32, device=emb.device)
    m = min(n, V)
    listed = torch.arange(m, device=emb.device)[None, :] < count[:, None]
    ids[:, :m] = torch.where(listed, order[:, :m].to(torch.int32), ids[:, :m])
    scores[:, :m] = torch.where(listed, torch.gather(score, 1, order[:, :m]).float(), scores[:, :m])
    return Shortlist(ids, scores, count.to(torch.int32))


class Shortlister(object):
    """Shortlister(embeddings, names=None): a (V, E) table of video embeddings, row v belonging to store position v -- a contiguous
    CUDA tensor, bfloat16 or float32, V >= 1 and E >= 1, kept by reference.  Non-finite embeddings are refused here (ONE
    synchronise, once).  names: kept when given; check(store) raises unless they are the store's, before any launch."""

    def __init__(self, embeddings, names=None):
        if not torch.is_tensor(embeddings) or not embeddings.is_cuda:
            raise DrnError("Shortlister: the embeddings must be a tensor on the GPU; there is no CPU fallback")
        if embeddings.dtype not in (torch.bfloat16, torch.float32):
            raise DrnError("Shortlister: the embeddings must be bfloat16 or float32, not %s" % embeddings.dtype)
        if embeddings.dim() != 2 or embeddings.shape[0] < 1 or embeddings.shape[1] < 1 or not embeddings.is_contiguous():
            raise DrnError("Shortlister: the embeddings must be a contiguous (V, E) tensor with V >= 1 and E >= 1, not %s"
                           % (tuple(embeddings.shape),))
        self.names = None if names is None else list(names)
        if self.names is not None and len(self.names) != int(embeddings.shape[0]):
            raise DrnError("Shortlister: %d names for %d embeddings" % (len(self.names), int(embeddings.shape[0])))
        if not bool(torch.isfinite(embeddings).all()):
            raise DrnError("Shortlister: the embeddings hold values that are not finite")
        self.embeddings = embeddings
        self._ws = {}

    def __len__(self):
        return int(self.embeddings.shape[0])

    def check(self, store):
        """Raises unless this table's names are the store's (a FeatureStore or a SearchIndex), position by position."""
        if self.names is None or self.names != list(store.names):
            raise DrnError("Shortlister: the table's names are not the store's (row v must belong to store position v)")

    def _check(self, queries, n, out):
        """shortlist's refusals, before the library is reached -> (S, n)."""
        emb = self.embeddings
        if not torch.is_tensor(queries):
            raise DrnError("Shortlister.shortlist: the queries must be a tensor")
        if queries.dim() != 2 or queries.shape[0] < 1 or queries.shape[1] != emb.shape[1]:
            raise DrnError("Shortlister.shortlist: the queries must be (S, %d), not %s" % (int(emb.shape[1]), tuple(queries.shape)))
        if queries.dtype != emb.dtype:
            raise DrnError("Shortlister.shortlist: the queries are %s, the table is %s" % (queries.dtype, emb.dtype))
        n = int(n)
        if not 1 <= n <= SHORTLIST_MAX:
            raise DrnError("Shortlister.shortlist: n = %d outside [1, %d]" % (n, SHORTLIST_MAX))
        if not queries.is_cuda:
            raise DrnError("Shortlister.shortlist: the queries must be on the GPU; there is no CPU fallback")
        S = int(queries.shape[0])
        if out is not None:
            for name, t, dt, shape in zip(Shortlist._fields, out, (torch.int32, torch.float32, torch.int32), ((S, n), (S, n), (S,))):
                if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                    raise DrnError("Shortlister.shortlist: out.%s must be a contiguous %s %s tensor on the GPU" % (name, shape, dt))
        return S, n

    def shortlist(self, queries, n, out=None):
        """queries (S, E) on the device in the table's dtype, 1 <= n <= SHORTLIST_MAX -> Shortlist (shortlist_reference defines it),
        on the device.  out: a Shortlist (or 3-tuple) of buffers written in place, every element, and returned.  Runs on the current
        stream without a host synchronisation and can be captured in a graph (the workspace is kept per (S, n): warm the shape once
        before capturing).  Scores are accumulated in fp32 in an order that is fixed per (sentence, video): the same bits whatever
        V, S or n."""
        S, n = self._check(queries, n, out)
        dev = self.embeddings.device
        if out is None:
            out = (torch.empty((S, n), dtype=torch.int32, device=dev), torch.empty((S, n), dtype=torch.float32, device=dev),
                   torch.empty((S,), dtype=torch.int32, device=dev))
        ws = self._ws.get((S, n))
        if ws is None:
            ws = self._ws[(S, n)] = torch.empty(ops.shortlist_ws_keys(len(self), S, n), dtype=torch.int64, device=dev)
        ops.shortlist_topn(self.embeddings, queries.contiguous(), n, ws, *out)
        return Shortlist(*out)
