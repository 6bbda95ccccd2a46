"""A projected search index: prop_fc once per video, not once per search.

Grounder.search on a FeatureStore re-runs, for every chunk of every call, the part of the forward that no sentence touches: the
proposal pooling (drn_pool_props), the cast, the prop_fc GEMM (2 T D^2 FLOPs per video) and the position embedding.  SearchIndex.build
runs exactly those launches once per video and keeps their outputs for the real proposals, packed ragged:

  rows (P_total + 1, Dp + P), the model's compute dtype: columns [0, Dp) the un-gated prop_fc output, [Dp, Dp + P) the position
  embedding; video v owns rows[prop_off[v] : prop_off[v + 1]]; the last row is the PAD row -- what the same launches give for a zero
  feature row with zero bounds, i.e. what conv0 is fed past a video's proposals and for an empty chunk slot.

Grounder.search(tokens, lengths, index) then builds conv0's input of a chunk with ONE launch (drn_gate_gather_packed) and runs the
trunk as before.  The index is bound to the weights it was built from (is_current / refresh)."""
import weakref

import numpy as np
import torch

from . import ops
from ._lib import DrnError
from .store import FeatureStore, _upload


class SearchIndex(object):
    """names, index, nprops, D, dtype, device, nbytes and len() with FeatureStore's meaning (positions are store positions); rows,
    prop_off (device int32, the index's own copy of the store's table), pad_row (the position of the pad row), Dp (the zero-padded
    feature width the model's front runs on: 512 for D = 500 in bf16, D otherwise), P (position-embedding width).  The index holds no
    reference to the store's features (only a weak one to the store, for refresh): the store may be dropped."""

    # Rows (videos x T) one build step projects by default.  A CHOICE, not a measurement: 8192 rows of D = 4096 in bf16 are 64 MiB of
    # pooled features and as much again of projected rows per step, and a GEMM of that height fills the device.
    BUILD_ROWS = 8192

    def __init__(self):
        self.rows = self.prop_off = None

    def __len__(self):
        return len(self.names)

    ids_of = FeatureStore.ids_of

    @staticmethod
    def bytes_of(proposals, width, dtype, videos):
        """Device bytes of an index: the packed rows with the pad row, and prop_off (int32)."""
        return (int(proposals) + 1) * int(width) * torch.empty((), dtype=dtype).element_size() + (int(videos) + 1) * 4

    @staticmethod
    def _stamp(model):
        ps = (model.prop_fc.weight, model.prop_fc.bias, model.position_transform.weight, model.position_transform.bias)
        return tuple((id(p), p.data_ptr(), p._version) for p in ps) + (model.compute_dtype,)

    @classmethod
    def build(cls, model, store, chunk=None, max_bytes=None):
        """Walk the whole store once, in store order, in chunks of `chunk` videos (one shape: the last chunk is padded with position
        -1): store.gather on device positions with T = the store's largest proposal count -> model.prepare_input(split_gate=True)
        (cast, prop_fc, position embedding), eval mode under no_grad -> the real proposals' rows copied into the packed table on the
        device, no host synchronisation.  Raises DrnError BEFORE anything is allocated when the index would exceed max_bytes."""
        if model.training:
            raise DrnError("SearchIndex.build is inference only: call model.eval() first")
        if not store.feats.is_cuda:
            raise DrnError("SearchIndex.build needs a store on the GPU (this one lives on %s); there is no CPU fallback" % store.device)
        if store.dtype != model.compute_dtype:
            raise DrnError("SearchIndex.build: the store holds %s, the model computes in %s" % (store.dtype, model.compute_dtype))
        if store.D != model.feature_dim:
            raise DrnError("SearchIndex.build: the store's features have %d columns, the model's %d" % (store.D, model.feature_dim))
        self = cls()
        self.names, self.index = list(store.names), dict(store.index)
        self.nprops = store.nprops.copy()
        self.D, self.dtype, self.device = store.D, store.dtype, store.device
        self.Dp = self.D + model._front_pad(self.D)
        self.P = int(model.position_transform.weight.shape[0])
        self.T = int(self.nprops.max()) if len(self.names) else 0
        total = int(self.nprops.sum())
        self.pad_row = total
        self.nbytes = self.bytes_of(total, self.Dp + self.P, self.dtype, len(self.names))
        if max_bytes is not None and self.nbytes > max_bytes:
            raise DrnError("SearchIndex: %d videos (%d proposals x %d, %s) need %d bytes on the device, max_bytes is %d"
                           % (len(self.names), total, self.Dp + self.P, self.dtype, self.nbytes, max_bytes))
        self.rows = torch.empty((total + 1, self.Dp + self.P), dtype=self.dtype, device=self.device)
        self.prop_off = store.prop_off.clone()
        self._fill(model, store, chunk)
        return self

    def _fill(self, model, store, chunk):
        Nv, T = len(self.names), max(self.T, 1)
        Vc = max(1, min(Nv, self.BUILD_ROWS // T)) if chunk is None else int(chunk)
        if Vc < 1:
            raise DrnError("SearchIndex.build: chunk must be at least 1")
        nchunks = -(-Nv // Vc)
        off = np.concatenate([[0], np.cumsum(self.nprops, dtype=np.int64)])
        # the pad row comes out of the walk's own launches: the last padded position of the last chunk that has one -- past a
        # video's proposals or in an empty slot -- and, when no chunk has one, one more chunk of empty slots
        vids = np.full((nchunks, Vc), -1, dtype=np.int32)
        vids.reshape(-1)[:Nv] = np.arange(Nv, dtype=np.int32)
        counts = np.where(vids >= 0, self.nprops[np.maximum(vids, 0)], 0)
        padded = np.nonzero((counts < T).any(axis=1))[0]
        if padded.size == 0:
            vids = np.concatenate([vids, np.full((1, Vc), -1, dtype=np.int32)])
            counts = np.concatenate([counts, np.zeros((1, Vc), dtype=counts.dtype)])
            pad_chunk = nchunks
        else:
            pad_chunk = int(padded[-1])
        # ONE upload: the chunks' store positions, then per chunk the positions (slot * T + t) of its real proposals in chunk order
        # (= packed order: the chunks walk the store in order), then the pad position
        take = [np.concatenate([s * T + np.arange(n, dtype=np.int64) for s, n in enumerate(c)] + [np.zeros(0, np.int64)]) for c in counts]
        pad_slot = int(np.nonzero(counts[pad_chunk] < T)[0][-1])
        plan = np.concatenate([vids.reshape(-1).astype(np.int64)] + take + [np.asarray([pad_slot * T + T - 1], dtype=np.int64)])
        plan = _upload(torch.from_numpy(plan), self.device)
        vid_dev = plan[:vids.size].to(torch.int32).view(vids.shape)
        Dp, at = self.Dp, vids.size
        with torch.no_grad():
            for c in range(vids.shape[0]):
                n = int(counts[c].sum())
                if n == 0 and c != pad_chunk:
                    continue
                feats, pse, _ = store.gather(vid_dev[c], T=T)
                prep = model.prepare_input(feats, pse, split_gate=True)
                if prep.G0 is None or prep.Z is None or prep.Z.shape[2] != Dp:
                    raise DrnError("SearchIndex.build: the model's input stage did not produce the projected rows")
                Z, G0 = prep.Z.view(Vc * T, Dp), prep.G0.view(Vc * T, Dp + self.P)
                first = int(off[min(c * Vc, Nv)])
                for idx, dst in ((plan[at:at + n], self.rows[first:first + n]),) + \
                        (((plan[-1:], self.rows[self.pad_row:]),) if c == pad_chunk else ()):
                    if idx.numel():
                        dst[:, :Dp] = Z.index_select(0, idx)
                        dst[:, Dp:] = G0[:, Dp:].index_select(0, idx)
                at += n
        self.stamp = self._stamp(model)
        self._chunk, self._store = chunk, weakref.ref(store)

    def is_current(self, model):
        """Whether the rows are what `model` would project now: prop_fc / position_transform weight and bias are the tensors they
        were (identity, address, version) and the compute dtype is the same."""
        return self.stamp == self._stamp(model)

    def refresh(self, model, store=None):
        """Rebuild into the SAME buffers with the model's present weights.  store: default the store the index was built from, while
        the caller still holds it (the index keeps only a weak reference); otherwise a store of the same videos and proposals."""
        store = self._store() if store is None else store
        if store is None:
            raise DrnError("SearchIndex.refresh: the store the index was built from is gone: pass one with the same videos")
        if model.training:
            raise DrnError("SearchIndex.refresh is inference only: call model.eval() first")
        if store.dtype != model.compute_dtype or store.dtype != self.dtype or store.D != self.D or store.D != model.feature_dim \
                or self.Dp != self.D + model._front_pad(self.D) or self.P != int(model.position_transform.weight.shape[0]):
            raise DrnError("SearchIndex.refresh: the model or the store no longer has the index's dtype or widths: build a new index")
        if list(store.names) != self.names or not np.array_equal(store.nprops, self.nprops) or not store.feats.is_cuda:
            raise DrnError("SearchIndex.refresh: the store does not hold the index's videos and proposals on the GPU")
        self._fill(model, store, self._chunk)
        return self

    def check(self, model, what="SearchIndex"):
        if not self.is_current(model):
            raise DrnError("%s: the index is stale (prop_fc / position_transform changed, or it was built for another model or "
                           "compute dtype): call index.refresh(model)" % what)
