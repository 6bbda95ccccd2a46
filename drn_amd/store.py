"""Proposal features built on the device from a resident feature store.

The host data path (drn_amd.data: one torch.load and one torch.max per proposal per SAMPLE, then collate_data's padding and a
B x T x D copy over PCIe per step) stays the oracle; this module is its device twin for training and grounding at speed:

  FeatureStore   every video's sliding-window features, packed (R, D) in the model's dtype, on the device ONCE, with the per-video
                 tables of proposal windows [lo, hi] and bounds (drn_amd.data.proposal_windows);
  store.gather   one drn_pool_props launch: (B, T, D) proposal features + (B, T, 2) bounds of B videos, zero-padded to T;
  StoreLoader    a DataLoader stand-in that yields collate_data's 8-tuple with the five model inputs on the device: per step only
                 the tokens, lengths, ground truth and video indices leave the host.

Values: a proposal's feature is the max over its rows of the STORED values.  A bf16 store holds the fp32 features rounded to nearest
even, and rounding is monotone, so max-then-round (collate_data(feature_dtype=torch.bfloat16)) and round-then-max (here) agree
bit for bit (up to the sign of a zero maximum)."""
import os

import numpy as np
import torch

from . import ops
from ._lib import DrnError
from .data import proposal_windows


class FeatureStore(object):
    """names: the videos in store order; index: name -> position; nprops / nframes / nrows: per-video host arrays; D, dtype, device;
    nbytes: bytes the store occupies on the device (features + tables)."""

    def __init__(self, names, feats, seg_off, prop_off, win, pse, nframes, device):
        self.names = list(names)
        self.index = {n: i for i, n in enumerate(self.names)}
        self.nrows = np.diff(seg_off.numpy()).astype(np.int64)
        self.nprops = np.diff(prop_off.numpy()).astype(np.int32)
        self.nframes = np.asarray(nframes, dtype=np.int64)
        self.max_rows = int(self.nrows.max()) if len(self.names) else 0
        self.D, self.dtype = int(feats.shape[1]), feats.dtype
        self.nbytes = self.bytes_of(feats.shape[0], self.D, self.dtype, len(self.names), win.shape[0])
        self.device = torch.device(device)
        mv = lambda t: t.to(self.device)
        self.feats, self.seg_off, self.prop_off, self.win, self.pse = mv(feats), mv(seg_off), mv(prop_off), mv(win), mv(pse)

    @staticmethod
    def bytes_of(rows, D, dtype, videos, proposals):
        """Device bytes of a store: the packed features, seg_off (int64), prop_off (int32), win (2 x int32), pse (2 x float64)."""
        es = torch.empty((), dtype=dtype).element_size()
        return int(rows) * int(D) * es + (int(videos) + 1) * 12 + int(proposals) * 24

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_tensors(cls, videos, device, dtype, max_bytes=None):
        """videos: iterable of (name, feats (S, D) float tensor, lo (P,), hi (P,), pse (P, 2), num_frames) -- lo / hi / pse as
        proposal_windows returns them.  Casts to `dtype` (float32 / bfloat16), refuses non-finite values (the kernel's maximum is
        defined for finite values), a video without rows, a feature dimension that differs between videos and windows outside the
        video; raises DrnError BEFORE anything is uploaded when the store would exceed max_bytes."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise DrnError("FeatureStore: dtype must be torch.float32 or torch.bfloat16, not %s" % dtype)
        names, parts, los, his, pses, nframes, seg, prop = [], [], [], [], [], [], [0], [0]
        D, seen = None, set()
        for name, f, lo, hi, pse, nf in videos:
            f = torch.as_tensor(f)
            if f.dim() != 2 or f.shape[0] < 1 or not f.is_floating_point():
                raise DrnError("FeatureStore: video %s: features must be a (segments >= 1, dim) float tensor" % name)
            D = int(f.shape[1]) if D is None else D
            if int(f.shape[1]) != D:
                raise DrnError("FeatureStore: video %s has feature dimension %d, the videos before it %d" % (name, f.shape[1], D))
            f = f.detach().to(device="cpu", dtype=dtype)
            if not bool(torch.isfinite(f).all()):
                raise DrnError("FeatureStore: video %s holds NaN or Inf (after the cast to %s)" % (name, dtype))
            lo, hi = np.asarray(lo, dtype=np.int32).reshape(-1), np.asarray(hi, dtype=np.int32).reshape(-1)
            pse = np.asarray(pse, dtype=np.float64).reshape(-1, 2)
            if not (len(lo) == len(hi) == len(pse)) or (len(lo) and (lo.min() < 0 or (hi < lo).any() or hi.max() >= f.shape[0])):
                raise DrnError("FeatureStore: video %s: proposal windows must satisfy 0 <= lo <= hi < %d" % (name, f.shape[0]))
            if name in seen:
                raise DrnError("FeatureStore: video %s is listed twice" % name)
            seen.add(name)
            names.append(name); parts.append(f); los.append(lo); his.append(hi); pses.append(pse); nframes.append(int(nf))
            seg.append(seg[-1] + int(f.shape[0])); prop.append(prop[-1] + len(lo))
        if not names:
            raise DrnError("FeatureStore: no videos")
        if prop[-1] > 0x7fffffff:
            raise DrnError("FeatureStore: more than 2^31 proposals")
        need = cls.bytes_of(seg[-1], D, dtype, len(names), prop[-1])
        if max_bytes is not None and need > max_bytes:
            raise DrnError("FeatureStore: %d videos (%d rows x %d, %s) need %d bytes on the device, max_bytes is %d"
                           % (len(names), seg[-1], D, dtype, need, max_bytes))
        win = np.stack([np.concatenate(los), np.concatenate(his)], axis=1).astype(np.int32) if prop[-1] else np.zeros((0, 2), np.int32)
        pse = np.concatenate(pses).astype(np.float64) if prop[-1] else np.zeros((0, 2), np.float64)
        return cls(names, torch.cat(parts), torch.tensor(seg, dtype=torch.int64), torch.tensor(prop, dtype=torch.int32),
                   torch.from_numpy(np.ascontiguousarray(win)), torch.from_numpy(np.ascontiguousarray(pse)), nframes, device)

    @classmethod
    def from_dataset(cls, dataset, device, dtype, max_bytes=None):
        """Every video of the dataset's props table (drn_amd.data.CharadesSTA: `props`, `ft_root`, window size / overlap), each
        feature file loaded once."""
        def videos():
            for vid, (num_frames, proposals) in dataset.props.items():
                f = torch.load(os.path.join(dataset.ft_root, "%s.pt" % vid))
                lo, hi, pse = proposal_windows(proposals, num_frames, len(f), dataset.ft_window_size, dataset.ft_overlap)
                yield vid, f, lo, hi, pse, num_frames
        return cls.from_tensors(videos(), device, dtype, max_bytes)

    def ids_of(self, names_or_ids):
        """-> (B,) int32 host tensor of store positions; names are looked up, integers are taken as they are (range-checked by
        the launch)."""
        if torch.is_tensor(names_or_ids):
            return names_or_ids.detach().to(device="cpu", dtype=torch.int32).reshape(-1).contiguous()
        ids = []
        for x in names_or_ids:
            if isinstance(x, str):
                if x not in self.index:
                    raise DrnError("FeatureStore: no video named %s" % x)
                x = self.index[x]
            ids.append(int(x))
        return torch.tensor(ids, dtype=torch.int32)

    def gather(self, names_or_ids, out=None, out_pse=None, T=None):
        """(B, T, D) proposal features in the store dtype, (B, T, 2) float64 bounds -- both on the device, zero past each video's
        proposals -- and the (B,) int64 host tensor of proposal counts: one drn_pool_props launch on the current stream, no host
        synchronisation.  names_or_ids: video names, store positions, or a host tensor of positions (checked on the host: a position
        outside the store raises before the launch); T: the padded proposal count, default the largest count of the batch.
        A DEVICE int32 tensor of positions is used as it is (a captured graph re-reads it at every replay): T is then required,
        nothing is checked on the host, a position outside the store yields zero rows, and the third value is None.
        out / out_pse: buffers of exactly that shape and dtype to write into instead of new ones (every element is overwritten)."""
        if torch.is_tensor(names_or_ids) and names_or_ids.is_cuda:
            if T is None:
                raise DrnError("FeatureStore.gather: device indices need T (nothing is read back to find it)")
            vids, vids_host, counts, nprops = names_or_ids, None, None, None
            if vids.dtype != torch.int32 or vids.dim() != 1 or not vids.is_contiguous():
                raise DrnError("FeatureStore.gather: device indices must be a contiguous (B,) int32 tensor")
        else:
            vids_host = self.ids_of(names_or_ids)
            inside = (vids_host >= 0) & (vids_host < len(self.names))
            counts = torch.from_numpy(self.nprops)[vids_host.long().clamp(0, len(self.names) - 1)] * inside.to(torch.int32)
            counts = counts.to(torch.int32).contiguous()
            if T is None:
                T = int(counts.max()) if counts.numel() else 0
            nprops = counts.to(torch.int64)
            vids = None
        B, T = int(vids_host.numel() if vids is None else vids.numel()), int(T)
        for name, buf, shape, dt in (("out", out, (B, T, self.D), self.dtype), ("out_pse", out_pse, (B, T, 2), torch.float64)):
            if buf is not None and (tuple(buf.shape) != shape or buf.dtype != dt or buf.device != self.feats.device or not buf.is_contiguous()):
                raise DrnError("FeatureStore.gather: %s must be a contiguous %s %s tensor on %s" % (name, shape, dt, self.feats.device))
        if not self.feats.is_cuda:
            raise DrnError("FeatureStore.gather runs on the GPU only (this store lives on %s); there is no CPU fallback" % self.device)
        if vids is None:
            vids = _upload(vids_host, self.device)
        out = torch.empty((B, T, self.D), dtype=self.dtype, device=self.device) if out is None else out
        out_pse = torch.empty((B, T, 2), dtype=torch.float64, device=self.device) if out_pse is None else out_pse
        ops.pool_props(self.feats, self.seg_off, self.prop_off, self.win, self.pse, vids, T, out, out_pse, vids_host=vids_host,
                       counts_host=counts, max_rows=self.max_rows, tag="pool_props")
        return out, out_pse, nprops


def _upload(t, device):
    """A small host tensor -> the device through pinned memory, not waited for (the caching host allocator keeps the pinned block
    until the copy has run)."""
    return t.pin_memory().to(device, non_blocking=True)


class StoreLoader(object):
    """Iterable over the batches of `dataset` (drn_amd.data.CharadesSTA) in the order and composition of
    DataLoader(dataset, batch_size, shuffle, sampler, drop_last, generator, collate_fn=collate_data), yielding collate_data's 8-tuple
    (names, props_start_end, props_features, gt, tokens, query_length, nprops, nframes) with the five model inputs ON THE DEVICE --
    features and bounds from store.gather (one launch), ground truth / tokens / lengths through one pinned non-blocking copy each --
    and nprops / nframes on the host, as collate_data leaves them.  Within a batch the samples are ordered by query length,
    descending and stable.  dataset[i] is never called: no feature file is opened after the store was built.
    `.sampler` is the index sampler (Trainer.train_epoch calls its set_epoch); host_batches() yields the host half alone."""

    def __init__(self, dataset, store, batch_size, shuffle=False, sampler=None, drop_last=False, generator=None):
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        if sampler is not None and shuffle:
            raise ValueError("StoreLoader: sampler and shuffle exclude each other")
        if sampler is None:
            sampler = RandomSampler(dataset, generator=generator) if shuffle else SequentialSampler(dataset)
        self.dataset, self.store, self.sampler = dataset, store, sampler
        self.batch_sampler = BatchSampler(sampler, int(batch_size), bool(drop_last))
        self._meta = [dataset.meta(i) for i in range(len(dataset))]
        missing = sorted(set(m[0] for m in self._meta) - set(store.index))
        if missing:
            raise DrnError("StoreLoader: the store lacks %d of the dataset's videos (%s ...)" % (len(missing), missing[0]))

    def __len__(self):
        return len(self.batch_sampler)

    def host_batches(self):
        """Per batch (names, video positions (B,) int32, gt (B, 2) float64, tokens (B, Lmax) int64, query_length (B,) int64,
        nprops (B,) int64, nframes (B,) int64), all on the host, in collate_data's order."""
        for indices in self.batch_sampler:
            rows = sorted((self._meta[i] for i in indices), key=lambda m: len(m[1]), reverse=True)
            names = [m[0] for m in rows]
            vids = torch.tensor([self.store.index[n] for n in names], dtype=torch.int32)
            qlen = torch.tensor([len(m[1]) for m in rows], dtype=torch.int64)
            tok = torch.zeros((len(rows), int(qlen.max()) if len(rows) else 0), dtype=torch.int64)
            for i, m in enumerate(rows):
                tok[i, :len(m[1])] = m[1]
            gt = torch.tensor([m[2] for m in rows], dtype=torch.float64).reshape(len(rows), 2)
            nprops = torch.from_numpy(self.store.nprops)[vids.long()].to(torch.int64)
            nframes = torch.tensor([m[3] for m in rows], dtype=torch.int64)
            yield names, vids, gt, tok, qlen, nprops, nframes

    def __iter__(self):
        dev = self.store.device
        for names, vids, gt, tok, qlen, nprops, nframes in self.host_batches():
            feats, pse, _ = self.store.gather(vids)
            yield names, pse, feats, _upload(gt, dev), _upload(tok, dev), _upload(qlen, dev), nprops, nframes
