"""A projected search index: prop_fc once per video, not once per search.

Grounder.search on a FeatureStore re-runs, for every chunk of every call, the part of the forward that no sentence touches: the
proposal pooling (drn_pool_props), the cast, the prop_fc GEMM (2 T D^2 FLOPs per video) and the position embedding.  SearchIndex.build
runs exactly those launches once per video and keeps their outputs for the real proposals, packed ragged:

  rows (P_total + 1, Dp + P), the model's compute dtype: columns [0, Dp) the un-gated prop_fc output, [Dp, Dp + P) the position
  embedding; video v owns rows[prop_off[v] : prop_off[v + 1]]; the last row is the PAD row -- what the same launches give for a zero
  feature row with zero bounds, i.e. what conv0 is fed past a video's proposals and for an empty chunk slot.

Grounder.search(tokens, lengths, index) then builds conv0's input of a chunk with ONE launch (drn_gate_gather_packed) and runs the
trunk as before.  The index is bound to the weights it was built from (is_current / refresh).

SearchIndex.build(..., quantize="mxfp8") keeps the prop_fc columns in block-scaled FP8 instead (the MX layout: OCP e4m3fn codes, one
power-of-two scale per 32 columns; mx8_quantize below is the definition, drn_quantize_rows_mx8 its device twin): codes
(P_total + 1, Dp) u8, scales (P_total + 1, Dp / 32) u8 and pos (P_total + 1, P) in the compute dtype -- Dp + Dp / 32 + P * itemsize
bytes a row instead of (Dp + P) * itemsize.  drn_gate_gather_packed_q8 dequantises inside the same one launch.  A dequantised value is
exact in fp32 and bf16, so the quantised index answers bit for bit like index.dequantized(), a plain index of the dequantised rows."""
import weakref

import numpy as np
import torch

from . import ops
from ._lib import DrnError
from .store import FeatureStore, _upload


MX8_BLOCK, MX8_EMIN = 32, -110
QUANTIZE = (None, "mxfp8")


def mx8_quantize(x):
    """x (n, C) float32 / bfloat16 (finite), C % 32 == 0 -> (codes (n, C) uint8, scales (n, C / 32) uint8): THE DEFINITION of the
    format.  Per block of 32 columns: amax = max |x| in fp32 = m * 2^k, m in [0.5, 1) (frexp); e = k - 9 if m <= 0.875 else k - 8 --
    the smallest e with amax <= 448 * 2^e -- a zero block takes e = -110, and e is clamped to [-110, 127] (with the lower bound every
    dequantised value is zero or a normal number in fp32 and bf16); scale byte = e + 127, an e8m0 exponent and the fp32 exponent
    field of 2^e; code = e4m3fn(x * 2^-e), round to nearest even, the sign kept where the value rounds to zero."""
    if x.dim() != 2 or x.shape[1] % MX8_BLOCK:
        raise DrnError("mx8_quantize: x must be (n, C) with C a multiple of %d (got %s)" % (MX8_BLOCK, tuple(x.shape)))
    n, C = x.shape
    blocks = x.float().reshape(n, C // MX8_BLOCK, MX8_BLOCK)
    amax = blocks.abs().amax(dim=2)
    m, k = torch.frexp(amax)
    e = torch.where(m <= 0.875, k - 9, k - 8)
    e = torch.where(amax == 0, torch.full_like(e, MX8_EMIN), e).clamp(MX8_EMIN, 127)
    codes = torch.ldexp(blocks, -e.unsqueeze(2)).to(torch.float8_e4m3fn).view(torch.uint8).reshape(n, C)
    return codes, (e + 127).to(torch.uint8)


def mx8_dequantize(codes, scales, dtype=torch.float32):
    """float(code) * 2^(scale - 127) per block of 32 columns -> (n, C) in `dtype`: exact in float32 and in bfloat16.  (A code is
    decoded through the table of all 256 e4m3fn values, built on the host.)"""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2 \
            or codes.shape[0] != scales.shape[0] or codes.shape[1] != scales.shape[1] * MX8_BLOCK:
        raise DrnError("mx8_dequantize: codes (n, C) and scales (n, C / %d) must be uint8" % MX8_BLOCK)
    n, C = codes.shape
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(codes.device)
    vals = table[codes.long()].reshape(n, C // MX8_BLOCK, MX8_BLOCK)
    return torch.ldexp(vals, (scales.to(torch.int32) - 127).unsqueeze(2)).reshape(n, C).to(dtype)


def mx8_gate_weights(W, gate, D, Dp):
    """The sentence gate folded into conv0's weight and quantised to the index's format: THE DEFINITION of what
    drn_gate_quantize_weights_mx8 writes.  W: conv0's fp32 parameter (Cout, D + P, 3); gate: the level-0 gate (S, D) in fp32.
    Wg[s, tap, n, c] = gate[s, c] * W[n, c, tap] for c < D (one fp32 multiply), zero for D <= c < Dp; the result is mx8_quantize of Wg
    viewed as (S * 3 * Cout, Dp) -> (wcodes (S, 3, Cout, Dp) u8, wscales (S, 3, Cout, Dp / 32) u8), K contiguous as a B fragment
    wants it."""
    D, Dp = int(D), int(Dp)
    if W.dim() != 3 or W.shape[2] != 3 or W.shape[1] < D or gate.dim() != 2 or gate.shape[1] != D or Dp < D or Dp % MX8_BLOCK:
        raise DrnError("mx8_gate_weights: W must be (Cout, >= D, 3), gate (S, D), and Dp >= D a multiple of %d" % MX8_BLOCK)
    S, Cout = int(gate.shape[0]), int(W.shape[0])
    Wg = torch.zeros((S, 3, Cout, Dp), dtype=torch.float32, device=W.device)
    Wg[..., :D] = gate.float()[:, None, None, :] * W.detach().float()[:, :D, :].permute(2, 0, 1)[None]
    codes, scales = mx8_quantize(Wg.view(S * 3 * Cout, Dp))
    return codes.view(S, 3, Cout, Dp), scales.view(S, 3, Cout, Dp // MX8_BLOCK)


def mx8_conv0_reference(index, wcodes, wscales, Wpos, pair_q, pair_v, vids, L):
    """The oracle of drn_conv0_mx8, in float64 on the host: raw (Q, L, Cout),
      raw[p, t, n] = sum_tap sum_c dq(index)[src(p, t + tap - 1), c] * dq(w)[pair_q[p], tap, n, c]
                   + sum_tap sum_j pos[src(p, t + tap - 1), j] * Wpos[tap, n, j]
    index: anything with codes / scales / pos (None or width 0: no position part) / prop_off / pad_row as a quantised SearchIndex has
    them; Wpos (3, Cout, P): W[n, D + j, tap] rounded to the index's dtype.  src(p, u), 0 <= u < L, is drn_gate_gather_packed_q8's
    row: prop_off[v] + u while u is below video v = vids[pair_v[p]]'s proposal count (a video with more than L proposals is cut at L),
    else pad_row, as for a slot or a position out of range.  A tap at u < 0 or u >= L contributes zero (the conv's own zero padding, not
    the pad row).  No bias."""
    cpu = lambda t: t.detach().cpu()
    codes, scales, off = cpu(index.codes), cpu(index.scales), cpu(index.prop_off).long()
    z = mx8_dequantize(codes, scales).double()
    S, _, Cout, C = wcodes.shape
    w = mx8_dequantize(cpu(wcodes).reshape(S * 3 * Cout, C), cpu(wscales).reshape(S * 3 * Cout, C // MX8_BLOCK)).double().view(S, 3, Cout, C)
    pos = getattr(index, "pos", None)
    pos = None if pos is None or pos.shape[1] == 0 or Wpos is None else cpu(pos).double()
    wp = cpu(Wpos).double() if pos is not None else None
    pq, pv, vd = cpu(pair_q).long().tolist(), cpu(pair_v).long().tolist(), cpu(vids).long().tolist()
    L, Nv, pad = int(L), int(off.numel()) - 1, int(index.pad_row)
    raw = torch.zeros((len(pq), L, Cout), dtype=torch.float64)
    for p in range(len(pq)):
        v = vd[pv[p]] if 0 <= pv[p] < len(vd) else -1
        base, cnt = (int(off[v]), int(off[v + 1] - off[v])) if 0 <= v < Nv else (0, 0)
        src = torch.tensor([base + u if u < cnt else pad for u in range(L)])
        x = z[src]
        xp = pos[src] if pos is not None else None
        for tap in range(3):
            lo, hi = max(0, 1 - tap), min(L, L + 1 - tap)                 # output rows t whose tap row u = t + tap - 1 is in [0, L)
            if hi <= lo:
                continue
            u = slice(lo + tap - 1, hi + tap - 1)
            raw[p, lo:hi] += x[u] @ w[pq[p], tap].t()
            if xp is not None:
                raw[p, lo:hi] += xp[u] @ wp[tap].t()
    return raw


class SearchIndex(object):
    """names, index, nprops, D, dtype, device, nbytes and len() with FeatureStore's meaning (positions are store positions); rows,
    prop_off (device int32, the index's own copy of the store's table), pad_row (the position of the pad row), Dp (the zero-padded
    feature width the model's front runs on: 512 for D = 500 in bf16, D otherwise), P (position-embedding width).  The index holds no
    reference to the store's features (only a weak one to the store, for refresh): the store may be dropped.
    quantize: None, or "mxfp8" -- then rows is None and the table is codes (P_total + 1, Dp) u8 | scales (P_total + 1, Dp / 32) u8 |
    pos (P_total + 1, P) in dtype, the pad row quantised like any other.  resident: the tensor that says where the index lives."""

    # Rows (videos x T) one build step projects by default.  A CHOICE, not a measurement: 8192 rows of D = 4096 in bf16 are 64 MiB of
    # pooled features and as much again of projected rows per step, and a GEMM of that height fills the device.
    BUILD_ROWS = 8192

    def __init__(self):
        self.rows = self.prop_off = self.codes = self.scales = self.pos = self.quantize = None

    @property
    def resident(self):
        return self.codes if self.rows is None else self.rows

    def __len__(self):
        return len(self.names)

    ids_of = FeatureStore.ids_of

    @staticmethod
    def bytes_of(proposals, width, dtype, videos, quantize=None, P=None):
        """Device bytes of an index: the packed rows with the pad row, and prop_off (int32).  width = Dp + P.  quantize="mxfp8" needs
        P, the position columns' share of width: a row is then Dp codes, Dp / 32 scales and P elements of dtype."""
        if quantize not in QUANTIZE:
            raise DrnError("SearchIndex: quantize must be None or \"mxfp8\" (got %r)" % (quantize,))
        item = torch.empty((), dtype=dtype).element_size()
        if quantize is None:
            row = int(width) * item
        else:
            if P is None or not 0 <= int(P) <= int(width) or (int(width) - int(P)) % MX8_BLOCK:
                raise DrnError("SearchIndex: a quantised row needs P, and width - P a multiple of %d (got width %s, P %s)"
                               % (MX8_BLOCK, width, P))
            Dp = int(width) - int(P)
            row = Dp + Dp // MX8_BLOCK + int(P) * item
        return (int(proposals) + 1) * row + (int(videos) + 1) * 4

    @staticmethod
    def _stamp(model):
        ps = (model.prop_fc.weight, model.prop_fc.bias, model.position_transform.weight, model.position_transform.bias)
        return tuple((id(p), p.data_ptr(), p._version) for p in ps) + (model.compute_dtype,)

    @classmethod
    def build(cls, model, store, chunk=None, max_bytes=None, quantize=None):
        """Walk the whole store once, in store order, in chunks of `chunk` videos (one shape: the last chunk is padded with position
        -1): store.gather on device positions with T = the store's largest proposal count -> model.prepare_input(split_gate=True)
        (cast, prop_fc, position embedding), eval mode under no_grad -> the real proposals' rows copied into the packed table on the
        device, no host synchronisation.  Raises DrnError BEFORE anything is allocated when the index would exceed max_bytes.
        quantize="mxfp8": each chunk's selected rows are quantised straight into codes / scales (one drn_quantize_rows_mx8 launch per
        destination slice); max_bytes is checked against the quantised size."""
        if quantize not in QUANTIZE:
            raise DrnError("SearchIndex.build: quantize must be None or \"mxfp8\" (got %r)" % (quantize,))
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
        self.quantize = quantize
        if quantize is not None and self.Dp % MX8_BLOCK:
            raise DrnError("SearchIndex.build: quantize=%r needs a feature width that is a multiple of %d (the model's front runs on %d "
                           "columns)" % (quantize, MX8_BLOCK, self.Dp))
        self.nbytes = self.bytes_of(total, self.Dp + self.P, self.dtype, len(self.names), quantize=quantize, P=self.P)
        if max_bytes is not None and self.nbytes > max_bytes:
            raise DrnError("SearchIndex: %d videos (%d proposals x %d, %s%s) need %d bytes on the device, max_bytes is %d"
                           % (len(self.names), total, self.Dp + self.P, self.dtype, ", " + quantize if quantize else "", self.nbytes,
                              max_bytes))
        if quantize is None:
            self.rows = torch.empty((total + 1, self.Dp + self.P), dtype=self.dtype, device=self.device)
        else:
            self.codes = torch.empty((total + 1, self.Dp), dtype=torch.uint8, device=self.device)
            self.scales = torch.empty((total + 1, self.Dp // MX8_BLOCK), dtype=torch.uint8, device=self.device)
            self.pos = torch.empty((total + 1, self.P), dtype=self.dtype, device=self.device)
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
                for idx, lo, hi in ((plan[at:at + n], first, first + n),) + \
                        (((plan[-1:], self.pad_row, self.pad_row + 1),) if c == pad_chunk else ()):
                    if not idx.numel():
                        continue
                    if self.quantize is None:
                        self.rows[lo:hi, :Dp] = Z.index_select(0, idx)
                        self.rows[lo:hi, Dp:] = G0[:, Dp:].index_select(0, idx)
                    else:
                        ops.quantize_rows_mx8(Z.index_select(0, idx), self.codes[lo:hi], self.scales[lo:hi])
                        self.pos[lo:hi] = G0[:, Dp:].index_select(0, idx)
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

    def dequantized(self):
        """A plain SearchIndex holding mx8_dequantize(codes, scales) next to pos in its rows -- what this index really holds, and the
        index it answers like bit for bit.  The same names, tables and stamp: it is current for the same model."""
        if self.quantize is None:
            raise DrnError("SearchIndex.dequantized: this index is not quantised")
        plain = SearchIndex()
        for name in ("names", "index", "nprops", "D", "dtype", "device", "Dp", "P", "T", "pad_row", "prop_off", "stamp", "_chunk", "_store"):
            setattr(plain, name, getattr(self, name))
        plain.rows = torch.cat([mx8_dequantize(self.codes, self.scales, self.dtype), self.pos], dim=1)
        plain.nbytes = self.bytes_of(self.pad_row, self.Dp + self.P, self.dtype, len(self.names))
        return plain

    def check(self, model, what="SearchIndex"):
        if not self.is_current(model):
            raise DrnError("%s: the index is stale (prop_fc / position_transform changed, or it was built for another model or "
                           "compute dtype): call index.refresh(model)" % what)
