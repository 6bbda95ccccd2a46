"""A coarse table that is actually SMALL: one SIGN BIT per dimension, ranked by Hamming distance on the device.

The cheapest resident table of drn_amd.retrieve is block-scaled FP8, E + E / 32 bytes a row; a sign-bit table is E / 8 -- 64 B a row at
E = 512, 1/16 of bfloat16 -- and the standard first stage of a dual-encoder cascade: popcounts rank it, and the full-precision or FP8
table reranks the few hundred survivors (Shortlister.rerank takes up to 1024).

THE FORMAT.  codes (rows, W) int32, W = ceil(E / 32): bit e & 31 of word e >> 5 is 1 unless x[row, e] < 0 -- so +0 and -0 give 1 -- and
the bits at or past E are 0: a packed allow mask's bit convention, so pack_allow over ~(x < 0) is the quantiser on the device and
binary_quantize_reference the definition.  binary_dequantize gives the (rows, E) table of +-1 the codes stand for, binary_signs the +-1
of a query by the same rule (a row that holds an element that is not finite becomes all NaN: it lists nothing).

THE SCORE.  score[s, r] = E - 2 * popcount(code(q_s) xor codes[r]) over the E real bits = sum_e sign(q_e) * sign(x_e): an integer in
[-E, E], so every field is exact and ties are everywhere -- at E = 32 there are 33 distinct scores -- and the total order (score
descending, then position ascending, then the lowest segment) is the whole answer.  binary_shortlist_reference is the definition, in
integer arithmetic; by construction it is shortlist_reference / segment_shortlist_reference over binary_dequantize(codes) and
binary_signs(queries).

BinaryShortlister keeps such a table on the device -- built from embeddings (no reference to the wide table is kept) or taken from
codes made elsewhere -- and shortlist() / shortlist_deep() rank it through drn_shortlist_bin (csrc/retrieve_bin.hip): up to
SHORTLIST_DEEP_MAX videos a sentence under either name, plain or ragged, with allow=, out= and graph capture as Shortlister's, every
field bit for bit what dequantized().shortlist_deep(binary_signs(queries), n, allow=allow) gives.  It is a legal `coarse` of
drn_amd.search_eval.evaluate_cascade(..., deep=True).

THE ASYMMETRIC SCORE.  score[s, r] = sum_e q[s, e] * sign(x[r, e]): the query keeps its magnitudes, which cost nothing to keep, and the
table stays one bit a dimension.  It is the PLAIN shortlist over the +-1 table the codes stand for, so it has no arithmetic of its own:
binary_asym_shortlist_reference is shortlist_reference / segment_shortlist_reference over binary_dequantize(codes, E, float64), and
shortlist_asym() (drn_shortlist_bin_asym, csrc/retrieve_bin_asym.hip: the plain MFMA chain with its table operand built from the code
bits in registers) is bit for bit dequantized().shortlist_deep(queries, n, allow=allow).  asymmetric() is a view of the same table
whose shortlist() / shortlist_deep() score that way: the `coarse` of evaluate_cascade(..., deep=True) that compares the two scorings
on one resident table.

What this is NOT: there is no rank / rerank / scores / late interaction on a binary table and no binary shard of a
ShardedShortlister, and nothing here says anything about recall: that is what evaluate_cascade measures on real embeddings."""
import numpy as np
import torch

from . import ops
from ._lib import BINARY_MAX_E, SHORTLIST_DEEP_MAX, DrnError     # BINARY_MAX_E = 4096 is a CHOICE: 16 sentences' query codes in 8 KiB of LDS
from .retrieve import (SegmentShortlist, Shortlist, Shortlister, _allow_of, _allowed, _check_list_out, _check_packed_allow, _list_buffers,
                       _listed, check_segment_offsets, pack_allow_reference, segment_shortlist_reference, shortlist_reference)

BINARY_PACK_ELEMS = 1 << 26   # elements of the bool temporary one pack_allow launch of the constructor reads (64 MiB): a CHOICE, not a measurement


def binary_quantize_reference(x):
    """THE DEFINITION of the sign codes: x (rows, E), a numpy array or a tensor of any float dtype -> codes (rows, W) int32, W =
    ceil(E / 32): bit e & 31 of word e >> 5 is 1 unless x[row, e] < 0 (+0, -0 and NaN give 1), bits at or past E are 0.  A numpy array
    gives a numpy array; a tensor gives a tensor on its device (the packing itself is pack_allow_reference, on the host)."""
    if torch.is_tensor(x):
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise DrnError("binary_quantize_reference: x must be (rows, E) with rows >= 1 and E >= 1, not %s" % (tuple(x.shape),))
        return torch.from_numpy(pack_allow_reference(~(x.detach() < 0).cpu())).to(x.device)
    a = np.asarray(x)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise DrnError("binary_quantize_reference: x must be (rows, E) with rows >= 1 and E >= 1, not %s" % (a.shape,))
    return pack_allow_reference(~(a < 0))


def _check_codes(what, codes, E):
    """codes (rows, ceil(E / 32)) int32, a tensor or an array -> (the tensor, E)."""
    E = int(E)
    codes = codes if torch.is_tensor(codes) else torch.from_numpy(np.ascontiguousarray(codes))
    if E < 1 or codes.dtype != torch.int32 or codes.dim() != 2 or codes.shape[0] < 1 or int(codes.shape[1]) != ops.binary_words(E):
        raise DrnError("%s: codes must be int32 (rows, W) with rows >= 1 and W = ceil(E / 32) = %d for E = %d, not %s %s"
                       % (what, ops.binary_words(max(E, 1)), E, codes.dtype, tuple(codes.shape)))
    return codes, E


def _bits(codes, E):
    """codes (rows, W) int32 -> bool (rows, E): bit e & 31 of word e >> 5."""
    shifts = torch.arange(32, device=codes.device, dtype=torch.int64)
    return (((codes.to(torch.int64)[:, :, None] >> shifts) & 1) != 0).reshape(int(codes.shape[0]), -1)[:, :E]


def binary_dequantize(codes, E, dtype):
    """codes (rows, W) int32 -> the (rows, E) table of +-1 in dtype that they stand for (bit set: +1), on their device."""
    codes, E = _check_codes("binary_dequantize", codes, E)
    bits = _bits(codes, E)
    return torch.where(bits, torch.ones((), dtype=dtype, device=codes.device), -torch.ones((), dtype=dtype, device=codes.device)).contiguous()


def binary_signs(queries):
    """queries (S, E) floats -> +-1 in their dtype by the codes' rule (-1 where the element is < 0, else +1, +0 and -0 included); a row
    that holds an element that is not finite becomes all NaN, and so lists nothing wherever it is scored."""
    if not torch.is_tensor(queries) or queries.dim() != 2 or not queries.is_floating_point():
        raise DrnError("binary_signs: the queries must be a float tensor (S, E)")
    one = torch.ones((), dtype=queries.dtype, device=queries.device)
    signs = torch.where(queries < 0, -one, one)
    wild = ~torch.isfinite(queries).all(dim=1, keepdim=True)
    return torch.where(wild, torch.full_like(signs, float("nan")), signs).contiguous()


def _popcount32(x):
    """The set bits of the low 32 bits of each int64 element."""
    x = x & 0xffffffff
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0f0f0f0f
    return ((x * 0x01010101) & 0xffffffff) >> 24


def binary_shortlist_reference(codes, E, queries, n, offsets=None, allow=None):
    """THE DEFINITION of a binary shortlist, in integer arithmetic (usable on the CPU).  codes (rows, W) int32 sign codes over E columns,
    queries (S, E) floats: score[s, r] = E - 2 * popcount(code(q_s) xor codes[r]), code(q_s) = binary_quantize_reference(queries)[s]
    (both sides have zero pad bits: only the E real bits count).  A plain table -> shortlist_reference's Shortlist over those scores;
    with offsets (V + 1 non-decreasing integers from 0 to rows) -> segment_shortlist_reference's SegmentShortlist: a video scored by
    its best row, rows the lowest segment that reaches it, a video without rows never listed.  allow: a bool tensor (V,) or (S, V),
    exactly as in those references.  A query row that holds an element that is not finite lists nothing.  By construction this is
    shortlist_reference(binary_dequantize(codes, E, torch.float64), binary_signs(queries), n, allow) and its segment twin."""
    codes, E = _check_codes("binary_shortlist_reference", codes, E)
    if not torch.is_tensor(queries) or queries.dim() != 2 or int(queries.shape[1]) != E or queries.shape[0] < 1:
        raise DrnError("binary_shortlist_reference: the queries must be a float tensor (S, %d)" % E)
    dev = codes.device
    qcodes = binary_quantize_reference(queries).to(dev)
    R, S = int(codes.shape[0]), int(qcodes.shape[0])
    hamming = _popcount32(qcodes.to(torch.int64)[:, None, :] ^ codes.to(torch.int64)[None, :, :]).sum(dim=2)       # (S, R)
    score = (E - 2 * hamming).double()
    tame = torch.isfinite(queries).all(dim=1).to(dev)[:, None]
    if offsets is None:
        finite = tame.expand(S, R)
        if allow is not None:
            finite = finite & _allowed(allow, S, R, dev)
        ids, scores, count, _ = _listed(score, finite, int(n))
        return Shortlist(ids, scores, count)
    off = torch.as_tensor(check_segment_offsets(offsets, R), device=dev)
    V = int(off.shape[0]) - 1
    lens = off[1:] - off[:-1]
    video = torch.repeat_interleave(torch.arange(V, device=dev), lens)             # (R,) the video of a row
    segment = torch.arange(R, device=dev) - off[video]
    index = video[None, :].expand(S, R)
    best = torch.full((S, V), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(1, index, score, "amax", include_self=True)
    reaches = score == torch.gather(best, 1, index)
    rows = torch.full((S, V), R, dtype=torch.int64, device=dev).scatter_reduce(
        1, index, torch.where(reaches, segment[None, :].expand(S, R), torch.full_like(index, R)), "amin", include_self=True)
    finite = tame & (lens > 0)[None, :]
    if allow is not None:
        finite = finite & _allowed(allow, S, V, dev)
    ids, scores, count, (order, listed) = _listed(best, finite, int(n))
    segs = torch.full(tuple(ids.shape), -1, dtype=torch.int32, device=dev)
    m = int(order.shape[1])
    segs[:, :m] = torch.where(listed, torch.gather(rows, 1, order).to(torch.int32), segs[:, :m])
    return SegmentShortlist(ids, scores, count, segs)


def binary_asym_shortlist_reference(codes, E, queries, n, offsets=None, allow=None):
    """THE DEFINITION of an ASYMMETRIC binary shortlist, in float64 (usable on the CPU).  codes (rows, W) int32 sign codes over E columns,
    queries (S, E) floats, NOT binarised: score[s, r] = sum_e queries[s, e] * (+1 where bit e of codes[r] is set, else -1).  It is
    shortlist_reference(binary_dequantize(codes, E, torch.float64), queries.double(), n, allow) on a plain table and, with offsets (V +
    1 non-decreasing integers from 0 to rows), segment_shortlist_reference over the same table: a Shortlist or a SegmentShortlist under
    the total order score descending, then position ascending, then the lowest segment.  allow: a bool tensor (V,) or (S, V), exactly
    as in those references.  A query row that holds an element that is not finite lists nothing: each of its scores is a sum with an
    infinity or a NaN among its terms, so none is finite.  The refusals are binary_shortlist_reference's."""
    codes, E = _check_codes("binary_asym_shortlist_reference", codes, E)
    if not torch.is_tensor(queries) or queries.dim() != 2 or int(queries.shape[1]) != E or queries.shape[0] < 1:
        raise DrnError("binary_asym_shortlist_reference: the queries must be a float tensor (S, %d)" % E)
    wide = binary_dequantize(codes, E, torch.float64)
    q = queries.double().to(codes.device)
    if offsets is None:
        return shortlist_reference(wide, q, n, allow)
    return segment_shortlist_reference(wide, offsets, q, n, allow)


class BinaryShortlister(object):
    """BinaryShortlister(embeddings, names=None, offsets=None): a table of SIGN CODES over the rows of `embeddings` -- a contiguous CUDA
    tensor (rows, E), bfloat16 or float32, finite, rows >= 1 and 1 <= E <= BINARY_MAX_E = 4096 (a CHOICE: 16 sentences' query codes
    are 8 KiB of LDS) -- rows * 4 * ceil(E / 32) bytes.  The codes are made on the device by pack_allow over ~(embeddings < 0), in row
    chunks of at most BINARY_PACK_ELEMS elements so the bool temporary stays bounded, and equal binary_quantize_reference(embeddings)
    byte for byte; NO reference to `embeddings` is kept.  names, offsets (a ragged table: video v owns the rows offsets[v] ..
    offsets[v + 1] - 1), their host-side checks, the block plan and the ONE synchronise are Shortlister's.  from_codes takes tables
    made elsewhere.

    Attributes a caller may rely on: codes (rows, W) int32; E; dtype (of the queries shortlist() takes: the embeddings'); device; names;
    offsets and plan on a ragged table; nbytes == bytes_of(rows, E)."""

    _seg = _off_host = offsets = plan = None             # (what a table of one row per video has)
    _init_table, _init_segments = Shortlister._init_table, Shortlister._init_segments   # (names, offsets, the plan, the one synchronise)
    _nblocks, _workspace, _all_allowed = Shortlister._nblocks, Shortlister._workspace, Shortlister._all_allowed
    _check_queries = Shortlister._check_queries
    __len__, check = Shortlister.__len__, Shortlister.check

    def __init__(self, embeddings, names=None, offsets=None):
        what = "BinaryShortlister"
        if not torch.is_tensor(embeddings) or not embeddings.is_cuda:
            raise DrnError("%s: the embeddings must be a tensor on the GPU; there is no CPU fallback" % what)
        if embeddings.dtype not in (torch.bfloat16, torch.float32):
            raise DrnError("%s: the embeddings must be bfloat16 or float32, not %s" % (what, embeddings.dtype))
        if embeddings.dim() != 2 or embeddings.shape[0] < 1 or embeddings.shape[1] < 1 or not embeddings.is_contiguous():
            raise DrnError("%s: the embeddings must be a contiguous (V, E) tensor with V >= 1 and E >= 1, not %s"
                           % (what, tuple(embeddings.shape)))
        rows, E = (int(x) for x in embeddings.shape)
        if E > BINARY_MAX_E:
            raise DrnError("%s: E = %d outside [1, %d] (a choice: 16 sentences' query codes are kept in 8 KiB of LDS)" % (what, E, BINARY_MAX_E))
        self.E, self.dtype = E, embeddings.dtype
        self.codes = embeddings.new_empty((rows, ops.binary_words(E)), dtype=torch.int32)
        self._init_table(rows, embeddings.device, names, offsets, lambda: torch.isfinite(embeddings).all(),
                         "the embeddings hold values that are not finite")
        step = max(1, BINARY_PACK_ELEMS // E)
        for a in range(0, rows, step):
            ops.pack_allow(~(embeddings[a:a + step] < 0), self.codes[a:a + step])

    @classmethod
    def from_codes(cls, codes, E, dtype, names=None, offsets=None):
        """A BinaryShortlister on codes the caller made: a contiguous CUDA tensor (rows, ceil(E / 32)) int32, kept by reference, 1 <= E
        <= BINARY_MAX_E; dtype (torch.bfloat16 or torch.float32) is that of the queries.  A wrong shape, dtype or device is refused
        before any launch; a set bit at or past E is refused in the ONE synchronise that also serves the offsets.  names and offsets
        as in the constructor."""
        what = "BinaryShortlister.from_codes"
        if not torch.is_tensor(codes) or not codes.is_cuda:
            raise DrnError("%s: the codes must be a tensor on the GPU; there is no CPU fallback" % what)
        if codes.dtype != torch.int32:
            raise DrnError("%s: the codes must be torch.int32 words, not %s" % (what, codes.dtype))
        E = int(E)
        if not 1 <= E <= BINARY_MAX_E:
            raise DrnError("%s: E = %d outside [1, %d] (a choice: 16 sentences' query codes are kept in 8 KiB of LDS)" % (what, E, BINARY_MAX_E))
        W = ops.binary_words(E)
        if codes.dim() != 2 or codes.shape[0] < 1 or int(codes.shape[1]) != W or not codes.is_contiguous():
            raise DrnError("%s: the codes must be a contiguous (rows, %d) tensor with rows >= 1, ceil(E / 32) words a row for E = %d, not %s"
                           % (what, W, E, tuple(codes.shape)))
        if dtype not in (torch.bfloat16, torch.float32):
            raise DrnError("%s: dtype (of the queries) must be bfloat16 or float32, not %s" % (what, dtype))

        def sound():
            if E % 32 == 0:
                return torch.ones((), dtype=torch.bool, device=codes.device)
            return ((codes[:, W - 1] >> (E % 32)) == 0).all()         # (an arithmetic shift: a set bit 31 leaves -1, not 0)
        self = cls.__new__(cls)
        self.E, self.dtype, self.codes = E, dtype, codes
        self._init_table(int(codes.shape[0]), codes.device, names, offsets, sound, "the codes have a set bit at or past E = %d" % E)
        return self

    def _table(self):
        return self.codes

    @property
    def device(self):
        return self.codes.device

    @staticmethod
    def bytes_of(rows, E):
        """The bytes of a table of `rows` rows of sign codes over E columns: rows * 4 * ceil(E / 32) (64 a row at E = 512)."""
        return int(rows) * 4 * ops.binary_words(E)

    @property
    def nbytes(self):
        """The bytes of the codes this object holds (the offsets, the plan and the workspaces are not counted)."""
        return self.codes.numel() * self.codes.element_size()

    def dequantized(self):
        """A plain Shortlister over binary_dequantize(codes, E, dtype) with the same names and offsets: what the codes stand for, and
        the oracle shortlist() answers bit for bit like when it is given binary_signs(queries)."""
        return Shortlister(binary_dequantize(self.codes, self.E, self.dtype), names=self.names,
                           offsets=None if self._seg is None else self._seg[0])

    def allow_of(self, keep=None, drop=None):
        """Shortlister.allow_of: HOST names or store positions -> a packed mask (W,) int32 on the table's device."""
        return _allow_of("BinaryShortlister.allow_of", self.names, len(self), self.codes.device, keep, drop)

    def shortlist(self, queries, n, out=None, allow=None):
        """queries (S, E) on the device in self.dtype -- FLOATS: the launch binarises them by the codes' rule -- and 1 <= n <=
        SHORTLIST_DEEP_MAX -> Shortlist, or SegmentShortlist on a ragged table, on the device (binary_shortlist_reference defines it):
        ids, scores (the integers E - 2 * Hamming distance, as float32), n and rows, padded with -1 / 0 / -1.  A query row that holds
        an element that is not finite lists nothing.  out: the buffers of the result, written in place, every element, and returned.
        allow: a packed mask (W,) or (S, W) as Shortlister.shortlist takes it, over videos; its contents may change between replays
        of a captured graph.  No host synchronisation, and the call can be captured once the (S, n) workspace is warm.  Every field
        is bit for bit dequantized().shortlist_deep(binary_signs(queries), n, allow=allow).  One entry (drn_shortlist_bin): two
        launches, three on a ragged table.  shortlist_deep is the same method under the name evaluate_cascade(deep=True) calls."""
        return self._shortlist("BinaryShortlister.shortlist", ops.shortlist_bin, queries, n, out, allow)

    shortlist_deep = shortlist

    def shortlist_asym(self, queries, n, out=None, allow=None):
        """The ASYMMETRIC shortlist: queries (S, E) on the device in self.dtype, scored AS THEY ARE against the +-1 the codes stand for
        (score[s, r] = sum_e q[s, e] * sign(x[r, e]); binary_asym_shortlist_reference defines it), and 1 <= n <= SHORTLIST_DEEP_MAX ->
        Shortlist, or SegmentShortlist on a ragged table, on the device.  The checks, out=, the packed allow=, the workspaces (kept
        per (S, n) and shared with shortlist()), the result types and the -1 / 0 / -1 padding are shortlist()'s.  A query row that
        holds an element that is not finite lists nothing.  No host synchronisation, and the call can be captured once the (S, n)
        workspace is warm; the mask's contents may change between replays.  Every field is bit for bit
        dequantized().shortlist_deep(queries, n, allow=allow).  One entry (drn_shortlist_bin_asym): two launches, three on a ragged
        table."""
        return self._shortlist("BinaryShortlister.shortlist_asym", ops.shortlist_bin_asym, queries, n, out, allow)

    def _shortlist(self, what, entry, queries, n, out, allow):
        """shortlist and shortlist_asym: the refusals, the buffers, the workspace and the ONE call of `entry` (an ops wrapper)."""
        S, n = self._check_queries(what, queries, n=n, on_table=False, cap=SHORTLIST_DEEP_MAX)
        seg = self._seg
        if out is not None:
            _check_list_out(what, out, S, n, rows=seg is not None)
        if allow is not None:
            _check_packed_allow(allow, S, len(self), self.codes.device)
        else:
            allow = self._all_allowed()
        if out is None:
            out = _list_buffers(self.codes.device, S, n, rows=seg is not None)
        if seg is None:
            ws = self._workspace((S, n), lambda: ops.shortlist_ws_keys(len(self), S, n))
            entry(self.codes, self.E, queries.contiguous(), (), n, ws, tuple(out), allow)
            return Shortlist(*out)
        ws = self._workspace((S, n), lambda: ops.shortlist_segments_ws_keys(self._nblocks(), S, n))
        entry(self.codes, self.E, queries.contiguous(), seg, n, ws, tuple(out), allow)
        return SegmentShortlist(*out)

    def asymmetric(self):
        """A light VIEW of this table whose shortlist() / shortlist_deep() are shortlist_asym(): the same codes, names, offsets and plan,
        nothing copied.  It is a legal `coarse` of drn_amd.search_eval.evaluate_cascade(..., deep=True), so the two scorings can be
        compared on one resident table."""
        return AsymmetricBinaryView(self)


class AsymmetricBinaryView(object):
    """BinaryShortlister.asymmetric(): the table `base` under ASYMMETRIC scoring.  shortlist and shortlist_deep are base.shortlist_asym;
    names, device, dtype, E, codes, offsets, plan, nbytes, len(), check, allow_of and dequantized are base's own.  Nothing is copied and
    no workspace is kept here."""

    def __init__(self, base):
        if not isinstance(base, BinaryShortlister):
            raise DrnError("AsymmetricBinaryView: the table must be a BinaryShortlister")
        self.base = base

    names = property(lambda self: self.base.names)
    device = property(lambda self: self.base.device)
    dtype = property(lambda self: self.base.dtype)
    E = property(lambda self: self.base.E)
    codes = property(lambda self: self.base.codes)
    offsets = property(lambda self: self.base.offsets)
    plan = property(lambda self: self.base.plan)
    nbytes = property(lambda self: self.base.nbytes)

    def __len__(self):
        return len(self.base)

    def check(self, store):
        return self.base.check(store)

    def allow_of(self, keep=None, drop=None):
        return self.base.allow_of(keep=keep, drop=drop)

    def dequantized(self):
        """base.dequantized(): the oracle shortlist() answers bit for bit like, given the queries as they are."""
        return self.base.dequantized()

    def shortlist(self, queries, n, out=None, allow=None):
        """base.shortlist_asym(queries, n, out=out, allow=allow)."""
        return self.base.shortlist_asym(queries, n, out=out, allow=allow)

    shortlist_deep = shortlist
