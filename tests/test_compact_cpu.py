"""Compacting a sharded corpus, the host side: compact_reference on CPU tensors (positions, order, names, ragged offsets, the four
format pairs), the equivalence that justifies the feature on the references alone (the compacted rows answer as the concatenated
rows do under allow=keep, ids mapped through positions), the two C entries drn_compact_plan and drn_compact_rows at ABI 9 with their
argument checks, every refusal of ShardedShortlister.compact that needs no GPU, and the compiler's notes on the kernels.
tests/test_compact_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_late_shortlist_cpu import Resident, _no_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN, ROWS = "drn_compact_plan", "drn_compact_rows"


def stand_in(rows, offsets=None, quantize=None, dtype=None, names=None, device=None):
    """A shard whose constructor was not run, on any device: rows is a plain (R, E) tensor, or with quantize="mxfp8" the pair (codes,
    scales) -- or a plain tensor to be quantised by the definition."""
    from drn_amd import Shortlister, plan_segment_blocks
    from drn_amd.index import mx8_quantize
    sl = Shortlister.__new__(Shortlister)
    sl.names, sl._ws, sl._seg = names, {}, None
    put = (lambda t: t) if device is None else (lambda t: t.to(device))
    if quantize is None:
        sl.embeddings = put(rows).contiguous()
    else:
        codes, scales = rows if isinstance(rows, tuple) else mx8_quantize(rows)
        sl.embeddings, sl.quantize, sl._dtype = None, quantize, dtype if dtype is not None else rows.dtype
        sl.codes, sl.scales = put(codes).contiguous(), put(scales).contiguous()
    if offsets is not None:
        plan = plan_segment_blocks(offsets)
        sl.plan = plan
        sl._seg = tuple(put(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))) for a in (np.asarray(offsets), plan.blk_vid, plan.vid_blk))
        sl.offsets = sl._seg[0]
    return sl


def int_rows(n, E, dtype=torch.float32, seed=0):
    """Integer-valued rows in [-4, 4]: exact in bfloat16, in e4m3fn under any block scale the quantiser picks, and in every sum."""
    return torch.randint(-4, 5, (n, E), generator=torch.Generator().manual_seed(seed)).to(dtype)


def positions_by_hand(mask):
    out, at = [], 0
    for bit in mask.tolist():
        out.append(at if bit else -1)
        at += int(bit)
    return torch.tensor(out, dtype=torch.int32)


SIZES = (5, 70, 33)            # bases 0, 5, 75, 108: no base after 0 is a multiple of 32


def masks(V, sizes=SIZES, seed=1):
    """The masks of the plain cases: all kept, first and last dropped, shard 0 dropped, the middle shard dropped, one survivor."""
    rnd = torch.rand(V, generator=torch.Generator().manual_seed(seed)) < 0.7
    ends = rnd.clone()
    ends[0] = ends[V - 1] = False
    first = torch.ones(V, dtype=torch.bool)
    first[:sizes[0]] = False
    middle = rnd.clone()
    middle[sizes[0]:sizes[0] + sizes[1]] = False
    one = torch.zeros(V, dtype=torch.bool)
    one[sizes[0] + sizes[1] - 1] = True
    return {"all": torch.ones(V, dtype=torch.bool), "ends": ends, "shard0": first, "middle": middle, "one": one}


# -- compact_reference on CPU tensors -----------------------------------------------------------------------------------------------------

def test_the_reference_keeps_order_positions_and_names_on_plain_shards():
    from drn_amd import Compacted, compact_reference, pack_allow_reference
    V = sum(SIZES)
    whole = int_rows(V, 8)
    names = ["v%d" % v for v in range(V)]
    cuts = np.cumsum((0,) + SIZES)
    shards = [stand_in(whole[a:b], names=names[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for what, mask in masks(V).items():
        got = compact_reference(shards, keep=mask)
        assert isinstance(got, Compacted) and got.kept == int(mask.sum()) == len(got.table), what
        assert got.positions.dtype == torch.int32 and torch.equal(got.positions, positions_by_hand(mask)), what
        assert got.table.quantize is None and torch.equal(got.table.embeddings, whole[mask]), what
        assert got.table.names == [n for n, bit in zip(names, mask.tolist()) if bit], what
        packed = compact_reference(shards, keep=torch.from_numpy(pack_allow_reference(mask)))      # the packed words mean the same
        assert torch.equal(packed.positions, got.positions) and torch.equal(packed.table.embeddings, got.table.embeddings), what
    everything = compact_reference(shards)
    assert everything.kept == V and torch.equal(everything.positions, torch.arange(V, dtype=torch.int32))
    assert torch.equal(everything.table.embeddings, whole) and everything.table.names == names
    assert everything.table.embeddings.data_ptr() != whole.data_ptr()
    # names only where every shard has them
    assert compact_reference([shards[0], stand_in(whole[5:75])], keep=None).table.names is None


RAGGED = ([0, 0, 1, 71, 71, 74], [0, 0, 0, 0], [0, 3, 3, 5, 6])        # videos of 0, 1 and 70 rows; a shard whose videos own no rows


def ragged_case(dtype=torch.float32):
    rows = [int_rows(off[-1], 8, dtype, seed=k) for k, off in enumerate(RAGGED)]
    names = [["s%d_%d" % (k, v) for v in range(len(off) - 1)] for k, off in enumerate(RAGGED)]
    V = sum(len(off) - 1 for off in RAGGED)
    return rows, names, V


def ragged_masks(V):
    rnd = torch.tensor([True, False, True, True, False, True, True, False, True, True, False, True])      # (0-row, 1-row, 70-row videos kept and dropped)
    flip = ~rnd
    flip[3] = False                                                                                        # the 70-row video dropped too
    return {"all": torch.ones(V, dtype=torch.bool), "mix": rnd, "flip": flip}


def test_the_reference_makes_new_offsets_on_ragged_shards():
    from drn_amd import compact_reference, plan_segment_blocks
    rows, names, V = ragged_case()
    assert V == 12
    shards = [stand_in(r if len(r) else torch.zeros(0, 8), offsets=off, names=n) for r, off, n in zip(rows, RAGGED, names)]
    for what, mask in ragged_masks(V).items():
        got = compact_reference(shards, keep=mask)
        want_rows, want_off, v = [], [0], 0
        for r, off in zip(rows, RAGGED):
            for i in range(len(off) - 1):
                if mask[v]:
                    want_rows.append(r[off[i]:off[i + 1]])
                    want_off.append(want_off[-1] + off[i + 1] - off[i])
                v += 1
        assert torch.equal(got.table.embeddings, torch.cat(want_rows)), what
        assert got.table.offsets.dtype == torch.int32 and got.table.offsets.tolist() == want_off, what
        assert len(got.table) == got.kept == int(mask.sum()) and torch.equal(got.positions, positions_by_hand(mask)), what
        plan = plan_segment_blocks(want_off)
        assert np.array_equal(got.table.plan.blk_vid, plan.blk_vid) and np.array_equal(got.table.plan.vid_blk, plan.vid_blk), what
        assert got.table.names == [n for n, bit in zip(sum(names, []), mask.tolist()) if bit], what
    # a kept video without rows stays one: "mix" keeps video 0 (no rows) and the whole middle shard's survivors own none
    got = compact_reference(shards, keep=ragged_masks(V)["mix"])
    assert got.table.offsets.tolist()[:2] == [0, 0]


def test_the_reference_refuses_an_empty_table():
    from drn_amd import _lib, compact_reference
    rows, names, V = ragged_case()
    shards = [stand_in(r if len(r) else torch.zeros(0, 8), offsets=off) for r, off in zip(rows, RAGGED)]
    with pytest.raises(_lib.DrnError, match="keeps no video"):
        compact_reference(shards, keep=torch.zeros(V, dtype=torch.bool))
    norows = torch.zeros(V, dtype=torch.bool)
    norows[0] = norows[5] = norows[6] = True
    with pytest.raises(_lib.DrnError, match="3 videos the mask keeps own no row"):
        compact_reference(shards, keep=norows)
    with pytest.raises(_lib.DrnError, match="keep must be a bool mask"):
        compact_reference(shards, keep=torch.zeros(V + 1, dtype=torch.bool))


def test_the_four_format_pairs_of_the_reference():
    from drn_amd import _lib, compact_reference
    from drn_amd.index import mx8_dequantize, mx8_quantize
    g = torch.Generator().manual_seed(5)
    plain = (torch.randn(9, 64, generator=g) * 3).to(torch.bfloat16)
    # an FP8 shard mx8_quantize would never have written: random codes (no NaN code) under arbitrary legal scale bytes
    codes = torch.randint(0, 256, (7, 64), generator=g).to(torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x11
    codes[0, :32] = 0x08                                                    # a block of 2^-6s: the quantiser would have scaled it up to 448
    scales = torch.randint(17, 255, (7, 2), generator=g).to(torch.uint8)
    scales[0, 0] = 130
    again = mx8_quantize(mx8_dequantize(codes, scales, torch.float32))
    assert not torch.equal(again[0][0, :32], codes[0, :32]) and int(again[1][0, 0]) != 130      # requantising WOULD change the bytes
    shards = [stand_in(plain), stand_in((codes, scales), quantize="mxfp8", dtype=torch.bfloat16)]
    mask = torch.rand(16, generator=g) < 0.6
    mask[9] = True                                                          # (the row whose requantisation differs survives)
    a, b = mask[:9], mask[9:]
    # -> plain
    got = compact_reference(shards, keep=mask, quantize=None).table
    assert got.quantize is None and got.embeddings.dtype == torch.bfloat16
    assert torch.equal(got.embeddings[:int(a.sum())].view(torch.int16), plain[a].view(torch.int16))
    assert torch.equal(got.embeddings[int(a.sum()):].view(torch.int16), mx8_dequantize(codes[b], scales[b], torch.bfloat16).view(torch.int16))
    # -> mxfp8
    got = compact_reference(shards, keep=mask, quantize="mxfp8").table
    assert got.quantize == "mxfp8" and got.dtype == torch.bfloat16 and got.embeddings is None
    qc, qs = mx8_quantize(plain[a])
    assert torch.equal(got.codes[:int(a.sum())], qc) and torch.equal(got.scales[:int(a.sum())], qs)
    assert torch.equal(got.codes[int(a.sum()):], codes[b]) and torch.equal(got.scales[int(a.sum()):], scales[b])      # a byte copy
    # "same": the common format, and never a silent choice between two
    with pytest.raises(_lib.DrnError, match='quantize="same" needs shards of one format and these are mixed'):
        compact_reference(shards, keep=mask)
    same = compact_reference(shards[1:], keep=b).table
    assert same.quantize == "mxfp8" and torch.equal(same.codes, codes[b]) and torch.equal(same.scales, scales[b])
    assert compact_reference(shards[:1], keep=a).table.quantize is None
    with pytest.raises(_lib.DrnError, match="quantize must be \"same\" or one of"):
        compact_reference(shards, quantize="fp4")
    with pytest.raises(_lib.DrnError, match="needs E to be a multiple of 32, not E = 40"):
        compact_reference([stand_in(int_rows(3, 40))], quantize="mxfp8")


# -- the equivalence, on the references alone -----------------------------------------------------------------------------------------

def mapped(ids, positions):
    """Corpus positions -> the compacted table's, -1 staying -1."""
    return torch.where(ids >= 0, positions.to(ids.device)[ids.clamp(min=0).long()], torch.full_like(ids, -1))


def twin_corpus(dtype=torch.float32):
    """Three plain parts of 5, 70 and 33 videos with twins on both sides of each cut and of a dropped video; the middle part becomes FP8."""
    V = sum(SIZES)
    whole = int_rows(V, 32, dtype, seed=7)
    for a, b in ((4, 5), (74, 75), (3, 5), (40, 42), (76, 4)):             # 4 | 5 and 74 | 75 straddle the cuts; 41 is dropped between 40 and 42
        whole[b] = whole[a]
    mask = torch.rand(V, generator=torch.Generator().manual_seed(9)) < 0.75
    for v in (3, 4, 5, 40, 42, 74, 75, 76):
        mask[v] = True
    mask[41] = mask[0] = False
    return whole, mask


def test_the_compacted_rows_answer_as_the_masked_corpus_does_on_the_references():
    from drn_amd import compact_reference, shortlist_reference
    whole, mask = twin_corpus()
    cuts = np.cumsum((0,) + SIZES)
    shards = [stand_in(whole[a:b], quantize="mxfp8" if k == 1 else None) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    got = compact_reference(shards, keep=mask, quantize=None)
    assert torch.equal(got.table.embeddings, whole[mask])                    # (integers survive the FP8 shard exactly)
    q = int_rows(6, 32, seed=11)
    for n in (1, 7, 128):
        want = shortlist_reference(whole, q, n, allow=mask)
        have = shortlist_reference(got.table.embeddings, q, n)
        assert torch.equal(have.ids, mapped(want.ids, got.positions)) and torch.equal(have.scores, want.scores) and torch.equal(have.n, want.n), n
    wide = shortlist_reference(whole, q, 128, allow=mask)
    assert bool(((wide.scores[:, 1:] == wide.scores[:, :-1]) & (wide.ids[:, 1:] >= 0)).any())        # the lists hold ties


def test_the_compacted_ragged_rows_answer_as_the_masked_corpus_does_on_the_references():
    from drn_amd import compact_reference, late_shortlist_reference, segment_shortlist_reference
    offs = ([0, 2, 2, 5, 6], [0, 1, 4, 4, 7, 9], [0, 3, 4])
    rows = [int_rows(off[-1], 32, seed=20 + k) for k, off in enumerate(offs)]
    rows[1][0] = rows[0][5]                                                 # twins across the first cut (videos 3 | 4) ...
    rows[2][0] = rows[1][8]                                                 # ... and the second (videos 8 | 9)
    rows[1][4] = rows[1][1]                                                 # video 5 and video 7 tie, video 6 (no rows) between them
    mask = torch.tensor([True, True, False, True, True, True, True, True, False, True, True])
    shards = [stand_in(r, offsets=off, quantize="mxfp8" if k == 0 else None) for k, (r, off) in enumerate(zip(rows, offs))]
    got = compact_reference(shards, keep=mask, quantize=None)
    whole = torch.cat(rows)
    whole_off = np.concatenate([[0]] + [np.asarray(off[1:]) + base for off, base in zip(offs, np.cumsum([0] + [o[-1] for o in offs[:-1]]))]).tolist()
    new_off = got.table.offsets.tolist()
    q = int_rows(4, 32, seed=31)
    for n in (1, 4, 16):
        want = segment_shortlist_reference(whole, whole_off, q, n, allow=mask)
        have = segment_shortlist_reference(got.table.embeddings, new_off, q, n)
        for f in ("scores", "n", "rows"):
            assert torch.equal(getattr(have, f), getattr(want, f)), (n, f)
        assert torch.equal(have.ids, mapped(want.ids, got.positions)), n
    ql = torch.stack([int_rows(3, 32, seed=40 + s) for s in range(4)])
    lengths = torch.tensor([3, 1, 0, 2])
    for n in (2, 16):
        want = late_shortlist_reference(whole, whole_off, ql, lengths, n, allow=mask)
        have = late_shortlist_reference(got.table.embeddings, new_off, ql, lengths, n)
        assert torch.equal(have.ids, mapped(want.ids, got.positions)) and torch.equal(have.scores, want.scores) and torch.equal(have.n, want.n), n


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_two_compact_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name, count in ((PLAN, 10), (ROWS, 17)):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
    for public in ("Compacted", "compact_reference"):
        assert hasattr(drn_amd, public), public
    assert callable(drn_amd.ShardedShortlister.compact) and callable(ops.compact_plan) and callable(ops.compact_rows)
    assert drn_amd.Compacted._fields == ("table", "positions", "kept")
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_compact.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["compact_plan_kernel", "compact_rows_kernel"]
    hdr = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert re.search(r"#define DRN_COMPACT_PLAIN\s+0\b", hdr) and re.search(r"#define DRN_COMPACT_MX8\s+1\b", hdr)


def test_the_two_compact_entries_check_their_arguments_before_anything_is_launched():
    lib = built_lib()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
    err = lambda: lib.drn_last_error()

    # keep offsets | carry positions new_offsets
    def plan(V=70, k=1, K=3, cap=109, ptrs=(p, p, p, p, p)):
        return lib.drn_compact_plan(ptrs[0], ptrs[1], V, k, K, cap, ptrs[2], ptrs[3], ptrs[4], None)
    for i in (2, 3):
        assert plan(ptrs=[None if j == i else p for j in range(5)]) != 0 and b"null pointer" in err(), i
    for i in (1, 4):                                                          # offsets on one side only
        assert plan(ptrs=[None if j == i else p for j in range(5)]) != 0 and b"must both be given" in err(), i
    for K in (0, -1, 65):
        assert plan(K=K) != 0 and b"shards outside [1, 64]" in err(), K
    for k in (-1, 3):
        assert plan(k=k) != 0 and b"outside [0, 3)" in err(), k
    for V in (0, -4):
        assert plan(V=V) != 0 and b"bad args" in err(), V
    assert plan(cap=1) != 0 and b"below 2" in err()
    for i in range(5):
        assert plan(ptrs=[odd if j == i else p for j in range(5)]) != 0 and b"4-byte aligned" in err(), i

    PLAIN, MX8, F32, BF16 = 0, 1, 0, 1
    # src src_scales src_offsets positions dst_offsets | dst dst_scales
    def rows(ptrs=None, V=5, src_rows=5, E=64, sf=PLAIN, df=PLAIN, dtype=BF16, dst_videos=3, row0=0, dst_rows=3):
        a = [p, None, None, p, None, p, None] if ptrs is None else ptrs
        return lib.drn_compact_rows(a[0], a[1], a[2], a[3], a[4], V, src_rows, E, sf, df, dtype, dst_videos, row0, dst_rows, a[5], a[6], None)
    for i in (0, 3, 5):
        assert rows(ptrs=[None if j == i else x for j, x in enumerate([p, None, None, p, None, p, None])]) != 0 and b"null pointer" in err(), i
    for sf, df in ((2, 0), (0, -1), (7, 7)):
        assert rows(sf=sf, df=df) != 0 and b"each must be DRN_COMPACT_PLAIN (0) or DRN_COMPACT_MX8 (1)" in err(), (sf, df)
    assert rows(ptrs=[p, None, None, p, None, p, p], df=MX8) != 0 and b"plain -> mxfp8 is not taken here" in err()
    assert rows(sf=MX8) != 0 and b"scale bytes must be given exactly beside" in err()                      # an FP8 source without its scales
    assert rows(ptrs=[p, p, None, p, None, p, None]) != 0 and b"scale bytes must be given exactly beside" in err()      # scales beside a plain one
    assert rows(ptrs=[p, p, None, p, None, p, None], sf=MX8, df=MX8) != 0 and b"scale bytes must be given exactly beside" in err()
    for one in (2, 4):
        assert rows(ptrs=[p if j == one else x for j, x in enumerate([p, None, None, p, None, p, None])], src_rows=9) != 0 \
            and b"must both be given" in err(), one
    for kw in (dict(V=0, src_rows=0), dict(E=0), dict(src_rows=0)):
        assert rows(**kw) != 0 and b"bad args" in err(), kw
    assert rows(src_rows=6) != 0 and b"one row a video has src_rows == V" in err()
    for kw in (dict(dst_videos=0), dict(row0=-1), dict(dst_rows=0)):
        assert rows(**kw) != 0 and b"bad destination" in err(), kw
    assert rows(dtype=2) != 0 and b"bad dtype" in err()
    for E in (33, 40, 16):
        assert rows(ptrs=[p, p, None, p, None, p, None], sf=MX8, E=E) != 0 and b"needs E to be a multiple of 32" in err(), E
        assert rows(ptrs=[p, p, None, p, None, p, p], sf=MX8, df=MX8, E=E) != 0 and b"needs E to be a multiple of 32" in err(), E
    ragged = [p, None, p, p, p, p, None]
    for i in (2, 3, 4):
        assert rows(ptrs=[odd if j == i else x for j, x in enumerate(ragged)], src_rows=9) != 0 and b"must be 4-byte aligned" in err(), i
    for i in (0, 5):
        assert rows(ptrs=[odd if j == i else x for j, x in enumerate(ragged)], src_rows=9, dtype=F32) != 0 and b"aligned to its element size" in err(), i


# -- refusals, before the library is reached ---------------------------------------------------------------------------------------------

def test_compact_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import ShardedShortlister, _lib
    _no_library(monkeypatch)
    res = lambda t: t.as_subclass(Resident)
    plain = stand_in(res(torch.zeros(40, 64, dtype=torch.bfloat16)))
    fp8 = stand_in((res(torch.zeros(30, 64, dtype=torch.uint8)), res(torch.zeros(30, 2, dtype=torch.uint8))), quantize="mxfp8", dtype=torch.bfloat16)
    sh = ShardedShortlister([plain, fp8])                                      # V = 70: W = 3
    words = lambda *shape, dtype=torch.int32: res(torch.zeros(*shape, dtype=dtype))
    with pytest.raises(_lib.DrnError, match='quantize="same" needs shards of one format and these are mixed .*pass quantize=None'):
        sh.compact(words(3))
    with pytest.raises(_lib.DrnError, match="quantize must be \"same\" or one of"):
        sh.compact(words(3), quantize="int8")
    odd = ShardedShortlister([stand_in(res(torch.zeros(4, 40, dtype=torch.bfloat16)))])
    with pytest.raises(_lib.DrnError, match="quantize='mxfp8' needs E to be a multiple of 32, not E = 40"):
        odd.compact(quantize="mxfp8")
    with pytest.raises(_lib.DrnError, match=r"per-sentence mask \(2, 3\); a compaction takes ONE mask \(3,\)"):
        sh.compact(words(2, 3), quantize=None)
    for bad in (words(4), words(2), words(0)):
        with pytest.raises(_lib.DrnError, match=r"keep must be a contiguous \(3,\) tensor, ceil\(V / 32\) words for V = 70 videos"):
            sh.compact(bad, quantize=None)
    for bad in (words(3, dtype=torch.int64), words(70, dtype=torch.bool), [1, 2, 3]):
        with pytest.raises(_lib.DrnError, match="keep must be a packed mask, a torch.int32 tensor"):
            sh.compact(bad, quantize=None)
    with pytest.raises(_lib.DrnError, match="keep must be on the shards' device"):
        sh.compact(torch.zeros(3, dtype=torch.int32), quantize=None)          # (a host tensor)
    with pytest.raises(_lib.DrnError, match="stage_elems = 0 below 1"):
        sh.compact(words(3), quantize="mxfp8", stage_elems=0)
    # a table that is not on a GPU can be asked for its reference, never for a compaction
    host = ShardedShortlister([stand_in(torch.zeros(4, 32))])
    with pytest.raises(_lib.DrnError, match="the shards must be on the GPU; there is no CPU fallback"):
        host.compact()


def test_the_compact_wrappers_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops
    _no_library(monkeypatch)
    res = lambda t: t.as_subclass(Resident)
    i32 = lambda *shape: res(torch.zeros(*shape, dtype=torch.int32))
    with pytest.raises(_lib.DrnError, match=r"carry must be a contiguous \(K \+ 1, 2\)"):
        ops.compact_plan(None, None, 0, i32(3), i32(5))
    with pytest.raises(_lib.DrnError, match=r"shard k = 2 outside \[0, 2\)"):
        ops.compact_plan(None, None, 2, i32(3, 2), i32(5))
    with pytest.raises(_lib.DrnError, match=r"keep must be a contiguous \(3,\)"):
        ops.compact_plan(i32(2), None, 0, i32(3, 2), i32(70))
    with pytest.raises(_lib.DrnError, match="offsets and new_offsets must both be given"):
        ops.compact_plan(None, i32(6), 0, i32(3, 2), i32(5))
    with pytest.raises(_lib.DrnError, match=r"offsets must be a contiguous \(6,\)"):
        ops.compact_plan(None, i32(5), 0, i32(3, 2), i32(5), i32(9))
    bf = lambda *shape: res(torch.zeros(*shape, dtype=torch.bfloat16))
    u8 = lambda *shape: res(torch.zeros(*shape, dtype=torch.uint8))
    with pytest.raises(_lib.DrnError, match="plain -> mxfp8 is not taken here"):
        ops.compact_rows(bf(5, 64), None, i32(5), None, 3, (u8(3, 64), u8(3, 2)))
    with pytest.raises(_lib.DrnError, match="src has E = 64 columns, dst 32"):
        ops.compact_rows(bf(5, 64), None, i32(5), None, 3, bf(3, 32))
    with pytest.raises(_lib.DrnError, match="src is torch.bfloat16, dst torch.float32"):
        ops.compact_rows(bf(5, 64), None, i32(5), None, 3, res(torch.zeros(3, 64)))
    with pytest.raises(_lib.DrnError, match="dtype .of the queries. must be float32 or bfloat16 between two quantised tables"):
        ops.compact_rows((u8(5, 64), u8(5, 2)), None, i32(5), None, 3, (u8(3, 64), u8(3, 2)))
    with pytest.raises(_lib.DrnError, match="a quantised src is codes"):
        ops.compact_rows((u8(5, 40), u8(5, 1)), None, i32(5), None, 3, bf(3, 40))
    with pytest.raises(_lib.DrnError, match="one row a video has 6 rows for 5 positions"):
        ops.compact_rows(bf(6, 64), None, i32(5), None, 3, bf(3, 64))
    with pytest.raises(_lib.DrnError, match=r"dst_offsets must be a contiguous 1-D torch.int32 tensor of at least dst_videos \+ 1 = 4"):
        ops.compact_rows(bf(9, 64), i32(6), i32(5), i32(3), 3, bf(3, 64))


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_compact_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_compact.hip compiled for gfx950 on its own: the plan kernel and the ten instantiations of the rows kernel, each
    without scratch and without a spilled register.  Static LDS is what the source's arrays come to: the plan's two buffers of one
    64-bit total per wavefront of its 1024 threads (2 x 16 x 8 bytes), none for the rows.  The plan runs 1024 threads a workgroup, four
    wavefronts a SIMD: at most 128 registers."""
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_compact.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_compact.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_compact.hip")).read()
    threads = int(re.search(r"#define CP_THREADS (\d+)", src).group(1))
    claims = {"compact_plan_kernel": 2 * (threads // 64) * 8, "compact_rows_kernel": 0}
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == 11 and sum("compact_plan_kernel" in name for name in seen) == 1, sorted(seen)
    for name, (lds, scratch, vspill, sspill, regs) in seen.items():
        claim = [v for k, v in claims.items() if k in name]
        assert len(claim) == 1, name
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds == claim[0] and regs <= 128, (name, lds, regs)
