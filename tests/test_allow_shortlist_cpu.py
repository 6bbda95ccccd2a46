"""Filtered shortlists, the host side: the definitions with allow= (unchanged without it, equal to the sub-table form with it),
pack_allow_reference and Shortlister.allow_of, every refusal of shortlist(allow=), pack_allow and the wrappers before the library is
reached, the five C entries at ABI 9 and the compiler's resource notes for csrc/retrieve_allow.hip.
tests/test_allow_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_q8_shortlist_cpu import _no_library, resident, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKED = ("drn_shortlist_topn_allow", "drn_shortlist_segments_topn_allow", "drn_shortlist_topn_q8_allow",
          "drn_shortlist_segments_topn_q8_allow")
ENTRIES = MASKED + ("drn_pack_allow",)
BLOCK = 256


def exact_host(V, E, S_, seed=0):
    """tests/test_shortlist_gpu.py's exact_data, on the host in float32: integers in [-4, 4] with whole rows duplicated."""
    g = torch.Generator().manual_seed(seed + 1000 * V + E)
    emb = torch.randint(-4, 5, (V, E), generator=g).float()
    for a, b in ((1, 0), (V - 1, 0), (V // 2, V // 3), (BLOCK, 0), (BLOCK + 5, 2 * BLOCK + 3), (3 * BLOCK + 6, BLOCK - 1), (70, 5)):
        if 0 <= a < V and 0 <= b < V:
            emb[a] = emb[b]
    return emb, torch.randint(-4, 5, (S_, E), generator=g).float()


def same(got, want, what=""):
    assert type(got) is type(want), what
    for f in got._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


def masks_of(V, S_, seed):
    g = torch.Generator().manual_seed(seed)
    per = torch.rand(S_, V, generator=g) < 0.4
    per[:, 0], per[:, 1] = False, True                                          # the twins 0 and 1: the tie is split
    per[2] = False                                                              # a sentence that may list nothing
    return per[0].clone(), per


# -- 1. the references -------------------------------------------------------------------------------------------------------------------------

def test_the_references_are_unchanged_without_a_mask():
    """allow=None is the call without the argument, equals the all-ones mask, and -- on a case small enough to rank by hand -- a
    plain Python ranking by (score descending, position ascending)."""
    from drn_amd import segment_shortlist_reference, shortlist_reference
    emb, q = exact_host(33, 8, 5)
    off = [0, 3, 3, 10, 11, 33]
    for n in (1, 5, 64):
        same(shortlist_reference(emb, q, n, allow=None), shortlist_reference(emb, q, n))
        same(shortlist_reference(emb, q, n, allow=torch.ones(33, dtype=torch.bool)), shortlist_reference(emb, q, n))
        same(segment_shortlist_reference(emb, off, q, n, allow=None), segment_shortlist_reference(emb, off, q, n))
        same(segment_shortlist_reference(emb, off, q, n, allow=torch.ones(5, 5, dtype=torch.bool)), segment_shortlist_reference(emb, off, q, n))
    got = shortlist_reference(emb, q, 7)
    score = (q.double() @ emb.double().t()).tolist()
    for s in range(5):
        order = sorted(range(33), key=lambda v: (-score[s][v], v))[:7]
        assert got.ids[s].tolist() == order and got.scores[s].tolist() == [score[s][v] for v in order] and int(got.n[s]) == 7


@pytest.mark.parametrize("V", [33, 65])
@pytest.mark.parametrize("E", [8, 40])
def test_the_masked_references_equal_the_sub_table_form(V, E):
    """The reference over emb[keep] with the ids mapped back, field for field, for a shared and a per-sentence mask; for the ragged
    table the kept VIDEOS' runs are gathered and the offsets rebuilt."""
    from drn_amd import segment_shortlist_reference, shortlist_reference
    emb, q = exact_host(V, E, 5)
    shared, per = masks_of(V, 5, V + E)
    for n in (1, 5, 64):
        got = shortlist_reference(emb, q, n, allow=shared)
        keep = torch.nonzero(shared)[:, 0]
        sub = shortlist_reference(emb[keep], q, n)
        assert torch.equal(got.ids, torch.where(sub.ids >= 0, keep[sub.ids.clamp(min=0).long()].to(torch.int32), sub.ids))
        assert torch.equal(got.scores, sub.scores) and torch.equal(got.n, sub.n)
        assert 0 not in got.ids.tolist()[0] and bool((got.ids[:, :1] >= 0).all())
        rows = shortlist_reference(emb, q, n, allow=per)
        for s in range(5):
            keep = torch.nonzero(per[s])[:, 0]
            if len(keep) == 0:
                assert int(rows.n[s]) == 0 and bool((rows.ids[s] == -1).all()) and bool((rows.scores[s] == 0).all())
                continue
            sub = shortlist_reference(emb[keep], q[s:s + 1], n)
            assert torch.equal(rows.ids[s], torch.where(sub.ids[0] >= 0, keep[sub.ids[0].clamp(min=0).long()].to(torch.int32), sub.ids[0]))
            assert torch.equal(rows.scores[s], sub.scores[0]) and int(rows.n[s]) == int(sub.n[0])
    # ragged: V videos over the same rows, run lengths cycling 1 / 3 / 0 / 17 until the rows are used up
    lens, left = [], V
    while left:
        lens.append(min((1, 3, 0, 17)[len(lens) % 4], left))
        left -= lens[-1]
    off = np.concatenate([[0], np.cumsum(lens)])
    Vv = len(lens)
    shared, per = masks_of(Vv, 5, 3 * V + E)
    shared[2] = True                                                            # an empty video whose bit is set
    for n in (1, 5, 64):
        for mask in (shared, per):
            got = segment_shortlist_reference(emb, off, q, n, allow=mask)
            assert not bool((got.ids == 2).any())
            for s in range(5):
                keep = torch.nonzero(mask if mask.dim() == 1 else mask[s])[:, 0].tolist()
                if not keep:
                    assert int(got.n[s]) == 0 and bool((got.rows[s] == -1).all())
                    continue
                rows_kept = torch.cat([torch.arange(off[v], off[v + 1]) for v in keep])
                sub_off = np.concatenate([[0], np.cumsum([lens[v] for v in keep])])
                if len(rows_kept) == 0:
                    assert int(got.n[s]) == 0
                    continue
                sub = segment_shortlist_reference(emb[rows_kept], sub_off, q[s:s + 1], n)
                back = torch.tensor(keep, dtype=torch.int32)
                assert torch.equal(got.ids[s], torch.where(sub.ids[0] >= 0, back[sub.ids[0].clamp(min=0).long()], sub.ids[0])), (n, s)
                assert torch.equal(got.scores[s], sub.scores[0]) and torch.equal(got.rows[s], sub.rows[0]) and int(got.n[s]) == int(sub.n[0])


def test_a_masked_out_nan_or_best_score_changes_nothing_for_the_others():
    from drn_amd import _lib, segment_shortlist_reference, shortlist_reference
    emb, q = exact_host(33, 8, 5)
    shared, per = masks_of(33, 5, 1)
    dropped = int(torch.nonzero(~shared)[1, 0])
    for poison in (float("nan"), float("inf"), 1e30):
        bad = emb.clone()
        bad[dropped] = poison
        bad[0] = poison                                                         # (video 0 is dropped by every row of both masks)
        same(shortlist_reference(bad, q, 9, allow=shared), shortlist_reference(emb, q, 9, allow=shared), poison)
        off = list(range(0, 34, 3))
        vshared = torch.ones(11, dtype=torch.bool)
        vshared[dropped // 3] = vshared[0] = False
        same(segment_shortlist_reference(bad, off, q, 9, allow=vshared), segment_shortlist_reference(emb, off, q, 9, allow=vshared), poison)
    for wrong in (torch.ones(33), torch.ones(32, dtype=torch.bool), torch.ones(4, 33, dtype=torch.bool), [True] * 33):
        with pytest.raises(_lib.DrnError, match="allow must be a bool tensor"):
            shortlist_reference(emb, q, 9, allow=wrong)


# -- 2. pack_allow_reference and allow_of ----------------------------------------------------------------------------------------------------

def test_pack_allow_reference_puts_video_v_at_bit_v_and_31_of_word_v_over_32():
    from drn_amd import _lib, pack_allow_reference
    g = np.random.RandomState(3)
    for V in (1, 31, 32, 33, 775):
        for shape in ((V,), (1, V), (17, V)):
            mask = g.rand(*shape) < 0.5
            mask[..., V - 1] = True
            words = pack_allow_reference(mask)
            assert words.dtype == np.int32 and words.shape == shape[:-1] + (-(-V // 32),)
            flat, w = mask.reshape(-1, V), words.reshape(-1, words.shape[-1]).view(np.uint32)
            for s in range(flat.shape[0]):
                for v in range(V):
                    assert bool((w[s, v >> 5] >> (v & 31)) & 1) == bool(flat[s, v]), (V, s, v)
                if V % 32:
                    assert int(w[s, -1]) >> (V % 32) == 0
            assert (pack_allow_reference(torch.from_numpy(mask)) == words).all() and (pack_allow_reference(mask.tolist()) == words).all()
    assert pack_allow_reference(np.array([True] + [False] * 30 + [True, True])).view(np.uint32).tolist() == [0x80000001, 1]
    for wrong in (np.ones(4), np.ones((2, 2, 2), dtype=bool), np.ones((0,), dtype=bool), np.ones((0, 4), dtype=bool)):
        with pytest.raises(_lib.DrnError, match="must be booleans"):
            pack_allow_reference(wrong)


def test_allow_of_packs_names_and_positions_and_refuses_what_it_cannot_resolve(monkeypatch):
    from drn_amd import Shortlister, _lib, pack_allow_reference
    _no_library(monkeypatch)
    codes, scales = tables(rows=40)
    names = ["vid%d" % v for v in range(40)]
    plain = Shortlister.from_mx8(codes, scales, torch.bfloat16, names=names)
    ragged = Shortlister.from_mx8(codes, scales, torch.bfloat16, names=names[:3], offsets=[0, 2, 2, 40])

    def bits(words):
        assert words.dtype == torch.int32 and words.dim() == 1 and words.is_contiguous()
        return words.numpy().view(np.uint32).tolist()
    assert bits(plain.allow_of(keep=["vid0", 33, "vid39", np.int64(5)])) == [1 | 1 << 5, 1 << 1 | 1 << 7]
    assert bits(plain.allow_of(drop=["vid31", 32])) == [0x7fffffff, 0xfe]
    assert bits(plain.allow_of(keep=[])) == [0, 0] and bits(plain.allow_of(drop=())) == [0xffffffff, 0xff]
    assert bits(plain.allow_of(keep=[7, "vid7", 7])) == [1 << 7, 0]
    assert bits(ragged.allow_of(drop=["vid1"])) == [0b101] and bits(ragged.allow_of(keep=[2])) == [0b100]       # (videos, not rows)
    want = np.zeros(40, dtype=bool)
    want[[3, 4, 38]] = True
    assert (plain.allow_of(keep=[38, "vid3", 4]).numpy() == pack_allow_reference(want)).all()
    for kw in ({}, {"keep": [1], "drop": [2]}):
        with pytest.raises(_lib.DrnError, match="exactly one of keep= and drop="):
            plain.allow_of(**kw)
    with pytest.raises(_lib.DrnError, match="no video named 'vid40'"):
        plain.allow_of(drop=["vid1", "vid40"])
    with pytest.raises(_lib.DrnError, match="no video named 'vid3'"):
        ragged.allow_of(keep=["vid3"])
    for bad in (-1, 40, 1 << 40):
        with pytest.raises(_lib.DrnError, match=r"outside \[0, 40\)"):
            plain.allow_of(keep=[0, bad])
    with pytest.raises(_lib.DrnError, match=r"position 3 outside \[0, 3\)"):
        ragged.allow_of(drop=[3])
    for bad in (1.0, None, True, b"vid1"):
        with pytest.raises(_lib.DrnError, match="a name or a position"):
            plain.allow_of(keep=[bad])
    with pytest.raises(_lib.DrnError, match="has no names"):
        Shortlister.from_mx8(codes, scales, torch.bfloat16).allow_of(keep=["vid1"])


# -- 3. the interface -------------------------------------------------------------------------------------------------------------------------

def test_shortlist_refuses_a_bad_mask_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    codes, scales = tables(rows=40)
    q = resident(torch.zeros(3, 64, dtype=torch.bfloat16))
    for sl, W in ((Shortlister.from_mx8(codes, scales, torch.bfloat16), 2), (Shortlister.from_mx8(codes, scales, torch.bfloat16, offsets=[0, 2, 2, 40]), 1)):
        good = resident(torch.zeros(3, W, dtype=torch.int32))
        with pytest.raises(_lib.DrnError, match="pack_allow"):
            sl.shortlist(q, 2, allow=resident(torch.ones(3, len(sl), dtype=torch.bool)))
        with pytest.raises(_lib.DrnError, match="allow must be a packed mask, a tensor"):
            sl.shortlist(q, 2, allow=[0] * W)
        for dt in (torch.int64, torch.uint8, torch.float32, torch.int16):
            with pytest.raises(_lib.DrnError, match="allow must be torch.int32"):
                sl.shortlist(q, 2, allow=resident(torch.zeros(3, W, dtype=dt)))
        with pytest.raises(_lib.DrnError, match="on the table's device"):
            sl.shortlist(q, 2, allow=torch.zeros(3, W, dtype=torch.int32))      # a host tensor
        for shape in ((W + 1,), (3, W + 1), (2, W), (4, W), (1, 3, W), (3 * W,) if W > 1 else (3, W, 1), ()):
            with pytest.raises(_lib.DrnError, match=r"allow must be \(%d,\)" % W):
                sl.shortlist(q, 2, allow=resident(torch.zeros(shape, dtype=torch.int32)))
        with pytest.raises(_lib.DrnError, match="allow must be contiguous"):
            sl.shortlist(q, 2, allow=resident(torch.zeros(3, 2 * W, dtype=torch.int32)[:, ::2]))
        # the other refusals come first and are unchanged
        with pytest.raises(_lib.DrnError, match=r"outside \[1, 128\]"):
            sl.shortlist(q, 129, allow=good)
        # a good mask, per sentence or shared, passes them all
        assert sl._check_allow(good, 3) is None and sl._check_allow(resident(torch.zeros(W, dtype=torch.int32)), 3) is None


def test_pack_allow_and_the_wrappers_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops, pack_allow
    _no_library(monkeypatch)
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        pack_allow(torch.ones(40, dtype=torch.bool))
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        pack_allow([True] * 40)
    for bad in (torch.ones(40), torch.ones(40, dtype=torch.uint8), torch.ones(2, 2, 2, dtype=torch.bool), torch.ones(0, dtype=torch.bool),
                torch.ones(0, 4, dtype=torch.bool), torch.ones(40, 3, dtype=torch.bool).t(), torch.tensor(True)):
        with pytest.raises(_lib.DrnError, match="contiguous bool tensor"):
            pack_allow(resident(bad))
    mask = resident(torch.ones(3, 40, dtype=torch.bool))
    for out in (torch.zeros(3, 2, dtype=torch.int32), resident(torch.zeros(3, 2, dtype=torch.int64)), resident(torch.zeros(3, 1, dtype=torch.int32)),
                resident(torch.zeros(2, dtype=torch.int32)), resident(torch.zeros(2, 3, dtype=torch.int32).t()), [0] * 6):
        with pytest.raises(_lib.DrnError, match=r"out must be a contiguous \(3, 2\) torch.int32"):
            pack_allow(mask, out=out)
    with pytest.raises(AssertionError, match="the library was reached"):
        pack_allow(mask, out=resident(torch.zeros(3, 2, dtype=torch.int32)))
    # the wrappers: host tensors, and a mask of the wrong type or shape
    assert ops.allow_words(1) == ops.allow_words(32) == 1 and ops.allow_words(33) == 2 and ops.allow_words(775) == 25
    codes, scales = tables(rows=40)
    i32 = lambda *shape: resident(torch.zeros(shape, dtype=torch.int32))
    emb, q, ws = resident(torch.zeros(40, 64)), resident(torch.zeros(3, 64)), resident(torch.zeros(64, dtype=torch.int64))
    outs = (i32(3, 2), resident(torch.zeros(3, 2)), i32(3))
    seg = (i32(4), i32(2), i32(3))                                              # offsets (V = 3), blk_vid (one block), vid_blk
    calls = {
        "shortlist_topn_allow": (lambda a: ops.shortlist_topn(emb, q, 2, ws, *outs, allow=a), 2),
        "shortlist_segments_topn_allow": (lambda a: ops.shortlist_segments_topn(emb, q, *seg, 2, ws, *outs, i32(3, 2), allow=a), 1),
        "shortlist_topn_q8_allow": (lambda a: ops.shortlist_topn((codes, scales), q, 2, ws, *outs, allow=a), 2),
        "shortlist_segments_topn_q8_allow": (lambda a: ops.shortlist_segments_topn((codes, scales), q, *seg, 2, ws, *outs, i32(3, 2), allow=a), 1),
    }
    for name, (call, W) in calls.items():
        with pytest.raises(_lib.DrnError, match="GPU only"):
            call(torch.zeros(W, dtype=torch.int32))
        for bad in (resident(torch.zeros(W, dtype=torch.int64)), resident(torch.ones(3, 40, dtype=torch.bool)), i32(W + 1), i32(2, W), i32(3, W + 1),
                    i32(3, 2 * W)[:, ::2]):
            with pytest.raises(_lib.DrnError, match="%s: allow must be a contiguous torch.int32 tensor" % name):
                call(bad)
        for good in (i32(W), i32(3, W)):
            with pytest.raises(AssertionError, match="the library was reached"):
                call(good)
    with pytest.raises(_lib.DrnError, match=r"shortlist_topn_allow: n = 129 outside \[1, 128\]"):
        ops.shortlist_topn(emb, q, 129, ws, *outs, allow=i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_topn_allow: ws must be"):
        ops.shortlist_topn(emb, q, 2, ws[:5], *outs, allow=i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_segments_topn_allow: vid_blk must be"):
        ops.shortlist_segments_topn(emb, q, seg[0], seg[1], i32(4), 2, ws, *outs, i32(3, 2), allow=i32(1))


def test_library_exports_the_five_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name in ENTRIES:
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig), (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
        wrapper = name[len("drn_"):]                                         # a masked entry is its twin's wrapper with allow=
        assert callable(getattr(ops, wrapper[:wrapper.index("_topn") + len("_topn")] if name in MASKED else wrapper))
    # each masked entry is its twin plus (allow, allow_stride), in front of the sizes
    for name in MASKED:
        twin, mine = _header_params(name[:-len("_allow")]), _header_params(name)
        at = mine.index("const int32_t* allow")
        assert mine[at + 1] == "int allow_stride" and mine[:at] + mine[at + 2:] == twin, name
        assert mine[at + 2] in ("int V", "int R")
    assert callable(drn_amd.pack_allow) and callable(drn_amd.pack_allow_reference) and callable(drn_amd.Shortlister.allow_of)
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_allow.hip")).read()
    assert int(re.search(r"#define AL_BLOCK\s+(\d+)", src).group(1)) == _lib.SHORTLIST_BLOCK == _lib.SHORTLIST_SEG_BLOCK


def test_the_entries_check_their_arguments_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def plain(V=300, E=64, S=2, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 7 if ptrs is None else ptrs                                # emb queries allow ws | ids scores counts
        return L.drn_shortlist_topn_allow(a[0], a[1], a[2], stride, V, E, S, n, dtype, a[3], keys, a[4], a[5], a[6], None)

    def segs(R=900, V=300, nblocks=2, E=64, S=2, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 11 if ptrs is None else ptrs                               # emb queries offsets blk_vid vid_blk allow ws | ids scores counts rows
        return L.drn_shortlist_segments_topn_allow(a[0], a[1], a[2], a[3], a[4], a[5], stride, R, V, nblocks, E, S, n, dtype, a[6], keys, a[7],
                                                   a[8], a[9], a[10], None)

    def plain_q8(V=300, E=64, S=2, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 8 if ptrs is None else ptrs                                # codes scales queries allow ws | ids scores counts
        return L.drn_shortlist_topn_q8_allow(a[0], a[1], a[2], a[3], stride, V, E, S, n, dtype, a[4], keys, a[5], a[6], a[7], None)

    def segs_q8(R=900, V=300, nblocks=2, E=64, S=2, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 12 if ptrs is None else ptrs                               # codes scales queries offsets blk_vid vid_blk allow ws | ids scores counts rows
        return L.drn_shortlist_segments_topn_q8_allow(a[0], a[1], a[2], a[3], a[4], a[5], a[6], stride, R, V, nblocks, E, S, n, dtype, a[7], keys,
                                                      a[8], a[9], a[10], a[11], None)
    # (function, pointers, where the mask is among them, where the queries are)
    for fn, nptr, mask_at, q_at in ((plain, 7, 2, 1), (segs, 11, 5, 1), (plain_q8, 8, 3, 2), (segs_q8, 12, 6, 2)):
        for i in range(nptr):
            assert fn(ptrs=[None if j == i else p for j in range(nptr)]) != 0 and b"null pointer" in L.drn_last_error(), (fn.__name__, i)
        assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in L.drn_last_error()
        for n in (0, 129):
            assert fn(n=n) != 0 and b"outside [1, 128]" in L.drn_last_error()
        assert fn(dtype=2) != 0 and b"dtype" in L.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1004)] + [p] * (nptr - 1)) != 0 and b"16-byte aligned" in L.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1008) if j == q_at else p for j in range(nptr)]) != 0 and b"16-byte aligned" in L.drn_last_error()
        # the mask: its stride is 0 or ceil(300 / 32) = 10, and it is 4-byte aligned
        for stride in (1, 9, 11, -10, 300):
            assert fn(stride=stride) != 0 and b"neither 0" in L.drn_last_error() and b"ceil(V / 32) = 10" in L.drn_last_error(), stride
        for off in (1, 2, 3):
            assert fn(ptrs=[ctypes.c_void_p(0x1000 + off) if j == mask_at else p for j in range(nptr)]) != 0 \
                and b"mask must be 4-byte aligned" in L.drn_last_error()
        assert fn(V=320, stride=11) != 0 and fn(V=321, stride=10) != 0 and b"neither 0" in L.drn_last_error()
    for fn in (plain_q8, segs_q8):
        for E in (8, 48, 33, 500):
            assert fn(E=E) != 0 and b"not a multiple of the block of 32 columns" in L.drn_last_error(), E
    for fn in (plain, plain_q8):
        assert fn(keys=2 * 2 * 4 - 1) != 0 and b"16 are needed" in L.drn_last_error()
        assert fn(keys=2 * 2 * 4 - 1, stride=10) != 0 and b"16 are needed" in L.drn_last_error()
        assert fn(V=1 << 30, S=1 << 10, n=128, keys=0x7fffffff) != 0 and b"are needed" in L.drn_last_error()          # (no int overflow)
    for fn in (segs, segs_q8):
        assert fn(R=0) != 0 and b"bad args" in L.drn_last_error()
        for nblocks in (0, 1, 301):                                          # (300 videos need two blocks of 256 at least, 300 at most)
            assert fn(nblocks=nblocks) != 0 and b"blocks outside" in L.drn_last_error(), nblocks
        assert fn(keys=16 + 8 - 1) != 0 and b"24 are needed" in L.drn_last_error()
    # drn_pack_allow
    pack = lambda mask=p, S=2, V=40, words=p: L.drn_pack_allow(mask, S, V, words, None)
    assert pack(mask=None) != 0 and b"null pointer" in L.drn_last_error() and pack(words=None) != 0 and b"null pointer" in L.drn_last_error()
    assert pack(S=0) != 0 and pack(V=0) != 0 and b"bad args" in L.drn_last_error()
    assert pack(words=ctypes.c_void_p(0x1002)) != 0 and b"4-byte aligned" in L.drn_last_error()


# -- 4. the compiler's resource notes ---------------------------------------------------------------------------------------------------------

def test_the_masked_kernels_spill_nothing_and_keep_the_register_cap(tmp_path):
    """csrc/retrieve_allow.hip compiled for gfx950 on its own: two phase-one bodies, each instantiated for the four table operands
    (plain bf16 / fp32, FP8 codes under bf16 / fp32 queries), and the packing kernel.  Every one without scratch and without a spilled
    register, at most 128 VGPRs + AGPRs (the cap the unmasked kernels are held to), and static LDS exactly what the arrays come to:
    the twin's 16 x 256 keys plus 16 x 8 mask words and 4 flags = 33,296 B; the twin's 50,272 B plus 16 x 9 mask words (a ragged block
    starts inside a word) and 4 flags = 50,864 B; none for the packing."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_allow.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_allow.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    B = _lib.SHORTLIST_SEG_BLOCK
    ranking = 16 * _lib.SHORTLIST_BLOCK * 8 + 16 * (_lib.SHORTLIST_BLOCK // 32) * 4 + 4 * 4
    segmented = 16 * B * 8 + 16 * (B + 1) * 4 + (B + 4) * 4 + 4 * 4 + 16 * (B // 32 + 1) * 4 + 4 * 4
    assert (ranking, segmented) == (33296, 50864)
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_allow.hip")).read()
    assert sorted(re.findall(r"__global__[^\n]*?void (\w+)\(", src)) == ["pack_allow_kernel", "shortlist_block_allow_kernel",
                                                                           "shortlist_segments_allow_kernel"]
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    claims = {"shortlist_block_allow_kernel": (ranking, 4), "shortlist_segments_allow_kernel": (segmented, 4), "pack_allow_kernel": (0, 1)}
    assert len(seen) == sum(count for _, count in claims.values()), sorted(seen)
    for stem, (lds_claim, count) in claims.items():
        mine = {k: v for k, v in seen.items() if stem in k}
        assert len(mine) == count, (stem, sorted(mine))
        if count == 4:                                                       # one per operand: plain and FP8, bf16 and fp32
            assert sorted(("AlQ8" in k, "DF16b" in k) for k in mine) == [(False, False), (False, True), (True, False), (True, True)], sorted(mine)
        for name, (lds, scratch, vspill, sspill, regs) in mine.items():
            assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
            assert lds == lds_claim and regs <= 128, (name, lds, regs)
