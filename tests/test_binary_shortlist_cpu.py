"""Binary shortlists, the host side: the format of the sign codes (drn_amd/binary.py), the definition against the float64 references over
the dequantised table, every refusal of BinaryShortlister, from_codes, shortlist and ops.shortlist_bin before the library is reached, the
C entry drn_shortlist_bin at ABI 9 with its argument checks -- by calls that FAIL validation only: nothing here may launch -- and the
compiler's resource notes for csrc/retrieve_bin.hip.  tests/test_binary_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from drn_amd.binary import BinaryShortlister, binary_dequantize, binary_quantize_reference, binary_shortlist_reference, binary_signs
from test_allow_shortlist_cpu import same
from test_grounding_cpu import _header_params, built_lib
from test_q8_shortlist_cpu import _no_library, resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 31, 32, 33, 40, 64, 96, 512)


def table(rows, E, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * rows + E)
    return torch.randn(rows, E, generator=g)


def ragged_offsets(rows):
    """Runs cycling 1 / 3 / 0 / 17 over `rows` rows: videos without rows among them."""
    lens, left = [], rows
    while left:
        lens.append(min((1, 3, 0, 17)[len(lens) % 4], left))
        left -= lens[-1]
    lens.append(0)                                                              # (and one at the very end)
    return np.concatenate([[0], np.cumsum(lens)])


# -- 1. the format -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", WIDTHS)
def test_quantise_and_dequantise_round_trip_and_the_pad_bits_are_zero(E):
    from drn_amd import pack_allow_reference
    x = table(7, E)
    codes = binary_quantize_reference(x)
    W = -(-E // 32)
    assert torch.is_tensor(codes) and codes.dtype == torch.int32 and tuple(codes.shape) == (7, W)
    # bit by bit, in plain Python
    for r in range(7):
        words = [int(w) & 0xffffffff for w in codes[r].tolist()]
        for e in range(32 * W):
            assert (words[e >> 5] >> (e & 31)) & 1 == (1 if e < E and not float(x[r, e]) < 0 else 0), (r, e)
    assert np.array_equal(codes.numpy(), pack_allow_reference(~(x < 0))), "the bit convention is pack_allow's"
    assert np.array_equal(binary_quantize_reference(x.numpy()), codes.numpy()), "an array gives the same words"
    for dtype in (torch.float64, torch.float32, torch.bfloat16):
        dq = binary_dequantize(codes, E, dtype)
        assert dq.dtype == dtype and tuple(dq.shape) == (7, E) and dq.is_contiguous()
        assert torch.equal(dq.double(), torch.where(x < 0, -1.0, 1.0).double())
        assert torch.equal(binary_quantize_reference(dq), codes)
    # all-negative rows are all-zero words; all-positive rows have exactly the E real bits set
    assert bool((binary_quantize_reference(-torch.ones(2, E)) == 0).all())
    full = binary_quantize_reference(torch.ones(2, E)).numpy().view(np.uint32)
    assert int(sum(bin(int(w)).count("1") for w in full[0])) == E
    if E % 32:
        assert int(full[0, -1]) == (1 << (E % 32)) - 1
    assert torch.equal(binary_quantize_reference(x.bfloat16()), binary_quantize_reference(x.bfloat16().float()))


def test_both_zeros_map_to_bit_one_and_to_plus_one():
    x = torch.tensor([[0.0, -0.0, -1.0, 1.0, -1e-30, 1e-30]])
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        assert binary_quantize_reference(x.to(dtype)).tolist() == [[0b101011]]
        signs = binary_signs(x.to(dtype))
        assert signs.dtype == dtype and signs.tolist() == [[1.0, 1.0, -1.0, 1.0, -1.0, 1.0]]
    assert binary_dequantize(torch.tensor([[0b101011]], dtype=torch.int32), 6, torch.float32).tolist() == [[1.0, 1.0, -1.0, 1.0, -1.0, 1.0]]


def test_a_query_row_that_is_not_finite_becomes_all_nan():
    q = table(5, 40)
    q[1, 7], q[3, 0], q[4, 39] = float("nan"), float("inf"), float("-inf")
    for dtype in (torch.float32, torch.bfloat16):
        signs = binary_signs(q.to(dtype))
        assert signs.dtype == dtype and signs.is_contiguous()
        assert torch.isnan(signs).all(dim=1).tolist() == [False, True, False, True, True]
        assert torch.equal(signs[[0, 2]].double(), torch.where(q[[0, 2]] < 0, -1.0, 1.0).double())


def test_the_definitions_refuse_what_is_not_a_table():
    from drn_amd import _lib
    for bad in (torch.zeros(4), torch.zeros(0, 4), torch.zeros(4, 0), np.zeros((2, 3, 4))):
        with pytest.raises(_lib.DrnError, match="binary_quantize_reference"):
            binary_quantize_reference(bad)
    codes = binary_quantize_reference(table(4, 40))
    for c, E in ((codes, 97), (codes, 65), (codes, 32), (codes, 0), (codes.long(), 40), (codes[0], 40)):
        with pytest.raises(_lib.DrnError, match="binary_dequantize: codes must be int32"):
            binary_dequantize(c, E, torch.float32)
        with pytest.raises(_lib.DrnError, match="binary_shortlist_reference: codes must be int32"):
            binary_shortlist_reference(c, E, torch.zeros(2, 40), 3)
    with pytest.raises(_lib.DrnError, match=r"queries must be a float tensor \(S, 40\)"):
        binary_shortlist_reference(codes, 40, torch.zeros(2, 41), 3)
    with pytest.raises(_lib.DrnError, match="binary_signs"):
        binary_signs(torch.zeros(3, dtype=torch.float32))


# -- 2. the definition -------------------------------------------------------------------------------------------------------------------------

def test_the_reference_is_a_plain_python_ranking_of_popcounts():
    """Small enough to rank by hand: E = 32, one word a row, 33 possible scores over 70 rows -- ties everywhere."""
    E, V = 32, 70
    x, q = table(V, E), table(3, E, seed=9)
    codes = binary_quantize_reference(x)
    cw = [int(w) & 0xffffffff for w in codes[:, 0].tolist()]
    qw = [int(w) & 0xffffffff for w in binary_quantize_reference(q)[:, 0].tolist()]
    for n in (1, 5, 70, 100):
        got = binary_shortlist_reference(codes, E, q, n)
        assert got.ids.dtype == torch.int32 and got.scores.dtype == torch.float32 and got.n.dtype == torch.int32
        for s in range(3):
            score = [E - 2 * bin(qw[s] ^ cw[v]).count("1") for v in range(V)]
            order = sorted(range(V), key=lambda v: (-score[v], v))[:n]
            assert got.ids[s, :len(order)].tolist() == order and got.scores[s, :len(order)].tolist() == [float(score[v]) for v in order]
            assert bool((got.ids[s, len(order):] == -1).all()) and bool((got.scores[s, len(order):] == 0).all()) and int(got.n[s]) == len(order)
    far = binary_shortlist_reference(codes, E, q, 70)
    assert bool(((far.scores[:, 1:] == far.scores[:, :-1]) & (far.ids[:, 1:] > far.ids[:, :-1])).any()), "no tie in the data"


@pytest.mark.parametrize("E", [32, 40, 96])
def test_the_reference_equals_the_float64_references_over_the_dequantised_table(E):
    """Plain and ragged (videos without rows among them); no mask, a shared mask, a mask per sentence with an all-zero row; a NaN query
    row and an inf query row, which list nothing."""
    from drn_amd import segment_shortlist_reference, shortlist_reference
    R, S = 300, 6
    x, q = table(R, E), table(S, E, seed=3)
    q[1, E // 2], q[4, 0] = float("nan"), float("inf")
    codes = binary_quantize_reference(x)
    wide, signs = binary_dequantize(codes, E, torch.float64), binary_signs(q)
    off = ragged_offsets(R)
    V = len(off) - 1
    assert bool((np.diff(off) == 0).any())
    g = torch.Generator().manual_seed(E)
    for rows, offsets in ((R, None), (V, off)):
        per = torch.rand(S, rows, generator=g) < 0.5
        per[2] = False
        for allow in (None, per[0].clone(), per):
            for n in (1, 7, 128, 400):
                got = binary_shortlist_reference(codes, E, q, n, offsets=offsets, allow=allow)
                want = (shortlist_reference(wide, signs, n, allow=allow) if offsets is None
                        else segment_shortlist_reference(wide, offsets, signs, n, allow=allow))
                same(got, want, (E, offsets is not None, None if allow is None else allow.dim(), n))
                assert got.n[1] == 0 and got.n[4] == 0 and bool((got.ids[[1, 4]] == -1).all()) and bool((got.scores[[1, 4]] == 0).all())
                if allow is per:
                    assert got.n[2] == 0
                assert int(got.n[0]) > 0
        if offsets is not None:
            far = binary_shortlist_reference(codes, E, q, 400, offsets=offsets)
            owners = int((np.diff(off) > 0).sum())
            assert far.n.tolist() == [owners, 0, owners, owners, 0, owners] and bool((far.rows[0, :owners] >= 0).all())
            empty = set(np.nonzero(np.diff(off) == 0)[0].tolist())
            assert not empty & set(far.ids[0, :owners].tolist()), "a video without rows is listed"


def test_rows_names_the_lowest_tied_segment():
    """One video of five identical rows between two others: every row reaches the best score, segment 0 is named."""
    E = 40
    x = table(7, E)
    x[1:6] = x[1]
    got = binary_shortlist_reference(binary_quantize_reference(x), E, x[1:2].clone(), 3, offsets=[0, 1, 6, 7])
    assert got.ids[0, 0] == 1 and got.scores[0, 0] == E and got.rows[0, 0] == 0


# -- 3. the interface --------------------------------------------------------------------------------------------------------------------------

def test_bytes_of_and_the_public_names():
    import drn_amd
    from drn_amd import _lib, ops
    assert BinaryShortlister.bytes_of(1, 512) == 64 and BinaryShortlister.bytes_of(65536, 512) == 4 << 20
    assert [BinaryShortlister.bytes_of(3, E) for E in (1, 32, 33, 40, 96, 4096)] == [12, 12, 24, 24, 36, 3 * 512]
    assert 16 * BinaryShortlister.bytes_of(10, 512) == drn_amd.Shortlister.bytes_of(10, 512, torch.bfloat16)
    assert drn_amd.BINARY_MAX_E == _lib.BINARY_MAX_E == 4096 and ops.binary_words(4096) * 16 * 4 == 8192
    for name in ("BinaryShortlister", "binary_quantize_reference", "binary_dequantize", "binary_signs", "binary_shortlist_reference"):
        assert getattr(drn_amd, name) is getattr(drn_amd.binary, name), name
    assert BinaryShortlister.shortlist_deep is BinaryShortlister.shortlist
    sl = BinaryShortlister.from_codes(resident(binary_quantize_reference(table(40, 96))), 96, torch.bfloat16, names=["v%d" % v for v in range(40)])
    assert len(sl) == 40 and sl.E == 96 and sl.dtype == torch.bfloat16 and sl.nbytes == BinaryShortlister.bytes_of(40, 96) == 480
    assert sl.offsets is None and sl.plan is None and sl.device == sl.codes.device
    rag = BinaryShortlister.from_codes(resident(binary_quantize_reference(table(40, 96))), 96, torch.float32, offsets=[0, 2, 2, 40])
    assert len(rag) == 3 and rag.offsets.tolist() == [0, 2, 2, 40] and rag.plan.blk_vid.tolist() == [0, 3] and rag.nbytes == 480
    assert sl.allow_of(keep=["v1", 33]).tolist() == [2, 2] and rag.allow_of(drop=[1]).tolist() == [5]
    with pytest.raises(_lib.DrnError, match="BinaryShortlister.allow_of: exactly one"):
        sl.allow_of()

    class Store(object):
        names = ["v%d" % v for v in range(40)]
    sl.check(Store)
    with pytest.raises(_lib.DrnError, match="names are not the store's"):
        rag.check(Store)


def test_the_module_never_imports_the_oracle():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "drn_amd", "binary.py")).read())
    mods = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            mods.append(node.module or "")
    assert mods and not any(m.split(".")[0] == "oracle" for m in mods), mods


def test_the_constructor_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib
    _no_library(monkeypatch)
    with pytest.raises(_lib.DrnError, match="BinaryShortlister: the embeddings must be a tensor on the GPU"):
        BinaryShortlister(torch.zeros(4, 64))
    with pytest.raises(_lib.DrnError, match="BinaryShortlister: the embeddings must be a tensor on the GPU"):
        BinaryShortlister([[0.0] * 64])
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(_lib.DrnError, match="bfloat16 or float32, not %s" % dt):
            BinaryShortlister(resident(torch.zeros(4, 64, dtype=dt)))
    for bad in (torch.zeros(64), torch.zeros(0, 64), torch.zeros(4, 0), torch.zeros(2, 2, 64), torch.zeros(64, 4).t()):
        with pytest.raises(_lib.DrnError, match=r"contiguous \(V, E\) tensor"):
            BinaryShortlister(resident(bad))
    with pytest.raises(_lib.DrnError, match=r"E = 4097 outside \[1, 4096\]"):
        BinaryShortlister(resident(torch.zeros(2, 4097)))
    x = torch.zeros(4, 64)
    x[2, 5] = float("inf")
    with pytest.raises(_lib.DrnError, match="Shortlister: the embeddings hold values that are not finite"):
        BinaryShortlister(resident(x))
    with pytest.raises(_lib.DrnError, match="3 names for 4 embeddings"):
        BinaryShortlister(resident(torch.zeros(4, 64)), names=["a", "b", "c"])
    for off, why in (([0, 2, 5], "end at R = 4"), ([1, 4], "start at 0"), ([0, 3, 2, 4], "decrease at video 1"), ([0.0, 4.0], "must be integers")):
        with pytest.raises(_lib.DrnError, match=why):
            BinaryShortlister(resident(torch.zeros(4, 64)), offsets=off)
    with pytest.raises(_lib.DrnError, match="1 names for 2 videos"):
        BinaryShortlister(resident(torch.zeros(4, 64)), names=["a"], offsets=[0, 1, 4])
    with pytest.raises(AssertionError, match="the library was reached"):            # a good table goes on to pack_allow
        BinaryShortlister(resident(torch.zeros(4, 64)), offsets=[0, 1, 4])


def test_from_codes_refuses_what_is_not_a_table_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib
    _no_library(monkeypatch)
    what = "BinaryShortlister.from_codes"
    codes = binary_quantize_reference(table(6, 40))
    with pytest.raises(_lib.DrnError, match=what + ": the codes must be a tensor on the GPU"):
        BinaryShortlister.from_codes(codes, 40, torch.bfloat16)
    with pytest.raises(_lib.DrnError, match=what + ": the codes must be a tensor on the GPU"):
        BinaryShortlister.from_codes(codes.numpy(), 40, torch.bfloat16)
    for dt in (torch.int64, torch.uint8, torch.float32):
        with pytest.raises(_lib.DrnError, match=what + ": the codes must be torch.int32 words, not %s" % dt):
            BinaryShortlister.from_codes(resident(codes.to(dt)), 40, torch.bfloat16)
    for E in (0, -5, 4097):
        with pytest.raises(_lib.DrnError, match=what + r": E = %d outside \[1, 4096\]" % E):
            BinaryShortlister.from_codes(resident(codes), E, torch.bfloat16)
    for E in (32, 65, 512):
        with pytest.raises(_lib.DrnError, match=what + r": the codes must be a contiguous \(rows, %d\) tensor" % (-(-E // 32))):
            BinaryShortlister.from_codes(resident(codes), E, torch.bfloat16)
    for bad in (codes[0], codes[:0], codes[None], codes.t().contiguous().t()):
        with pytest.raises(_lib.DrnError, match=what + r": the codes must be a contiguous \(rows, 2\) tensor"):
            BinaryShortlister.from_codes(resident(bad), 40, torch.bfloat16)
    for dt in (torch.float16, torch.float64, None):
        with pytest.raises(_lib.DrnError, match=what + r": dtype \(of the queries\) must be bfloat16 or float32"):
            BinaryShortlister.from_codes(resident(codes), 40, dt)
    for bit in (8, 20, 31):                                                       # a set bit at or past E = 40: the soundness check
        dirty = codes.clone()
        dirty[3, 1] |= int(np.array([1 << bit], dtype=np.uint32).view(np.int32)[0])
        with pytest.raises(_lib.DrnError, match="Shortlister: the codes have a set bit at or past E = 40"):
            BinaryShortlister.from_codes(resident(dirty), 40, torch.bfloat16)
    clean = codes.clone()
    clean[3, 1] |= 1 << 7                                                         # (bit 39 is a real bit)
    assert len(BinaryShortlister.from_codes(resident(clean), 40, torch.bfloat16)) == 6
    assert len(BinaryShortlister.from_codes(resident(torch.full((3, 2), -1, dtype=torch.int32)), 64, torch.float32)) == 3
    with pytest.raises(_lib.DrnError, match="5 names for 6 embeddings"):
        BinaryShortlister.from_codes(resident(codes), 40, torch.bfloat16, names=list("abcde"))
    with pytest.raises(_lib.DrnError, match="end at R = 6"):
        BinaryShortlister.from_codes(resident(codes), 40, torch.bfloat16, offsets=[0, 7])


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_shortlist_refuses_before_the_library_is_reached(monkeypatch, ragged):
    from drn_amd import _lib
    _no_library(monkeypatch)
    codes = resident(binary_quantize_reference(table(40, 64)))
    sl = BinaryShortlister.from_codes(codes, 64, torch.bfloat16, offsets=[0, 2, 2, 40] if ragged else None)
    W = 1 if ragged else 2
    q = resident(torch.zeros(3, 64, dtype=torch.bfloat16))
    for fn in (sl.shortlist, sl.shortlist_deep):
        what = "BinaryShortlister.shortlist"
        with pytest.raises(_lib.DrnError, match=what + ".*on the GPU"):
            fn(torch.zeros(3, 64, dtype=torch.bfloat16), 300)                    # host queries
        with pytest.raises(_lib.DrnError, match=what + ".*must be a tensor"):
            fn([[0.0] * 64], 300)
        for n in (0, -1, 1025):
            with pytest.raises(_lib.DrnError, match=what + r": n = %d outside \[1, 1024\]" % n):
                fn(q, n)
        for shape in ((3, 63), (3, 65), (64,), (3, 1, 64), (0, 64), (3, 2)):       # (3, 2): codes are not queries
            with pytest.raises(_lib.DrnError, match=what + r": the queries must be \(S, 64\)"):
                fn(resident(torch.zeros(shape, dtype=torch.bfloat16)), 300)
        for dt in (torch.float32, torch.float16, torch.int32):
            with pytest.raises(_lib.DrnError, match=what + ": the queries are %s" % dt):
                fn(resident(torch.zeros(3, 64, dtype=dt)), 300)
        with pytest.raises(_lib.DrnError, match="bool tensor; pack it first"):
            fn(q, 300, allow=resident(torch.ones(3, len(sl), dtype=torch.bool)))
        with pytest.raises(_lib.DrnError, match=r"allow must be \(%d,\)" % W):
            fn(q, 300, allow=resident(torch.zeros(W + 1, dtype=torch.int32)))
        with pytest.raises(_lib.DrnError, match="allow must be on the table's device|allow must be a packed mask"):
            fn(q, 300, allow=[1] * W)
        good = (resident(torch.zeros(3, 300, dtype=torch.int32)), resident(torch.zeros(3, 300)), resident(torch.zeros(3, dtype=torch.int32)))
        with pytest.raises(_lib.DrnError, match=what + ": out must hold the %s buffers" % ("four" if ragged else "three")):
            fn(q, 300, out=good + (good[0],) * (0 if ragged else 1))
        with pytest.raises(_lib.DrnError, match=what + r": out.ids must be a contiguous \(3, 300\)"):
            fn(q, 300, out=(resident(torch.zeros(3, 128, dtype=torch.int32)),) + good[1:] + ((good[0],) if ragged else ()))
        with pytest.raises(_lib.DrnError, match=what + r": out.scores must be a contiguous \(3, 300\)"):
            fn(q, 300, out=(good[0], resident(torch.zeros(3, 300, dtype=torch.float64)), good[2]) + ((good[0],) if ragged else ()))


def test_the_wrapper_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops
    _no_library(monkeypatch)
    i32 = lambda *shape: resident(torch.zeros(shape, dtype=torch.int32))
    codes, q, ws = i32(40, 2), resident(torch.zeros(3, 64)), resident(torch.zeros(4096, dtype=torch.int64))
    outs = (i32(3, 300), resident(torch.zeros(3, 300)), i32(3))
    seg = (i32(4), i32(2), i32(3))                                              # offsets (V = 3), blk_vid (one block), vid_blk
    with pytest.raises(_lib.DrnError, match="shortlist_bin: allow is required"):
        ops.shortlist_bin(codes, 64, q, (), 300, ws, outs, None)
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.shortlist_bin(codes, 64, q, (), 300, ws, outs, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.shortlist_bin(torch.zeros(40, 2, dtype=torch.int32), 64, q, (), 300, ws, outs, i32(2))
    for E in (0, 4097):
        with pytest.raises(_lib.DrnError, match=r"shortlist_bin: E = %d outside \[1, 4096\]" % E):
            ops.shortlist_bin(codes, E, q, (), 300, ws, outs, i32(2))
    for bad, E in ((codes, 32), (codes, 65), (resident(torch.zeros(40, 2, dtype=torch.int64)), 64), (i32(2), 64), (i32(0, 2), 64), (i32(2, 40).t(), 64)):
        with pytest.raises(_lib.DrnError, match="shortlist_bin: codes must be a contiguous"):
            ops.shortlist_bin(bad, E, resident(torch.zeros(3, E)), (), 300, ws, outs, i32(2))
    for bad in (resident(torch.zeros(3, 63)), resident(torch.zeros(64)), resident(torch.zeros(3, 64, dtype=torch.float16)), resident(torch.zeros(64, 3).t()),
                i32(3, 64)):
        with pytest.raises(_lib.DrnError, match="shortlist_bin: queries must be a contiguous"):
            ops.shortlist_bin(codes, 64, bad, (), 300, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match=r"shortlist_bin: n = 1025 outside \[1, 1024\]"):
        ops.shortlist_bin(codes, 64, q, (), 1025, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match=r"shortlist_bin: n = 0 outside \[1, 1024\]"):
        ops.shortlist_bin(codes, 64, q, (), 0, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_bin: ids must be"):
        ops.shortlist_bin(codes, 64, q, (), 299, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_bin: ws must be a contiguous int64 tensor of at least 768"):
        ops.shortlist_bin(codes, 64, q, (), 300, ws[:767], outs, i32(2))         # 3 sentences x 1 block x min(300, 256) keys
    with pytest.raises(_lib.DrnError, match="shortlist_bin: ws must be a contiguous int64 tensor of at least 1152"):
        ops.shortlist_bin(codes, 64, q, seg, 300, ws[:1151], outs + (i32(3, 300),), i32(1))       # and half as many again
    with pytest.raises(_lib.DrnError, match="shortlist_bin: allow must be a contiguous torch.int32 tensor"):
        ops.shortlist_bin(codes, 64, q, (), 300, ws, outs, i32(3))
    with pytest.raises(_lib.DrnError, match="shortlist_bin: seg must be"):
        ops.shortlist_bin(codes, 64, q, seg, 300, ws, outs, i32(1))              # a ragged table needs rows
    with pytest.raises(_lib.DrnError, match="shortlist_bin: seg must be"):
        ops.shortlist_bin(codes, 64, q, seg[:2], 300, ws, outs, i32(1))
    with pytest.raises(_lib.DrnError, match="shortlist_bin: vid_blk must be"):
        ops.shortlist_bin(codes, 64, q, (seg[0], seg[1], i32(4)), 300, ws, outs + (i32(3, 300),), i32(1))
    for s, o, W in (((), outs, 2), (seg, outs + (i32(3, 300),), 1)):
        for good in (i32(W), i32(3, W)):
            with pytest.raises(AssertionError, match="the library was reached"):
                ops.shortlist_bin(codes, 64, q, s, 300, ws, o, good)


# -- 4. the C boundary -------------------------------------------------------------------------------------------------------------------------

def test_library_declares_and_exports_the_binary_entry_at_abi_9():
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    name = "drn_shortlist_bin"
    assert name in _lib.declared_symbols() and hasattr(lib, name)
    params, sig = _header_params(name), _lib.SIGNATURES[name]
    assert len(params) == len(sig) == 21, params
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(lib.drn_shortlist_bin.argtypes) == list(sig) and callable(ops.shortlist_bin)
    # drn_shortlist_deep's parameters without its scales
    deep = _header_params("drn_shortlist_deep")
    assert params[0] == "const int32_t* codes" and params[1:] == deep[2:]
    header = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert int(re.search(r"#define DRN_BINARY_MAX_E\s+(\d+)", header).group(1)) == _lib.BINARY_MAX_E


def test_the_binary_entry_checks_its_arguments_before_anything_is_launched():
    """EVERY call below fails validation: a call with these placeholder pointers that passed it would launch on a machine with a GPU."""
    L = built_lib()
    p = ctypes.c_void_p(0x1000)
    # codes queries offsets blk_vid vid_blk allow ws | ids scores counts rows
    CODES, QUERIES, OFFSETS, BLK_VID, VID_BLK, ALLOW, WS, IDS, SCORES, COUNTS, ROWS = range(11)
    RAGGED = (OFFSETS, BLK_VID, VID_BLK, ROWS)

    def bin_(ragged=False, R=900, V=300, nblocks=2, E=64, S=2, n=300, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        changed = dict(R=R, V=V, nblocks=nblocks, E=E, S=S, n=n, dtype=dtype, keys=keys, stride=stride) != dict(
            R=900, V=300, nblocks=2, E=64, S=2, n=300, dtype=1, keys=1 << 20, stride=0)
        assert changed or ptrs, "a call that would pass validation"
        a = [p] * 11
        if not ragged:
            for i in RAGGED:
                a[i] = None
        for i, value in (ptrs or {}).items():
            a[i] = value
        return L.drn_shortlist_bin(a[0], a[1], a[2], a[3], a[4], a[5], stride, R, V, nblocks, E, S, n, dtype, a[6], keys, a[7], a[8], a[9], a[10], None)
    err = L.drn_last_error
    for ragged in (False, True):
        fn = lambda **kw: bin_(ragged=ragged, **kw)
        needed = [CODES, QUERIES, ALLOW, WS, IDS, SCORES, COUNTS] + (list(RAGGED) if ragged else [])
        for i in needed:
            assert fn(ptrs={i: None}) != 0 and b"drn_shortlist_bin" in err() and b"null pointer" in err(), (ragged, i)
        if not ragged:                                                           # half a ragged argument set, either half
            for i in (BLK_VID, VID_BLK, ROWS):
                assert fn(ptrs={i: p}) != 0 and b"null pointer" in err() and b"offsets is NULL" in err(), i
            assert fn(ptrs={OFFSETS: p}) != 0 and b"null pointer" in err()
        assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in err()
        for E in (4097, 1 << 20):
            assert fn(E=E) != 0 and b"drn_shortlist_bin: E = %d columns above 4096" % E in err()
        for n in (0, -1, 1025):
            assert fn(n=n) != 0 and b"drn_shortlist_bin: n = %d outside [1, 1024]" % n in err()
        for dtype in (-1, 2):
            assert fn(dtype=dtype) != 0 and b"dtype" in err()
        assert fn(ptrs={CODES: ctypes.c_void_p(0x1004)}) != 0 and b"16-byte aligned" in err()
        assert fn(ptrs={QUERIES: ctypes.c_void_p(0x1008)}) != 0 and b"16-byte aligned" in err()
        assert fn(ptrs={WS: ctypes.c_void_p(0x1004)}) != 0 and b"8-byte aligned" in err()
        for stride in (1, 9, 11, -10, 300):
            assert fn(stride=stride) != 0 and b"neither 0" in err() and b"ceil(V / 32) = 10" in err(), stride
        for off in (1, 2, 3):
            assert fn(ptrs={ALLOW: ctypes.c_void_p(0x1000 + off)}) != 0 and b"mask must be 4-byte aligned" in err()
        if ragged:
            assert fn(R=0) != 0 and b"bad args" in err()
            for nblocks in (0, 1, 301):
                assert fn(nblocks=nblocks) != 0 and b"blocks outside" in err(), nblocks
            # 2 sentences x 2 blocks x min(300, 256) = 1024 keys, and half as many again for the segments
            assert fn(keys=1535) != 0 and b"1536 are needed" in err()
            assert fn(n=1024, keys=1535) != 0 and b"1536 are needed" in err()
            assert fn(n=129, keys=2 * 2 * 129 + 258 - 1) != 0 and b"774 are needed" in err()
        else:
            assert fn(keys=1023) != 0 and b"1024 are needed" in err()
            assert fn(keys=1023, stride=10) != 0 and b"1024 are needed" in err()
            assert fn(n=129, keys=2 * 2 * 129 - 1) != 0 and b"516 are needed" in err()
            assert fn(nblocks=0, keys=0) != 0 and b"1024 are needed" in err()     # (nblocks is ignored without offsets)
            assert fn(V=1 << 30, S=1 << 10, n=1024, keys=0x7fffffff) != 0 and b"are needed" in err()             # (no int overflow)
        assert fn(S=16 * 65535 + 1, n=1, keys=0x7fffffff) != 0 and b"more than 65535 tiles" in err()


# -- 5. the compiler's resource notes ---------------------------------------------------------------------------------------------------------

def test_the_binary_kernels_spill_nothing_and_hold_the_lds_their_comments_state(tmp_path):
    """csrc/retrieve_bin.hip compiled for gfx950 on its own: the two kernels in their four instances each (bf16 / fp32 queries, 16-byte /
    word loads), each without scratch and without a spilled register, at most 128 VGPRs + AGPRs, and static LDS exactly what the arrays
    come to, which is the size the comment above each kernel states."""
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_bin.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_bin.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_bin.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shortlist_bin_block_kernel", "shortlist_bin_segments_kernel"]
    keys, qc, bad = 16 * 256 * 8, 16 * 128 * 4, 16 * 4
    claims = {"shortlist_bin_block_kernel": keys + qc + 16 * 8 * 4 + bad,
              "shortlist_bin_segments_kernel": keys + 16 * 257 * 4 + qc + 260 * 4 + 16 * 9 * 4 + bad + 4 * 4}
    assert claims == {"shortlist_bin_block_kernel": 41536, "shortlist_bin_segments_kernel": 59104}
    stated = [int(x.replace(",", "")) for x in re.findall(r"// Static LDS:[^\n]*= ([\d,]+) B\.", src)]
    assert stated == [claims["shortlist_bin_block_kernel"], claims["shortlist_bin_segments_kernel"]]
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == 8, sorted(seen)
    for kernel, lds_claim in claims.items():
        mine = [v for k, v in seen.items() if kernel in k]
        assert len(mine) == 4, (kernel, sorted(seen))
        for lds, scratch, vspill, sspill, regs in mine:
            assert scratch == 0 and vspill == 0 and sspill == 0, (kernel, scratch, vspill, sspill)
            assert lds == lds_claim and regs <= 128, (kernel, lds, regs)
