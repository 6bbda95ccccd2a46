"""Asymmetric binary shortlists, the host side: the definition binary_asym_shortlist_reference (drn_amd/binary.py) against the float64
references over the dequantised table, a ranking written out by hand, the planted-neighbour fixture that says why the scoring exists,
every refusal of BinaryShortlister.shortlist_asym, of the asymmetric() view and of ops.shortlist_bin_asym before the library is reached,
the C entry drn_shortlist_bin_asym at ABI 9 with its argument checks -- by calls that FAIL validation only: nothing here may launch --
and the compiler's resource notes for csrc/retrieve_bin_asym.hip.  tests/test_binary_asym_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from drn_amd.binary import (BinaryShortlister, binary_asym_shortlist_reference, binary_dequantize, binary_quantize_reference,
                            binary_shortlist_reference)
from test_allow_shortlist_cpu import same
from test_binary_shortlist_cpu import ragged_offsets, table
from test_grounding_cpu import _header_params, built_lib
from test_q8_shortlist_cpu import _no_library, resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- 1. the definition -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [8, 32, 40, 96])
def test_the_definition_is_the_float64_references_over_the_dequantised_table(E):
    """Plain and ragged (runs cycling 1 / 3 / 0 / 17: videos without rows among them); no mask, a shared mask, a mask per sentence with an
    all-zero row.  The queries are scored AS THEY ARE: float32 and bfloat16 queries alike are widened, never binarised."""
    from drn_amd import segment_shortlist_reference, shortlist_reference
    R, S = 300, 6
    x, q = table(R, E), table(S, E, seed=3)
    codes = binary_quantize_reference(x)
    wide = binary_dequantize(codes, E, torch.float64)
    off = ragged_offsets(R)
    V = len(off) - 1
    assert bool((np.diff(off) == 0).any())
    g = torch.Generator().manual_seed(E)
    for rows, offsets in ((R, None), (V, off)):
        per = torch.rand(S, rows, generator=g) < 0.5
        per[2] = False
        for allow in (None, per[0].clone(), per):
            for n in (1, 7, 128, 400):
                for queries in (q, q.bfloat16()):
                    got = binary_asym_shortlist_reference(codes, E, queries, n, offsets=offsets, allow=allow)
                    want = (shortlist_reference(wide, queries.double(), n, allow=allow) if offsets is None
                            else segment_shortlist_reference(wide, offsets, queries.double(), n, allow=allow))
                    same(got, want, (E, offsets is not None, None if allow is None else allow.dim(), n, queries.dtype))
                    assert got.ids.dtype == torch.int32 and got.scores.dtype == torch.float32 and got.n.dtype == torch.int32
                    if allow is per:
                        assert got.n[2] == 0
                    assert int(got.n[0]) > 0
    # it is NOT the Hamming definition: the magnitudes count
    assert not torch.equal(binary_asym_shortlist_reference(codes, E, q, 7).scores, binary_shortlist_reference(codes, E, q, 7).scores)


def test_a_ranking_written_out_by_hand_with_planted_ties():
    """Five rows over E = 8: rows 1 and 2 are twins, row 3 is row 0 negated.  Plain: ties go to the lower position.  Ragged, videos
    {0}, {1, 2}, {}, {3, 4}: video 1's twins tie and `rows` names segment 0; video 2 owns no row and is never listed."""
    signs = torch.tensor([[+1, +1, +1, +1, +1, +1, +1, +1],
                          [+1, +1, +1, +1, -1, -1, -1, -1],
                          [+1, +1, +1, +1, -1, -1, -1, -1],
                          [-1, -1, -1, -1, -1, -1, -1, -1],
                          [+1, -1, +1, -1, +1, -1, +1, -1]], dtype=torch.float32)
    codes = binary_quantize_reference(signs)
    assert codes.tolist() == [[0xff], [0x0f], [0x0f], [0x00], [0x55]]
    q = torch.tensor([[1, 2, 3, 4, .5, .5, .5, .5],             # scores 12, 8, 8, -12, -2
                      [0, 0, 0, 0, 1, 1, 1, 1]])                # scores 4, -4, -4, -4, 0
    got = binary_asym_shortlist_reference(codes, 8, q, 6)
    assert got.ids.tolist() == [[0, 1, 2, 4, 3, -1], [0, 4, 1, 2, 3, -1]]
    assert got.scores.tolist() == [[12., 8., 8., -2., -12., 0.], [4., 0., -4., -4., -4., 0.]]
    assert got.n.tolist() == [5, 5]
    assert binary_asym_shortlist_reference(codes, 8, q, 2).ids.tolist() == [[0, 1], [0, 4]]
    rag = binary_asym_shortlist_reference(codes, 8, q, 4, offsets=[0, 1, 3, 3, 5])
    assert rag.ids.tolist() == [[0, 1, 3, -1], [0, 3, 1, -1]]
    assert rag.scores.tolist() == [[12., 8., -2., 0.], [4., 0., -4., 0.]]
    assert rag.rows.tolist() == [[0, 0, 1, -1], [0, 1, 0, -1]] and rag.n.tolist() == [3, 3]
    mask = torch.tensor([[True, False, True, True], [False, True, True, True]])
    cut = binary_asym_shortlist_reference(codes, 8, q, 4, offsets=[0, 1, 3, 3, 5], allow=mask)
    assert cut.ids.tolist() == [[0, 3, -1, -1], [3, 1, -1, -1]] and cut.rows.tolist() == [[0, 1, -1, -1], [1, 0, -1, -1]]


def test_a_query_row_that_is_not_finite_lists_nothing_and_leaves_the_others_alone():
    """Every score of such a row is a sum with an infinity or a NaN among its terms: none is finite, so the references list nothing."""
    E, R = 40, 300
    x, q = table(R, E), table(6, E, seed=5)
    codes = binary_quantize_reference(x)
    bad = q.clone()
    bad[1, E // 2], bad[3, 0], bad[4, E - 1] = float("nan"), float("inf"), float("-inf")
    off = ragged_offsets(R)
    for offsets in (None, off):
        clean = binary_asym_shortlist_reference(codes, E, q, 50, offsets=offsets)
        got = binary_asym_shortlist_reference(codes, E, bad, 50, offsets=offsets)
        for s in (1, 3, 4):
            assert int(got.n[s]) == 0 and bool((got.ids[s] == -1).all()) and bool((got.scores[s] == 0).all())
        if offsets is not None:
            assert bool((got.rows[[1, 3, 4]] == -1).all())
        for f in got._fields:
            assert torch.equal(getattr(got, f)[[0, 2, 5]], getattr(clean, f)[[0, 2, 5]]), f
        owners = R if offsets is None else int((np.diff(off) > 0).sum())
        assert got.n[[0, 2, 5]].tolist() == [min(50, owners)] * 3


def test_asymmetric_scoring_recalls_more_planted_neighbours_than_hamming():
    """x ~ N(0, 1), q = x[target] + 1.5 noise: the planted video is in the asymmetric list of 10 strictly more often than in the Hamming
    list of 10 over the same codes.  (Synthetic data: the direction, not a figure, is asserted.)"""
    V, E, S, sigma, n = 2048, 64, 256, 1.5, 10
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(V, E, generator=g)
    target = torch.randperm(V, generator=g)[:S]
    q = x[target] + sigma * torch.randn(S, E, generator=g)
    codes = binary_quantize_reference(x)

    def recall(lists):
        return float((lists.ids.long() == target[:, None]).any(dim=1).double().mean())
    hamming = recall(binary_shortlist_reference(codes, E, q, n))
    asym = recall(binary_asym_shortlist_reference(codes, E, q, n))
    print("recall@%d of the planted video: Hamming %.3f, asymmetric %.3f" % (n, hamming, asym))
    assert asym > hamming


def test_the_definition_refuses_what_binary_shortlist_reference_refuses():
    from drn_amd import _lib
    codes = binary_quantize_reference(table(4, 40))
    for c, E in ((codes, 97), (codes, 65), (codes, 32), (codes, 0), (codes.long(), 40), (codes[0], 40)):
        with pytest.raises(_lib.DrnError, match="binary_asym_shortlist_reference: codes must be int32"):
            binary_asym_shortlist_reference(c, E, torch.zeros(2, 40), 3)
    for bad in (torch.zeros(2, 41), torch.zeros(40), torch.zeros(0, 40), [[0.0] * 40]):
        with pytest.raises(_lib.DrnError, match=r"binary_asym_shortlist_reference: the queries must be a float tensor \(S, 40\)"):
            binary_asym_shortlist_reference(codes, 40, bad, 3)
    with pytest.raises(_lib.DrnError, match="end at R = 4"):
        binary_asym_shortlist_reference(codes, 40, torch.zeros(2, 40), 3, offsets=[0, 5])


# -- 2. the interface --------------------------------------------------------------------------------------------------------------------------

def test_the_public_names_and_the_view():
    import drn_amd
    from drn_amd import _lib
    for name in ("binary_asym_shortlist_reference", "AsymmetricBinaryView", "BinaryShortlister"):
        assert getattr(drn_amd, name) is getattr(drn_amd.binary, name), name
    assert BinaryShortlister.shortlist_deep is BinaryShortlister.shortlist and BinaryShortlister.shortlist_asym is not BinaryShortlister.shortlist
    names = ["v%d" % v for v in range(3)]
    sl = BinaryShortlister.from_codes(resident(binary_quantize_reference(table(40, 96))), 96, torch.bfloat16, names=names, offsets=[0, 2, 2, 40])
    view = sl.asymmetric()
    assert isinstance(view, drn_amd.AsymmetricBinaryView) and view.base is sl
    assert view.codes is sl.codes and view.names is sl.names and view.offsets is sl.offsets and view.plan is sl.plan, "something was copied"
    assert len(view) == 3 and view.E == 96 and view.dtype == torch.bfloat16 and view.device == sl.device and view.nbytes == sl.nbytes
    assert type(view).shortlist_deep is type(view).shortlist and hasattr(view, "dequantized")
    assert view.allow_of(drop=[1]).tolist() == [5] and view.allow_of(keep=["v0"]).tolist() == [1]

    class Store(object):
        pass
    Store.names = names
    view.check(Store)
    Store.names = names[::-1]
    with pytest.raises(_lib.DrnError, match="names are not the store's"):
        view.check(Store)
    with pytest.raises(_lib.DrnError, match="AsymmetricBinaryView: the table must be a BinaryShortlister"):
        drn_amd.AsymmetricBinaryView(view)


def test_the_module_still_never_imports_the_oracle():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "drn_amd", "binary.py")).read())
    mods = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            mods.append(node.module or "")
    assert mods and not any(m.split(".")[0] == "oracle" for m in mods), mods


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "segments"])
def test_shortlist_asym_and_the_view_refuse_before_the_library_is_reached(monkeypatch, ragged):
    from drn_amd import _lib
    _no_library(monkeypatch)
    codes = resident(binary_quantize_reference(table(40, 64)))
    sl = BinaryShortlister.from_codes(codes, 64, torch.bfloat16, offsets=[0, 2, 2, 40] if ragged else None)
    view = sl.asymmetric()
    W = 1 if ragged else 2
    q = resident(torch.zeros(3, 64, dtype=torch.bfloat16))
    what = "BinaryShortlister.shortlist_asym"
    for fn in (sl.shortlist_asym, view.shortlist, view.shortlist_deep):
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
            fn(q, 300, allow=resident(torch.zeros(W + 1, dtype=torch.int32)))      # a mask of the wrong width
        with pytest.raises(_lib.DrnError, match=r"allow must be \(%d,\)" % W):
            fn(q, 300, allow=resident(torch.zeros(3, W + 1, dtype=torch.int32)))
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
    fn = ops.shortlist_bin_asym
    with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: allow is required"):
        fn(codes, 64, q, (), 300, ws, outs, None)
    with pytest.raises(_lib.DrnError, match="GPU only"):
        fn(codes, 64, q, (), 300, ws, outs, torch.zeros(2, dtype=torch.int32))
    for E in (0, 4097):
        with pytest.raises(_lib.DrnError, match=r"shortlist_bin_asym: E = %d outside \[1, 4096\]" % E):
            fn(codes, E, q, (), 300, ws, outs, i32(2))
    for bad, E in ((codes, 32), (codes, 65), (resident(torch.zeros(40, 2, dtype=torch.int64)), 64), (i32(2), 64), (i32(2, 40).t(), 64)):
        with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: codes must be a contiguous"):
            fn(bad, E, resident(torch.zeros(3, E)), (), 300, ws, outs, i32(2))
    for bad in (resident(torch.zeros(3, 63)), resident(torch.zeros(64)), resident(torch.zeros(3, 64, dtype=torch.float16)), i32(3, 64)):
        with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: queries must be a contiguous"):
            fn(codes, 64, bad, (), 300, ws, outs, i32(2))
    for n in (0, 1025):
        with pytest.raises(_lib.DrnError, match=r"shortlist_bin_asym: n = %d outside \[1, 1024\]" % n):
            fn(codes, 64, q, (), n, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: ws must be a contiguous int64 tensor of at least 768"):
        fn(codes, 64, q, (), 300, ws[:767], outs, i32(2))                        # 3 sentences x 1 block x min(300, 256) keys
    with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: ws must be a contiguous int64 tensor of at least 1152"):
        fn(codes, 64, q, seg, 300, ws[:1151], outs + (i32(3, 300),), i32(1))     # and half as many again
    with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: allow must be a contiguous torch.int32 tensor"):
        fn(codes, 64, q, (), 300, ws, outs, i32(3))
    with pytest.raises(_lib.DrnError, match="shortlist_bin_asym: seg must be"):
        fn(codes, 64, q, seg, 300, ws, outs, i32(1))                            # a ragged table needs rows
    for s, o, W in (((), outs, 2), (seg, outs + (i32(3, 300),), 1)):
        for good in (i32(W), i32(3, W)):
            with pytest.raises(AssertionError, match="the library was reached"):
                fn(codes, 64, q, s, 300, ws, o, good)


# -- 3. the C boundary -------------------------------------------------------------------------------------------------------------------------

def test_library_declares_and_exports_the_asymmetric_entry_at_abi_9():
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    name = "drn_shortlist_bin_asym"
    assert name in _lib.declared_symbols() and hasattr(lib, name)
    params, sig = _header_params(name), _lib.SIGNATURES[name]
    assert len(params) == len(sig) == 21, params
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(lib.drn_shortlist_bin_asym.argtypes) == list(sig) and callable(ops.shortlist_bin_asym)
    assert params == _header_params("drn_shortlist_bin"), "the argument list is drn_shortlist_bin's"
    assert list(sig) == list(_lib.SIGNATURES["drn_shortlist_bin"])


def test_the_asymmetric_entry_checks_its_arguments_before_anything_is_launched():
    """EVERY call below fails validation: a call with these placeholder pointers that passed it would launch on a machine with a GPU."""
    L = built_lib()
    p = ctypes.c_void_p(0x1000)
    # codes queries offsets blk_vid vid_blk allow ws | ids scores counts rows
    CODES, QUERIES, OFFSETS, BLK_VID, VID_BLK, ALLOW, WS, IDS, SCORES, COUNTS, ROWS = range(11)
    RAGGED = (OFFSETS, BLK_VID, VID_BLK, ROWS)
    DEFAULTS = dict(R=900, V=300, nblocks=2, E=64, S=2, n=300, dtype=1, keys=1 << 20, stride=0)

    def asym(ragged=False, ptrs=None, **kw):
        assert set(kw) <= set(DEFAULTS)
        a = dict(DEFAULTS, **kw)
        assert a != DEFAULTS or ptrs, "a call that would pass validation"
        ptr = [p] * 11
        if not ragged:
            for i in RAGGED:
                ptr[i] = None
        for i, value in (ptrs or {}).items():
            ptr[i] = value
        return L.drn_shortlist_bin_asym(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], a["stride"], a["R"], a["V"], a["nblocks"], a["E"], a["S"],
                                        a["n"], a["dtype"], ptr[6], a["keys"], ptr[7], ptr[8], ptr[9], ptr[10], None)
    err = L.drn_last_error
    for ragged in (False, True):
        fn = lambda **kw: asym(ragged=ragged, **kw)
        needed = [CODES, QUERIES, ALLOW, WS, IDS, SCORES, COUNTS] + (list(RAGGED) if ragged else [])
        for i in needed:
            assert fn(ptrs={i: None}) != 0 and b"drn_shortlist_bin_asym" in err() and b"null pointer" in err(), (ragged, i)
        if not ragged:                                                           # half a ragged argument set, either half
            for i in (BLK_VID, VID_BLK, ROWS):
                assert fn(ptrs={i: p}) != 0 and b"null pointer" in err() and b"offsets is NULL" in err(), i
            assert fn(ptrs={OFFSETS: p}) != 0 and b"null pointer" in err()
        assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in err()
        for E in (4097, 1 << 20):
            assert fn(E=E) != 0 and b"drn_shortlist_bin_asym: E = %d columns above 4096" % E in err()
        for n in (0, -1, 1025):
            assert fn(n=n) != 0 and b"drn_shortlist_bin_asym: n = %d outside [1, 1024]" % n in err()
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


# -- 4. the compiler's resource notes ---------------------------------------------------------------------------------------------------------

def test_the_asymmetric_kernels_spill_nothing_and_hold_the_lds_their_comments_state(tmp_path):
    """csrc/retrieve_bin_asym.hip compiled for gfx950 on its own: the two kernels in their four instances each (bf16 / fp32 queries,
    16-byte / word loads), each without scratch and without a spilled register, and static LDS exactly what the arrays come to, which
    is the size the comment above each kernel states."""
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_bin_asym.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_bin_asym.hip"],
                   cwd=os.path.join(ROOT, "drn_amd", "csrc"), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_bin_asym.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shortlist_bin_asym_block_kernel", "shortlist_bin_asym_segments_kernel"]
    keys = 16 * 256 * 8
    claims = {"shortlist_bin_asym_block_kernel": keys + 16 * 8 * 4,
              "shortlist_bin_asym_segments_kernel": keys + 16 * 257 * 4 + 260 * 4 + 16 * 9 * 4 + 4 * 4}
    assert claims == {"shortlist_bin_asym_block_kernel": 33280, "shortlist_bin_asym_segments_kernel": 50848}
    stated = [int(x.replace(",", "")) for x in re.findall(r"// Static LDS:[^\n]*= ([\d,]+) B\.", src)]
    assert stated == [claims["shortlist_bin_asym_block_kernel"], claims["shortlist_bin_asym_segments_kernel"]]
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"))
    assert len(seen) == 8, sorted(seen)
    for kernel, lds_claim in claims.items():
        mine = [v for k, v in seen.items() if kernel in k]
        assert len(mine) == 4, (kernel, sorted(seen))
        for lds, scratch, vspill, sspill in mine:
            assert scratch == 0 and vspill == 0 and sspill == 0, (kernel, scratch, vspill, sspill)
            assert lds == lds_claim, (kernel, lds)
