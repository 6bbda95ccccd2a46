"""Reranking a candidate list, the host side: candidates_mask (what a candidates tensor means) and the three rerank references on a
hand-written case, each against its parent reference under allow = mask; the refusals of Shortlister.rerank / rerank_late and of
evaluate_cascade that need no GPU; the C entry drn_shortlist_rerank at ABI 9 and its argument checks.
tests/test_rerank_shortlist_gpu.py holds the kernel."""
import ctypes
import os
import re

import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_late_shortlist_cpu import Resident, _no_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "drn_shortlist_rerank"


# -- the definition ----------------------------------------------------------------------------------------------------------------------

def hand_case():
    """V = 5 videos of one row, E = 2.  Against the query (1, 0) the scores are 3, 1, 3, 2, 5: videos 0 and 2 tie.  The first list
    holds 2 before 0 (the tie must still fall by position), a repeat of 2, a -1 and an id equal to V; the second lists video 4 alone,
    among padding."""
    emb = torch.tensor([[3., 0.], [1., 1.], [3., 2.], [2., 0.], [5., 1.]])
    q = torch.tensor([[1., 0.], [1., 0.]])
    cand = torch.tensor([[2, 3, 2, -1, 0, 5], [-1, 4, -1, -1, 7, -9]], dtype=torch.int32)
    return emb, q, cand


def test_candidates_mask_on_a_hand_written_case():
    from drn_amd import _lib, candidates_mask
    _, _, cand = hand_case()
    mask = candidates_mask(cand, 5)
    assert mask.dtype == torch.bool and mask.shape == (2, 5) and mask.is_contiguous()
    assert mask.tolist() == [[True, False, True, True, False], [False, False, False, False, True]]
    # int64 lists, a value of 2^31 - 1, an all-padding row, V = 1
    assert candidates_mask(torch.tensor([[2 ** 31 - 1, 0], [-1, -1]]), 1).tolist() == [[True], [False]]
    # the order of a row, repeats and padding mean nothing
    assert torch.equal(candidates_mask(torch.tensor([[0, 3, 2]]), 5), candidates_mask(torch.tensor([[2, -1, 3, 3, 0, 9, 2]]), 5))
    for bad in (torch.zeros(2, 3), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.bool), [[1, 2]]):
        with pytest.raises(_lib.DrnError, match=r"integer tensor \(S, C\)"):
            candidates_mask(bad, 5)


def test_rerank_reference_on_the_hand_written_case():
    from drn_amd import Shortlist, rerank_reference
    emb, q, cand = hand_case()
    got = rerank_reference(emb, cand, q, 8)                                   # n = 8 > C = 6
    assert isinstance(got, Shortlist) and got.ids.shape == got.scores.shape == (2, 8) and got.n.shape == (2,)
    assert got.ids.dtype == got.n.dtype == torch.int32 and got.scores.dtype == torch.float32
    # sentence 0 lists {0, 2, 3}: 0 and 2 tie at 3 and fall by POSITION though the list names 2 first; 4, the best video, is not listed
    assert got.ids[0].tolist() == [0, 2, 3, -1, -1, -1, -1, -1] and got.scores[0].tolist() == [3., 3., 2., 0., 0., 0., 0., 0.]
    assert got.ids[1].tolist() == [4] + [-1] * 7 and got.scores[1].tolist() == [5.] + [0.] * 7 and got.n.tolist() == [3, 1]
    cut = rerank_reference(emb, cand, q, 2)
    assert cut.ids.tolist() == [[0, 2], [4, -1]] and cut.n.tolist() == [2, 1]
    # a mask combines with the list: shared, and per sentence
    shared = rerank_reference(emb, cand, q, 3, allow=torch.tensor([False, True, True, True, True]))
    assert shared.ids.tolist() == [[2, 3, -1], [4, -1, -1]] and shared.n.tolist() == [2, 1]
    per = rerank_reference(emb, cand, q, 3, allow=torch.tensor([[True] * 5, [True, True, True, True, False]]))
    assert per.ids.tolist() == [[0, 2, 3], [-1, -1, -1]] and per.n.tolist() == [3, 0]


def test_segment_and_late_rerank_references_on_a_hand_written_case():
    from drn_amd import Shortlist, late_rerank_reference, segment_rerank_reference
    # V = 5: video 1 owns no row; rows along the axes
    emb = torch.tensor([[3., 0.], [0., 3.], [2., 2.], [1., 1.], [-1., 0.], [3., 3.]])
    off = [0, 2, 2, 3, 5, 6]
    q = torch.tensor([[[1., 0.], [0., 1.]], [[1., 0.], [0., 1.]]])
    cand = torch.tensor([[3, 1, 0, 3, 5], [4, 2, -1, 2, 0]], dtype=torch.int32)
    seg = segment_rerank_reference(emb, off, cand, q[:, 0].contiguous(), 6)
    assert isinstance(seg, Shortlist) and seg._fields == ("ids", "scores", "n")
    # best rows against (1, 0): v0 = 3, v2 = 2, v3 = 1, v4 = 3; a listed video without rows (1) is no candidate
    assert seg.ids.tolist() == [[0, 3, -1, -1, -1, -1], [0, 4, 2, -1, -1, -1]] and seg.n.tolist() == [2, 3]
    assert seg.scores.tolist() == [[3., 1., 0., 0., 0., 0.], [3., 3., 2., 0., 0., 0.]]
    late = late_rerank_reference(emb, off, cand, q, [2, 1], 2)
    # sentence 0, both tokens: v0 = 3 + 3, v3 = 1 + 1; sentence 1, one token: the segment scores, 0 and 4 tie by position
    assert late.ids.tolist() == [[0, 3], [0, 4]] and late.scores.tolist() == [[6., 2.], [3., 3.]] and late.n.tolist() == [2, 2]
    assert late_rerank_reference(emb, off, cand, q, [0, 2], 2).n.tolist() == [0, 2]     # a sentence without a live token lists nothing


def test_each_reference_is_its_parent_under_allow_equal_to_the_mask():
    from drn_amd import (candidates_mask, late_rerank_reference, late_shortlist_reference, rerank_reference, segment_rerank_reference,
                         segment_shortlist_reference, shortlist_reference)
    g = torch.Generator().manual_seed(11)
    lens = [1, 3, 0, 4, 2, 0, 1, 2]
    V, R = len(lens), sum(lens)
    off = [0] + torch.tensor(lens).cumsum(0).tolist()
    emb = torch.randint(-4, 5, (R, 8), generator=g).float()
    emb[4], emb[9] = emb[0], emb[1]                                          # planted equal scores across videos
    tok = torch.randint(-4, 5, (3, 4, 8), generator=g).float()
    tok[1, 3, 2] = float("nan")                                              # (a dead token of sentence 1 below)
    lengths = [4, 3, 0]
    cand = torch.tensor([[7, 3, 3, -1, 0, 8, 1, 2], [-1, -1, 6, 4, 6, 99, -5, 4], [-1] * 8], dtype=torch.int32)
    mask = candidates_mask(cand, V)
    allow = torch.tensor([True, True, True, False, True, True, True, True])
    q = tok[:, 0].contiguous()
    for n in (1, 3, 9):
        for extra in (None, allow):
            both = mask if extra is None else mask & extra
            a, b = segment_rerank_reference(emb, off, cand, q, n, allow=extra), segment_shortlist_reference(emb, off, q, n, allow=both)
            c, d = late_rerank_reference(emb, off, cand, tok, lengths, n, allow=extra), late_shortlist_reference(emb, off, tok, lengths, n, allow=both)
            e, f = rerank_reference(emb[:V], cand, q, n, allow=extra), shortlist_reference(emb[:V], q, n, allow=both)
            for got, want in ((a, b), (c, d), (e, f)):
                for field in ("ids", "scores", "n"):
                    assert torch.equal(getattr(got, field), getattr(want, field)), (n, field)
            assert int(a.n[2]) == 0 and int(c.n[2]) == 0 and int(e.n[2]) == 0   # an all-padding row lists nothing


# -- refusals, before the library is reached -------------------------------------------------------------------------------------------------

def _resident(t):
    return t.as_subclass(Resident)


def _stand_in(ragged=True, quantize=None, resident=True):
    """A table that only stands in for a resident one (the constructor was not run): V = 3 videos, E = 32."""
    from drn_amd import Shortlister
    sl = Shortlister.__new__(Shortlister)
    sl.names, sl._ws = ["a", "b", "c"], {}
    rows = 6 if ragged else 3
    sl._seg = None
    if ragged:
        sl._seg = (torch.tensor([0, 2, 2, 6], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    put = _resident if resident else (lambda t: t)
    if quantize is None:
        sl.embeddings = put(torch.zeros(rows, 32, dtype=torch.bfloat16))
    else:
        sl.embeddings, sl.quantize, sl._dtype = None, quantize, torch.float32
        sl.codes, sl.scales = put(torch.zeros(rows, 32, dtype=torch.uint8)), put(torch.zeros(rows, 1, dtype=torch.uint8))
    return sl


def test_rerank_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    import drn_amd
    from drn_amd import _lib
    _no_library(monkeypatch)
    assert _lib.RERANK_MAX_CANDIDATES == _lib.CANDIDATES_MAX == 1024 and _lib.RERANK_GROUP == 16
    cand = torch.tensor([[0, 2, -1, 1], [1, 1, 0, 7]], dtype=torch.int32)
    rc = _resident(cand)
    q = torch.zeros(2, 32, dtype=torch.bfloat16)
    rq = _resident(q)
    tok = _resident(torch.zeros(2, 3, 32, dtype=torch.bfloat16))
    rl = _resident(torch.tensor([3, 1], dtype=torch.int32))
    for ragged in (True, False):
        sl = _stand_in(ragged)
        calls = [("rerank", lambda c, n=None, **kw: sl.rerank(c, rq, n, **kw))]
        if ragged:
            calls.append(("rerank_late", lambda c, n=None, **kw: sl.rerank_late(c, tok, rl, n, **kw)))
        for name, call in calls:
            with pytest.raises(_lib.DrnError, match="%s: candidates must be a tensor" % name):
                call([[0, 1], [1, 2]])
            for bad in (cand.bool(), cand.long(), cand.float()):
                with pytest.raises(_lib.DrnError, match="candidates must be torch.int32"):
                    call(_resident(bad))
            for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(2, 2, 2, dtype=torch.int32)):
                with pytest.raises(_lib.DrnError, match=r"candidates must be \(S, C\)"):
                    call(_resident(bad))
            for C in (0, 1025):
                with pytest.raises(_lib.DrnError, match=r"C = %d candidates a sentence outside \[1, 1024\]" % C):
                    call(_resident(torch.zeros(2, C, dtype=torch.int32)))
            with pytest.raises(_lib.DrnError, match="candidates must be on the table's device"):
                call(cand)                                                   # a host list
            with pytest.raises(_lib.DrnError, match="candidates must be contiguous"):
                call(_resident(torch.zeros(2, 8, dtype=torch.int32)[:, ::2]))
            for n in (0, -1, 129):
                with pytest.raises(_lib.DrnError, match=r"n = %d outside \[1, 128\]" % n):
                    call(rc, n)
            # the wrong S: three rows of candidates for two sentences
            with pytest.raises(_lib.DrnError, match="a row per row of candidates|the queries hold 2 sentences, candidates has 3 rows"):
                call(_resident(torch.zeros(3, 4, dtype=torch.int32)))
            # out=: three buffers, each of its shape and dtype (n = None: min(C, 128) = 4)
            good = lambda: [_resident(torch.zeros((2, 4), dtype=torch.int32)), _resident(torch.zeros((2, 4))),
                            _resident(torch.zeros((2,), dtype=torch.int32))]
            with pytest.raises(_lib.DrnError, match="three buffers"):
                call(rc, out=good() + [_resident(torch.zeros((2, 4), dtype=torch.int32))])
            for i, field in enumerate(("ids", "scores", "n")):
                for wrong in (_resident(torch.zeros((2, 5), dtype=torch.int32)), _resident(torch.zeros((2, 4), dtype=torch.float64)),
                              torch.zeros(good()[i].shape, dtype=good()[i].dtype), None):
                    out = good()
                    out[i] = wrong
                    with pytest.raises(_lib.DrnError, match="out.%s must be a contiguous" % field):
                        call(rc, out=out)
            for bad, match in ((torch.ones(3, dtype=torch.bool), "pack it first"), (torch.zeros(1, dtype=torch.int64), "torch.int32 packed words"),
                               ([1], "packed mask")):
                with pytest.raises(_lib.DrnError, match=match):
                    call(rc, allow=bad)
        # the queries of rerank: a tensor (S, E) of the table's dtype on its device
        with pytest.raises(_lib.DrnError, match="queries must be a tensor"):
            sl.rerank(rc, [[1.0]])
        for bad in (torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(2, 3, 32, dtype=torch.bfloat16), torch.zeros(32, dtype=torch.bfloat16)):
            with pytest.raises(_lib.DrnError, match=r"queries must be \(2, 32\)"):
                sl.rerank(rc, _resident(bad))
        with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
            sl.rerank(rc, _resident(q.float()))
        with pytest.raises(_lib.DrnError, match="no CPU fallback"):
            sl.rerank(rc, q)
    # the queries and lengths of rerank_late are refused as shortlist_late refuses them
    sl = _stand_in()
    with pytest.raises(_lib.DrnError, match=r"rerank_late: the queries must be \(S, L, 32\)"):
        sl.rerank_late(rc, rq, rl)
    with pytest.raises(_lib.DrnError, match=r"L = 65 tokens outside \[1, 64\]"):
        sl.rerank_late(rc, _resident(torch.zeros(2, 65, 32, dtype=torch.bfloat16)), rl)
    with pytest.raises(_lib.DrnError, match=r"lengths must be a contiguous \(2,\) torch.int32"):
        sl.rerank_late(rc, tok, _resident(torch.tensor([3, 1])))
    with pytest.raises(_lib.DrnError, match="never read on the host"):
        sl.rerank_late(rc, tok, torch.tensor([3, 1], dtype=torch.int32))
    # a table on the CPU, plain and quantised
    for host in (_stand_in(resident=False), _stand_in(False, resident=False), _stand_in(quantize="mxfp8", resident=False)):
        with pytest.raises(_lib.DrnError, match="rerank: the table must be on the GPU; there is no CPU fallback"):
            host.rerank(rc, rq)
    with pytest.raises(_lib.DrnError, match="rerank_late: the table must be on the GPU"):
        _stand_in(resident=False).rerank_late(rc, tok, rl)
    # a quantised table takes queries of the recorded dtype
    with pytest.raises(_lib.DrnError, match="the table is torch.float32"):
        _stand_in(quantize="mxfp8").rerank(rc, rq)
    # rerank_late on a table without offsets: shortlist_late's reason
    with pytest.raises(_lib.DrnError, match=r"rerank_late: this table has one row per video.*\(sum_t q_t\) \. emb_v.*call rerank\(\)"):
        _stand_in(False).rerank_late(rc, tok, rl)
    for public in ("candidates_mask", "rerank_reference", "segment_rerank_reference", "late_rerank_reference", "evaluate_cascade"):
        assert callable(getattr(drn_amd, public)), public


def test_evaluate_cascade_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, evaluate_cascade
    _no_library(monkeypatch)
    coarse, fine = _stand_in(False), _stand_in()

    def batches():
        raise AssertionError("a batch was read")
        yield
    for depth in (0, 129, -3):
        with pytest.raises(_lib.DrnError, match=r"depth = %d outside \[1, 128\]" % depth):
            evaluate_cascade(coarse, fine, batches(), depth)
    other = _stand_in()
    other.names = ["a", "c", "b"]
    nameless = _stand_in()
    nameless.names = None
    for a, b in ((coarse, other), (other, fine), (nameless, nameless)):
        with pytest.raises(_lib.DrnError, match="must carry the same names"):
            evaluate_cascade(a, b, batches(), 4)
    with pytest.raises(_lib.DrnError, match="at least one top-k"):
        evaluate_cascade(coarse, fine, batches(), 4, topks=())
    # a name the tables lack is refused on the host, before the batch's first launch
    with pytest.raises(_lib.DrnError, match="no video named zz"):
        evaluate_cascade(coarse, fine, [(["a", "zz"], None, None)], 4)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_rerank_entry_at_abi_9():
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    assert ENTRY in _lib.declared_symbols() and hasattr(lib, ENTRY)
    params, sig = _header_params(ENTRY), _lib.SIGNATURES[ENTRY]
    assert len(params) == len(sig) == 22, params
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(getattr(lib, ENTRY).argtypes) == list(sig)
    assert callable(ops.shortlist_rerank)
    for C, S, n in ((1, 1, 1), (16, 3, 128), (17, 3, 5), (1024, 7, 16), (33, 2, 20), (257, 64, 128)):
        assert ops.shortlist_rerank_ws_keys(C, S, n) == S * -(-C // 16) * min(n, 16), (C, S, n)
    hdr = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert int(re.search(r"#define DRN_RERANK_MAX_CANDIDATES\s+(\d+)", hdr).group(1)) == _lib.RERANK_MAX_CANDIDATES
    assert int(re.search(r"#define DRN_RERANK_GROUP\s+(\d+)", hdr).group(1)) == _lib.RERANK_GROUP
    assert int(re.search(r"#define DRN_CANDIDATES_MAX\s+(\d+)", hdr).group(1)) == _lib.RERANK_MAX_CANDIDATES
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_rerank.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shortlist_rerank_kernel"]       # ONE kernel body


def test_the_rerank_kernel_spills_nothing_and_keeps_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_rerank.hip compiled for gfx950 on its own: ONE kernel body instantiated for the four table operands, each without
    scratch and without a spilled register; static LDS is what the arrays come to -- 1,024 candidates, 16 x 16 states of 8 bytes, 16 x
    257 scores, 17 offsets, 3 x 16 slot words, 16 sums and the longest run = 22,920 B, plus the compiler's alignment padding: six
    workgroups a CU by LDS, so 512 / 6 = 85 registers would be needed for the registers not to set the occupancy; they do set it, at
    the 128 the neighbouring kernels run at (VGPRs + AGPRs stay at or below 128: four wavefronts a SIMD)."""
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_rerank.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_rerank.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    lds_claim = 1024 * 4 + 16 * 16 * 8 + 16 * 257 * 4 + 17 * 4 + 3 * 16 * 4 + 16 * 4 + 4
    assert lds_claim == 22920
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == 4 and all("shortlist_rerank_kernel" in k for k in seen), sorted(seen)
    assert sorted(("AlQ8" in k, "DF16b" in k) for k in seen) == [(False, False), (False, True), (True, False), (True, True)], sorted(seen)
    for name, (lds, scratch, vspill, sspill, regs) in seen.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds_claim <= lds <= lds_claim + 64, (name, lds)
        assert regs <= 128, (name, regs)


def test_the_rerank_entry_checks_its_arguments_before_anything_is_launched():
    lib = built_lib()
    p = ctypes.c_void_p(0x1000)
    # table scales queries lengths offsets candidates allow | ws ids scores counts
    OPTIONAL = (1, 3, 4, 6)

    def call(R=900, V=300, E=64, S=2, L=4, C=40, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 11 if ptrs is None else ptrs
        return lib.drn_shortlist_rerank(a[0], a[1], a[2], a[3], a[4], a[5], a[6], stride, R, V, E, S, L, C, n, dtype, a[7], keys, a[8], a[9],
                                        a[10], None)
    for i in range(11):
        if i in OPTIONAL:                                                    # (null is a meaning there, not an error)
            continue
        assert call(ptrs=[None if j == i else p for j in range(11)]) != 0 and b"null pointer" in lib.drn_last_error(), i
    assert call(R=0) != 0 and call(V=0) != 0 and call(E=0) != 0 and call(S=0) != 0 and b"bad args" in lib.drn_last_error()
    # without offsets row v is video v
    assert call(ptrs=[None if j == 4 else p for j in range(11)]) != 0 and b"without offsets" in lib.drn_last_error()
    for L in (0, -1, 65):
        assert call(L=L) != 0 and b"tokens outside [1, 64]" in lib.drn_last_error(), L
    for C in (0, -1, 1025):
        assert call(C=C) != 0 and b"candidates a sentence outside [1, 1024]" in lib.drn_last_error(), C
    for n in (0, 129):
        assert call(n=n) != 0 and b"outside [1, 128]" in lib.drn_last_error()
    assert call(dtype=2) != 0 and b"dtype" in lib.drn_last_error()
    assert call(ptrs=[ctypes.c_void_p(0x1004)] + [p] * 10) != 0 and b"16-byte aligned" in lib.drn_last_error()      # a misaligned table
    assert call(ptrs=[ctypes.c_void_p(0x1008) if j == 2 else p for j in range(11)]) != 0 and b"16-byte aligned" in lib.drn_last_error()
    assert call(ptrs=[ctypes.c_void_p(0x1004) if j == 7 else p for j in range(11)]) != 0 and b"8-byte aligned" in lib.drn_last_error()
    assert call(ptrs=[ctypes.c_void_p(0x1002) if j == 5 else p for j in range(11)]) != 0 and b"4-byte aligned" in lib.drn_last_error()
    for stride in (1, 9, 11, -10, 300):
        assert call(stride=stride) != 0 and b"neither 0" in lib.drn_last_error() and b"ceil(V / 32) = 10" in lib.drn_last_error(), stride
    assert call(ptrs=[ctypes.c_void_p(0x1002) if j == 6 else p for j in range(11)]) != 0 and b"mask must be 4-byte aligned" in lib.drn_last_error()
    # the workspace: S * ceil(C / 16) * min(n, 16) = 2 * 3 * 4 keys
    assert call(keys=2 * 3 * 4 - 1) != 0 and b"24 are needed" in lib.drn_last_error()
    assert call(n=128, C=1024, keys=2 * 64 * 16 - 1) != 0 and b"2048 are needed" in lib.drn_last_error()
    assert call(S=65536, keys=0x7fffffff) != 0 and b"more than 65535 sentences" in lib.drn_last_error()
    for E in (8, 48, 33, 500):
        assert call(E=E) != 0 and b"not a multiple of the block of 32 columns" in lib.drn_last_error(), E
