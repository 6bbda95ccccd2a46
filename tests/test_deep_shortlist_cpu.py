"""Deep shortlists, the host side: the references at depths beyond SHORTLIST_MAX (no new definition: a prefix of a deep list is the
shorter list), every refusal of Shortlister.shortlist_deep and evaluate_cascade(deep=True) before the library is reached, the C entry
drn_shortlist_deep at ABI 9 with its argument checks, and the compiler's resource notes for csrc/retrieve_deep.hip.
tests/test_deep_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_allow_shortlist_cpu import exact_host, same
from test_grounding_cpu import _header_params, built_lib
from test_q8_shortlist_cpu import _no_library, resident, tables
from test_sharded_shortlist_cpu import _stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- 1. the definition -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [100, 300, 1543])
def test_the_references_hold_at_depth_and_a_prefix_of_a_deep_list_is_the_shorter_list(V):
    """n = 129 / 257 / 1024 on exact integer data with planted ties, V below and above n: the list is a plain Python ranking by (score
    descending, position ascending), padded with -1 / 0, and its first k columns are the reference at n = k."""
    from drn_amd import segment_shortlist_reference, shortlist_reference
    emb, q = exact_host(V, 8, 3)
    score = (q.double() @ emb.double().t()).tolist()
    deep = {n: shortlist_reference(emb, q, n) for n in (129, 257, 1024)}
    for n, got in deep.items():
        assert tuple(got.ids.shape) == (3, n) and got.n.tolist() == [min(n, V)] * 3
        for s in range(3):
            order = sorted(range(V), key=lambda v: (-score[s][v], v))[:n]
            assert got.ids[s, :len(order)].tolist() == order and got.scores[s, :len(order)].tolist() == [score[s][v] for v in order]
            assert bool((got.ids[s, len(order):] == -1).all()) and bool((got.scores[s, len(order):] == 0).all())
        tied = (got.scores[:, 1:] == got.scores[:, :-1]) & (got.ids[:, 1:] > got.ids[:, :-1]) & (got.ids[:, 1:] >= 0)
        assert bool(tied.any()), "no tie in the data"
    for k in (1, 128, 129, 257):
        short = shortlist_reference(emb, q, k)
        assert torch.equal(deep[1024].ids[:, :k], short.ids) and torch.equal(deep[1024].scores[:, :k], short.scores)
        assert torch.equal(deep[1024].n.clamp(max=k), short.n)
    # ragged: runs cycling 1 / 3 / 0 / 17 over the same rows
    lens, left = [], V
    while left:
        lens.append(min((1, 3, 0, 17)[len(lens) % 4], left))
        left -= lens[-1]
    off = np.concatenate([[0], np.cumsum(lens)])
    owners = sum(1 for x in lens if x)
    far = segment_shortlist_reference(emb, off, q, 1024)
    assert far.n.tolist() == [min(1024, owners)] * 3
    for k in (129, 257):
        short = segment_shortlist_reference(emb, off, q, k)
        for f in ("ids", "scores", "rows"):
            assert torch.equal(getattr(far, f)[:, :k], getattr(short, f)), (k, f)
    mask = torch.rand(3, len(lens), generator=torch.Generator().manual_seed(V)) < 0.5
    same(segment_shortlist_reference(emb, off, q, 257, allow=mask),
         type(far)(*(x[:, :257] if x.dim() == 2 else x.clamp(max=257) for x in segment_shortlist_reference(emb, off, q, 1024, allow=mask))))


def test_the_deep_cap_is_the_width_its_consumers_take():
    import drn_amd
    from drn_amd import _lib
    header = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    define = lambda name: int(re.search(r"#define %s\s+(\d+)" % name, header).group(1))
    assert define("DRN_SHORTLIST_DEEP_MAX") == _lib.SHORTLIST_DEEP_MAX == _lib.RERANK_MAX_CANDIDATES == _lib.CANDIDATES_MAX == 1024
    assert define("DRN_SHORTLIST_DEEP_MAX") == define("DRN_RERANK_MAX_CANDIDATES") == define("DRN_CANDIDATES_MAX")
    assert drn_amd.SHORTLIST_DEEP_MAX == 1024 and _lib.SHORTLIST_MAX == define("DRN_SHORTLIST_MAX") == 128
    assert callable(drn_amd.Shortlister.shortlist_deep) and not hasattr(drn_amd.ShardedShortlister, "shortlist_deep")


# -- 2. the interface --------------------------------------------------------------------------------------------------------------------------

def test_shortlist_deep_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    codes, scales = tables(rows=40)
    q = resident(torch.zeros(3, 64, dtype=torch.bfloat16))
    for sl, W in ((Shortlister.from_mx8(codes, scales, torch.bfloat16), 2), (Shortlister.from_mx8(codes, scales, torch.bfloat16, offsets=[0, 2, 2, 40]), 1),
                  (_stand_in(40, E=64), 2), (_stand_in(20, ragged=True, E=64), 1)):
        what = "Shortlister.shortlist_deep"
        with pytest.raises(_lib.DrnError, match=what + ".*on the GPU"):
            sl.shortlist_deep(torch.zeros(3, 64, dtype=torch.bfloat16), 300)                  # host queries
        with pytest.raises(_lib.DrnError, match=what + ".*must be a tensor"):
            sl.shortlist_deep([[0.0] * 64], 300)
        for n in (0, -1, 1025):
            with pytest.raises(_lib.DrnError, match=what + r": n = %d outside \[1, 1024\]" % n):
                sl.shortlist_deep(q, n)
        for shape in ((3, 63), (3, 65), (64,), (3, 1, 64), (0, 64)):
            with pytest.raises(_lib.DrnError, match=what + r": the queries must be \(S, 64\)"):
                sl.shortlist_deep(resident(torch.zeros(shape, dtype=torch.bfloat16)), 300)
        for dt in (torch.float32, torch.float16):
            with pytest.raises(_lib.DrnError, match=what + ": the queries are %s" % dt):
                sl.shortlist_deep(resident(torch.zeros(3, 64, dtype=dt)), 300)
        with pytest.raises(_lib.DrnError, match="bool tensor; pack it first"):
            sl.shortlist_deep(q, 300, allow=resident(torch.ones(3, len(sl), dtype=torch.bool)))
        with pytest.raises(_lib.DrnError, match=r"allow must be \(%d,\)" % W):
            sl.shortlist_deep(q, 300, allow=resident(torch.zeros(W + 1, dtype=torch.int32)))
        ragged = sl._seg is not None
        good = (resident(torch.zeros(3, 300, dtype=torch.int32)), resident(torch.zeros(3, 300)), resident(torch.zeros(3, dtype=torch.int32)))
        with pytest.raises(_lib.DrnError, match=what + ": out must hold the %s buffers" % ("four" if ragged else "three")):
            sl.shortlist_deep(q, 300, out=good + (good[0],) * (0 if ragged else 1))
        with pytest.raises(_lib.DrnError, match=what + r": out.ids must be a contiguous \(3, 300\)"):
            sl.shortlist_deep(q, 300, out=(resident(torch.zeros(3, 128, dtype=torch.int32)),) + good[1:] + ((good[0],) if ragged else ()))
        # shortlist() keeps its cap and its message
        with pytest.raises(_lib.DrnError, match=r"Shortlister.shortlist: n = 129 outside \[1, 128\]"):
            sl.shortlist(q, 129)


def test_the_wrapper_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops
    _no_library(monkeypatch)
    codes, scales = tables(rows=40)
    i32 = lambda *shape: resident(torch.zeros(shape, dtype=torch.int32))
    emb, q, ws = resident(torch.zeros(40, 64)), resident(torch.zeros(3, 64)), resident(torch.zeros(4096, dtype=torch.int64))
    outs = (i32(3, 300), resident(torch.zeros(3, 300)), i32(3))
    seg = (i32(4), i32(2), i32(3))                                              # offsets (V = 3), blk_vid (one block), vid_blk
    with pytest.raises(_lib.DrnError, match="shortlist_deep: allow is required"):
        ops.shortlist_deep(emb, q, (), 300, ws, outs, None)
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.shortlist_deep(emb, q, (), 300, ws, outs, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.DrnError, match=r"shortlist_deep: n = 1025 outside \[1, 1024\]"):
        ops.shortlist_deep(emb, q, (), 1025, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_deep: ids must be"):
        ops.shortlist_deep(emb, q, (), 299, ws, outs, i32(2))
    with pytest.raises(_lib.DrnError, match="shortlist_deep: ws must be a contiguous int64 tensor of at least 768"):
        ops.shortlist_deep(emb, q, (), 300, ws[:767], outs, i32(2))              # 3 sentences x 1 block x min(300, 256) keys
    with pytest.raises(_lib.DrnError, match="shortlist_deep: allow must be a contiguous torch.int32 tensor"):
        ops.shortlist_deep(emb, q, (), 300, ws, outs, i32(3))
    with pytest.raises(_lib.DrnError, match="shortlist_deep: seg must be"):
        ops.shortlist_deep(emb, q, seg, 300, ws, outs, i32(1))                  # a ragged table needs rows
    with pytest.raises(_lib.DrnError, match="shortlist_deep: vid_blk must be"):
        ops.shortlist_deep(emb, q, (seg[0], seg[1], i32(4)), 300, ws, outs + (i32(3, 300),), i32(1))
    with pytest.raises(_lib.DrnError, match="shortlist_deep: emb .* and queries"):
        ops.shortlist_deep(emb, resident(torch.zeros(3, 32)), (), 300, ws, outs, i32(2))
    for table, s, o, W in ((emb, (), outs, 2), ((codes, scales), (), outs, 2), (emb, seg, outs + (i32(3, 300),), 1),
                           ((codes, scales), seg, outs + (i32(3, 300),), 1)):
        for good in (i32(W), i32(3, W)):
            with pytest.raises(AssertionError, match="the library was reached"):
                ops.shortlist_deep(table, q, s, 300, ws, o, good)


def test_evaluate_cascade_deep_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import ShardedShortlister, _lib, evaluate_cascade
    _no_library(monkeypatch)
    coarse, fine = _stand_in(3), _stand_in(3, ragged=True)

    def batches():
        raise AssertionError("a batch was read")
        yield
    for depth in (0, 1025, -3):
        with pytest.raises(_lib.DrnError, match=r"depth = %d outside \[1, 1024\]" % depth):
            evaluate_cascade(coarse, fine, batches(), depth, deep=True)
    for depth in (129, 1024):                                                   # the default keeps its cap and its message
        with pytest.raises(_lib.DrnError, match=r"depth = %d outside \[1, 128\]" % depth):
            evaluate_cascade(coarse, fine, batches(), depth)
    sh = ShardedShortlister([_stand_in(1), _stand_in(2)])
    sh.names = list(fine.names)
    with pytest.raises(_lib.DrnError, match="deep=True needs a single Shortlister.*compact"):
        evaluate_cascade(sh, fine, batches(), 300, deep=True)
    with pytest.raises(_lib.DrnError, match="at least one top-k"):
        evaluate_cascade(coarse, fine, batches(), 300, topks=(), deep=True)


# -- 3. the C boundary -------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_deep_entry_at_abi_9():
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    name = "drn_shortlist_deep"
    assert name in _lib.declared_symbols() and hasattr(lib, name)
    params, sig = _header_params(name), _lib.SIGNATURES[name]
    assert len(params) == len(sig) == 22, params
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(lib.drn_shortlist_deep.argtypes) == list(sig) and callable(ops.shortlist_deep)
    # the ragged quantised masked entry's parameters under the names of the rank and rerank convention
    twin = _header_params("drn_shortlist_segments_topn_q8_allow")
    assert params[0] == "const void* table" and params[1:] == twin[1:]


def test_the_deep_entry_checks_its_arguments_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)
    # table scales queries offsets blk_vid vid_blk allow ws | ids scores counts rows
    TABLE, SCALES, QUERIES, OFFSETS, BLK_VID, VID_BLK, ALLOW, WS, IDS, SCORES, COUNTS, ROWS = range(12)
    RAGGED = (OFFSETS, BLK_VID, VID_BLK, ROWS)

    def deep(ragged=False, q8=False, R=900, V=300, nblocks=2, E=64, S=2, n=300, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 12
        if not ragged:
            for i in RAGGED:
                a[i] = None
        if not q8:
            a[SCALES] = None
        for i, value in (ptrs or {}).items():
            a[i] = value
        return L.drn_shortlist_deep(a[0], a[1], a[2], a[3], a[4], a[5], a[6], stride, R, V, nblocks, E, S, n, dtype, a[7], keys, a[8], a[9], a[10],
                                    a[11], None)
    err = L.drn_last_error
    for ragged in (False, True):
        for q8 in (False, True):
            fn = lambda **kw: deep(ragged=ragged, q8=q8, **kw)
            needed = [TABLE, QUERIES, ALLOW, WS, IDS, SCORES, COUNTS] + (list(RAGGED) if ragged else [])
            for i in needed:
                assert fn(ptrs={i: None}) != 0 and b"drn_shortlist_deep" in err() and b"null pointer" in err(), (ragged, q8, i)
            if not ragged:                                                       # half a ragged argument set, either half
                for i in (BLK_VID, VID_BLK, ROWS):
                    assert fn(ptrs={i: p}) != 0 and b"null pointer" in err(), i
                assert deep(q8=q8, ptrs={OFFSETS: p}) != 0 and b"null pointer" in err()
            assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in err()
            for n in (0, 1025):
                assert fn(n=n) != 0 and b"drn_shortlist_deep: n = %d outside [1, 1024]" % n in err()
            assert fn(dtype=2) != 0 and b"dtype" in err()
            assert fn(ptrs={TABLE: ctypes.c_void_p(0x1004)}) != 0 and b"16-byte aligned" in err()
            assert fn(ptrs={QUERIES: ctypes.c_void_p(0x1008)}) != 0 and b"16-byte aligned" in err()
            assert fn(ptrs={WS: ctypes.c_void_p(0x1004)}) != 0 and b"8-byte aligned" in err()
            for stride in (1, 9, 11, -10, 300):
                assert fn(stride=stride) != 0 and b"neither 0" in err() and b"ceil(V / 32) = 10" in err(), stride
            for off in (1, 2, 3):
                assert fn(ptrs={ALLOW: ctypes.c_void_p(0x1000 + off)}) != 0 and b"mask must be 4-byte aligned" in err()
            if q8:
                for E in (8, 48, 33, 500):
                    assert fn(E=E) != 0 and b"not a multiple of the block of 32 columns" in err(), E
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
                assert fn(V=1 << 30, S=1 << 10, n=1024, keys=0x7fffffff) != 0 and b"are needed" in err()             # (no int overflow)
    # the four masked entries keep their cap and their message
    assert L.drn_shortlist_topn_allow(p, p, p, 0, 300, 64, 2, 129, 1, p, 1 << 20, p, p, p, None) != 0 and b"drn_shortlist_topn_allow: n = 129 outside [1, 128]" in err()


# -- 4. the compiler's resource notes ---------------------------------------------------------------------------------------------------------

def test_the_deep_merge_spills_nothing_and_keeps_the_register_cap(tmp_path):
    """csrc/retrieve_deep.hip compiled for gfx950 on its own: exactly the three instances of the merge, CAP = 256 / 512 / 1024.  Each
    without scratch and without a spilled register, at most 128 VGPRs + AGPRs, and static LDS exactly what the arrays come to -- 2 CAP
    keys of 8 bytes and two sets of four counts -- which is the size the comment above the kernel states."""
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_deep.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_deep.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_deep.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shortlist_merge_deep_kernel"]
    claims = {cap: 2 * cap * 8 + 2 * 4 * 4 for cap in (256, 512, 1024)}
    assert claims == {256: 4128, 512: 8224, 1024: 16416}
    stated = re.search(r"// Static LDS:[^\n]*?([\d,]+) / ([\d,]+) / ([\d,]+) B at CAP = 256 / 512 / 1024", src)
    assert stated and [int(x.replace(",", "")) for x in stated.groups()] == [claims[256], claims[512], claims[1024]]
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == 3 and all("shortlist_merge_deep_kernel" in k for k in seen), sorted(seen)
    for cap, lds_claim in claims.items():
        mine = [v for k, v in seen.items() if "ILi%dE" % cap in k]
        assert len(mine) == 1, (cap, sorted(seen))
        lds, scratch, vspill, sspill, regs = mine[0]
        assert scratch == 0 and vspill == 0 and sspill == 0, (cap, scratch, vspill, sspill)
        assert lds == lds_claim and regs <= 128, (cap, lds, regs)
