"""The shortlist over a block-scaled FP8 table, the host side: the refusals of Shortlister(quantize=), Shortlister.from_mx8 and shortlist()
that need no GPU, bytes_of, the definition (the plain references over mx8_dequantize), the two C entries at ABI 9 and the compiler's
resource notes for csrc/retrieve_q8.hip.  tests/test_q8_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("drn_shortlist_topn_q8", "drn_shortlist_segments_topn_q8")


def _no_library(monkeypatch):
    from drn_amd import ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_library)


class Resident(torch.Tensor):
    """A host tensor that says it is resident: the refusals behind the "on the GPU" checks are reached without a GPU (nothing is
    launched on it: the library is unreachable)."""
    is_cuda = True


def resident(t):
    return t.as_subclass(Resident)


def tables(rows=6, E=64):
    from drn_amd.index import mx8_quantize
    g = torch.Generator().manual_seed(rows + E)
    codes, scales = mx8_quantize(torch.randn(rows, E, generator=g))
    return resident(codes.contiguous()), resident(scales.contiguous())


# -- refusals, before the library is reached ---------------------------------------------------------------------------------------------

def test_the_constructor_refuses_a_bad_quantize_and_a_bad_width_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    for bad in ("fp8", "mxfp4", True, 8):
        with pytest.raises(_lib.DrnError, match="quantize must be one of"):
            Shortlister(resident(torch.zeros(4, 64)), quantize=bad)
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        Shortlister(torch.zeros(4, 64), quantize="mxfp8")                       # a host table
    for E in (8, 31, 33, 48, 500):
        for kw in ({}, {"offsets": [0, 4]}):
            with pytest.raises(_lib.DrnError, match="E to be a multiple of 32.*not E = %d" % E):
                Shortlister(resident(torch.zeros(4, E, dtype=torch.bfloat16)), quantize="mxfp8", **kw)
    with pytest.raises(_lib.DrnError, match="bfloat16 or float32"):
        Shortlister(resident(torch.zeros(4, 64, dtype=torch.float16)), quantize="mxfp8")


def test_from_mx8_refuses_what_is_not_a_table_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    codes, scales = tables()
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        Shortlister.from_mx8(torch.zeros(6, 64, dtype=torch.uint8), torch.zeros(6, 2, dtype=torch.uint8), torch.bfloat16)
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        Shortlister.from_mx8([[0] * 64], scales, torch.bfloat16)
    for c, s in ((resident(codes.to(torch.int8)), scales), (codes, resident(scales.to(torch.int32))), (resident(codes.float()), scales)):
        with pytest.raises(_lib.DrnError, match="must be uint8"):
            Shortlister.from_mx8(c, s, torch.bfloat16)
    for c in (resident(codes.reshape(-1)), resident(codes[:0]), resident(codes.t()), resident(codes[:, ::2])):
        with pytest.raises(_lib.DrnError, match="codes must be a contiguous"):
            Shortlister.from_mx8(c, scales, torch.bfloat16)
    with pytest.raises(_lib.DrnError, match="E must be a multiple of 32.*not E = 48"):
        Shortlister.from_mx8(resident(codes[:, :48].contiguous()), scales, torch.bfloat16)
    for s in (resident(scales[:5].contiguous()), resident(scales[:, :1].contiguous()), resident(scales.reshape(-1)),
              resident(torch.zeros(6, 4, dtype=torch.uint8)[:, ::2])):
        with pytest.raises(_lib.DrnError, match=r"scales must be a contiguous \(6, 2\)"):
            Shortlister.from_mx8(codes, s, torch.bfloat16)
    for dt in (torch.float16, torch.float64, torch.uint8, None):
        with pytest.raises(_lib.DrnError, match="dtype .of the queries. must be bfloat16 or float32"):
            Shortlister.from_mx8(codes, scales, dt)
    with pytest.raises(_lib.DrnError, match="2 names for 6 embeddings"):
        Shortlister.from_mx8(codes, scales, torch.float32, names=["a", "b"])
    with pytest.raises(_lib.DrnError, match="start at 0 and end at R = 6"):
        Shortlister.from_mx8(codes, scales, torch.float32, offsets=[0, 5])


def test_from_mx8_refuses_a_nan_code_a_bad_scale_and_a_value_that_is_not_finite(monkeypatch):
    """(The checks are torch's, on the tables' device: on these host stand-ins they run without the library.)"""
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    codes, scales = tables()
    for dtype in (torch.bfloat16, torch.float32):
        for kw in ({}, {"offsets": [0, 2, 2, 6], "names": ["a", "b", "c"]}):
            good = Shortlister.from_mx8(codes, scales, dtype, **kw)
            assert good.quantize == "mxfp8" and good.embeddings is None and good.codes is codes and good.scales is scales
            assert good.dtype == dtype and good.E == 64 and len(good) == (3 if kw else 6)
            for bad in (0x7f, 0xff):
                c = codes.clone()
                c[5, 63] = bad
                with pytest.raises(_lib.DrnError, match="a NaN code 0x7f / 0xff"):
                    Shortlister.from_mx8(c, scales, dtype, **kw)
            for bad in (0, 16, 255):
                s = scales.clone()
                s[3, 1] = bad
                with pytest.raises(_lib.DrnError, match=r"a scale byte outside \[17, 254\]"):
                    Shortlister.from_mx8(codes, s, dtype, **kw)
            c, s = codes.clone(), scales.clone()
            c[0, 0], s[0, 0] = 0x7e, 254                                        # 448 * 2^127
            with pytest.raises(_lib.DrnError, match="not finite in %s" % dtype):
                Shortlister.from_mx8(c, s, dtype, **kw)
            s[0, 0] = 17                                                        # the lowest scale the format writes
            assert len(Shortlister.from_mx8(c, s, dtype, **kw)) == len(good)


def test_shortlist_on_a_quantised_table_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    codes, scales = tables()
    for dtype, other in ((torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16)):
        for kw in ({}, {"offsets": [0, 2, 2, 6]}):
            sl = Shortlister.from_mx8(codes, scales, dtype, **kw)
            q = torch.zeros(2, 64, dtype=dtype)
            with pytest.raises(_lib.DrnError, match="on the GPU"):
                sl.shortlist(q, 2)                                              # host queries
            for n in (0, -1, 129):
                with pytest.raises(_lib.DrnError, match=r"outside \[1, 128\]"):
                    sl.shortlist(resident(q), n)
            with pytest.raises(_lib.DrnError, match=r"must be \(S, 64\)"):
                sl.shortlist(resident(torch.zeros(2, 32, dtype=dtype)), 2)
            with pytest.raises(_lib.DrnError, match="the queries are %s, the table is %s" % (other, dtype)):
                sl.shortlist(resident(q.to(other)), 2)
            with pytest.raises(_lib.DrnError, match="out.ids must be a contiguous"):
                sl.shortlist(resident(q), 2, out=[None] * (4 if kw else 3))
            with pytest.raises(_lib.DrnError, match="names are not the store's"):
                sl.check(type("Store", (), {"names": ["a"] * len(sl)})())
    # the wrappers themselves refuse host tensors, and widths the format does not have, before the library
    from drn_amd import ops
    with pytest.raises(_lib.DrnError):
        ops.shortlist_topn((codes.as_subclass(torch.Tensor), scales.as_subclass(torch.Tensor)), torch.zeros(2, 64), 2,
                           torch.zeros(8, dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 2)),
                           torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.DrnError, match="E a multiple of 32"):
        ops._q8_table("shortlist_topn_q8", torch.zeros((4, 48), dtype=torch.uint8), torch.zeros((4, 1), dtype=torch.uint8), torch.zeros(2, 48))


# -- sizes and the definition ---------------------------------------------------------------------------------------------------------------

def test_bytes_of_is_e_plus_e_over_32_bytes_a_row():
    from drn_amd import Shortlister, _lib
    assert Shortlister.bytes_of(1, 512, torch.float32, "mxfp8") == Shortlister.bytes_of(1, 512, torch.bfloat16, "mxfp8") == 528
    assert Shortlister.bytes_of(1, 512, torch.bfloat16) == 1024 and Shortlister.bytes_of(1, 512, torch.float32) == 2048
    assert Shortlister.bytes_of(120, 512, torch.bfloat16) == 122880 and Shortlister.bytes_of(120, 512, torch.bfloat16, "mxfp8") == 63360
    assert Shortlister.bytes_of(65536, 32, torch.float32, quantize="mxfp8") == 65536 * 33
    with pytest.raises(_lib.DrnError, match="multiple of 32"):
        Shortlister.bytes_of(4, 40, torch.bfloat16, "mxfp8")
    with pytest.raises(_lib.DrnError, match="quantize must be one of"):
        Shortlister.bytes_of(4, 64, torch.bfloat16, "fp8")
    assert Shortlister.bytes_of(4, 40, torch.bfloat16) == 320
    codes, scales = tables(6, 64)
    sl = Shortlister.from_mx8(codes, scales, torch.bfloat16)
    assert sl.nbytes == Shortlister.bytes_of(6, 64, torch.bfloat16, "mxfp8") == 6 * 66


def test_the_docstrings_name_the_definition():
    from drn_amd import Shortlister, retrieve
    for doc in (retrieve.__doc__, Shortlister.shortlist.__doc__):
        text = " ".join(doc.split())
        assert "shortlist_reference(mx8_dequantize(codes, scales), queries, n)" in text and "segment_shortlist_reference" in text
    for attr in ("codes", "scales", "dtype", "E", "quantize", "embeddings"):
        assert re.search(r"\b%s\b" % attr, Shortlister.__doc__), attr


def test_the_score_bound_is_the_formats_bound_per_element():
    """quantized_score_bound on a host table: with a one-hot query the bound of (s, row) is the element's own bound plus the rounding
    term, and every dequantised element lies inside its bound."""
    from drn_amd.index import mx8_dequantize, mx8_quantize
    from drn_amd.retrieve import quantized_score_bound
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(5, 64, generator=g) * torch.tensor([1e-3, 1.0, 30.0, 1e4, 1e-8])[:, None]).bfloat16()
    x[2, 3] = 1e-4                                                              # far below its block's scale: a subnormal or zero code
    codes, scales = mx8_quantize(x)
    dq = mx8_dequantize(codes, scales).double()
    e = scales.double() - 127
    per = torch.maximum(x.double().abs() / 16, torch.exp2(e - 10).repeat_interleave(32, dim=1))
    assert bool(((dq - x.double()).abs() <= per).all())
    bound = quantized_score_bound(x, scales, torch.eye(64)[:7])
    assert bound.shape == (7, 5) and bound.dtype == torch.float64
    assert torch.allclose(bound, (per[:, :7] + 64 * 2.0 ** -23 * x.double().abs()[:, :7]).t(), rtol=1e-12, atol=0)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_two_q8_entries_at_abi_9():
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
    assert callable(ops.shortlist_topn) and callable(ops.shortlist_segments_topn)
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_q8.hip")).read()
    assert int(re.search(r"#define SQ_BLOCK\s+(\d+)", src).group(1)) == _lib.SHORTLIST_BLOCK == _lib.SHORTLIST_SEG_BLOCK


def test_the_q8_entries_check_their_arguments_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def topn(V=300, E=64, S=2, n=4, dtype=1, keys=1 << 20, ptrs=None):
        a = [p] * 7 if ptrs is None else ptrs                                # codes scales queries ws | ids scores counts
        return L.drn_shortlist_topn_q8(a[0], a[1], a[2], V, E, S, n, dtype, a[3], keys, a[4], a[5], a[6], None)

    def segs(R=900, V=300, nblocks=2, E=64, S=2, n=4, dtype=1, keys=1 << 20, ptrs=None):
        a = [p] * 11 if ptrs is None else ptrs                               # codes scales queries offsets blk_vid vid_blk ws | ids scores counts rows
        return L.drn_shortlist_segments_topn_q8(a[0], a[1], a[2], a[3], a[4], a[5], R, V, nblocks, E, S, n, dtype, a[6], keys, a[7], a[8],
                                                a[9], a[10], None)
    for fn, nptr in ((topn, 7), (segs, 11)):
        for i in range(nptr):
            assert fn(ptrs=[None if j == i else p for j in range(nptr)]) != 0 and b"null pointer" in L.drn_last_error(), i
        assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in L.drn_last_error()
        for E in (8, 48, 33, 500):
            assert fn(E=E) != 0 and b"not a multiple of the block of 32 columns" in L.drn_last_error(), E
        for n in (0, 129):
            assert fn(n=n) != 0 and b"outside [1, 128]" in L.drn_last_error()
        assert fn(dtype=2) != 0 and b"dtype" in L.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1004)] + [p] * (nptr - 1)) != 0 and b"aligned" in L.drn_last_error()
        assert fn(ptrs=[p, p, ctypes.c_void_p(0x1008)] + [p] * (nptr - 3)) != 0 and b"aligned" in L.drn_last_error()
    assert topn(keys=2 * 2 * 4 - 1) != 0 and b"16 are needed" in L.drn_last_error()
    assert topn(V=1 << 30, S=1 << 10, n=128, keys=0x7fffffff) != 0 and b"are needed" in L.drn_last_error()          # (no int overflow)
    assert segs(R=0) != 0 and b"bad args" in L.drn_last_error()
    for nblocks in (0, 1, 301):                                              # (300 videos need two blocks of 256 at least, 300 at most)
        assert segs(nblocks=nblocks) != 0 and b"blocks outside" in L.drn_last_error(), nblocks
    assert segs(keys=16 + 8 - 1) != 0 and b"24 are needed" in L.drn_last_error()
    assert segs(V=1 << 30, nblocks=1 << 22, S=1 << 10, n=128, keys=0x7fffffff) != 0 and b"are needed" in L.drn_last_error()


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_q8_kernels_spill_nothing_and_keep_the_lds_of_their_plain_twins(tmp_path):
    """csrc/retrieve_q8.hip compiled for gfx950 on its own: exactly its four kernels (the ranking workgroup and the segmented ranking
    workgroup, each for bf16 and fp32 queries), every one without scratch and without a spilled register, static LDS that of the plain
    twin -- 16 x 256 keys of 8 bytes = 32,768 B, and with the 16 x 257 scores, 260 offsets and 4 run lengths 50,272 B -- and at most
    128 VGPRs + AGPRs, the cap the plain kernels are held to."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_q8.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_q8.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    B = _lib.SHORTLIST_SEG_BLOCK
    ranking, segmented = 16 * _lib.SHORTLIST_BLOCK * 8, 16 * B * 8 + 16 * (B + 1) * 4 + (B + 4) * 4 + 4 * 4
    assert (ranking, segmented) == (32768, 50272)
    claims = {"shortlist_block_q8_kernelIDF16b": ranking, "shortlist_block_q8_kernelIf": ranking,
              "shortlist_segments_q8_kernelIDF16b": segmented, "shortlist_segments_q8_kernelIf": segmented}
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_q8.hip")).read()
    assert sorted(re.findall(r"__global__[^\n]*?void (\w+)\(", src)) == ["shortlist_block_q8_kernel", "shortlist_segments_q8_kernel"]
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == len(claims), sorted(seen)
    for name, (lds, scratch, vspill, sspill, regs) in seen.items():
        claim = [v for k, v in claims.items() if k in name]
        assert len(claim) == 1, name
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds == claim[0] and regs <= 128, (name, lds, regs)
