"""Pooled tables, the host side: pool_segments_reference against a naive per-video loop, the proof that the order-sensitive inputs can
tell a wrong add order from the definition, the identities, every refusal of Shortlister.pooled / ShardedShortlister.pooled /
ops.pool_segments before the library is reached, the C entry drn_pool_segments at ABI 9 with its argument checks, and the compiler's
resource notes for csrc/retrieve_pool.hip.  tests/test_pooled_gpu.py holds the kernel."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_q8_shortlist_cpu import _no_library, resident
from test_sharded_shortlist_cpu import _stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# THE SHAPE TABLE: leading, inner and trailing videos without rows, a single row, runs of 2 and 17, and a run past 256
RUNS = [0, 1, 2, 0, 17, 300, 1, 0]
OFFSETS = np.concatenate([[0], np.cumsum(RUNS)]).astype(np.int64)
R = int(OFFSETS[-1])
GROUPS = [None, 1, 2, 16, 17, 300, 301]
HOWS = ["mean", "max"]
DTYPES = [torch.bfloat16, torch.float32]
# E: one lane group; not a multiple of a lane's columns, 8 in bf16 and 4 in fp32 (rows that are not 16-byte aligned: the element by
# element path -- 36 in bf16 and 22 in fp32; 20 IS a multiple of 4 and stays on the 16-byte path with a last group of lanes half
# idle); one full wavefront pass in bf16; past it, and legal for FP8
WIDTHS = {torch.bfloat16: [8, 36, 512, 544], torch.float32: [8, 20, 22, 512, 544]}
TAIL_WIDTHS = {torch.bfloat16: 36, torch.float32: 22}
assert all(TAIL_WIDTHS[t] % lane and TAIL_WIDTHS[t] in WIDTHS[t] for t, lane in ((torch.bfloat16, 8), (torch.float32, 4)))
_CACHE = {}


def order_sensitive(E, dtype, offsets=OFFSETS, seed=0):
    """The ORDER-SENSITIVE rows of a table with these offsets, from a fixed seed, made once per shape and never changed.  Every element
    is randn * 2^randint(-12, 12): exponents 24 binades apart, so an fp32 sum of three or more is inexact and depends on the order.
    That alone does not survive a rounding to bfloat16 -- a sum is dominated by its largest terms and two orders differ in its last
    fp32 bits --, so every run of three or more rows is laid out in triples (B, -B, s) per column, |B| in [2^9, 2^12) and |s| in
    [2^-12, 2^-9) times randn: the large terms cancel EXACTLY, what is left is of the size of the rounding errors made on the way
    (ulp(B) is 2^-14 .. 2^-12), and which of them are made depends on the order -- (B - B) + s = s, but (s + B) - B is s rounded to
    ulp(B).  A window of the run (a group) is balanced whenever it starts and ends between triples, which happens in every group size
    of the shape table; the function below this one proves it on the data."""
    key = ("x", E, dtype, tuple(int(o) for o in offsets), seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * seed + E)
        rnd = lambda n, lo, hi: torch.randn(n, E, generator=g) * torch.pow(2.0, torch.randint(lo, hi, (n, E), generator=g).float())
        x = rnd(int(offsets[-1]), -12, 12)
        for a, b in zip(offsets[:-1], offsets[1:]):
            t = int(b - a) // 3
            if t:
                big, small = rnd(t, 9, 12), rnd(t, -12, -9)
                x[a:a + 3 * t:3], x[a + 1:a + 3 * t:3], x[a + 2:a + 3 * t:3] = big, -big, small
        _CACHE[key] = x.to(dtype)
    return _CACHE[key]


def reference(E, dtype, how, group, q8=False):
    """pool_segments_reference on the shape table's rows (q8: on their block-scaled FP8 form), computed once and shared."""
    from drn_amd import pool_segments_reference
    from drn_amd.index import mx8_dequantize, mx8_quantize
    key = ("ref", E, dtype, how, group, q8)
    if key not in _CACHE:
        x = order_sensitive(E, dtype)
        if q8:
            x = mx8_dequantize(*mx8_quantize(x), dtype)
        _CACHE[key] = pool_segments_reference(x, OFFSETS, how, group)
    return _CACHE[key]


def groups_of(offsets, group):
    """[(video, first row, end row)] of every pooled row, in order, by the plainest loop there is."""
    out = []
    for v in range(len(offsets) - 1):
        a, b = int(offsets[v]), int(offsets[v + 1])
        if group is None:
            out.append((v, a, b))
        else:
            out += [(v, s, min(s + group, b)) for s in range(a, b, group)]
    return out


def to_dtype_bits(acc, dtype):
    """fp32 numpy -> the bits of the value rounded to dtype (nearest even), as uint32 / uint16."""
    u = np.ascontiguousarray(acc, dtype=np.float32).view(np.uint32)
    if dtype == torch.float32:
        return u
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint16)


# -- 1. the definition -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("group", GROUPS)
def test_the_reference_is_the_naive_loop(dtype, group):
    """Per video, per group, per row: acc = acc + row in numpy float32, one division, one rounding -- and the offsets by counting."""
    from drn_amd import pool_offsets
    E = TAIL_WIDTHS[dtype]
    x = order_sensitive(E, dtype).float().numpy()
    plan = groups_of(OFFSETS, group)
    for how in HOWS:
        got = reference(E, dtype, how, group)
        want = np.zeros((len(plan), E), dtype=np.float32)
        for i, (v, a, b) in enumerate(plan):
            if b == a:
                continue
            acc = np.zeros(E, dtype=np.float32) if how == "mean" else x[a].copy()
            for r in range(a, b):
                acc = (acc + x[r]).astype(np.float32) if how == "mean" else np.where(x[r] > acc, x[r], acc)
            want[i] = acc / np.float32(b - a) if how == "mean" else acc
            if how == "max":
                assert np.array_equal(acc, x[a:b].max(axis=0))
        assert got.rows.dtype == dtype and tuple(got.rows.shape) == (len(plan), E)
        assert np.array_equal(bits(got.rows), to_dtype_bits(want, dtype)), (how, group)
        if group is None:
            assert got.offsets is None and len(plan) == len(RUNS)
            assert bool((got.rows[[0, 3, 7]] == 0).all()) and not bool(torch.signbit(got.rows[[0, 3, 7]]).any())
        else:
            counts = [sum(1 for p in plan if p[0] == v) for v in range(len(RUNS))]
            assert got.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() == pool_offsets(OFFSETS, group).tolist()
            assert counts == [-(-n // group) for n in RUNS]


def _mutant(x, offsets, group, order):
    """A WRONG mean: the rows added in descending order, or by torch.sum, whose order nobody states -- taken along the contiguous
    dimension of a transposed copy, where it sums with several accumulators (along dim 0 of a small (rows, E) slice it happens to
    add row after row, which is the definition and no mutant)."""
    vals, out = x.float(), []
    for v, a, b in groups_of(offsets, group):
        if b == a:
            out.append(torch.zeros(vals.shape[1]))
        elif order == "sum":
            out.append(vals[a:b].t().contiguous().sum(dim=1) / float(b - a))
        else:
            acc = torch.zeros(vals.shape[1])
            for r in range(b - 1, a - 1, -1):
                acc = acc + vals[r]
            out.append(acc / float(b - a))
    return torch.stack(out).to(x.dtype)


@pytest.mark.parametrize("q8", [False, True], ids=["plain", "mxfp8"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("group", [g for g in GROUPS if g is None or g >= 3])
def test_the_inputs_can_tell_a_wrong_order_from_the_definition(dtype, group, q8):
    """Can the GPU test fail?  On the inputs it uses -- the rows as they are and, at the widths FP8 takes, what their block-scaled FP8
    form holds -- a mean that adds in DESCENDING order and one that calls torch.sum each differ from the definition in at least one
    element, at every width.  Every group size here has a group of 3 or more rows."""
    from drn_amd.index import mx8_dequantize, mx8_quantize
    for E in [E for E in WIDTHS[dtype] if E % 32 == 0] if q8 else WIDTHS[dtype]:
        x = order_sensitive(E, dtype)
        if q8:
            x = mx8_dequantize(*mx8_quantize(x), dtype)
        want = reference(E, dtype, "mean", group, q8=q8).rows
        for order in ("descending", "sum"):
            got = _mutant(x, OFFSETS, group, order)
            assert got.shape == want.shape and not np.array_equal(bits(got), bits(want)), (E, order)


def test_the_identities():
    from drn_amd import pool_segments_reference
    from drn_amd.index import mx8_dequantize, mx8_quantize
    for dtype in DTYPES:
        E = 64
        x = order_sensitive(E, dtype)
        for how in HOWS:                                                        # group = 1: the source, rows and offsets
            got = pool_segments_reference(x, OFFSETS, how, 1)
            assert np.array_equal(bits(got.rows), bits(x)) and got.offsets.tolist() == OFFSETS.tolist(), (dtype, how)
        codes, scales = mx8_quantize(x)
        dq = mx8_dequantize(codes, scales, dtype)
        assert bool(torch.signbit(dq[dq == 0]).any()), "no -0 in the FP8 table"
        table = _stand_in(len(RUNS), ragged=True, quantize="mxfp8", E=E, dtype=dtype)
        table.codes, table.scales, table._seg = codes, scales, (torch.from_numpy(OFFSETS.astype(np.int32)),) + table._seg[1:]
        assert np.array_equal(bits(pool_segments_reference(table, how="max", group=1).rows), bits(dq))
        assert torch.equal(pool_segments_reference(table, how="mean", group=1).rows, dq)      # (a -0 comes back as +0: equal, not the same bits)
        # how = "max", one row a video: the table
        one = pool_segments_reference(x[:9], np.arange(10), "max", None)
        assert one.offsets is None and np.array_equal(bits(one.rows), bits(x[:9]))
        # a group at least as long as the longest run: offsets 0, 1, ... over the videos that own a row, with group=None's rows
        owners = [v for v, n in enumerate(RUNS) if n]
        for how in HOWS:
            whole = pool_segments_reference(x, OFFSETS, how, None)
            for g in (300, 301, 10 ** 6):
                got = pool_segments_reference(x, OFFSETS, how, g)
                assert got.offsets.tolist() == np.concatenate([[0], np.cumsum([1 if n else 0 for n in RUNS])]).tolist()
                assert np.array_equal(bits(got.rows), bits(whole.rows[owners])), (dtype, how, g)


# -- 2. the interface --------------------------------------------------------------------------------------------------------------------------

def test_pooled_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import ShardedShortlister, Shortlister, _lib
    _no_library(monkeypatch)
    assert callable(Shortlister.pooled) and callable(ShardedShortlister.pooled)
    ragged, q8 = _stand_in(4, ragged=True), _stand_in(4, ragged=True, quantize="mxfp8")
    for what, make in (("Shortlister.pooled", lambda sl: sl), ("ShardedShortlister.pooled", lambda sl: ShardedShortlister([sl, sl]))):
        for plain in (_stand_in(4), _stand_in(4, quantize="mxfp8")):
            with pytest.raises(_lib.DrnError, match=what + ".*one row a video already"):
                make(plain).pooled()
        for sl in (ragged, q8):
            for how in ("sum", "avg", None, 0):
                with pytest.raises(_lib.DrnError, match=what + ": how must be one of"):
                    make(sl).pooled(how=how)
            for group in (0, -1, 2.0, "4", True, 2 ** 31):
                with pytest.raises(_lib.DrnError, match=what + ": group must be None"):
                    make(sl).pooled(group=group)
            for quantize in ("fp8", "mxfp4", True, 8):
                with pytest.raises(_lib.DrnError, match=what + ": quantize must be \"same\" or one of"):
                    make(sl).pooled(quantize=quantize)
            with pytest.raises(_lib.DrnError, match=what + ": stage_elems = 0 below 1"):
                make(sl).pooled(quantize="mxfp8", stage_elems=0)
        with pytest.raises(_lib.DrnError, match=what + ".*E to be a multiple of 32, not E = 40"):
            make(_stand_in(4, ragged=True, E=40)).pooled(quantize="mxfp8")
        with pytest.raises(_lib.DrnError, match=what + ".*no CPU fallback"):
            make(_stand_in(4, ragged=True, resident=False)).pooled()
    mixed = ShardedShortlister([ragged, q8])
    with pytest.raises(_lib.DrnError, match="ShardedShortlister.pooled: quantize=\"same\" needs shards of one format"):
        mixed.pooled()
    with pytest.raises(_lib.DrnError, match="ShardedShortlister.pooled: quantize=\"same\" needs shards of one format"):
        mixed.pooled(how="max", group=2, quantize="same")


def test_the_wrapper_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops
    _no_library(monkeypatch)
    i32 = lambda *v: resident(torch.tensor(v, dtype=torch.int32))
    emb, out, off = resident(torch.zeros(6, 64, dtype=torch.bfloat16)), resident(torch.zeros(3, 64, dtype=torch.bfloat16)), i32(0, 2, 2, 6)
    codes, scales = resident(torch.zeros(6, 64, dtype=torch.uint8)), resident(torch.zeros(6, 2, dtype=torch.uint8))
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.pool_segments(emb, off, torch.zeros(3, 64, dtype=torch.bfloat16))
    for how in ("sum", None, 1):
        with pytest.raises(_lib.DrnError, match="pool_segments: how must be one of"):
            ops.pool_segments(emb, off, out, how=how)
    for group in (0, -2, 1.5, True, 2 ** 31):
        with pytest.raises(_lib.DrnError, match="pool_segments: group must be None"):
            ops.pool_segments(emb, off, out, group=group, out_offsets=i32(0, 1, 1, 3))
    with pytest.raises(_lib.DrnError, match="pool_segments: out_offsets must be given exactly with group="):
        ops.pool_segments(emb, off, out, group=2)
    with pytest.raises(_lib.DrnError, match="pool_segments: out_offsets must be given exactly with group="):
        ops.pool_segments(emb, off, out, out_offsets=i32(0, 1, 1, 3))
    with pytest.raises(_lib.DrnError, match=r"pool_segments: out_offsets must be a contiguous \(4,\)"):
        ops.pool_segments(emb, off, out, group=2, out_offsets=i32(0, 1, 3))
    with pytest.raises(_lib.DrnError, match="pool_segments: offsets must be a contiguous"):
        ops.pool_segments(emb, resident(torch.tensor([0, 2, 2, 6])), out)
    with pytest.raises(_lib.DrnError, match="pool_segments: out must be float32 or bfloat16, and of a plain table's dtype"):
        ops.pool_segments(emb, off, resident(torch.zeros(3, 64)))
    with pytest.raises(_lib.DrnError, match=r"pool_segments: out must be a contiguous \(rows, 64\)"):
        ops.pool_segments(emb, off, resident(torch.zeros(3, 32, dtype=torch.bfloat16)))
    with pytest.raises(_lib.DrnError, match=r"pool_segments: out holds the pooled rows \[0, 4\), outside \[0, 3\]"):
        ops.pool_segments(emb, off, resident(torch.zeros(4, 64, dtype=torch.bfloat16)))
    with pytest.raises(_lib.DrnError, match=r"pool_segments: out holds the pooled rows \[1, 4\), outside \[0, 3\]"):
        ops.pool_segments(emb, off, out, out_row0=1)
    with pytest.raises(_lib.DrnError, match=r"pool_segments: out holds the pooled rows \[4, 7\), outside \[0, 6\]"):
        ops.pool_segments(emb, off, out, group=2, out_offsets=i32(0, 1, 1, 3), out_row0=4)
    with pytest.raises(_lib.DrnError, match="pool_segments: a plain table must be float32 or bfloat16"):
        ops.pool_segments(resident(torch.zeros(6, 64, dtype=torch.float16)), off, out)
    with pytest.raises(_lib.DrnError, match="pool_segments: a quantised table is codes"):
        ops.pool_segments((resident(torch.zeros(6, 40, dtype=torch.uint8)), resident(torch.zeros(6, 1, dtype=torch.uint8))), off,
                          resident(torch.zeros(3, 40, dtype=torch.bfloat16)))
    with pytest.raises(_lib.DrnError, match="pool_segments: a quantised table is codes"):
        ops.pool_segments((codes, scales[:, :1]), off, out)
    for table in (emb, (codes, scales)):
        for kw in ({}, {"how": "max"}, {"group": 2, "out_offsets": i32(0, 1, 1, 3)}, {"group": 4, "out_offsets": i32(0, 1, 1, 2), "out_row0": 1}):
            with pytest.raises(AssertionError, match="the library was reached"):
                ops.pool_segments(table, off, out[:2] if "out_row0" in kw else out, **kw)


# -- 3. the C boundary -------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_pool_entry_at_abi_9():
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    name = "drn_pool_segments"
    assert name in _lib.declared_symbols() and hasattr(lib, name)
    params, sig = _header_params(name), _lib.SIGNATURES[name]
    assert len(params) == len(sig) == 14, params
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(lib.drn_pool_segments.argtypes) == list(sig) and callable(ops.pool_segments)
    assert params[:4] == ["const void* table", "const uint8_t* scales", "const int32_t* offsets", "const int32_t* out_offsets"]
    header = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert ops.POOL_HOW == {"mean": int(re.search(r"#define DRN_POOL_MEAN\s+(\d+)", header).group(1)),
                            "max": int(re.search(r"#define DRN_POOL_MAX\s+(\d+)", header).group(1))}


def test_the_pool_entry_checks_its_arguments_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)
    err = L.drn_last_error
    TABLE, SCALES, OFFS, OUT_OFFS, OUT = range(5)

    def pool(q8=False, grouped=False, R=900, V=300, R_out=None, row0=0, E=64, how=0, dtype=1, ptrs=None):
        a = [p, p if q8 else None, p, p if grouped else None, p]
        for i, value in (ptrs or {}).items():
            a[i] = value
        R_out = (450 if grouped else V) if R_out is None else R_out
        return L.drn_pool_segments(a[0], a[1], a[2], a[3], R, V, R_out, row0, E, 2 if grouped else 0, how, dtype, a[4], None)
    for q8 in (False, True):
        for grouped in (False, True):
            fn = lambda **kw: pool(q8=q8, grouped=grouped, **kw)
            for i in (TABLE, OFFS, OUT):
                assert fn(ptrs={i: None}) != 0 and b"drn_pool_segments: null pointer" in err(), (q8, grouped, i)
            assert fn(R=0) != 0 and fn(V=0) != 0 and fn(E=0) != 0 and b"bad args" in err()
            for R_out in (0, -1):
                assert fn(R_out=R_out) != 0 and b"R_out = %d outside [1, 2^31)" % R_out in err()
            assert fn(row0=-1) != 0 and b"out_row0 = -1 below 0" in err()
            for how in (-1, 2):
                assert fn(how=how) != 0 and b"neither DRN_POOL_MEAN" in err()
            assert fn(dtype=2) != 0 and b"dtype" in err()
            assert fn(ptrs={TABLE: ctypes.c_void_p(0x1008)}) != 0 and b"16-byte aligned" in err()
            assert fn(ptrs={OUT: ctypes.c_void_p(0x1004)}) != 0 and b"16-byte aligned" in err()
            assert fn(ptrs={OFFS: ctypes.c_void_p(0x1002)}) != 0 and b"4-byte aligned" in err()
            if q8:
                for E in (8, 48, 33, 500):
                    assert fn(E=E) != 0 and b"not a multiple of the block of 32 columns" in err(), E
            if grouped:
                assert fn(ptrs={OUT_OFFS: None}) != 0 and b"out_offsets must be given exactly with group >= 1" in err()
                assert fn(ptrs={OUT_OFFS: ctypes.c_void_p(0x1001)}) != 0 and b"4-byte aligned" in err()
                assert fn(R_out=901) != 0 and fn(R_out=900, row0=1) != 0 and b"a group holds at least one row" in err()
                assert fn(R_out=0x7fffffff, row0=0x7fffffff) != 0 and b"a group holds at least one row" in err()       # (no int overflow)
            else:
                assert fn(ptrs={OUT_OFFS: p}) != 0 and b"out_offsets must be given exactly with group >= 1" in err()
                assert fn(R_out=301) != 0 and fn(R_out=300, row0=1) != 0 and b"do not lie inside the V = 300 videos" in err()
    assert L.drn_pool_segments(p, None, p, p, 900, 300, 450, 0, 64, -2, 0, 1, p, None) != 0 and b"group = -2 below 0" in err()


# -- 4. the compiler's resource notes ---------------------------------------------------------------------------------------------------------

def test_the_pool_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """csrc/retrieve_pool.hip compiled for gfx950 on its own: ONE kernel body, twelve instances (2 dtypes x 3 sources x 2 hows), each
    without scratch, without a spilled register and without LDS."""
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_pool.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_pool.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_pool.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["pool_segments_kernel"]
    assert "atomic" not in src.lower().replace("no atomics", "") and "__shared__" not in src
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"))
    want = {"_Z20pool_segments_kernelI%sLi%dELi%dEEv6PlArgs" % (t, s, h) for t in ("DF16b", "f") for s in range(3) for h in range(2)}
    assert set(seen) == want, sorted(seen)
    for name, (lds, scratch, vspill, sspill) in seen.items():
        assert lds == 0 and scratch == 0 and vspill == 0 and sspill == 0, (name, lds, scratch, vspill, sspill)
