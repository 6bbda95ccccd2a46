"""The shortlist by late interaction, the host side: late_shortlist_reference (the definition) on hand-made data, against
segment_shortlist_reference with one token per sentence, its lengths, padding, NaN, allow and tie rules; the refusals of
Shortlister.shortlist_late that need no GPU; the two C entries at ABI 9 and the compiler's resource notes for csrc/retrieve_late.hip.
tests/test_late_shortlist_gpu.py holds the kernel."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("drn_shortlist_late_topn", "drn_shortlist_late_topn_q8")
NAN = float("nan")


# -- the definition ----------------------------------------------------------------------------------------------------------------------

def hand_case():
    """Three videos, E = 2, the tokens along the axes.  Video 0 answers each token in a different row (3 and 3), video 1 answers both
    half well in its one row (2 and 2), video 2 owns a weak and a negative row."""
    emb = torch.tensor([[3., 0.], [0., 3.], [2., 2.], [1., 1.], [-1., 0.]])
    off = [0, 2, 3, 5]
    q = torch.tensor([[[1., 0.], [0., 1.]]])
    return emb, off, q


def test_reference_on_a_hand_computed_case_where_pooling_ranks_the_wrong_video_first():
    from drn_amd import Shortlist, late_shortlist_reference, segment_shortlist_reference
    emb, off, q = hand_case()
    got = late_shortlist_reference(emb, off, q, torch.tensor([2]), 4)
    assert isinstance(got, Shortlist) and got._fields == ("ids", "scores", "n")
    assert got.ids.dtype == got.n.dtype == torch.int32 and got.scores.dtype == torch.float32
    assert got.ids.shape == got.scores.shape == (1, 4) and got.n.shape == (1,)
    # late: v0 = 3 (row 0) + 3 (row 1), v1 = 2 + 2, v2 = 1 + 1
    assert got.ids.tolist() == [[0, 1, 2, -1]] and got.scores.tolist() == [[6., 4., 2., 0.]] and got.n.tolist() == [3]
    # the pooled sentence vector (1, 1) matches neither row of video 0 well: v1 = 4, v0 = 3, v2 = 2
    pooled = segment_shortlist_reference(emb, off, q.sum(dim=1), 4)
    assert pooled.ids.tolist() == [[1, 0, 2, -1]] and pooled.scores.tolist() == [[4., 3., 2., 0.]]
    # the first token alone: v0 = 3, v1 = 2, v2 = 1
    one = late_shortlist_reference(emb, off, q, [1], 2)
    assert one.ids.tolist() == [[0, 1]] and one.scores.tolist() == [[3., 2.]] and one.n.tolist() == [2]


def test_reference_with_one_token_is_the_segment_reference():
    from drn_amd import late_shortlist_reference, segment_shortlist_reference
    g = torch.Generator().manual_seed(5)
    lens = [1, 3, 0, 4, 2, 0, 1]
    emb = torch.randint(-4, 5, (sum(lens), 8), generator=g).float()
    emb[4], emb[9] = emb[0], emb[1]                                          # planted equal scores across videos
    off = [0] + torch.tensor(lens).cumsum(0).tolist()
    q = torch.randint(-4, 5, (3, 8), generator=g).float()
    q[1, 3] = NAN
    allow = torch.tensor([True, False, True, True, True, True, False])
    for n in (2, 5, 9):
        for mask in (None, allow):
            a = segment_shortlist_reference(emb, off, q, n, allow=mask)
            b = late_shortlist_reference(emb, off, q[:, None, :], torch.ones(3, dtype=torch.int32), n, allow=mask)
            for f in ("ids", "scores", "n"):
                assert torch.equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, (n, f)
    assert b.n.tolist() == [3, 0, 3]                                         # (n = 9, masked: five owners, two of them not allowed)


def test_reference_lengths_padding_and_nan():
    from drn_amd import late_shortlist_reference
    emb, off, q1 = hand_case()
    # sentence 0: two live tokens and NaN padding; 1: a live NaN token; 2: no live token; 3: lengths above L; 4: a negative length
    q = torch.zeros(5, 3, 2)
    q[:, :2] = q1[0]
    q[0, 2] = NAN
    q[1, 1, 0] = NAN
    got = late_shortlist_reference(emb, off, q, torch.tensor([2, 2, 0, 7, -3]), 3)
    assert got.n.tolist() == [3, 0, 0, 3, 0]
    assert got.ids[0].tolist() == [0, 1, 2] and got.scores[0].tolist() == [6., 4., 2.]             # NaN in the padding is ignored
    assert got.ids[1].tolist() == [-1] * 3 and got.scores[1].tolist() == [0.] * 3                   # a live NaN empties its sentence only
    assert got.ids[2].tolist() == [-1] * 3 and got.scores[2].tolist() == [0.] * 3                   # lengths 0 lists nothing
    assert got.ids[3].tolist() == [0, 1, 2] and got.scores[3].tolist() == [6., 4., 2.]             # 7 is clamped to L = 3 (token 2 is zero)
    assert got.ids[4].tolist() == [-1] * 3                                                         # -3 is clamped to 0
    # the lengths may be a list, an int64 or an int32 tensor
    for lengths in ([2, 2, 0, 7, -3], torch.tensor([2, 2, 0, 7, -3], dtype=torch.int32)):
        again = late_shortlist_reference(emb, off, q, lengths, 3)
        assert all(torch.equal(a, b) for a, b in zip(again, got))
    # a NaN row of the table makes its video's score NaN for every live token: the video is not listed, the others are
    bad = emb.clone()
    bad[2, 0] = NAN
    got = late_shortlist_reference(bad, off, q1, [2], 3)
    assert got.ids.tolist() == [[0, 2, -1]] and got.n.tolist() == [2]
    # a sum that overflows float64 is not finite and not listed
    big = late_shortlist_reference(torch.tensor([[1e308], [1.]], dtype=torch.float64), [0, 1, 2],
                                   torch.tensor([[[1.], [1.]]], dtype=torch.float64), [2], 2)
    assert big.ids.tolist() == [[1, -1]] and big.scores.tolist() == [[2., 0.]]


def test_reference_respects_allow_empty_videos_and_ties():
    from drn_amd import _lib, late_shortlist_reference
    # videos 0 and 3 own no row; 1 and 4 reach 8 by different splits (3 + 5 and 5 + 3); 2 reaches 8 in one row
    emb = torch.tensor([[3., 0.], [0., 5.], [4., 4.], [5., 0.], [0., 3.], [1., 1.]])
    off = [0, 0, 2, 3, 3, 5, 6]
    q = torch.tensor([[[1., 0.], [0., 1.]], [[1., 0.], [1., 0.]]])
    got = late_shortlist_reference(emb, off, q, [2, 2], 6)
    assert got.ids[0].tolist() == [1, 2, 4, 5, -1, -1] and got.scores[0].tolist() == [8., 8., 8., 2., 0., 0.]     # ties go by position
    assert got.ids[1].tolist() == [4, 2, 1, 5, -1, -1] and got.scores[1].tolist() == [10., 8., 6., 2., 0., 0.]
    assert got.n.tolist() == [4, 4]
    shared = late_shortlist_reference(emb, off, q, [2, 2], 6, allow=torch.tensor([True, False, True, True, True, False]))
    assert shared.ids[0].tolist() == [2, 4, -1, -1, -1, -1] and shared.ids[1].tolist() == [4, 2, -1, -1, -1, -1] and shared.n.tolist() == [2, 2]
    each = torch.tensor([[True, True, False, True, False, True], [False] * 6])
    per = late_shortlist_reference(emb, off, q, [2, 2], 2, allow=each)
    assert per.ids.tolist() == [[1, 5], [-1, -1]] and per.scores.tolist() == [[8., 2.], [0., 0.]] and per.n.tolist() == [2, 0]
    with pytest.raises(_lib.DrnError, match="allow must be a bool tensor"):
        late_shortlist_reference(emb, off, q, [2, 2], 2, allow=torch.ones(5, dtype=torch.bool))
    with pytest.raises(_lib.DrnError, match="start at 0 and end at R = 6"):
        late_shortlist_reference(emb, [0, 2, 5], q, [2, 2], 2)


# -- refusals, before the library is reached -------------------------------------------------------------------------------------------------

def _no_library(monkeypatch):
    from drn_amd import ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_library)


class Resident(torch.Tensor):
    """A host tensor that says it is resident: the refusals behind "on the GPU" are reached, nothing is launched on it."""
    is_cuda = True


def _stand_in(quantize=None):
    """A ragged table that only stands in for a resident one (the constructor was not run)."""
    from drn_amd import Shortlister
    sl = Shortlister.__new__(Shortlister)
    sl.names, sl._ws = ["a", "b", "c"], {}
    sl._seg = (torch.tensor([0, 2, 2, 6], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    if quantize is None:
        sl.embeddings = torch.zeros(6, 32, dtype=torch.bfloat16)
    else:
        sl.embeddings, sl.quantize, sl._dtype = None, quantize, torch.float32
        sl.codes, sl.scales = torch.zeros(6, 32, dtype=torch.uint8), torch.zeros(6, 1, dtype=torch.uint8)
    return sl


def test_shortlist_late_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    import drn_amd
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    assert drn_amd.LATE_MAX_TOKENS == _lib.LATE_MAX_TOKENS == 64
    sl = _stand_in()
    q = torch.zeros(2, 3, 32, dtype=torch.bfloat16)
    rq = q.as_subclass(Resident)
    lengths = torch.tensor([3, 1], dtype=torch.int32)
    rl = lengths.as_subclass(Resident)
    with pytest.raises(_lib.DrnError, match="must be a tensor"):
        sl.shortlist_late([[1.0]], rl, 2)
    for bad in (torch.zeros(2, 32, dtype=torch.bfloat16), torch.zeros(2, 3, 16, dtype=torch.bfloat16), torch.zeros(0, 3, 32, dtype=torch.bfloat16),
                torch.zeros(2, 3, 1, 32, dtype=torch.bfloat16)):
        with pytest.raises(_lib.DrnError, match=r"must be \(S, L, 32\)"):
            sl.shortlist_late(bad.as_subclass(Resident), rl, 2)
    for L in (0, 65):
        with pytest.raises(_lib.DrnError, match=r"L = %d tokens outside \[1, 64\]" % L):
            sl.shortlist_late(torch.zeros(2, L, 32, dtype=torch.bfloat16).as_subclass(Resident), rl, 2)
    with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
        sl.shortlist_late(q.float().as_subclass(Resident), rl, 2)
    for n in (0, -1, 129):
        with pytest.raises(_lib.DrnError, match=r"outside \[1, 128\]"):
            sl.shortlist_late(rq, rl, n)
    with pytest.raises(_lib.DrnError, match="no CPU fallback"):
        sl.shortlist_late(q, rl, 2)                                          # host queries
    with pytest.raises(_lib.DrnError, match="queries must be contiguous"):
        sl.shortlist_late(torch.zeros(2, 6, 32, dtype=torch.bfloat16)[:, ::2].as_subclass(Resident), rl, 2)
    for bad in (lengths.long(), lengths.float(), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                torch.zeros(4, dtype=torch.int32)[::2], [3, 1]):
        with pytest.raises(_lib.DrnError, match=r"lengths must be a contiguous \(2,\) torch.int32"):
            sl.shortlist_late(rq, bad.as_subclass(Resident) if torch.is_tensor(bad) else bad, 2)
    with pytest.raises(_lib.DrnError, match="never read on the host"):
        sl.shortlist_late(rq, lengths, 2)                                    # host lengths
    # out=: three buffers, each of its shape and dtype
    good = lambda: [torch.zeros((2, 4), dtype=torch.int32).as_subclass(Resident), torch.zeros((2, 4)).as_subclass(Resident),
                    torch.zeros((2,), dtype=torch.int32).as_subclass(Resident)]
    with pytest.raises(_lib.DrnError, match="three buffers"):
        sl.shortlist_late(rq, rl, 4, out=good() + [torch.zeros((2, 4), dtype=torch.int32).as_subclass(Resident)])
    for i, name in enumerate(("ids", "scores", "n")):
        for wrong in (torch.zeros((2, 5), dtype=torch.int32).as_subclass(Resident), torch.zeros((2, 4), dtype=torch.float64).as_subclass(Resident),
                      torch.zeros(good()[i].shape, dtype=good()[i].dtype), None):
            out = good()
            out[i] = wrong
            with pytest.raises(_lib.DrnError, match="out.%s must be a contiguous" % name):
                sl.shortlist_late(rq, rl, 4, out=out)
    # allow=: the refusals of shortlist(allow=) -- V = 3 videos are one word
    for bad, match in ((torch.ones(3, dtype=torch.bool), "pack it first"), (torch.zeros(1, dtype=torch.int64), "torch.int32 packed words"),
                       (torch.zeros(1, dtype=torch.int32), "on the table's device"), ([1], "packed mask")):
        with pytest.raises(_lib.DrnError, match=match):
            sl.shortlist_late(rq, rl, 2, allow=bad)
    # a quantised table takes queries of the recorded dtype
    sq = _stand_in("mxfp8")
    with pytest.raises(_lib.DrnError, match="the table is torch.float32"):
        sq.shortlist_late(rq, rl, 2)
    with pytest.raises(_lib.DrnError, match=r"outside \[1, 128\]"):
        sq.shortlist_late(q.float().as_subclass(Resident), rl, 200)
    # a table without offsets is refused, and the message says what to do instead
    plain = Shortlister.__new__(Shortlister)
    plain.embeddings, plain.names, plain._ws, plain._seg = torch.zeros(6, 32, dtype=torch.bfloat16), None, {}, None
    with pytest.raises(_lib.DrnError, match=r"one row per video.*\(sum_t q_t\) \. emb_v.*call shortlist\(\)"):
        plain.shortlist_late(rq, rl, 2)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_late_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name, count in zip(ENTRIES, (21, 22)):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
    # the quantised twin takes (codes, scales) where the plain entry takes emb
    assert _header_params(ENTRIES[1])[2:] == _header_params(ENTRIES[0])[1:]
    for public in ("late_shortlist_reference", "LATE_MAX_TOKENS"):
        assert hasattr(drn_amd, public), public
    assert callable(drn_amd.Shortlister.shortlist_late) and callable(ops.shortlist_late_topn)
    assert ops.shortlist_late_ws_keys(2, 3, 128) == 768 and ops.shortlist_late_ws_keys(5, 7, 300) == 5 * 7 * 256
    assert ops.shortlist_late_ws_keys(1, 1, 1) == 1
    hdr = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert int(re.search(r"#define DRN_LATE_MAX_TOKENS\s+(\d+)", hdr).group(1)) == _lib.LATE_MAX_TOKENS
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_late.hip")).read()
    assert int(re.search(r"#define LT_BLOCK\s+(\d+)", src).group(1)) == _lib.SHORTLIST_SEG_BLOCK


def test_the_late_entries_check_their_arguments_before_anything_is_launched():
    lib = built_lib()
    p = ctypes.c_void_p(0x1000)

    def plain(R=900, V=300, nblocks=2, E=64, S=2, L=4, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 10 if ptrs is None else ptrs                               # emb queries lengths offsets blk_vid allow ws | ids scores counts
        return lib.drn_shortlist_late_topn(a[0], a[1], a[2], a[3], a[4], a[5], stride, R, V, nblocks, E, S, L, n, dtype, a[6], keys, a[7], a[8],
                                           a[9], None)

    def q8(R=900, V=300, nblocks=2, E=64, S=2, L=4, n=4, dtype=1, keys=1 << 20, stride=0, ptrs=None):
        a = [p] * 11 if ptrs is None else ptrs                               # codes scales queries lengths offsets blk_vid allow ws | ids scores counts
        return lib.drn_shortlist_late_topn_q8(a[0], a[1], a[2], a[3], a[4], a[5], a[6], stride, R, V, nblocks, E, S, L, n, dtype, a[7], keys,
                                              a[8], a[9], a[10], None)
    for fn, nptr, mask_at, q_at in ((plain, 10, 5, 1), (q8, 11, 6, 2)):
        for i in range(nptr):
            if i == mask_at:                                                 # (no mask is no error: the call would be launched)
                continue
            assert fn(ptrs=[None if j == i else p for j in range(nptr)]) != 0 and b"null pointer" in lib.drn_last_error(), (fn.__name__, i)
        assert fn(R=0) != 0 and fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in lib.drn_last_error()
        for L in (0, -1, 65):
            assert fn(L=L) != 0 and b"tokens outside [1, 64]" in lib.drn_last_error(), L
        for nblocks in (0, 1, 301):
            assert fn(nblocks=nblocks) != 0 and b"blocks outside" in lib.drn_last_error(), nblocks
        for n in (0, 129):
            assert fn(n=n) != 0 and b"outside [1, 128]" in lib.drn_last_error()
        assert fn(dtype=2) != 0 and b"dtype" in lib.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1004)] + [p] * (nptr - 1)) != 0 and b"16-byte aligned" in lib.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1008) if j == q_at else p for j in range(nptr)]) != 0 and b"16-byte aligned" in lib.drn_last_error()
        for stride in (1, 9, 11, -10, 300):
            assert fn(stride=stride) != 0 and b"neither 0" in lib.drn_last_error() and b"ceil(V / 32) = 10" in lib.drn_last_error(), stride
        assert fn(ptrs=[ctypes.c_void_p(0x1002) if j == mask_at else p for j in range(nptr)]) != 0 \
            and b"mask must be 4-byte aligned" in lib.drn_last_error()
        assert fn(keys=2 * 2 * 4 - 1) != 0 and b"16 are needed" in lib.drn_last_error()
        assert fn(V=1 << 30, nblocks=1 << 22, S=1 << 10, n=128, keys=0x7fffffff) != 0 and b"are needed" in lib.drn_last_error()   # (no int overflow)
        assert fn(S=65536, keys=0x7fffffff) != 0 and b"more than 65535 sentences" in lib.drn_last_error()
    for E in (8, 48, 33, 500):
        assert q8(E=E) != 0 and b"not a multiple of the block of 32 columns" in lib.drn_last_error(), E


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_late_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_late.hip compiled for gfx950 on its own: ONE kernel body instantiated for the four table operands (plain bf16 /
    fp32, FP8 codes under bf16 / fp32 queries), each without scratch and without a spilled register, and static LDS exactly what the
    arrays come to: 16 x 256 states of 8 bytes, 16 x 257 scores, 260 offsets, 256 sums and 4 run lengths of 4 bytes = 51,296 B.  That
    LDS lets three workgroups -- three wavefronts a SIMD -- share a CU, which leaves each 512 / 3 registers: VGPRs + AGPRs stay at or
    below 168, so the registers never lower the occupancy the LDS sets."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_late.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_late.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    B = _lib.SHORTLIST_SEG_BLOCK
    lds_claim = 16 * B * 8 + 16 * (B + 1) * 4 + (B + 4) * 4 + B * 4 + 4 * 4
    assert lds_claim == 51296 and 3 * lds_claim <= 160 * 1024 < 4 * lds_claim
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_late.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shortlist_late_kernel"]
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == 4 and all("shortlist_late_kernel" in k for k in seen), sorted(seen)
    assert sorted(("AlQ8" in k, "DF16b" in k) for k in seen) == [(False, False), (False, True), (True, False), (True, True)], sorted(seen)
    for name, (lds, scratch, vspill, sspill, regs) in seen.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds == lds_claim and regs <= 168, (name, lds, regs)
