"""The segmented shortlist, the host side: segment_shortlist_reference (the definition) on hand-made data and against shortlist_reference
with one row per video, plan_segment_blocks (the block plan), the refusals that need no GPU, the new C entry at ABI 9 and the compiler's
resource notes for csrc/retrieve_seg.hip.  tests/test_segment_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the definition ----------------------------------------------------------------------------------------------------------------------

def test_reference_on_hand_made_data():
    """Seven videos over nine rows with E = 2 and queries along the axes: empty videos first, in the middle and last; rows that tie
    inside a video (the lowest wins); videos that tie (the lower position first); n above V; a NaN query."""
    from drn_amd import SegmentShortlist, segment_shortlist_reference
    #                 v1: rows 0-2        v3: row 3   v4: rows 4-6                 v5: rows 7-8
    emb = torch.tensor([[1., 5.], [2., 0.], [2., 1.], [0., 7.], [-1., 2.], [2., 2.], [2., 9.], [1., 9.], [1., 9.]])
    off = [0, 0, 3, 3, 4, 7, 9, 9]                                            # videos 0, 2 and 6 own no row
    q = torch.tensor([[1., 0.], [0., 1.], [float("nan"), 0.], [0., -1.]])
    got = segment_shortlist_reference(emb, off, q, 9)
    assert isinstance(got, SegmentShortlist) and got._fields == ("ids", "scores", "n", "rows")
    assert got.ids.dtype == got.n.dtype == got.rows.dtype == torch.int32 and got.scores.dtype == torch.float32
    assert got.ids.shape == got.scores.shape == got.rows.shape == (4, 9) and got.n.tolist() == [4, 4, 0, 4]
    pad = lambda xs, fill: list(xs) + [fill] * (9 - len(xs))
    # sentence 0 (column 0): v1 = 2 at rows 1 and 2, v4 = 2 at rows 1 and 2 -> the lower video first, the lower row in each
    assert got.ids[0].tolist() == pad([1, 4, 5, 3], -1) and got.scores[0].tolist() == pad([2., 2., 1., 0.], 0.)
    assert got.rows[0].tolist() == pad([1, 1, 0, 0], -1)
    # sentence 1 (column 1): v4 = 9 at row 2, v5 = 9 at rows 0 and 1
    assert got.ids[1].tolist() == pad([4, 5, 3, 1], -1) and got.scores[1].tolist() == pad([9., 9., 7., 5.], 0.)
    assert got.rows[1].tolist() == pad([2, 0, 0, 0], -1)
    assert got.ids[2].tolist() == [-1] * 9 and got.scores[2].tolist() == [0.] * 9 and got.rows[2].tolist() == [-1] * 9
    # sentence 3 (minus column 1): v1 = 0 at row 1 (-0.0 ties with nothing here), v4 = -2, v3 = -7, v5 = -9
    assert got.ids[3].tolist() == pad([1, 4, 3, 5], -1) and got.rows[3].tolist() == pad([1, 0, 0, 0], -1)
    cut = segment_shortlist_reference(emb, np.asarray(off), q, 2)
    for f in ("ids", "scores", "rows"):
        assert torch.equal(getattr(cut, f), getattr(got, f)[:, :2]), f
    assert cut.n.tolist() == [2, 2, 0, 2]
    # a score that is not finite is not listed: video 0's best row overflows to +inf
    inf = segment_shortlist_reference(torch.tensor([[1e308, 1e308], [1.0, 0.0], [3.0, 0.0], [2.0, 0.0]], dtype=torch.float64),
                                      torch.tensor([0, 2, 4]), torch.tensor([[10.0, 10.0]], dtype=torch.float64), 2)
    assert inf.ids.tolist() == [[1, -1]] and inf.n.tolist() == [1] and inf.rows.tolist() == [[0, -1]] and inf.scores.tolist() == [[30.0, 0.0]]


def test_reference_with_one_row_per_video_is_the_plain_reference():
    from drn_amd import segment_shortlist_reference, shortlist_reference
    g = torch.Generator().manual_seed(3)
    emb = torch.randint(-4, 5, (9, 8), generator=g).float()
    emb[7], emb[2], emb[5] = emb[4], emb[4], emb[0]                          # planted equal scores
    q = torch.randint(-4, 5, (3, 8), generator=g).float()
    q[1, 3] = float("nan")
    for n in (4, 9, 12):
        a, b = shortlist_reference(emb, q, n), segment_shortlist_reference(emb, torch.arange(10), q, n)
        for f in ("ids", "scores", "n"):
            assert torch.equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, (n, f)
        assert torch.equal(b.rows, torch.where(b.ids >= 0, 0, -1).to(torch.int32))


# -- the block plan ------------------------------------------------------------------------------------------------------------------------

def _blocks(lens, **kw):
    from drn_amd import plan_segment_blocks
    off = np.concatenate([[0], np.cumsum(lens)])
    plan = plan_segment_blocks(off, **kw)
    b = plan.blk_vid
    assert b.dtype == plan.vid_blk.dtype == np.int32 and b[0] == 0 and b[-1] == len(lens) and (np.diff(b) >= 1).all()
    # every video in exactly one block, in order
    assert plan.vid_blk.shape == (len(lens),) and (np.diff(plan.vid_blk) >= 0).all()
    for k in range(len(b) - 1):
        assert (plan.vid_blk[b[k]:b[k + 1]] == k).all()
        assert b[k + 1] - b[k] <= kw.get("max_videos", 256)
        rows = int(off[b[k + 1]] - off[b[k]])
        assert rows <= kw.get("row_target", 256) or b[k + 1] - b[k] == 1
    return b.tolist()


def test_block_plan_keeps_every_video_whole_and_respects_both_caps():
    from drn_amd import _lib, plan_segment_blocks
    from drn_amd.retrieve import SEGMENT_ROW_TARGET
    assert _lib.SHORTLIST_SEG_BLOCK == 256 and SEGMENT_ROW_TARGET == 256
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_seg.hip")).read()
    assert int(re.search(r"#define SG_BLOCK\s+(\d+)", src).group(1)) == _lib.SHORTLIST_SEG_BLOCK
    assert _blocks([1]) == [0, 1]
    assert _blocks([1] * 256) == [0, 256] and _blocks([1] * 257) == [0, 256, 257]        # the video cap, at it and one past
    assert _blocks([0] * 600) == [0, 256, 512, 600]                                      # (empty videos count as videos)
    assert _blocks([100, 100, 56, 7]) == [0, 3, 4]                                       # closes exactly at the row target
    assert _blocks([100, 100, 57, 7]) == [0, 2, 4]                                       # one past it
    assert _blocks([128, 128, 128, 128]) == [0, 2, 4]
    assert _blocks([3, 600, 0, 2, 256, 1, 257]) == [0, 1, 2, 4, 5, 6, 7]                 # a 600-row video sits alone
    assert _blocks([600]) == [0, 1]
    assert _blocks([16] * 64) == list(range(0, 65, 16)) and _blocks([120] * 7) == [0, 2, 4, 6, 7]
    assert _blocks([1, 3, 0, 17] * 30, max_videos=5, row_target=40)[:3] == [0, 5, 10]    # (22 and 24 rows: the video cap closes them)
    assert _blocks([1, 3, 0, 17] * 30, max_videos=5, row_target=20)[:3] == [0, 3, 5]     # (4 + 17 and 18 + 3 rows would pass 20)
    g = np.random.RandomState(0)
    for _ in range(20):
        _blocks(g.randint(0, 90, g.randint(1, 700)).tolist())
    with pytest.raises(_lib.DrnError, match="max_videos"):
        plan_segment_blocks([0, 1], max_videos=257)


# -- refusals, before the library is reached -------------------------------------------------------------------------------------------------

def _no_library(monkeypatch):
    from drn_amd import ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_library)


def test_bad_offsets_and_names_are_refused_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    from drn_amd.retrieve import check_segment_offsets
    _no_library(monkeypatch)
    assert check_segment_offsets([0, 2, 2, 5], 5).tolist() == [0, 2, 2, 5]
    assert check_segment_offsets(torch.tensor([0, 5], dtype=torch.int32), 5, names=["a"]).dtype == np.int64
    assert check_segment_offsets(np.array([0, 1, 5], dtype=np.uint8), 5, names=["a", "b"]).tolist() == [0, 1, 5]
    for bad, R, match in (([1, 3, 5], 5, "start at 0 and end at R = 5"), ([0, 3, 4], 5, "start at 0 and end at R = 5"),
                          ([0, 3, 6], 5, "start at 0 and end at R = 5"), ([0, 4, 3, 5], 5, "decrease at video 1"),
                          ([0], 0, "V >= 1"), ([], 0, "integers|V >= 1"), ([[0, 5]], 5, "V >= 1"), ([0, 0], 0, r"outside \[1, 2\^31\)"),
                          ([0, 2 ** 31], 2 ** 31, r"outside \[1, 2\^31\)"), ([0.0, 5.0], 5, "must be integers"),
                          (torch.tensor([0.0, 5.0]), 5, "must be integers"), ("ab", 5, "integers")):
        with pytest.raises(_lib.DrnError, match=match):
            check_segment_offsets(bad, R)
    with pytest.raises(_lib.DrnError, match="2 names for 3 videos"):
        check_segment_offsets([0, 2, 2, 5], 5, names=["a", "b"])
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        Shortlister(torch.zeros(4, 8), offsets=[0, 4])                       # a host table, ragged or not


def test_segment_shortlist_refuses_bad_buffers_before_the_library_is_reached(monkeypatch):
    from drn_amd import SegmentShortlist, Shortlister, _lib
    _no_library(monkeypatch)
    # a ragged table that only stands in for a resident one (the constructor was not run): every refusal of shortlist() answers first
    sl = Shortlister.__new__(Shortlister)
    sl.embeddings, sl.names, sl._ws = torch.zeros(6, 8, dtype=torch.bfloat16), ["a", "b", "c"], {}
    sl._seg = (torch.tensor([0, 2, 2, 6], dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    assert len(sl) == 3
    q = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        sl.shortlist(q, 2)                                                    # host queries
    for n in (0, -1, 129):
        with pytest.raises(_lib.DrnError, match=r"outside \[1, 128\]"):
            sl.shortlist(q, n)
    with pytest.raises(_lib.DrnError, match=r"must be \(S, 8\)"):
        sl.shortlist(torch.zeros(2, 16, dtype=torch.bfloat16), 2)
    with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
        sl.shortlist(q.float(), 2)
    # out=: host queries are refused before the buffers are looked at, so the buffers' refusals are reached with host tensors that
    # say they are resident (nothing is launched on them: the library is unreachable)
    class Resident(torch.Tensor):
        is_cuda = True
    rq = q.as_subclass(Resident)
    good = lambda: [torch.zeros((2, 4), dtype=torch.int32).as_subclass(Resident), torch.zeros((2, 4)).as_subclass(Resident),
                    torch.zeros((2,), dtype=torch.int32).as_subclass(Resident), torch.zeros((2, 4), dtype=torch.int32).as_subclass(Resident)]
    assert sl._check(rq, 4, SegmentShortlist(*good())) == (2, 4)
    with pytest.raises(_lib.DrnError, match="four buffers"):
        sl._check(rq, 4, tuple(good()[:3]))
    for i, name in enumerate(SegmentShortlist._fields):
        for wrong in (torch.zeros((2, 5), dtype=torch.int32).as_subclass(Resident), torch.zeros((2, 4), dtype=torch.float64).as_subclass(Resident),
                      torch.zeros((4, 2), dtype=good()[i].dtype).t().as_subclass(Resident) if i != 2 else torch.zeros((3,), dtype=torch.int32).as_subclass(Resident),
                      torch.zeros(good()[i].shape, dtype=good()[i].dtype), None):
            out = good()
            out[i] = wrong
            with pytest.raises(_lib.DrnError, match="out.%s must be a contiguous" % name):
                sl._check(rq, 4, out)
    with pytest.raises(_lib.DrnError, match="out.rows must be a contiguous"):
        sl.shortlist(rq, 4, out=good()[:3] + [torch.zeros((2, 4), dtype=torch.int64).as_subclass(Resident)])


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_segment_entry_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    name = "drn_shortlist_segments_topn"
    assert name in _lib.declared_symbols() and hasattr(lib, name)
    params, sig = _header_params(name), _lib.SIGNATURES[name]
    assert len(params) == len(sig) == 19, params
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(getattr(lib, name).argtypes) == list(sig)
    for public in ("Shortlister", "SegmentShortlist", "segment_shortlist_reference", "plan_segment_blocks"):
        assert hasattr(drn_amd, public), public
    assert callable(ops.shortlist_segments_topn)
    assert ops.shortlist_segments_ws_keys(2, 3, 128) == 768 + 384 and ops.shortlist_segments_ws_keys(1, 1, 1) == 2


def test_the_segment_entry_checks_its_arguments_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def topn(R=900, V=300, nblocks=2, E=8, S=2, n=4, dtype=1, keys=1 << 20, ptrs=None):
        a = [p] * 10 if ptrs is None else ptrs                               # emb queries offsets blk_vid vid_blk ws | ids scores counts rows
        return L.drn_shortlist_segments_topn(a[0], a[1], a[2], a[3], a[4], R, V, nblocks, E, S, n, dtype, a[5], keys, a[6], a[7], a[8], a[9], None)
    for i in range(10):
        assert topn(ptrs=[None if j == i else p for j in range(10)]) != 0 and b"null pointer" in L.drn_last_error(), i
    assert topn(R=0) != 0 and topn(V=0) != 0 and topn(E=0) != 0 and topn(S=0) != 0 and b"bad args" in L.drn_last_error()
    for nblocks in (0, 1, 301):                                              # (300 videos need two blocks of 256 at least, 300 at most)
        assert topn(nblocks=nblocks) != 0 and b"blocks outside" in L.drn_last_error(), nblocks
    for n in (0, 129):
        assert topn(n=n) != 0 and b"outside [1, 128]" in L.drn_last_error()
    assert topn(dtype=2) != 0 and b"dtype" in L.drn_last_error()
    assert topn(keys=16 + 8 - 1) != 0 and b"24 are needed" in L.drn_last_error()
    assert topn(V=1 << 30, nblocks=1 << 22, S=1 << 10, n=128, keys=0x7fffffff) != 0 and b"are needed" in L.drn_last_error()   # (no int overflow)
    assert topn(ptrs=[ctypes.c_void_p(0x1004)] + [p] * 9) != 0 and b"aligned" in L.drn_last_error()


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_segment_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_seg.hip compiled for gfx950 on its own: its three kernels (the ranking workgroup in bf16 and fp32, the segment
    look-up) without scratch and without a spilled register, and static LDS exactly what the arrays come to -- 16 x 256 keys of 8
    bytes, 16 x 257 scores (the winning segments reuse them), 260 offsets and 4 run lengths of 4 bytes for the ranking workgroup, none
    for the look-up."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_seg.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_seg.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    B = _lib.SHORTLIST_SEG_BLOCK
    ranking = 16 * B * 8 + 16 * (B + 1) * 4 + (B + 4) * 4 + 4 * 4
    claims = {"shortlist_segments_kernelIDF16b": ranking, "shortlist_segments_kernelIf": ranking, "shortlist_segment_rows_kernel": 0}
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
