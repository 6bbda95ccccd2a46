"""The shortlist and device candidates, the host side: plan_candidate_steps and plan_candidates_reference (the shape-only plan of a search
over a device candidates tensor and the numpy definition of its data half), shortlist_reference (the definition of a shortlist), the
refusals that need no GPU, the two C entries at ABI 9 and the compiler's resource notes for csrc/retrieve.hip.
tests/test_shortlist_gpu.py holds the kernels and the search."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- the plan --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,N", list(itertools.product((1, 3, 17), (1, 5, 64))))
def test_plan_candidate_steps_owns_every_pair_once(S, N):
    from drn_amd import plan_candidate_steps
    for pairs, cap in itertools.product((1, 4, 7, 16, 512), (1, 2, 64)):
        plan = plan_candidate_steps(S, N, pairs, cap)
        Sc, Nc = plan.Sc, plan.Nc
        assert Nc == min(N, cap, pairs) and Sc == min(S, pairs // Nc) and plan.pairs == pairs and Sc * Nc <= pairs
        steps = (-(-S // Sc)) * (-(-N // Nc))
        assert plan.pair_q.shape == plan.pair_v.shape == (steps, pairs) and plan.pair_off.shape == (steps, S + 1)
        assert plan.first.shape == (steps, 1) and plan.first[:, 0].tolist() == [1] + [0] * (steps - 1)
        assert all(a.dtype == np.int32 for a in plan[3:])
        assert (plan.pair_v == np.arange(pairs)[None, :]).all()
        owners = np.zeros((S, N), dtype=np.int64)
        ncb = -(-N // Nc)
        for c in range(steps):
            off = plan.pair_off[c]
            assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= pairs
            assert (np.diff(off) <= cap).all()                              # no sentence has more than cap pairs in a step
            sb, cb = c // ncb, c % ncb
            for s in range(S):
                for i in range(off[s], off[s + 1]):
                    assert plan.pair_q[c, i] == s == sb * Sc + i // Nc
                    j = cb * Nc + i % Nc
                    if j < N:
                        owners[s, j] += 1
            assert (plan.pair_q[c, off[S]:] == 0).all()                     # padding past pair_off[S]
        assert (owners == 1).all(), (S, N, pairs, cap)
    # the defaults: no cap, min(SEARCH_PAIR_BUDGET, S * N) pairs
    from drn_amd import Grounder
    plan = plan_candidate_steps(S, N)
    assert plan.pairs == min(Grounder.SEARCH_PAIR_BUDGET, S * N) and plan.Nc == min(N, plan.pairs)


def test_plan_candidate_steps_refuses_empty_shapes():
    from drn_amd import _lib, plan_candidate_steps
    for bad in ((0, 4, 4, 4), (3, 0, 4, 4), (3, 4, 0, 4), (3, 4, 4, 0)):
        with pytest.raises(_lib.DrnError, match="at least 1"):
            plan_candidate_steps(*bad)


# the cases tests/test_shortlist_gpu.py holds the launch to as well: (C, num_videos, pairs, cap)
PLAN_CASES = [
    ([[1, 1, 2, 9, 1], [0, -1, 3, 3, 4], [7, 7, 7, 7, 7]], 8, 4, 2),          # N = 5, Nc = 2: repeats in another column block
    ([[1, 1, 2, 9, 1], [0, -1, 3, 3, 4], [7, 7, 7, 7, 7]], 8, 7, 64),         # Nc = 5, Sc = 1, two padded pairs per step
    ([[1, 1, 2, 9, 1], [0, -1, 3, 3, 4], [7, 7, 7, 7, 7]], 8, 512, 64),       # one step
    ([[5], [5], [-3], [0]], 6, 3, 1),                                         # N = 1
    ([[0, 1, 2, 3, 4, 5, 6, 7]], 4, 3, 64),                                   # S = 1, positions past the store
]


def test_plan_candidates_reference_drops_what_is_no_candidate():
    from drn_amd import plan_candidate_steps
    from drn_amd.grounding import plan_candidates_reference
    C = PLAN_CASES[0][0]
    table = plan_candidates_reference(C, 8, 3, 5, 4, 2)
    plan = plan_candidate_steps(3, 5, 4, 2)
    assert (plan.Sc, plan.Nc) == (2, 2) and table.shape == plan.pair_q.shape == (6, 4) and table.dtype == np.int32
    # steps: (sentences 0-1) x columns (0-1, 2-3, 4), then (sentence 2) x the same; pair = sl * 2 + jl
    assert table.tolist() == [[1, -1, 0, -1],           # row 0: 1, then its repeat; row 1: 0, then -1
                              [2, -1, 3, -1],           # row 0: 2, then 9 >= 8; row 1: 3, then its repeat
                              [-1, -1, 4, -1],          # row 0: the 1 again, in ANOTHER column block; column 5 does not exist
                              [7, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]
    for C, Nv, pairs, cap in PLAN_CASES:
        S, N = len(C), len(C[0])
        table = plan_candidates_reference(C, Nv, S, N, pairs, cap)
        plan = plan_candidate_steps(S, N, pairs, cap)
        assert table.shape == plan.pair_q.shape
        for s in range(S):
            want = []
            for v in C[s]:
                if 0 <= v < Nv and v not in want:
                    want.append(v)
            got = [int(table[c, i]) for c in range(table.shape[0]) for i in range(plan.pair_off[c, s], plan.pair_off[c, s + 1])
                   if table[c, i] >= 0]
            assert got == want, (C, s)
        for c in range(table.shape[0]):
            assert (table[c, plan.pair_off[c, S]:] == -1).all()


# -- the definition of a shortlist -----------------------------------------------------------------------------------------------------

def test_shortlist_reference_orders_equal_scores_by_position_and_fills_past_the_list():
    from drn_amd import Shortlist, shortlist_reference
    g = torch.Generator().manual_seed(3)
    emb = torch.randint(-4, 5, (9, 8), generator=g).float()
    emb[7], emb[2], emb[5] = emb[4], emb[4], emb[0]                          # planted equal scores
    q = torch.randint(-4, 5, (3, 8), generator=g).float()
    q[1, 3] = float("nan")
    got = shortlist_reference(emb, q, 12)
    assert isinstance(got, Shortlist) and got.ids.dtype == got.n.dtype == torch.int32 and got.scores.dtype == torch.float32
    assert got.ids.shape == got.scores.shape == (3, 12) and got.n.tolist() == [9, 0, 9]
    assert (got.ids[1] == -1).all() and (got.scores[1] == 0).all()
    score = (q.double() @ emb.double().t())
    for s in (0, 2):
        ids = got.ids[s, :9].tolist()
        assert sorted(ids) == list(range(9)) and (got.ids[s, 9:] == -1).all() and (got.scores[s, 9:] == 0).all()
        assert got.scores[s, :9].tolist() == [float(score[s, v]) for v in ids]
        for a, b in zip(ids, ids[1:]):
            assert score[s, a] > score[s, b] or (score[s, a] == score[s, b] and a < b)
        assert ids.index(2) < ids.index(4) < ids.index(7) and ids.index(0) < ids.index(5)
    cut = shortlist_reference(emb, q, 4)
    assert torch.equal(cut.ids, got.ids[:, :4]) and torch.equal(cut.scores, got.scores[:, :4]) and cut.n.tolist() == [4, 0, 4]
    inf = shortlist_reference(torch.tensor([[1e308, 1e308], [1.0, 0.0]], dtype=torch.float64), torch.tensor([[10.0, 10.0]],
                              dtype=torch.float64), 2)
    assert inf.ids.tolist() == [[1, -1]] and inf.n.tolist() == [1]            # a score that is not finite is not listed


# -- refusals, before the library is reached ---------------------------------------------------------------------------------------------

def _no_library(monkeypatch):
    from drn_amd import ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_library)


def test_shortlister_refuses_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    from drn_amd._lib import SHORTLIST_MAX
    _no_library(monkeypatch)
    assert SHORTLIST_MAX == 128
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        Shortlister(torch.zeros(4, 8))                                        # a host table
    # a table that only stands in for a resident one (the constructor was not run): every refusal of shortlist() answers first
    sl = Shortlister.__new__(Shortlister)
    sl.embeddings, sl.names, sl._ws = torch.zeros(4, 8, dtype=torch.bfloat16), ["a", "b", "c", "d"], {}
    q = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.DrnError, match="on the GPU"):
        sl.shortlist(q, 2)                                                    # host queries
    for n in (0, -1, SHORTLIST_MAX + 1):
        with pytest.raises(_lib.DrnError, match=r"outside \[1, 128\]"):
            sl.shortlist(q, n)
    with pytest.raises(_lib.DrnError, match=r"must be \(S, 8\)"):
        sl.shortlist(torch.zeros(2, 16, dtype=torch.bfloat16), 2)
    with pytest.raises(_lib.DrnError, match=r"must be \(S, 8\)"):
        sl.shortlist(torch.zeros(8, dtype=torch.bfloat16), 2)
    with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
        sl.shortlist(q.float(), 2)
    store = lambda names: type("Store", (), {"names": names})()
    sl.check(store(["a", "b", "c", "d"]))
    for names in (["a", "b", "d", "c"], ["a", "b", "c"]):
        with pytest.raises(_lib.DrnError, match="names are not the store's"):
            sl.check(store(names))
    sl.names = None
    with pytest.raises(_lib.DrnError, match="names are not the store's"):
        sl.check(store(["a", "b", "c", "d"]))


def test_device_candidates_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import FeatureStore, SearchIndex, _lib
    from drn_amd.grounding import check_device_candidates
    _no_library(monkeypatch)
    assert _lib.CANDIDATES_MAX == 1024
    videos = [("v%d" % v, torch.randn(8, 64), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64) for v in range(3)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    C = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(_lib.DrnError, match="every .sentence, video. pair would\\s+pool and project its own video -- build an index"):
        check_device_candidates(C, 2, store)
    index = SearchIndex.__new__(SearchIndex)                                  # (only its type is looked at)
    check_device_candidates(C, 2, index)
    check_device_candidates(torch.zeros((2, 1024), dtype=torch.int32), 2, index)
    with pytest.raises(_lib.DrnError, match="1 <= N <= 1024"):
        check_device_candidates(torch.zeros((2, 1025), dtype=torch.int32), 2, index)
    with pytest.raises(_lib.DrnError, match="1 <= N <= 1024"):
        check_device_candidates(torch.zeros((2, 0), dtype=torch.int32), 2, index)
    with pytest.raises(_lib.DrnError, match=r"must be \(3, N\)"):
        check_device_candidates(C, 3, index)
    for dt in (torch.int64, torch.float32, torch.int16):
        with pytest.raises(_lib.DrnError, match="must be int32"):
            check_device_candidates(C.to(dt), 2, index)
    with pytest.raises(_lib.DrnError, match="chunk= does not apply"):
        check_device_candidates(C, 2, index, chunk=2)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_two_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert int(re.search(r"#define DRN_SHORTLIST_MAX\s+(\d+)", hdr).group(1)) == _lib.SHORTLIST_MAX
    assert int(re.search(r"#define DRN_CANDIDATES_MAX\s+(\d+)", hdr).group(1)) == _lib.CANDIDATES_MAX
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve.hip")).read()
    assert int(re.search(r"#define SL_BLOCK\s+(\d+)", src).group(1)) == _lib.SHORTLIST_BLOCK
    for name in ("drn_shortlist_topn", "drn_plan_candidates"):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig), (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
    for name in ("Shortlister", "Shortlist", "shortlist_reference", "plan_candidate_steps"):
        assert hasattr(drn_amd, name), name
    assert callable(ops.shortlist_topn) and callable(ops.plan_candidates)
    assert ops.shortlist_ws_keys(257, 3, 128) == 3 * 2 * 128 and ops.shortlist_ws_keys(1, 1, 1) == 1


def test_the_entries_check_their_arguments_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def topn(V=300, E=8, S=2, n=4, dtype=1, keys=1 << 20, ptrs=None):
        a = [p] * 6 if ptrs is None else ptrs                                # emb queries ws | ids scores counts
        return L.drn_shortlist_topn(a[0], a[1], V, E, S, n, dtype, a[2], keys, a[3], a[4], a[5], None)
    for i in range(6):
        assert topn(ptrs=[None if j == i else p for j in range(6)]) != 0 and b"null pointer" in L.drn_last_error(), i
    assert topn(V=0) != 0 and topn(E=0) != 0 and topn(S=0) != 0
    for n in (0, 129):
        assert topn(n=n) != 0 and b"outside [1, 128]" in L.drn_last_error()
    assert topn(dtype=2) != 0 and b"dtype" in L.drn_last_error()
    assert topn(keys=2 * 2 * 4 - 1) != 0 and b"16 are needed" in L.drn_last_error()
    assert topn(V=1 << 30, S=1 << 10, n=128, keys=0x7fffffff) != 0 and b"are needed" in L.drn_last_error()          # (no int overflow)
    assert topn(ptrs=[ctypes.c_void_p(0x1004)] + [p] * 5) != 0 and b"aligned" in L.drn_last_error()

    def plan(S=3, N=5, Nv=8, Sc=2, Nc=2, pairs=4, steps=6, ptrs=(p, p)):
        return L.drn_plan_candidates(ptrs[0], S, N, Nv, Sc, Nc, pairs, steps, ptrs[1], None)
    assert plan(ptrs=(None, p)) != 0 and plan(ptrs=(p, None)) != 0 and b"null pointer" in L.drn_last_error()
    assert plan(N=1025, Nc=2) != 0 and b"at most 1024" in L.drn_last_error()
    assert plan(S=0) != 0 and plan(N=0) != 0 and plan(Nv=-1) != 0
    assert plan(pairs=3) != 0 and b"does not fit 3 pairs" in L.drn_last_error()
    assert plan(Sc=0) != 0 and plan(Nc=0) != 0 and plan(Sc=4) != 0 and plan(Nc=6) != 0
    assert plan(steps=5) != 0 and b"the shapes make 6" in L.drn_last_error()


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_retrieve_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve.hip compiled for gfx950 on its own: every kernel of the file without scratch and without a spilled register, and
    static LDS exactly what its arrays come to -- 16 sentences x SL_BLOCK keys of 8 bytes for the ranking workgroup, 2 x SL_MAX_N keys
    for the merging wavefront, DRN_CANDIDATES_MAX words for a plan row."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    claims = {"shortlist_block_kernelIDF16b": 16 * _lib.SHORTLIST_BLOCK * 8, "shortlist_block_kernelIf": 16 * _lib.SHORTLIST_BLOCK * 8,
              "shortlist_merge_kernel": 2 * _lib.SHORTLIST_MAX * 8, "plan_candidates_kernel": _lib.CANDIDATES_MAX * 4}
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
