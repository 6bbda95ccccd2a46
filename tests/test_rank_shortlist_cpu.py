"""The rank of a target video in the full shortlist order, the host side: rank_reference, segment_rank_reference and late_rank_reference
(the definitions) on hand-computed cases and against the lists of the three shortlist references; the refusals of Shortlister.rank and
rank_late that need no GPU; the three C entries at ABI 9 and what they refuse before any launch; metrics.recall_from_ranks; and the
compiler's resource notes for csrc/retrieve_rank.hip.  tests/test_rank_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_late_shortlist_cpu import Resident, _no_library, _stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("drn_shortlist_rank", "drn_shortlist_segments_rank", "drn_shortlist_late_rank")
NAN = float("nan")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# -- the definitions ---------------------------------------------------------------------------------------------------------------------

def test_rank_reference_on_a_hand_computed_case():
    """E = 1, q = 1: the scores are the table.  Videos 1, 3 and 5 tie at 5; 0 is the best; 6 is NaN; 2 and 4 lie below."""
    from drn_amd import TargetRank, rank_reference
    emb = torch.tensor([[7.], [5.], [1.], [5.], [-2.], [5.], [NAN]])
    q = torch.ones(9, 1)
    targets = [0, 1, 3, 5, 2, 4, 6, -1, 7]
    got = rank_reference(emb, q, targets)
    assert isinstance(got, TargetRank) and got._fields == ("rank", "score", "total")
    assert got.rank.dtype == got.total.dtype == torch.int32 and got.score.dtype == torch.float32
    assert got.rank.shape == got.score.shape == got.total.shape == (9,)
    # a tie after the target (1), before and after (3), before (5); a NaN target and the two values outside [0, V) give -1
    assert got.rank.tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1]
    assert got.score.tolist() == [7., 5., 5., 5., 1., -2., 0., 0., 0.]
    assert got.total.tolist() == [6] * 9
    # the targets may be a list, an int64 or an int32 tensor; INT_MIN and INT_MAX are legal
    for t in (torch.tensor(targets), torch.tensor(targets, dtype=torch.int32)):
        assert all(torch.equal(a, b) for a, b in zip(rank_reference(emb, q, t), got))
    far = rank_reference(emb, q[:2], [INT_MIN, INT_MAX])
    assert far.rank.tolist() == [-1, -1] and far.score.tolist() == [0., 0.] and far.total.tolist() == [6, 6]
    # a masked target gives -1; a masked rival is not counted, and the others' ranks are what they were without it
    allow = torch.tensor([True, False, True, True, True, True, True])
    masked = rank_reference(emb, q, targets, allow=allow)
    assert masked.rank.tolist() == [0, -1, 1, 2, 3, 4, -1, -1, -1] and masked.total.tolist() == [5] * 9
    assert masked.score.tolist() == [7., 0., 5., 5., 1., -2., 0., 0., 0.]
    per = torch.ones(9, 7, dtype=torch.bool)
    per[2, 0] = per[2, 1] = False                                            # sentence 2 alone loses the two videos ahead of its target
    got2 = rank_reference(emb, q, targets, allow=per)
    assert got2.rank.tolist() == [0, 1, 0, 3, 4, 5, -1, -1, -1] and got2.total.tolist() == [6, 6, 4, 6, 6, 6, 6, 6, 6]
    # a NaN query row has no candidate
    qn = q.clone()
    qn[4, 0] = NAN
    got3 = rank_reference(emb, qn, targets)
    assert got3.rank.tolist() == [0, 1, 2, 3, -1, 5, -1, -1, -1] and got3.total.tolist() == [6, 6, 6, 6, 0, 6, 6, 6, 6]
    with pytest.raises(Exception, match="targets for 9 sentences"):
        rank_reference(emb, q, targets[:4])


def test_segment_rank_reference_on_a_hand_computed_case():
    """Best rows: v0 = 4, v1 owns no row, v2 = 6 (its second row), v3 = 4 (a tie with v0), v4 = NaN, v5 = 6 (a tie with v2)."""
    from drn_amd import segment_rank_reference
    emb = torch.tensor([[4.], [1.], [6.], [4.], [-1.], [NAN], [2.], [6.]])
    off = [0, 1, 1, 3, 5, 7, 8]
    q = torch.ones(8, 1)
    targets = [0, 1, 2, 3, 4, 5, 6, -9]
    got = segment_rank_reference(emb, off, q, targets)
    assert got.rank.tolist() == [2, -1, 0, 3, -1, 1, -1, -1]
    assert got.score.tolist() == [4., 0., 6., 4., 0., 6., 0., 0.] and got.total.tolist() == [4] * 8
    masked = segment_rank_reference(emb, off, q, targets, allow=torch.tensor([True, True, False, True, True, True]))
    assert masked.rank.tolist() == [1, -1, -1, 2, -1, 0, -1, -1] and masked.total.tolist() == [3] * 8


def test_late_rank_reference_on_a_hand_computed_case():
    """The tie case of tests/test_late_shortlist_cpu.py: videos 0 and 3 own no row; 1, 2 and 4 reach 8 for sentence 0."""
    from drn_amd import late_rank_reference
    emb = torch.tensor([[3., 0.], [0., 5.], [4., 4.], [5., 0.], [0., 3.], [1., 1.]])
    off = [0, 0, 2, 3, 3, 5, 6]
    q = torch.tensor([[[1., 0.], [0., 1.]], [[1., 0.], [1., 0.]], [[1., 0.], [0., 1.]], [[1., 0.], [0., 1.]]])
    got = late_rank_reference(emb, off, q, [2, 2, 2, 0], [4, 4, 0, 2])
    # sentence 0: [1, 2, 4, 5]; sentence 1: [4, 2, 1, 5]; sentence 2 asks for a video without rows; sentence 3 has no live token
    assert got.rank.tolist() == [2, 0, -1, -1] and got.score.tolist() == [8., 10., 0., 0.] and got.total.tolist() == [4, 4, 4, 0]
    shared = late_rank_reference(emb, off, q, [2, 2, 2, 2], [4, 2, 5, 1], allow=torch.tensor([True, False, True, True, True, False]))
    assert shared.rank.tolist() == [1, 1, -1, -1] and shared.total.tolist() == [2] * 4


def small_tables():
    g = torch.Generator().manual_seed(11)
    lens = [1, 3, 0, 4, 2, 0, 1, 2, 1]
    emb = torch.randint(-3, 4, (sum(lens), 6), generator=g).float()
    emb[4], emb[9], emb[12] = emb[0], emb[1], emb[0]                         # planted equal scores across videos
    off = [0] + torch.tensor(lens).cumsum(0).tolist()
    q = torch.randint(-3, 4, (4, 3, 6), generator=g).float()
    q[2, 0, 1] = NAN                                                         # (a sentence without candidates, pooled or not)
    return emb, off, q


def test_a_rank_is_the_place_in_every_list_long_enough():
    """rank[s] = k >= 0 exactly when the list of every n > k holds the target at place k, with its score; -1 exactly when no list holds
    it -- every video of a small table as the target, the three definitions, with and without a mask."""
    from drn_amd import (late_rank_reference, late_shortlist_reference, rank_reference, segment_rank_reference,
                         segment_shortlist_reference, shortlist_reference)
    emb, off, q3 = small_tables()
    q, lengths = q3[:, 0].contiguous(), [3, 1, 2, 0]
    S = 4
    cases = []
    for allow in (None, torch.arange(emb.shape[0]) % 4 != 1):
        cases.append((int(emb.shape[0]), lambda t, a=allow: rank_reference(emb, q, t, allow=a),
                      lambda n, a=allow: shortlist_reference(emb, q, n, allow=a)))
    V = len(off) - 1
    for allow in (None, torch.arange(V) % 3 != 1, torch.rand(S, V, generator=torch.Generator().manual_seed(2)) < 0.6):
        cases.append((V, lambda t, a=allow: segment_rank_reference(emb, off, q, t, allow=a),
                      lambda n, a=allow: segment_shortlist_reference(emb, off, q, n, allow=a)))
        cases.append((V, lambda t, a=allow: late_rank_reference(emb, off, q3, lengths, t, allow=a),
                      lambda n, a=allow: late_shortlist_reference(emb, off, q3, lengths, n, allow=a)))
    found = missed = 0
    for size, rank_of, list_of in cases:
        lists = {n: list_of(n) for n in range(1, size + 2)}
        assert torch.equal(rank_of([0] * S).total, lists[size + 1].n)
        for t in range(size):
            got = rank_of([t] * S)
            for s in range(S):
                k = int(got.rank[s])
                if k < 0:
                    assert t not in lists[size + 1].ids[s].tolist() and float(got.score[s]) == 0.0
                    missed += 1
                    continue
                found += 1
                for n in range(1, size + 2):
                    if n > k:
                        assert int(lists[n].ids[s, k]) == t and float(lists[n].scores[s, k]) == float(got.score[s]), (t, s, n)
                    else:
                        assert t not in lists[n].ids[s].tolist()
    assert found > 100 and missed > 50


def test_late_rank_with_one_token_is_the_segment_rank():
    from drn_amd import late_rank_reference, segment_rank_reference
    emb, off, q3 = small_tables()
    q = q3[:, 1].contiguous()
    for allow in (None, torch.arange(len(off) - 1) % 3 != 0):
        for t in range(-1, len(off)):
            a = segment_rank_reference(emb, off, q, [t] * 4, allow=allow)
            b = late_rank_reference(emb, off, q[:, None, :], torch.ones(4, dtype=torch.int32), [t] * 4, allow=allow)
            assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)), t


def test_recall_from_ranks_on_a_hand_case():
    from drn_amd import metrics
    ranks = np.array([0, 3, -1, 9, 10, 0, 999, -1], dtype=np.int32)
    assert metrics.recall_from_ranks(ranks, (1, 10, 100, 1000)) == [2 / 8, 4 / 8, 5 / 8, 6 / 8]
    assert metrics.recall_from_ranks(ranks.tolist(), [4]) == [3 / 8]
    assert metrics.recall_from_ranks([], (1, 5)) == [0.0, 0.0]
    assert metrics.mrr_from_ranks(ranks) == pytest.approx((1 + 1 / 4 + 0 + 1 / 10 + 1 / 11 + 1 + 1 / 1000 + 0) / 8, abs=1e-15)
    assert metrics.mrr_from_ranks([]) == 0.0
    # a miss counts as infinitely deep: sorted, the ranks are 0 0 3 9 | 10 999 inf inf
    assert metrics.median_rank_from_ranks(ranks) == 9.5
    assert metrics.median_rank_from_ranks([-1, 2, -1]) == float("inf") and metrics.median_rank_from_ranks([4, 2, -1]) == 4.0
    assert metrics.median_rank_from_ranks([]) != metrics.median_rank_from_ranks([])         # (nan)


# -- refusals, before the library is reached -------------------------------------------------------------------------------------------------

def _res(t):
    return t.as_subclass(Resident)


def test_rank_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    plain = Shortlister.__new__(Shortlister)
    plain.embeddings, plain.names, plain._ws, plain._seg = torch.zeros(6, 32, dtype=torch.bfloat16), None, {}, None
    q = torch.zeros(2, 32, dtype=torch.bfloat16)
    t = torch.tensor([1, 5], dtype=torch.int32)
    for sl in (plain, _stand_in()):
        with pytest.raises(_lib.DrnError, match="Shortlister.rank: the queries must be a tensor"):
            sl.rank([[1.0]], _res(t))
        for bad in (torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(0, 32, dtype=torch.bfloat16), torch.zeros(2, 1, 32, dtype=torch.bfloat16)):
            with pytest.raises(_lib.DrnError, match=r"must be \(S, 32\)"):
                sl.rank(_res(bad), _res(t))
        with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
            sl.rank(_res(q.float()), _res(t))
        with pytest.raises(_lib.DrnError, match="no CPU fallback"):
            sl.rank(q, _res(t))                                              # host queries
        for bad in (t.long(), t.float(), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                    torch.zeros(4, dtype=torch.int32)[::2], [1, 5]):
            with pytest.raises(_lib.DrnError, match=r"targets must be a contiguous \(2,\) torch.int32"):
                sl.rank(_res(q), _res(bad) if torch.is_tensor(bad) else bad)
        with pytest.raises(_lib.DrnError, match="never read on the host"):
            sl.rank(_res(q), t)                                              # host targets
        good = lambda: [_res(torch.zeros(2, dtype=torch.int32)), _res(torch.zeros(2)), _res(torch.zeros(2, dtype=torch.int32))]
        with pytest.raises(_lib.DrnError, match="three buffers"):
            sl.rank(_res(q), _res(t), out=good()[:2])
        for i, name in enumerate(("rank", "score", "total")):
            for wrong in (_res(torch.zeros(3, dtype=good()[i].dtype)), _res(torch.zeros(2, dtype=torch.float64)),
                          torch.zeros(2, dtype=good()[i].dtype), _res(torch.zeros(4, dtype=good()[i].dtype)[::2]), None):
                out = good()
                out[i] = wrong
                with pytest.raises(_lib.DrnError, match="out.%s must be a contiguous" % name):
                    sl.rank(_res(q), _res(t), out=out)
        # allow=: the refusals of shortlist(allow=) -- at most 6 videos are one word
        for bad, match in ((torch.ones(len(sl), dtype=torch.bool), "pack it first"), (torch.zeros(1, dtype=torch.int64), "torch.int32 packed words"),
                           (torch.zeros(1, dtype=torch.int32), "on the table's device"), ([1], "packed mask")):
            with pytest.raises(_lib.DrnError, match=match):
                sl.rank(_res(q), _res(t), allow=bad)
    sq = _stand_in("mxfp8")
    with pytest.raises(_lib.DrnError, match="the table is torch.float32"):
        sq.rank(_res(q), _res(t))


def test_rank_late_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import Shortlister, _lib
    _no_library(monkeypatch)
    sl = _stand_in()
    q = torch.zeros(2, 3, 32, dtype=torch.bfloat16)
    lengths, t = torch.tensor([3, 1], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(_lib.DrnError, match="Shortlister.rank_late: the queries must be a tensor"):
        sl.rank_late([[1.0]], _res(lengths), _res(t))
    for bad in (torch.zeros(2, 32, dtype=torch.bfloat16), torch.zeros(2, 3, 16, dtype=torch.bfloat16), torch.zeros(0, 3, 32, dtype=torch.bfloat16)):
        with pytest.raises(_lib.DrnError, match=r"must be \(S, L, 32\)"):
            sl.rank_late(_res(bad), _res(lengths), _res(t))
    for L in (0, 65):
        with pytest.raises(_lib.DrnError, match=r"L = %d tokens outside \[1, 64\]" % L):
            sl.rank_late(_res(torch.zeros(2, L, 32, dtype=torch.bfloat16)), _res(lengths), _res(t))
    with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
        sl.rank_late(_res(q.float()), _res(lengths), _res(t))
    with pytest.raises(_lib.DrnError, match="no CPU fallback"):
        sl.rank_late(q, _res(lengths), _res(t))
    with pytest.raises(_lib.DrnError, match="queries must be contiguous"):
        sl.rank_late(_res(torch.zeros(2, 6, 32, dtype=torch.bfloat16)[:, ::2]), _res(lengths), _res(t))
    for bad in (lengths.long(), torch.zeros(3, dtype=torch.int32), [3, 1]):
        with pytest.raises(_lib.DrnError, match=r"lengths must be a contiguous \(2,\) torch.int32"):
            sl.rank_late(_res(q), _res(bad) if torch.is_tensor(bad) else bad, _res(t))
    with pytest.raises(_lib.DrnError, match="lengths must be on the table's device"):
        sl.rank_late(_res(q), lengths, _res(t))
    for bad in (t.long(), torch.zeros(3, dtype=torch.int32), [0, 2]):
        with pytest.raises(_lib.DrnError, match=r"targets must be a contiguous \(2,\) torch.int32"):
            sl.rank_late(_res(q), _res(lengths), _res(bad) if torch.is_tensor(bad) else bad)
    with pytest.raises(_lib.DrnError, match="targets must be on the table's device"):
        sl.rank_late(_res(q), _res(lengths), t)
    with pytest.raises(_lib.DrnError, match="three buffers"):
        sl.rank_late(_res(q), _res(lengths), _res(t), out=[])
    with pytest.raises(_lib.DrnError, match="pack it first"):
        sl.rank_late(_res(q), _res(lengths), _res(t), allow=torch.ones(3, dtype=torch.bool))
    # a table without offsets is refused with shortlist_late's reason
    plain = Shortlister.__new__(Shortlister)
    plain.embeddings, plain.names, plain._ws, plain._seg = torch.zeros(6, 32, dtype=torch.bfloat16), None, {}, None
    with pytest.raises(_lib.DrnError, match=r"one row per video.*\(sum_t q_t\) \. emb_v.*call rank\(\)"):
        plain.rank_late(_res(q), _res(lengths), _res(t))


def test_evaluate_shortlist_resolves_names_before_anything_else(monkeypatch):
    from drn_amd import _lib, evaluate_shortlist
    _no_library(monkeypatch)
    sl = _stand_in()
    with pytest.raises(_lib.DrnError, match="no video named nobody"):
        evaluate_shortlist(sl, [(["a", "nobody"], None)])
    with pytest.raises(_lib.DrnError, match="at least one top-k"):
        evaluate_shortlist(sl, [], topks=())
    sl.names = None
    with pytest.raises(_lib.DrnError, match="has no names"):
        evaluate_shortlist(sl, [])
    got = evaluate_shortlist(_stand_in(), [], topks=(1, 200))
    assert got.n == 0 and got.topks == [1, 200] and got.recall == [0.0, 0.0] and got.mrr == 0.0 and got.ranks.shape == (0,)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_rank_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name, count in zip(ENTRIES, (16, 20, 22)):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
    for public in ("TargetRank", "rank_reference", "segment_rank_reference", "late_rank_reference", "evaluate_shortlist", "ShortlistRecall"):
        assert hasattr(drn_amd, public), public
    assert callable(drn_amd.Shortlister.rank) and callable(drn_amd.Shortlister.rank_late)
    assert callable(ops.shortlist_rank) and callable(ops.shortlist_segments_rank) and callable(ops.shortlist_late_rank)
    assert ops.shortlist_rank_ws_bytes(1, 1) == 16 and ops.shortlist_rank_ws_bytes(4, 17) == 8 * 17 * 5
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_rank.hip")).read()
    assert int(re.search(r"#define RK_BLOCK\s+(\d+)", src).group(1)) == _lib.SHORTLIST_SEG_BLOCK == _lib.SHORTLIST_BLOCK


def test_the_rank_entries_check_their_arguments_before_anything_is_launched():
    lib = built_lib()
    p = ctypes.c_void_p(0x1000)

    def plain(V=300, E=64, S=2, dtype=1, nbytes=1 << 20, stride=0, ptrs=None, **_):
        a = [p] * 9 if ptrs is None else ptrs                                # table scales queries targets allow ws | rank score total
        return lib.drn_shortlist_rank(a[0], a[1], a[2], a[3], a[4], stride, V, E, S, dtype, a[5], nbytes, a[6], a[7], a[8], None)

    def ragged(R=900, V=300, nblocks=2, E=64, S=2, dtype=1, nbytes=1 << 20, stride=0, ptrs=None, **_):
        a = [p] * 11 if ptrs is None else ptrs                               # table scales queries offsets blk_vid targets allow ws | ...
        return lib.drn_shortlist_segments_rank(a[0], a[1], a[2], a[3], a[4], a[5], a[6], stride, R, V, nblocks, E, S, dtype, a[7], nbytes,
                                               a[8], a[9], a[10], None)

    def late(R=900, V=300, nblocks=2, E=64, S=2, L=4, dtype=1, nbytes=1 << 20, stride=0, ptrs=None):
        a = [p] * 12 if ptrs is None else ptrs                               # table scales queries lengths offsets blk_vid targets allow ws | ...
        return lib.drn_shortlist_late_rank(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], stride, R, V, nblocks, E, S, L, dtype, a[8], nbytes,
                                           a[9], a[10], a[11], None)
    for fn, nptr, mask_at, ws_at in ((plain, 9, 4, 5), (ragged, 11, 6, 7), (late, 12, 7, 8)):
        for i in range(nptr):
            if i in (1, mask_at):                                            # (no scales is a plain table, no mask no filter: no error)
                continue
            assert fn(ptrs=[None if j == i else p for j in range(nptr)]) != 0 and b"null pointer" in lib.drn_last_error(), (fn.__name__, i)
        assert fn(V=0) != 0 and fn(E=0) != 0 and fn(S=0) != 0 and b"bad args" in lib.drn_last_error()
        assert fn(dtype=2) != 0 and b"dtype" in lib.drn_last_error()
        for at in (0, 2):                                                    # the table, the queries
            assert fn(ptrs=[ctypes.c_void_p(0x1008) if j == at else p for j in range(nptr)]) != 0 and b"16-byte aligned" in lib.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1004) if j == ws_at else p for j in range(nptr)]) != 0 and b"8-byte aligned" in lib.drn_last_error()
        assert fn(ptrs=[ctypes.c_void_p(0x1002) if j == mask_at - 1 else p for j in range(nptr)]) != 0 \
            and b"targets and lengths must be 4-byte aligned" in lib.drn_last_error()
        for E in (8, 48, 33, 500):
            assert fn(E=E) != 0 and b"not a multiple of the block of 32 columns" in lib.drn_last_error(), E
            ptrs = [None if j == 1 else p for j in range(nptr)]              # (without scales any E >= 1 passes this check)
            assert fn(E=E, ptrs=ptrs, nbytes=0) != 0 and b"are needed" in lib.drn_last_error(), E
        for stride in (1, 9, 11, -10, 300):
            assert fn(stride=stride) != 0 and b"neither 0" in lib.drn_last_error() and b"ceil(V / 32) = 10" in lib.drn_last_error(), stride
        assert fn(ptrs=[ctypes.c_void_p(0x1002) if j == mask_at else p for j in range(nptr)]) != 0 \
            and b"mask must be 4-byte aligned" in lib.drn_last_error()
        assert fn(nbytes=8 * 2 * 3 - 1) != 0 and b"48 are needed" in lib.drn_last_error()            # (two blocks either way)
        assert fn(V=1 << 30, nblocks=1 << 22, S=1 << 10, nbytes=0x7fffffff) != 0 and b"are needed" in lib.drn_last_error()  # (no int overflow)
    assert plain(S=16 * 65535 + 1, nbytes=0x7fffffff) != 0 and b"more than 65535 tiles" in lib.drn_last_error()
    assert ragged(S=16 * 65535 + 1, nbytes=0x7fffffff) != 0 and b"more than 65535 tiles" in lib.drn_last_error()
    assert late(S=65536, nbytes=0x7fffffff) != 0 and b"more than 65535 sentences" in lib.drn_last_error()
    for fn in (ragged, late):
        assert fn(R=0) != 0 and b"bad args" in lib.drn_last_error()
        for nblocks in (0, 1, 301):
            assert fn(nblocks=nblocks) != 0 and b"blocks outside" in lib.drn_last_error(), nblocks
    for L in (0, -1, 65):
        assert late(L=L) != 0 and b"tokens outside [1, 64]" in lib.drn_last_error(), L
    assert late(ptrs=[ctypes.c_void_p(0x1002) if j == 3 else p for j in range(12)]) != 0 and b"4-byte aligned" in lib.drn_last_error()


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_rank_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_rank.hip compiled for gfx950 on its own: five kernel bodies instantiated for the four table operands each, and the
    reduce -- 21 kernels, each without scratch and without a spilled register, and static LDS exactly what its arrays come to.  The two
    counting kernels of the ragged tables hold the 32 KiB of states and the 16 x 257 scores of the kernels they follow: three workgroups
    -- three wavefronts a SIMD -- share a CU, which leaves each 512 / 3 registers, so VGPRs + AGPRs stay at or below 168."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_rank.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_rank.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    B = _lib.SHORTLIST_SEG_BLOCK
    states, scores, voff = 16 * B * 8, 16 * (B + 1) * 4, (B + 4) * 4
    claims = {
        "rank_target_kernel": 0,
        "rank_target_rows_kernel": 4 * 16 * 4 + 16 * 4,                      # wmax, st
        "rank_block_kernel": 16 * 8 * 4 + 4 * 4 + 4 * 16 * 4,                # mw, wany, wc
        "rank_segments_kernel": states + scores + voff + 4 * 4 + 16 * 9 * 4 + 4 * 4 + 16 * 8 + 16 * 4 * 4,   # ... wlong, mw, wany, tk, wc
        "rank_late_kernel": states + scores + voff + B * 4 + 4 * 4 + 4 * 4,  # ... sums, wlong, wc
        "rank_reduce_kernel": 0,
    }
    assert claims["rank_segments_kernel"] == 51248 and claims["rank_late_kernel"] == 51312
    assert all(3 * c <= 160 * 1024 for c in claims.values())
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_rank.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == list(claims)
    seen = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        seen[name] = (get("group_segment_fixed_size"), get("private_segment_fixed_size"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                      get("vgpr_count") + int(blk.split()[0]))
    assert len(seen) == 21, sorted(seen)
    for body, lds_claim in claims.items():
        mine = [k for k in seen if re.search(r"\d%sI" % body, k) or (body == "rank_reduce_kernel" and body in k)]
        assert len(mine) == (1 if body == "rank_reduce_kernel" else 4), (body, sorted(seen))
        if len(mine) == 4:
            assert sorted(("AlQ8" in k, "DF16b" in k) for k in mine) == [(False, False), (False, True), (True, False), (True, True)], mine
        for name in mine:
            lds, scratch, vspill, sspill, regs = seen[name]
            assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
            assert lds == lds_claim and regs <= 168, (name, lds, regs)
