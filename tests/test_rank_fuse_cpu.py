"""Rank fusion, the host side: rank_fuse_reference and rank_fuse_rank_reference on hand-worked cases and against a brute-force Python
loop in numpy float32 (ties, repeats, junk entries, both `missing` modes, zero / negative / infinite weights, k0 = 0, masks), their
identities, the two C entries in the header, in _lib.SIGNATURES and in the built library at ABI 9, their argument checks -- which answer
before anything is launched, so they run without a GPU -- and the Python refusals, which are raised before the library is reached.
tests/test_rank_fuse_gpu.py holds the kernel."""
import ctypes

import numpy as np
import pytest
import torch

from test_fused_shortlist_cpu import bits, host_tables
from test_grounding_cpu import _header_params, built_lib
from test_q8_shortlist_cpu import _no_library, resident

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
f32 = np.float32


def vote(w, k0, j):
    """w / (k0 + float(j + 1)), each operation rounded to float32."""
    with np.errstate(all="ignore"):
        return f32(f32(w) / f32(f32(k0) + f32(j + 1)))


def loop_rrf(lists, V, w, k0, missing, allow=None):
    """The fusion by hand -> per sentence the (video, acc) candidates in the total order.  lists: M nested lists of S rows."""
    M, S = len(lists), len(lists[0])
    out = []
    for s in range(S):
        acc, held = {}, {}
        for m in range(M):
            seen = set()
            for j, v in enumerate(lists[m][s]):
                if 0 <= v < V and v not in seen:
                    seen.add(v)
                    with np.errstate(all="ignore"):
                        acc[v] = f32(acc.get(v, f32(0.0)) + vote(w[m], k0, j))
                    held[v] = held.get(v, 0) + 1
        rows = [(v, a) for v, a in acc.items() if np.isfinite(a) and (missing == "skip" or held[v] == M)
                and (allow is None or allow[s][v])]
        out.append(sorted(rows, key=lambda r: (-float(r[1]), r[0])))
    return out


def cut(rows, n):
    ids = [[v for v, _ in r[:n]] + [-1] * (n - len(r[:n])) for r in rows]
    scores = [[float(a) + 0.0 for _, a in r[:n]] + [0.0] * (n - len(r[:n])) for r in rows]
    return ids, torch.tensor(scores, dtype=torch.float32).view(len(rows), n), [min(len(r), n) for r in rows]


def same(got, rows, n, what=""):
    ids, scores, counts = cut(rows, n)
    assert got.ids.tolist() == ids and got.n.tolist() == counts, (what, got.ids.tolist(), ids)
    assert got.ids.dtype == torch.int32 and got.n.dtype == torch.int32 and got.scores.dtype == torch.float32
    assert torch.equal(bits(got.scores), bits(scores)), what


def t32(rows):
    return torch.tensor(rows, dtype=torch.int32)


# -- 1. hand-worked cases ----------------------------------------------------------------------------------------------------------------------

def test_two_lists_of_three_with_ties_decided_by_position():
    from drn_amd import Shortlist, rank_fuse_reference
    a, b = t32([[2, 0, 1]]), t32([[0, 2, 3]])
    got = rank_fuse_reference([a, b], 5, 4)
    assert isinstance(got, Shortlist)
    # videos 0 and 2 hold the ranks (1, 0) and (0, 1): the same two votes; 1 and 3 hold rank 2 in one list each
    top, low = f32(vote(1, 60, 0) + vote(1, 60, 1)), vote(1, 60, 2)
    assert got.ids.tolist() == [[0, 2, 1, 3]] and got.n.tolist() == [4]
    assert torch.equal(bits(got.scores), bits(torch.tensor([[top, top, low, low]], dtype=torch.float32)))
    assert float(got.scores[0, 0]) == float(f32(f32(1) / f32(61)) + f32(f32(1) / f32(62)))
    # the stacked tensor is the sequence; an int64 list too
    again = rank_fuse_reference(torch.stack([a, b]), 5, 4)
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    again = rank_fuse_reference([a.long(), b.long()], 5, 4)
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_a_repeat_and_junk_take_no_rank_but_keep_their_columns():
    from drn_amd import rank_fuse_reference
    # video 3 at column 0; its repeat at column 2 counts for nothing; -1, V, INT_MIN and INT_MAX mean nothing; video 1 sits at column 6
    row = [3, -1, 3, 7, INT_MIN, INT_MAX, 1]
    got = rank_fuse_reference([t32([row])], 7, 5)
    assert got.ids.tolist() == [[3, 1, -1, -1, -1]] and got.n.tolist() == [2]
    want = torch.tensor([[vote(1, 60, 0), vote(1, 60, 6), 0, 0, 0]], dtype=torch.float32)
    assert torch.equal(bits(got.scores), bits(want))              # (the rank is the COLUMN: 6, not the count of valid entries before)


def test_skip_against_drop():
    from drn_amd import rank_fuse_reference
    lists = [t32([[4, 1, 0]]), t32([[1, 2, -1]])]
    skip = rank_fuse_reference(lists, 5, 5)
    drop = rank_fuse_reference(lists, 5, 5, missing="drop")
    assert skip.ids.tolist() == [[1, 4, 2, 0, -1]] and skip.n.tolist() == [4]
    assert drop.ids.tolist() == [[1, -1, -1, -1, -1]] and drop.n.tolist() == [1]
    assert torch.equal(bits(drop.scores[:, :1]), bits(skip.scores[:, :1]))
    assert float(skip.scores[0, 0]) == float(f32(vote(1, 60, 1) + vote(1, 60, 0)))


def test_zero_negative_and_infinite_weights_and_k0_zero():
    from drn_amd import rank_fuse_reference
    lists = [t32([[0, 1, 2]]), t32([[2, 1, 3]])]
    # a zero weight: list 1 votes 0, its videos are candidates all the same (video 3 with the score 0, last)
    got = rank_fuse_reference(lists, 4, 4, weights=[1.0, 0.0])
    assert got.ids.tolist() == [[0, 1, 2, 3]] and float(got.scores[0, 3]) == 0.0 and got.n.tolist() == [4]
    # a negative weight: list 1 votes against; 0 (only in list 0) first, 3 (only in list 1, at rank 2) above 2 and 1
    got = rank_fuse_reference(lists, 4, 4, weights=[1.0, -2.0])
    same(got, loop_rrf([l.tolist() for l in lists], 4, [1.0, -2.0], 60.0, "skip"), 4)
    assert got.ids[0, 0].tolist() == 0 and float(got.scores[0, 3]) < 0
    # an infinite weight: what list 1 holds has a sum that is not finite and is no candidate
    got = rank_fuse_reference(lists, 4, 4, weights=[1.0, float("inf")])
    assert got.ids.tolist() == [[0, -1, -1, -1]] and got.n.tolist() == [1]
    got = rank_fuse_reference(lists, 4, 4, weights=torch.tensor([float("nan"), 1.0]))
    assert got.ids.tolist() == [[3, -1, -1, -1]] and float(got.scores[0, 0]) == float(vote(1, 60, 2))
    # k0 = 0: the votes are 1, 1/2, 1/3
    got = rank_fuse_reference(lists, 4, 4, k0=0)
    assert got.ids.tolist() == [[2, 0, 1, 3]]
    want = [f32(vote(1, 0, 2) + vote(1, 0, 0)), f32(1.0), f32(f32(0.5) + f32(0.5)), vote(1, 0, 2)]
    assert torch.equal(bits(got.scores), bits(torch.tensor([want], dtype=torch.float32)))
    assert float(got.scores[0, 0]) == float(f32(f32(1) / f32(3)) + f32(1)) and got.scores[0, 1:3].tolist() == [1.0, 1.0]


def test_n_larger_than_the_union_and_masks_shared_and_per_sentence():
    from drn_amd import rank_fuse_reference
    lists = [t32([[0, 1], [3, 2]]), t32([[1, 4], [2, 2]])]
    got = rank_fuse_reference(lists, 5, 9)
    assert tuple(got.ids.shape) == (2, 9) and got.n.tolist() == [3, 2]
    assert got.ids.tolist() == [[1, 0, 4] + [-1] * 6, [2, 3] + [-1] * 7] and bool((got.scores[:, 3:] == 0).all())
    shared = torch.tensor([True, False, True, True, True])
    got = rank_fuse_reference(lists, 5, 3, allow=shared)
    assert got.ids.tolist() == [[0, 4, -1], [2, 3, -1]] and got.n.tolist() == [2, 2]
    assert float(got.scores[0, 0]) == float(vote(1, 60, 0))     # (a masked video changes nothing for the others: ranks stay)
    each = torch.tensor([[False, True, True, True, False], [True, True, False, True, True]])
    got = rank_fuse_reference(lists, 5, 3, allow=each)
    assert got.ids.tolist() == [[1, -1, -1], [3, -1, -1]] and got.n.tolist() == [1, 1]


# -- 2. against the loop, and the identities ---------------------------------------------------------------------------------------------------

def random_lists(M, S, V, widths, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for m in range(M):
        c = torch.randint(-2, V + 2, (S, widths[m % len(widths)]), generator=g)
        c[0, 0] = INT_MAX if m % 2 else INT_MIN
        out.append(c.to(torch.int32))
    return out


@pytest.mark.parametrize("missing", ["skip", "drop"])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_the_reference_equals_the_loop(M, missing):
    from drn_amd import rank_fuse_rank_reference, rank_fuse_reference
    V, S = 12, 5
    lists = random_lists(M, S, V, (7, 4, 9), seed=M)
    w = [1.0, 0.5, -0.25, 0.0, 2.0, 1.0, 3.0, 0.125][:M]
    g = torch.Generator().manual_seed(100 + M)
    allow = torch.rand(S, V, generator=g) < 0.7
    for k0 in (0.0, 0.5, 60.0):
        for mask in (None, allow, allow[2].clone()):
            rows = None if mask is None else (mask if mask.dim() == 2 else mask[None].expand(S, V)).tolist()
            want = loop_rrf([l.tolist() for l in lists], V, w, k0, missing, rows)
            for n in (1, 5, 20):
                same(rank_fuse_reference(lists, V, n, weights=w, k0=k0, missing=missing, allow=mask), want, n, (k0, n))
            # the rank reference agrees with the list: rank = k exactly when ids[s, k] is the target
            full = rank_fuse_reference(lists, V, V, weights=w, k0=k0, missing=missing, allow=mask)
            for t in range(-1, V + 1):
                rk = rank_fuse_rank_reference(lists, V, [t] * S, weights=w, k0=k0, missing=missing, allow=mask)
                assert rk.total.tolist() == [len(r) for r in want] and rk.rank.dtype == torch.int32
                for s in range(S):
                    place = [k for k in range(V) if full.ids[s, k].tolist() == t and t >= 0]
                    assert rk.rank[s].tolist() == (place[0] if place else -1), (t, s)
                    score = full.scores[s, place[0]] if place else torch.zeros(())
                    assert torch.equal(bits(rk.score[s:s + 1]), bits(score.reshape(1)))
    ties = (full.scores[:, 1:] == full.scores[:, :-1]) & (full.ids[:, 1:] >= 0)
    assert bool((full.ids[:, 1:][ties] > full.ids[:, :-1][ties]).all()), "ties fall by position"


def test_one_list_of_weight_one_keeps_its_distinct_valid_entries_in_order():
    from drn_amd import rank_fuse_reference
    V = 9
    c = random_lists(1, 6, V, (11,), seed=4)[0]
    got = rank_fuse_reference([c], V, 11)
    for s, row in enumerate(c.tolist()):
        want = []
        for v in row:
            if 0 <= v < V and v not in want:
                want.append(v)
        assert got.ids[s].tolist() == want + [-1] * (11 - len(want)) and got.n[s].tolist() == len(want)
    # padding with -1 changes nothing, nor does a wider stacked buffer
    padded = torch.cat([c, torch.full((6, 5), -1, dtype=torch.int32)], dim=1)
    assert all(torch.equal(x, y) for x, y in zip(got, rank_fuse_reference(padded[None], V, 11)))


def test_the_references_refuse_what_the_definition_does_not_cover():
    from drn_amd import RANK_FUSE_MAX_LISTS, _lib, rank_fuse_rank_reference, rank_fuse_reference
    err = _lib.DrnError
    a = t32([[0, 1]])
    assert RANK_FUSE_MAX_LISTS == 8
    for k0 in (-1.0, float("inf"), float("nan"), 1e39, "60", None, True):
        with pytest.raises(err, match="k0"):
            rank_fuse_reference([a], 3, 2, k0=k0)
    with pytest.raises(err, match=r"9 lists outside \[1, 8\]"):
        rank_fuse_reference([a] * 9, 3, 2)
    with pytest.raises(err, match=r"0 lists outside \[1, 8\]"):
        rank_fuse_reference([], 3, 2)
    with pytest.raises(err, match="missing must be"):
        rank_fuse_reference([a], 3, 2, missing="mean")
    with pytest.raises(err, match="integer tensor"):
        rank_fuse_reference([a.float()], 3, 2)
    with pytest.raises(err, match="list 1 holds 2 sentences, list 0 holds 1"):
        rank_fuse_reference([a, t32([[0], [1]])], 3, 2)
    with pytest.raises(err, match=r"C = 1025 entries a sentence outside \[1, 1024\]"):
        rank_fuse_reference([torch.zeros(1, 1025, dtype=torch.int32)], 3, 2)
    for n in (0, 1025):
        with pytest.raises(err, match=r"n = %d outside \[1, 1024\]" % n):
            rank_fuse_reference([a], 3, n)
    with pytest.raises(err, match="V = 0 videos"):
        rank_fuse_reference([a], 0, 2)
    with pytest.raises(err, match="weights must be 2 float32 numbers"):
        rank_fuse_reference([a, a], 3, 2, weights=[1.0])
    with pytest.raises(err, match="allow must be a bool tensor"):
        rank_fuse_reference([a], 3, 2, allow=torch.ones(4, dtype=torch.bool))
    with pytest.raises(err, match="2 targets for 1 sentences"):
        rank_fuse_rank_reference([a], 3, [0, 1])
    assert "column" in rank_fuse_reference.__doc__ and "first occurrence" in rank_fuse_reference.__doc__
    assert "NOT" in rank_fuse_reference.__doc__ and "DEPTH" in rank_fuse_reference.__doc__


# -- 3. the C boundary -------------------------------------------------------------------------------------------------------------------------

ENTRIES = (("drn_rank_fuse_topn", 17), ("drn_rank_fuse_rank", 17))


def test_library_exports_the_two_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name, count in ENTRIES:
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("long long ") else ctypes.c_float \
                if p.startswith("float ") else ctypes.c_int
            assert t is want, (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig) and callable(getattr(ops, name[4:]))
    header = open(_lib.HEADER_PATH).read()
    assert "#define DRN_RANK_FUSE_MAX_LISTS %d\n" % _lib.RANK_FUSE_MAX_LISTS in header and _lib.RANK_FUSE_MAX_LISTS == 8
    assert _lib.FUSE_MODES == {"drop": 0, "skip": 1}
    for public in ("rank_fuse_reference", "rank_fuse_rank_reference", "rank_fuse", "rank_fuse_rank", "RankFusedShortlister",
                   "RANK_FUSE_MAX_LISTS"):
        assert hasattr(drn_amd, public), public


def test_the_two_entries_check_their_arguments_before_anything_is_launched():
    """Every call below is refused by the entry's own checks: nothing is launched, so no GPU is needed.  The pointers only have to be
    non-null and aligned."""
    lib = built_lib()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
    last = lambda: lib.drn_last_error().decode()

    # drn_rank_fuse_topn(lists, stride_m, ld, C, M, V, weights, k0, mode, allow, allow_stride, S, n, ids, scores, counts, stream)
    def topn(stride_m=80, ld=40, C=40, M=2, V=300, k0=60.0, mode=1, stride=0, S=2, n=4, ptrs=None):
        a = [p] * 6 if ptrs is None else ptrs             # lists weights allow | ids scores counts
        return lib.drn_rank_fuse_topn(a[0], stride_m, ld, C, M, V, a[1], k0, mode, a[2], stride, S, n, a[3], a[4], a[5], None)

    # drn_rank_fuse_rank(lists, stride_m, ld, C, M, V, weights, k0, mode, allow, allow_stride, S, targets, rank, score, total, stream)
    def rank(stride_m=80, ld=40, C=40, M=2, V=300, k0=60.0, mode=1, stride=0, S=2, ptrs=None):
        a = [p] * 7 if ptrs is None else ptrs             # lists weights allow | targets rank score total
        return lib.drn_rank_fuse_rank(a[0], stride_m, ld, C, M, V, a[1], k0, mode, a[2], stride, S, a[3], a[4], a[5], a[6], None)

    for call, name, count in ((topn, "drn_rank_fuse_topn", 6), (rank, "drn_rank_fuse_rank", 7)):
        for i in [0, 1] + list(range(3, count)):          # (null is a meaning for allow)
            assert call(ptrs=[None if j == i else p for j in range(count)]) != 0 and "%s: null pointer" % name in last(), (name, i)
        assert call(V=0) != 0 and "bad args" in last() and call(S=0) != 0 and "bad args" in last()
        for M in (0, 9):
            assert call(M=M) != 0 and "%s: M = %d lists outside [1, 8]" % (name, M) in last()
        for C in (0, 1025):
            assert call(C=C, ld=2000, stride_m=4000) != 0 and "%s: C = %d entries a list outside [1, 1024]" % (name, C) in last()
        for mode in (-1, 2):
            assert call(mode=mode) != 0 and "%s: mode = %d is neither 0 (drop) nor 1 (skip)" % (name, mode) in last()
        for k0 in (-1.0, float("inf"), float("nan")):
            assert call(k0=k0) != 0 and "is not a finite number >= 0" in last(), k0
        assert call(ld=39) != 0 and "%s: ld = 39 below C = 40" % name in last()
        assert call(stride_m=79) != 0 and "stride_m = 79 below the (S - 1) * ld + C = 80" in last()
        for stride in (1, 9, 11, 300):
            assert call(stride=stride) != 0 and "%s: allow_stride = %d is neither 0" % (name, stride) in last()
        assert call(ptrs=[odd if j == 2 else p for j in range(count)]) != 0 and "mask must be 4-byte aligned" in last()
        assert call(ptrs=[odd if j == 0 else p for j in range(count)]) != 0 and "lists and weights must be 4-byte aligned" in last()
        assert call(ptrs=[odd if j == count - 1 else p for j in range(count)]) != 0 and "must be 4-byte aligned" in last()
        assert call(S=65536, stride_m=40 * 65536) != 0 and "more than 65535 sentences" in last()
    for n in (0, 1025):
        assert topn(n=n) != 0 and "drn_rank_fuse_topn: n = %d outside [1, 1024]" % n in last()


# -- 4. the refusals of the Python layer -------------------------------------------------------------------------------------------------------

def test_rank_fuse_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops, rank_fuse, rank_fuse_rank
    _no_library(monkeypatch)
    err = _lib.DrnError
    a, b = resident(torch.zeros(2, 5, dtype=torch.int32)), resident(torch.zeros(2, 3, dtype=torch.int32))
    stacked = resident(torch.zeros(2, 2, 5, dtype=torch.int32))
    tgt = resident(torch.zeros(2, dtype=torch.int32))
    for call in (lambda lists, V=9, **kw: rank_fuse(lists, V, 4, **kw), lambda lists, V=9, **kw: rank_fuse_rank(lists, V, tgt, **kw)):
        with pytest.raises(err, match="on the GPU; there is no CPU fallback"):
            call([torch.zeros(2, 5, dtype=torch.int32)])                          # a host list
        with pytest.raises(err, match="on the GPU; there is no CPU fallback"):
            call(torch.zeros(1, 2, 5, dtype=torch.int32))
        with pytest.raises(err, match=r"contiguous \(S, C\) torch.int32"):
            call([resident(torch.zeros(2, 5, dtype=torch.int64))])
        with pytest.raises(err, match=r"contiguous \(S, C\) torch.int32"):
            call([resident(torch.zeros(2, 10, dtype=torch.int32))[:, ::2]])
        with pytest.raises(err, match=r"contiguous \(M, S, C\) torch.int32"):
            call(a)                                                               # a tensor is the stacked form
        with pytest.raises(err, match=r"9 lists outside \[1, 8\]"):
            call([a] * 9)
        with pytest.raises(err, match=r"9 lists outside \[1, 8\]"):
            call(resident(torch.zeros(9, 2, 5, dtype=torch.int32)))
        with pytest.raises(err, match=r"C = 1025 entries a sentence outside \[1, 1024\]"):
            call([resident(torch.zeros(2, 1025, dtype=torch.int32))])
        with pytest.raises(err, match="list 1 holds 3 sentences, list 0 holds 2"):
            call([a, resident(torch.zeros(3, 5, dtype=torch.int32))])
        with pytest.raises(err, match="V = 0 videos"):
            call([a], V=0)
        with pytest.raises(err, match="missing must be"):
            call([a], missing="mean")
        for k0 in (-0.5, float("inf"), float("nan"), 1e39, "60"):
            with pytest.raises(err, match="k0"):
                call([a, b], k0=k0)
        with pytest.raises(err, match="3 weights for 2 lists"):
            call([a, b], weights=[1.0, 2.0, 3.0])
        with pytest.raises(err, match="weights must be None, 2 numbers"):
            call([a, b], weights=["x", 1.0])
        with pytest.raises(err, match=r"contiguous \(2,\) torch.float32, one weight per list"):
            call(stacked, weights=torch.ones(2, dtype=torch.float64))
        with pytest.raises(err, match="bool tensor; pack it first"):
            call([a], allow=resident(torch.ones(9, dtype=torch.bool)))
        with pytest.raises(err, match=r"allow must be \(1,\)"):
            call([a], allow=resident(torch.zeros(2, dtype=torch.int32)))
    for n in (0, 1025):
        with pytest.raises(err, match=r"n = %d outside \[1, 1024\]" % n):
            rank_fuse([a, b], 9, n)
    with pytest.raises(err, match="three buffers of a Shortlist"):
        rank_fuse([a, b], 9, 4, out=(a, a))
    with pytest.raises(err, match=r"out.ids must be a contiguous \(2, 4\)"):
        rank_fuse([a, b], 9, 4, out=(a, resident(torch.zeros(2, 4)), tgt))
    with pytest.raises(err, match=r"targets must be a contiguous \(2,\) torch.int32"):
        rank_fuse_rank([a, b], 9, resident(torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(err, match="targets must be on the table's device"):
        rank_fuse_rank([a, b], 9, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(err, match="three buffers of a TargetRank"):
        rank_fuse_rank([a, b], 9, tgt, out=(tgt, tgt))
    # the wrappers under them refuse what the functions cannot meet
    w = resident(torch.ones(2))
    with pytest.raises(err, match="on the GPU only"):
        ops.rank_fuse_topn(torch.zeros(2, 2, 5, dtype=torch.int32), 9, w, 60.0, "skip", 4, None, None, None)
    with pytest.raises(err, match=r"lists must be \(M, S, C\) torch.int32"):
        ops.rank_fuse_topn(resident(torch.zeros(2, 2, 5)), 9, w, 60.0, "skip", 4, a, a, a)
    with pytest.raises(err, match="missing must be one of"):
        ops.rank_fuse_rank(stacked, 9, w, 60.0, "mean", tgt, tgt, tgt, tgt)
    with pytest.raises(err, match="k0 = -1.0 is not a finite number"):
        ops.rank_fuse_rank(stacked, 9, w, -1.0, "skip", tgt, tgt, tgt, tgt)
    with pytest.raises(err, match="lists that do not overlap"):
        ops.rank_fuse_topn(resident(torch.zeros(2, 5, dtype=torch.int32))[None].expand(2, 2, 5), 9, w, 60.0, "skip", 4, a, a, a)
    with pytest.raises(err, match=r"ids must be a contiguous \(2, 4\)"):
        ops.rank_fuse_topn(stacked, 9, w, 60.0, "skip", 4, a, a, a)


def test_the_class_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import FusedShortlister, RankFusedShortlister, ShardedShortlister, Shortlister, _lib
    from drn_amd._lib import SHORTLIST_MAX
    _no_library(monkeypatch)
    err = _lib.DrnError
    plain, ragged, q8 = host_tables()
    sharded = ShardedShortlister([plain])
    with pytest.raises(err, match="must be a sequence of Shortlister"):
        RankFusedShortlister(plain)
    with pytest.raises(err, match=r"RankFusedShortlister: 9 tables outside \[1, 8\]"):
        RankFusedShortlister([plain] * 9)
    with pytest.raises(err, match="table 1 must be a Shortlister or a ShardedShortlister, not FusedShortlister"):
        RankFusedShortlister([plain, FusedShortlister([plain])])
    with pytest.raises(err, match="table 1 holds 4 videos, table 0 holds 3"):
        RankFusedShortlister([plain, Shortlister(resident(torch.zeros(4, 8)))])
    with pytest.raises(err, match="the names of table 1 are not those of the tables before it"):
        RankFusedShortlister([plain, Shortlister(resident(torch.zeros(3, 8)), names=["a", "c", "b"])])
    with pytest.raises(err, match="missing must be"):
        RankFusedShortlister([plain], missing="mean")
    for k0 in (-1.0, float("nan"), None):
        with pytest.raises(err, match="k0"):
            RankFusedShortlister([plain], k0=k0)
    for depth in (0, 1025):
        with pytest.raises(err, match=r"depth = %d outside \[1, 1024\]" % depth):
            RankFusedShortlister([plain], depth=depth)
    with pytest.raises(err, match="table 1 is a ShardedShortlister, which has no deep entry"):
        RankFusedShortlister([plain, sharded], depth=SHORTLIST_MAX + 1)
    with pytest.raises(err, match="2 weights for 3 tables"):
        RankFusedShortlister([plain, ragged, q8], weights=[1.0, 2.0])
    rf = RankFusedShortlister([plain, ragged, q8, sharded], weights=[1.0, 0.5, 0.0, -1.0], k0=0.5, depth=SHORTLIST_MAX)
    assert rf.names == ["a", "b", "c"] and len(rf) == 3 and rf.device == plain.device and rf.depth == 128 and rf.k0 == 0.5
    assert rf.missing == "skip" and rf.weights.tolist() == [1.0, 0.5, 0.0, -1.0] and rf.tables == [plain, ragged, q8, sharded]
    qp, qr = resident(torch.zeros(2, 32, dtype=torch.bfloat16)), resident(torch.zeros(2, 8))
    late = (resident(torch.zeros(2, 4, 64, dtype=torch.bfloat16)), resident(torch.zeros(2, dtype=torch.int32)))
    items, tgt = [qp, qr, late, qp], resident(torch.zeros(2, dtype=torch.int32))
    for call in (lambda q, **kw: rf.shortlist(q, 4, **kw), lambda q, **kw: rf.rank(q, tgt, **kw)):
        with pytest.raises(err, match="a sequence of 4 items"):
            call(qp)
        with pytest.raises(err, match=r"table 0\): the queries must be on the table's device"):
            call([torch.zeros(2, 32, dtype=torch.bfloat16), qr, late, qp])
        with pytest.raises(err, match="item 1 holds 3 sentences, item 0 holds 2"):
            call([qp, resident(torch.zeros(3, 8)), late, qp])
        with pytest.raises(err, match="one row per video"):
            call([(resident(torch.zeros(2, 4, 32, dtype=torch.bfloat16)), late[1]), qr, late, qp])
        with pytest.raises(err, match="bool tensor; pack it first"):
            call(items, allow=resident(torch.ones(3, dtype=torch.bool)))
    for n in (0, 1025):
        with pytest.raises(err, match=r"n = %d outside \[1, 1024\]" % n):
            rf.shortlist(items, n)
    with pytest.raises(err, match="three buffers of a Shortlist"):
        rf.shortlist(items, 4, out=(tgt, tgt))
    with pytest.raises(err, match=r"targets must be a contiguous \(2,\) torch.int32"):
        rf.rank(items, [0, 1])
    with pytest.raises(err, match="three buffers of a TargetRank"):
        rf.rank(items, tgt, out=(tgt,))
    # a late item at depth: refused in the call, before any launch, and it says why
    deep = RankFusedShortlister([plain, q8], depth=300)
    with pytest.raises(err, match="item 1 selects late interaction, which has no deep entry"):
        deep.shortlist([qp, late], 4)
    with pytest.raises(err, match="item 1 selects late interaction, which has no deep entry"):
        deep.rank([qp, late], tgt)
    assert not hasattr(FusedShortlister, "k0")                                   # (FusedShortlister keeps its surface)
