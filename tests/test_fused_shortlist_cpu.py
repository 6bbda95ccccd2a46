"""Dense scores and fused shortlists, the host side: the fold of fuse_scores_reference is a stated ORDER (not a sum, not an FMA), drop
and skip differ where they should, scores_reference agrees with the shortlist references it shares its scores with, every refusal
happens before the library is reached, and the three C entries stand in the header, in _lib.SIGNATURES and in the built library at ABI 9
with kernels that do not spill.  tests/test_fused_shortlist_gpu.py holds the kernels."""
import ctypes
import re

import numpy as np
import pytest
import torch

from test_allow_shortlist_cpu import exact_host, masks_of, same
from test_grounding_cpu import _header_params, built_lib
from test_kernel_resources_cpu import kernel_table
from test_q8_shortlist_cpu import _no_library, resident

NINF = float("-inf")


def bits(t):
    return t.contiguous().view(torch.int32)


def dense_of(short, V):
    """A complete list (n >= V) -> (S, V) float32 with -inf where a video is not listed."""
    out = torch.full((short.ids.shape[0], V + 1), NINF, dtype=torch.float32)
    at = torch.where(short.ids >= 0, short.ids.long(), torch.full_like(short.ids, V).long())
    return out.scatter_(1, at, torch.where(short.ids >= 0, short.scores, torch.full_like(short.scores, NINF)))[:, :V]


def ragged_offsets(R):
    """Run lengths cycling 1 / 3 / 0 / 17 over R rows -> V + 1 offsets."""
    lens, left = [], R
    while left:
        lens.append(min((1, 3, 0, 17)[len(lens) % 4], left))
        left -= lens[-1]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# -- 1. the fold is not a sum ------------------------------------------------------------------------------------------------------------------

def test_the_fold_has_an_order_and_two_roundings_a_term():
    from drn_amd import fuse_scores_reference
    # (a) the order: ((0 + 1e8) + 1) - 1e8 = 0 in fp32 (1e8 + 1 rounds back to 1e8), while (0 + 1e8 - 1e8) + 1 = 1
    terms = [1e8, 1.0, -1e8]
    sc = torch.tensor(terms, dtype=torch.float32).view(3, 1, 1)
    fused, cand = fuse_scores_reference(sc, [1.0, 1.0, 1.0])
    assert bool(cand.all()) and float(fused) == 0.0
    other, _ = fuse_scores_reference(sc[[0, 2, 1]], [1.0, 1.0, 1.0])
    assert float(other) == 1.0
    assert float(sc.sum()) in (0.0, 1.0)                     # (whatever torch.sum does, the definition does not ask it)
    # (b) no FMA: w * s = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds (to even) to 1 + 2^-11, and -(1 + 2^-11) + that = 0; one rounding
    # of acc + w * s would leave 2^-24
    a, b = 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -11)
    sc = torch.tensor([b, a], dtype=torch.float32).view(2, 1, 1)
    assert float(sc[0]) == b and float(sc[1]) == a
    fused, cand = fuse_scores_reference(sc, [1.0, a])
    assert bool(cand.all()) and float(fused) == 0.0 and not np.signbit(float(fused))
    fma = np.float32(np.float64(a) * np.float64(a) + np.float64(b))          # (exact in float64, then ONE rounding)
    assert float(fma) == 2.0 ** -24
    # (c) a sequence of matrices and a stacked tensor are the same input; weights None = all ones
    g = torch.Generator().manual_seed(3)
    mats = [torch.randn(4, 9, generator=g) for _ in range(3)]
    x, y = fuse_scores_reference(mats, None), fuse_scores_reference(torch.stack(mats), [1, 1, 1])
    assert torch.equal(bits(x[0]), bits(y[0])) and torch.equal(x[1], y[1])
    want = ((torch.zeros(4, 9) + mats[0]) + mats[1]) + mats[2]
    assert torch.equal(bits(x[0]), bits(want))


def test_drop_and_skip_differ_where_a_term_is_missing():
    from drn_amd import fuse_scores_reference, fused_rank_reference, fused_shortlist_reference
    #                 both    -inf in 1   overflow      none         nan in 0
    sc = torch.tensor([[[2.0, 3.0,        10.0,         NINF,        float("nan")]],
                       [[0.5, NINF,       1.0,          float("inf"), 4.0]]])
    w = [2.0, 0.25]
    drop, dc = fuse_scores_reference(sc, w, "drop")
    skip, kc = fuse_scores_reference(sc, w, "skip")
    assert dc.tolist() == [[True, False, True, False, False]]
    assert kc.tolist() == [[True, True, True, False, True]]
    assert skip[0].tolist() == [4.125, 6.0, 20.25, 0.0, 1.0] and float(drop[0, 0]) == 4.125 and float(drop[0, 2]) == 20.25
    # w = 0 beside -inf: 0 * -inf = NaN under drop (the video is missing), nothing under skip
    drop, dc = fuse_scores_reference(sc, [1.0, 0.0], "drop")
    skip, kc = fuse_scores_reference(sc, [1.0, 0.0], "skip")
    assert dc.tolist() == [[True, False, True, False, False]] and bool(torch.isnan(drop[0, 1]))
    assert kc.tolist() == [[True, True, True, False, True]] and skip[0].tolist() == [2.0, 3.0, 10.0, 0.0, 0.0]
    # an overflowing product: every term present, the fold not finite -> no candidate in either mode
    for mode in ("drop", "skip"):
        f, c = fuse_scores_reference(sc, [3e38, 1.0], mode)
        assert c[0, 2].item() is False and float(f[0, 2]) == float("inf")
    # the list and the rank follow the candidates
    got = fused_shortlist_reference(sc, w, 4, "skip")
    assert got.ids.tolist() == [[2, 1, 0, 4]] and got.scores.tolist() == [[20.25, 6.0, 4.125, 1.0]] and got.n.tolist() == [4]
    got = fused_shortlist_reference(sc, w, 4, "drop", allow=torch.tensor([True, True, False, True, True]))
    assert got.ids.tolist() == [[0, -1, -1, -1]] and got.n.tolist() == [1]
    r = fused_rank_reference(sc, w, [1], "skip")
    assert (r.rank.tolist(), r.score.tolist(), r.total.tolist()) == ([1], [6.0], [4])
    r = fused_rank_reference(sc, w, [1], "drop")
    assert (r.rank.tolist(), r.score.tolist(), r.total.tolist()) == ([-1], [0.0], [2])
    with pytest.raises(RuntimeError, match="drop.*skip"):
        fuse_scores_reference(sc, w, "mean")
    with pytest.raises(RuntimeError, match="2 numbers"):
        fuse_scores_reference(sc, [1.0], "drop")
    with pytest.raises(RuntimeError, match=r"\(M, S, V\) float32"):
        fuse_scores_reference(sc.double(), w)


def test_one_table_of_weight_one_is_the_matrix_itself():
    from drn_amd import fuse_scores_reference, fused_shortlist_reference
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 40, generator=g)
    x[0, 3], x[1, 7], x[2, 9], x[0, 11], x[1, 1] = NINF, float("nan"), float("inf"), -0.0, 0.0
    x[2, 20] = x[2, 4]                                                           # a tie: position 4 first
    for mode in ("drop", "skip"):
        fused, cand = fuse_scores_reference(x[None], [1.0], mode)
        assert torch.equal(cand, torch.isfinite(x))
        assert torch.equal(bits(fused)[cand], bits(x + 0.0)[cand]) and not np.signbit(float(fused[0, 11]))
    got = fused_shortlist_reference(x[None], None, 40)
    for s in range(3):
        order = sorted((v for v in range(40) if np.isfinite(float(x[s, v]))), key=lambda v: (-float(x[s, v]), v))
        assert got.ids[s, :len(order)].tolist() == order and int(got.n[s]) == len(order)
    assert got.ids[2].tolist().index(4) + 1 == got.ids[2].tolist().index(20)


# -- 2. scores_reference agrees with the shortlist references ------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
def test_scores_reference_is_the_matrix_the_shortlist_references_cut(masked):
    from drn_amd import late_shortlist_reference, scores_reference, segment_shortlist_reference, shortlist_reference
    V, E, S = 70, 8, 3
    emb, q = exact_host(V, E, S)
    q[1, 0] = float("nan")                                                       # a sentence that lists nothing
    shared, per = masks_of(V, S, 11)
    for allow in ((shared, per) if masked else (None,)):
        got = scores_reference(emb, q, allow=allow)
        want = dense_of(shortlist_reference(emb, q, V, allow=allow), V)
        assert got.dtype == torch.float32 and torch.equal(bits(got), bits(want))
        assert bool((got[1] == NINF).all()) and not bool(torch.isnan(got).any())
    off = ragged_offsets(V)
    Vr = len(off) - 1
    shared, per = masks_of(Vr, S, 12)
    empty = torch.from_numpy(np.diff(off) == 0)
    for allow in ((shared, per) if masked else (None,)):
        got = scores_reference(emb, q, offsets=off, allow=allow)
        want = dense_of(segment_shortlist_reference(emb, off, q, Vr, allow=allow), Vr)
        assert torch.equal(bits(got), bits(want)) and bool((got[:, empty] == NINF).all())
        g = torch.Generator().manual_seed(13)
        tok = torch.randint(-4, 5, (S, 5, E), generator=g).float()
        lengths = torch.tensor([5, 0, 2], dtype=torch.int32)
        tok[2, 3] = float("nan")                                                 # (a dead token: ignored)
        got = scores_reference(emb, tok, offsets=off, lengths=lengths, allow=allow)
        want = dense_of(late_shortlist_reference(emb, off, tok, lengths, Vr, allow=allow), Vr)
        assert torch.equal(bits(got), bits(want)) and bool((got[1] == NINF).all())
        if allow is None:
            assert bool(torch.isfinite(got[2, ~empty]).all()) and bool(torch.isfinite(got[0, ~empty]).all())
    with pytest.raises(RuntimeError, match="need offsets"):
        scores_reference(emb, q[:, None, :], lengths=torch.ones(S, dtype=torch.int32))


def test_a_fused_list_of_one_exact_table_is_its_shortlist():
    from drn_amd import fused_rank_reference, fused_shortlist_reference, rank_reference, scores_reference, shortlist_reference
    emb, q = exact_host(300, 8, 3)
    sc = scores_reference(emb, q)
    for n in (1, 128, 300):
        same(fused_shortlist_reference(sc[None], None, n), shortlist_reference(emb, q, n), n)
    t = [0, 299, 300]
    same(fused_rank_reference(sc[None], None, t), rank_reference(emb, q, t))


# -- 3. refusals, before the library is reached ------------------------------------------------------------------------------------------------

def host_tables():
    """A plain bf16 table (E = 32), a ragged fp32 one (E = 8) and an FP8 ragged one (E = 64) over the same 3 named videos: host tensors
    that say they are resident."""
    from drn_amd import Shortlister
    names = ["a", "b", "c"]
    plain = Shortlister(resident(torch.zeros(3, 32, dtype=torch.bfloat16)), names=names)
    ragged = Shortlister(resident(torch.zeros(6, 8)), offsets=[0, 2, 2, 6])
    q8 = Shortlister.from_mx8(resident(torch.zeros(6, 64, dtype=torch.uint8)), resident(torch.full((6, 2), 127, dtype=torch.uint8)),
                              torch.bfloat16, names=names, offsets=[0, 2, 2, 6])
    return plain, ragged, q8


def test_scores_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import ShardedShortlister, _lib
    _no_library(monkeypatch)
    plain, ragged, q8 = host_tables()
    q = resident(torch.zeros(2, 32, dtype=torch.bfloat16))
    err = _lib.DrnError
    with pytest.raises(err, match="on the table's device"):
        plain.scores(torch.zeros(2, 32, dtype=torch.bfloat16))                   # host queries
    with pytest.raises(err, match=r"must be \(S, 32\)"):
        plain.scores(resident(torch.zeros(2, 8, dtype=torch.bfloat16)))
    with pytest.raises(err, match="the queries are torch.float32, the table is torch.bfloat16"):
        plain.scores(resident(torch.zeros(2, 32)))
    with pytest.raises(err, match="must be a tensor"):
        plain.scores([[0.0] * 32])
    for bad in (torch.zeros(2, 3), resident(torch.zeros(2, 3, dtype=torch.float64)), resident(torch.zeros(3, 2)), resident(torch.zeros(6))):
        with pytest.raises(err, match=r"out must be a \(2, 3\) torch.float32 tensor on the table's device"):
            plain.scores(q, out=bad)
    for bad in (resident(torch.zeros(3, 2)).t(), resident(torch.zeros(2, 6))[:, ::2], resident(torch.zeros(4, 3))[::2].as_strided((2, 3), (2, 1))):
        with pytest.raises(err, match="last stride 1 and row stride >= 3"):
            plain.scores(q, out=bad)
    with pytest.raises(err, match="bool tensor; pack it first"):
        plain.scores(q, allow=resident(torch.ones(3, dtype=torch.bool)))
    with pytest.raises(err, match=r"allow must be \(1,\)"):
        plain.scores(q, allow=resident(torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(err, match="one row per video"):
        plain.scores_late(resident(torch.zeros(2, 4, 32, dtype=torch.bfloat16)), resident(torch.zeros(2, dtype=torch.int32)))
    tok, lengths = resident(torch.zeros(2, 4, 8)), resident(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(err, match=r"must be \(S, L, 8\)"):
        ragged.scores_late(resident(torch.zeros(2, 8)), lengths)
    with pytest.raises(err, match=r"L = 65 tokens outside \[1, 64\]"):
        ragged.scores_late(resident(torch.zeros(2, 65, 8)), lengths)
    with pytest.raises(err, match="lengths must be a contiguous"):
        ragged.scores_late(tok, resident(torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(err, match="lengths must be on the table's device"):
        ragged.scores_late(tok, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(err, match="must be contiguous"):
        ragged.scores_late(resident(torch.zeros(2, 8, 8))[:, ::2], lengths)
    with pytest.raises(err, match="the queries are torch.float32, the table is torch.bfloat16"):
        q8.scores(resident(torch.zeros(2, 64)))
    corpus = ShardedShortlister([plain, host_tables()[0]])
    with pytest.raises(err, match=r"out must be a \(2, 6\)"):
        corpus.scores(q, out=resident(torch.zeros(2, 3)))
    with pytest.raises(err, match="these tables have one row per video"):
        corpus.scores_late(resident(torch.zeros(2, 4, 32, dtype=torch.bfloat16)), resident(torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(err, match=r"allow must be \(1,\)"):
        corpus.scores(q, allow=resident(torch.zeros(3, dtype=torch.int32)))


def test_shortlist_scores_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, shortlist_scores
    _no_library(monkeypatch)
    err = _lib.DrnError
    good = resident(torch.zeros(2, 40))
    with pytest.raises(err, match="on the GPU"):
        shortlist_scores(torch.zeros(2, 40), 5)
    with pytest.raises(err, match="on the GPU"):
        shortlist_scores([[0.0]], 1)
    for bad in (resident(torch.zeros(2, 40, dtype=torch.float64)), resident(torch.zeros(2, 40, dtype=torch.bfloat16)), resident(torch.zeros(40)),
                resident(torch.zeros(1, 2, 40)), resident(torch.zeros(0, 40))):
        with pytest.raises(err, match=r"\(S, V\) torch.float32"):
            shortlist_scores(bad, 5)
    for bad in (resident(torch.zeros(40, 2)).t(), resident(torch.zeros(2, 80))[:, ::2]):
        with pytest.raises(err, match="last stride 1 and row stride >= 40"):
            shortlist_scores(bad, 5)
    for n in (0, -1, 1025):
        with pytest.raises(err, match=r"n = %d outside \[1, 1024\]" % n):
            shortlist_scores(good, n)
    with pytest.raises(err, match="bool tensor; pack it first"):
        shortlist_scores(good, 5, allow=resident(torch.ones(40, dtype=torch.bool)))
    with pytest.raises(err, match="three buffers of a Shortlist"):
        shortlist_scores(good, 5, out=(resident(torch.zeros(2, 5, dtype=torch.int32)),))
    with pytest.raises(err, match=r"out.scores must be a contiguous \(2, 5\)"):
        shortlist_scores(good, 5, out=(resident(torch.zeros(2, 5, dtype=torch.int32)), resident(torch.zeros(2, 6)),
                                       resident(torch.zeros(2, dtype=torch.int32))))


def test_the_fused_shortlister_refuses_bad_arguments_before_the_library_is_reached(monkeypatch):
    from drn_amd import FUSE_MAX_TABLES, FusedShortlister, ShardedShortlister, Shortlister, _lib
    _no_library(monkeypatch)
    err = _lib.DrnError
    plain, ragged, q8 = host_tables()
    assert FUSE_MAX_TABLES == 8
    with pytest.raises(err, match=r"0 tables outside \[1, 8\]"):
        FusedShortlister([])
    with pytest.raises(err, match=r"9 tables outside \[1, 8\]"):
        FusedShortlister([plain] * 9)
    with pytest.raises(err, match="must be a sequence"):
        FusedShortlister(plain)
    with pytest.raises(err, match="table 1 must be a Shortlister or a ShardedShortlister, not Tensor"):
        FusedShortlister([plain, torch.zeros(3, 32)])
    with pytest.raises(err, match="table 1 holds 4 videos, table 0 holds 3"):
        FusedShortlister([plain, Shortlister(resident(torch.zeros(4, 32)))])
    with pytest.raises(err, match="names of table 1 are not those"):
        FusedShortlister([plain, Shortlister(resident(torch.zeros(3, 32)), names=["a", "c", "b"])])
    for bad in ("mean", None, 0):
        with pytest.raises(err, match="missing must be"):
            FusedShortlister([plain], missing=bad)
    with pytest.raises(err, match="3 weights for 2 tables"):
        FusedShortlister([plain, ragged], weights=[1.0, 2.0, 3.0])
    with pytest.raises(err, match="weights must be None, 2 numbers"):
        FusedShortlister([plain, ragged], weights=["a", "b"])
    for bad in (resident(torch.ones(2, dtype=torch.float64)), resident(torch.ones(3)), resident(torch.ones(4))[::2]):
        with pytest.raises(err, match=r"contiguous \(2,\) torch.float32"):
            FusedShortlister([plain, ragged], weights=bad)
    fused = FusedShortlister([plain, ragged, q8, ShardedShortlister([plain])], weights=[1.0, -0.5, 0.0, 0.125], missing="skip")
    assert len(fused) == 3 and fused.names == ["a", "b", "c"] and fused.device == plain.device and fused.missing == "skip"
    assert fused.weights.tolist() == [1.0, -0.5, 0.0, 0.125] and fused.weights.dtype == torch.float32
    kept = resident(torch.ones(1))
    assert FusedShortlister([ragged], weights=kept).weights is kept and FusedShortlister([ragged]).names is None
    qp, qr = resident(torch.zeros(2, 32, dtype=torch.bfloat16)), resident(torch.zeros(2, 8))
    late = (resident(torch.zeros(2, 4, 64, dtype=torch.bfloat16)), resident(torch.zeros(2, dtype=torch.int32)))
    items = [qp, qr, late, qp]
    targets = resident(torch.zeros(2, dtype=torch.int32))
    for call in (lambda x: fused.shortlist(x, 5), lambda x: fused.rank(x, targets)):
        with pytest.raises(err, match="a sequence of 4 items"):
            call(qp)
        with pytest.raises(err, match="a sequence of 4 items"):
            call(items[:3])
        with pytest.raises(err, match=r"table 1\): the queries are torch.bfloat16, the table is torch.float32"):
            call([qp, resident(torch.zeros(2, 8, dtype=torch.bfloat16)), late, qp])
        with pytest.raises(err, match=r"table 0\): the queries must be on the table's device"):
            call([torch.zeros(2, 32, dtype=torch.bfloat16), qr, late, qp])
        with pytest.raises(err, match="item 1 holds 3 sentences, item 0 holds 2"):
            call([qp, resident(torch.zeros(3, 8)), late, qp])
        with pytest.raises(err, match=r"table 0\).*one row per video"):
            call([(resident(torch.zeros(2, 4, 32, dtype=torch.bfloat16)), late[1]), qr, late, qp])
        with pytest.raises(err, match="item 2 must be a queries tensor or a pair"):
            call([qp, qr, (late[0], late[1], late[1]), qp])
        with pytest.raises(err, match="lengths of item 2"):
            call([qp, qr, (late[0], [4, 4]), qp])
    for n in (0, 1025):
        with pytest.raises(err, match=r"n = %d outside \[1, 1024\]" % n):
            fused.shortlist(items, n)
    with pytest.raises(err, match="bool tensor; pack it first"):
        fused.shortlist(items, 5, allow=resident(torch.ones(3, dtype=torch.bool)))
    with pytest.raises(err, match="three buffers of a Shortlist"):
        fused.shortlist(items, 5, out=(targets, targets))
    with pytest.raises(err, match="targets must be a contiguous"):
        fused.rank(items, resident(torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(err, match="targets must be on the table's device"):
        fused.rank(items, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(err, match=r"allow must be \(1,\)"):
        fused.rank(items, targets, allow=resident(torch.zeros(2, dtype=torch.int32)))
    # the wrappers under them refuse what the classes cannot meet
    from drn_amd import ops
    with pytest.raises(err, match="missing must be one of"):
        ops.shortlist_fuse_topn(resident(torch.zeros(1, 2, 3)), kept, "mean", 1, None, None, None, None)
    with pytest.raises(err, match=r"1 <= M <= 8"):
        ops.shortlist_fuse_rank(resident(torch.zeros(9, 2, 3)), kept, "drop", targets, None, None, None)
    with pytest.raises(err, match="matrices that do not overlap"):
        ops.shortlist_fuse_rank(resident(torch.zeros(2, 3)).expand(2, 2, 3), resident(torch.ones(2)), "drop", targets, None, None, None)


# -- 4. the C boundary -------------------------------------------------------------------------------------------------------------------------

ENTRIES = (("drn_shortlist_scores", 18), ("drn_shortlist_fuse_topn", 17), ("drn_shortlist_fuse_rank", 15))


def test_library_exports_the_three_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    for name, count in ENTRIES:
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("long long ") else ctypes.c_int
            assert t is want, (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig) and callable(getattr(ops, name[4:]))
    hdr = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define DRN_FUSE_MAX_TABLES\s+(\d+)", hdr).group(1)) == _lib.FUSE_MAX_TABLES == drn_amd.FUSE_MAX_TABLES == 8
    assert int(re.search(r"#define DRN_FUSE_DROP\s+(\d+)", hdr).group(1)) == _lib.FUSE_MODES["drop"] == 0
    assert int(re.search(r"#define DRN_FUSE_SKIP\s+(\d+)", hdr).group(1)) == _lib.FUSE_MODES["skip"] == 1
    for public in ("FusedShortlister", "shortlist_scores", "scores_reference", "fuse_scores_reference", "fused_shortlist_reference",
                   "fused_rank_reference"):
        assert hasattr(drn_amd, public), public
    for cls in (drn_amd.Shortlister, drn_amd.ShardedShortlister):
        assert callable(cls.scores) and callable(cls.scores_late)
    assert not hasattr(drn_amd.FusedShortlister, "rerank")


def test_the_entries_check_their_arguments_before_anything_is_launched():
    """Every call below is refused by the entry's own checks: nothing is launched, so no GPU is needed.  The pointers are host buffers
    that only have to be non-null and aligned."""
    from drn_amd import _lib
    lib = built_lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    last = lambda: lib.drn_last_error().decode()
    # drn_shortlist_scores(table, scales, queries, lengths, offsets, blk_vid, allow, allow_stride, R, V, nblocks, E, S, L, dtype, out, ld_out, stream)
    scores = lambda *a: lib.drn_shortlist_scores(*a)
    assert scores(None, None, p, None, None, None, None, 0, 0, 8, 0, 8, 1, 1, 0, p, 8, None) == -1 and "null pointer" in last()
    assert scores(p, None, p, None, p, None, None, 0, 8, 8, 1, 8, 1, 1, 0, p, 8, None) == -1 and "given together" in last()
    assert scores(p, None, p, p, None, None, None, 0, 0, 8, 0, 8, 1, 1, 0, p, 8, None) == -1 and "need a ragged table" in last()
    assert scores(p, None, p, None, None, None, None, 0, 0, 8, 0, 8, 1, 2, 0, p, 8, None) == -1 and "L must be 1" in last()
    assert scores(p, None, p, p, p, p, None, 0, 8, 8, 1, 8, 1, 65, 0, p, 8, None) == -1 and "tokens outside [1, 64]" in last()
    assert scores(p, None, p, None, None, None, None, 0, 0, 8, 0, 8, 1, 1, 0, p, 7, None) == -1 and "ld_out = 7 below V = 8" in last()
    assert scores(p, p, p, None, None, None, None, 0, 0, 8, 0, 40, 1, 1, 0, p, 8, None) == -1 and "multiple of the block" in last()
    assert scores(p, None, p, None, None, None, None, 0, 0, 8, 0, 8, 1, 1, 2, p, 8, None) == -1 and "dtype 2" in last()
    assert scores(p, None, p, None, p, p, None, 0, 8, 600, 2, 8, 1, 1, 0, p, 600, None) == -1 and "blocks outside" in last()
    assert scores(p, None, p, None, None, None, p, 3, 0, 8, 0, 8, 1, 1, 0, p, 8, None) == -1 and "allow_stride = 3" in last()
    # drn_shortlist_fuse_topn(scores, stride_m, ld, weights, M, mode, allow, allow_stride, V, S, n, ws, ws_keys, ids, out_scores, counts, stream)
    topn = lambda *a: lib.drn_shortlist_fuse_topn(*a)
    assert topn(p, 16, 8, p, 0, 0, None, 0, 8, 2, 1, p, 64, p, p, p, None) == -1 and "M = 0 tables outside [1, 8]" in last()
    assert topn(p, 16, 8, p, 9, 0, None, 0, 8, 2, 1, p, 64, p, p, p, None) == -1 and "M = 9 tables outside [1, 8]" in last()
    assert topn(p, 16, 8, p, 2, 2, None, 0, 8, 2, 1, p, 64, p, p, p, None) == -1 and "mode = 2" in last()
    assert topn(p, 16, 7, p, 2, 0, None, 0, 8, 2, 1, p, 64, p, p, p, None) == -1 and "ld = 7 below V = 8" in last()
    assert topn(p, 15, 8, p, 2, 0, None, 0, 8, 2, 1, p, 64, p, p, p, None) == -1 and "stride_m = 15 below" in last()
    assert topn(p, 16, 8, p, 2, 0, None, 0, 8, 2, 0, p, 64, p, p, p, None) == -1 and "n = 0 outside [1, 1024]" in last()
    assert topn(p, 16, 8, p, 2, 0, None, 0, 8, 2, 1025, p, 64, p, p, p, None) == -1 and "n = 1025 outside [1, 1024]" in last()
    assert topn(p, 16, 8, p, 2, 0, None, 0, 8, 2, 4, p, 7, p, p, p, None) == -1 and "the workspace holds 7 keys, 8 are needed" in last()
    assert topn(p, 16, 8, None, 2, 0, None, 0, 8, 2, 4, p, 8, p, p, p, None) == -1 and "null pointer" in last()
    # drn_shortlist_fuse_rank(scores, stride_m, ld, weights, M, mode, targets, allow, allow_stride, V, S, rank, score, total, stream)
    rank = lambda *a: lib.drn_shortlist_fuse_rank(*a)
    assert rank(p, 16, 8, p, 2, 0, None, None, 0, 8, 2, p, p, p, None) == -1 and "null pointer" in last()
    assert rank(p, 16, 8, p, 2, 0, p, p, 2, 8, 2, p, p, p, None) == -1 and "allow_stride = 2" in last()
    assert rank(p, 0, 8, p, 1, 0, p, None, 0, 8, 70000, p, p, p, None) == -1 and "more than 65535 sentences" in last()


def test_the_new_kernels_do_not_spill(tmp_path):
    """Every kernel of csrc/retrieve_fuse.hip, from the notes of the built code object: no spilled register, no scratch."""
    table = kernel_table(tmp_path)
    mine = {k: r for k, r in table.items() if re.search(r"scores_block_kernel|scores_segments_kernel|scores_late_kernel|fuse_block_kernel|"
                                                         r"fuse_rank_kernel", k)}
    assert len(mine) == 4 + 4 + 4 + 1 + 1, sorted(mine)          # three score kernels x (bf16, fp32) x (plain, FP8), and the two fuse kernels
    # (the ragged kernels hold 51 KB of LDS: three workgroups of four waves a CU, three waves a SIMD, 512 / 3 = 170 registers a lane)
    for k, r in mine.items():
        assert r["spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 168, (k, r)
