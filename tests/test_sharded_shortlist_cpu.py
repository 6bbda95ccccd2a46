"""Sharded shortlist tables, the host side: merge_shortlists_reference of per-part references EQUALS the reference on the whole table
(plain, masked, ragged, late), slice_allow_reference against pack_allow_reference, every refusal of ShardedShortlister that needs no GPU,
the mirrored constants, the two C entries drn_shortlist_merge_lists and drn_allow_slices at ABI 9 with their argument checks, and the
compiler's notes on their kernels.
tests/test_sharded_shortlist_gpu.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib
from test_late_shortlist_cpu import Resident, _no_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE, SLICES = "drn_shortlist_merge_lists", "drn_allow_slices"
V = 775
CUTS = ([0, 1, V], [0, 64, V], [0, 321, V], [0, 1, 64, 321, V])


def same(got, want, what):
    assert type(got) is type(want), what
    for f in want._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


# -- merge equals whole, on the references ---------------------------------------------------------------------------------------------------

def plain_case():
    g = torch.Generator().manual_seed(3)
    emb = torch.randint(-4, 5, (V, 8), generator=g).float()
    for a, b in ((1, 0), (63, 64), (320, 321), (321, 0), (774, 5), (400, 64)):      # equal scores across every cut
        emb[a] = emb[b]
    q = torch.randint(-4, 5, (5, 8), generator=g).float()
    q[3] = float("nan")                                                       # a sentence that lists nothing
    mask = torch.rand((5, V), generator=g) < 0.5
    mask[2, :64] = False                                                      # a part wholly masked for one sentence
    return emb, q, mask


def test_merging_the_parts_of_a_plain_table_is_the_whole_table():
    from drn_amd import Shortlist, merge_shortlists_reference, shortlist_reference
    emb, q, mask = plain_case()
    for bases in CUTS:
        for n in (1, 5, 128):
            for allow in (None, mask):
                want = shortlist_reference(emb, q, n, allow=allow)
                parts = [shortlist_reference(emb[a:b], q, n, allow=None if allow is None else allow[:, a:b]) for a, b in zip(bases[:-1], bases[1:])]
                got = merge_shortlists_reference(parts, bases, n)
                assert isinstance(got, Shortlist) and got.ids.dtype == got.n.dtype == torch.int32 and got.scores.dtype == torch.float32
                same(got, want, (bases, n, allow is not None))
                assert int(got.n[3]) == 0 and int(got.n[0]) == min(n, V if allow is None else int(mask[0].sum()))
    # equal scores on either side of a cut are in the data (videos 320 | 321 are twins, 0 | 1 | 321 triplets): the lists above hold ties
    whole = shortlist_reference(emb, q, 128)
    assert bool(((whole.scores[:, 1:] == whole.scores[:, :-1]) & (whole.ids[:, 1:] > whole.ids[:, :-1]) & (whole.ids[:, 1:] >= 0)).any())
    # a wider input than the cut, and lists of different widths
    parts = [shortlist_reference(emb[:321], q, 128), shortlist_reference(emb[321:], q, 7)]
    same(merge_shortlists_reference(parts, [0, 321, V], 5), shortlist_reference(emb, q, 5), "128 and 7 -> 5")


def test_the_merge_reference_drops_what_is_no_candidate_and_pads():
    from drn_amd import Shortlist, SegmentShortlist, _lib, merge_shortlists_reference
    nan, big = float("nan"), 2 ** 31 - 1
    a = Shortlist(torch.tensor([[2, 0, 3, big]], dtype=torch.int32), torch.tensor([[5., 4., 9., 9.]]), torch.tensor([2], dtype=torch.int32))
    b = Shortlist(torch.tensor([[1, 0, -2 ** 31, 1]], dtype=torch.int32), torch.tensor([[5., nan, 8., float("inf")]]), torch.tensor([9], dtype=torch.int32))
    got = merge_shortlists_reference([a, b], [0, 3, 5], 6)
    # a: entries 0, 1 (count 2); b: count 9 is clamped to the width; its NaN, its INT_MIN id and its infinite score are no candidates
    assert got.ids.tolist() == [[2, 4, 0, -1, -1, -1]] and got.scores.tolist() == [[5., 5., 4., 0., 0., 0.]] and got.n.tolist() == [3]
    assert merge_shortlists_reference([a, b], [0, 3, 5], 1).ids.tolist() == [[2]]                 # the tie: position 2 before 3 + 1
    assert merge_shortlists_reference([a, b], [0, 2, 4], 6).ids.tolist() == [[3, 0, -1, -1, -1, -1]]  # id 2 is outside a shard of 2 videos
    ra = SegmentShortlist(*a, torch.tensor([[7, 8, 9, 9]], dtype=torch.int32))
    rb = SegmentShortlist(*b, torch.tensor([[6, 5, 4, 3]], dtype=torch.int32))
    seg = merge_shortlists_reference([ra, rb], [0, 3, 5], 4)
    assert isinstance(seg, SegmentShortlist) and seg.rows.tolist() == [[7, 6, 8, -1]] and seg.ids.tolist() == [[2, 4, 0, -1]]
    with pytest.raises(_lib.DrnError, match="2 lists need 3 bases"):
        merge_shortlists_reference([a, b], [0, 3], 2)
    with pytest.raises(_lib.DrnError, match="all be Shortlists or all be SegmentShortlists"):
        merge_shortlists_reference([a, rb], [0, 3, 5], 2)


def test_merging_the_parts_of_a_ragged_table_is_the_whole_table():
    from drn_amd import SegmentShortlist, late_shortlist_reference, merge_shortlists_reference, segment_shortlist_reference
    lens = [1, 3, 0, 17] * 20                                                 # V = 80; video 2 owns no row: the cut at 3 lies next to it
    off = np.concatenate([[0], np.cumsum(lens)])
    g = torch.Generator().manual_seed(5)
    emb = torch.randint(-4, 5, (int(off[-1]), 8), generator=g).float()
    emb[off[70]], emb[off[3]] = emb[off[0]], emb[off[1]]                     # equal scores across the cuts
    tok = torch.randint(-4, 5, (4, 3, 8), generator=g).float()
    tok[2, 0, 1] = float("nan")
    lengths = [3, 1, 2, 0]
    mask = torch.rand((4, 80), generator=g) < 0.6
    bases = [0, 3, 70, 80]
    part = lambda a, b: (emb[off[a]:off[b]], off[a:b + 1] - off[a])
    for n in (1, 5, 128):
        for allow in (None, mask):
            cut = lambda a, b: None if allow is None else allow[:, a:b]
            want = segment_shortlist_reference(emb, off, tok[:, 0], n, allow=allow)
            got = merge_shortlists_reference([segment_shortlist_reference(*part(a, b), tok[:, 0], n, allow=cut(a, b))
                                              for a, b in zip(bases[:-1], bases[1:])], bases, n)
            assert isinstance(got, SegmentShortlist)
            same(got, want, ("segments", n, allow is not None))
            assert int(got.n[2]) == 0 and int(got.n[0]) > 0
            want = late_shortlist_reference(emb, off, tok, lengths, n, allow=allow)
            got = merge_shortlists_reference([late_shortlist_reference(*part(a, b), tok, lengths, n, allow=cut(a, b))
                                              for a, b in zip(bases[:-1], bases[1:])], bases, n)
            same(got, want, ("late", n, allow is not None))
            assert got.n.tolist()[2:] == [0, 0] and int(got.n[1]) > 0


def test_slice_allow_reference_is_pack_allow_reference_of_the_bits():
    from drn_amd import _lib, pack_allow_reference, slice_allow_reference
    g = torch.Generator().manual_seed(9)
    for shape in ((V,), (3, V)):
        mask = (torch.rand(shape, generator=g) < 0.5).numpy()
        words = pack_allow_reference(mask)
        stuffed = words.copy()
        stuffed[..., -1] |= np.int32(-1) << np.int32(V % 32)                  # bits at or past V: never part of a slice
        for bases in CUTS + ([0, 32, 64, 320, V],):
            for a, b in zip(bases[:-1], bases[1:]):
                want = pack_allow_reference(mask[..., a:b])
                for w in (words, stuffed, torch.from_numpy(words)):
                    got = slice_allow_reference(w, V, a, b)
                    assert got.dtype == np.int32 and got.shape == shape[:-1] + (-(-(b - a) // 32),) and np.array_equal(got, want), (shape, a, b)
    one = slice_allow_reference(np.array([-1], dtype=np.int32), 32, 31, 32)
    assert one.tolist() == [1]
    for bad in ((words, V, 5, 5), (words, V, -1, 4), (words, V, 0, V + 1), (words[:, :-1], V, 0, 4), (words.astype(np.int64), V, 0, 4)):
        with pytest.raises(_lib.DrnError, match="slice_allow_reference"):
            slice_allow_reference(*bad)


# -- refusals, before the library is reached ---------------------------------------------------------------------------------------------------

def _stand_in(videos=3, ragged=False, quantize=None, E=32, dtype=torch.bfloat16, names=True, resident=True):
    """A shard that only stands in for a resident one (the constructor was not run): `videos` videos, two rows each when ragged."""
    from drn_amd import Shortlister
    sl = Shortlister.__new__(Shortlister)
    sl.names, sl._ws, sl._seg = (["v%d" % v for v in range(videos)] if names else None), {}, None
    rows = 2 * videos if ragged else videos
    if ragged:
        sl._seg = (torch.arange(0, rows + 1, 2, dtype=torch.int32), torch.tensor([0, videos], dtype=torch.int32), torch.zeros(videos, dtype=torch.int32))
    put = (lambda t: t.as_subclass(Resident)) if resident else (lambda t: t)
    if quantize is None:
        sl.embeddings = put(torch.zeros(rows, E, dtype=dtype))
    else:
        sl.embeddings, sl.quantize, sl._dtype = None, quantize, dtype
        sl.codes, sl.scales = put(torch.zeros(rows, E, dtype=torch.uint8)), put(torch.zeros(rows, E // 32, dtype=torch.uint8))
    return sl


def test_the_constructor_and_append_refuse_before_the_library_is_reached(monkeypatch):
    import drn_amd
    from drn_amd import ShardedShortlister, _lib
    _no_library(monkeypatch)
    assert _lib.SHARDS_MAX == drn_amd.SHARDS_MAX == 64
    for bad in ([], [_stand_in()] * 65):
        with pytest.raises(_lib.DrnError, match=r"%d shards outside \[1, 64\]" % len(bad)):
            ShardedShortlister(bad)
    with pytest.raises(_lib.DrnError, match="must be a sequence of Shortlister objects"):
        ShardedShortlister(5)
    with pytest.raises(_lib.DrnError, match="a shard must be a Shortlister, not Tensor"):
        ShardedShortlister([_stand_in(), torch.zeros(3, 32)])
    clashes = ((dict(E=64), "shard 1 has E = 64 columns, the others 32"), (dict(dtype=torch.float32), "shard 1 takes torch.float32 queries, the others torch.bfloat16"),
               (dict(ragged=True), "shard 1 is ragged, the others are not"), (dict(quantize="mxfp8", dtype=torch.float32), "takes torch.float32 queries"))
    for kw, match in clashes:
        with pytest.raises(_lib.DrnError, match=match):
            ShardedShortlister([_stand_in(), _stand_in(**kw)])
        sh = ShardedShortlister([_stand_in()])
        with pytest.raises(_lib.DrnError, match=match):
            sh.append(_stand_in(**kw))
        assert len(sh.shards) == 1 and sh.bases == [0, 3] and len(sh) == 3     # a refused shard changes nothing
    with pytest.raises(_lib.DrnError, match="shard 1 is plain, the others are not"):
        ShardedShortlister([_stand_in(ragged=True), _stand_in()])
    other = _stand_in()
    other.embeddings = torch.zeros(3, 32, dtype=torch.bfloat16, device="meta")
    with pytest.raises(_lib.DrnError, match="shard 1 is on meta, the others on cpu"):
        ShardedShortlister([_stand_in(), other])
    # the corpus stays below 2^31 videos
    huge = _stand_in()
    huge.embeddings = torch.zeros(2 ** 31 - 3, 32, dtype=torch.bfloat16, device="meta")
    tiny = _stand_in()
    tiny.embeddings = torch.zeros(3, 32, dtype=torch.bfloat16, device="meta")
    sh = ShardedShortlister.__new__(ShardedShortlister)
    sh.shards, sh.bases, sh.names = [], [0], []
    sh._admit(huge)
    with pytest.raises(_lib.DrnError, match=r"2147483648 videos with shard 1, outside \[1, 2\^31\)"):
        sh._admit(tiny)
    # the 65th shard
    sh = ShardedShortlister([_stand_in(1) for _ in range(64)])
    assert len(sh) == 64 and sh.bases == list(range(65))
    with pytest.raises(_lib.DrnError, match=r"65 shards outside \[1, 64\]"):
        sh.append(_stand_in(1))


def test_the_attributes_of_a_sharded_table():
    from drn_amd import ShardedShortlister, _lib
    a, b, c = _stand_in(3), _stand_in(1, quantize="mxfp8"), _stand_in(70)
    b.names, c.names = ["x"], ["w%d" % v for v in range(70)]
    sh = ShardedShortlister((a, b))
    assert sh.shards == [a, b] and sh.shards[0] is a and sh.bases == [0, 3, 4] and len(sh) == 4 and sh.E == 32 and sh.dtype == torch.bfloat16
    assert sh.bases_device.dtype == torch.int32 and sh.bases_device.tolist() == [0, 3, 4]
    assert sh.nbytes == 3 * 32 * 2 + (32 + 1) and sh.names == ["v0", "v1", "v2", "x"]
    sh._bufs["stale"] = 1
    assert sh.append(c) is sh and sh._bufs == {} and sh.bases == [0, 3, 4, 74] and sh.bases_device.tolist() == [0, 3, 4, 74] and len(sh.names) == 74
    store = lambda names: type("Store", (), {"names": names})()
    sh.check(store(a.names + b.names + c.names))
    with pytest.raises(_lib.DrnError, match="names are not the store's"):
        sh.check(store(a.names + c.names + b.names))
    # allow_of over the corpus: names and corpus positions
    words = sh.allow_of(keep=["x", 0, 73, "w0"])
    assert words.dtype == torch.int32 and words.shape == (3,) and words.tolist() == [0b11001, 0, 1 << (73 - 64)]
    assert sh.allow_of(drop=[2]).tolist() == [-1 & ~4, -1, (1 << 10) - 1]
    for kw, match in ((dict(), "exactly one of keep= and drop="), (dict(keep=[74]), r"position 74 outside \[0, 74\)"), (dict(drop=["nobody"]), "no video named 'nobody'"),
                      (dict(keep=[1.5]), "an entry must be a name or a position")):
        with pytest.raises(_lib.DrnError, match="ShardedShortlister.allow_of: " + match):
            sh.allow_of(**kw)
    # names are the concatenation only when every shard has them
    assert ShardedShortlister([a, _stand_in(names=False)]).names is None
    nameless = ShardedShortlister([_stand_in(names=False)])
    nameless.append(a)
    assert nameless.names is None
    with pytest.raises(_lib.DrnError, match="names are not the store's"):
        nameless.check(store(a.names))
    with pytest.raises(_lib.DrnError, match="is a name and this table has no names"):
        nameless.allow_of(keep=["v0"])


def test_shortlist_and_shortlist_late_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import ShardedShortlister, _lib
    _no_library(monkeypatch)
    res = lambda t: t.as_subclass(Resident)
    q = res(torch.zeros(2, 32, dtype=torch.bfloat16))
    for ragged in (False, True):
        sh = ShardedShortlister([_stand_in(3, ragged), _stand_in(70, ragged, quantize="mxfp8")])       # V = 73: W = 3
        with pytest.raises(_lib.DrnError, match="queries must be a tensor"):
            sh.shortlist([[0.0] * 32], 2)
        with pytest.raises(_lib.DrnError, match=r"must be \(S, 32\)"):
            sh.shortlist(res(torch.zeros(2, 16, dtype=torch.bfloat16)), 2)
        with pytest.raises(_lib.DrnError, match="the table is torch.bfloat16"):
            sh.shortlist(res(torch.zeros(2, 32)), 2)
        with pytest.raises(_lib.DrnError, match="on the GPU"):
            sh.shortlist(torch.zeros(2, 32, dtype=torch.bfloat16), 2)
        for n in (0, -1, 129):
            with pytest.raises(_lib.DrnError, match=r"n = %d outside \[1, 128\]" % n):
                sh.shortlist(q, n)
        good = lambda: [res(torch.zeros((2, 4), dtype=torch.int32)), res(torch.zeros((2, 4))), res(torch.zeros((2,), dtype=torch.int32))] \
            + ([res(torch.zeros((2, 4), dtype=torch.int32))] if ragged else [])
        for i, field in enumerate(("ids", "scores", "n", "rows")[:len(good())]):
            for wrong in (res(torch.zeros((2, 5), dtype=torch.int32)), torch.zeros(good()[i].shape, dtype=good()[i].dtype), None):
                out = good()
                out[i] = wrong
                with pytest.raises(_lib.DrnError, match="out.%s must be a contiguous" % field):
                    sh.shortlist(q, 4, out=out)
        if ragged:
            with pytest.raises(_lib.DrnError, match="four buffers of a SegmentShortlist"):
                sh.shortlist(q, 4, out=good()[:3])
        # allow: the packed mask over the WHOLE corpus
        for bad, match in ((torch.ones(73, dtype=torch.bool), "pack it first"), (res(torch.zeros(3, dtype=torch.int64)), "torch.int32 packed words"),
                           ([1], "packed mask"), (torch.zeros(3, dtype=torch.int32), "on the table's device"),
                           (res(torch.zeros(1, dtype=torch.int32)), r"must be \(3,\) -- one mask for all sentences -- or \(2, 3\).*V = 73"),
                           (res(torch.zeros(2, 6, dtype=torch.int32))[:, ::2], "must be contiguous")):
            with pytest.raises(_lib.DrnError, match=match):
                sh.shortlist(q, 2, allow=bad)
    # shortlist_late: ragged shards only, then shortlist_late's own refusals
    tok, lengths = res(torch.zeros(2, 3, 32, dtype=torch.bfloat16)), res(torch.tensor([3, 1], dtype=torch.int32))
    with pytest.raises(_lib.DrnError, match=r"shortlist_late: these tables have one row per video.*\(sum_t q_t\) \. emb_v.*call shortlist\(\)"):
        ShardedShortlister([_stand_in()]).shortlist_late(tok, lengths, 2)
    sh = ShardedShortlister([_stand_in(3, True), _stand_in(70, True)])
    with pytest.raises(_lib.DrnError, match=r"shortlist_late: the queries must be \(S, L, 32\)"):
        sh.shortlist_late(q, lengths, 2)
    with pytest.raises(_lib.DrnError, match=r"L = 65 tokens outside \[1, 64\]"):
        sh.shortlist_late(res(torch.zeros(2, 65, 32, dtype=torch.bfloat16)), lengths, 2)
    with pytest.raises(_lib.DrnError, match="never read on the host"):
        sh.shortlist_late(tok, torch.tensor([3, 1], dtype=torch.int32), 2)
    with pytest.raises(_lib.DrnError, match=r"n = 129 outside \[1, 128\]"):
        sh.shortlist_late(tok, lengths, 129)
    with pytest.raises(_lib.DrnError, match="three buffers"):
        sh.shortlist_late(tok, lengths, 4, out=[None] * 4)
    with pytest.raises(_lib.DrnError, match="out.scores must be a contiguous"):
        sh.shortlist_late(tok, lengths, 4, out=[res(torch.zeros((2, 4), dtype=torch.int32)), res(torch.zeros((2, 4), dtype=torch.int32)),
                                                res(torch.zeros((2,), dtype=torch.int32))])
    with pytest.raises(_lib.DrnError, match="pack it first"):
        sh.shortlist_late(tok, lengths, 4, allow=torch.ones(73, dtype=torch.bool))


def test_the_wrappers_refuse_before_the_library_is_reached(monkeypatch):
    from drn_amd import _lib, ops
    _no_library(monkeypatch)
    res = lambda t: t.as_subclass(Resident)
    i32 = lambda *shape: res(torch.zeros(shape, dtype=torch.int32))
    f32 = lambda *shape: res(torch.zeros(shape))
    args = lambda K=2, S=3, n_in=4, n=4: [i32(K, S, n_in), f32(K, S, n_in), i32(K, S), None, i32(K + 1), n, i32(S, n), f32(S, n), i32(S)]
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.shortlist_merge_lists(*([torch.zeros((2, 3, 4), dtype=torch.int32)] + args()[1:]))
    for kw in (dict(K=65), dict(n_in=129)):
        with pytest.raises(_lib.DrnError, match=r"in_ids must be \(K, S, n_in\) with 1 <= K <= 64, S >= 1 and 1 <= n_in <= 128"):
            ops.shortlist_merge_lists(*args(**kw))
    for n in (0, 129):
        with pytest.raises(_lib.DrnError, match=r"n = %d outside \[1, 128\]" % n):
            ops.shortlist_merge_lists(*args(n=n))
    a = args()
    a[3] = i32(2, 3, 4)
    with pytest.raises(_lib.DrnError, match="rows must be given on both sides"):
        ops.shortlist_merge_lists(*a)
    with pytest.raises(_lib.DrnError, match="rows must be given on both sides"):
        ops.shortlist_merge_lists(*args(), rows=i32(3, 4))
    for at, wrong, name in ((1, i32(2, 3, 4), "in_scores"), (2, i32(3, 2), "in_counts"), (4, i32(2), "bases"), (6, i32(3, 5), "ids"), (8, i32(4), "counts")):
        a = args()
        a[at] = wrong
        with pytest.raises(_lib.DrnError, match="%s must be a contiguous" % name):
            ops.shortlist_merge_lists(*a)
    # the slices
    assert ops.allow_slice_words([0, 1, 64, 321, 775]) == 1 + 2 + 9 + 15 and ops.allow_slice_words([0, 775]) == 25
    words, bases, host = i32(25), i32(4), [0, 1, 64, 775]
    total = ops.allow_slice_words(host)
    with pytest.raises(_lib.DrnError, match=r"words must be a contiguous torch.int32 tensor \(25,\) or \(S, 25\)"):
        ops.allow_slices(i32(24), bases, host, i32(total))
    with pytest.raises(_lib.DrnError, match=r"out must be a contiguous \(%d,\) torch.int32 tensor \(2 rows of %d words\)" % (2 * total, total)):
        ops.allow_slices(i32(2, 25), bases, host, i32(total))
    with pytest.raises(_lib.DrnError, match=r"bases must be a contiguous \(4,\)"):
        ops.allow_slices(words, i32(3), host, i32(total))
    for bad in ([0], [1, 5], [0, 5, 5], list(range(66))):
        with pytest.raises(_lib.DrnError, match="host_bases must be the K \\+ 1 running sums"):
            ops.allow_slices(words, bases, bad, i32(total))


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_two_entries_at_abi_9():
    import drn_amd
    from drn_amd import _lib, ops
    lib = built_lib()
    assert lib.drn_abi_version() == 9
    hdr = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert int(re.search(r"#define DRN_SHARDS_MAX\s+(\d+)", hdr).group(1)) == _lib.SHARDS_MAX == 64
    assert int(re.search(r"#define DRN_SHORTLIST_MAX\s+(\d+)", hdr).group(1)) == _lib.SHORTLIST_MAX
    for name, count in ((MERGE, 14), (SLICES, 8)):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params, sig = _header_params(name), _lib.SIGNATURES[name]
        assert len(params) == len(sig) == count, (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
    for public in ("ShardedShortlister", "merge_shortlists_reference", "slice_allow_reference", "SHARDS_MAX"):
        assert hasattr(drn_amd, public), public
    assert callable(ops.shortlist_merge_lists) and callable(ops.allow_slices)
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "retrieve_shard.hip")).read()
    assert re.findall(r"__global__[^\n]*?void (\w+)\(", src) == ["shortlist_merge_lists_kernel", "allow_slices_kernel"]


def test_the_two_entries_check_their_arguments_before_anything_is_launched():
    lib = built_lib()
    p = ctypes.c_void_p(0x1000)
    # in_ids in_scores in_counts in_rows bases | ids scores counts rows
    def merge(K=3, S=2, n_in=5, n=4, ptrs=None):
        a = [p, p, p, None, p, p, p, p, None] if ptrs is None else ptrs
        return lib.drn_shortlist_merge_lists(a[0], a[1], a[2], a[3], a[4], K, S, n_in, n, a[5], a[6], a[7], a[8], None)
    for i in (0, 1, 2, 4, 5, 6, 7):
        assert merge(ptrs=[None if j in (i, 3, 8) else p for j in range(9)]) != 0 and b"null pointer" in lib.drn_last_error(), i
    for one in (3, 8):                                                        # rows on one side only
        assert merge(ptrs=[None if j == one else p for j in range(9)]) != 0 and b"rows must be given on both sides" in lib.drn_last_error(), one
    for K in (0, -1, 65):
        assert merge(K=K) != 0 and b"lists a sentence outside [1, 64]" in lib.drn_last_error(), K
    assert merge(S=0) != 0 and b"bad args" in lib.drn_last_error()
    for bad in (0, 129):
        assert merge(n_in=bad) != 0 and b"n_in = %d outside [1, 128]" % bad in lib.drn_last_error()
        assert merge(n=bad) != 0 and b"n = %d outside [1, 128]" % bad in lib.drn_last_error()
    for i in (0, 3, 8):
        assert merge(ptrs=[ctypes.c_void_p(0x1002) if j == i else p for j in range(9)]) != 0 and b"4-byte aligned" in lib.drn_last_error(), i

    def slices(rows=2, V=775, K=4, total=27, ptrs=(p, p, p)):
        return lib.drn_allow_slices(ptrs[0], rows, V, ptrs[1], K, total, ptrs[2], None)
    for i in range(3):
        assert slices(ptrs=[None if j == i else p for j in range(3)]) != 0 and b"null pointer" in lib.drn_last_error(), i
    assert slices(rows=0) != 0 and slices(V=0) != 0 and b"bad args" in lib.drn_last_error()
    for K in (0, 65):
        assert slices(K=K) != 0 and b"shards outside [1, 64]" in lib.drn_last_error(), K
    # K = 4 shards of 775 videos come to between 25 and 28 words a row
    for total in (24, 29, 0, -5):
        assert slices(total=total) != 0 and b"between 25 and 28" in lib.drn_last_error(), total
    assert slices(ptrs=(p, p, ctypes.c_void_p(0x1001))) != 0 and b"4-byte aligned" in lib.drn_last_error()
    assert slices(rows=1 << 27, total=25) != 0 and b"more than 2^31 words" in lib.drn_last_error()


# -- the compiler's resource notes --------------------------------------------------------------------------------------------------------

def test_the_shard_kernels_spill_nothing_and_keep_the_lds_the_source_claims(tmp_path):
    """csrc/retrieve_shard.hip compiled for gfx950 on its own: the merging wavefront with and without rows and the slicing kernel, each
    without scratch and without a spilled register; static LDS is what the arrays come to -- 2 x SL_MAX_N keys of 8 bytes and
    DRN_SHARDS_MAX + 1 bases for the merge, two tables of DRN_SHARDS_MAX + 1 words for the slices -- plus the compiler's alignment
    padding; VGPRs + AGPRs at or below 64, so eight wavefronts a SIMD."""
    from drn_amd import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(hipcc) and os.path.exists(readelf)):
        pytest.skip("hipcc / llvm-readelf not found")
    out = os.path.join(str(tmp_path), "retrieve_shard.co")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", out, "retrieve_shard.hip"], cwd=os.path.join(ROOT, "drn_amd", "csrc"),
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    notes = subprocess.run([readelf, "--notes", out], check=True, capture_output=True, text=True).stdout
    merge = 2 * _lib.SHORTLIST_MAX * 8 + (_lib.SHARDS_MAX + 1) * 4
    claims = {"shortlist_merge_lists_kernelILb0E": merge, "shortlist_merge_lists_kernelILb1E": merge, "allow_slices_kernel": 2 * (_lib.SHARDS_MAX + 1) * 4}
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
        assert claim[0] <= lds <= claim[0] + 16 and regs <= 64, (name, lds, regs)
