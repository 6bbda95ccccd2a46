"""The projected search index on the device: drn_gate_gather_packed against torch indexing on the same rows (bit for bit),
SearchIndex.build against prepare_input on the store's own gathers (bit for bit, whatever the build chunk), and Grounder.search on an
index against Grounder.search on the store it was built from: every Hits field equal, eagerly, by graph replay, after a refresh, with
the store gone, and on the committed mini dataset.  No tolerance anywhere: a GEMM row here does not depend on the batch it is
computed in (tests/test_search_gpu.py::test_search_does_not_depend_on_the_chunk_size rests on the same)."""
import functools
import gc

import pytest
import torch

from test_grounding_engine_gpu import DEV, dev_batch, tiny_model
from test_search_gpu import D, NV, S, T, boosted, dev_vids, per_pair_moments, same_hits, sentences, small_store

pytestmark = pytest.mark.gpu
PROPS = [32, 20, 32, 7, 32, 1, 25]           # small_store()'s proposal counts


# -- 1. the kernel alone -------------------------------------------------------------------------------------------------------------------

def packed_case(dtype, C, P, extra):
    """Videos of 12, 5, 1, 0 and 20 proposals at T = 12 (exact fit, ragged, one row, empty, truncated); vids with a repeat, -1 and
    Nv; 2 sentences x 7 slots.  rows / out are `extra` columns wider than C + P (row strides above the row)."""
    g = torch.Generator().manual_seed(C + P)
    nprops, L = [12, 5, 1, 0, 20], 12
    off = torch.tensor([0, 12, 17, 18, 18, 38], dtype=torch.int32)
    wide = torch.randn(39, C + P + extra, generator=g).to(dtype).to(DEV)
    rows = wide[:, :C + P]
    gate = torch.randn(2, C, generator=g).to(DEV)
    vids = [4, 1, -1, 3, 0, 5, 1]
    pair = torch.arange(14, dtype=torch.int32, device=DEV)
    pq, pv = torch.div(pair, 7, rounding_mode="floor"), torch.remainder(pair, 7)
    want = torch.empty(14, L, C + P, dtype=dtype, device=DEV)
    for p in range(14):
        v = vids[p % 7]
        n = nprops[v] if 0 <= v < 5 else 0
        src = torch.tensor([int(off[v]) + t if t < n else 38 for t in range(L)], device=DEV)
        want[p, :, :C] = (rows[src, :C].float() * gate[p // 7]).to(dtype)
        want[p, :, C:] = rows[src, C:]
    return rows, off.to(DEV), gate, pq, pv, dev_vids(vids), L, want


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P", [16, 0])
def test_gate_gather_packed_equals_torch_indexing(dtype, P):
    """Bit for bit, the pairs of -1, Nv and the empty video included: they are the pad row, gated.  168 rows of output in groups of 8
    rows per thread inside a pair: T = 12 leaves every pair a partial group.  P = 0: the wrapper allows an index without position
    columns."""
    from drn_amd import ops
    C, extra = 64, 8
    rows, off, gate, pq, pv, vids, L, want = packed_case(dtype, C, P, extra)
    out = torch.full((14, L, C + P + extra), 7.0, dtype=dtype, device=DEV)
    ops.gate_gather_packed(rows, 38, off, gate, pq, pv, vids, out, L, C, P, ops.dtype_code(rows), pq_host=pq.cpu())
    assert torch.equal(out[:, :, :C + P], want)
    assert bool((out[:, :, C + P:] == 7.0).all())                  # (columns past the row are not written)
    pad = torch.cat([(rows[38, :C].float() * gate[0]).to(dtype), rows[38, C:]])
    for p in (2, 3, 5):                                            # -1, the empty video, Nv: every row is the gated pad row
        assert torch.equal(out[p, :, :C + P], pad.expand(L, C + P)), p
    assert torch.equal(out[1, 5:, :C + P], pad.expand(L - 5, C + P))
    assert not torch.equal(out[0, :, :C], out[7, :, :C]) and torch.equal(out[0, :, C:], out[7, :, C:])


def test_gate_gather_packed_refuses_a_host_index_out_of_range():
    from drn_amd import _lib, ops
    rows, off, gate, pq, pv, vids, L, _ = packed_case(torch.float32, 64, 16, 0)
    out = torch.zeros(14, L, 80, device=DEV)
    bad = pq.cpu().clone()
    bad[9] = 2
    with pytest.raises(_lib.DrnError, match="pair 9 reads sentence 2 of 2"):
        ops.gate_gather_packed(rows, 38, off, gate, pq, pv, vids, out, L, 64, 16, 0, pq_host=bad)
    with pytest.raises(_lib.DrnError, match="int32"):
        ops.gate_gather_packed(rows, 38, off, gate, pq.long(), pv, vids, out, L, 64, 16, 0)
    assert not out.any()


# -- 2. the index --------------------------------------------------------------------------------------------------------------------------

def store_of(dim, dtype):
    """small_store()'s videos at another feature width."""
    from drn_amd.store import FeatureStore
    g = torch.Generator().manual_seed(5)
    videos = []
    for v, P in enumerate(PROPS):
        lo = torch.randint(0, 40, (P,), generator=g)
        hi = torch.minimum(lo + torch.randint(0, 12, (P,), generator=g), torch.tensor(39))
        pse = torch.stack([lo.double() / 40, (hi.double() + 1) / 40], dim=1)
        videos.append(("vid%d" % v, torch.randn(40, dim, generator=g), lo.numpy(), hi.numpy(), pse.numpy(), 320))
    return FeatureStore.from_tensors(videos, DEV, dtype)


@pytest.mark.parametrize("dim,dtype", [(64, torch.float32), (64, torch.bfloat16), (500, torch.bfloat16)])
def test_index_rows_are_prepare_inputs_rows(dim, dtype):
    """Per video the first nprops rows of Z | pos of prepare_input(split_gate=True) on store.gather([v], T = 32), the pad row = row 31
    of video 5 (one proposal), the same rows whatever the build chunk; (500, bf16): the zero-padded width 512."""
    from drn_amd import SearchIndex
    m = tiny_model(T, dim, dtype)
    store = small_store(dtype) if dim == 64 else store_of(dim, dtype)
    index = SearchIndex.build(m, store)
    Dp = 512 if dim == 500 else dim
    assert index.Dp == Dp and index.P == 256 and tuple(index.rows.shape) == (sum(PROPS) + 1, Dp + 256) and index.rows.dtype == dtype
    assert index.pad_row == sum(PROPS) and len(index) == NV and index.names == store.names and index.index == store.index
    assert index.nprops.tolist() == PROPS and index.D == dim and index.dtype == dtype and index.device == store.device
    assert index.prop_off.data_ptr() != store.prop_off.data_ptr() and torch.equal(index.prop_off, store.prop_off)
    assert index.nbytes == index.rows.numel() * index.rows.element_size() + index.prop_off.numel() * 4
    assert index.nbytes == index.rows.untyped_storage().nbytes() + index.prop_off.untyped_storage().nbytes()
    assert index.is_current(m)
    off = store.prop_off.tolist()
    with torch.no_grad():
        for v in range(NV):
            feats, pse, _ = store.gather([v], T=T)
            prep = m.prepare_input(feats, pse, split_gate=True)
            want = torch.cat([prep.Z.view(T, Dp), prep.G0.view(T, Dp + 256)[:, Dp:]], dim=1)
            assert torch.equal(index.rows[off[v]:off[v + 1]], want[:PROPS[v]]), v
            if v == 5:
                assert torch.equal(index.rows[index.pad_row], want[31])
    if dim == 500:
        assert not index.rows[:, 500:512].any() and bool(index.rows[:, :500].any())
    for chunk in (1, 3):
        assert torch.equal(SearchIndex.build(m, store, chunk=chunk).rows, index.rows), chunk


def test_a_store_without_a_padded_position_gets_its_pad_row_from_an_extra_chunk():
    """Two videos of 8 proposals each at T = 8, chunk = 1 and 2: no position of the walk is padding, so the pad row comes from one
    more chunk of empty slots -- and equals the pad row of a store that has padding."""
    from drn_amd import SearchIndex
    from drn_amd.store import FeatureStore
    m = tiny_model(T, D, torch.float32)
    g = torch.Generator().manual_seed(2)
    lo, hi = torch.arange(8).numpy(), (torch.arange(8) + 1).numpy()
    pse = torch.stack([torch.arange(8).double() / 9, (torch.arange(8).double() + 2) / 9], dim=1).numpy()
    full = FeatureStore.from_tensors([(name, torch.randn(9, D, generator=g), lo, hi, pse, 72) for name in ("a", "b")], DEV, torch.float32)
    ragged = SearchIndex.build(m, small_store())
    for chunk in (1, 2):
        index = SearchIndex.build(m, full, chunk=chunk)
        assert tuple(index.rows.shape) == (17, D + 256) and index.pad_row == 16
        assert torch.equal(index.rows[16], ragged.rows[ragged.pad_row]), chunk
        assert bool((index.rows[:16, :D] != index.rows[16, :D]).any(dim=1).all())


def test_max_bytes_one_byte_short_raises_and_allocates_nothing():
    from drn_amd import SearchIndex, _lib
    m, store = tiny_model(T, D, torch.float32), small_store()
    need = SearchIndex.bytes_of(sum(PROPS), D + 256, torch.float32, NV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.DrnError, match="max_bytes is %d" % (need - 1)):
        SearchIndex.build(m, store, max_bytes=need - 1)
    assert torch.cuda.memory_allocated() == before
    assert SearchIndex.build(m, store, max_bytes=need).nbytes == need


# -- 3. the search on an index -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared():
    """The boosted tiny fp32 model, small_store(), its index and two sets of sentences: built once, changed by no test."""
    from drn_amd import SearchIndex
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    return m, store, SearchIndex.build(m, store), sentences(7), sentences(11)


@pytest.mark.parametrize("per_video,top_k", [(1, 4), (3, 10)])
def test_search_on_the_index_equals_search_on_the_store(per_video, top_k):
    from drn_amd import Grounder, search
    m, store, index, (tok, qlen), _ = shared()
    grounder = Grounder(m, top_k=5)
    kw = dict(top_k=top_k, per_video=per_video)
    for extra in (dict(chunk=1), dict(chunk=3), dict(chunk=7), dict(), dict(videos=["vid4", "vid1"]), dict(T=40), dict(T=20, chunk=3)):
        want = grounder.search(tok, qlen, store, **dict(kw, **extra))
        same_hits(grounder.search(tok, qlen, index, **dict(kw, **extra)), want, extra)
        assert int(want.n.min()) > 0
    same_hits(search(m, tok, qlen, index, per_video=per_video), search(m, tok, qlen, store, per_video=per_video), "module-level search")
    assert m.fcos.box_selector_test.device_only is False


@pytest.mark.parametrize("vids", [[6, -1, -1], [3, 5, 0]])
def test_per_pair_moments_of_a_chunk_agree(vids):
    """select_moments' outputs for the pairs of one chunk, padded slots included: the index path's equal the store path's."""
    from drn_amd import Grounder
    m, store, index, (tok, qlen), _ = shared()
    grounder = Grounder(m, top_k=5)
    with torch.no_grad():
        gates = m.encode_query(tok, qlen)
        want = per_pair_moments(grounder, gates, store, vids, 3)
        pair = torch.arange(S * len(vids), dtype=torch.int32, device=DEV)
        pq, pv = torch.div(pair, len(vids), rounding_mode="floor"), torch.remainder(pair, len(vids))
        got = grounder._select(3, index, dev_vids(vids), pq, pv, gates, T, entry="forward_heads_packed")
    for a, b in zip(got, want):
        assert a.cpu().numpy().tobytes() == b.tobytes()


def test_search_on_the_index_by_graph_replay():
    """graph=True == eager; one capture for two sets of sentences and two chunk lists of the same shape; one more after a head
    parameter changed in place (the index stays current: it does not depend on the heads)."""
    from drn_amd import Grounder, SearchIndex
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    index = SearchIndex.build(m, store)
    eager, graphed = Grounder(m, top_k=6), Grounder(m, top_k=6, graph=True)
    (tok, qlen), (tok2, qlen2) = sentences(7), sentences(11)
    first = graphed.search(tok, qlen, index, per_video=2, chunk=3)
    same_hits(first, eager.search(tok, qlen, store, per_video=2, chunk=3), "first search")
    assert graphed.captures == 1
    kept = first.score.clone()
    second = graphed.search(tok2, qlen2, index, per_video=2, chunk=3)
    same_hits(second, eager.search(tok2, qlen2, index, per_video=2, chunk=3), "other sentences")
    assert graphed.captures == 1 and not torch.equal(second.score, first.score) and torch.equal(first.score, kept)
    same_hits(graphed.search(tok, qlen, index, per_video=2, chunk=3, videos=[6, 0, 3, 2]),
              eager.search(tok, qlen, store, per_video=2, chunk=3, videos=[6, 0, 3, 2]), "two chunks of the same shape")
    assert graphed.captures == 1
    with torch.no_grad():
        m.fcos.head.cls_logits.bias.add_(0.25)
    assert index.is_current(m)
    same_hits(graphed.search(tok, qlen, index, per_video=2, chunk=3), eager.search(tok, qlen, store, per_video=2, chunk=3), "new bias")
    assert graphed.captures == 2
    # the store path's graph of the same shape is another signature
    same_hits(graphed.search(tok, qlen, store, per_video=2, chunk=3), eager.search(tok, qlen, index, per_video=2, chunk=3), "store graph")
    assert graphed.captures == 3
    assert m.fcos.box_selector_test.device_only is False


def test_a_stale_index_raises_before_any_launch_and_refresh_mends_it():
    from drn_amd import Grounder, SearchIndex, _lib, ops
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    tok, qlen = sentences(7)
    index = SearchIndex.build(m, store)
    rows_at, old = index.rows.data_ptr(), index.rows.clone()
    grounder = Grounder(m, top_k=6)
    before = grounder.search(tok, qlen, index, per_video=2)
    with torch.no_grad():
        m.prop_fc.bias.add_(0.1)
    assert not index.is_current(m)
    ops.kernel_timer = []
    try:
        for g in (grounder, Grounder(m, top_k=6, graph=True)):
            with pytest.raises(_lib.DrnError, match="stale"):
                g.search(tok, qlen, index, per_video=2)
        launches = len(ops.kernel_timer)
    finally:
        ops.kernel_timer = None
    assert launches == 0
    other = tiny_model(T, D, torch.float32)
    with pytest.raises(_lib.DrnError, match="stale"):
        Grounder(other, top_k=6).search(tok, qlen, index, per_video=2)
    assert index.refresh(m) is index and index.is_current(m)
    assert index.rows.data_ptr() == rows_at and not torch.equal(index.rows, old)
    after = grounder.search(tok, qlen, index, per_video=2)
    same_hits(after, grounder.search(tok, qlen, store, per_video=2), "after the refresh")
    assert not torch.equal(after.score, before.score)
    assert torch.equal(SearchIndex.build(m, store).rows, index.rows)


def test_an_indexed_search_launches_no_pooling_and_fewer_kernels_per_chunk():
    from drn_amd import Grounder, ops
    m, store, index, (tok, qlen), _ = shared()
    grounder = Grounder(m, top_k=6)
    tags = {}
    for name, where in (("store", store), ("index", index)):
        ops.kernel_timer = []
        try:
            grounder.search(tok, qlen, where, per_video=2, chunk=3)
            tags[name] = [t[0] for t in ops.kernel_timer]
        finally:
            ops.kernel_timer = None
    print("timed launches over 3 chunks: store %d, index %d" % (len(tags["store"]), len(tags["index"])))
    assert tags["store"].count("pool_props") == 3 and "pool_props" not in tags["index"]
    assert tags["index"].count("gate_gather_packed") == 3 and "gate_gather_packed" not in tags["store"]
    # the sentences are encoded once in both; the rest is per chunk: 3 chunks, at least one launch fewer in each
    assert len(tags["store"]) - len(tags["index"]) >= 3


def test_the_index_outlives_its_store():
    from drn_amd import Grounder, SearchIndex, _lib
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    tok, qlen = sentences(7)
    grounder = Grounder(m, top_k=6)
    index = SearchIndex.build(m, store)
    want = grounder.search(tok, qlen, store, per_video=2, chunk=3)
    names = list(store.names)
    del store
    gc.collect()
    assert index._store() is None
    same_hits(grounder.search(tok, qlen, index, per_video=2, chunk=3), want, "after del store")
    assert grounder.search(tok, qlen, index, per_video=2, chunk=3).tolist(names=index.names)[0][0][0] in names
    with pytest.raises(_lib.DrnError, match="store the index was built from is gone"):
        index.refresh(m)
    index.refresh(m, small_store())
    same_hits(grounder.search(tok, qlen, index, per_video=2, chunk=3), want, "refreshed from an equal store")


def test_search_on_the_mini_dataset_index_equals_the_store():
    """test_search_on_the_mini_dataset_against_ground's setup (bf16, every sentence of the test split against the whole store)."""
    from drn_amd import Grounder, SearchIndex
    from drn_amd.store import FeatureStore
    from test_store_gpu import hip_model, host_loader, mini, mini_cfg
    ds = mini("test", 3)
    st = FeatureStore.from_dataset(ds, DEV, torch.bfloat16)
    m = hip_model(3, cfg=mini_cfg(3))
    m.set_compute_dtype(torch.bfloat16)
    boosted(m).eval()
    names, _, _, _, tok, qlen, _, _ = next(iter(host_loader(ds, len(ds), torch.bfloat16)))
    tok, qlen = tok.to(DEV), qlen.to(DEV)
    Nv = len(st)
    index = SearchIndex.build(m, st)
    assert index.nbytes == SearchIndex.bytes_of(int(st.nprops.sum()), index.Dp + index.P, torch.bfloat16, Nv)
    grounder = Grounder(m, top_k=5)
    want = grounder.search(tok, qlen, st, top_k=5 * Nv, per_video=5)
    got = grounder.search(tok, qlen, index, top_k=5 * Nv, per_video=5)
    same_hits(got, want, "mini dataset")
    assert int(got.n.max()) > 5
