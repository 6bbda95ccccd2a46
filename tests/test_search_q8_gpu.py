"""The block-scaled FP8 search index on the device: drn_quantize_rows_mx8 against the host definition (drn_amd.index.mx8_quantize,
pinned by tests/test_search_q8_cpu.py) byte for byte, drn_gate_gather_packed_q8 against drn_gate_gather_packed on the dequantised
rows bit for bit, SearchIndex.build(quantize="mxfp8") against the definition applied to the plain index's rows, and every search path
on the quantised index against the same path on index.dequantized(): every Hits / Moments field equal.  No tolerance anywhere: a
dequantised value is exact in fp32 and bf16."""
import functools

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV, tiny_model
from test_search_gpu import D, NV, S, T, boosted, dev_vids, same_hits, sentences, small_store
from test_search_index_gpu import PROPS, packed_case, store_of
from test_search_q8_cpu import corner_rows

pytestmark = pytest.mark.gpu
MOMENT = ("seg", "score", "level", "index", "n")


# -- 1. the quantise kernel against the definition -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 1088])
def test_quantize_rows_equals_the_definition_byte_for_byte(dtype, C):
    """39 rows: the 12 corner rows of the CPU test (in bf16: what bf16 makes of them), then 27 random rows whose magnitudes span
    2^-20 .. 2^20.  1088 columns = 34 blocks = 68 lanes of 16 columns: one wave's span and a partial second one.  Row strides above the
    rows: x C + 8, codes C + 16, scales C / 32 + 3, and what lies past a row keeps its fill."""
    from drn_amd import ops
    from drn_amd.index import mx8_quantize
    g = torch.Generator().manual_seed(C)
    x = torch.cat([corner_rows(C)[0], torch.randn(27, C, generator=g) * torch.exp2(torch.linspace(-20, 20, 27)).unsqueeze(1)]).to(dtype)
    if C > 64:
        x[:12, 64:] = x[12:24, 64:] * 2.0 ** -6                      # (the corner rows' other blocks are not all zero)
        x[2, 1056:] = 0.0
    wide = torch.full((39, C + 8), 5.0, dtype=dtype, device=DEV)
    wide[:, :C] = x.to(DEV)
    codes = torch.full((39, C + 16), 0xa5, dtype=torch.uint8, device=DEV)
    scales = torch.full((39, C // 32 + 3), 0xa5, dtype=torch.uint8, device=DEV)
    ops.quantize_rows_mx8(wide[:, :C], codes[:, :C], scales[:, :C // 32])
    want_c, want_s = mx8_quantize(x)
    got_c, got_s = codes.cpu(), scales.cpu()
    bad = (got_s[:, :C // 32] != want_s).nonzero()
    assert bad.numel() == 0, ("scales", bad[:8].tolist(), got_s[:, :C // 32][want_s != got_s[:, :C // 32]][:8], want_s[want_s != got_s[:, :C // 32]][:8])
    bad = (got_c[:, :C] != want_c).nonzero()
    assert bad.numel() == 0, ("codes", bad[:8].tolist(), got_c[:, :C][want_c != got_c[:, :C]][:8], want_c[want_c != got_c[:, :C]][:8])
    assert bool((got_c[:, C:] == 0xa5).all()) and bool((got_s[:, C // 32:] == 0xa5).all())
    assert int(want_s.min()) == 17 and int(want_s.max()) > 127 + 20 and 0x80 in want_c[8].tolist() and 0xfe in want_c[4].tolist()


# -- 2. the gather kernel against the plain one on the dequantised rows ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P", [16, 0])
@pytest.mark.parametrize("C", [64, 1088])
def test_gate_gather_q8_equals_the_plain_kernel_on_dequantised_rows(dtype, P, C):
    """test_search_index_gpu.packed_case's videos, slots and pairs; the codes and scales come from the host definition, with row
    strides above the rows.  out is 8 columns wider than a row."""
    from drn_amd import ops
    from drn_amd.index import mx8_dequantize, mx8_quantize
    rows, off, gate, pq, pv, vids, L, _ = packed_case(dtype, C, P, 8)
    rows[5, 32:64] = 0.0                                               # a zero block, and a row of another magnitude
    rows[7, :C] *= 2.0 ** -12
    c, s = mx8_quantize(rows[:, :C].cpu())
    codes = torch.full((39, C + 16), 0x7e, dtype=torch.uint8, device=DEV)
    scales = torch.full((39, C // 32 + 3), 0xfe, dtype=torch.uint8, device=DEV)
    codes[:, :C], scales[:, :C // 32] = c.to(DEV), s.to(DEV)
    pos = rows[:, C:] if P else None
    plain = torch.cat([mx8_dequantize(c, s, dtype).to(DEV), rows[:, C:]], dim=1).contiguous()
    assert not torch.equal(plain[:, :C], rows[:, :C])
    want = torch.full((14, L, C + P + 8), 7.0, dtype=dtype, device=DEV)
    ops.gate_gather_packed(plain, 38, off, gate, pq, pv, vids, want, L, C, P, ops.dtype_code(plain), pq_host=pq.cpu())
    out = torch.full((14, L, C + P + 8), 7.0, dtype=dtype, device=DEV)
    ops.gate_gather_packed_q8(codes[:, :C], scales[:, :C // 32], pos, 38, off, gate, pq, pv, vids, out, L, C, P, ops.dtype_code(out),
                              pq_host=pq.cpu())
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(out.view(bits), want.view(bits))               # (the bits: -0 is not +0 here)
    assert bool((out[:, :, C + P:] == 7.0).all())                      # (columns past the row are not written)
    pad = torch.cat([(plain[38, :C].float() * gate[0]).to(dtype), plain[38, C:]])
    for p in (2, 3, 5):                                                # -1, the empty video, Nv: every row is the gated, dequantised pad row
        assert torch.equal(out[p, :, :C + P], pad.expand(L, C + P)), p
    assert torch.equal(out[1, 5:, :C + P], pad.expand(L - 5, C + P))
    assert not torch.equal(out[0, :, :C], out[7, :, :C]) and torch.equal(out[0, :, C:C + P], out[7, :, C:C + P])


def test_gate_gather_q8_refuses_a_host_index_out_of_range():
    from drn_amd import _lib, ops
    from drn_amd.index import mx8_quantize
    rows, off, gate, pq, pv, vids, L, _ = packed_case(torch.float32, 64, 16, 0)
    c, s = (t.to(DEV) for t in mx8_quantize(rows[:, :64].cpu()))
    out = torch.zeros(14, L, 80, device=DEV)
    bad = pq.cpu().clone()
    bad[9] = 2
    with pytest.raises(_lib.DrnError, match="pair 9 reads sentence 2 of 2"):
        ops.gate_gather_packed_q8(c, s, rows[:, 64:], 38, off, gate, pq, pv, vids, out, L, 64, 16, 0, pq_host=bad)
    with pytest.raises(_lib.DrnError, match="int32"):
        ops.gate_gather_packed_q8(c, s, rows[:, 64:], 38, off, gate, pq.long(), pv, vids, out, L, 64, 16, 0)
    assert not out.any()


# -- 3. the index --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,dtype", [(64, torch.float32), (64, torch.bfloat16), (500, torch.bfloat16)])
def test_a_quantised_index_holds_the_definition_of_the_plain_rows(dim, dtype):
    from drn_amd import SearchIndex
    from drn_amd.index import mx8_quantize
    m = tiny_model(T, dim, dtype)
    store = small_store(dtype) if dim == 64 else store_of(dim, dtype)
    plain = SearchIndex.build(m, store)
    q = SearchIndex.build(m, store, quantize="mxfp8")
    Dp, n = (512 if dim == 500 else dim), sum(PROPS) + 1
    assert q.quantize == "mxfp8" and plain.quantize is None and q.rows is None and q.resident is q.codes and plain.resident is plain.rows
    assert q.Dp == Dp and q.P == 256 and q.pad_row == n - 1 and len(q) == NV and q.names == store.names
    assert q.codes.dtype == q.scales.dtype == torch.uint8 and q.pos.dtype == dtype
    assert tuple(q.codes.shape) == (n, Dp) and tuple(q.scales.shape) == (n, Dp // 32) and tuple(q.pos.shape) == (n, 256)
    want_c, want_s = mx8_quantize(plain.rows[:, :Dp].cpu())
    assert torch.equal(q.codes.cpu(), want_c) and torch.equal(q.scales.cpu(), want_s)          # the pad row like any other row
    assert torch.equal(q.pos, plain.rows[:, Dp:]) and torch.equal(q.prop_off, plain.prop_off)
    if dim == 500:
        assert not q.codes[:, 500:512].any() and bool(q.codes[:, :500].any())
    for chunk in (1, 3):
        other = SearchIndex.build(m, store, chunk=chunk, quantize="mxfp8")
        assert torch.equal(other.codes, q.codes) and torch.equal(other.scales, q.scales) and torch.equal(other.pos, q.pos), chunk
    need = SearchIndex.bytes_of(sum(PROPS), Dp + 256, dtype, NV, quantize="mxfp8", P=256)
    assert q.nbytes == need == n * (Dp + Dp // 32 + 256 * q.pos.element_size()) + (NV + 1) * 4
    assert need == sum(t.untyped_storage().nbytes() for t in (q.codes, q.scales, q.pos, q.prop_off))
    assert need < plain.nbytes
    # the dequantised twin: a plain index of the same videos, current for the same model, within the format's error of the plain rows
    ref = q.dequantized()
    assert ref.quantize is None and ref.codes is None and ref.rows.dtype == dtype and tuple(ref.rows.shape) == tuple(plain.rows.shape)
    assert ref.is_current(m) and q.is_current(m) and ref.names == q.names and ref.pad_row == q.pad_row and ref.nbytes == plain.nbytes
    assert torch.equal(ref.rows[:, Dp:], plain.rows[:, Dp:]) and torch.equal(ref.prop_off, plain.prop_off)
    a, b = ref.rows[:, :Dp].float().cpu(), plain.rows[:, :Dp].float().cpu()
    e = (want_s.to(torch.int32) - 127).repeat_interleave(32, dim=1)
    assert bool(((a - b).abs() <= torch.maximum(b.abs() * 2.0 ** -4, torch.ldexp(torch.ones(()), e - 10))).all())
    assert not torch.equal(a, b)


def test_max_bytes_is_checked_against_the_quantised_size_and_allocates_nothing():
    from drn_amd import SearchIndex, _lib
    m, store = tiny_model(T, D, torch.float32), small_store()
    need = SearchIndex.bytes_of(sum(PROPS), D + 256, torch.float32, NV, quantize="mxfp8", P=256)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(_lib.DrnError, match="max_bytes is %d" % (need - 1)):
        SearchIndex.build(m, store, max_bytes=need - 1, quantize="mxfp8")
    assert torch.cuda.memory_allocated() == before
    assert SearchIndex.build(m, store, max_bytes=need, quantize="mxfp8").nbytes == need        # (the plain index would not fit)
    with pytest.raises(_lib.DrnError, match="max_bytes is %d" % need):
        SearchIndex.build(m, store, max_bytes=need)
    with pytest.raises(_lib.DrnError, match="quantize must be None or"):
        SearchIndex.build(m, store, quantize="int4")
    assert torch.cuda.memory_allocated() == before


# -- 4. the search on a quantised index ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared():
    """The boosted tiny fp32 model, small_store(), its plain index, its quantised index and that one's dequantised twin, and two sets
    of sentences: built once, changed by no test."""
    from drn_amd import SearchIndex
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    q = SearchIndex.build(m, store, quantize="mxfp8")
    return m, store, SearchIndex.build(m, store), q, q.dequantized(), sentences(7), sentences(11)


@pytest.mark.parametrize("per_video,top_k", [(1, 4), (3, 10)])
def test_search_on_the_quantised_index_equals_search_on_its_dequantised_twin(per_video, top_k):
    from drn_amd import Grounder, search
    m, store, plain, q, ref, (tok, qlen), _ = shared()
    grounder = Grounder(m, top_k=5)
    kw = dict(top_k=top_k, per_video=per_video)
    shortlists = [["vid1", "vid4", "vid6"], [], [0, 6, 3, 5, 2]]
    for extra in (dict(chunk=1), dict(chunk=3), dict(chunk=7), dict(), dict(videos=["vid4", "vid1"]), dict(T=40), dict(T=20, chunk=3),
                  dict(candidates=shortlists), dict(candidates=shortlists, pairs=3, chunk=2)):
        want = grounder.search(tok, qlen, ref, **dict(kw, **extra))
        same_hits(grounder.search(tok, qlen, q, **dict(kw, **extra)), want, extra)
        if "candidates" in extra:
            assert want.n.tolist()[1] == 0 and want.n.tolist()[0] > 0 and want.n.tolist()[2] > 0
        else:
            assert int(want.n.min()) > 0                               # every sentence has at least one hit
    same_hits(search(m, tok, qlen, q, per_video=per_video), search(m, tok, qlen, ref, per_video=per_video), "module-level search")
    # not by reading a plain table: the plain index scores differently somewhere
    assert not torch.equal(grounder.search(tok, qlen, q, **kw).score, grounder.search(tok, qlen, plain, **kw).score)
    assert m.fcos.box_selector_test.device_only is False


def test_ground_stored_and_evaluate_search_agree_with_the_twin():
    from drn_amd import Grounder, evaluate_search
    m, store, plain, q, ref, (tok, qlen), (tok2, qlen2) = shared()
    grounder = Grounder(m, top_k=5)
    names = ["vid2", "vid5", "vid2"]
    got, want = grounder.ground_stored(tok, qlen, q, names, T=T), grounder.ground_stored(tok, qlen, ref, names, T=T)
    for f in MOMENT:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    gt = want.seg[:, 0].double().cpu()
    batches = [(names, tok, qlen, gt), (["vid5", "vid6", "vid3"], tok2, qlen2, torch.tensor([[0.0, 0.5], [0.125, 0.625], [0.375, 1.0]]))]
    kw = dict(ious=(0.3, 0.5, 0.7), topks=(1, 5, 10), per_video=2, chunk=3)
    a, b = evaluate_search(grounder, batches, q, **kw), evaluate_search(grounder, batches, ref, **kw)
    assert a.first_hits.tolist() == b.first_hits.tolist() and a.moment == b.moment and a.video == b.video and a.n == 6
    assert (a.first_hits < 10).any()


def test_search_on_the_mini_dataset_quantised_index_equals_its_twin():
    """test_search_index_gpu.test_search_on_the_mini_dataset_index_equals_the_store's setup (bf16, D = 12 padded to 64 columns)."""
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
    q = SearchIndex.build(m, st, quantize="mxfp8")
    assert q.Dp == 64 and q.nbytes == SearchIndex.bytes_of(int(st.nprops.sum()), q.Dp + q.P, torch.bfloat16, Nv, quantize="mxfp8", P=q.P)
    ref = q.dequantized()
    grounder = Grounder(m, top_k=5)
    got = grounder.search(tok, qlen, q, top_k=5 * Nv, per_video=5)
    same_hits(got, grounder.search(tok, qlen, ref, top_k=5 * Nv, per_video=5), "mini dataset")
    assert int(got.n.min()) > 0 and int(got.n.max()) > 5
    videos = [st.index[name] for name in names]
    a, b = grounder.ground_stored(tok, qlen, q, videos), grounder.ground_stored(tok, qlen, ref, videos)
    for f in MOMENT:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


# -- 5. graph replay -------------------------------------------------------------------------------------------------------------------------

def test_search_on_the_quantised_index_by_graph_replay():
    """graph=True on the quantised index == eager on its twin; one capture for two sets of sentences; the plain index of the same
    shape is another signature and takes one more."""
    from drn_amd import Grounder
    m, store, plain, q, ref, (tok, qlen), (tok2, qlen2) = shared()
    eager, graphed = Grounder(m, top_k=6), Grounder(m, top_k=6, graph=True)
    first = graphed.search(tok, qlen, q, per_video=2, chunk=3)
    same_hits(first, eager.search(tok, qlen, ref, per_video=2, chunk=3), "first search")
    assert graphed.captures == 1
    second = graphed.search(tok2, qlen2, q, per_video=2, chunk=3)
    same_hits(second, eager.search(tok2, qlen2, ref, per_video=2, chunk=3), "other sentences")
    assert graphed.captures == 1 and not torch.equal(second.score, first.score)
    on_plain = graphed.search(tok, qlen, plain, per_video=2, chunk=3)
    same_hits(on_plain, eager.search(tok, qlen, plain, per_video=2, chunk=3), "the plain index's graph")
    assert graphed.captures == 2 and not torch.equal(on_plain.score, first.score)
    same_hits(graphed.search(tok, qlen, q, per_video=2, chunk=3), first, "the first graph again")
    assert graphed.captures == 2
    assert m.fcos.box_selector_test.device_only is False


# -- 6. a stale index and refresh ------------------------------------------------------------------------------------------------------------

def test_a_stale_quantised_index_raises_before_any_launch_and_refresh_mends_it():
    from drn_amd import Grounder, SearchIndex, _lib, ops
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    tok, qlen = sentences(7)
    q = SearchIndex.build(m, store, quantize="mxfp8")
    at, old = (q.codes.data_ptr(), q.scales.data_ptr(), q.pos.data_ptr()), q.codes.clone()
    grounder = Grounder(m, top_k=6)
    before = grounder.search(tok, qlen, q, per_video=2)
    with torch.no_grad():
        m.prop_fc.bias.add_(0.1)
    assert not q.is_current(m)
    ops.kernel_timer = []
    try:
        for g in (grounder, Grounder(m, top_k=6, graph=True)):
            with pytest.raises(_lib.DrnError, match="stale"):
                g.search(tok, qlen, q, per_video=2)
        launches = len(ops.kernel_timer)
    finally:
        ops.kernel_timer = None
    assert launches == 0
    assert q.refresh(m) is q and q.is_current(m) and q.quantize == "mxfp8" and q.rows is None
    assert (q.codes.data_ptr(), q.scales.data_ptr(), q.pos.data_ptr()) == at and not torch.equal(q.codes, old)
    after = grounder.search(tok, qlen, q, per_video=2)
    same_hits(after, grounder.search(tok, qlen, q.dequantized(), per_video=2), "after the refresh")
    assert not torch.equal(after.score, before.score)
    fresh = SearchIndex.build(m, store, quantize="mxfp8")
    assert torch.equal(fresh.codes, q.codes) and torch.equal(fresh.scales, q.scales) and torch.equal(fresh.pos, q.pos)


# -- 7. launch tags ----------------------------------------------------------------------------------------------------------------------------

def test_a_quantised_search_launches_its_own_gather_and_nothing_of_the_build():
    from drn_amd import Grounder, SearchIndex, ops
    m, store, plain, q, ref, (tok, qlen), _ = shared()
    grounder = Grounder(m, top_k=6)
    tags = {}
    for name, where in (("plain", plain), ("q8", q)):
        ops.kernel_timer = []
        try:
            grounder.search(tok, qlen, where, per_video=2, chunk=3)
            tags[name] = [t[0] for t in ops.kernel_timer]
        finally:
            ops.kernel_timer = None
    assert tags["q8"].count("gate_gather_packed_q8") == 3 and "gate_gather_packed_q8" not in tags["plain"]
    assert "gate_gather_packed" not in tags["q8"] and "pool_props" not in tags["q8"] and "quantize_rows_mx8" not in tags["q8"]
    assert len(tags["q8"]) == len(tags["plain"])                      # (one launch for one launch)
    ops.kernel_timer = []
    try:
        SearchIndex.build(m, store, chunk=3, quantize="mxfp8")
        built = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    # 3 chunks of 3 slots: one quantise launch per chunk with proposals, one more for the pad row
    assert built.count("quantize_rows_mx8") == 4 and "gate_gather_packed_q8" not in built
