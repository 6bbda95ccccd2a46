"""Host side of the projected search index (drn_amd.SearchIndex, Grounder.search on an index): the C-ABI boundary of
drn_gate_gather_packed and the refusals that need no GPU."""
import ctypes
import types

import pytest
import torch

from test_grounding_cpu import _header_params, built_lib


def test_library_exports_gate_gather_packed_at_abi_9():
    import drn_amd
    from drn_amd import _lib, index, ops
    lib = built_lib()
    assert "drn_gate_gather_packed" in _lib.declared_symbols() and hasattr(lib, "drn_gate_gather_packed")
    assert lib.drn_abi_version() == 9
    assert callable(ops.gate_gather_packed)
    assert drn_amd.SearchIndex is index.SearchIndex and callable(drn_amd.SearchIndex.build)
    from drn_amd.model import mainModel
    assert callable(mainModel.forward_heads_packed)


def test_header_and_ctypes_signatures_agree():
    from drn_amd import _lib
    params = _header_params("drn_gate_gather_packed")
    sig = _lib.SIGNATURES["drn_gate_gather_packed"]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(built_lib().drn_gate_gather_packed.argtypes) == list(sig)


def test_argument_checks_answer_before_anything_is_launched():
    """Every refusal is an error return with a text and no device work (this runs without a GPU)."""
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def call(ptrs=None, pq_host=None, ld_rows=80, n_rows=71, pad_row=70, Nv=5, ldg=64, S=2, Vc=7, ld_out=80, Q=14, T=12, C=64, P=16, dtype=1):
        a = [p] * 7 if ptrs is None else ptrs          # rows prop_off gate pq pv vids out
        return L.drn_gate_gather_packed(a[0], ld_rows, n_rows, pad_row, a[1], Nv, a[2], ldg, S, a[3], pq_host, a[4], a[5], Vc, a[6], ld_out,
                                        Q, T, C, P, dtype, None)
    for i in range(7):
        assert call(ptrs=[None if j == i else p for j in range(7)]) != 0, i
        assert b"null pointer" in L.drn_last_error()
    for dtype, C in ((1, 60), (0, 62)):                # 60 bf16 = 120 bytes, 62 f32 = 248 bytes
        assert call(C=C, dtype=dtype) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(P=12) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(ld_out=72) != 0 and b"shorter than its row" in L.drn_last_error()          # ld_out < C + P
    assert call(ld_rows=72) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ldg=32) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(pad_row=71) != 0 and call(pad_row=-1) != 0 and call(n_rows=0, pad_row=0) != 0
    assert call(Q=0) != 0 and call(T=0) != 0 and call(C=0) != 0 and call(P=-8) != 0 and call(S=0) != 0 and call(Vc=0) != 0 and call(Nv=0) != 0
    assert call(Q=1 << 20, T=1 << 12) != 0 and b"2^31 rows" in L.drn_last_error()
    assert call(dtype=7) != 0 and b"bad dtype" in L.drn_last_error()
    for bad, text in ((2, b"pair 3 reads sentence 2 of 2"), (-1, b"pair 3 reads sentence -1 of 2")):
        pq = (ctypes.c_int32 * 14)(*([0, 1, 1, bad] + [0] * 10))
        assert call(pq_host=ctypes.cast(pq, ctypes.c_void_p)) != 0 and text in L.drn_last_error()


def test_the_wrapper_refuses_host_tensors_and_wrong_index_types():
    from drn_amd import _lib, ops
    rows, gate = torch.zeros(71, 80), torch.zeros(2, 64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.gate_gather_packed(rows, 70, i32(6), gate, i32(14), i32(14), i32(7), torch.zeros(14, 12, 80), 12, 64, 16, 0)


def test_search_on_an_index_refuses_as_on_a_store():
    """Train mode, host sentences, an index on the host, a dtype that is not the model's, and a stale index: each raises before
    anything is read from the device (stand-ins that only claim to live there)."""
    from drn_amd import Grounder, SearchIndex, _lib
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, synthetic_batch
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1)))
    tok, qlen = synthetic_batch(2, 32, 64)[:2]
    idx = SearchIndex()
    idx.names, idx.index, idx.dtype, idx.device = ["a", "b"], {"a": 0, "b": 1}, torch.float32, torch.device("cpu")
    idx.rows = torch.zeros(4, 64 + 256)
    with pytest.raises(_lib.DrnError, match="eval"):
        Grounder(m.train()).search(tok, qlen, idx)
    m.eval()
    with pytest.raises(_lib.DrnError, match="no CPU fallback"):
        Grounder(m).search(tok, qlen, idx)
    dtok = types.SimpleNamespace(is_cuda=True, shape=(2, 8), device="cuda:0")
    for g in (Grounder(m), Grounder(m, graph=True)):
        with pytest.raises(_lib.DrnError, match="store on the GPU"):
            g.search(dtok, dtok, idx)
    idx.rows = types.SimpleNamespace(is_cuda=True, device="cuda:0")
    idx.dtype = torch.bfloat16
    with pytest.raises(_lib.DrnError, match="the store holds"):
        Grounder(m).search(dtok, dtok, idx)
    idx.dtype = torch.float32
    idx.stamp = SearchIndex._stamp(m)
    assert idx.is_current(m)
    with torch.no_grad():
        m.prop_fc.bias.add_(0.1)
    assert not idx.is_current(m)
    with pytest.raises(_lib.DrnError, match="stale"):
        Grounder(m).search(dtok, dtok, idx)
    other = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1))).eval()
    idx.stamp = SearchIndex._stamp(other)
    with pytest.raises(_lib.DrnError, match="stale"):
        Grounder(m).search(dtok, dtok, idx)
    idx.stamp = SearchIndex._stamp(m)
    m.set_compute_dtype(torch.bfloat16)
    assert not idx.is_current(m)


def test_build_refuses_before_anything_is_allocated():
    from drn_amd import FeatureStore, SearchIndex, _lib
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1)))
    videos = [("v%d" % v, torch.randn(8, 64), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64) for v in range(3)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    with pytest.raises(_lib.DrnError, match="eval"):
        SearchIndex.build(m.train(), store)
    m.eval()
    with pytest.raises(_lib.DrnError, match="store on the GPU"):
        SearchIndex.build(m, store)
    store.feats = types.SimpleNamespace(is_cuda=True, device="cuda:0")
    need = SearchIndex.bytes_of(6, 64 + 256, torch.float32, 3)
    assert need == 7 * 320 * 4 + 4 * 4
    with pytest.raises(_lib.DrnError, match="max_bytes is %d" % (need - 1)):
        SearchIndex.build(m, store, max_bytes=need - 1)
    store.dtype = torch.bfloat16
    with pytest.raises(_lib.DrnError, match="the store holds"):
        SearchIndex.build(m, store)
