"""Host side of the search across a store's videos (Grounder.search): the C-ABI boundary of drn_merge_moments, the ordering rule on
host records (metrics.merge_moments, which tests/test_search_gpu.py uses as the kernel's model) and the refusals that need no GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_merge_moments_at_abi_9():
    import drn_amd
    from drn_amd import _lib, grounding, ops
    lib = built_lib()
    assert "drn_merge_moments" in _lib.declared_symbols() and hasattr(lib, "drn_merge_moments")
    assert lib.drn_abi_version() == 9
    assert callable(ops.merge_moments) and callable(ops.merge_state)
    assert drn_amd.Hits is grounding.Hits and drn_amd.search is grounding.search and callable(drn_amd.Grounder.search)
    hdr = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    assert int(re.search(r"#define DRN_MERGE_MAX_CAND\s+(\d+)", hdr).group(1)) == _lib.MERGE_MAX_CAND


def test_header_and_ctypes_signatures_agree():
    from drn_amd import _lib
    params = _header_params("drn_merge_moments")
    sig = _lib.SIGNATURES["drn_merge_moments"]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(built_lib().drn_merge_moments.argtypes) == list(sig)


def test_argument_checks_answer_before_anything_is_launched():
    """Every refusal is an error return with a text and no device work (this runs without a GPU)."""
    from drn_amd import _lib
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def call(S=2, Vc=3, kv=2, K=4, ptrs=None):
        a = [p] * 12 if ptrs is None else ptrs        # seg score level index n | vids | st_seg st_score st_video st_level st_rank st_n
        return L.drn_merge_moments(a[0], a[1], a[2], a[3], a[4], S, Vc, kv, a[5], 5, K, 1, None, *a[6:], None)
    for i in range(12):
        assert call(ptrs=[None if j == i else p for j in range(12)]) != 0, i
        assert b"null pointer" in L.drn_last_error()
    assert call(K=0) != 0 and b"K = 0" in L.drn_last_error()
    assert call(K=-3) != 0 and b"K = -3" in L.drn_last_error()
    assert call(kv=0) != 0 and b"kv = 0" in L.drn_last_error()
    assert call(S=0) != 0 and call(Vc=0) != 0
    cap = _lib.MERGE_MAX_CAND
    assert call(K=cap - 5, Vc=3, kv=2) != 0 and (b"%d candidates per sentence (max %d)" % (cap + 1, cap)) in L.drn_last_error()
    assert call(K=1, Vc=1 << 20, kv=1 << 12) != 0 and b"candidates per sentence" in L.drn_last_error()      # (no int overflow)


# -- the ordering rule on host records --------------------------------------------------------------------------------------------------

def test_host_merge_ties_and_drops():
    from drn_amd.metrics import merge_moments
    # a score tie across two videos goes to the lower position, whatever the order the pairs are listed in
    got = merge_moments([[[0.1, 0.2, 0.5]], [[0.3, 0.4, 0.5]]], [6, 2], 5)
    assert got == [[2, 0.3, 0.4, 0.5, 0], [6, 0.1, 0.2, 0.5, 0]]
    # a tie inside a pair goes to the lower rank; a higher score elsewhere still comes first
    got = merge_moments([[[0.1, 0.2, 0.5, 7], [0.3, 0.4, 0.5, 3]], [[0.0, 0.5, 0.75, 0]]], [1, 4], 5)
    assert got == [[4, 0.0, 0.5, 0.75, 0], [1, 0.1, 0.2, 0.5, 0], [1, 0.3, 0.4, 0.5, 1]]
    # the fallback moment (index < 0), padded pairs (video None / negative), padded records (None) and non-finite scores are dropped;
    # a dropped record still counts for the rank of the ones behind it
    pairs = [[[0.0, 1.0, 1.0, -1]],
             [[0.1, 0.2, 0.9, 0]],
             [[0.1, 0.2, 0.8, 0]],
             [[0.2, 0.3, float("nan"), 4], [0.2, 0.4, 0.3, 5], None],
             [[0.2, 0.3, float("inf"), 4], [0.5, 0.6, -math.inf, 1], [0.5, 0.7, 0.25, 2]]]
    got = merge_moments(pairs, [0, -1, None, 3, 5], 5)
    assert got == [[3, 0.2, 0.4, 0.3, 1], [5, 0.5, 0.7, 0.25, 2]]
    # k larger than the candidate count: a short list; k = 0 and no pairs: empty
    assert len(merge_moments(pairs, [0, 1, 2, 3, 5], 50)) == 4
    assert merge_moments(pairs, [0, 1, 2, 3, 5], 0) == [] and merge_moments([], [], 3) == []
    assert merge_moments(pairs, [0, 1, 2, 3, 5], 1) == [[1, 0.1, 0.2, 0.9, 0]]


def test_host_merge_does_not_depend_on_the_chunks():
    """7 videos x 3 moments with planted ties, merged at once and through state in chunks of 1, 2, 3 and 7."""
    from drn_amd.metrics import merge_moments
    g = torch.Generator().manual_seed(0)
    scores = (torch.randint(0, 4, (7, 3), generator=g).float() / 4).tolist()          # four distinct values: ties everywhere
    pairs = [[[0.01 * v, 0.01 * v + 0.1 * (r + 1), scores[v][r], r if (v, r) != (2, 0) else -1] for r in range(3)] for v in range(7)]
    vids = [5, 3, 6, 0, 4, 1, 2]
    for k in (1, 4, 30):
        want = merge_moments(pairs, vids, k)
        assert len(want) == min(k, 20) and [w[3] for w in want] == sorted((w[3] for w in want), reverse=True)
        for chunk in (1, 2, 3, 7):
            state = None
            for c in range(0, 7, chunk):
                state = merge_moments(pairs[c:c + chunk], vids[c:c + chunk], k, state=state)
            assert state == want, (k, chunk)


# -- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_search_refuses_train_mode_host_tensors_and_a_host_store():
    from drn_amd import FeatureStore, Grounder, _lib
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, synthetic_batch
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1)))
    tok, qlen = synthetic_batch(2, 32, 64)[:2]
    videos = [("v%d" % v, torch.randn(8, 64), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64) for v in range(3)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    with pytest.raises(_lib.DrnError, match="eval"):
        Grounder(m.train()).search(tok, qlen, store)
    m.eval()
    with pytest.raises(_lib.DrnError, match="no CPU fallback"):
        Grounder(m).search(tok, qlen, store)                    # host tensors
    # stand-ins that only claim to live on the device: each later refusal answers before anything is read from them or launched
    import types
    dtok = types.SimpleNamespace(is_cuda=True, shape=(2, 8), device="cuda:0")
    for g in (Grounder(m), Grounder(m, graph=True)):
        with pytest.raises(_lib.DrnError, match="store on the GPU"):
            g.search(dtok, dtok, store)                         # a host store
    store.feats = types.SimpleNamespace(is_cuda=True, device="cuda:0")
    with pytest.raises(_lib.DrnError, match="per_video and top_k"):
        Grounder(m).search(dtok, dtok, store, per_video=0)
    with pytest.raises(_lib.DrnError, match="per_video and top_k"):
        Grounder(m).search(dtok, dtok, store, top_k=0)
    with pytest.raises(_lib.DrnError, match="no videos"):
        Grounder(m).search(dtok, dtok, store, videos=[])
    with pytest.raises(_lib.DrnError, match="outside"):
        Grounder(m).search(dtok, dtok, store, videos=[0, 3])
    with pytest.raises(_lib.DrnError, match="no video named"):
        Grounder(m).search(dtok, dtok, store, videos=["v1", "nobody"])
    store.dtype = torch.bfloat16
    with pytest.raises(_lib.DrnError, match="the store holds"):
        Grounder(m).search(dtok, dtok, store)
    assert m.fcos.box_selector_test.device_only is False
