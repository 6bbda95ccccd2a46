"""Host side of the corpus evaluator (drn_amd.search_eval): the twin metrics.search_first_hits on hand-written rows, recalls from its
tables for both kinds of column, search_batches on both kinds of loader, and the C-ABI boundary of drn_search_recall with the
refusals that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IOUS = (0.5, 0.7)


def first_hits(rows, gt_video, gt, K, ious=IOUS):
    from drn_amd.metrics import search_first_hits
    out = search_first_hits(rows, gt_video, gt, ious, K)
    assert out.shape == (len(rows), len(ious) + 1) and out.dtype == np.int32
    return out.tolist()


# -- the twin on hand-written rows --------------------------------------------------------------------------------------------------------

def test_a_tiou_exactly_at_the_threshold_counts():
    """(0, 0.5) against (0, 1): 0.5 / 1.0 == 0.5 in double, every value exact in float32."""
    assert first_hits([[[3, 0.0, 0.5, 0.9]]], [3], [[0.0, 1.0]], 4) == [[0, 4, 0]]
    assert first_hits([[[3, 0.0, 0.5, 0.9]]], [3], [[0.0, 1.0]], 4, ious=(0.5000000000000001,)) == [[4, 0]]


def test_the_right_moment_in_the_wrong_video_is_no_hit():
    rows = [[[2, 0.25, 0.75, 0.9], [3, 0.0, 0.125, 0.8]]]
    assert first_hits(rows, [3], [[0.25, 0.75]], 5) == [[5, 5, 1]]
    assert first_hits(rows, [2], [[0.25, 0.75]], 5) == [[0, 0, 0]]


def test_a_disjoint_moment_in_the_right_video_is_negative_and_no_hit():
    rows = [[[1, 0.0, 0.25, 0.9]]]
    assert first_hits(rows, [1], [[0.5, 1.0]], 3, ious=(0.5, 0.0, -0.1, -0.25, -0.26)) == [[3, 3, 3, 0, 0, 0]]       # (0.25 - 0.5) / 1


def test_no_rows_and_no_ground_truth_video_give_k_everywhere():
    rows = [[], [[0, 0.0, 1.0, 0.9]], [[0, 0.0, 1.0, 0.9]]]
    assert first_hits(rows, [0, -1, 4], [[0.0, 1.0]] * 3, 7) == [[7, 7, 7]] * 3


def test_a_videos_second_moment_does_not_push_other_videos_down():
    """Rows [A, A, B, gt]: the moment columns say 3, the video column 2."""
    rows = [[[8, 0.0, 0.5, 0.9], [8, 0.5, 1.0, 0.8], [5, 0.0, 1.0, 0.7], [1, 0.0, 1.0, 0.6], [1, 0.0, 0.875, 0.5]]]
    assert first_hits(rows, [1], [[0.0, 1.0]], 10) == [[3, 3, 2]]
    # the first row of the right video misses, the second hits: the video column stays where the video first appears
    rows = [[[8, 0.0, 0.5, 0.9], [1, 0.0, 0.125, 0.8], [8, 0.5, 1.0, 0.7], [4, 0.0, 1.0, 0.6], [1, 0.0, 0.625, 0.5], [1, 0.0, 0.75, 0.4]]]
    assert first_hits(rows, [1], [[0.0, 1.0]], 10) == [[4, 5, 1]]


def test_only_the_first_k_rows_are_read_and_nan_or_empty_pairs_are_no_hit():
    rows = [[[0, 0.0, 0.125, 0.9], [0, 0.0, 1.0, 0.8]]]
    assert first_hits(rows, [0], [[0.0, 1.0]], 1) == [[1, 1, 0]]
    assert first_hits(rows, [0], [[float("nan"), 1.0]], 2) == [[2, 2, 0]]
    assert first_hits(rows, [0], [[0.0, float("nan")]], 2) == [[2, 2, 0]]
    assert first_hits([[[0, 0.5, 0.5, 0.9]]], [0], [[0.5, 0.5]], 2, ious=(0.5, -1.0)) == [[2, 2, 0]]        # 0 / 0
    assert first_hits([[[0, 0.5, 0.5, 0.9]]], [0], [[1.0, 0.0]], 2, ious=(0.5, -1.0)) == [[2, 2, 0]]        # -1 / 0


def test_tensors_and_arrays_are_accepted_as_ground_truth():
    rows = [[[2, 0.0, 0.5, 0.9]], [[1, 0.25, 0.5, 0.9]]]
    want = first_hits(rows, [2, 1], [[0.0, 1.0], [0.25, 0.5]], 3)
    assert want == [[0, 3, 0], [0, 0, 0]]
    assert first_hits(rows, torch.tensor([2, 1], dtype=torch.int32), torch.tensor([[0.0, 1.0], [0.25, 0.5]]), 3) == want
    assert first_hits(rows, np.asarray([2, 1]), np.asarray([[0.0, 1.0], [0.25, 0.5]]), 3, ious=torch.tensor(IOUS, dtype=torch.float64)) == want


def test_recalls_from_a_twin_table_for_both_kinds_of_column():
    from drn_amd.metrics import recall_from_first_hits, search_first_hits
    rows = [[[8, 0.0, 0.5, 0.9], [8, 0.5, 1.0, 0.8], [5, 0.0, 1.0, 0.7], [1, 0.0, 1.0, 0.6]],      # moment 3, video 2
            [[1, 0.0, 0.625, 0.9]],                                                                 # 0.625: hits 0.5 only
            [[2, 0.0, 1.0, 0.9]],                                                                   # the wrong video
            []]
    fh = search_first_hits(rows, [1, 1, 1, 1], [[0.0, 1.0]] * 4, IOUS, 4)
    assert fh.tolist() == [[3, 3, 2], [0, 4, 0], [4, 4, 4], [4, 4, 4]]
    assert recall_from_first_hits(fh[:, :2], IOUS, (1, 3, 4)) == [0.25, 0.25, 0.5, 0.0, 0.0, 0.25]
    assert recall_from_first_hits(fh[:, 2:], IOUS[:1], (1, 3, 4)) == [0.25, 0.5, 0.5]


# -- search_batches ---------------------------------------------------------------------------------------------------------------------------

def test_search_batches_reads_host_batches_or_collate_tuples():
    from drn_amd import search_batches

    class FakeStoreLoader(object):
        def host_batches(self):
            for b in range(2):
                yield ["v%d" % b], "vids", "gt%d" % b, "tok%d" % b, "qlen%d" % b, "nprops", "nframes"

        def __iter__(self):
            raise AssertionError("a loader with host_batches() is not iterated: nothing is to be gathered")
    assert list(search_batches(FakeStoreLoader())) == [(["v0"], "tok0", "qlen0", "gt0"), (["v1"], "tok1", "qlen1", "gt1")]
    tuples = [(["a", "b"], "pse", "feats", "gt", "tok", "qlen", "nprops", "nframes")]
    assert list(search_batches(tuples)) == [(["a", "b"], "tok", "qlen", "gt")]
    assert list(search_batches([])) == []


def test_no_batches_give_an_empty_table_and_recalls_of_zero():
    import drn_amd
    from drn_amd import FeatureStore
    videos = [("v0", torch.randn(8, 16), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    res = drn_amd.evaluate_search(None, [], store, ious=(0.5, 0.7), topks=(1, 10))
    assert isinstance(res, drn_amd.SearchRecall)
    assert res.n == 0 and res.ious == [0.5, 0.7] and res.topks == [1, 10]
    assert res.moment == [0.0] * 4 and res.video == [0.0] * 2
    assert res.first_hits.shape == (0, 3) and res.first_hits.dtype == np.int32


def test_a_name_the_store_lacks_raises_before_the_search():
    from drn_amd import FeatureStore, _lib, evaluate_search

    class NoSearch(object):
        def search(self, *a, **kw):
            raise AssertionError("the batch was searched")
    videos = [("v0", torch.randn(8, 16), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    batch = (["v0", "nowhere"], torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 3]), torch.zeros(2, 2))
    with pytest.raises(_lib.DrnError, match="no video named nowhere"):
        evaluate_search(NoSearch(), [batch], store)


# -- the C-ABI boundary -------------------------------------------------------------------------------------------------------------------

def built_lib():
    from drn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_library_exports_search_recall_at_abi_9():
    import drn_amd
    from drn_amd import _lib, metrics, ops
    lib = built_lib()
    assert "drn_search_recall" in _lib.declared_symbols() and hasattr(lib, "drn_search_recall")
    assert lib.drn_abi_version() == 9
    assert callable(ops.search_recall) and callable(metrics.search_first_hits) and callable(drn_amd.evaluate_search)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drn_hip.h")).read(), flags=re.S)
    params = re.search(r"\bint\s+drn_search_recall\s*\(([^)]*)\)\s*;", txt).group(1).split(",")
    sig = _lib.SIGNATURES["drn_search_recall"]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(lib.drn_search_recall.argtypes) == list(sig)


def test_search_recall_argument_checks_answer_before_anything_is_launched():
    from drn_amd import _lib
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def call(S=2, K=4, I=2, ptrs=None):
        a = [p] * 7 if ptrs is None else ptrs            # seg video n gt_video gt | ious | first_hit
        return L.drn_search_recall(a[0], a[1], a[2], a[3], a[4], 0, a[5], S, K, I, a[6], None)
    for i in range(7):
        assert call(ptrs=[None if j == i else p for j in range(7)]) != 0, i
        assert b"null pointer" in L.drn_last_error()
    assert call(S=0) != 0 and b"S = 0" in L.drn_last_error()
    assert call(K=0) != 0 and b"K = 0" in L.drn_last_error()
    assert call(K=-3) != 0 and b"K = -3" in L.drn_last_error()
    assert call(I=0) != 0 and b"I = 0" in L.drn_last_error()
    cap = _lib.MERGE_MAX_CAND
    assert call(K=cap + 1) != 0 and (b"K = %d hit slots per sentence (max %d)" % (cap + 1, cap)) in L.drn_last_error()


def test_ops_search_recall_refuses_host_tensors():
    from drn_amd import _lib, ops
    from drn_amd.grounding import Hits
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    hits = Hits(torch.zeros(2, 3, 2), torch.zeros(2, 3), z(2, 3), z(2, 3), z(2, 3), z(2))
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.search_recall(hits, z(2), torch.zeros(2, 2), torch.tensor([0.5], dtype=torch.float64))
