"""Host side of the search over per-sentence candidate lists (Grounder.search(candidates=), Grounder.ground_stored): the planner
plan_pairs on random ragged inputs, the C-ABI boundary of drn_merge_moments_ragged, and the refusals that need no GPU."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("vids", "pair_q", "pair_v", "pair_video", "pair_off")


def ragged(seed, Nv):
    """Six to nine sentences over Nv videos: an empty list, a list with duplicates, one sentence listing every video (shuffled),
    the rest random subsets in random order."""
    g = np.random.RandomState(seed)
    lists = [[], [3, 1, 3, 3, 1, 0], [int(v) for v in g.permutation(Nv)]]
    for _ in range(g.randint(3, 7)):
        lists.append([int(v) for v in g.choice(Nv, size=g.randint(1, Nv + 1), replace=g.rand() < 0.5)])
    order = g.permutation(len(lists))
    return [lists[i] for i in order]


def check_plan(plan, lists, Nv, pairs, slots, cap):
    S = len(lists)
    want = {(s, v) for s, l in enumerate(lists) for v in l}
    C = plan.vids.shape[0]
    assert [getattr(plan, f).dtype for f in FIELDS] == [np.int32] * 5
    assert plan.vids.shape == (C, slots) and plan.pair_off.shape == (C, S + 1)                  # all chunks have one shape
    assert plan.pair_q.shape == plan.pair_v.shape == plan.pair_video.shape == (C, pairs)
    seen = []
    for c in range(C):
        vids, pq, pv, pvideo, off = (getattr(plan, f)[c] for f in FIELDS)
        assert off[0] == 0 and (np.diff(off) >= 0).all()
        m = int(off[S])
        assert 1 <= m <= pairs
        assert int(np.diff(off).max()) <= cap
        real = vids[vids >= 0]
        assert 1 <= real.size <= slots and (vids[real.size:] == -1).all() and np.unique(real).size == real.size
        for s in range(S):
            assert (pq[off[s]:off[s + 1]] == s).all()
        assert (vids[pv[:m]] == pvideo[:m]).all() and (pvideo[:m] >= 0).all() and (pvideo[:m] < Nv).all()
        assert set(pvideo[:m].tolist()) == set(real.tolist())                                   # no slot without a pair
        assert (pvideo[m:] == -1).all()                                                         # padded pairs: past pair_off[S], video -1,
        assert ((pq[m:] >= 0) & (pq[m:] < S)).all() and ((pv[m:] >= 0) & (pv[m:] < slots)).all()   # sentence and slot in range
        seen += list(zip(pq[:m].tolist(), pvideo[:m].tolist()))
    assert len(seen) == len(set(seen)) == len(want) and set(seen) == want                       # every distinct pair exactly once
    return C


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_plan_pairs_on_random_ragged_lists(seed):
    from drn_amd.grounding import plan_pairs
    Nv = 9 + seed
    lists = ragged(seed, Nv)
    total = len({(s, v) for s, l in enumerate(lists) for v in l})
    for pairs, slots, cap in ((1, 1, 1), (1, 4, 3), (5, 1, 5), (7, 3, 1), (6, 4, 2), (512, Nv, 1000), (total, Nv, Nv)):
        plan = plan_pairs(lists, Nv, pairs, slots, cap)
        C = check_plan(plan, lists, Nv, pairs, slots, cap)
        if pairs == 1:
            assert C == total
        if (pairs, slots, cap) == (total, Nv, Nv):
            assert C == 1 and int(plan.pair_off[0, -1]) == total                                # nothing forces a cut
        again = plan_pairs([list(l) for l in lists], Nv, pairs, slots, cap)                     # deterministic
        for f in FIELDS:
            assert np.array_equal(getattr(plan, f), getattr(again, f)), f
        # the CSR pair and host tensors name the same lists
        ids = np.asarray([v for l in lists for v in l], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
        for form in ((ids, off), (torch.from_numpy(ids).int(), torch.from_numpy(off)), [torch.tensor(l, dtype=torch.int32) for l in lists]):
            other = plan_pairs(form, Nv, pairs, slots, cap)
            for f in FIELDS:
                assert np.array_equal(getattr(plan, f), getattr(other, f)), f


def test_plan_pairs_orders_by_video_then_sorts_a_chunk_by_sentence():
    """Three sentences over videos {0, 2}, {2}, {0, 1, 2} at 3 pairs per chunk: (video, sentence) order is (0,0) (0,2) (1,2) | (2,0)
    (2,1) (2,2); inside chunk 0 the pairs are then grouped by sentence."""
    from drn_amd.grounding import plan_pairs
    plan = plan_pairs([[2, 0], [2], [0, 1, 2]], 3, 3, 3, 9)
    assert plan.vids.tolist() == [[0, 1, -1], [2, -1, -1]]
    assert plan.pair_q.tolist() == [[0, 2, 2], [0, 1, 2]] and plan.pair_video.tolist() == [[0, 0, 1], [2, 2, 2]]
    assert plan.pair_v.tolist() == [[0, 0, 1], [0, 0, 0]] and plan.pair_off.tolist() == [[0, 1, 1, 3], [0, 1, 2, 3]]
    # two slots per chunk cut where the third video would come in; the last chunk is padded
    plan = plan_pairs([[2, 0], [2], [0, 1, 2]], 3, 4, 2, 9)
    assert plan.vids.tolist() == [[0, 1], [2, -1]] and plan.pair_off[:, -1].tolist() == [3, 3]
    assert plan.pair_video.tolist() == [[0, 0, 1, -1], [2, 2, 2, -1]]
    # cap = 1: sentence 2 may appear once per chunk -- (0,0) (0,2) | (1,2) (2,0) (2,1) | (2,2)
    plan = plan_pairs([[2, 0], [2], [0, 1, 2]], 3, 4, 3, 1)
    assert plan.pair_off[:, -1].tolist() == [2, 3, 1] and int(np.diff(plan.pair_off, axis=1).max()) == 1


def test_plan_pairs_without_pairs_and_refusals():
    from drn_amd import _lib
    from drn_amd.grounding import plan_pairs
    plan = plan_pairs([[], [], []], 5, 4, 2, 3)
    assert plan.vids.shape == (0, 2) and plan.pair_q.shape == (0, 4) and plan.pair_off.shape == (0, 4)
    for bad in ([[0, 5]], [[-1]], (np.asarray([7]), np.asarray([0, 1]))):
        with pytest.raises(_lib.DrnError, match="outside"):
            plan_pairs(bad, 5, 4, 2, 3)
    for pairs, slots, cap in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(_lib.DrnError, match="at least 1"):
            plan_pairs([[0]], 5, pairs, slots, cap)
    with pytest.raises(_lib.DrnError, match="offsets"):
        plan_pairs((np.asarray([0, 1]), np.asarray([0, 3])), 5, 4, 2, 3)
    with pytest.raises(_lib.DrnError, match="ids_of"):
        plan_pairs([["vid0"]], 5, 4, 2, 3)


# -- the C-ABI boundary -----------------------------------------------------------------------------------------------------------------

def test_library_exports_merge_moments_ragged_at_abi_9():
    import drn_amd
    from drn_amd import _lib, grounding, ops
    lib = built_lib()
    assert "drn_merge_moments_ragged" in _lib.declared_symbols() and hasattr(lib, "drn_merge_moments_ragged")
    assert lib.drn_abi_version() == 9
    assert callable(ops.merge_moments_ragged) and callable(grounding.plan_pairs) and callable(drn_amd.Grounder.ground_stored)
    params = _header_params("drn_merge_moments_ragged")
    sig = _lib.SIGNATURES["drn_merge_moments_ragged"]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(lib.drn_merge_moments_ragged.argtypes) == list(sig)


def test_ragged_argument_checks_answer_before_anything_is_launched():
    from drn_amd import _lib
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def call(S=2, P=6, kv=2, K=4, ptrs=None):
        a = [p] * 13 if ptrs is None else ptrs    # seg score level index n | pair_video pair_off | st_seg st_score st_video st_level st_rank st_n
        return L.drn_merge_moments_ragged(a[0], a[1], a[2], a[3], a[4], S, P, kv, a[5], a[6], 5, K, 1, None, *a[7:], None)
    for i in range(13):
        assert call(ptrs=[None if j == i else p for j in range(13)]) != 0, i
        assert b"null pointer" in L.drn_last_error()
    assert call(K=0) != 0 and b"K = 0" in L.drn_last_error()
    assert call(kv=0) != 0 and b"kv = 0" in L.drn_last_error()
    assert call(S=0) != 0 and call(P=0) != 0 and call(S=-1) != 0
    cap = _lib.MERGE_MAX_CAND
    assert call(K=cap - 1, kv=2) != 0 and (b"%d candidates for one pair (max %d)" % (cap + 1, cap)) in L.drn_last_error()
    assert call(K=1 << 30, kv=1 << 30) != 0 and b"candidates for one pair" in L.drn_last_error()          # (no int overflow)
    assert call(P=1 << 30, kv=4) != 0 and b"2^31" in L.drn_last_error()


# -- refusals of the public interface -----------------------------------------------------------------------------------------------------

def test_search_with_candidates_refuses_before_touching_a_gpu():
    from drn_amd import FeatureStore, Grounder, _lib
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1))).eval()
    videos = [("v%d" % v, torch.randn(8, 64), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64) for v in range(3)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    # stand-ins that only claim to live on the device (as in tests/test_search_cpu.py): each refusal answers before anything is read
    dtok = types.SimpleNamespace(is_cuda=True, shape=(2, 8), device="cuda:0")
    store.feats = types.SimpleNamespace(is_cuda=True, device="cuda:0")
    for g in (Grounder(m), Grounder(m, graph=True)):
        with pytest.raises(_lib.DrnError, match="exclude each other"):
            g.search(dtok, dtok, store, candidates=[[0], [1]], videos=[0, 1])
        with pytest.raises(_lib.DrnError, match="3 candidate lists for 2 sentences"):
            g.search(dtok, dtok, store, candidates=[[0], [1], [2]])
        with pytest.raises(_lib.DrnError, match="outside"):
            g.search(dtok, dtok, store, candidates=[[0, 3], [1]])
        with pytest.raises(_lib.DrnError, match="no video named"):
            g.search(dtok, dtok, store, candidates=[["v0"], ["nobody"]])
        with pytest.raises(_lib.DrnError, match="exceeds"):
            g.search(dtok, dtok, store, candidates=[[0], [1]], top_k=_lib.MERGE_MAX_CAND, per_video=1)      # cap < 1
        with pytest.raises(_lib.DrnError, match="pairs and chunk"):
            g.search(dtok, dtok, store, candidates=[[0], [1]], pairs=0)
        with pytest.raises(_lib.DrnError, match="pairs= is the step size"):
            g.search(dtok, dtok, store, pairs=4)
        with pytest.raises(_lib.DrnError, match="3 videos for 2 sentences"):
            g.ground_stored(dtok, dtok, store, ["v0", "v1", "v2"])
        with pytest.raises(_lib.DrnError, match="outside"):
            g.ground_stored(dtok, dtok, store, [0, 3])
    with pytest.raises(_lib.DrnError, match="no CPU fallback"):
        Grounder(m).ground_stored(torch.zeros(2, 8, dtype=torch.long), torch.tensor([8, 8]), store, [0, 1])
    with pytest.raises(_lib.DrnError, match="eval"):
        Grounder(m.train()).ground_stored(dtok, dtok, store, [0, 1])
    assert m.fcos.box_selector_test.device_only is False
