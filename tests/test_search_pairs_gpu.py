"""Search over per-sentence candidate lists on the device: drn_merge_moments_ragged against the host twin (metrics.merge_moments,
exact equality of every field), Grounder.search(candidates=) against the search without candidates -- all videos for every sentence,
and ragged lists against the union's full ranking filtered on the host -- on a store and on an index, eagerly and by graph replay, and
Grounder.ground_stored against Grounder.ground.  No tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV, dev_batch, tiny_model
from test_search_gpu import D, NV, S, STATE, T, boosted, check_state, garbage_state, on_device, planted, same_hits, sentences, small_store

pytestmark = pytest.mark.gpu
MOMENT = ("seg", "score", "level", "index", "n")


# -- 1. drn_merge_moments_ragged against the host twin ----------------------------------------------------------------------------------

def i32(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=DEV)


def ragged_twin(chunks, S_, K, Nv):
    """metrics.merge_moments over `chunks` = [(arrays, pair_video, pair_off), ...] streamed through its state: sentence s is given the
    pairs [pair_off[s], pair_off[s + 1]) of each chunk and nothing else -> (lists, levels) as test_search_gpu.twin."""
    from drn_amd.metrics import merge_moments
    lists, levels = [], []
    for s in range(S_):
        state, lv = None, {}
        for (seg, score, level, index, n), pvideo, off in chunks:
            mine = range(off[s], off[s + 1])
            pairs = [[[float(seg[p, r, 0]), float(seg[p, r, 1]), float(score[p, r]), int(index[p, r])] for r in range(n[p])] for p in mine]
            for p in mine:
                for r in range(n[p]):
                    lv[(pvideo[p], r)] = int(level[p, r])
            state = merge_moments(pairs, [pvideo[p] if 0 <= pvideo[p] < Nv else None for p in mine], K, state=state)
        lists.append(state)
        levels.append(lv)
    return lists, levels


def ragged_case(counts, kv, seed, padded=3):
    """One chunk: sentence s owns counts[s] pairs, `padded` more follow pair_off[S].  The entries are planted(): score ties, n = 0
    pairs, fallback moments, NaN / +-Inf scores, winning scores past n[p].  Every sentence's videos are distinct positions of a store
    of Nv = P + 3 videos; where a sentence has more than four pairs, two of them carry the positions -1 and Nv.  The padded pairs
    carry winning scores and positions INSIDE the store: only their place past pair_off[S] keeps them out."""
    g = np.random.RandomState(seed)
    real = int(sum(counts))
    P = real + padded
    Nv = P + 3
    arrays = planted(1, P, kv, seed)
    off = [0] + [int(x) for x in np.cumsum(counts)]
    pvideo = []
    for c in counts:
        v = [int(x) for x in g.permutation(Nv)[:c]]
        if c > 4:
            v[1], v[-2] = -1, Nv
        pvideo += v
    pvideo += [int(x) for x in g.randint(0, Nv, padded)]
    seg, score, level, index, n = arrays
    for p in range(real, P):
        n[p], score[p], index[p] = kv, 50.0, 7
    return arrays, pvideo, off, Nv


@pytest.mark.parametrize("counts,kv,K", [((0, 1, 40), 2, 4), ((40, 12), 3, 70), ((3, 0), 2, 10), ((1,), 1, 1)])
def test_ragged_merge_equals_the_host_twin(counts, kv, K):
    """(0, 1, 40), kv = 2, K = 4: 84 staged candidates, past one 64-lane stride, beside an empty sentence and a one-pair one;
    K = 70 over 40 pairs of 3 slots: the output slots cross a stride; K = 10 above the number of candidates; the smallest problem."""
    from drn_amd import ops
    arrays, pvideo, off, Nv = ragged_case(counts, kv, seed=K, padded=0 if K == 1 else 3)
    lists, levels = ragged_twin([(arrays, pvideo, off)], len(counts), K, Nv)
    assert all(0 <= w[0] < Nv and np.isfinite(w[3]) and w[3] <= 1.0 for want in lists for w in want)      # (no padded pair's 50.0)
    if counts == (0, 1, 40):
        assert lists[0] == [] and len(lists[2]) == K
    if K == 70:
        assert len(lists[0]) == K > 64 and len(lists[1]) < K
        assert any(a[3] == b[3] and a[0] != b[0] for a, b in zip(lists[0], lists[0][1:]))      # ties across videos ...
        assert any(a[3] == b[3] and a[0] == b[0] for a, b in zip(lists[0], lists[0][1:]))      # ... and inside a pair
    if K == 10:
        assert 0 < len(lists[0]) < K and lists[1] == []
    if K == 1:
        assert arrays[0].shape[0] == 1
    state = ops.merge_moments_ragged(on_device(arrays), i32(pvideo), i32(off), Nv, garbage_state(len(counts), K), True)
    check_state(state, lists, levels, K)


@pytest.mark.parametrize("device_flag", [False, True])
def test_a_sentence_absent_from_a_chunk(device_flag):
    """Two chunks streamed.  Chunk 1 has pairs of sentences 0 and 1 only and enters on a garbage state with first != 0: sentence 2 comes
    out empty with clean tails.  Chunk 2 has pairs of sentences 1 and 2 only: sentence 0's state bytes do not change."""
    from drn_amd import ops
    kv, K = 2, 6
    a, va, oa, half = ragged_case((5, 4, 0), kv, seed=21)
    b, vb, ob, _ = ragged_case((0, 3, 6), kv, seed=22)
    # one store of twice the videos: chunk 1 takes its pairs from the lower half and chunk 2 from the upper, so that no (sentence,
    # video) pair comes twice -- as in a plan; -1 stays -1 and `half` (one past a case's store) becomes one past this store
    Nv = 2 * half
    va = [v if v < half else Nv for v in va]
    vb = [v + half if 0 <= v < half else (v if v < 0 else Nv) for v in vb]
    assert Nv in va and -1 in va and Nv in vb and -1 in vb
    flag = (lambda f: torch.tensor([int(f)], dtype=torch.int32, device=DEV)) if device_flag else (lambda f: f)
    state = ops.merge_moments_ragged(on_device(a), i32(va), i32(oa), Nv, garbage_state(3, K), flag(True))
    lists, levels = ragged_twin([(a, va, oa)], 3, K, Nv)
    assert lists[2] == [] and len(lists[0]) > 0
    check_state(state, lists, levels, K)
    kept = [t[0].clone() for t in state[:5]] + [state[5][:1].clone()]
    ops.merge_moments_ragged(on_device(b), i32(vb), i32(ob), Nv, state, flag(False))
    lists, levels = ragged_twin([(a, va, oa), (b, vb, ob)], 3, K, Nv)
    assert len(lists[2]) > 0
    check_state(state, lists, levels, K)
    for t, was in zip(state, kept):
        assert t[:1].reshape(was.shape).cpu().numpy().tobytes() == was.cpu().numpy().tobytes()


def test_the_same_pairs_cut_in_two_ways_give_one_state():
    """The pairs of four ragged lists through plan_pairs at (pairs, slots, cap) = (all, all, all) -- one chunk -- and at (5, 2, 3):
    the same state, which is the twin's."""
    from drn_amd import ops
    from drn_amd.grounding import plan_pairs
    kv, K, Nv = 2, 7, 9
    lists_in = [[0, 3, 4, 8, 1, 6, 7], [], [4], [8, 2, 3, 4, 5]]
    S_ = len(lists_in)
    pool = planted(1, 40, kv, seed=5)                                  # row of pair (s, v): s * Nv + v
    row = lambda s, v: s * Nv + v
    states = []
    for pairs, slots, cap in ((13, Nv, 13), (5, 2, 3)):
        plan = plan_pairs(lists_in, Nv, pairs, slots, cap)
        state, chunks = garbage_state(S_, K), []
        for c in range(plan.vids.shape[0]):
            pq, pvideo, off = plan.pair_q[c], plan.pair_video[c], plan.pair_off[c]
            rows = [row(int(q), int(v)) if v >= 0 else 37 for q, v in zip(pq, pvideo)]      # (row 37: what a padded pair computes)
            arrays = tuple(f[rows].copy() for f in pool)
            chunks.append((arrays, pvideo.tolist(), off.tolist()))
            ops.merge_moments_ragged(on_device(arrays), i32(pvideo), i32(off), Nv, state, c == 0)
        want, levels = ragged_twin(chunks, S_, K, Nv)
        check_state(state, want, levels, K)
        states.append(state)
    assert plan.vids.shape[0] > 2
    for x, y in zip(*states):
        assert torch.equal(x, y)


def test_ragged_merge_refuses_what_does_not_fit():
    from drn_amd import _lib, ops
    arrays, pvideo, off, Nv = ragged_case((2, 1), 2, seed=0)
    dev = on_device(arrays)
    with pytest.raises(_lib.DrnError, match="candidates for one pair"):
        ops.merge_moments_ragged(dev, i32(pvideo), i32(off), Nv, ops.merge_state(2, _lib.MERGE_MAX_CAND - 1, DEV), True)
    with pytest.raises(_lib.DrnError, match="pair_off"):
        ops.merge_moments_ragged(dev, i32(pvideo), i32(off + [6]), Nv, ops.merge_state(2, 4, DEV), True)
    with pytest.raises(_lib.DrnError, match="pair_video"):
        ops.merge_moments_ragged(dev, i32(pvideo[:-1]), i32(off), Nv, ops.merge_state(2, 4, DEV), True)
    with pytest.raises(_lib.DrnError):
        ops.merge_moments_ragged(dev, i32(pvideo).cpu(), i32(off), Nv, ops.merge_state(2, 4, DEV), True)


# -- 2. end to end, on a store and on an index built from it --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared():
    """The boosted tiny fp32 model, small_store(), its index, two sets of sentences: built once, changed by no test."""
    from drn_amd import SearchIndex
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    return m, {"store": store, "index": SearchIndex.build(m, store)}, sentences(7), sentences(11)


RAGGED = [[5, 0, 6, 2], [], ["vid3"]]
OTHER = [[1], [4, "vid3", 6, 0], [2, 2]]          # other lists: the same signature at the same pairs, chunk and T


def filtered(full, lists, store, K):
    """The oracle: `full` = the Hits of every sentence against the union with top_k large enough to keep every entry, cut on the host
    to each sentence's own candidates and to K -> per sentence the kept positions in `full`."""
    n, video = full.n.tolist(), full.video.cpu().numpy()
    keep = []
    for s, l in enumerate(lists):
        mine = set(store.ids_of(l).tolist())
        keep.append([i for i in range(n[s]) if int(video[s, i]) in mine][:K])
    return keep


def check_against(hits, full, keep, K, what):
    got = {f: getattr(hits, f).cpu().numpy() for f in STATE}
    want = {f: getattr(full, f).cpu().numpy() for f in STATE}
    for s, rows in enumerate(keep):
        m = len(rows)
        assert int(got["n"][s]) == m, (what, s, int(got["n"][s]), m)
        for f in STATE[:5]:
            assert got[f][s, :m].tobytes() == want[f][s, rows].tobytes(), (what, s, f)
            assert (got[f][s, m:] == (0 if f in ("seg", "score") else -1)).all(), (what, s, f)


@pytest.mark.parametrize("where", ["store", "index"])
def test_every_video_for_every_sentence_is_the_search_without_candidates(where):
    from drn_amd import Grounder, search
    m, stores, (tok, qlen), _ = shared()
    grounder, st = Grounder(m, top_k=6), stores[where]
    want = grounder.search(tok, qlen, st, per_video=2)
    assert int(want.n.min()) == 6
    everything = [list(range(NV))] * S
    same_hits(grounder.search(tok, qlen, st, per_video=2, candidates=everything), want, "default shape")
    same_hits(grounder.search(tok, qlen, st, per_video=2, candidates=[list(st.names)] * S, pairs=5, chunk=2), want, "by name, small steps")
    csr = (np.tile(np.arange(NV), S), np.arange(S + 1) * NV)
    same_hits(search(m, tok, qlen, st, top_k=6, per_video=2, candidates=csr, pairs=4), want, "module-level search, CSR")
    assert m.fcos.box_selector_test.device_only is False


@pytest.mark.parametrize("where", ["store", "index"])
@pytest.mark.parametrize("per_video,K", [(1, 3), (2, 5)])
def test_ragged_lists_equal_the_unions_ranking_filtered(where, per_video, K):
    """Lists of four videos, none and one (by name).  The union's search keeps every entry (top_k = 7 x per_video); the order is
    total, so a sentence's own ranking is that list filtered.  Identical for pairs in {1, 3, default} and for a video-slot limit that
    cuts chunks; lists that name nothing give n = 0."""
    from drn_amd import Grounder
    m, stores, (tok, qlen), _ = shared()
    grounder, st = Grounder(m, top_k=K), stores[where]
    full = grounder.search(tok, qlen, st, top_k=NV * per_video, per_video=per_video, videos=[0, 2, 3, 5, 6])
    keep = filtered(full, RAGGED, st, K)
    assert len(keep[0]) == K and keep[1] == [] and 1 <= len(keep[2]) <= per_video
    for kw in (dict(pairs=1), dict(pairs=3), dict(), dict(chunk=2), dict(pairs=4, chunk=1), dict(T=32)):
        check_against(grounder.search(tok, qlen, st, per_video=per_video, candidates=RAGGED, **kw), full, keep, K, kw)
    dup = [[5, 0, 6, 2, 5, 5, 0], [], [3, "vid3"]]
    check_against(grounder.search(tok, qlen, st, per_video=per_video, candidates=dup), full, keep, K, "duplicates")
    nothing = grounder.search(tok, qlen, st, per_video=per_video, candidates=[[], [], []])
    check_against(nothing, full, [[], [], []], K, "no pairs at all")


@pytest.mark.parametrize("where", ["store", "index"])
def test_candidates_by_graph_replay(where):
    """graph=True == eager; other lists and other sentences of the same signature replay the same graph."""
    from drn_amd import Grounder
    m, stores, (tok, qlen), (tok2, qlen2) = shared()
    st = stores[where]
    eager, graphed = Grounder(m, top_k=5), Grounder(m, top_k=5, graph=True)
    kw = dict(per_video=2, pairs=4, chunk=3, T=T)
    first = graphed.search(tok, qlen, st, candidates=RAGGED, **kw)
    same_hits(first, eager.search(tok, qlen, st, candidates=RAGGED, **kw), "first call")
    assert graphed.captures == 1 and int(first.n[0]) == 5 and int(first.n[1]) == 0
    kept = first.score.clone()
    second = graphed.search(tok2, qlen2, st, candidates=OTHER, **kw)
    same_hits(second, eager.search(tok2, qlen2, st, candidates=OTHER, **kw), "other lists, other sentences")
    assert graphed.captures == 1 and torch.equal(first.score, kept) and not torch.equal(second.score, first.score)
    full = eager.search(tok2, qlen2, st, top_k=NV * 2, per_video=2)
    check_against(second, full, filtered(full, OTHER, st, 5), 5, "replayed")
    # the search without candidates is another signature, and is not disturbed
    same_hits(graphed.search(tok, qlen, st, per_video=2, chunk=3), eager.search(tok, qlen, st, per_video=2, chunk=3), "cartesian")
    assert graphed.captures == 2
    same_hits(graphed.search(tok, qlen, st, candidates=RAGGED, **kw), first, "again")
    assert graphed.captures == 2 and m.fcos.box_selector_test.device_only is False


@pytest.mark.parametrize("where", ["store", "index"])
def test_ground_stored_equals_ground(where):
    """Five sentences, vid4 named by two of them, in steps of 2 pairs (the last step has a padded pair), of 1, of 3, in one step and
    in one step of 8 (three padded pairs): every Moments field equal to ground()'s on the gathered features.  vid5 has one proposal."""
    from drn_amd import Grounder, group_by_video
    m, stores, _, _ = shared()
    st, store = stores[where], stores["store"]
    tok, qlen = dev_batch(5, T, D, 13)[:2]
    videos = ["vid4", "vid1", "vid4", "vid5", "vid3"]
    unique, video_index = group_by_video(videos)
    for model in (m, tiny_model(T, D, torch.float32)) if where == "store" else (m,):       # (the plain classifier: fallback moments)
        grounder = Grounder(model, top_k=4)
        Tmax = int(store.nprops[store.ids_of(unique).numpy()].max())
        feats, pse, _ = store.gather(unique, T=Tmax)
        want = grounder.ground(tok, qlen, feats, pse, video_index)
        for kw in (dict(pairs=2), dict(pairs=1), dict(pairs=3), dict(), dict(pairs=8)):
            got = grounder.ground_stored(tok, qlen, st, videos, **kw)
            for f in MOMENT:
                assert torch.equal(getattr(got, f), getattr(want, f)), (kw, f)
            assert tuple(got.seg.shape) == (5, 4, 2) and len(got) == 5
        by_position = grounder.ground_stored(tok, qlen, st, [4, 1, 4, 5, 3], pairs=2)
        for f in MOMENT:
            assert torch.equal(getattr(by_position, f), getattr(want, f)), f
    assert m.fcos.box_selector_test.device_only is False


def test_refusals_come_before_any_launch():
    from drn_amd import Grounder, SearchIndex, _lib, ops
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    tok, qlen = sentences(7)
    index = SearchIndex.build(m, store)
    with torch.no_grad():
        m.prop_fc.bias.add_(0.1)
    ops.kernel_timer = []
    try:
        for g in (Grounder(m, top_k=6), Grounder(m, top_k=6, graph=True)):
            with pytest.raises(_lib.DrnError, match="stale"):
                g.search(tok, qlen, index, per_video=2, candidates=RAGGED)
            with pytest.raises(_lib.DrnError, match="stale"):
                g.ground_stored(tok, qlen, index, [0, 1, 2])
            for st in (store, index):
                with pytest.raises(_lib.DrnError, match="exclude each other"):
                    g.search(tok, qlen, st, candidates=RAGGED, videos=[0, 1])
            with pytest.raises(_lib.DrnError, match="2 candidate lists for 3 sentences"):
                g.search(tok, qlen, store, candidates=RAGGED[:2])
            with pytest.raises(_lib.DrnError, match="outside"):
                g.search(tok, qlen, store, candidates=[[0], [NV], [1]])
        launches = len(ops.kernel_timer)
    finally:
        ops.kernel_timer = None
    assert launches == 0
