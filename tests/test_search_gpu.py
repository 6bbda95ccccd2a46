"""Search across the videos of a store on the device (Grounder.search): drn_merge_moments against its host twin
(metrics.merge_moments, pinned by tests/test_search_cpu.py) with exact equality of every field, forward_heads_shared's gates= /
query_index= keywords against gate rows expanded by hand, and the search end to end -- against the twin on per-pair moments, across
chunk sizes, by graph replay, and on the committed mini dataset against Grounder.ground."""
import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV, dev_batch, tiny_model

pytestmark = pytest.mark.gpu
STATE = ("seg", "score", "video", "level", "rank", "n")


# -- 1. drn_merge_moments against the host twin -----------------------------------------------------------------------------------------

def planted(S, Vc, kv, seed):
    """One chunk's select_moments outputs as numpy arrays, planted: scores from eight values (ties across videos and inside pairs),
    pairs 3, 26, ... without an entry (n = 0), pairs 2, 31, ... the fallback moment, pairs 4, 35, ... with a NaN / +-Inf score, one
    pair in ten with fewer entries than slots, and past n[p] entries that would win if they were read (score 9)."""
    g = np.random.RandomState(seed)
    P = S * Vc
    seg = np.sort(g.rand(P, kv, 2).astype(np.float32), axis=2)
    score = (g.randint(1, 9, (P, kv)) / 8.0).astype(np.float32)
    level = g.randint(0, 3, (P, kv)).astype(np.int32)
    index = g.randint(0, 500, (P, kv)).astype(np.int32)
    n = np.where(g.rand(P) < 0.1, g.randint(1, kv + 1, (P,)), kv).astype(np.int32)
    for p in range(P):
        if p % 23 == 3:
            n[p] = 0
        elif p % 29 == 2:
            n[p], seg[p, 0], score[p, 0], level[p, 0], index[p, 0] = 1, (0.0, 1.0), 1.0, -1, -1
        elif p % 31 == 4:
            score[p, 0] = (np.nan, np.inf, -np.inf)[p % 3]
        score[p, n[p]:], index[p, n[p]:] = 9.0, 5
    return seg, score, level, index, n


def twin(chunks, S, K, Nv):
    """metrics.merge_moments over `chunks` = [(arrays, vids), ...] streamed through its state -> per sentence the records
    [video, start, end, score, rank] and {(video, rank): level}."""
    from drn_amd.metrics import merge_moments
    lists, levels = [], []
    for s in range(S):
        state, lv = None, {}
        for (seg, score, level, index, n), vids in chunks:
            Vc, pairs = len(vids), []
            for slot in range(Vc):
                p = s * Vc + slot
                pairs.append([[float(seg[p, r, 0]), float(seg[p, r, 1]), float(score[p, r]), int(index[p, r])] for r in range(n[p])])
                for r in range(n[p]):
                    lv[(vids[slot], r)] = int(level[p, r])
            state = merge_moments(pairs, [v if 0 <= v < Nv else None for v in vids], K, state=state)
        lists.append(state)
        levels.append(lv)
    return lists, levels


def check_state(state, lists, levels, K):
    """Exact equality of every field: n; video, rank, level and the bits of seg and score of the first n entries; 0 / -1 past them."""
    seg, score, video, level, rank, n = (t.cpu().numpy() for t in state)
    assert seg.dtype == score.dtype == np.float32 and video.dtype == level.dtype == rank.dtype == n.dtype == np.int32
    assert seg.shape == (len(lists), K, 2)
    for s, want in enumerate(lists):
        m = len(want)
        assert int(n[s]) == m, (s, int(n[s]), m)
        assert video[s, :m].tolist() == [w[0] for w in want] and rank[s, :m].tolist() == [w[4] for w in want], (s, video[s], rank[s], want)
        assert seg[s, :m].tobytes() == np.asarray([w[1:3] for w in want], dtype=np.float32).reshape(m, 2).tobytes(), s
        assert score[s, :m].tobytes() == np.asarray([w[3] for w in want], dtype=np.float32).tobytes(), s
        assert level[s, :m].tolist() == [levels[s][(w[0], w[4])] for w in want], s
        assert not seg[s, m:].any() and not score[s, m:].any(), s
        assert (video[s, m:] == -1).all() and (level[s, m:] == -1).all() and (rank[s, m:] == -1).all(), s


def garbage_state(S, K):
    """A state nobody wrote: NaN scores, videos and ranks that would sort first, more entries than slots."""
    from drn_amd import ops
    state = ops.merge_state(S, K, DEV)
    state[0].fill_(float("nan")); state[1].fill_(float("inf")); state[2].fill_(0); state[3].fill_(7); state[4].fill_(0); state[5].fill_(1000)
    return state


def on_device(arrays):
    return tuple(torch.from_numpy(a).to(DEV) for a in arrays)


def dev_vids(vids):
    return torch.tensor(vids, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("S,Vc,kv,K", [(3, 5, 2, 4), (1, 1, 1, 1), (2, 40, 2, 70), (2, 3, 2, 10)])
def test_merge_moments_equals_the_host_twin(S, Vc, kv, K):
    """(2, 40, 2, 70): 150 staged candidates and 70 output slots, both past one 64-lane stride; (2, 3, 2, 10): K above the number of
    candidates.  The store has Nv = Vc + 3 videos; two slots of the chunk are out of it (-1 and Nv) when it has more than two."""
    from drn_amd import ops
    Nv = Vc + 3
    vids = list(np.random.RandomState(Vc).permutation(Nv)[:Vc])
    if Vc > 2:
        vids[1], vids[-1] = -1, Nv
    vids = [int(v) for v in vids]
    arrays = planted(S, Vc, kv, seed=K)
    lists, levels = twin([(arrays, vids)], S, K, Nv)
    assert all(0 <= w[0] < Nv and np.isfinite(w[3]) for want in lists for w in want)
    if Vc == 40:
        assert max(len(want) for want in lists) > 64 and min(len(want) for want in lists) < K
        assert any(a[3] == b[3] and a[0] != b[0] for want in lists for a, b in zip(want, want[1:]))      # ties across videos ...
        assert any(a[3] == b[3] and a[0] == b[0] for want in lists for a, b in zip(want, want[1:]))      # ... and inside a pair
    if K == 10:
        assert all(len(want) < K for want in lists) and [] in lists             # (one sentence is left with nothing at all)
    state = ops.merge_moments(on_device(arrays), dev_vids(vids), Nv, garbage_state(S, K), True)
    check_state(state, lists, levels, K)


@pytest.mark.parametrize("device_flag", [False, True])
def test_a_three_chunk_stream_equals_the_one_shot_merge(device_flag):
    """15 videos in three chunks of 5 (the last with two padded slots) through the state == all 15 slots in one launch == the twin;
    the first-chunk flag as a host value and as a device word."""
    from drn_amd import ops
    S, Vc, kv, K, Nv = 3, 5, 2, 4, 20
    order = [int(v) for v in np.random.RandomState(1).permutation(Nv)[:13]] + [-1, -1]
    parts = [(planted(S, Vc, kv, seed=10 + c), order[c:c + Vc]) for c in (0, 5, 10)]
    lists, levels = twin(parts, S, K, Nv)
    state = garbage_state(S, K)
    for c, (arrays, vids) in enumerate(parts):
        first = torch.tensor([int(c == 0)], dtype=torch.int32, device=DEV) if device_flag else c == 0
        ops.merge_moments(on_device(arrays), dev_vids(vids), Nv, state, first)
    check_state(state, lists, levels, K)
    # the same entries as ONE chunk of 15 slots: pair (s, slot) of chunk c becomes pair (s, 5 c + slot)
    whole = tuple(np.concatenate([a[0][f].reshape((S, Vc) + a[0][f].shape[1:]) for a in parts], axis=1).reshape((S * 15,) + parts[0][0][f].shape[1:])
                  for f in range(5))
    once = ops.merge_moments(on_device(whole), dev_vids(order), Nv, garbage_state(S, K), True)
    check_state(once, lists, levels, K)
    for a, b in zip(once, state):
        assert torch.equal(a, b)


def test_the_first_chunk_flag_decides_whether_the_state_is_read():
    from drn_amd import ops
    S, Vc, kv, K, Nv = 2, 4, 2, 6, 9
    a, va = planted(S, Vc, kv, seed=3), [8, 2, 5, 0]
    b, vb = planted(S, Vc, kv, seed=4), [1, 7, 3, 6]
    only_b, lv_b = twin([(b, vb)], S, K, Nv)
    both, lv = twin([(a, va), (b, vb)], S, K, Nv)
    assert only_b != both
    one, zero = (torch.tensor([x], dtype=torch.int32, device=DEV) for x in (1, 0))
    for first_a, first_b, want, levels in ((True, False, both, lv), (one, zero, both, lv), (True, True, only_b, lv_b), (one, one, only_b, lv_b)):
        state = ops.merge_moments(on_device(a), dev_vids(va), Nv, garbage_state(S, K), first_a)
        ops.merge_moments(on_device(b), dev_vids(vb), Nv, state, first_b)
        check_state(state, want, levels, K)


def test_merge_moments_refuses_what_does_not_fit():
    from drn_amd import _lib, ops
    arrays, vids = on_device(planted(2, 3, 2, seed=0)), dev_vids([0, 1, 2])
    with pytest.raises(_lib.DrnError, match="candidates per sentence"):
        ops.merge_moments(arrays, vids, 5, ops.merge_state(2, _lib.MERGE_MAX_CAND - 5, DEV), True)
    with pytest.raises(_lib.DrnError, match="sentences x"):
        ops.merge_moments(arrays, dev_vids([0, 1, 2, 3]), 5, ops.merge_state(2, 4, DEV), True)
    with pytest.raises(_lib.DrnError):
        ops.merge_moments(arrays, vids.cpu(), 5, ops.merge_state(2, 4, DEV), True)


# -- 2. gates= and query_index= -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,D,dtype", [(32, 64, torch.float32), (32, 64, torch.bfloat16), (64, 500, torch.bfloat16)])
def test_query_index_equals_gate_rows_expanded_by_hand(T, D, dtype):
    """S = 2 sentences x V = 3 videos, the gates passed to both sides: every head output bit for bit, with a host and with a device
    index.  (64, 500, bf16) runs the shared front on the zero-padded width."""
    m = tiny_model(T, D, dtype)
    tok, qlen, _, _ = dev_batch(2, T, D, 7)
    _, _, feats, pse = dev_batch(3, T, D, 8)
    qi, vi = torch.tensor([0, 0, 0, 1, 1, 1]), torch.tensor([0, 1, 2, 0, 1, 2])
    with torch.no_grad():
        gates = m.encode_query(tok, qlen)
        by_hand = [torch.stack([g[0], g[0], g[0], g[1], g[1], g[1]]) for g in gates]
        want = m.forward_heads_shared(None, None, feats, pse, video_index=vi, gates=by_hand)
        for index in (qi, qi.to(DEV), qi.to(DEV, torch.int32)):
            got = m.forward_heads_shared(None, None, feats, pse, video_index=vi, query_index=index, gates=gates)
            for j in (1, 2, 3):
                assert len(got[j]) == len(want[j]) == 3
                for a, b in zip(got[j], want[j]):
                    assert a.shape[0] == 6 and torch.equal(a, b), j
        # tokens instead of gates: the encoder runs, on the S sentences
        again = m.forward_heads_shared(tok, qlen, feats, pse, video_index=vi, query_index=qi)
        for j in (1, 2, 3):
            for a, b in zip(again[j], want[j]):
                assert torch.equal(a, b), j
    assert not torch.equal(want[1][0][0], want[1][0][3])         # (the two sentences do gate video 0 differently)


def test_a_host_query_index_out_of_range_raises_and_launches_nothing():
    from drn_amd import _lib, ops
    m = tiny_model(32, 64, torch.float32)
    tok, qlen, _, _ = dev_batch(2, 32, 64, 7)
    _, _, feats, pse = dev_batch(3, 32, 64, 8)
    with torch.no_grad():
        gates = m.encode_query(tok, qlen)
        ops.kernel_timer = []
        try:
            for bad in ([0, 2, 1], [0, -1, 1]):
                with pytest.raises(_lib.DrnError, match="query_index outside"):
                    m.forward_heads_shared(None, None, feats, pse, video_index=torch.tensor([0, 1, 2]), query_index=torch.tensor(bad), gates=gates)
            with pytest.raises(_lib.DrnError, match="query_index"):
                m.forward_heads_shared(None, None, feats, pse, query_index=torch.tensor([0.0, 1.0, 1.0]), gates=gates)
            launches = len(ops.kernel_timer)
        finally:
            ops.kernel_timer = None
    assert launches == 0


# -- 3. the search end to end on a small synthetic store ------------------------------------------------------------------------------

NV, T, D, S = 7, 32, 64, 3


def boosted(m):
    """A classifier that passes most locations (as tests/test_grounding_gpu.py does on the mini dataset): every pair has candidates
    and the NMS has work to do."""
    with torch.no_grad():
        m.fcos.head.cls_logits.bias.fill_(0.5)
        m.fcos.head.cls_logits.weight.mul_(30.0)
    return m


def small_store(dtype=torch.float32):
    """7 videos of 40 rows with 32, 20, 32, 7, 32, 1 and 25 proposals (T = 32: ragged padding)."""
    from drn_amd.store import FeatureStore
    g = torch.Generator().manual_seed(5)
    videos = []
    for v, P in enumerate([32, 20, 32, 7, 32, 1, 25]):
        lo = torch.randint(0, 40, (P,), generator=g)
        hi = torch.minimum(lo + torch.randint(0, 12, (P,), generator=g), torch.tensor(39))
        pse = torch.stack([lo.double() / 40, (hi.double() + 1) / 40], dim=1)
        videos.append(("vid%d" % v, torch.randn(40, D, generator=g), lo.numpy(), hi.numpy(), pse.numpy(), 320))
    return FeatureStore.from_tensors(videos, DEV, dtype)


def sentences(seed):
    tok, qlen, _, _ = dev_batch(S, T, D, seed)
    return tok, qlen


def per_pair_moments(grounder, gates, store, vids, per_video):
    """The per-pair moments of ONE chunk by the path the search is made of -- store.gather on device positions, forward_heads_shared
    with the gates, the selector, ops.select_moments -- as numpy arrays, pair p = (sentence p // Vc, slot p % Vc)."""
    Vc = len(vids)
    pair = torch.arange(S * Vc, device=DEV)
    feats, pse, _ = store.gather(dev_vids(vids), T=T)
    with torch.no_grad():
        mom = grounder._select(per_video, None, None, feats, pse, video_index=pair % Vc, query_index=pair // Vc, gates=gates)
    return tuple(t.cpu().numpy() for t in mom)


def same_hits(a, b, what=""):
    for f in STATE:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


@pytest.mark.parametrize("per_video,top_k", [(1, 4), (3, 10)])
def test_search_equals_the_twin_on_per_pair_moments(per_video, top_k):
    """7 videos in chunks of 3 (the last chunk padded with two -1 slots): video, rank, seg, score, level and n exactly those of
    metrics.merge_moments applied to the per-pair moments of the same chunks."""
    from drn_amd import Grounder
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    tok, qlen = sentences(7)
    grounder = Grounder(m, top_k=5)
    hits = grounder.search(tok, qlen, store, top_k=top_k, per_video=per_video, chunk=3)
    assert m.fcos.box_selector_test.device_only is False
    with torch.no_grad():
        gates = m.encode_query(tok, qlen)
    chunks = [[0, 1, 2], [3, 4, 5], [6, -1, -1]]
    lists, levels = twin([(per_pair_moments(grounder, gates, store, vids, per_video), vids) for vids in chunks], S, top_k, NV)
    check_state([getattr(hits, f) for f in STATE], lists, levels, top_k)
    assert all(len(want) == min(top_k, per_video * NV) for want in lists)         # (every pair had candidates: nothing was a fallback)
    got = hits.tolist(names=store.names)
    for s, want in enumerate(lists):
        assert got[s] == [["vid%d" % w[0], w[1], w[2], w[3]] for w in want]
    assert hits.tolist()[0][0][0] == lists[0][0][0]
    # a subset, by name, in the caller's order
    sub = grounder.search(tok, qlen, store, top_k=top_k, per_video=per_video, videos=["vid4", "vid1"], chunk=3)
    assert set(sub.video[sub.video >= 0].tolist()) <= {1, 4}


def test_one_video_with_per_video_top_k_is_grounds_answer():
    """videos=[v], per_video = top_k: exactly the pair's moments from ground() (the S sentences over that one video), minus the
    fallback moment of a pair without candidates -- checked with the classifier as it is and boosted."""
    from drn_amd import Grounder
    store = small_store()
    tok, qlen = sentences(9)
    fallbacks = 0
    for m in (tiny_model(T, D, torch.float32), boosted(tiny_model(T, D, torch.float32))):
        grounder = Grounder(m, top_k=5)
        for v in (2, 5):
            feats, pse, _ = store.gather([v], T=T)
            mom = grounder.ground(tok, qlen, feats, pse, torch.zeros(S, dtype=torch.int64))
            hits = grounder.search(tok, qlen, store, per_video=5, videos=[v], T=T)
            for s in range(S):
                real = int(mom.index[s, 0]) >= 0
                fallbacks += not real
                n = int(mom.n[s]) if real else 0
                assert int(hits.n[s]) == n, (v, s)
                assert torch.equal(hits.seg[s, :n], mom.seg[s, :n]) and torch.equal(hits.score[s, :n], mom.score[s, :n]), (v, s)
                assert torch.equal(hits.level[s, :n], mom.level[s, :n]) and hits.rank[s, :n].tolist() == list(range(n)), (v, s)
                assert (hits.video[s, :n] == v).all() and (hits.video[s, n:] == -1).all(), (v, s)
    print("pairs whose only moment was the fallback: %d of 12" % fallbacks)


def test_search_does_not_depend_on_the_chunk_size():
    """Chunks of 1, 3 and 7 videos run the trunk on 3, 9 and 21 pairs and prop_fc on 32, 96 and 224 rows.  The shared-video test
    (tests/test_grounding_gpu.py) already relies on a row's result not depending on the batch it is computed in; if that holds here
    too, the three results are bit-identical in every field, which is what is asserted.  Observed: nothing yet -- no GPU run of this
    test is on record; should one show a difference, the scores are to be compared within the tolerance measured against chunk = 7,
    on a seed whose consecutive returned scores lie more than 10x that tolerance apart."""
    from drn_amd import Grounder
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    tok, qlen = sentences(7)
    grounder = Grounder(m, top_k=6)
    want = grounder.search(tok, qlen, store, per_video=2, chunk=7)
    assert int(want.n.min()) == 6
    for chunk in (1, 3):
        same_hits(grounder.search(tok, qlen, store, per_video=2, chunk=chunk), want, chunk)
    same_hits(grounder.search(tok, qlen, store, per_video=2), want, "default chunk")


def test_search_by_graph_replay():
    """graph=True == eager bit for bit over the 3-chunk search; one capture, none for other sentences of the same shape, one more
    after a parameter changed in place; results are copies."""
    from drn_amd import Grounder
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    eager, graphed = Grounder(m, top_k=6), Grounder(m, top_k=6, graph=True)
    tok, qlen = sentences(7)
    first = graphed.search(tok, qlen, store, per_video=2, chunk=3)
    same_hits(first, eager.search(tok, qlen, store, per_video=2, chunk=3), "first search")
    assert graphed.captures == 1
    kept = [getattr(first, f).clone() for f in STATE]
    tok2, qlen2 = sentences(11)
    second = graphed.search(tok2, qlen2, store, per_video=2, chunk=3)
    same_hits(second, eager.search(tok2, qlen2, store, per_video=2, chunk=3), "other sentences")
    assert graphed.captures == 1 and not torch.equal(second.score, first.score)
    for f, c in zip(STATE, kept):
        assert torch.equal(getattr(first, f), c), f
    with torch.no_grad():
        m.fcos.head.cls_logits.bias.add_(0.25)
    same_hits(graphed.search(tok, qlen, store, per_video=2, chunk=3), eager.search(tok, qlen, store, per_video=2, chunk=3), "new bias")
    assert graphed.captures == 2
    same_hits(graphed.search(tok, qlen, store, per_video=2, chunk=3, videos=[6, 0, 3, 2]),
              eager.search(tok, qlen, store, per_video=2, chunk=3, videos=[6, 0, 3, 2]), "two chunks of the same shape")
    assert graphed.captures == 2
    assert m.fcos.box_selector_test.device_only is False


# -- 4. the mini dataset -----------------------------------------------------------------------------------------------------------------

def test_search_on_the_mini_dataset_against_ground():
    """Every sentence of the test split against the whole store: every returned video is a store position, nothing returned is a
    fallback moment, and a sentence's hits in its own video are ground()'s moments for that (sentence, video) pair."""
    from drn_amd import Grounder
    from drn_amd.store import FeatureStore
    from test_store_gpu import hip_model, host_loader, mini, mini_cfg
    ds = mini("test", 3)
    st = FeatureStore.from_dataset(ds, DEV, torch.bfloat16)
    m = hip_model(3, cfg=mini_cfg(3))
    m.set_compute_dtype(torch.bfloat16)
    boosted(m).eval()
    names, _, _, _, tok, qlen, _, _ = next(iter(host_loader(ds, len(ds), torch.bfloat16)))
    tok, qlen = tok.to(DEV), qlen.to(DEV)
    Q, Nv, Tm = len(names), len(st), int(st.nprops.max())
    grounder = Grounder(m, top_k=5)
    hits = grounder.search(tok, qlen, st, top_k=5 * Nv, per_video=5)
    feats, pse, _ = st.gather(list(range(Nv)), T=Tm)
    own = torch.tensor([st.index[name] for name in names])
    mom = grounder.ground(tok, qlen, feats, pse, own)
    n = hits.n.tolist()
    compared = 0
    for q in range(Q):
        video, score = hits.video[q, :n[q]], hits.score[q, :n[q]]
        assert bool(((video >= 0) & (video < Nv)).all()) and bool((hits.level[q, :n[q]] >= 0).all()), q
        assert bool(torch.isfinite(score).all()) and bool((score[:-1] >= score[1:]).all()), q
        mine = (video == int(own[q])).nonzero().flatten()
        k = int(mom.n[q]) if int(mom.index[q, 0]) >= 0 else 0
        assert mine.numel() == k, (q, mine.numel(), k)
        assert torch.equal(hits.seg[q, mine], mom.seg[q, :k]) and torch.equal(hits.score[q, mine], mom.score[q, :k]), q
        assert hits.rank[q, mine].tolist() == list(range(k)), q
        compared += k
    assert compared > 0 and max(n) > 5
