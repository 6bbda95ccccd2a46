"""Corpus recall of a search on the device (drn_amd.search_eval): drn_search_recall against its host twin
(metrics.search_first_hits, pinned by tests/test_search_eval_cpu.py) on planted tables, its refusals, evaluate_search end to end on
test_search_gpu's small store -- against the twin on Hits.tolist(), on an index, by graph replay, with shortlists, and tied back to
the single-video path -- and Trainer.evaluate_search on the committed mini dataset.  Every comparison is exact equality."""
import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV, tiny_model
from test_search_gpu import D, T, boosted, sentences, small_store

pytestmark = pytest.mark.gpu
IOUS = {1: (0.5,), 2: (0.5, 0.7), 3: (0.3, 0.5, 0.7)}


# -- 1. drn_search_recall against the host twin -------------------------------------------------------------------------------------------

def planted(S, K, seed):
    """A Hits table and its ground truth as numpy arrays, planted: videos from a small range (repeats), segment bounds from multiples
    of 1/8 (tIoU exactly 0.5 occurs), in every row of three entries or more the right video with a moment that misses and, later, the
    ground truth itself, rows with n < K whose entries past n WOULD hit (the ground truth's video and segment), and -- where S allows --
    a row with n = 0, one with n above K, one with gt_video = -1, one with a NaN ground truth, one whose video no entry names.
    -> seg (S, K, 2) f32, video (S, K) i32, n (S,) i32, gt_video (S,) i32, gt (S, 2) f64."""
    g = np.random.RandomState(seed)
    nvid = 4 if K < 64 else 24
    video = g.randint(0, nvid, (S, K)).astype(np.int32)
    seg = (np.sort(g.randint(0, 9, (S, K, 2)), axis=2) / 8.0).astype(np.float32)
    gt_video = g.randint(0, nvid, (S,)).astype(np.int32)
    start = g.randint(0, 8, (S,))
    gt = np.stack([start, start + 1 + g.randint(0, 8, (S,)) % (8 - start)], axis=1) / 8.0
    n = np.full((S,), K, dtype=np.int32)
    if (S, K) == (1, 1):                         # one entry: the right video, a moment that misses -> [K, 0]
        video[0, 0], seg[0, 0], gt[0] = gt_video[0], (0.0, 0.125), (0.25, 0.75)
    if K > 1:
        n[0] = K // 2 + 1
    if S >= 5:
        n[1], n[2], gt_video[3], gt[4, 0] = 0, K + 3, -1, np.nan
    if S == 3:
        n[0], n[1], n[2] = K, 67, K + 5
    if K == 130:
        # row 0: 85 entries of 70 distinct videos (15 of them twice), shuffled; the ground truth's video first at 85 with a moment that
        # misses, again at 90 with tIoU exactly 0.5 -> [90, 70]
        n[0], n[1], gt_video[0], gt[0] = K, 100, 7, (0.25, 0.75)
        video[0, :85] = g.permutation(np.concatenate([np.arange(100, 170), np.arange(100, 115)]))
        video[0, 85:] = g.randint(100, 104, (K - 85,))
        video[0, 85], seg[0, 85] = 7, (0.0, 0.125)
        video[0, 90], seg[0, 90] = 7, (0.25, 0.5)
    for s in range(S):
        m = min(max(int(n[s]), 0), K)
        if m >= 3 and not (K == 130 and s == 0):
            # the right video at m // 3 with a moment that misses every threshold, the ground truth itself at 2 m // 3
            video[s, m // 3], seg[s, m // 3] = max(int(gt_video[s]), 0), ((0.0, 0.125) if gt[s, 1] > 0.5 and not gt[s, 0] < 0.5 else (0.875, 1.0))
            video[s, 2 * m // 3], seg[s, 2 * m // 3] = max(int(gt_video[s]), 0), gt[s].astype(np.float32)
        video[s, m:], seg[s, m:] = max(int(gt_video[s]), 0), gt[s].astype(np.float32)
    if K == 130:                                 # row 1: the right video is there, but before n none of its moments hits
        seg[1, :100][video[1, :100] == gt_video[1]] = (0.0, 0.125) if gt[1, 0] >= 0.5 else (0.875, 1.0)
    if S == 3:
        gt_video[2] = 99                         # a video that is in none of the row's entries
    return seg, video, n, gt_video, gt


def rows_of(seg, video, n):
    """What Hits.tolist() makes of the table: per sentence [[video, start, end, score], ...], the first min(max(n, 0), K) entries."""
    K = video.shape[1]
    return [[[int(video[s, p]), float(seg[s, p, 0]), float(seg[s, p, 1]), 0.0] for p in range(min(max(int(n[s]), 0), K))]
            for s in range(video.shape[0])]


def as_hits(seg, video, n):
    from drn_amd.grounding import Hits
    t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return Hits(t(seg), None, t(video), None, None, t(n))


@pytest.mark.parametrize("gt_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("S,K,I", [(1, 1, 1), (5, 4, 2), (3, 70, 3), (2, 130, 1)])
def test_search_recall_equals_the_host_twin(S, K, I, gt_dtype):
    """(3, 70, 3) and (2, 130, 1) cross the 64-lane stride; in the latter sentence 0 meets its video first at position 85, after 70
    distinct videos and 15 repeats.  The ground truth is exact in float32 (multiples of 1/8), so both dtypes have one twin table."""
    from drn_amd import ops
    from drn_amd.metrics import search_first_hits
    seg, video, n, gt_video, gt = planted(S, K, seed=K)
    ious = IOUS[I]
    want = search_first_hits(rows_of(seg, video, n), gt_video, gt, ious, K)
    # not vacuous: hits, misses, and a video ranked higher than its moment
    assert (want < K).any() and (want == K).any() and (want[:, I:] < want[:, :I]).any(), want
    if K == 130:
        assert want[0].tolist() == [90, 70]
    if S >= 5:
        assert want[1].tolist() == want[3].tolist() == [K] * (I + 1) and want[4, :I].tolist() == [K] * I
    got = ops.search_recall(as_hits(seg, video, n), torch.from_numpy(gt_video).to(DEV), torch.from_numpy(gt).to(DEV, gt_dtype),
                            torch.tensor(ious, dtype=torch.float64, device=DEV))
    assert got.dtype == torch.int32 and tuple(got.shape) == (S, I + 1)
    assert got.cpu().numpy().tolist() == want.tolist()


def test_search_recall_refuses_what_it_cannot_score():
    from drn_amd import _lib, ops
    seg, video, n, gt_video, gt = (torch.from_numpy(a).to(DEV) for a in planted(5, 4, seed=4))
    ious = torch.tensor([0.5, 0.7], dtype=torch.float64, device=DEV)
    assert tuple(ops.search_recall(as_hits(seg, video, n), gt_video, gt, ious).shape) == (5, 3)
    with pytest.raises(_lib.DrnError, match="K = 0"):
        ops.search_recall(as_hits(seg[:, :0].contiguous(), video[:, :0].contiguous(), n), gt_video, gt, ious)
    with pytest.raises(_lib.DrnError, match="I = 0"):
        ops.search_recall(as_hits(seg, video, n), gt_video, gt, ious[:0])
    big = _lib.MERGE_MAX_CAND + 1
    with pytest.raises(_lib.DrnError, match="K = %d hit slots per sentence" % big):
        ops.search_recall(as_hits(torch.zeros(5, big, 2, device=DEV), torch.zeros(5, big, dtype=torch.int32, device=DEV), n), gt_video, gt, ious)
    wide = torch.zeros(5, 8, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.DrnError, match="video must be a contiguous"):
        ops.search_recall(as_hits(seg, wide[:, ::2], n), gt_video, gt, ious)
    with pytest.raises(_lib.DrnError, match="seg must be a contiguous"):
        ops.search_recall(as_hits(seg.double(), video, n), gt_video, gt, ious)
    with pytest.raises(_lib.DrnError, match="gt_video must be a contiguous"):
        ops.search_recall(as_hits(seg, video, n), gt_video.long(), gt, ious)


# -- 2. evaluate_search end to end on the small store ------------------------------------------------------------------------------------

NAMES = (["vid2", "vid5", "vid0"], ["vid5", "vid6", "vid3"])
GT = [[0.0, 0.5], [0.125, 0.625], [0.375, 1.0]]


@pytest.fixture(scope="module")
def world():
    """The boosted tiny model, the 7-video store and its index, and two batches of S = 3 annotated sentences: the ground-truth videos of
    a batch are three different positions, one of them video 5 (a single proposal).  The first batch is "annotated" with the model's
    own best moment of each (sentence, video) pair, so a search that ranks that video's best moment at all hits with tIoU 1; the
    second with fixed fractions.  The tokens are on the device, the ground truth of the first batch on the host in float64, that of
    the second on the device in float32."""
    from drn_amd import Grounder, SearchIndex
    m, store = boosted(tiny_model(T, D, torch.float32)), small_store()
    batches = []
    for b, seed in enumerate((7, 11)):
        tok, qlen = sentences(seed)
        if b == 0:
            gt = Grounder(m, top_k=5).ground_stored(tok, qlen, store, NAMES[b], T=T).seg[:, 0].double().cpu()
        else:
            gt = torch.tensor(GT, dtype=torch.float32, device=DEV)
        batches.append((NAMES[b], tok, qlen, gt))
    return m, store, SearchIndex.build(m, store), batches


def twin_table(grounder, batches, store, ious, K, **kw):
    """metrics.search_first_hits on grounder.search(...).tolist() of every batch, concatenated."""
    from drn_amd.metrics import search_first_hits
    parts = []
    for names, tok, qlen, gt in batches:
        rows = grounder.search(tok, qlen, store, top_k=K, **kw).tolist()
        parts.append(search_first_hits(rows, [store.index[name] for name in names], gt.tolist(), ious, K))
    return np.concatenate(parts)


@pytest.mark.parametrize("per_video", [1, 3])
def test_evaluate_search_equals_the_twin_on_the_hits(world, per_video):
    from drn_amd import Grounder, SearchRecall, evaluate_search
    from drn_amd.metrics import recall_from_first_hits
    m, store, index, batches = world
    grounder = Grounder(m, top_k=5)
    ious, topks = (0.3, 0.5, 0.7), (1, 5, 10)
    res = evaluate_search(grounder, batches, store, ious=ious, topks=topks, per_video=per_video, chunk=3)
    want = twin_table(grounder, batches, store, ious, 10, per_video=per_video, chunk=3)
    print("first hits, per_video = %d:\n%s" % (per_video, res.first_hits))
    assert isinstance(res, SearchRecall) and res.n == 6 and res.ious == list(ious) and res.topks == list(topks)
    assert res.first_hits.dtype == np.int32 and res.first_hits.tolist() == want.tolist()
    assert res.moment == recall_from_first_hits(want[:, :3], ious, topks) and len(res.moment) == 9
    assert res.video == recall_from_first_hits(want[:, 3:], ious[:1], topks) and len(res.video) == 3
    assert (want[:, 3] <= want[:, :3].min(axis=1)).all()          # (a video is never ranked below its own moments)
    assert (want[:, :3] < 10).any() and (want[:, :3] == 10).any()  # hits (the first batch's annotations) and misses
    assert m.fcos.box_selector_test.device_only is False
    # the index: the same table
    assert evaluate_search(grounder, batches, index, ious=ious, topks=topks, per_video=per_video, chunk=3).first_hits.tolist() == want.tolist()


def test_evaluate_search_by_graph_replay(world):
    from drn_amd import Grounder, evaluate_search
    m, store, index, batches = world
    eager, graphed = Grounder(m, top_k=5), Grounder(m, top_k=5, graph=True)
    want = evaluate_search(eager, batches, store, topks=(1, 6), per_video=2, chunk=3).first_hits
    first = evaluate_search(graphed, batches, store, topks=(1, 6), per_video=2, chunk=3)
    assert first.first_hits.tolist() == want.tolist() and graphed.captures == 1
    again = evaluate_search(graphed, batches, store, topks=(1, 6), per_video=2, chunk=3)
    assert again.first_hits.tolist() == want.tolist() and graphed.captures == 1
    assert again.moment == first.moment and again.video == first.video


def test_evaluate_search_with_candidates(world):
    """All videos for every sentence: the table of candidates=None.  Everything but the own video: K everywhere."""
    from drn_amd import Grounder, evaluate_search
    m, store, index, batches = world
    grounder = Grounder(m, top_k=5)
    want = evaluate_search(grounder, batches, store, topks=(1, 8), per_video=2)
    calls = []

    def everything(names, tok, qlen):
        calls.append((list(names), tuple(tok.shape), tuple(qlen.shape)))
        return [list(range(len(store)))] * len(names)
    got = evaluate_search(grounder, batches, store, topks=(1, 8), per_video=2, candidates=everything)
    assert got.first_hits.tolist() == want.first_hits.tolist() and got.moment == want.moment and got.video == want.video
    assert calls == [(list(names), tuple(tok.shape), tuple(qlen.shape)) for names, tok, qlen, _ in batches]       # once per batch
    others = lambda names, tok, qlen: [[v for v in range(len(store)) if v != store.index[name]] for name in names]
    none = evaluate_search(grounder, batches, store, topks=(1, 8), per_video=2, candidates=others)
    assert none.first_hits.tolist() == [[8, 8, 8]] * 6 and none.moment == [0.0] * 4 and none.video == [0.0] * 2


def test_the_own_video_alone_is_the_single_video_answer(world):
    """A shortlist of only the sentence's own video with per_video = top_k = 5: the moment columns are the first hit among
    ground_stored()'s moments of that (sentence, video) pair, for every sentence whose pair has a candidate at all."""
    from drn_amd import Grounder, evaluate_search
    from drn_amd.metrics import search_first_hits
    m, store, index, batches = world
    grounder = Grounder(m, top_k=5)
    ious = (0.3, 0.5, 0.7)
    own = lambda names, tok, qlen: [[store.index[name]] for name in names]
    # (T given: the second batch's own videos have 1, 25 and 7 proposals, and the pyramid needs an even count)
    res = evaluate_search(grounder, batches, store, ious=ious, topks=(5,), per_video=5, candidates=own, T=T)
    qualify, o = 0, 0
    for names, tok, qlen, gt in batches:
        mom = grounder.ground_stored(tok, qlen, store, names, T=T)
        ids, real = [store.index[name] for name in names], (mom.index[:, 0] >= 0).tolist()
        rows = [[[v, r[0], r[1], r[2]] for r in moments] for v, moments in zip(ids, mom.tolist())]
        want = search_first_hits(rows, ids, gt.tolist(), ious, 5)
        for q in range(len(names)):
            if real[q]:
                assert res.first_hits[o + q, :3].tolist() == want[q, :3].tolist(), (o, q)
                assert res.first_hits[o + q, 3] == 0
                qualify += 1
            else:
                assert res.first_hits[o + q].tolist() == [5] * 4, (o, q)
        o += len(names)
    assert qualify >= 2


def test_every_video_is_found_among_seven(world):
    """per_video = 1, topks = (7,): the boosted model has a candidate in every (sentence, video) pair, so each of the 7 videos is in
    every sentence's hits and video recall at 7 is 1."""
    from drn_amd import Grounder, evaluate_search
    m, store, index, batches = world
    res = evaluate_search(Grounder(m, top_k=5), batches, store, topks=(7,), per_video=1)
    assert res.video == [1.0], res.first_hits


def test_a_name_the_store_lacks_raises_before_any_launch(world):
    from drn_amd import Grounder, _lib, evaluate_search, ops
    m, store, index, batches = world
    names, tok, qlen, gt = batches[0]
    ops.kernel_timer = []
    try:
        with pytest.raises(_lib.DrnError, match="no video named vid9"):
            evaluate_search(Grounder(m, top_k=5), [(["vid2", "vid9", "vid0"], tok, qlen, gt)], store, topks=(1, 5))
        launches = len(ops.kernel_timer)
    finally:
        ops.kernel_timer = None
    assert launches == 0
    assert m.fcos.box_selector_test.device_only is False


# -- 3. the mini dataset -----------------------------------------------------------------------------------------------------------------

def test_trainer_evaluate_search_on_the_mini_dataset():
    """n = len(ds), rows in loader order, every batch's rows the twin on a direct search of that batch, the training flag restored."""
    from drn_amd import Grounder
    from drn_amd import trainer as TR
    from drn_amd.metrics import recall_from_first_hits, search_first_hits
    from drn_amd.store import FeatureStore, StoreLoader
    from test_store_gpu import hip_model, mini, mini_cfg
    ds = mini("test", 3)
    st = FeatureStore.from_dataset(ds, DEV, torch.bfloat16)
    m = hip_model(3, cfg=mini_cfg(3))
    m.set_compute_dtype(torch.bfloat16)
    boosted(m)
    tr = TR.Trainer(m, 3, lr=1e-4)
    loader = StoreLoader(ds, st, 4)
    ious, topks = (0.5, 0.7), (1, 5)
    m.train()
    res = tr.evaluate_search(loader, st, ious=ious, topks=topks)
    assert m.training is True
    m.eval()
    again = tr.evaluate_search(loader, st, ious=ious, topks=topks)
    assert m.training is False and again.first_hits.tolist() == res.first_hits.tolist()
    grounder = Grounder(m)
    # batches of 4 (the whole split in one) and of 3 (two batches: the tables are joined in loader order)
    for loader, got in ((loader, res), (StoreLoader(ds, st, 3), None)):
        got = tr.evaluate_search(loader, st, ious=ious, topks=topks, grounder=grounder) if got is None else got
        parts = []
        for names, vids, gt, tok, qlen, _, _ in loader.host_batches():
            rows = grounder.search(tok.to(DEV), qlen.to(DEV), st, top_k=5, per_video=1).tolist()
            parts.append(search_first_hits(rows, vids.tolist(), gt.tolist(), ious, 5))
        want = np.concatenate(parts)
        assert len(parts) == len(loader) and got.n == len(ds) and tuple(got.first_hits.shape) == (len(ds), 3)
        assert got.first_hits.tolist() == want.tolist()
        assert got.moment == recall_from_first_hits(want[:, :2], ious, topks) and got.video == recall_from_first_hits(want[:, 2:], ious[:1], topks)
    assert len(parts) == 2
    print("mini dataset, synthetic weights: first hits\n%s" % res.first_hits)
