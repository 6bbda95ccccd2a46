"""The shortlist and device candidates on the device: drn_shortlist_topn against shortlist_reference (exact data: torch.equal on every
field; random data: a derived bound), its independence of S, V and n, drn_plan_candidates against plan_candidates_reference inside a
guard band, and Grounder.search(candidates= a device tensor) against the same rows passed as host lists -- on a plain index, a quantised
one, conv0="mxfp8" and its fused form, eagerly and by graph replay -- and the two stages end to end.
tests/test_shortlist_cpu.py holds the plan, the definition and the refusals."""
import functools

import numpy as np
import pytest
import torch

from test_grounding_engine_gpu import DEV, tiny_model
from test_search_gpu import D, NV, S, T, boosted, same_hits, sentences, small_store
from test_shortlist_cpu import PLAN_CASES

pytestmark = pytest.mark.gpu
BLOCK = 256                                                # (= _lib.SHORTLIST_BLOCK, asserted below)
FIELDS = ("ids", "scores", "n")


# -- 1. drn_shortlist_topn ----------------------------------------------------------------------------------------------------------------

def exact_data(V, E, S_, dtype, seed=0):
    """Integer-valued embeddings and queries in [-4, 4]: exact in bf16, every dot product exact in fp32 (|score| <= 16 E), with whole
    rows duplicated -- neighbours, rows a block apart and rows in different blocks -- so that equal scores are certain."""
    g = torch.Generator().manual_seed(seed + 1000 * V + E)
    emb = torch.randint(-4, 5, (V, E), generator=g).float()
    for a, b in ((1, 0), (V - 1, 0), (V // 2, V // 3), (BLOCK, 0), (BLOCK + 5, 2 * BLOCK + 3), (3 * BLOCK + 6, BLOCK - 1), (70, 5)):
        if 0 <= a < V and 0 <= b < V:
            emb[a] = emb[b]
    q = torch.randint(-4, 5, (S_, E), generator=g).float()
    return emb.to(DEV, dtype).contiguous(), q.to(DEV, dtype).contiguous()


def same_shortlist(got, want, what=""):
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), (what, f)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("E", [8, 40, 512])
def test_shortlist_equals_the_reference_exactly(dtype, E):
    """V: one video, one short of / exactly / one past a 64-video wave tile, one block + 1, three blocks + 7; E = 40 is no multiple of
    the MFMA's 32 (nor of the fp32 step's 16); S = 17 is a second sentence tile of one row; n up to the cap, above V and above a block's
    share.  ids, scores and n equal to the float64 definition, bit for bit."""
    from drn_amd import Shortlister, _lib, shortlist_reference
    assert BLOCK == _lib.SHORTLIST_BLOCK and _lib.SHORTLIST_MAX == 128
    for V in (1, 63, 64, 65, BLOCK + 1, 3 * BLOCK + 7):
        emb, q17 = exact_data(V, E, 17, dtype)
        sl = Shortlister(emb)
        for S_ in (1, 16, 17):
            q = q17[:S_].contiguous()
            for n in (1, 5, 64, 128):
                want = shortlist_reference(emb, q, n)
                if 1 < V <= n:                                          # (every video is listed, the planted twins among them)
                    assert bool(((want.scores[:, 1:] == want.scores[:, :-1]) & (want.ids[:, 1:] > want.ids[:, :-1])
                                 & (want.ids[:, 1:] >= 0)).any()), "no tie in the data"
                same_shortlist(sl.shortlist(q, n), want, (V, S_, n))


def test_shortlist_with_odd_widths_reads_no_vector_past_a_row():
    """E = 5 (bf16 rows are not 16-byte aligned: the element-wise loader) and E = 36 (aligned rows, a partial last step)."""
    from drn_amd import Shortlister, shortlist_reference
    for E in (1, 5, 36):
        for dtype in (torch.bfloat16, torch.float32):
            emb, q = exact_data(BLOCK + 9, E, 3, dtype)
            same_shortlist(Shortlister(emb).shortlist(q, 7), shortlist_reference(emb, q, 7), (E, dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_a_score_does_not_depend_on_the_other_sentences_or_on_the_size_of_the_table(dtype):
    """Random data, where a changed summation order would show.  A sentence shortlisted alone (row 0 of its tile) and among 17 (row s of
    tile 0, or row 0 of tile 1): bit-equal rows.  A prefix of the table cut one past a block edge: every video listed by both has the
    same bits, and on exact data the prefix's list is the prefix's reference."""
    from drn_amd import Shortlister, shortlist_reference
    g = torch.Generator().manual_seed(9)
    V, E = 3 * BLOCK + 7, 200
    emb = torch.randn(V, E, generator=g).to(DEV, dtype).contiguous()
    q = torch.randn(17, E, generator=g).to(DEV, dtype).contiguous()
    full = Shortlister(emb).shortlist(q, 128)
    assert int(full.n.min()) == 128
    for s in (0, 5, 16):
        alone = Shortlister(emb).shortlist(q[s:s + 1].contiguous(), 128)
        for f in FIELDS:
            assert torch.equal(getattr(alone, f)[0], getattr(full, f)[s]), (s, f)
        cut = Shortlister(emb).shortlist(q[s:s + 1].contiguous(), 16)
        assert torch.equal(cut.ids[0], full.ids[s, :16]) and torch.equal(cut.scores[0], full.scores[s, :16])
    prefix = Shortlister(emb[:BLOCK + 1].contiguous()).shortlist(q, 128)
    both = 0
    for s in range(17):
        a = dict(zip(full.ids[s].tolist(), full.scores[s].cpu().numpy().view(np.uint32).tolist()))
        b = dict(zip(prefix.ids[s].tolist(), prefix.scores[s].cpu().numpy().view(np.uint32).tolist()))
        shared = set(a) & set(b)
        both += len(shared)
        assert all(a[v] == b[v] for v in shared), s
    assert both > 17 * 20
    emb, q = exact_data(3 * BLOCK + 7, 40, 17, dtype)
    cut = emb[:BLOCK + 1].contiguous()
    same_shortlist(Shortlister(cut).shortlist(q, 64), shortlist_reference(cut, q, 64), "prefix")


def random_case_ratio(emb, q, got):
    """The checks of random data -> the largest |error| / tol.  tol[s, v] = E * 2^-23 * sum_e |q[s, e] * emb[v, e]|: E fp32 roundings
    of a partial sum that never exceeds the sum of the absolute products, each at most 2^-24 relative, with a factor two of margin --
    derived, not measured."""
    E = int(emb.shape[1])
    ref = q.double() @ emb.double().t()
    tol = E * 2.0 ** -23 * (q.double().abs() @ emb.double().abs().t())
    worst = 0.0
    for s in range(q.shape[0]):
        n = int(got.n[s])
        ids, sc = got.ids[s, :n].long(), got.scores[s, :n].double()
        assert n == got.ids.shape[1] and len(set(ids.tolist())) == n
        err = (sc - ref[s, ids]).abs()
        assert bool((err <= tol[s, ids]).all()), s
        worst = max(worst, float((err / tol[s, ids]).max()))
        # sorted by (score descending, position ascending) on the RETURNED scores
        assert bool(((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:-1] < ids[1:]))).all()), s
        # nobody left out is better than the last one listed by more than both tolerances
        out = torch.ones(emb.shape[0], dtype=torch.bool, device=emb.device)
        out[ids] = False
        last = ids[-1]
        assert bool((ref[s][out] <= ref[s, last] + tol[s][out] + tol[s, last]).all()), s
    return worst


def test_shortlist_on_random_bf16_data_is_within_the_derived_bound():
    from drn_amd import Shortlister
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(300, 512, generator=g).to(DEV, torch.bfloat16).contiguous()
    q = torch.randn(5, 512, generator=g).to(DEV, torch.bfloat16).contiguous()
    ratio = random_case_ratio(emb, q, Shortlister(emb).shortlist(q, 16))
    print("largest error / tol: %.4f" % ratio)
    assert ratio <= 1.0


def test_a_nan_query_row_lists_nothing_and_leaves_the_others_alone():
    from drn_amd import Shortlister, _lib, shortlist_reference
    emb, q = exact_data(BLOCK + 30, 40, 17, torch.bfloat16)
    clean = Shortlister(emb).shortlist(q, 9)
    bad = q.clone()
    bad[2, 7], bad[16, 0] = float("nan"), float("inf")                  # (inf * 0 is NaN somewhere, +-inf elsewhere: nothing finite)
    got = Shortlister(emb).shortlist(bad, 9)
    same_shortlist(got, shortlist_reference(emb, bad, 9))
    assert int(got.n[2]) == 0 and bool((got.ids[2] == -1).all()) and bool((got.scores[2] == 0).all()) and int(got.n[16]) < 9
    keep = [s for s in range(17) if s not in (2, 16)]
    for f in FIELDS:
        assert torch.equal(getattr(got, f)[keep], getattr(clean, f)[keep]), f
    poisoned = emb.clone()
    poisoned[3, 3] = float("nan")
    with pytest.raises(_lib.DrnError, match="not finite"):
        Shortlister(poisoned)


def test_out_buffers_are_written_in_place_and_a_captured_shortlist_replays():
    from drn_amd import Shortlist, Shortlister, shortlist_reference
    emb, q = exact_data(2 * BLOCK + 3, 40, 5, torch.bfloat16)
    emb2, q2 = exact_data(2 * BLOCK + 3, 40, 5, torch.bfloat16, seed=7)
    sl = Shortlister(emb)
    n = 100                                                              # (above a sentence's 64-lane stride, below the cap)
    out = Shortlist(torch.full((5, n), 77, dtype=torch.int32, device=DEV), torch.full((5, n), 7.5, device=DEV),
                    torch.full((5,), 77, dtype=torch.int32, device=DEV))
    got = sl.shortlist(q, n, out=out)
    assert all(a is b for a, b in zip(got, out))
    same_shortlist(out, shortlist_reference(emb, q, n), "every element")
    small = Shortlister(emb[:3].contiguous())
    out[0].fill_(77), out[1].fill_(7.5)
    same_shortlist(small.shortlist(q, n, out=out), shortlist_reference(emb[:3], q, n), "the tail past the list")
    # capture on one stream, then replay on other queries written into the captured buffer
    qbuf = q.clone()
    from drn_amd.graph import capture_graph                              # (torch.cuda.graph with the collector held off)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sl.shortlist(qbuf, n, out=out)                                   # (warm: the workspace of this shape exists)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    with capture_graph(graph, stream):
        sl.shortlist(qbuf, n, out=out)
    for queries in (q2, q):
        qbuf.copy_(queries)
        out[0].fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        same_shortlist(out, sl.shortlist(queries, n), "replay == eager")
        same_shortlist(out, shortlist_reference(emb, queries, n), "replay == reference")


# -- 2. drn_plan_candidates -----------------------------------------------------------------------------------------------------------------

def launch_plan(C, Nv, pairs, cap):
    """ops.plan_candidates into the middle of a buffer of sentinels -> (table as numpy, the two guard bands)."""
    from drn_amd import ops, plan_candidate_steps
    Cd = torch.tensor(C, dtype=torch.int32, device=DEV)
    plan = plan_candidate_steps(Cd.shape[0], Cd.shape[1], pairs, cap)
    steps, GUARD = plan.pair_q.shape[0], 256
    buf = torch.full((steps * plan.pairs + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    table = buf[GUARD:GUARD + steps * plan.pairs].view(steps, plan.pairs)
    ops.plan_candidates(Cd, Nv, plan.Sc, plan.Nc, plan.pairs, steps, table)
    return table.cpu().numpy(), torch.cat([buf[:GUARD], buf[GUARD + steps * plan.pairs:]]).cpu().numpy()


def test_plan_candidates_equals_the_reference_and_writes_nothing_outside_its_table():
    from drn_amd.grounding import plan_candidates_reference
    INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
    g = np.random.RandomState(2)
    wide = g.randint(-3, 40, (17, 64))                                   # many repeats, entries below 0 and past the store
    wide[3, 10], wide[3, 50], wide[8, 0], wide[8, 63] = INT_MIN, INT_MAX, INT_MAX, INT_MIN
    longest = g.randint(0, 600, (2, 1024))                               # DRN_CANDIDATES_MAX columns: four strides of the workgroup
    cases = list(PLAN_CASES) + [([[INT_MIN, 3, INT_MAX, 3, -1], [INT_MAX, INT_MAX, 0, INT_MIN, 0]], 8, 4, 2),
                                (wide.tolist(), 32, 16, 5), (wide.tolist(), 32, 100, 64), (wide.tolist(), 32, 7, 64),
                                (longest.tolist(), 600, 512, 300), (longest.tolist(), 600, None, None)]
    for C, Nv, pairs, cap in cases:
        got, guard = launch_plan(C, Nv, pairs, cap)
        want = plan_candidates_reference(C, Nv, len(C), len(C[0]), pairs, cap)
        assert got.shape == want.shape and (got == want).all(), (len(C), len(C[0]), Nv, pairs, cap)
        assert (guard == 0x5A5A5A5A).all()


# -- 3. the search ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def world(kind):
    """kind -> (model, store, index, Grounder keywords): "plain" and "q8" a boosted tiny fp32 model on a plain / a quantised index,
    "mx" and "mxfused" a bf16 one on a quantised index with conv0 on FP8 MFMAs.  Built once, changed by no test."""
    from drn_amd import SearchIndex
    dtype = torch.float32 if kind in ("plain", "q8") else torch.bfloat16
    m, store = boosted(tiny_model(T, D, dtype)), small_store(dtype)
    index = SearchIndex.build(m, store, **({} if kind == "plain" else {"quantize": "mxfp8"}))
    kw = {"plain": {}, "q8": {}, "mx": {"conv0": "mxfp8"}, "mxfused": {"conv0": "mxfp8", "fused": True}}[kind]
    return m, store, index, kw


def cleaned(C):
    """What a device candidates tensor means, as host lists: per row the positions inside the store, first occurrences only."""
    rows = []
    for row in C.tolist():
        keep = []
        for v in row:
            if 0 <= v < NV and v not in keep:
                keep.append(v)
        rows.append(keep)
    return rows


def dev_cands(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


CANDS = [[5, 0, 5, -1], [-1, -1, -1, -1], [3, 3, 6, 2]]                 # repeats, -1, a sentence without a candidate
OTHER = [[1, 9, 4, 4], [6, 0, 2, 3], [-7, 5, 5, 1]]                      # the same shape: the same graph


@pytest.mark.parametrize("kind", ["plain", "q8", "mx", "mxfused"])
def test_device_candidates_equal_the_same_rows_as_host_lists(kind):
    """S = 3, N = 4.  pairs = 2: one sentence and two columns per step; 5: one sentence, four columns and a padded pair; 12 and the
    default: one step.  per_video = 2 with top_k = 5 and 1 with top_k = 3."""
    from drn_amd import Grounder
    m, store, index, kw = world(kind)
    tok, qlen = sentences(7)
    C = dev_cands(CANDS)
    assert cleaned(C) == [[5, 0], [], [3, 6, 2]]
    for per_video, K in ((2, 5), (1, 3)):
        grounder = Grounder(m, top_k=K, **kw)
        want = grounder.search(tok, qlen, index, per_video=per_video, candidates=cleaned(C), T=index.T)
        assert int(want.n[0]) > 1 and int(want.n[1]) == 0 and int(want.n[2]) > 1
        for pairs in (2, 5, 12, None):
            got = grounder.search(tok, qlen, index, per_video=per_video, candidates=C, T=index.T, pairs=pairs)
            same_hits(got, want, (kind, per_video, pairs))
        same_hits(grounder.search(tok, qlen, index, per_video=per_video, candidates=C), want, "T defaults to index.T")
    assert m.fcos.box_selector_test.device_only is False


@pytest.mark.parametrize("kind", ["plain", "mxfused"])
def test_every_video_as_device_candidates_is_the_search_without_candidates(kind):
    from drn_amd import Grounder
    m, store, index, kw = world(kind)
    tok, qlen = sentences(7)
    grounder = Grounder(m, top_k=6, **kw)
    want = grounder.search(tok, qlen, index, per_video=2)
    everything = torch.arange(len(index), dtype=torch.int32, device=DEV).repeat(S, 1)
    same_hits(grounder.search(tok, qlen, index, per_video=2, candidates=everything), want, "default")
    same_hits(grounder.search(tok, qlen, index, per_video=2, candidates=everything, pairs=5), want, "pairs = 5")
    short = grounder.search(tok, qlen, index, per_video=2, candidates=dev_cands([[3], [3], [3]]), T=16)        # (vid3: 7 proposals)
    same_hits(short, grounder.search(tok, qlen, index, per_video=2, candidates=[[3], [3], [3]], T=16), "a short T, passed")
    assert int(short.n.min()) > 0


@pytest.mark.parametrize("kind", ["plain", "q8", "mx", "mxfused"])
def test_device_candidates_by_graph_replay(kind):
    """graph=True == eager; another tensor of the same shape and other sentences replay the same graph; one plan launch per search."""
    from drn_amd import Grounder, ops
    m, store, index, kw = world(kind)
    (tok, qlen), (tok2, qlen2) = sentences(7), sentences(11)
    eager, graphed = Grounder(m, top_k=5, **kw), Grounder(m, top_k=5, graph=True, **kw)
    skw = dict(per_video=2, pairs=5)
    C, C2 = dev_cands(CANDS), dev_cands(OTHER)
    first = graphed.search(tok, qlen, index, candidates=C, **skw)
    same_hits(first, eager.search(tok, qlen, index, candidates=C, **skw), "first call")
    assert graphed.captures == 1 and int(first.n[1]) == 0
    kept = first.score.clone()
    ops.kernel_timer = []
    try:
        second = graphed.search(tok2, qlen2, index, candidates=C2, **skw)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags.count("plan_candidates") == 1
    same_hits(second, eager.search(tok2, qlen2, index, candidates=C2, **skw), "another tensor, other sentences")
    same_hits(second, eager.search(tok2, qlen2, index, candidates=cleaned(C2), T=index.T, per_video=2), "as host lists")
    assert graphed.captures == 1 and torch.equal(first.score, kept) and not torch.equal(second.score, first.score)
    same_hits(graphed.search(tok, qlen, index, candidates=C, **skw), first, "again")
    assert graphed.captures == 1 and m.fcos.box_selector_test.device_only is False
    ops.kernel_timer = []
    try:
        eager.search(tok, qlen, index, candidates=C, **skw)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags.count("plan_candidates") == 1


def test_device_candidates_refuse_before_any_launch():
    from drn_amd import Grounder, _lib, ops
    m, store, index, _ = world("plain")
    tok, qlen = sentences(7)
    C = dev_cands(CANDS)
    ops.kernel_timer = []
    try:
        for g in (Grounder(m, top_k=5), Grounder(m, top_k=5, graph=True)):
            with pytest.raises(_lib.DrnError, match="build an index"):
                g.search(tok, qlen, store, candidates=C)
            with pytest.raises(_lib.DrnError, match="exclude each other"):
                g.search(tok, qlen, index, candidates=C, videos=[0, 1])
            with pytest.raises(_lib.DrnError, match="must be int32"):
                g.search(tok, qlen, index, candidates=C.long())
            with pytest.raises(_lib.DrnError, match=r"must be \(3, N\)"):
                g.search(tok, qlen, index, candidates=C[:2].contiguous())
            with pytest.raises(_lib.DrnError, match="1 <= N <= 1024"):
                g.search(tok, qlen, index, candidates=torch.zeros((3, 1025), dtype=torch.int32, device=DEV))
            with pytest.raises(_lib.DrnError, match="chunk= does not apply"):
                g.search(tok, qlen, index, candidates=C, chunk=2)
            with pytest.raises(_lib.DrnError, match="at least 1"):
                g.search(tok, qlen, index, candidates=C, pairs=0)
        launches = len(ops.kernel_timer)
    finally:
        ops.kernel_timer = None
    assert launches == 0


# -- 4. the two stages end to end ------------------------------------------------------------------------------------------------------------

def test_shortlist_then_search_never_leaves_the_device():
    """search(candidates=shortlist.ids) == the same search fed the shortlist read back as host lists; evaluate_search with a callable
    that returns the device tensor == with one that returns the lists; one shortlist_topn tag per shortlist."""
    from drn_amd import Grounder, Shortlister, evaluate_search, ops
    m, store, index, kw = world("plain")
    g = torch.Generator().manual_seed(12)
    emb = torch.randint(-4, 5, (NV, 16), generator=g).float()
    emb[4] = emb[1]                                                       # a tie the shortlist must break by position
    sl = Shortlister(emb.to(DEV).contiguous(), names=store.names)
    sl.check(store), sl.check(index)
    qe = torch.randint(-4, 5, (S, 16), generator=g).float().to(DEV)
    qe[1] = float("nan")                                                  # a sentence whose shortlist is empty: ids all -1
    grounder = Grounder(m, top_k=5, **kw)
    tok, qlen = sentences(7)
    n = 4
    ops.kernel_timer = []
    try:
        short = sl.shortlist(qe, n)
        tags = [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None
    assert tags == ["shortlist_topn"]
    lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]
    assert [len(l) for l in lists] == [n, 0, n]
    got = grounder.search(tok, qlen, index, per_video=2, candidates=short.ids)
    same_hits(got, grounder.search(tok, qlen, index, per_video=2, candidates=lists, T=index.T), "two stages")
    assert int(got.n[0]) > 0 and int(got.n[1]) == 0
    batches = [(["vid0", "vid3", "vid5"], tok, qlen, torch.tensor([[0.1, 0.5], [0.0, 1.0], [0.3, 0.9]], dtype=torch.float64)),
               (["vid6", "vid2", "vid4"], *sentences(11), torch.tensor([[0.2, 0.4], [0.5, 1.0], [0.0, 0.3]], dtype=torch.float64))]
    on_device = lambda names, t, l: sl.shortlist(qe, n).ids
    on_host = lambda names, t, l: [row[:k] for row, k in zip(*(x.tolist() for x in sl.shortlist(qe, n)[::2]))]
    for gr in (grounder, Grounder(m, top_k=5, graph=True, **kw)):
        a = evaluate_search(gr, batches, index, topks=(1, 5), per_video=2, candidates=on_device, T=index.T)
        b = evaluate_search(grounder, batches, index, topks=(1, 5), per_video=2, candidates=on_host, T=index.T)
        assert a.first_hits.tolist() == b.first_hits.tolist() and a.moment == b.moment and a.video == b.video and a.n == 6
