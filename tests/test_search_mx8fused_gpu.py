"""conv0 of a search on block-scaled FP8 MFMAs with BatchNorm, ReLU and the gate in the same launch (drn_conv0_mx8_bn, LDS-staged tiles
of 256 rows that may hold several pairs and sentences), on the device: EQUAL to the float64 oracle on exact data, independent of the
order and grouping of the pairs, within a derived tolerance on random data through the epilogue -- and Grounder(conv0="mxfp8",
fused=True) end to end: the launches it makes, conv0's outputs, the invariances of the search and its agreement with the unfused mode."""
import os

import pytest
import torch

from test_grounding_engine_gpu import DEV, tiny_model
from test_search_gpu import D, S, T, boosted, dev_vids, same_hits, sentences
from test_search_index_gpu import store_of
from test_search_mx8conv_gpu import BF, MOMENT, conv0_parts, exact_case, launch_tags, random_case, raw_bound, shared

pytestmark = pytest.mark.gpu
FILL = 7.0


def run_bn(case, L, dtype, ss=None, gate=None, extra=0, **kw):
    """ops.conv0_mx8_bn on a case of test_search_mx8conv_gpu -> (out, gated or None, the buffers they are column slices of)."""
    from drn_amd import ops
    index, wcodes, wscales, wpos, pq, pv, vids = case
    Dp, P, Cout, Q = int(wcodes.shape[3]), 0 if wpos is None else int(wpos.shape[2]), int(wcodes.shape[2]), int(pq.numel())
    wide = [torch.full((Q + 1, L, Cout + extra), FILL, dtype=dtype, device=DEV) for _ in range(2 if gate is not None else 1)]
    out = wide[0][:Q, :, :Cout]
    gated = wide[1][:Q, :, :Cout] if gate is not None else None
    ops.conv0_mx8_bn(index.codes, index.scales, index.pos, index.pad_row, index.prop_off, wcodes, wscales, wpos, pq, pv, vids, ss, gate, out,
                     gated, L, Dp, P, **kw)
    return out, gated, wide


def permuted(case, perm):
    index, wcodes, wscales, wpos, pq, pv, vids = case
    perm = perm.to(DEV)
    return index, wcodes, wscales, wpos, pq[perm].contiguous(), pv[perm].contiguous(), vids


INTERLEAVED = torch.tensor([0, 7, 1, 8, 2, 9, 3, 10, 4, 11, 5, 12, 6, 13])                   # pq = 0, 1, 0, 1, ...
SHUFFLED = torch.randperm(14, generator=torch.Generator().manual_seed(5))


# -- 1. exact data: EQUAL to the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Dp,P,Cout", [(Dp, P, Cout) for Dp in (64, 160, 384) for P in (0, 32) for Cout in (16, 48)] + [(64, 32, 272)])
def test_the_bare_convolution_on_exact_data_equals_the_oracle(Dp, P, Cout):
    """ss = None, fp32: the accumulators themselves.  14 pairs x L = 12 or 5 is ONE tile of 256 rows that holds both sentences (they meet
    between pairs 6 and 7); L = 20: two tiles, pair 12 across them; L = 70: every pair but four straddles a tile edge; L = 300: every
    pair is longer than a tile, so the taps reach across tile edges.  Cout = 272: a second channel group of 16; Cout = 16, 48: fragments
    and whole waves past Cout."""
    from drn_amd.index import mx8_conv0_reference
    case = exact_case(Dp, P, Cout, 7 * Dp + P + Cout)
    for L in (12, 5) + ((20, 70, 300) if (Dp, Cout) == (160, 48) else ()):
        out, _, wide = run_bn(case, L, torch.float32, pq_host=case[4].cpu())
        want = mx8_conv0_reference(*case, L)
        got = out.double().cpu()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (L, bad.shape[0], bad[:6].tolist(), got[want != got][:6].tolist(), want[want != got][:6].tolist())
        assert float(want.abs().max()) > 64 and not torch.equal(want[0], want[7])          # (two sentences with different weights)
        assert torch.equal(got[2], got[3]) and torch.equal(got[2], got[5])                  # slot -1, the empty video, Nv: the pad row
        assert bool((wide[0][14] == FILL).all())                                            # the rows past the last pair


# -- 2. the order and the grouping of the pairs do not matter --------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [12, 70])
def test_a_pairs_output_does_not_depend_on_the_order_of_the_pairs_exact(L):
    """The same pairs with the sentences interleaved (14 passes' worth of sentence changes inside a tile, two distinct sentences) and in
    a random order: each pair's output bit for bit that of the unpermuted run, hence the oracle's."""
    from drn_amd.index import mx8_conv0_reference
    case = exact_case(160, 32, 48, 21)
    base = run_bn(case, L, torch.float32)[0]
    assert torch.equal(base.double().cpu(), mx8_conv0_reference(*case, L))
    for perm in (INTERLEAVED, SHUFFLED):
        got = run_bn(permuted(case, perm), L, torch.float32)[0]
        assert torch.equal(got, base[perm.to(DEV)]), perm.tolist()


def epilogue_case():
    """random_case(384, 256, 64) with a scale / shift table of mixed signs and a gate per pair."""
    case = random_case(384, 256, 64, 11)
    g = torch.Generator().manual_seed(17)
    ss = torch.stack([torch.randn(64, generator=g) * 0.5, torch.randn(64, generator=g) * 2.0]).to(DEV)
    gate = torch.randn(14, 64 + 8, generator=g).to(DEV)[:, :64]                              # (row stride above the row)
    return case, ss, gate


def test_a_pairs_output_does_not_depend_on_the_order_of_the_pairs_bf16_with_the_epilogue():
    case, ss, gate = epilogue_case()
    L = 40
    out, gated, _ = run_bn(case, L, BF, ss=ss, gate=gate)
    for perm in (INTERLEAVED, SHUFFLED):
        gp = gate[perm.to(DEV)]
        o, g, _ = run_bn(permuted(case, perm), L, BF, ss=ss, gate=gp)
        assert torch.equal(o, out[perm.to(DEV)]) and torch.equal(g, gated[perm.to(DEV)]), perm.tolist()


# -- 3. random data through the epilogue, within the derived tolerance ---------------------------------------------------------------------------

def test_random_data_through_batchnorm_relu_and_gate_is_within_the_derived_tolerance():
    """Dp = 384, P = 256, Cout = 64, L = 40 (560 rows: three tiles, both sentences in the second), bf16.  want = relu(ref scale + shift)
    in float64; tolerance = |scale| K 2^-23 sum |a b| (the fp32 summation of K = 3 (Dp + P) exact products in any order)
    + 2^-8 |want| (out's bf16 rounding) + 2^-20 (|ref scale| + |shift|) (the affine map in fp32) -- test_search_mx8conv_gpu's bound
    without raw's own 2^-8 |ref|: raw is not rounded here.  gated: |gate| tol (1 + 2^-7) + 2^-8 |want gate|.  Columns past Cout and the
    rows past the last pair keep their fill."""
    from drn_amd.index import mx8_conv0_reference
    case, ss, gate = epilogue_case()
    L = 40
    out, gated, wide = run_bn(case, L, BF, ss=ss, gate=gate, extra=8)
    ref = mx8_conv0_reference(*case, L)
    mag_bound = raw_bound(*case, L, ref) - 2.0 ** -8 * ref.abs()                              # K 2^-23 sum |a b|
    scale, shift = ss[0].double().cpu(), ss[1].double().cpu()
    want = torch.relu(ref * scale + shift)
    tol = scale.abs() * mag_bound + 2.0 ** -8 * want.abs() + 2.0 ** -20 * ((ref * scale).abs() + shift.abs())
    ratio = ((out.double().cpu() - want).abs() / tol.clamp_min(1e-30)).max()
    g1 = gate.double().cpu()[:, None, :]
    want_g = want * g1
    tol_g = g1.abs() * tol * (1 + 2.0 ** -7) + 2.0 ** -8 * want_g.abs()
    ratio_g = ((gated.double().cpu() - want_g).abs() / tol_g.clamp_min(1e-30)).max()
    print("conv0_mx8_bn bf16: largest error / tolerance = %.4f (out), %.4f (gated)" % (float(ratio), float(ratio_g)))
    assert float(ratio) <= 1.0 and float(ratio_g) <= 1.0
    assert float(want.max()) > 1.0 and 0.1 < float((want == 0).double().mean()) < 0.9 and bool((scale < 0).any()) and bool((scale > 0).any())
    for w in wide:
        assert bool((w[:14, :, 64:] == FILL).all()) and bool((w[14] == FILL).all())
    # without a gate there is no gated output, and out is the same
    alone, none, _ = run_bn(case, L, BF, ss=ss)
    assert none is None and torch.equal(alone, out)


# -- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_the_fused_launch_refuses_bad_arguments_before_the_launch():
    from drn_amd import _lib, ops
    index, wcodes, wscales, wpos, pq, pv, vids = exact_case(64, 32, 16, 3)
    out, gated = torch.zeros(14, 12, 16, device=DEV), torch.zeros(14, 12, 16, device=DEV)
    gate = torch.ones(14, 16, device=DEV)
    args = lambda **kw: dict(dict(codes=index.codes, scales=index.scales, pos=index.pos, pad_row=38, prop_off=index.prop_off, wcodes=wcodes,
                                  wscales=wscales, wpos=wpos, pq=pq, pv=pv, vids=vids, ss=None, gate=gate, out=out, gated=gated, L=12, C=64,
                                  P=32), **kw)
    bad = pq.cpu().clone()
    bad[9] = 2
    with pytest.raises(_lib.DrnError, match="pair 9 reads sentence 2 of 2"):
        ops.conv0_mx8_bn(**args(pq_host=bad))
    for kw in (dict(pq=pq.long()), dict(pv=pv.long()), dict(vids=vids.long()), dict(prop_off=index.prop_off.long())):
        with pytest.raises(_lib.DrnError, match="int32"):
            ops.conv0_mx8_bn(**args(**kw))
    with pytest.raises(_lib.DrnError, match="multiples of 32"):
        ops.conv0_mx8_bn(**args(C=48))
    with pytest.raises(_lib.DrnError, match="multiples of 32"):
        ops.conv0_mx8_bn(**args(P=16, pos=index.pos[:, :16], wpos=wpos[:, :, :16].contiguous()))
    with pytest.raises(_lib.DrnError, match="multiple of 16"):
        ops.conv0_mx8_bn(**args(wcodes=wcodes[:, :, :8].contiguous(), wscales=wscales[:, :, :8].contiguous(), wpos=wpos[:, :8].contiguous(),
                                out=out[:, :, :8].contiguous(), gated=gated[:, :, :8].contiguous(), gate=gate[:, :8].contiguous()))
    with pytest.raises(_lib.DrnError, match="out must be"):
        ops.conv0_mx8_bn(**args(out=None))
    with pytest.raises(_lib.DrnError, match="gate and gated must come together"):
        ops.conv0_mx8_bn(**args(gate=None))
    with pytest.raises(_lib.DrnError, match="gate and gated must come together"):
        ops.conv0_mx8_bn(**args(gated=None))
    with pytest.raises(_lib.DrnError, match="gate must be"):
        ops.conv0_mx8_bn(**args(gate=gate[:2]))                                              # (one row per pair, not per sentence)
    with pytest.raises(_lib.DrnError, match="ss must be"):
        ops.conv0_mx8_bn(**args(ss=torch.zeros(16, device=DEV)))
    torch.cuda.synchronize()
    assert not out.any() and not gated.any()


# -- 5. the search -----------------------------------------------------------------------------------------------------------------------------

def grounders(**kw):
    from drn_amd import Grounder
    m = shared()[0]
    return Grounder(m, conv0="mxfp8", fused=True, **kw), Grounder(m, conv0="mxfp8", **kw)


def test_the_new_path_is_taken():
    """fused=True: one conv0_mx8_bn per chunk, no conv0_mx8, no gather, one set of gated weights per search; fused=False: today's tags."""
    m, store, q, (tok, qlen), _ = shared()
    fused, unfused = grounders(top_k=6)

    def expect(tags, chunks):
        assert tags.count("conv0_mx8_bn") == chunks and "conv0_mx8" not in tags and tags.count("gate_quantize_weights_mx8") == 1, tags
        assert "gate_gather_packed_q8" not in tags and "gate_gather_packed" not in tags and "quantize_rows_mx8" not in tags
    expect(launch_tags(lambda: fused.search(tok, qlen, q, per_video=2, chunk=3)), 3)
    expect(launch_tags(lambda: fused.search(tok, qlen, q, candidates=[[1, 4, 6], [], [0, 6, 3, 5, 2]], pairs=3)), 3)
    expect(launch_tags(lambda: fused.search(tok, qlen, q, videos=["vid2", "vid5"], per_video=2)), 1)
    expect(launch_tags(lambda: fused.ground_stored(tok, qlen, q, ["vid2", "vid5", "vid2"], pairs=2)), 2)
    tags = launch_tags(lambda: unfused.search(tok, qlen, q, per_video=2, chunk=3))
    assert tags.count("conv0_mx8") == 3 and "conv0_mx8_bn" not in tags and tags.count("gate_quantize_weights_mx8") == 1


@pytest.mark.parametrize("dim", [64, 500])
def test_fused_conv0_outputs_are_the_oracle_through_batchnorm_relu_and_gate(dim):
    """forward_heads_packed(conv0="mxfp8") inside fused_eval() with taps on: conv0's (out, gated) against the oracle carried through the
    affine map, the ReLU and the level-1 gate in float64, with section 3's tolerance (no 2^-8 |ref| of a rounded raw).  21 pairs x
    T = 32 rows: three tiles, the second and the third holding two sentences.  dim = 500: Dp = 512, twelve zero columns."""
    from drn_amd import SearchIndex
    from drn_amd import functional as DF
    from drn_amd.index import mx8_conv0_reference, mx8_gate_weights
    if dim == 64:
        m, store, q, (tok, qlen), _ = shared()
    else:
        m, store = boosted(tiny_model(T, dim, BF)), store_of(dim, BF)
        q = SearchIndex.build(m, store, quantize="mxfp8")
        tok, qlen = sentences(7)
    conv, bn = conv0_parts(m)
    vids = dev_vids([4, 1, -1, 3, 0, 7, 6])
    pair = torch.arange(S * 7, dtype=torch.int32, device=DEV)
    pq, pv = torch.div(pair, 7, rounding_mode="floor"), torch.remainder(pair, 7)
    m.taps = {}
    try:
        with torch.no_grad(), DF.fused_eval(True):
            gates = [g.contiguous() for g in m.encode_query(tok, qlen)]
            tags = launch_tags(lambda: m.forward_heads_packed(q, vids, pq, pv, gates, T, conv0="mxfp8"))
        out, gated = m.taps["conv0_mx8"]
    finally:
        m.taps = None
    assert tags.count("conv0_mx8_bn") == 1 and "conv0_mx8" not in tags and out.dtype == gated.dtype == BF
    W = conv.weight.detach().cpu()
    wcodes, wscales = mx8_gate_weights(W, gates[0].cpu(), q.D, q.Dp)
    wpos = W[:, q.D:, :].permute(2, 0, 1).to(BF).contiguous()
    case = (q, wcodes, wscales, wpos, pq, pv, vids)
    ref = mx8_conv0_reference(*case, T)
    mag_bound = raw_bound(*case, T, ref) - 2.0 ** -8 * ref.abs()
    f64 = lambda t: t.detach().double().cpu()
    scale = f64(bn.weight) / torch.sqrt(f64(bn.running_var) + bn.eps)
    shift = f64(bn.bias) + ((f64(conv.bias) if conv.bias is not None else 0.0) - f64(bn.running_mean)) * scale
    want = torch.relu(ref * scale + shift)
    tol = scale.abs() * mag_bound + 2.0 ** -8 * want + 2.0 ** -20 * ((ref * scale).abs() + shift.abs())
    err = (f64(out) - want).abs()
    print("fused conv0 out: largest error / tolerance = %.4f" % float((err / tol.clamp_min(1e-30)).max()))
    assert bool((err <= tol).all()), float((err / tol.clamp_min(1e-30)).max())
    g1 = f64(gates[1])[pq.long().cpu()][:, None, :]
    want_g = want * g1
    tol_g = (g1.abs() * tol) * (1 + 2.0 ** -7) + 2.0 ** -8 * want_g.abs()
    err_g = (f64(gated) - want_g).abs()
    assert bool((err_g <= tol_g).all()), float((err_g / tol_g.clamp_min(1e-30)).max())
    assert float(want.max()) > 0 and bool((want == 0).any()) and not torch.equal(out[0], out[7])


def test_the_fused_search_is_invariant_to_how_it_is_cut():
    m, store, q, (tok, qlen), _ = shared()
    grounder = grounders(top_k=5)[0]
    kw = dict(top_k=10, per_video=3)
    full = grounder.search(tok, qlen, q, **kw)
    assert int(full.n.min()) > 0
    for chunk in (1, 3, 7):
        same_hits(grounder.search(tok, qlen, q, chunk=chunk, **kw), full, chunk)
    everything = list(range(len(q)))
    same_hits(grounder.search(tok, qlen, q, candidates=[everything] * S, **kw), full, "candidates = all")
    same_hits(grounder.search(tok, qlen, q, candidates=[everything] * S, pairs=4, chunk=3, **kw), full, "candidates = all, cut small")
    deep = grounder.search(tok, qlen, q, top_k=3 * len(q), per_video=3)
    lists = [[1, 4, 6], [], [0, 6, 3, 5, 2]]
    short = grounder.search(tok, qlen, q, candidates=lists, top_k=3 * len(q), per_video=3)
    for s in range(S):
        keep = [i for i in range(int(deep.n[s])) if int(deep.video[s, i]) in lists[s]]
        assert int(short.n[s]) == len(keep), s
        for f in ("seg", "score", "video", "level", "rank"):
            assert torch.equal(getattr(short, f)[s, :len(keep)], getattr(deep, f)[s][keep]), (s, f)
    assert short.n.tolist()[1] == 0 and short.n.tolist()[0] > 0


def test_fused_graph_replay_equals_eager_with_one_capture_per_signature():
    from drn_amd import Grounder
    m, store, q, (tok, qlen), (tok2, qlen2) = shared()
    eager, graphed = grounders(top_k=6)[0], Grounder(m, top_k=6, graph=True, conv0="mxfp8", fused=True)
    kw = dict(per_video=2, chunk=3)
    first = graphed.search(tok, qlen, q, **kw)
    same_hits(first, eager.search(tok, qlen, q, **kw), "first search")
    second = graphed.search(tok2, qlen2, q, **kw)
    same_hits(second, eager.search(tok2, qlen2, q, **kw), "other sentences")
    assert graphed.captures == 1 and not torch.equal(second.score, first.score)
    same_hits(graphed.search(tok, qlen, q, **kw), first, "the first sentences again")
    lists = [[1, 4, 6], [2], [0, 6, 3, 5, 2]]
    same_hits(graphed.search(tok, qlen, q, candidates=lists, per_video=2), eager.search(tok, qlen, q, candidates=lists, per_video=2), "pairs")
    same_hits(graphed.search(tok2, qlen2, q, candidates=lists, per_video=2), eager.search(tok2, qlen2, q, candidates=lists, per_video=2),
              "pairs, other sentences")
    assert graphed.captures == 2


def test_fused_ground_stored_agrees_with_the_search_of_one_video():
    from drn_amd import Grounder, evaluate_search
    m, store, q, (tok, qlen), (tok2, qlen2) = shared()
    grounder = grounders(top_k=5)[0]
    names = ["vid2", "vid5", "vid2"]
    mom = grounder.ground_stored(tok, qlen, q, names, T=T)
    assert int(mom.n.min()) > 0
    for s, name in enumerate(names):
        hits = grounder.search(tok, qlen, q, videos=[name], per_video=5, top_k=5, T=T)
        n = int(mom.n[s])
        assert int(hits.n[s]) == n and torch.equal(hits.seg[s, :n], mom.seg[s, :n]) and torch.equal(hits.score[s, :n], mom.score[s, :n]), s
        assert torch.equal(hits.level[s, :n], mom.level[s, :n]) and hits.rank[s, :n].tolist() == list(range(n))
    same = grounder.ground_stored(tok, qlen, q, names, T=T, pairs=2)
    for f in MOMENT:
        assert torch.equal(getattr(same, f), getattr(mom, f)), f
    gt = mom.seg[:, 0].double().cpu()
    batches = [(names, tok, qlen, gt), (["vid5", "vid6", "vid3"], tok2, qlen2, torch.tensor([[0.0, 0.5], [0.125, 0.625], [0.375, 1.0]]))]
    kw = dict(ious=(0.3, 0.5, 0.7), topks=(1, 5, 10), per_video=2)
    a = evaluate_search(grounder, batches, q, chunk=3, **kw)
    b = evaluate_search(Grounder(m, top_k=5, graph=True, conv0="mxfp8", fused=True), batches, q, **kw)
    assert a.first_hits.tolist() == b.first_hits.tolist() and a.n == 6 and (a.first_hits < 10).any()


AGREEMENT_BIAS = -6.5            # see agreement_fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_mx8fused_scores.json")


def agreement_fixture():
    """The tiny bf16 model and small_store of the other tests, but NOT boosted: `boosted` (cls weight x 30) drives every first score to
    1.0 against 0.9999999 for the second, and even the plain classifier at bias 0.5 leaves them at 0.9995 against 0.9994 -- closer than
    one bf16 rounding, so equal first videos would be a coin toss on the reference path alone.  A classifier bias of -6.5 moves the
    logits of this model (6 to 8 at bias 0.5) to the steep part of the sigmoid; nothing else is changed."""
    from drn_amd import SearchIndex
    from test_search_gpu import small_store
    m = tiny_model(T, D, BF)
    with torch.no_grad():
        m.fcos.head.cls_logits.bias.fill_(AGREEMENT_BIAS)
    return m, SearchIndex.build(m, small_store(BF), quantize="mxfp8")


def test_the_fused_and_the_unfused_mode_name_the_same_first_video():
    """A condition, not bitwise: the unfused mode rounds raw to bf16 before the affine map, the fused one does not.  For every sentence
    of the fixture (sentences(7) and sentences(11), one hit per video) the first hits of the two modes name the same video; the largest
    score difference is printed (scripts/bench_search.py --mx-conv0-fused records it on its own index: profiles/
    search_mx8conv_fused_bench.json, agreement), and nothing tighter than the equal first video is asserted.  The unfused mode's first
    and second hits are those recorded in tests/golden/search_mx8fused_scores.json -- the same videos, scores within 2^-12, a sixteenth
    of the 2^-8 gap that tests/test_search_mx8fused_cpu.py demands of the record -- so the condition is one the reference path carries."""
    import json
    from drn_amd import Grounder
    m, q = agreement_fixture()
    golden = json.load(open(GOLDEN))
    assert golden["bias"] == AGREEMENT_BIAS
    fused, unfused = Grounder(m, top_k=6, conv0="mxfp8", fused=True), Grounder(m, top_k=6, conv0="mxfp8")
    worst = 0.0
    for seed in (7, 11):
        tok, qlen = sentences(seed)
        a, b = fused.search(tok, qlen, q, per_video=1, top_k=2), unfused.search(tok, qlen, q, per_video=1, top_k=2)
        rec = golden["sentences"][str(seed)]
        assert int(a.n.min()) >= 2 and int(b.n.min()) >= 2
        assert b.video.tolist() == rec["video"], (seed, b.video.tolist(), rec["video"])
        assert float((b.score.double().cpu() - torch.tensor(rec["score"], dtype=torch.float64)).abs().max()) <= 2.0 ** -12, seed
        assert a.video[:, 0].tolist() == b.video[:, 0].tolist(), (seed, a.video.tolist(), b.video.tolist())
        worst = max(worst, float((a.score[:, 0].double() - b.score[:, 0].double()).abs().max()))
    print("fused vs unfused conv0=\"mxfp8\": largest |first score difference| = %.3e" % worst)


def test_the_fused_mode_refuses_what_the_mode_refuses_before_any_launch():
    from drn_amd import Grounder, SearchIndex, _lib
    from test_search_gpu import small_store
    m, store, q, (tok, qlen), _ = shared()
    grounder = grounders(top_k=6)[0]
    plain = SearchIndex.build(m, store)
    m32, store32 = boosted(tiny_model(T, D, torch.float32)), small_store()
    q32 = SearchIndex.build(m32, store32, quantize="mxfp8")

    def refused():
        for g, where, what in ((grounder, store, "not a feature store"), (grounder, plain, "this one is plain"),
                               (Grounder(m32, conv0="mxfp8", fused=True), q32, "needs a bfloat16 model")):
            with pytest.raises(_lib.DrnError, match=what):
                g.search(tok, qlen, where)
            with pytest.raises(_lib.DrnError, match=what):
                g.search(tok, qlen, where, candidates=[[0], [1], [2]])
            with pytest.raises(_lib.DrnError, match=what):
                g.ground_stored(tok, qlen, where, [0, 1, 2])
    assert launch_tags(refused) == []
