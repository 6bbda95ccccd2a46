"""conv0 of a search on block-scaled FP8 MFMAs, on the device: drn_gate_quantize_weights_mx8 against its definition byte for byte,
drn_conv0_mx8 against the float64 oracle (drn_amd.index.mx8_conv0_reference, pinned against torch's conv1d by
tests/test_search_mx8conv_cpu.py) -- EQUAL on exact data, which is what establishes the operand and scale lane maps of
v_mfma_scale_f32_16x16x128_f8f6f4, and within a derived bound on random data -- and Grounder(conv0="mxfp8") end to end: conv0's
outputs against the oracle, the invariances of the search field for field, the launches it makes and the ones it refuses."""
import functools
import types

import pytest
import torch

from test_grounding_engine_gpu import DEV, tiny_model
from test_search_gpu import D, S, T, boosted, dev_vids, same_hits, sentences, small_store
from test_search_index_gpu import packed_case, store_of

pytestmark = pytest.mark.gpu
MOMENT = ("seg", "score", "level", "index", "n")
BF = torch.bfloat16


def abs_index(index):
    """The index with every value replaced by its magnitude (an e4m3 code's sign is bit 7): the oracle on it gives sum |a * b|."""
    return types.SimpleNamespace(codes=index.codes & 0x7f, scales=index.scales, pos=index.pos.abs() if index.pos is not None else None,
                                 prop_off=index.prop_off, pad_row=index.pad_row)


# -- 4. the weights kernel against the definition ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Dp,D", [(64, 64), (160, 160), (160, 148)])
def test_gate_quantize_weights_equals_the_definition_byte_for_byte(Dp, D):
    """S = 3, Cout = 16, gate magnitudes from 2^-12 to 2^12; w is the feature columns of a wider tap-major copy (row stride D + 32);
    wcodes / wscales are column slices of buffers 16 and 3 bytes wider, and what lies past a row keeps its fill."""
    from drn_amd import ops
    from drn_amd.index import mx8_gate_weights
    g = torch.Generator().manual_seed(Dp + D)
    Sn, Cout, P = 3, 16, 32
    W = torch.randn(Cout, D + P, 3, generator=g)
    gate = torch.randn(Sn, D, generator=g) * torch.exp2(torch.linspace(-12, 12, Sn * D).view(Sn, D))
    gwide = torch.full((Sn, D + 4), 3.0, device=DEV)
    gwide[:, :D] = gate.to(DEV)
    w = W.permute(2, 0, 1).contiguous().to(DEV)
    codes = torch.full((Sn, 3, Cout, Dp + 16), 0xa5, dtype=torch.uint8, device=DEV)
    scales = torch.full((Sn, 3, Cout, Dp // 32 + 3), 0xa5, dtype=torch.uint8, device=DEV)
    ops.gate_quantize_weights_mx8(w[:, :, :D], gwide[:, :D], D, Dp, codes[..., :Dp], scales[..., :Dp // 32])
    want_c, want_s = mx8_gate_weights(W, gate, D, Dp)
    got_c, got_s = codes.cpu(), scales.cpu()
    bad = (got_s[..., :Dp // 32] != want_s).nonzero()
    assert bad.numel() == 0, ("scales", bad[:8].tolist())
    bad = (got_c[..., :Dp] != want_c).nonzero()
    assert bad.numel() == 0, ("codes", bad[:8].tolist())
    assert bool((got_c[..., Dp:] == 0xa5).all()) and bool((got_s[..., Dp // 32:] == 0xa5).all())
    assert int(want_s.max()) - int(want_s.min()) >= 16
    if D < Dp:
        assert not want_c[..., D:].any()


# -- 5. exact data: EQUAL to the oracle ------------------------------------------------------------------------------------------------------

E4M3 = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44}          # the e4m3fn codes of 0, 1, 2, 3; bit 7 is the sign


def exact_codes(shape, g):
    v = torch.randint(-3, 4, shape, generator=g)
    table = torch.tensor([E4M3[abs(i)] | (0x80 if i < 0 else 0) for i in range(-3, 4)], dtype=torch.uint8)
    return table[v + 3]


def exact_case(Dp, P, Cout, seed):
    """packed_case's tables with integer data: codes and weight codes from {0, +-1, +-2, +-3}, a scale exponent from -2..2 per block on
    both sides, position values and weights small integers -- every product and every partial sum is a multiple of 2^-4 below 2^20,
    exact in fp32 in any order.  Independent draws for the two operands: a swapped row / column, or a scale byte applied to another
    block or lane, changes the result.  codes / scales / pos are column slices of wider buffers."""
    _, off, _, pq, pv, vids, _, _ = packed_case(torch.float32, 64, 0, 0)
    g = torch.Generator().manual_seed(seed)
    codes = torch.full((39, Dp + 16), 0x7e, dtype=torch.uint8)
    scales = torch.full((39, Dp // 32 + 3), 0xfe, dtype=torch.uint8)
    codes[:, :Dp] = exact_codes((39, Dp), g)
    scales[:, :Dp // 32] = torch.randint(125, 130, (39, Dp // 32), generator=g).to(torch.uint8)
    pos = torch.full((39, P + 8), 7.0).to(BF)
    pos[:, :P] = torch.randint(-3, 4, (39, P), generator=g).to(BF)
    wcodes = exact_codes((2, 3, Cout, Dp), g)
    wscales = torch.randint(125, 130, (2, 3, Cout, Dp // 32), generator=g).to(torch.uint8)
    wpos = torch.randint(-3, 4, (3, Cout, P), generator=g).to(BF)
    dev = lambda t: t.to(DEV)
    index = types.SimpleNamespace(codes=dev(codes)[:, :Dp], scales=dev(scales)[:, :Dp // 32], pos=dev(pos)[:, :P] if P else None,
                                  prop_off=off, pad_row=38)
    return index, dev(wcodes), dev(wscales), dev(wpos) if P else None, pq, pv, vids


def run_conv0(index, wcodes, wscales, wpos, pq, pv, vids, L, dtype, **kw):
    from drn_amd import ops
    Dp, P = int(wcodes.shape[3]), 0 if wpos is None else int(wpos.shape[2])
    raw = torch.full((int(pq.numel()), L, int(wcodes.shape[2])), 7.0, dtype=dtype, device=DEV)
    ops.conv0_mx8(index.codes, index.scales, index.pos, index.pad_row, index.prop_off, wcodes, wscales, wpos, pq, pv, vids, raw, L, Dp, P, **kw)
    return raw


@pytest.mark.parametrize("Cout", [16, 48])
@pytest.mark.parametrize("P", [0, 32])
@pytest.mark.parametrize("Dp", [64, 160, 384])
def test_conv0_on_exact_data_equals_the_oracle(Dp, P, Cout):
    """Dp = 64: half a K step; 160: one step and a quarter; 384: three.  L = 12 is packed_case's own; L = 5 cuts the videos; L = 20 and
    L = 70 take the kernel's 32- and 64-row tiles (70: two tiles of a pair, the second partial)."""
    from drn_amd.index import mx8_conv0_reference
    index, wcodes, wscales, wpos, pq, pv, vids = exact_case(Dp, P, Cout, 7 * Dp + P + Cout)
    for L in (12, 5) + ((20, 70) if (Dp, Cout) == (160, 48) else ()):
        raw = run_conv0(index, wcodes, wscales, wpos, pq, pv, vids, L, torch.float32, pq_host=pq.cpu())
        want = mx8_conv0_reference(index, wcodes, wscales, wpos, pq, pv, vids, L)
        got = raw.double().cpu()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (L, bad.shape[0], bad[:6].tolist(), got[want != got][:6].tolist(), want[want != got][:6].tolist())
        assert float(want.abs().max()) > 64 and not torch.equal(want[0], want[7])          # (two sentences with different weights)
        assert torch.equal(got[2], got[3]) and torch.equal(got[2], got[5])                  # slot -1, the empty video, Nv: the pad row


# -- 6. random data within the derived bound ---------------------------------------------------------------------------------------------------

def random_case(Dp, P, Cout, seed):
    from drn_amd.index import mx8_gate_weights, mx8_quantize
    _, off, _, pq, pv, vids, _, _ = packed_case(torch.float32, 64, 0, 0)
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(39, Dp, generator=g) * torch.exp2(torch.randint(-4, 5, (39, 1), generator=g).float())
    codes, scales = mx8_quantize(rows)
    pos = torch.randn(39, P, generator=g).to(BF)
    W = torch.randn(Cout, Dp + P, 3, generator=g) * 0.05
    gate = torch.randn(2, Dp, generator=g)
    wcodes, wscales = mx8_gate_weights(W, gate, Dp, Dp)
    wpos = W[:, Dp:, :].permute(2, 0, 1).to(BF).contiguous()
    dev = lambda t: t.to(DEV)
    index = types.SimpleNamespace(codes=dev(codes), scales=dev(scales), pos=dev(pos), prop_off=off, pad_row=38)
    return index, dev(wcodes), dev(wscales), dev(wpos), pq, pv, vids


def raw_bound(index, wcodes, wscales, wpos, pq, pv, vids, L, ref):
    """2^-8 |ref| + K 2^-23 sum |a b|, K = 3 (Dp + P) terms: the bf16 rounding of the result, and the bound of an fp32 summation of K
    exact products in any order (each of the K - 1 additions rounds by at most 2^-24 of a partial sum that sum |a b| bounds)."""
    from drn_amd.index import mx8_conv0_reference
    K = 3 * (int(wcodes.shape[3]) + (0 if wpos is None else int(wpos.shape[2])))
    mag = mx8_conv0_reference(abs_index(index), wcodes & 0x7f, wscales, None if wpos is None else wpos.abs(), pq, pv, vids, L)
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag


def test_conv0_on_random_data_is_within_the_derived_bound():
    """Dp = 384, P = 256, Cout = 64, L = 40 (64-row tiles), raw in bf16.  Observed on an MI355X: the largest error is 0.76 of the
    bound (printed here; profiles/search_mx8conv_bench.json, bound_ratio)."""
    from drn_amd.index import mx8_conv0_reference
    case = random_case(384, 256, 64, 11)
    L = 40
    raw = run_conv0(*case, L, BF)
    ref = mx8_conv0_reference(*case, L)
    ratio = ((raw.double().cpu() - ref).abs() / raw_bound(*case, L, ref)).max()
    print("conv0_mx8 bf16: largest |raw - ref| / bound = %.4f" % float(ratio))
    assert float(ratio) <= 1.0
    assert float(ref.abs().max()) > 1.0


# -- 7. refusals -------------------------------------------------------------------------------------------------------------------------------

def test_conv0_refuses_bad_arguments_before_the_launch():
    from drn_amd import _lib, ops
    index, wcodes, wscales, wpos, pq, pv, vids = exact_case(64, 32, 16, 3)
    raw = torch.zeros(14, 12, 16, device=DEV)
    args = lambda **kw: dict(dict(codes=index.codes, scales=index.scales, pos=index.pos, pad_row=38, prop_off=index.prop_off, wcodes=wcodes,
                                  wscales=wscales, wpos=wpos, pq=pq, pv=pv, vids=vids, raw=raw, L=12, C=64, P=32), **kw)
    bad = pq.cpu().clone()
    bad[9] = 2
    with pytest.raises(_lib.DrnError, match="pair 9 reads sentence 2 of 2"):
        ops.conv0_mx8(**args(pq_host=bad))
    for kw in (dict(pq=pq.long()), dict(pv=pv.long()), dict(vids=vids.long()), dict(prop_off=index.prop_off.long())):
        with pytest.raises(_lib.DrnError, match="int32"):
            ops.conv0_mx8(**args(**kw))
    with pytest.raises(_lib.DrnError, match="multiples of 32"):
        ops.conv0_mx8(**args(C=48))
    with pytest.raises(_lib.DrnError, match="multiples of 32"):
        ops.conv0_mx8(**args(P=16, pos=index.pos[:, :16], wpos=wpos[:, :, :16].contiguous()))
    with pytest.raises(_lib.DrnError, match="multiple of 16"):
        ops.conv0_mx8(**args(wcodes=wcodes[:, :, :8].contiguous(), wscales=wscales[:, :, :8].contiguous(), wpos=wpos[:, :8].contiguous(),
                             raw=raw[:, :, :8].contiguous()))
    torch.cuda.synchronize()
    assert not raw.any()


# -- 8-11. the search ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shared():
    """The boosted tiny bf16 model, small_store(bf16), its quantised index, and two sets of sentences: built once, changed by no test."""
    from drn_amd import SearchIndex
    m, store = boosted(tiny_model(T, D, BF)), small_store(BF)
    return m, store, SearchIndex.build(m, store, quantize="mxfp8"), sentences(7), sentences(11)


def conv0_parts(m):
    from drn_amd.model.basic_blocks import conv_bn
    return conv_bn(m.backbone_net.forward_conv0, "test")


@pytest.mark.parametrize("dim", [64, 500])
def test_conv0_outputs_are_the_oracle_through_batchnorm_relu_and_gate(dim):
    """forward_heads_packed(conv0="mxfp8") with taps on: conv0's (out, gated) against relu(raw * scale + shift) and that times the
    level-1 gate, raw from the oracle on the host definition of the gated weights.  Tolerance: test 6's bound on raw carried through
    the affine map (|scale| times it), 2^-8 of the result for its own bf16 rounding, and 2^-20 of the affine map's terms for its fp32
    arithmetic; the gated output the same times |gate| plus its own rounding.  dim = 500: Dp = 512, twelve zero columns."""
    from drn_amd import SearchIndex
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
        with torch.no_grad():
            gates = [g.contiguous() for g in m.encode_query(tok, qlen)]
            m.forward_heads_packed(q, vids, pq, pv, gates, T, conv0="mxfp8")
        out, gated = m.taps["conv0_mx8"]
        level0 = m.taps["backbone_net.forward_conv0"]
    finally:
        m.taps = None
    assert torch.equal(level0.permute(0, 2, 1), out) and out.dtype == gated.dtype == BF
    W = conv.weight.detach().cpu()
    wcodes, wscales = mx8_gate_weights(W, gates[0].cpu(), q.D, q.Dp)
    wpos = W[:, q.D:, :].permute(2, 0, 1).to(BF).contiguous()
    case = (q, wcodes, wscales, wpos, pq, pv, vids)
    ref = mx8_conv0_reference(*case, T)
    bound = raw_bound(*case, T, ref)
    f64 = lambda t: t.detach().double().cpu()
    scale = f64(bn.weight) / torch.sqrt(f64(bn.running_var) + bn.eps)
    shift = f64(bn.bias) + ((f64(conv.bias) if conv.bias is not None else 0.0) - f64(bn.running_mean)) * scale
    want = torch.relu(ref * scale + shift)
    tol = scale.abs() * bound + 2.0 ** -8 * want + 2.0 ** -20 * ((ref * scale).abs() + shift.abs())
    err = (f64(out) - want).abs()
    print("conv0 out: largest error / tolerance = %.4f" % float((err / tol.clamp_min(1e-30)).max()))
    assert bool((err <= tol).all()), float((err / tol.clamp_min(1e-30)).max())
    g1 = f64(gates[1])[pq.long().cpu()][:, None, :]
    want_g = want * g1
    tol_g = (g1.abs() * tol) * (1 + 2.0 ** -7) + 2.0 ** -8 * want_g.abs()
    err_g = (f64(gated) - want_g).abs()
    assert bool((err_g <= tol_g).all()), float((err_g / tol_g.clamp_min(1e-30)).max())
    assert float(want.max()) > 0 and bool((want == 0).any()) and not torch.equal(out[0], out[7])


def test_the_search_is_invariant_to_how_it_is_cut():
    from drn_amd import Grounder
    m, store, q, (tok, qlen), _ = shared()
    grounder = Grounder(m, top_k=5, conv0="mxfp8")
    kw = dict(top_k=10, per_video=3)
    full = grounder.search(tok, qlen, q, **kw)
    assert int(full.n.min()) > 0
    for chunk in (1, 3, 7):
        same_hits(grounder.search(tok, qlen, q, chunk=chunk, **kw), full, chunk)
    everything = list(range(len(q)))
    same_hits(grounder.search(tok, qlen, q, candidates=[everything] * S, **kw), full, "candidates = all")
    same_hits(grounder.search(tok, qlen, q, candidates=[everything] * S, pairs=4, chunk=3, **kw), full, "candidates = all, cut small")
    # a shortlist: the full ranking (deep enough to hold every moment) filtered to the listed videos
    deep = grounder.search(tok, qlen, q, top_k=3 * len(q), per_video=3)
    lists = [[1, 4, 6], [], [0, 6, 3, 5, 2]]
    short = grounder.search(tok, qlen, q, candidates=lists, top_k=3 * len(q), per_video=3)
    for s in range(S):
        keep = [i for i in range(int(deep.n[s])) if int(deep.video[s, i]) in lists[s]]
        assert int(short.n[s]) == len(keep), s
        for f in ("seg", "score", "video", "level", "rank"):
            assert torch.equal(getattr(short, f)[s, :len(keep)], getattr(deep, f)[s][keep]), (s, f)
    assert short.n.tolist()[1] == 0 and short.n.tolist()[0] > 0
    assert m.fcos.box_selector_test.device_only is False


def test_graph_replay_equals_eager_with_one_capture():
    from drn_amd import Grounder
    m, store, q, (tok, qlen), (tok2, qlen2) = shared()
    eager, graphed = Grounder(m, top_k=6, conv0="mxfp8"), Grounder(m, top_k=6, graph=True, conv0="mxfp8")
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
    # the default mode on the same index is another signature
    plain = Grounder(m, top_k=6, graph=True)
    assert not torch.equal(plain.search(tok, qlen, q, **kw).score, first.score)


def test_ground_stored_agrees_with_the_search_of_one_video():
    """Sentence s grounded in video names[s]: its moments are the hits of a search of that one video with per_video = top_k, in the
    same order (score descending, then the NMS rank); the boosted model leaves no pair without a candidate."""
    from drn_amd import Grounder, evaluate_search
    m, store, q, (tok, qlen), (tok2, qlen2) = shared()
    grounder = Grounder(m, top_k=5, conv0="mxfp8")
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
    a, b = evaluate_search(grounder, batches, q, chunk=3, **kw), evaluate_search(Grounder(m, top_k=5, graph=True, conv0="mxfp8"), batches, q, **kw)
    assert a.first_hits.tolist() == b.first_hits.tolist() and a.n == 6 and (a.first_hits < 10).any()


def launch_tags(run):
    from drn_amd import ops
    ops.kernel_timer = []
    try:
        run()
        return [t[0] for t in ops.kernel_timer]
    finally:
        ops.kernel_timer = None


def test_the_new_path_is_taken():
    from drn_amd import Grounder
    m, store, q, (tok, qlen), _ = shared()
    mx, default = Grounder(m, top_k=6, conv0="mxfp8"), Grounder(m, top_k=6)
    hits = {}
    tags = launch_tags(lambda: hits.update(mx=mx.search(tok, qlen, q, per_video=2, chunk=3)))
    assert tags.count("conv0_mx8") == 3 and tags.count("gate_quantize_weights_mx8") == 1             # 3 chunks, ONE set of weights
    assert "gate_gather_packed_q8" not in tags and "gate_gather_packed" not in tags and "quantize_rows_mx8" not in tags
    tags = launch_tags(lambda: hits.update(default=default.search(tok, qlen, q, per_video=2, chunk=3)))
    assert tags.count("gate_gather_packed_q8") == 3 and "conv0_mx8" not in tags and "gate_quantize_weights_mx8" not in tags
    assert not torch.equal(hits["mx"].score, hits["default"].score)
    tags = launch_tags(lambda: mx.search(tok, qlen, q, candidates=[[1, 4, 6], [], [0, 6, 3, 5, 2]], pairs=3))
    assert tags.count("conv0_mx8") == 3 and tags.count("gate_quantize_weights_mx8") == 1 and "gate_gather_packed_q8" not in tags
    tags = launch_tags(lambda: mx.ground_stored(tok, qlen, q, ["vid2", "vid5", "vid2"], pairs=2))
    assert tags.count("conv0_mx8") == 2 and tags.count("gate_quantize_weights_mx8") == 1 and "gate_gather_packed_q8" not in tags


def test_what_the_mode_refuses_and_what_it_follows():
    from drn_amd import Grounder, SearchIndex, _lib
    m, store, q, (tok, qlen), _ = shared()
    with pytest.raises(_lib.DrnError, match="conv0 must be None or"):
        Grounder(m, conv0="int4")
    grounder = Grounder(m, top_k=6, conv0="mxfp8")
    plain = SearchIndex.build(m, store)
    m32, store32 = boosted(tiny_model(T, D, torch.float32)), small_store()
    q32 = SearchIndex.build(m32, store32, quantize="mxfp8")

    def refused():
        for g, where, what in ((grounder, store, "not a feature store"), (grounder, plain, "this one is plain"),
                               (Grounder(m32, conv0="mxfp8"), q32, "needs a bfloat16 model")):
            with pytest.raises(_lib.DrnError, match=what):
                g.search(tok, qlen, where)
            with pytest.raises(_lib.DrnError, match=what):
                g.search(tok, qlen, where, candidates=[[0], [1], [2]])
            with pytest.raises(_lib.DrnError, match=what):
                g.ground_stored(tok, qlen, where, [0, 1, 2])
        with pytest.raises(_lib.DrnError, match="conv0 must be None or"):
            with torch.no_grad():
                m.forward_heads_packed(q, dev_vids([0]), dev_vids([0]), dev_vids([0]), [None] * 3, T, conv0="int4")
    assert launch_tags(refused) == []
    # a stale index still raises before any launch; an in-place change of conv0's weight reaches the next search, eager and replayed
    m2 = boosted(tiny_model(T, D, BF))
    q2 = SearchIndex.build(m2, store, quantize="mxfp8")
    eager, graphed = Grounder(m2, top_k=6, conv0="mxfp8"), Grounder(m2, top_k=6, graph=True, conv0="mxfp8")
    before = eager.search(tok, qlen, q2, per_video=2)
    same_hits(graphed.search(tok, qlen, q2, per_video=2), before, "before the change")
    conv, _ = conv0_parts(m2)
    with torch.no_grad():
        conv.weight.mul_(1.5)
    after = eager.search(tok, qlen, q2, per_video=2)
    assert not torch.equal(after.score, before.score)
    same_hits(graphed.search(tok, qlen, q2, per_video=2), after, "after the change")
    same_hits(Grounder(m2, top_k=6, conv0="mxfp8").search(tok, qlen, q2, per_video=2), after, "a new grounder")
    with torch.no_grad():
        m2.prop_fc.bias.add_(0.1)

    def stale():
        for g in (eager, graphed):
            with pytest.raises(_lib.DrnError, match="stale"):
                g.search(tok, qlen, q2, per_video=2)
    assert launch_tags(stale) == []
