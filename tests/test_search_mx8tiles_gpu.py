"""The narrow tiles of the fused FP8 conv0 (drn_conv0_mx8_bn_tile, conv0_mx8_narrow_kernel) on the device: every
shipped tile writes bit for bit what the wide tile writes -- bare accumulators in fp32 and bf16 through BatchNorm, ReLU and the gate --,
and what the wide tile wrote at the commit that tests/golden/search_mx8_tile_digests.json names, EQUALS the float64
oracle on exact data, writes nothing outside its columns and does not depend on the order of the pairs; the chooser is a shipped tile, a
function of the grid alone and the rule DESIGN.md states; and Grounder(conv0="mxfp8", fused=True), which now runs conv0 on the chosen
tile, returns field for field the hits of the same search with the chooser held to the wide tile."""
import hashlib
import json
import os
import types

import pytest
import torch

from test_grounding_engine_gpu import DEV
from test_search_gpu import S, T, same_hits
from test_search_mx8conv_gpu import BF, MOMENT, conv0_parts, exact_case, launch_tags, random_case, shared
from test_search_mx8fused_gpu import FILL, INTERLEAVED, SHUFFLED, permuted, run_bn

pytestmark = pytest.mark.gpu


def narrow_tiles():
    from drn_amd import ops
    return [t for t in ops.CONV0_MX8_TILES if t != ops.CONV0_MX8_WIDE]


NARROW = narrow_tiles()
SORTED = torch.arange(14)
# (L, Cout, Dp, P, order of the pairs): with 14 pairs, L = 12 is M = 168 -- several pairs and both sentences inside one 64-row tile, M
# no multiple of any tile; L = 70: pairs straddle 64-, 128- and 256-row tiles; L = 300: a pair longer than any tile, taps across tile
# edges.  Cout = 16: fewer channels than any COLS; 80: one group of 64 and a remainder of 16; 272: remainder groups at 64, 128 and 256
# columns.  Dp = 160: a partial last 128-column step.  P = 0: no position steps.
GEOMETRIES = [pytest.param(L, Cout, Dp, P, order, id="L%d-Cout%d-Dp%d-P%d-%s" % (L, Cout, Dp, P, name))
              for L, Cout, Dp, P, order, name in ((12, 16, 64, 0, SORTED, "sorted"), (70, 272, 160, 32, INTERLEAVED, "interleaved"),
                                                  (300, 80, 384, 32, SHUFFLED, "shuffled"), (12, 80, 384, 0, INTERLEAVED, "interleaved"),
                                                  (70, 272, 64, 32, SHUFFLED, "shuffled"))]


def case_of(Dp, P, Cout, seed):
    """random_case (rounding everywhere: a changed summation order shows), without its position columns when P = 0."""
    index, wcodes, wscales, wpos, pq, pv, vids = random_case(Dp, max(P, 32), Cout, seed)
    if P == 0:
        index, wpos = types.SimpleNamespace(codes=index.codes, scales=index.scales, pos=None, prop_off=index.prop_off, pad_row=index.pad_row), None
    return index, wcodes, wscales, wpos, pq, pv, vids


def epilogue_of(Cout, seed):
    g = torch.Generator().manual_seed(seed)
    ss = torch.stack([torch.randn(Cout, generator=g) * 0.5, torch.randn(Cout, generator=g) * 2.0]).to(DEV)
    return ss, torch.randn(14, Cout + 8, generator=g).to(DEV)[:, :Cout]                     # (the gate's row stride above its row)


# -- 1. bit for bit the wide tile ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", NARROW, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("L,Cout,Dp,P,order", GEOMETRIES)
def test_a_narrow_tile_writes_the_wide_tiles_bits(tile, L, Cout, Dp, P, order):
    """fp32 with ss = None: the accumulators themselves; bf16 through ss and the gate: out and gated.  The oracle is the wide tile
    (tile=None: drn_conv0_mx8_bn) in the same process on the same operands; no tolerance."""
    from drn_amd import ops
    case = permuted(case_of(Dp, P, Cout, 3 * Dp + P + Cout + L), order)
    ss, gate = epilogue_of(Cout, L + Cout)
    want = run_bn(case, L, torch.float32)[0]
    got = run_bn(case, L, torch.float32, tile=tile)[0]
    assert torch.equal(got, want), (tile, int((got != want).sum()), (got != want).nonzero()[:4].tolist())
    assert float(want.abs().max()) > 1.0 and bool(torch.isfinite(want).all())
    assert torch.equal(run_bn(case, L, torch.float32, tile=ops.CONV0_MX8_WIDE)[0], want)     # (the wide tile through the new entry)
    wo, wg, _ = run_bn(case, L, BF, ss=ss, gate=gate)
    o, g, _ = run_bn(case, L, BF, ss=ss, gate=gate, tile=tile)
    assert torch.equal(o, wo) and torch.equal(g, wg), tile
    assert 0.05 < float((wo == 0).float().mean()) < 0.95 and not torch.equal(wo, wg)


DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_mx8_tile_digests.json")


def sha256_of(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def tile_digests(L, Cout, Dp, P, order, tile):
    """The operands and the two runs of test_a_narrow_tile_writes_the_wide_tiles_bits on `tile` -> sha256 of the operands, of out (fp32,
    ss = None) and of out + gated (bf16 through ss and the gate).  Every operand value is drawn from a seeded generator on the host
    (random_case, epilogue_of) and then moved; pq / pv are integer arithmetic and `permuted` is an indexing."""
    case = permuted(case_of(Dp, P, Cout, 3 * Dp + P + Cout + L), order)
    ss, gate = epilogue_of(Cout, L + Cout)
    index, wcodes, wscales, wpos, pq, pv, vids = case
    operands = [index.codes, index.scales, index.prop_off, wcodes, wscales, pq, pv, vids, ss, gate] + ([index.pos, wpos] if P else [])
    out, gated, _ = run_bn(case, L, BF, ss=ss, gate=gate, tile=tile)
    return {"operands": sha256_of(*operands), "fp32": sha256_of(run_bn(case, L, torch.float32, tile=tile)[0]), "bf16": sha256_of(out, gated)}


@pytest.mark.parametrize("L,Cout,Dp,P,order", GEOMETRIES)
def test_every_tile_writes_the_recorded_bits(request, L, Cout, Dp, P, order):
    """tests/golden/search_mx8_tile_digests.json: what the wide tile wrote on an MI355X at the commit the file names.  The test
    above compares the tiles with one another, so a summation order that moved in every tile together -- as it can once the kernels
    share code -- would pass it; this one would not.  Both entries of the wide tile and every narrow tile, no tolerance."""
    from drn_amd import ops
    want = json.load(open(DIGESTS))["digests"][request.node.callspec.id]
    for tile in (None,) + tuple(ops.CONV0_MX8_TILES):
        got = tile_digests(L, Cout, Dp, P, order, tile)
        assert got["operands"] == want["operands"], "the operands are not the recorded ones: the generators, not the kernel"
        assert got == want, (tile, got, want)


# -- 2. the oracle itself, the guards, the order of the pairs --------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", NARROW, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("Dp,P,Cout", [(64, 32, 272), (160, 32, 48), (384, 0, 16)])
def test_a_narrow_tile_on_exact_data_equals_the_oracle(tile, Dp, P, Cout):
    """The data of test_the_bare_convolution_on_exact_data_equals_the_oracle (small integers, a scale exponent per block on both
    sides: exact in fp32 in any order), against mx8_conv0_reference, not against the sibling kernel."""
    from drn_amd.index import mx8_conv0_reference
    case = exact_case(Dp, P, Cout, 7 * Dp + P + Cout)
    for L in (12, 5) + ((70, 300) if (Dp, Cout) == (160, 48) else ()):
        out, _, wide = run_bn(case, L, torch.float32, pq_host=case[4].cpu(), tile=tile)
        want = mx8_conv0_reference(*case, L)
        got = out.double().cpu()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (tile, L, bad.shape[0], bad[:6].tolist(), got[want != got][:6].tolist(), want[want != got][:6].tolist())
        assert float(want.abs().max()) > 64 and not torch.equal(want[0], want[7])
        assert bool((wide[0][14] == FILL).all())                                            # the rows past the last pair


@pytest.mark.parametrize("tile", NARROW, ids=lambda t: "%dx%d" % t)
def test_a_narrow_tile_writes_nothing_outside_its_columns_and_rows(tile):
    """Cout = 80 inside buffers of 96 columns and 15 pairs' rows, filled beforehand: columns [80, 96) and the rows past the last pair
    keep the fill, in fp32 and in bf16 with a gated output."""
    case = case_of(160, 32, 80, 41)
    ss, gate = epilogue_of(80, 43)
    for L in (12, 70):
        for dtype, kw in ((torch.float32, {}), (BF, dict(ss=ss, gate=gate))):
            out, gated, wide = run_bn(case, L, dtype, extra=16, tile=tile, **kw)
            assert len(wide) == (2 if kw else 1) and tuple(wide[0].shape) == (15, L, 96)
            for w in wide:
                assert bool((w[:14, :, 80:] == FILL).all()) and bool((w[14] == FILL).all()), (tile, L, dtype)
            assert not bool((out == FILL).all(dim=2).any())                                  # every row of every pair was written


@pytest.mark.parametrize("tile", NARROW, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("L", [12, 70])
def test_a_pairs_rows_do_not_depend_on_the_order_of_the_pairs_on_a_narrow_tile(tile, L):
    case = case_of(160, 32, 48, 21)
    ss, gate = epilogue_of(48, 23)
    base = run_bn(case, L, torch.float32, tile=tile)[0]
    out, gated, _ = run_bn(case, L, BF, ss=ss, gate=gate, tile=tile)
    for perm in (INTERLEAVED, SHUFFLED):
        dperm = perm.to(DEV)
        assert torch.equal(run_bn(permuted(case, perm), L, torch.float32, tile=tile)[0], base[dperm]), (tile, perm.tolist())
        o, g, _ = run_bn(permuted(case, perm), L, BF, ss=ss, gate=gate[dperm], tile=tile)
        assert torch.equal(o, out[dperm]) and torch.equal(g, gated[dperm]), (tile, perm.tolist())


# -- 3. the chooser --------------------------------------------------------------------------------------------------------------------------

def test_auto_is_a_shipped_tile_a_function_of_the_grid_and_writes_the_same_bits():
    from drn_amd import ops
    case = case_of(160, 32, 80, 5)
    for L in (12, 300):
        tile = ops.conv0_mx8_bn_tile(14, L, 80)
        assert tile in ops.CONV0_MX8_TILES and all(ops.conv0_mx8_bn_tile(14, L, 80) == tile for _ in range(3))
        auto = run_bn(case, L, torch.float32, tile="auto")[0]
        assert torch.equal(auto, run_bn(case, L, torch.float32, tile=tile)[0]) and torch.equal(auto, run_bn(case, L, torch.float32)[0])
        for perm in (INTERLEAVED, SHUFFLED):                                                 # (other pairs, the same grid: the same tile)
            assert torch.equal(run_bn(permuted(case, perm), L, torch.float32, tile="auto")[0], auto[perm.to(DEV)])


def test_the_entry_chooses_for_itself_when_it_is_given_no_tile(monkeypatch):
    """tile_rows = tile_cols = 0 at the C entry (what "auto" would pass if the chooser answered (0, 0)): the launch drn_conv0_mx8_bn_choose
    names, hence the same bits, on a grid of either kind."""
    from drn_amd import ops
    case = case_of(160, 32, 80, 5)
    want = {L: run_bn(case, L, BF, *epilogue_of(80, 7))[:2] for L in (12, 300)}
    monkeypatch.setattr(ops, "conv0_mx8_bn_tile", lambda Q, L, Cout: (0, 0))
    for L in (12, 300):
        out, gated, _ = run_bn(case, L, BF, *epilogue_of(80, 7), tile="auto")
        assert torch.equal(out, want[L][0]) and torch.equal(gated, want[L][1]), L


def test_the_chooser_follows_its_rule():
    """with W = cdiv(Q L, 256) x cdiv(Cout, 256) wide-tile workgroups on a chip of `cus` compute units, 64 x 64
    while 16 W <= CONV0_MX8_SMALL_UPTO_16THS cus, 128 x 64 while 16 W <= CONV0_MX8_MID_UPTO_16THS cus, the wide tile above -- on both
    sides of both crossovers, by rows and by channels."""
    from drn_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    small_upto, mid_upto = ops.CONV0_MX8_SMALL_UPTO_16THS, ops.CONV0_MX8_MID_UPTO_16THS

    def want(Q, L, Cout):
        W = -(-Q * L // 256) * -(-Cout // 256)
        return (64, 64) if 16 * W <= small_upto * cus else (128, 64) if 16 * W <= mid_upto * cus else ops.CONV0_MX8_WIDE
    first_wide, first_mid = mid_upto * cus // 16 + 1, small_upto * cus // 16 + 1             # the smallest W of either class
    seen = set()
    for W in {1, first_mid - 1, first_mid, first_wide - 1, first_wide, 4 * first_wide} - {0}:
        for Q, L, Cout in ((W, 256, 256), (8 * W, 32, 16), (W, 255, 256), (-(-W // 2), 256, 272), (1, 256 * W, 64)):
            got = ops.conv0_mx8_bn_tile(Q, L, Cout)
            assert got == want(Q, L, Cout), (Q, L, Cout, got, cus)
            seen.add(got)
    assert seen == set(ops.CONV0_MX8_TILES)
    assert ops.conv0_mx8_bn_tile(64, 32, 256) != ops.CONV0_MX8_WIDE or cus < 8                # the interactive grid of the README


# -- 4. the search ---------------------------------------------------------------------------------------------------------------------------

def grounder(**kw):
    from drn_amd import Grounder
    return Grounder(shared()[0], conv0="mxfp8", fused=True, **kw)


def searches(g, tok, qlen, q, T_=None):
    """Cartesian in chunks, a videos= subset, candidates= shortlists, ground_stored -> ([Hits], Moments)."""
    lists = [[1, 4, 6], [2], [0, 6, 3, 5, 2]][:int(tok.shape[0])]
    names = ["vid2", "vid5", "vid2"][:int(tok.shape[0])]
    hits = [g.search(tok, qlen, q, per_video=2, chunk=3, T=T_), g.search(tok, qlen, q, videos=["vid2", "vid5"], per_video=2, T=T_),
            g.search(tok, qlen, q, candidates=lists, per_video=2, pairs=3, T=T_)]
    return hits, g.ground_stored(tok, qlen, q, names, T=T_)


def same_everything(a, b, what):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        same_hits(x, y, (what, i))
    for f in MOMENT:
        assert torch.equal(getattr(a[1], f), getattr(b[1], f)), (what, f)


@pytest.mark.parametrize("T_", [T, 48])
@pytest.mark.parametrize("n_sent", [1, S])
def test_the_search_on_the_chosen_tile_returns_the_wide_tiles_hits(monkeypatch, n_sent, T_):
    """T = 32: a 64-row tile holds two pairs; T = 48: pairs straddle the 64- and 128-row tiles.  Eagerly and by graph replay (one
    capture per signature), against the same searches with the chooser held to the wide tile: every field of every result."""
    from drn_amd import ops
    m, store, q, (tok, qlen), (tok2, qlen2) = shared()
    tok, qlen, tok2, qlen2 = tok[:n_sent], qlen[:n_sent], tok2[:n_sent], qlen2[:n_sent]
    Cout = int(conv0_parts(m)[0].weight.shape[0])
    assert ops.conv0_mx8_bn_tile(n_sent * 3, T_, Cout) != ops.CONV0_MX8_WIDE                 # the chunks of the first search: a narrow tile
    eager, graphed = grounder(top_k=6), grounder(top_k=6, graph=True)
    got, got_graph = searches(eager, tok, qlen, q, T_), searches(graphed, tok, qlen, q, T_)
    captures = graphed.captures
    got2 = searches(graphed, tok2, qlen2, q, T_)
    assert graphed.captures == captures                                                      # other sentences: the same signatures
    tags = launch_tags(lambda: eager.search(tok, qlen, q, per_video=2, chunk=3, T=T_))
    assert tags.count("conv0_mx8_bn") == 3 and "conv0_mx8" not in tags and tags.count("gate_quantize_weights_mx8") == 1, tags
    assert "gate_gather_packed_q8" not in tags and "gate_gather_packed" not in tags and "quantize_rows_mx8" not in tags

    chosen = []
    monkeypatch.setattr(ops, "conv0_mx8_bn_tile", lambda Q, L, C: chosen.append((Q, L, C)) or ops.CONV0_MX8_WIDE)
    wide_eager, wide_graphed = grounder(top_k=6), grounder(top_k=6, graph=True)
    want = searches(wide_eager, tok, qlen, q, T_)
    assert chosen and all(L == T_ and C == Cout for _, L, C in chosen)
    same_everything(got, want, "eager")
    same_everything(got_graph, want, "graph replay")
    same_everything(searches(wide_graphed, tok, qlen, q, T_), want, "graph replay on the wide tile")
    same_everything(got2, searches(wide_eager, tok2, qlen2, q, T_), "other sentences by replay")
    assert wide_graphed.captures == captures and int(want[0][0].n.min()) > 0 and int(want[1].n.min()) > 0
