"""Pooled tables on the device: Shortlister.pooled / ShardedShortlister.pooled / ops.pool_segments against pool_segments_reference
evaluated on the host, BIT FOR BIT -- no tolerance anywhere: the definition fixes the add order, the division and the rounding.  The
shape table (tests/test_pooled_cpu.py: leading, inner and trailing videos without rows, runs of 1, 2, 17 and 300, widths on every
path of the kernel in both dtypes -- 16-byte, element by element (36 in bf16, 22 in fp32) and FP8 --, every group size around the
runs) on order-sensitive inputs that the CPU file proves can tell a wrong order; then the pooled table inside shortlist / rank, the
sharded twin with its masks before and after an append, the bounded staging buffer, the guard row and the cascade."""
import numpy as np
import pytest
import torch

from test_allow_shortlist_cpu import same
from test_pooled_cpu import DTYPES, GROUPS, HOWS, OFFSETS, RUNS, WIDTHS, bits, order_sensitive, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["v%d" % v for v in range(len(RUNS))]
CASES = [pytest.param(dtype, E, id="%s-E%d" % ("bf16" if dtype == torch.bfloat16 else "fp32", E)) for dtype in DTYPES for E in WIDTHS[dtype]]


def raw(t):
    """A tensor's bytes on the host, so that a comparison is of bits and not of values (-0 is not +0 here)."""
    return t.detach().cpu().contiguous().view(torch.uint8)


def source(E, dtype, q8):
    from drn_amd import Shortlister
    return Shortlister(order_sensitive(E, dtype).to(DEV), names=NAMES, offsets=OFFSETS, quantize="mxfp8" if q8 else None)


def check_table(got, want, fp8, dtype, what):
    """got, a pooled Shortlister, holds want = Pooled(rows, offsets) of the reference: format, bytes, names, offsets, block plan."""
    from drn_amd import plan_segment_blocks
    from drn_amd.index import mx8_quantize
    assert got.quantize == ("mxfp8" if fp8 else None) and got.dtype == dtype and len(got) == len(RUNS) and got.names == NAMES, what
    if fp8:
        codes, scales = mx8_quantize(want.rows)
        assert got.embeddings is None and got.codes.is_cuda and tuple(got.codes.shape) == tuple(want.rows.shape), what
        assert torch.equal(got.codes.cpu(), codes) and torch.equal(got.scales.cpu(), scales), what
    else:
        assert got.embeddings.is_cuda and got.embeddings.dtype == dtype and tuple(got.embeddings.shape) == tuple(want.rows.shape), what
        assert torch.equal(raw(got.embeddings), raw(want.rows)), what
    if want.offsets is None:
        assert got._seg is None, what
    else:
        plan = plan_segment_blocks(want.offsets)
        assert got.offsets.dtype == torch.int32 and got.offsets.cpu().tolist() == want.offsets.tolist(), what
        assert np.array_equal(got.plan.blk_vid, plan.blk_vid) and np.array_equal(got.plan.vid_blk, plan.vid_blk), what
        assert got._seg[1].cpu().tolist() == plan.blk_vid.tolist() and got._seg[2].cpu().tolist() == plan.vid_blk.tolist(), what


# -- 1. the shape table ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,E", CASES)
def test_pooled_is_the_reference_bit_for_bit(dtype, E):
    """Every group size x how x source format x target format of the shape table at this (dtype, E)."""
    from drn_amd import pack_allow_reference
    owners = torch.from_numpy(pack_allow_reference(np.asarray(RUNS) > 0))
    for q8 in ((False, True) if E % 32 == 0 else (False,)):
        src = source(E, dtype, q8)
        before = [t.clone() for t in ((src.codes, src.scales) if q8 else (src.embeddings,))]
        for group in GROUPS:
            for how in HOWS:
                want = reference(E, dtype, how, group, q8=q8)
                for target in (("same", None, "mxfp8") if E % 32 == 0 else ("same", None)):
                    what = (q8, group, how, target)
                    got = src.pooled(how=how, group=group, quantize=target)
                    check_table(got, want, q8 if target == "same" else target is not None, dtype, what)
                    if group is None:
                        assert got.nonempty.dtype == torch.int32 and got.nonempty.is_cuda and torch.equal(got.nonempty.cpu(), owners), what
                        assert torch.equal(got.nonempty, src.allow_of(keep=[v for v, n in enumerate(RUNS) if n])), what
                    else:
                        assert got.nonempty is None, what
        assert all(torch.equal(raw(a), raw(b)) for a, b in zip(before, (src.codes, src.scales) if q8 else (src.embeddings,)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,E", CASES)
def test_every_output_element_is_written_and_nothing_past_them(dtype, E):
    """ops.pool_segments into a buffer that starts as NaN with a guard row behind it: the rows are the reference's (so none is NaN:
    every element was written) and the guard row stays NaN -- for the whole table and for a window in its middle."""
    from drn_amd import ops, pool_offsets
    for q8 in ((False, True) if E % 32 == 0 else (False,)):
        src = source(E, dtype, q8)
        for group in (None, 2, 16):
            out_off = None if group is None else torch.from_numpy(pool_offsets(OFFSETS, group).astype(np.int32)).to(DEV)
            for how in HOWS:
                want = reference(E, dtype, how, group, q8=q8).rows
                rows = int(want.shape[0])
                for r0, r1 in ((0, rows), (rows // 3, rows - 1)):
                    buf = torch.full((r1 - r0 + 1, E), float("nan"), dtype=dtype, device=DEV)
                    ops.pool_segments(src._operand(), src.offsets, buf[:r1 - r0], how, group, out_off, out_row0=r0)
                    assert torch.equal(raw(buf[:r1 - r0]), raw(want[r0:r1])), (q8, group, how, r0)
                    assert bool(torch.isnan(buf[r1 - r0]).all()), (q8, group, how, r0)
    torch.cuda.synchronize()


def test_a_small_staging_buffer_gives_the_bytes_of_one_chunk(monkeypatch):
    """quantize="mxfp8" through a staging buffer of 5 rows: ceil(rows / 5) pool launches and as many of the quantiser, the bytes of the
    one-chunk result; a sum that overflows fp32 raises as the constructor would."""
    from drn_amd import Shortlister, _lib, ops
    E, dtype = 64, torch.bfloat16
    for q8 in (False, True):
        src = source(E, dtype, q8)
        for group, rows in ((None, 8), (2, 162)):
            whole = src.pooled(group=group, quantize="mxfp8")
            monkeypatch.setattr(ops, "kernel_timer", [])
            got = src.pooled(group=group, quantize="mxfp8", stage_elems=5 * E + 3)
            tags = [t[0] for t in ops.kernel_timer]
            monkeypatch.setattr(ops, "kernel_timer", None)
            assert tags == ["pool_segments", "quantize_rows_mx8"] * -(-rows // 5), (q8, group, tags)
            assert torch.equal(got.codes, whole.codes) and torch.equal(got.scales, whole.scales), (q8, group)
            check_table(got, reference(E, dtype, "mean", group, q8=q8), True, dtype, (q8, group))
    big = torch.full((4, 32), 3.0e38, dtype=torch.float32, device=DEV)
    sl = Shortlister(big, offsets=[0, 4])
    assert bool(torch.isfinite(sl.pooled(how="max").embeddings).all())
    for target in (None, "mxfp8"):
        with pytest.raises(_lib.DrnError, match="Shortlister.pooled: the pooled rows hold values that are not finite"):
            sl.pooled(quantize=target)
    torch.cuda.synchronize()


# -- 2. the pooled table at work ---------------------------------------------------------------------------------------------------------------

EXACT_RUNS = [0, 1, 2, 0, 16, 4, 1, 0, 8, 16] * 4 + [2, 0]       # powers of two: a mean of small integers is exact in bfloat16


def exact_case(dtype, seed=3):
    """Integers in [-3, 3] in runs of 1 to 16 rows (some videos own none) with duplicated videos, and integer queries: every pooled
    value is k / 16 with |k| <= 48 and every score an exact fp32 number, so the float64 references give the kernels' bits and ties
    fall by position."""
    g = torch.Generator().manual_seed(seed)
    off = np.concatenate([[0], np.cumsum(EXACT_RUNS)]).astype(np.int64)
    x = torch.randint(-3, 4, (int(off[-1]), 32), generator=g).float()
    for a, b in ((4, 9), (5, 15), (8, 18)):                                     # equal runs hold equal rows: equal scores
        x[off[b]:off[b + 1]] = x[off[a]:off[a + 1]]
    return x.to(dtype), off, torch.randint(-3, 4, (5, 32), generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_a_pooled_table_shortlists_and_ranks_like_the_references_over_the_pooled_rows(dtype):
    from drn_amd import (Shortlister, pack_allow_reference, pool_segments_reference, rank_reference, segment_shortlist_reference,
                         shortlist_reference)
    x, off, q = exact_case(dtype)
    V, lens = len(EXACT_RUNS), np.asarray(EXACT_RUNS)
    fine = Shortlister(x.to(DEV), offsets=off)
    qd = q.to(DEV)
    owns = torch.from_numpy(lens > 0)
    targets = torch.tensor([4, 0, 9, V - 1, 14], dtype=torch.int32)
    host = lambda res: type(res)(*(t.cpu() for t in res))
    for how in HOWS:
        want = pool_segments_reference(x, off, how, None)
        table = fine.pooled(how=how)
        assert torch.equal(raw(table.embeddings), raw(want.rows)) and torch.equal(table.nonempty.cpu(), torch.from_numpy(pack_allow_reference(lens > 0)))
        for n in (7, V):
            # with allow=nonempty no video without rows is listed ...
            got = host(table.shortlist(qd, n, allow=table.nonempty))
            same(got, shortlist_reference(want.rows, q, n, allow=owns), (how, n))
            assert not bool(np.isin(got.ids.numpy(), np.nonzero(lens == 0)[0]).any())
            # ... and without it the zero rows ARE candidates, listed with score 0, as documented
            free = host(table.shortlist(qd, n))
            same(free, shortlist_reference(want.rows, q, n), (how, n, "no mask"))
        listed = free.ids[0].tolist()
        assert all(v in listed and float(free.scores[0, listed.index(v)]) == 0.0 for v in np.nonzero(lens == 0)[0].tolist())
        same(host(table.rank(qd, targets.to(DEV), allow=table.nonempty)), rank_reference(want.rows, q, targets, allow=owns), (how, "rank"))
        same(host(table.rank(qd, targets.to(DEV))), rank_reference(want.rows, q, targets), (how, "rank, no mask"))
        # a ragged result: best pooled segment per video, with the segment that wins
        for g in (2, 4):
            want = pool_segments_reference(x, off, how, g)
            ragged = fine.pooled(how=how, group=g)
            assert ragged.nonempty is None
            same(host(ragged.shortlist(qd, 9)), segment_shortlist_reference(want.rows, want.offsets, q, 9), (how, g))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_sharded_pooled_answers_like_the_single_table(dtype):
    """Three shards -- plain, FP8, plain; the first and the last begin and end with videos without rows -- against ONE table over the
    concatenated rows: the shards' pooled tables hold the single table's bytes, and shortlist() answers bit for bit."""
    from drn_amd import ShardedShortlister, Shortlister, _lib
    from drn_amd.index import mx8_dequantize, mx8_quantize
    E = 64
    x = order_sensitive(E, dtype)
    codes, scales = mx8_quantize(x[OFFSETS[3]:OFFSETS[5]])                     # the middle shard is FP8: the single table holds what it holds
    whole = torch.cat([x[:OFFSETS[3]], mx8_dequantize(codes, scales, dtype), x[OFFSETS[5]:]])
    local = lambda a, b: (OFFSETS[a:b + 1] - OFFSETS[a])
    rows = lambda a, b: whole[OFFSETS[a]:OFFSETS[b]].to(DEV)
    shards = [Shortlister(rows(0, 3), names=NAMES[0:3], offsets=local(0, 3)),
              Shortlister.from_mx8(codes.to(DEV).contiguous(), scales.to(DEV).contiguous(), dtype, names=NAMES[3:5], offsets=local(3, 5)),
              Shortlister(rows(5, 8), names=NAMES[5:8], offsets=local(5, 8))]
    sh = ShardedShortlister(shards)
    one = Shortlister(whole.to(DEV), names=NAMES, offsets=OFFSETS)
    with pytest.raises(_lib.DrnError, match="quantize=\"same\" needs shards of one format"):
        sh.pooled()
    q = order_sensitive(E, dtype, offsets=np.asarray([0, 6]), seed=5).to(DEV)
    for how in HOWS:
        for group in (None, 2, 17):
            for target in (None, "mxfp8"):
                got, want = sh.pooled(how=how, group=group, quantize=target), one.pooled(how=how, group=group, quantize=target)
                what = (how, group, target)
                assert isinstance(got, ShardedShortlister) and len(got) == len(sh) and got.bases == sh.bases and got.names == NAMES, what
                if target is None:
                    assert torch.equal(raw(torch.cat([s.embeddings for s in got.shards])), raw(want.embeddings)), what
                else:
                    assert torch.equal(torch.cat([s.codes for s in got.shards]), want.codes), what
                    assert torch.equal(torch.cat([s.scales for s in got.shards]), want.scales), what
                if group is None:
                    assert torch.equal(got.nonempty, want.nonempty), what
                    for allow in (None, want.nonempty):
                        same(got.shortlist(q, 8, allow=allow), want.shortlist(q, 8, allow=allow), what)
                else:
                    assert got.nonempty is None and want.nonempty is None, what
                    same(got.shortlist(q, 8), want.shortlist(q, 8), what)
    uniform = ShardedShortlister([shards[0], shards[2]]).pooled()              # "same" on shards of one format keeps it
    assert all(s.quantize is None for s in uniform.shards) and uniform.nonempty is not None
    # every shard carries the mask of its own videos, and the corpus's follows the shards through an append
    from drn_amd import pack_allow_reference
    own = lambda a, b: torch.from_numpy(pack_allow_reference(np.asarray(RUNS[a:b]) > 0))
    want = one.pooled(quantize=None)
    got = sh.pooled(quantize=None)
    assert [torch.equal(s.nonempty.cpu(), own(a, b)) for s, (a, b) in zip(got.shards, ((0, 3), (3, 5), (5, 8)))] == [True] * 3
    grown = ShardedShortlister(shards[:2]).pooled(quantize=None)
    assert torch.equal(grown.nonempty.cpu(), own(0, 5))
    grown.append(shards[2].pooled())
    assert len(grown) == len(RUNS) and torch.equal(grown.nonempty, want.nonempty)
    same(grown.shortlist(q, 8, allow=grown.nonempty), want.shortlist(q, 8, allow=want.nonempty), "after an append")
    full = Shortlister(order_sensitive(E, dtype, offsets=np.asarray([0, 2, 5]), seed=7).to(DEV), offsets=[0, 2, 5]).pooled()
    assert full.nonempty is None                                               # (every video owns a row: the shard allows them all)
    grown.append(full)
    assert torch.equal(grown.nonempty.cpu(), torch.from_numpy(pack_allow_reference(np.asarray(RUNS + [2, 3]) > 0)))
    assert ShardedShortlister([full, full]).nonempty is None
    torch.cuda.synchronize()


def test_a_cascade_from_the_one_table_the_caller_owns():
    """evaluate_cascade(coarse=fine.pooled(), fine=fine, allow=coarse.nonempty) runs on a tiny annotated batch: finite metrics, and the
    ranks are the fine table's full ranks under the mask "listed by the coarse stage", cut at depth."""
    from drn_amd import Shortlister, candidates_mask, evaluate_cascade, pack_allow
    x, off, q = exact_case(torch.bfloat16)
    V = len(EXACT_RUNS)
    names = ["v%d" % v for v in range(V)]
    fine = Shortlister(x.to(DEV), names=names, offsets=off)
    coarse = fine.pooled()
    assert coarse.names == names and len(coarse) == len(fine) and coarse.nonempty is not None
    qd, depth = q.to(DEV), 6
    annotated = [names[v] for v in (4, 1, 9, 14, 41)]
    got = evaluate_cascade(coarse, fine, iter([(annotated, qd, qd)]), depth, topks=(1, 5), allow=coarse.nonempty)
    assert got.n == 5 and all(np.isfinite(r) and 0.0 <= r <= 1.0 for r in got.recall) and np.isfinite(got.mrr)
    words = pack_allow(candidates_mask(coarse.shortlist(qd, depth, allow=coarse.nonempty).ids, V))
    targets = torch.tensor([names.index(n) for n in annotated], dtype=torch.int32, device=DEV)
    r = fine.rank(qd, targets, allow=words).rank
    assert np.array_equal(got.ranks, torch.where(r < depth, r, torch.full_like(r, -1)).cpu().numpy())
    torch.cuda.synchronize()
