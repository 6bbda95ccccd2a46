"""Compacting a sharded corpus on the device: ShardedShortlister.compact against compact_reference, byte for byte -- plain shards on the
16-byte and the one-element paths, mixed FP8 / plain shards to either format through a staging buffer smaller than a shard, ragged
shards with videos of 0, 1 and 70 rows --, the new table against the sharded object under allow=keep in all six methods, bit for bit,
the all-kept join against ONE Shortlister over the concatenated rows, the refusals, and the launch tags.
tests/test_compact_cpu.py holds the definition, the refusals and the C boundary."""
import numpy as np
import pytest
import torch

from test_compact_cpu import RAGGED, SIZES, int_rows, mapped, masks, ragged_masks, stand_in, twin_corpus

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])


def raw(t):
    """A tensor's bytes, so that a comparison is of bits and not of values."""
    return t.contiguous().view(torch.uint8)


def same_table(got, want, what):
    """Two Shortlisters hold the same table: format, bytes, names, offsets and block plan."""
    assert got.quantize == want.quantize and got.dtype == want.dtype and len(got) == len(want), what
    if want.quantize is None:
        assert got.embeddings.dtype == want.embeddings.dtype and got.embeddings.shape == want.embeddings.shape, what
        assert torch.equal(raw(got.embeddings), raw(want.embeddings.to(got.embeddings.device))), what
    else:
        assert torch.equal(got.codes, want.codes.to(got.codes.device)) and torch.equal(got.scales, want.scales.to(got.scales.device)), what
    assert got.names == want.names, what
    assert (got._seg is None) == (want._seg is None), what
    if want._seg is not None:
        for a, b in zip(got._seg, want._seg):
            assert a.dtype == torch.int32 and torch.equal(a.cpu(), b.cpu()), what
        assert np.array_equal(got.plan.blk_vid, want.plan.blk_vid) and np.array_equal(got.plan.vid_blk, want.plan.vid_blk), what


def same_compaction(got, want, what):
    assert got.kept == want.kept and isinstance(got.kept, int), what
    assert got.positions.dtype == torch.int32 and got.positions.is_cuda and torch.equal(got.positions.cpu(), want.positions.cpu()), what
    same_table(got.table, want.table, what)


def snapshot(sh):
    return [tuple(t.clone() for t in ((s.embeddings,) if s.quantize is None else (s.codes, s.scales))) for s in sh.shards]


def unchanged(sh, before):
    return all(torch.equal(raw(a), raw(b)) for s, old in zip(sh.shards, before)
               for a, b in zip((s.embeddings,) if s.quantize is None else (s.codes, s.scales), old))


def packed(mask):
    from drn_amd import pack_allow
    return pack_allow(mask.to(DEV).contiguous())


# -- 1. plain shards ---------------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("E", [40, 33], ids=["E40_vec16", "E33_scalar"])
def test_plain_shards_compact_to_the_reference_byte_for_byte(dtype, E):
    from drn_amd import ShardedShortlister, Shortlister, compact_reference
    V = sum(SIZES)
    whole = (torch.randn(V + 1, E, generator=torch.Generator().manual_seed(E)) * 3).to(dtype).to(DEV)
    names = ["v%d" % v for v in range(V)]
    big = whole[4:76].clone()                                                  # the middle shard is a row slice that starts at the odd row 1
    shards = [Shortlister(whole[0:5].clone(), names=names[0:5]), Shortlister(big[1:71], names=names[5:75]),
              Shortlister(whole[75:108].clone(), names=names[75:108])]
    assert shards[1].embeddings.data_ptr() == big.data_ptr() + E * big.element_size()
    sh = ShardedShortlister(shards)
    before = snapshot(sh)
    for what, mask in masks(V).items():
        got = sh.compact(packed(mask))
        same_compaction(got, compact_reference(sh, keep=mask), (what, E))
        assert torch.equal(raw(got.table.embeddings), raw(whole[:V][mask.to(DEV)])), what
        assert got.table.embeddings.is_contiguous() and all(got.table.embeddings.data_ptr() != s.embeddings.data_ptr() for s in shards), what
    assert unchanged(sh, before)
    torch.cuda.synchronize()


# -- 2. mixed formats --------------------------------------------------------------------------------------------------------------------------

@DTYPES
def test_mixed_shards_compact_to_either_format(dtype, monkeypatch):
    from drn_amd import ShardedShortlister, Shortlister, _lib, compact_reference, ops
    from drn_amd.index import mx8_dequantize, mx8_quantize
    E = 64
    g = torch.Generator().manual_seed(13)

    def fp8(n, shift=0):
        """Tables the quantiser would never have written: random codes (no NaN code) under arbitrary legal scale bytes; with shift,
        in storage that is not 8-byte aligned, where the kernels move one element a lane."""
        codes = torch.randint(0, 256, (n, E), generator=g).to(torch.uint8)
        codes[(codes & 0x7f) == 0x7f] = 0x11
        scales = torch.randint(100, 141, (n, E // 32), generator=g).to(torch.uint8)
        flat = torch.zeros(n * E + shift, dtype=torch.uint8, device=DEV)
        flat[shift:] = codes.reshape(-1).to(DEV)
        return Shortlister.from_mx8(flat[shift:].view(n, E), scales.to(DEV), dtype)
    plain = (torch.randn(33, E, generator=g) * 3).to(dtype).to(DEV)
    shards = [fp8(37), Shortlister(plain), fp8(6, shift=3)]
    assert shards[2].codes.data_ptr() % 8 == 3
    sh = ShardedShortlister(shards)
    V = len(sh)
    before = snapshot(sh)
    mask = torch.rand(V, generator=g) < 0.7
    mask[36] = mask[37] = mask[70] = True
    keep = packed(mask)
    kept_plain = plain[mask[37:70].to(DEV)]
    # -> plain: the FP8 rows dequantised exactly
    got = sh.compact(keep, quantize=None)
    same_compaction(got, compact_reference(sh, keep=mask, quantize=None), "to plain")
    a = int(mask[:37].sum())
    assert torch.equal(raw(got.table.embeddings[:a]), raw(mx8_dequantize(shards[0].codes, shards[0].scales, dtype)[mask[:37].to(DEV)]))
    assert torch.equal(raw(got.table.embeddings[a:a + len(kept_plain)]), raw(kept_plain))
    # -> FP8, the plain shard through a staging buffer of 7 rows: several quantise launches
    monkeypatch.setattr(ops, "kernel_timer", [])
    got = sh.compact(keep, quantize="mxfp8", stage_elems=7 * E)
    tags = [t[0] for t in ops.kernel_timer]
    monkeypatch.setattr(ops, "kernel_timer", None)
    chunks = -(-len(kept_plain) // 7)
    assert chunks >= 3 and tags == ["allow_slices"] + ["compact_plan"] * 3 + ["compact_rows"] + ["compact_rows", "quantize_rows_mx8"] * chunks + ["compact_rows"]
    same_compaction(got, compact_reference(sh, keep=mask, quantize="mxfp8"), "to FP8")
    assert torch.equal(got.table.codes[:a], shards[0].codes[mask[:37].to(DEV)]) and torch.equal(got.table.scales[:a], shards[0].scales[mask[:37].to(DEV)])
    qc, qs = mx8_quantize(kept_plain)
    assert torch.equal(got.table.codes[a:a + len(kept_plain)], qc) and torch.equal(got.table.scales[a:a + len(kept_plain)], qs)
    assert torch.equal(got.table.codes[a + len(kept_plain):], shards[2].codes[mask[70:].to(DEV)])
    # one chunk (the default staging buffer) writes the same bytes
    same_compaction(sh.compact(keep, quantize="mxfp8"), got, "one chunk")
    with pytest.raises(_lib.DrnError, match='quantize="same" needs shards of one format and these are mixed'):
        sh.compact(keep)
    assert unchanged(sh, before)
    torch.cuda.synchronize()


# -- 3. ragged shards --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,E,quantize", [(torch.bfloat16, 40, None), (torch.float32, 33, None), (torch.bfloat16, 64, "mxfp8")],
                         ids=["bf16_E40", "fp32_E33", "fp8_E64"])
def test_ragged_shards_compact_to_the_reference(dtype, E, quantize):
    from drn_amd import SegmentShortlist, ShardedShortlister, Shortlister, compact_reference
    shards = []
    for k, off in enumerate(RAGGED):
        names = ["s%d_%d" % (k, v) for v in range(len(off) - 1)]
        rows = int_rows(off[-1], E, dtype, seed=50 + k).to(DEV)
        if off[-1]:
            shards.append(Shortlister(rows, names=names, offsets=off, quantize=quantize))
        else:                                                                 # a shard whose videos own no rows: no constructor makes one
            shards.append(stand_in(torch.zeros(0, E, dtype=dtype), offsets=off, names=names, device=DEV) if quantize is None else
                          stand_in((torch.zeros(0, E, dtype=torch.uint8), torch.zeros(0, E // 32, dtype=torch.uint8)), offsets=off, quantize=quantize,
                                   dtype=dtype, names=names, device=DEV))
    sh = ShardedShortlister(shards)
    V = len(sh)
    before = snapshot(sh)
    for what, mask in ragged_masks(V).items():
        got = sh.compact(packed(mask))
        want = compact_reference(sh, keep=mask)
        same_compaction(got, want, what)
        assert got.table.offsets.tolist() == want.table.offsets.tolist() and len(got.table) == int(mask.sum()), what
    assert unchanged(sh, before)
    # the new table is a ragged table like any other: its shortlist carries rows
    q = int_rows(3, E, dtype, seed=60).to(DEV)
    out = got.table.shortlist(q, 4)
    assert isinstance(out, SegmentShortlist) and out.rows.shape == (3, 4)
    plain = got.table.dequantized()
    ref = Shortlister(plain.embeddings, offsets=plain.offsets).shortlist(q, 4)
    for f in SegmentShortlist._fields:
        assert torch.equal(getattr(out, f), getattr(ref, f)), f
    torch.cuda.synchronize()


# -- 4. end to end: the new table answers as the shards do under allow=keep ---------------------------------------------------------------

def fields_equal(got, want, positions, what):
    assert type(got) is type(want), what
    for f in want._fields:
        a, b = getattr(got, f), getattr(want, f)
        assert torch.equal(a, mapped(b, positions) if f == "ids" else b), (what, f)


FORMATS = pytest.mark.parametrize("formats", [(None, None, None), ("mxfp8", "mxfp8", "mxfp8"), (None, "mxfp8", None)], ids=["plain", "fp8", "mixed"])


@FORMATS
def test_the_compacted_plain_table_answers_as_the_masked_shards(formats):
    from drn_amd import ShardedShortlister, Shortlister
    whole, mask = twin_corpus(torch.bfloat16)
    cuts = np.cumsum((0,) + SIZES)
    sh = ShardedShortlister([Shortlister(whole[a:b].to(DEV).contiguous(), quantize=f) for f, a, b in zip(formats, cuts[:-1], cuts[1:])])
    keep = packed(mask)
    done = sh.compact(keep, quantize="same" if len(set(formats)) == 1 else None)
    table, pos, V = done.table, done.positions, len(sh)
    assert done.kept < 128
    q = int_rows(6, 32, torch.bfloat16, seed=11).to(DEV)
    for n in (1, 7, 128):                                                      # (128 is more than V')
        fields_equal(table.shortlist(q, n), sh.shortlist(q, n, allow=keep), pos, ("shortlist", n))
    wide = sh.shortlist(q, 128, allow=keep)
    assert bool(((wide.scores[:, 1:] == wide.scores[:, :-1]) & (wide.ids[:, 1:] >= 0)).any())            # the lists hold ties
    targets = torch.tensor([4, 5, 41, 75, -1, V], dtype=torch.int32, device=DEV)                          # (41 is dropped)
    local = mapped(targets.clamp(-1, V - 1), pos).where(targets < V, torch.full_like(targets, -1)).contiguous()
    fields_equal(table.rank(q, local), sh.rank(q, targets, allow=keep), pos, "rank")
    assert sh.rank(q, targets, allow=keep).rank.tolist()[2] == -1 and sh.rank(q, targets, allow=keep).rank.tolist()[0] >= 0
    cand = torch.randint(-1, V, (6, 24), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    cand[:, :6] = torch.tensor([3, 4, 5, 41, 74, 75], dtype=torch.int32, device=DEV)
    fields_equal(table.rerank(mapped(cand, pos).contiguous(), q, 9), sh.rerank(cand, q, 9, allow=keep), pos, "rerank")
    torch.cuda.synchronize()


@FORMATS
def test_the_compacted_ragged_table_answers_as_the_masked_shards(formats):
    from drn_amd import ShardedShortlister, Shortlister
    sizes, E = (5, 40, 20), 32
    lens = [(2, 1, 0, 3)[v % 4] for v in range(sum(sizes))]
    g = torch.Generator().manual_seed(21)
    shards, rows_of, at = [], [], 0
    for k, nv in enumerate(sizes):
        off = np.concatenate([[0], np.cumsum(lens[at:at + nv])])
        rows_of.append((int_rows(int(off[-1]), E, torch.bfloat16, seed=70 + k), off))
        at += nv
    rows_of[1][0][0] = rows_of[0][0][-1]                                       # twins across the cuts (videos 4 | 5, 44 | 45) ...
    rows_of[2][0][0] = rows_of[1][0][-1]
    rows_of[1][0][6] = rows_of[1][0][3]                                        # ... and on either side of video 9, which is dropped
    for f, (rows, off) in zip(formats, rows_of):
        shards.append(Shortlister(rows.to(DEV), offsets=off, quantize=f))
    sh = ShardedShortlister(shards)
    V = len(sh)
    mask = torch.rand(V, generator=g) < 0.75
    for v in (4, 5, 8, 11, 44, 45):
        mask[v] = True
    mask[9] = mask[0] = False
    keep = packed(mask)
    done = sh.compact(keep, quantize="same" if len(set(formats)) == 1 else None)
    table, pos = done.table, done.positions
    q = int_rows(5, E, torch.bfloat16, seed=12).to(DEV)
    for n in (3, 64):
        fields_equal(table.shortlist(q, n), sh.shortlist(q, n, allow=keep), pos, ("shortlist", n))
    ql = torch.stack([int_rows(3, E, torch.bfloat16, seed=80 + s) for s in range(5)]).to(DEV)
    lengths = torch.tensor([3, 1, 0, 2, 3], dtype=torch.int32, device=DEV)
    fields_equal(table.shortlist_late(ql, lengths, 10), sh.shortlist_late(ql, lengths, 10, allow=keep), pos, "shortlist_late")
    targets = torch.tensor([4, 5, 9, 45, V], dtype=torch.int32, device=DEV)
    local = mapped(targets.clamp(-1, V - 1), pos).where(targets < V, torch.full_like(targets, -1)).contiguous()
    fields_equal(table.rank(q, local), sh.rank(q, targets, allow=keep), pos, "rank")
    fields_equal(table.rank_late(ql, lengths, local), sh.rank_late(ql, lengths, targets, allow=keep), pos, "rank_late")
    cand = torch.randint(-1, V, (5, 20), generator=g).to(torch.int32).to(DEV)
    cand[:, :5] = torch.tensor([4, 5, 9, 44, 45], dtype=torch.int32, device=DEV)
    local_cand = mapped(cand, pos).contiguous()
    fields_equal(table.rerank(local_cand, q, 8), sh.rerank(cand, q, 8, allow=keep), pos, "rerank")
    fields_equal(table.rerank_late(local_cand, ql, lengths, 8), sh.rerank_late(cand, ql, lengths, 8, allow=keep), pos, "rerank_late")
    torch.cuda.synchronize()


# -- 5. all kept -------------------------------------------------------------------------------------------------------------------------------

def test_all_kept_joins_the_shards_into_the_table_of_the_concatenated_rows():
    from drn_amd import ShardedShortlister, Shortlister
    E, cuts = 64, [0, 1, 64, 321, 400]
    whole = (torch.randn(400, E, generator=torch.Generator().manual_seed(2)) * 2).to(torch.bfloat16).to(DEV)
    names = ["n%d" % v for v in range(400)]
    sh = ShardedShortlister([Shortlister(whole[a:b].clone(), names=names[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    got = sh.compact()
    same_table(got.table, Shortlister(whole, names=names), "joined")
    assert got.kept == 400 and torch.equal(got.positions, torch.arange(400, dtype=torch.int32, device=DEV))
    # to FP8: what the constructor writes over the same rows (lossy against the shards exactly as it is)
    same_table(sh.compact(quantize="mxfp8").table, Shortlister(whole, names=names, quantize="mxfp8"), "joined and quantised")
    torch.cuda.synchronize()


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
def test_shards_longer_than_one_step_of_the_plan(ragged):
    """The plan's workgroup walks 4096 videos a step and carries its totals from step to step, from wavefront to wavefront and from
    shard to shard: shards of more than two steps, every wavefront busy, no size a multiple of anything."""
    from drn_amd import ShardedShortlister, Shortlister, compact_reference
    g = torch.Generator().manual_seed(17)
    shards = []
    for k, nv in enumerate((9001, 4097, 5)):
        lens = torch.randint(0, 4, (nv,), generator=g)
        rows = int_rows(int(lens.sum()) if ragged else nv, 8, torch.float32, seed=90 + k).to(DEV)
        shards.append(Shortlister(rows, offsets=np.concatenate([[0], np.cumsum(lens.numpy())])) if ragged else Shortlister(rows))
    sh = ShardedShortlister(shards)
    mask = torch.rand(len(sh), generator=g) < 0.6
    same_compaction(sh.compact(packed(mask)), compact_reference(sh, keep=mask), ragged)
    torch.cuda.synchronize()


# -- 6. refusals -------------------------------------------------------------------------------------------------------------------------------

def test_an_empty_result_is_refused_and_the_shards_still_answer():
    from drn_amd import ShardedShortlister, Shortlister, _lib
    E = 32
    sh = ShardedShortlister([Shortlister(int_rows(5, E, torch.bfloat16, seed=1).to(DEV)), Shortlister(int_rows(40, E, torch.bfloat16, seed=2).to(DEV))])
    q = int_rows(3, E, torch.bfloat16, seed=3).to(DEV)
    before = sh.shortlist(q, 8)
    with pytest.raises(_lib.DrnError, match="keeps no video"):
        sh.compact(packed(torch.zeros(45, dtype=torch.bool)))
    after = sh.shortlist(q, 8)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    off = [0, 0, 3, 3, 4]
    rg = ShardedShortlister([Shortlister(int_rows(4, E, torch.bfloat16, seed=4).to(DEV), offsets=off)])
    before = rg.shortlist(q, 4)
    with pytest.raises(_lib.DrnError, match="2 videos the mask keeps own no row"):
        rg.compact(rg.allow_of(keep=[0, 2]))
    assert all(torch.equal(a, b) for a, b in zip(before, rg.shortlist(q, 4)))
    # ... and a single table drops videos through a sharded object of one shard
    one = rg.compact(rg.allow_of(drop=[1]))
    assert one.kept == 3 and one.positions.tolist() == [0, -1, 1, 2] and one.table.offsets.tolist() == [0, 0, 0, 1]
    torch.cuda.synchronize()


# -- 7. launch tags ----------------------------------------------------------------------------------------------------------------------------

def test_the_launches_of_a_compaction(monkeypatch):
    from drn_amd import ShardedShortlister, Shortlister, ops
    E, K = 32, 4
    sh = ShardedShortlister([Shortlister(int_rows(9 + k, E, torch.bfloat16, seed=k).to(DEV)) for k in range(K)])
    fp8 = ShardedShortlister([Shortlister(int_rows(9 + k, E, torch.bfloat16, seed=k).to(DEV), quantize="mxfp8") for k in range(K)])
    keep = sh.allow_of(drop=[0, 20])
    torch.cuda.synchronize()

    def tags_of(run):
        monkeypatch.setattr(ops, "kernel_timer", [])
        run()
        tags = [t[0] for t in ops.kernel_timer]
        monkeypatch.setattr(ops, "kernel_timer", None)
        return tags
    moved = ["compact_plan"] * K + ["compact_rows"] * K
    assert tags_of(lambda: sh.compact(keep)) == ["allow_slices"] + moved
    assert tags_of(lambda: sh.compact()) == moved
    assert tags_of(lambda: fp8.compact(keep)) == ["allow_slices"] + moved
    assert tags_of(lambda: fp8.compact(keep, quantize=None)) == ["allow_slices"] + moved
    assert tags_of(lambda: sh.compact(keep, quantize="mxfp8")) == ["allow_slices"] + ["compact_plan"] * K + ["compact_rows", "quantize_rows_mx8"] * K
    torch.cuda.synchronize()
