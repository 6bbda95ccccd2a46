"""The shortlist host path, pinned call by call: which C symbol each wrapper and each Shortlister method reaches, under which timer tag and
flop figure, and with exactly which arguments in the order of include/drn_hip.h.  No library and no GPU: ops.lib is replaced by a recorder,
and every expectation is a literal built here from the test's own data_ptr() values and integers, never from the wrappers."""
import ctypes

import pytest
import torch

from test_q8_shortlist_cpu import resident

STREAM = "the stream"
F32, BF16 = 0, 1
V, R, E, S, N, L, C = 40, 6, 64, 3, 2, 4, 5
WS = 70                                                                         # elements of the workspace handed to the wrappers


class Recorder(object):
    """Stands in for the library: every symbol is callable, returns 0 and records (symbol, args), a c_void_p reduced to its .value."""

    def __init__(self):
        self.calls, self.timed = [], []

    def __getattr__(self, symbol):
        def entry(*args):
            self.calls.append((symbol, tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args)))
            return 0
        return entry

    def time(self, tag, flops, launch):
        self.timed.append((tag, flops))
        return launch()

    def only(self):
        """The one call made since the last look -> (symbol, args, (tag, flops))."""
        assert len(self.calls) == 1 and len(self.timed) == 1, (self.calls, self.timed)
        (symbol, args), timed = self.calls.pop(), self.timed.pop()
        return symbol, args, timed


@pytest.fixture
def rec(monkeypatch):
    from drn_amd import ops
    r = Recorder()
    monkeypatch.setattr(ops, "lib", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "check", lambda rc, what=None: rc)
    monkeypatch.setattr(ops, "_timed", r.time)
    return r


def i32(*shape):
    return resident(torch.zeros(shape, dtype=torch.int32))


def ptr(t):
    return t.data_ptr()


def segment_tables():
    """offsets (V = 3 videos over R = 6 rows, one of them without rows), blk_vid (one block) and vid_blk."""
    return resident(torch.tensor([0, 2, 2, 6], dtype=torch.int32)), resident(torch.tensor([0, 3], dtype=torch.int32)), i32(3)


def wide(rows, dtype):
    return resident(torch.zeros(rows, E, dtype=dtype))


def q8(rows):
    return resident(torch.zeros(rows, E, dtype=torch.uint8)), resident(torch.zeros(rows, E // 32, dtype=torch.uint8))


# -- 1. the wrappers of drn_amd.ops ------------------------------------------------------------------------------------------------------------

# (ragged, quantised, masked) -> the call; table is emb or (codes, scales), seg the three segment tables, outs the three or four results
CALLS = {
    (False, False, False): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_topn(table, q, N, ws, *outs),
    (False, True, False): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_topn(table, q, N, ws, *outs),
    (False, False, True): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_topn(table, q, N, ws, *outs, allow=allow),
    (False, True, True): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_topn(table, q, N, ws, *outs, allow=allow),
    (True, False, False): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_segments_topn(table, q, *seg, N, ws, *outs),
    (True, True, False): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_segments_topn(table, q, *seg, N, ws, *outs),
    (True, False, True): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_segments_topn(table, q, *seg, N, ws, *outs, allow=allow),
    (True, True, True): lambda ops, table, q, seg, allow, ws, outs: ops.shortlist_segments_topn(table, q, *seg, N, ws, *outs, allow=allow),
}
SYMBOLS = {
    (False, False, False): "drn_shortlist_topn", (False, True, False): "drn_shortlist_topn_q8",
    (False, False, True): "drn_shortlist_topn_allow", (False, True, True): "drn_shortlist_topn_q8_allow",
    (True, False, False): "drn_shortlist_segments_topn", (True, True, False): "drn_shortlist_segments_topn_q8",
    (True, False, True): "drn_shortlist_segments_topn_allow", (True, True, True): "drn_shortlist_segments_topn_q8_allow",
}


@pytest.mark.parametrize("dtype,code", [(torch.float32, F32), (torch.bfloat16, BF16)])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("quantised", [False, True])
def test_each_wrapper_reaches_its_symbol_with_the_headers_arguments(rec, ragged, quantised, dtype, code):
    from drn_amd import ops
    rows = R if ragged else V
    table = q8(rows) if quantised else wide(rows, dtype)
    heads = tuple(ptr(t) for t in table) if quantised else (ptr(table),)
    q, ws = resident(torch.zeros(S, E, dtype=dtype)), resident(torch.zeros(WS, dtype=torch.int64))
    seg = segment_tables() if ragged else ()
    outs = (i32(S, N), resident(torch.zeros(S, N)), i32(S)) + ((i32(S, N),) if ragged else ())
    W = 1 if ragged else 2                                                      # ceil(3 / 32) and ceil(40 / 32) mask words a row
    for allow, stride in ((None, None), (i32(W), 0), (i32(S, W), W)):
        key = (ragged, quantised, allow is not None)
        got = CALLS[key](ops, table, q, seg, allow, ws, outs)
        assert len(got) == len(outs) and all(a is b for a, b in zip(got, outs))
        symbol, args, timed = rec.only()
        mask = () if allow is None else (ptr(allow), stride)
        if ragged:
            want = heads + (ptr(q), ptr(seg[0]), ptr(seg[1]), ptr(seg[2])) + mask + (6, 3, 1, 64, 3, 2, code, ptr(ws), 70,
                                                                                    ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), STREAM)
            flops = 2.0 * 3 * 6 * 64
        else:
            want = heads + (ptr(q),) + mask + (40, 64, 3, 2, code, ptr(ws), 70, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), STREAM)
            flops = 2.0 * 3 * 40 * 64
        assert symbol == SYMBOLS[key], key
        assert timed == (SYMBOLS[key][len("drn_"):], flops), key
        assert args == want, (key, stride)


# -- 2. Shortlister: which entry, which workspace key, which arguments ----------------------------------------------------------------------------

def stand_in(ragged, quantised, dtype=torch.bfloat16):
    """A Shortlister made without its constructor over resident host tensors -> (the object, the pointers that lead its entries'
    arguments: (emb,) or (codes, scales))."""
    from drn_amd import Shortlister
    sl = Shortlister.__new__(Shortlister)
    sl.names, sl._ws = None, {}
    rows = R if ragged else V
    if ragged:
        sl._seg = segment_tables()
    if quantised:
        sl.embeddings, sl.quantize, sl._dtype = None, "mxfp8", dtype
        sl.codes, sl.scales = q8(rows)
        return sl, (ptr(sl.codes), ptr(sl.scales))
    sl.embeddings = wide(rows, dtype)
    return sl, (ptr(sl.embeddings),)


@pytest.fixture
def made_on_the_host(monkeypatch):
    """The buffers a method makes itself land on the stand-in's device, the host: let the wrappers take them."""
    from drn_amd import ops
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("quantised", [False, True])
def test_shortlist_reaches_one_entry_with_the_workspace_of_its_key(rec, made_on_the_host, ragged, quantised):
    sl, heads = stand_in(ragged, quantised)
    q = resident(torch.zeros(S, E, dtype=torch.bfloat16))
    W = 1 if ragged else 2
    keys = 9 if ragged else 6                                                   # K + ceil(K / 2) with K = 3 * 1 * 2; 3 * ceil(40 / 256) * 2
    first = None
    for allow, stride in ((None, None), (i32(W), 0), (i32(S, W), W), (None, None)):
        got = sl.shortlist(q, N) if allow is None else sl.shortlist(q, N, allow=allow)
        assert type(got).__name__ == ("SegmentShortlist" if ragged else "Shortlist")
        assert list(sl._ws) == [(S, N)]
        ws = sl._ws[(S, N)]
        first = ws if first is None else first
        assert ws is first and ws.dtype == torch.int64 and ws.numel() == keys
        symbol, args, timed = rec.only()
        mask = () if allow is None else (ptr(allow), stride)
        if ragged:
            seg = sl._seg
            want = heads + (ptr(q), ptr(seg[0]), ptr(seg[1]), ptr(seg[2])) + mask + (6, 3, 1, 64, 3, 2, BF16, ptr(ws), 9,
                                                                                    ptr(got.ids), ptr(got.scores), ptr(got.n), ptr(got.rows), STREAM)
        else:
            want = heads + (ptr(q),) + mask + (40, 64, 3, 2, BF16, ptr(ws), 6, ptr(got.ids), ptr(got.scores), ptr(got.n), STREAM)
        assert symbol == SYMBOLS[(ragged, quantised, allow is not None)]
        assert timed == (symbol[len("drn_"):], 2.0 * 3 * (6 if ragged else 40) * 64)
        assert args == want
    # out= is written in place and handed back
    out = (i32(S, N), resident(torch.zeros(S, N)), i32(S)) + ((i32(S, N),) if ragged else ())
    got = sl.shortlist(q, N, out=out)
    assert all(a is b for a, b in zip(got, out))
    assert rec.only()[1][-1 - len(out):-1] == tuple(ptr(t) for t in out)


@pytest.mark.parametrize("quantised", [False, True])
def test_the_late_rank_and_rerank_methods_reach_their_entries_unchanged(rec, made_on_the_host, quantised):
    q = resident(torch.zeros(S, E, dtype=torch.bfloat16))
    tok = resident(torch.zeros(S, L, E, dtype=torch.bfloat16))
    lengths, targets, cand = i32(S), i32(S), i32(S, C)
    for ragged in (False, True):
        sl, heads = stand_in(ragged, quantised)
        tab = heads if quantised else heads + (None,)                         # (table, scales or NULL) of the rank and rerank entries
        W = 1 if ragged else 2
        off, bv = (ptr(sl._seg[0]), ptr(sl._seg[1])) if ragged else (None, None)
        for allow, stride in ((None, 0), (i32(W), 0), (i32(S, W), W)):
            kw = {} if allow is None else {"allow": allow}
            mask = (None if allow is None else ptr(allow), stride)

            got = sl.rank(q, targets, **kw)
            ws = sl._ws[("rank", S)]
            assert ws.numel() == 6                                              # 8 * S * (1 + one block) bytes
            outs = (ptr(got.rank), ptr(got.score), ptr(got.total), STREAM)
            if ragged:
                assert rec.only() == ("drn_shortlist_segments_rank", tab + (ptr(q), off, bv, ptr(targets)) + mask
                                      + (6, 3, 1, 64, 3, BF16, ptr(ws), 48) + outs, ("shortlist_segments_rank", 2.0 * 3 * 6 * 64))
            else:
                assert rec.only() == ("drn_shortlist_rank", tab + (ptr(q), ptr(targets)) + mask + (40, 64, 3, BF16, ptr(ws), 48) + outs,
                                      ("shortlist_rank", 2.0 * 3 * 40 * 64))

            got = sl.rerank(cand, q, **kw)                                      # n = None: min(C, 128) = 5
            ws = sl._ws[("rerank", S, C, 5)]
            assert ws.numel() == 15                                             # S * ceil(5 / 16) * min(5, 16)
            rows, videos = (6, 3) if ragged else (40, 40)
            assert rec.only() == ("drn_shortlist_rerank", tab + (ptr(q), None, off, ptr(cand)) + mask
                                  + (rows, videos, 64, 3, 1, 5, 5, BF16, ptr(ws), 15, ptr(got.ids), ptr(got.scores), ptr(got.n), STREAM),
                                  ("shortlist_rerank", 2.0 * 3 * 1 * 5 * (float(rows) / videos) * 64))
            if not ragged:
                continue

            got = sl.shortlist_late(tok, lengths, N, **kw)
            ws = sl._ws[("late", S, N)]
            assert ws.numel() == 6                                              # S * one block * min(n, 256)
            assert rec.only() == ("drn_shortlist_late_topn_q8" if quantised else "drn_shortlist_late_topn",
                                  heads + (ptr(tok), ptr(lengths), off, bv) + mask
                                  + (6, 3, 1, 64, 3, 4, 2, BF16, ptr(ws), 6, ptr(got.ids), ptr(got.scores), ptr(got.n), STREAM),
                                  ("shortlist_late_topn", 2.0 * 3 * 4 * 6 * 64))

            got = sl.rank_late(tok, lengths, targets, **kw)
            ws = sl._ws[("rank_late", S)]
            assert ws.numel() == 6
            assert rec.only() == ("drn_shortlist_late_rank", tab + (ptr(tok), ptr(lengths), off, bv, ptr(targets)) + mask
                                  + (6, 3, 1, 64, 3, 4, BF16, ptr(ws), 48, ptr(got.rank), ptr(got.score), ptr(got.total), STREAM),
                                  ("shortlist_late_rank", 2.0 * 3 * 4 * 6 * 64))

            got = sl.rerank_late(cand, tok, lengths, N, **kw)
            ws = sl._ws[("rerank", S, C, N)]
            assert ws.numel() == 6                                              # S * ceil(5 / 16) * min(2, 16)
            assert rec.only() == ("drn_shortlist_rerank", tab + (ptr(tok), ptr(lengths), off, ptr(cand)) + mask
                                  + (6, 3, 64, 3, 4, 5, 2, BF16, ptr(ws), 6, ptr(got.ids), ptr(got.scores), ptr(got.n), STREAM),
                                  ("shortlist_rerank", 2.0 * 3 * 4 * 5 * (6.0 / 3) * 64))
        assert sorted(map(str, sl._ws)) == sorted(map(str, [("rank", S), ("rerank", S, C, 5)] + (
            [("late", S, N), ("rank_late", S), ("rerank", S, C, N)] if ragged else [])))
