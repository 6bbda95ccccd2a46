"""The device feature store on the MI355X (drn_amd.store, drn_pool_props): StoreLoader batches against collate_data's on the committed
mini dataset (which tests/test_data_cpu.py pins to the reference's recorded batches), the kernel against torch's max over every
run on synthetic stores (both dtypes, vector / element-wise rows, LDS and through-L2 videos, ragged padding, poisoned outputs),
bad video indices, hipGraph capture, and training / evaluation / grounding fed from the store against the host feed, bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_trainer_gpu import hip_model      # noqa: E402  (the mini dataset's model: same seeded weights, same placement)

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "charades_mini")
DEV = "cuda:0"
TOK = lambda s: s.split()


def mini_cfg(stage):
    from drn_amd.utils.synthetic import default_cfg
    cfg = default_cfg("TINY", 12, stage)
    cfg["feature_type"] = "C3D"
    cfg["C3D"] = {"feature_root": "./features", "feature_dim": 12, "ft_window_size": 16, "ft_overlap": 0.5}
    cfg["props_file_path"] = "./data/dataset/Charades/mini_props.txt"
    return cfg


def mini(split, stage=1):
    from drn_amd.data import CharadesSTA
    return CharadesSTA(mini_cfg(stage), split, MINI, TOK)


def host_loader(ds, batch_size, dtype, **kw):
    from torch.utils.data import DataLoader
    from drn_amd.data import collate_data
    collate = functools.partial(collate_data, feature_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None)
    return DataLoader(ds, batch_size=batch_size, shuffle=False, collate_fn=collate, **kw)


def assert_batches_equal(got, want):
    assert got[0] == want[0]
    for i in range(1, 8):
        a, b = got[i], want[i]
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (i, a.dtype, b.dtype, a.shape, b.shape)
        assert a.is_cuda == (i <= 5), i                          # the five model inputs on the device, nprops / nframes on the host
        assert torch.equal(a.cpu(), b), i


# -- 1. mini dataset -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("split", ["train", "test"])
def test_store_loader_batches_equal_collate_data_on_the_mini_dataset(split, dtype):
    """D = 12: 48-byte rows in fp32 (three 16-byte chunks, the vector path) and 24-byte rows in bf16 (the element-wise path)."""
    from drn_amd.store import FeatureStore, StoreLoader
    ds = mini(split)
    st = FeatureStore.from_dataset(ds, DEV, dtype)
    assert st.feats.is_cuda and st.nbytes == FeatureStore.bytes_of(st.feats.shape[0], 12, dtype, len(st), st.win.shape[0])
    for bs in (1, 3, len(ds)):
        want, got = list(host_loader(ds, bs, dtype)), list(StoreLoader(ds, st, bs))
        assert len(got) == len(want) > 0
        for g, w in zip(got, want):
            assert_batches_equal(g, w)


# -- 2. synthetic stores ---------------------------------------------------------------------------------------------------------------
def synthetic(D, dtype, kind, B=6, seed=0):
    """Videos v0..v4 of 1, 2, 37 rows, one a row longer than the LDS path holds at this geometry (read through L2) and one of up to
    120 rows that the LDS path still holds (more rows than a workgroup stages in one pass), with 0, 1, 70, 5 and 40 proposals; the
    windows of every video with proposals start with a single row, the whole video, the clamped last row (lo == hi == S - 1) and a
    middle row, the rest are random runs of up to 70 rows."""
    from drn_amd import ops
    from drn_amd.store import FeatureStore
    g = torch.Generator().manual_seed(seed)
    limit = ops.pool_props_lds_rows(B, D, ops.dtype_code(torch.empty(0, dtype=dtype)))
    rows = [1, 2, 37, (limit + 1) if limit else 300, min(120, limit) if limit else 120]
    counts = [0, 1, 70, 5, 40]
    videos = []
    for v, (S, P) in enumerate(zip(rows, counts)):
        f = torch.randn(S, D, generator=g) * 3
        if kind == "negative":
            f = -f.abs() - 1.0                                   # every maximum is negative: an accumulator seeded with 0 returns 0
        elif kind == "large":
            f = torch.where(torch.rand(S, D, generator=g) < 0.3, torch.sign(f) * 3.0e38, f)       # +-3e38: finite in both dtypes
        lo = torch.randint(0, S, (P,), generator=g)
        hi = torch.minimum(lo + torch.randint(0, 70, (P,), generator=g), torch.tensor(S - 1))
        fixed = [(0, 0), (0, S - 1), (S - 1, S - 1), (S // 2, S // 2)]
        for i in range(min(P, len(fixed))):
            lo[i], hi[i] = fixed[i]
        if P == 1:
            lo[0], hi[0] = 0, S - 1
        videos.append(("v%d" % v, f, lo.numpy(), hi.numpy(), torch.rand(P, 2, generator=g, dtype=torch.float64).numpy() + 0.25, 8 * S))
    return FeatureStore.from_tensors(videos, DEV, dtype), limit


def expected(st, ids, T):
    """torch on the device: feats[lo:hi + 1].max(0).values per proposal, zeros past each video's count (and for ids outside)."""
    out = torch.zeros((len(ids), T, st.D), dtype=st.dtype, device=DEV)
    pse = torch.zeros((len(ids), T, 2), dtype=torch.float64, device=DEV)
    seg, prop, win = st.seg_off.tolist(), st.prop_off.tolist(), st.win.cpu().tolist()
    for b, v in enumerate(ids):
        if not 0 <= v < len(st):
            continue
        for t in range(prop[v + 1] - prop[v]):
            lo, hi = win[prop[v] + t]
            out[b, t] = st.feats[seg[v] + lo:seg[v] + hi + 1].max(0).values
        pse[b, :prop[v + 1] - prop[v]] = st.pse[prop[v]:prop[v + 1]]
    return out, pse


def poisoned(st, B, T):
    return (torch.full((B, T, st.D), float("nan"), dtype=st.dtype, device=DEV),
            torch.full((B, T, 2), -7.5, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("kind", ["normal", "negative", "large"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [8, 12, 264, 4096])
def test_pool_props_equals_the_max_over_every_run(D, dtype, kind):
    st, limit = synthetic(D, dtype, kind)
    assert st.max_rows > limit                                   # one video is read through L2, the others from LDS
    assert st.nrows.tolist()[:3] == [1, 2, 37] and st.nprops.tolist() == [0, 1, 70, 5, 40]
    assert st.nrows[4] <= limit or limit == 0                     # the long staged video: several staging passes per workgroup
    ids = [2, 3, 0, 1, 2, 4]                                     # proposal counts 70, 5, 0, 1, 70, 40: T = 70, ragged; video 2 twice
    out, out_pse = poisoned(st, len(ids), 70)
    feats, pse, nprops = st.gather(ids, out=out, out_pse=out_pse)
    assert feats is out and pse is out_pse                       # the buffers passed are the ones written
    assert nprops.dtype == torch.int64 and not nprops.is_cuda and nprops.tolist() == [70, 5, 0, 1, 70, 40]
    want, want_pse = expected(st, ids, 70)
    assert not torch.isnan(feats.float()).any(), "an element of out was never written"
    assert torch.equal(feats, want)
    assert torch.equal(pse, want_pse)
    for b, n in enumerate(nprops.tolist()):
        assert not feats[b, n:].float().abs().any() and not pse[b, n:].abs().any()      # padding rows: exactly zero
    if kind == "negative":
        assert float(feats[0].float().max()) < 0
    # fresh buffers, by name, at the batch's own T; and a T above it
    f2, p2, n2 = st.gather(["v1", "v3"])
    assert f2.shape == (2, 5, D) and torch.equal(f2, want[[3, 1], :5]) and torch.equal(p2, want_pse[[3, 1], :5]) and n2.tolist() == [1, 5]
    f3, _, _ = st.gather(torch.tensor([3], dtype=torch.int64), T=9)
    assert f3.shape == (1, 9, D) and torch.equal(f3[:, :5], want[1:2, :5]) and not f3[:, 5:].float().abs().any()


@pytest.mark.parametrize("B", [4, 32, 130])
def test_pool_props_on_staged_slabs_at_the_benchmarked_row_length(B):
    """D = 4096 in bf16 with videos of 120, 60 and 37 rows and runs of 8, 16, 32 and 64 rows (plus the full video and random runs):
    B = 4, 32 and 130 take column blocks of 8, 16 and 64 chunks, so a workgroup stages 32, 16 and 4 rows per pass and every slab
    the LDS path holds is filled in several passes; at B = 130 the 120-row video is beyond the LDS limit and goes through L2."""
    from drn_amd import ops
    from drn_amd.store import FeatureStore
    limit = ops.pool_props_lds_rows(B, 4096, ops.BF16)
    assert limit == {4: 512, 32: 256, 130: 64}[B]               # (8, 16, 64 chunks of 16 bytes per column block)
    g = torch.Generator().manual_seed(B)
    videos = []
    for v, S in enumerate([120, 60, 37]):
        lo, hi = [0], [S - 1]
        for rows in (8, 16, 32, 64):
            for start in (0, 3, S - rows):
                if 0 <= start and start + rows <= S:
                    lo.append(start)
                    hi.append(start + rows - 1)
        r = torch.randint(0, S, (20,), generator=g)
        lo += r.tolist()
        hi += torch.minimum(r + torch.randint(0, 64, (20,), generator=g), torch.tensor(S - 1)).tolist()
        P = len(lo)
        videos.append(("s%d" % v, torch.randn(S, 4096, generator=g) * 3, lo, hi, torch.rand(P, 2, generator=g, dtype=torch.float64).numpy(), 8 * S))
    st = FeatureStore.from_tensors(videos, DEV, torch.bfloat16)
    T = int(st.nprops.max())
    ids = [(5 * i + 1) % 3 for i in range(B)]
    out, out_pse = poisoned(st, B, T)
    f, p, n = st.gather(ids, out=out, out_pse=out_pse)
    want, want_pse = expected(st, [0, 1, 2], T)
    assert n.tolist() == [int(st.nprops[i]) for i in ids]
    assert torch.equal(f, want[ids]) and torch.equal(p, want_pse[ids])


def test_pool_props_with_one_clip_and_with_many():
    """B = 1 (the narrowest column blocks) and B = 130 (more workgroups than the chip holds at once, wide column blocks)."""
    st, _ = synthetic(264, torch.bfloat16, "normal", B=1)
    f, p, _ = st.gather([2])
    want, want_pse = expected(st, [2], 70)
    assert torch.equal(f, want) and torch.equal(p, want_pse)
    st, _ = synthetic(4096, torch.bfloat16, "normal", B=130)
    ids = [(7 * i) % 5 for i in range(130)]
    out, out_pse = poisoned(st, 130, 70)
    f, p, _ = st.gather(ids, out=out, out_pse=out_pse)
    want, want_pse = expected(st, [0, 1, 2, 3, 4], 70)
    assert torch.equal(f, want[ids]) and torch.equal(p, want_pse[ids])


# -- 3. video ids -----------------------------------------------------------------------------------------------------------------------
def test_a_bad_host_index_raises_and_launches_nothing():
    from drn_amd import ops
    from drn_amd._lib import DrnError
    st, _ = synthetic(264, torch.bfloat16, "normal")
    out, out_pse = poisoned(st, 3, 70)
    ops.kernel_timer = []
    try:
        for bad in (len(st), -1):
            with pytest.raises(DrnError, match="reads video"):
                st.gather([2, bad, 4], out=out, out_pse=out_pse, T=70)
        with pytest.raises(DrnError, match="proposals, T = 4"):
            st.gather([0, 1, 3], T=4)                            # T below a listed count
        with pytest.raises(DrnError):
            st.gather(["v0", "nobody"])
        launches = len(ops.kernel_timer)
    finally:
        ops.kernel_timer = None
    torch.cuda.synchronize()
    assert launches == 0
    assert torch.isnan(out.float()).all() and bool((out_pse == -7.5).all())


@pytest.mark.parametrize("D,dtype", [(264, torch.bfloat16), (12, torch.bfloat16), (12, torch.float32)])
def test_a_bad_device_index_yields_zero_rows_for_that_clip_only(D, dtype):
    st, _ = synthetic(D, dtype, "normal")
    ids = [2, len(st), 4, -1, 1 << 30]
    out, out_pse = poisoned(st, len(ids), 70)
    vids = torch.tensor(ids, dtype=torch.int32, device=DEV)
    feats, pse, nprops = st.gather(vids, out=out, out_pse=out_pse, T=70)
    assert nprops is None
    want, want_pse = expected(st, ids, 70)
    assert torch.equal(feats, want) and torch.equal(pse, want_pse)
    for b in (1, 3, 4):
        assert not feats[b].float().abs().any() and not pse[b].abs().any()


# -- 4. graph capture -------------------------------------------------------------------------------------------------------------------
def test_a_captured_gather_follows_the_index_buffer():
    from drn_amd.graph import capture_graph
    st, _ = synthetic(264, torch.bfloat16, "normal")
    vids = torch.tensor([2, 3, 1], dtype=torch.int32, device=DEV)
    out, out_pse = poisoned(st, 3, 70)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st.gather(vids, out=out, out_pse=out_pse, T=70)          # (warm: the code object is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_graph(g, s):                                    # one stream: a linear graph
        st.gather(vids, out=out, out_pse=out_pse, T=70)
    for ids in ([2, 3, 1], [4, 2, 4], [1, 0, 3]):
        vids.copy_(torch.tensor(ids, dtype=torch.int32))
        out.fill_(float("nan"))
        out_pse.fill_(-7.5)
        g.replay()
        torch.cuda.synchronize()
        want, want_pse = expected(st, ids, 70)
        assert torch.equal(out, want) and torch.equal(out_pse, want_pse), ids


# -- 5. end to end on the mini dataset ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_training_from_the_store_is_bit_identical_to_the_host_feed(graph):
    from drn_amd import functional as DF
    from drn_amd import trainer as T
    from drn_amd.store import FeatureStore, StoreLoader
    ds = mini("train")
    st = FeatureStore.from_dataset(ds, DEV, torch.bfloat16)
    runs = {}
    for feed in ("store", "host"):
        m = hip_model(1, cfg=mini_cfg(1))
        m.set_compute_dtype(torch.bfloat16)
        tr = T.Trainer(m, 1, lr=1e-4, graph=graph, graph_warmup=1)
        loader = StoreLoader(ds, st, 4) if feed == "store" else host_loader(ds, 4, torch.bfloat16)
        means = [tr.train_epoch(loader, e) for e in range(2)]
        torch.cuda.synchronize()
        DF.flush_bn_counters()
        if graph and feed == "store":
            assert any(s.graph is not None for s in tr._slots.values()), "no step was ever captured"
        runs[feed] = (means, {k: v.detach().clone() for k, v in m.state_dict().items()})
    assert all(np.isfinite(runs["store"][0])) and runs["store"][0] == runs["host"][0]
    for k, v in runs["host"][1].items():
        assert torch.equal(v, runs["store"][1][k]), k


def test_evaluate_predict_and_ground_from_the_store_equal_the_host_feed():
    from drn_amd import Grounder, group_by_video
    from drn_amd import trainer as T
    from drn_amd.store import FeatureStore, StoreLoader
    ds = mini("test", 3)
    st = FeatureStore.from_dataset(ds, DEV, torch.bfloat16)
    m = hip_model(3, cfg=mini_cfg(3))
    m.set_compute_dtype(torch.bfloat16)
    tr = T.Trainer(m, 3, lr=1e-4)
    host, store = host_loader(ds, 4, torch.bfloat16), StoreLoader(ds, st, 4)
    a, b = tr.evaluate(host, with_results=False), tr.evaluate(store, with_results=False)
    assert a[0] == b[0] and a[1] == b[1] and list(a[2]) == list(b[2]) and a[3] is None and b[3] is None
    assert tr.predict(host) == tr.predict(store)
    m.eval()
    grounder = Grounder(m)
    for names, pse, feats, _, tok, qlen, _, _ in host_loader(ds, len(ds), torch.bfloat16):
        names, tok, qlen = names + names[::-1], torch.cat([tok, tok.flip(0)]), torch.cat([qlen, qlen.flip(0)])
        unique, vid = group_by_video(names)                      # every video is asked about twice
        assert len(unique) < len(names)
        first = torch.tensor([names.index(u) for u in unique])
        want = grounder.ground(tok.to(DEV), qlen.to(DEV), feats[first].to(DEV), pse[first].to(DEV), vid)
        sf, sp, _ = st.gather(unique)
        assert torch.equal(sf.cpu(), feats[first]) and torch.equal(sp.cpu(), pse[first])
        got = grounder.ground(tok.to(DEV), qlen.to(DEV), sf, sp, vid)
        for f in ("seg", "score", "level", "index", "n"):
            assert torch.equal(getattr(got, f), getattr(want, f)), f
