"""Host side of the device feature store (drn_amd.store) without a GPU: the window arithmetic as a function against the literal
index list of CharadesSTA.__getitem__, CharadesSTA.meta, what the store builder refuses, StoreLoader's batch composition against
DataLoader + collate_data, and the C-ABI boundary of drn_pool_props (declared, exported, argument errors before any launch)."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from drn_amd.data import CharadesSTA, collate_data, proposal_windows

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "charades_mini")
CFG = {"feature_type": "C3D", "C3D": {"feature_root": "./features", "feature_dim": 12, "ft_window_size": 16, "ft_overlap": 0.5},
       "props_file_path": "./data/dataset/Charades/mini_props.txt"}
TOK = lambda s: s.split()


def literal(proposals, num_frames, n_segments, window, overlap):
    """CharadesSTA.__getitem__'s loop, statement for statement, without the features: index lists and normalised bounds."""
    interval = int(window * (1 - overlap))
    last = n_segments - 1
    lists, props = [], []
    for start, end in proposals:
        props.append((start / num_frames, end / num_frames))
        first = (int(start) // interval) * interval
        if end - start <= window:
            idx = [first // interval]
        else:
            idx = [x // interval for x in range(first, end, interval)]
        lists.append(sorted(min(last, x) for x in idx))
    return lists, np.array(props)


def check(proposals, num_frames, n_segments, window, overlap):
    lo, hi, pse = proposal_windows(proposals, num_frames, n_segments, window, overlap)
    lists, props = literal(proposals, num_frames, n_segments, window, overlap)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and pse.dtype == np.float64
    assert lo.shape == hi.shape == (len(proposals),) and pse.shape == (len(proposals), 2)
    for i, idx in enumerate(lists):
        # the clamp min(last, x) REPEATS the last stored segment once per window that lies past it ([.., 79, 80, 80, 80]): the rows
        # the max runs over are the list's distinct entries, and those must be exactly range(lo, hi + 1); a repeat anywhere but
        # at the last segment would be a different list
        assert sorted(set(idx)) == list(range(int(lo[i]), int(hi[i]) + 1)), (proposals[i], num_frames, n_segments, window, overlap, idx, lo[i], hi[i])
        assert idx == list(range(int(lo[i]), int(hi[i]))) + [int(hi[i])] * (len(idx) - int(hi[i] - lo[i])), idx
        assert len(idx) == int(hi[i] - lo[i]) + 1 or idx[-1] == n_segments - 1
        assert 0 <= lo[i] <= hi[i] < n_segments
    if len(proposals):
        np.testing.assert_array_equal(pse, props)


@pytest.mark.parametrize("split", ["train", "test"])
def test_proposal_windows_on_every_video_of_the_mini_dataset(split):
    ds = CharadesSTA(CFG, split=split, root=MINI, tokenizer=TOK)
    assert len(ds.props) >= 2
    for vid, (num_frames, proposals) in ds.props.items():
        n_segments = len(torch.load(os.path.join(ds.ft_root, "%s.pt" % vid)))
        check(proposals, num_frames, n_segments, ds.ft_window_size, ds.ft_overlap)


def test_proposal_windows_on_random_cases():
    rng = random.Random(7)
    seen = {"short": 0, "past": 0, "empty": 0, "long": 0, "clamped": 0}
    for case in range(2000):
        window, overlap = rng.choice([16, 32]), rng.choice([0, 0.5, 0.75])
        interval = int(window * (1 - overlap))
        num_frames = rng.randint(1, 600)
        full = max(1, -(-num_frames // interval))
        n_segments = rng.choice([full, max(1, full - rng.randint(1, 4)), 1, full + 1])       # fewer stored segments than frames too
        proposals = []
        for _ in range(rng.randint(0, 12)):
            start = float(rng.randint(0, num_frames))
            kind = rng.random()
            if kind < 0.15:
                end = int(start)                                                             # start == end
                seen["empty"] += 1
            elif kind < 0.35:
                end = num_frames + rng.randint(1, 200)                                       # ends past the video (an uncapped table)
                seen["past"] += 1
            else:
                end = rng.randint(int(start), num_frames)
            if rng.random() < 0.3:
                start += rng.random() * 0.99                                                 # fractional start frames (the table holds floats)
                end = max(end, int(start))
            seen["long" if end - start > window else "short"] += 1
            proposals.append((start, end))
        check(proposals, num_frames, n_segments, window, overlap)
        lo, hi, _ = proposal_windows(proposals, num_frames, n_segments, window, overlap)
        seen["clamped"] += int(((lo == n_segments - 1) & (hi == n_segments - 1)).sum())
    assert all(v > 100 for v in seen.values()), seen


def test_proposal_windows_refuses_a_zero_interval():
    with pytest.raises(ValueError):
        proposal_windows([(0.0, 10)], 100, 5, 16, 1.0)
    with pytest.raises(ValueError):
        proposal_windows([(0.0, 10)], 100, 5, 1, 0.5)


def test_meta_opens_no_feature_file(tmp_path):
    cfg = dict(CFG, C3D=dict(CFG["C3D"], feature_root=str(tmp_path / "no" / "such" / "dir")))
    ds = CharadesSTA(cfg, split="train", root=MINI, tokenizer=TOK)
    ref = CharadesSTA(CFG, split="train", root=MINI, tokenizer=TOK)
    assert not os.path.exists(ds.ft_root)
    with pytest.raises(Exception):
        ds[0]
    for i in range(len(ds)):
        vid, tokens, gt, num_frames = ds.meta(i)
        want = ref[i]
        assert vid == want[0] and torch.equal(tokens, want[4]) and gt == want[3] and num_frames == want[7]


def _video(name, S, D, P, seed, window=16, overlap=0.5):
    g = torch.Generator().manual_seed(seed)
    num_frames = S * 8
    props = [(float(8 * (i % S)), min(num_frames, 8 * (i % S) + 8 * (1 + i % 5))) for i in range(P)]
    lo, hi, pse = proposal_windows(props, num_frames, S, window, overlap)
    return name, torch.randn(S, D, generator=g), lo, hi, pse, num_frames


def test_store_builder_refuses_bad_inputs_before_uploading():
    from drn_amd._lib import DrnError
    from drn_amd.store import FeatureStore
    good = [_video("a", 5, 8, 3, 0), _video("b", 7, 8, 4, 1)]
    st = FeatureStore.from_tensors(good, "cpu", torch.bfloat16)
    assert len(st) == 2 and st.D == 8 and st.dtype == torch.bfloat16 and st.nprops.tolist() == [3, 4] and st.max_rows == 7
    assert st.nbytes == 12 * 8 * 2 + 3 * 12 + 7 * 24 == FeatureStore.bytes_of(12, 8, torch.bfloat16, 2, 7)
    assert torch.equal(st.feats, torch.cat([good[0][1], good[1][1]]).bfloat16())
    assert st.seg_off.tolist() == [0, 5, 12] and st.prop_off.tolist() == [0, 3, 7]
    for bad in (float("nan"), float("inf"), -float("inf")):
        v = list(_video("c", 4, 8, 2, 2))
        v[1] = v[1].clone()
        v[1][2, 3] = bad
        with pytest.raises(DrnError, match="NaN or Inf"):
            FeatureStore.from_tensors(good + [tuple(v)], "cpu", torch.float32)
    big = list(_video("c", 4, 8, 2, 2))
    big[1] = torch.full((4, 8), 3.4e38)                        # finite in fp32, rounds to Inf in bf16
    FeatureStore.from_tensors(good + [tuple(big)], "cpu", torch.float32)
    with pytest.raises(DrnError, match="NaN or Inf"):
        FeatureStore.from_tensors(good + [tuple(big)], "cpu", torch.bfloat16)
    with pytest.raises(DrnError, match="feature dimension"):
        FeatureStore.from_tensors(good + [_video("c", 4, 12, 2, 2)], "cpu", torch.float32)
    with pytest.raises(DrnError, match="max_bytes"):
        FeatureStore.from_tensors(good, "cpu", torch.bfloat16, max_bytes=st.nbytes - 1)
    with pytest.raises(DrnError, match="max_bytes"):
        # (refused before the upload: "meta" is a device nothing can be copied to or from)
        FeatureStore.from_tensors(good, "meta", torch.bfloat16, max_bytes=10)
    FeatureStore.from_tensors(good, "cpu", torch.bfloat16, max_bytes=st.nbytes)
    with pytest.raises(DrnError):
        st.gather(["a"])                                       # a host store has no gather: no CPU fallback


def test_store_from_dataset_packs_the_mini_dataset():
    from drn_amd.store import FeatureStore
    ds = CharadesSTA(CFG, split="train", root=MINI, tokenizer=TOK)
    st = FeatureStore.from_dataset(ds, "cpu", torch.float32)
    assert st.names == list(ds.props) and st.D == 12
    for i, vid in enumerate(st.names):
        f = torch.load(os.path.join(ds.ft_root, "%s.pt" % vid))
        assert torch.equal(st.feats[int(st.seg_off[i]):int(st.seg_off[i + 1])], f)
        assert st.nprops[i] == len(ds.props[vid][1]) and st.nframes[i] == ds.props[vid][0]


@pytest.mark.parametrize("split", ["train", "test"])
@pytest.mark.parametrize("batch_size,drop_last", [(1, False), (3, False), (3, True), (64, False)])
@pytest.mark.parametrize("seeded", [False, True])
def test_store_loader_composes_batches_like_the_dataloader(split, batch_size, drop_last, seeded):
    from torch.utils.data import DataLoader, RandomSampler
    from drn_amd.store import FeatureStore, StoreLoader
    ds = CharadesSTA(CFG, split=split, root=MINI, tokenizer=TOK)
    st = FeatureStore.from_dataset(ds, "cpu", torch.float32)
    sampler = lambda: RandomSampler(ds, generator=torch.Generator().manual_seed(11)) if seeded else None
    ref = DataLoader(ds, batch_size=batch_size, shuffle=False, sampler=sampler(), drop_last=drop_last, collate_fn=collate_data)
    got = StoreLoader(ds, st, batch_size, shuffle=False, sampler=sampler(), drop_last=drop_last)
    assert len(got) == len(ref) and hasattr(got, "sampler")
    n = 0
    for want, (names, vids, gt, tok, qlen, nprops, nframes) in zip(ref, got.host_batches()):
        assert names == want[0] and [st.names[v] for v in vids.tolist()] == names
        for a, b in ((gt, want[3]), (tok, want[4]), (qlen, want[5]), (nprops, want[6]), (nframes, want[7])):
            assert a.dtype == b.dtype and torch.equal(a, b)
        n += 1
    assert n == len(ref)


def test_store_loader_shuffles_with_a_generator_and_never_indexes_the_dataset():
    from drn_amd.store import FeatureStore, StoreLoader
    ds = CharadesSTA(CFG, split="train", root=MINI, tokenizer=TOK)
    st = FeatureStore.from_dataset(ds, "cpu", torch.float32)

    class NoItems(object):
        props = ds.props

        def meta(self, i):
            return ds.meta(i)

        def __len__(self):
            return len(ds)

        def __getitem__(self, i):
            raise AssertionError("StoreLoader called dataset[%d]" % i)
    order = lambda seed: [n for b in StoreLoader(NoItems(), st, 2, shuffle=True, generator=torch.Generator().manual_seed(seed)).host_batches()
                          for n in b[0]]
    assert order(1) == order(1) and sorted(order(1)) == sorted(s["vid"] for s in ds.samples)
    assert any(order(s) != order(1) for s in range(2, 8))


def built_lib():
    from drn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_pool_props_is_declared_and_exported_at_abi_9():
    from drn_amd import _lib, ops
    lib = built_lib()
    for name in ("drn_pool_props", "drn_pool_props_lds_rows"):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
    assert lib.drn_abi_version() == 9
    assert list(lib.drn_pool_props.argtypes) == _lib.SIGNATURES["drn_pool_props"]
    assert callable(ops.pool_props)
    # the LDS path's row limit is host logic: a column block never needs more than the 64 KB a workgroup may ask for
    assert ops.pool_props_lds_rows(32, 4096, ops.BF16) * 16 * 16 == 65536      # 1024 workgroups of 16 chunks at the benchmarked shape
    assert ops.pool_props_lds_rows(5, 12, ops.BF16) == 0                       # 24-byte rows: the element-wise path
    assert ops.pool_props_lds_rows(5, 12, ops.F32) > 0 and ops.pool_props_lds_rows(5, 8, ops.BF16) > 0


def test_pool_props_argument_errors_answer_before_anything_is_launched():
    """Null pointers, a negative count, T below a listed count, a host index outside the store, a dtype the kernel does not have:
    each an error code with a text and no device work (this runs without a GPU)."""
    from drn_amd import _lib
    L = built_lib()
    p = 0x1000
    ok = dict(feats=p, seg_off=p, prop_off=p, win=p, pse=p, vids=p, out=p, out_pse=p, Nv=4, B=3, T=8, D=64, dtype=1, max_rows=0)

    def call(**kw):
        d = _lib.PoolPropsDesc(**dict(ok, **kw))
        rc = L.drn_pool_props(ctypes.byref(d), None)
        return rc, L.drn_last_error()
    assert call(dtype=2)[0] == -1 and b"bad dtype 2" in call(dtype=2)[1]
    for field in ("feats", "seg_off", "prop_off", "win", "pse", "vids", "out", "out_pse"):
        rc, msg = call(**{field: None})
        assert rc == -1 and b"null pointer" in msg, field
    for field in ("Nv", "B", "T", "max_rows"):
        rc, msg = call(**{field: -1})
        assert rc == -1 and b"negative count" in msg, field
    assert call(D=0)[0] == -1
    vids = (ctypes.c_int32 * 3)(0, 4, 1)
    rc, msg = call(vids_host=ctypes.cast(vids, ctypes.c_void_p))
    assert rc == -1 and b"clip 1 reads video 4 of 4" in msg
    vids = (ctypes.c_int32 * 3)(0, -1, 1)
    assert call(vids_host=ctypes.cast(vids, ctypes.c_void_p))[0] == -1
    counts = (ctypes.c_int32 * 3)(8, 2, 9)
    rc, msg = call(counts_host=ctypes.cast(counts, ctypes.c_void_p))
    assert rc == -1 and b"clip 2 has 9 proposals, T = 8" in msg
    assert call(pse=0x1008)[0] == -1 and b"16-byte aligned" in call(pse=0x1008)[1]
    assert L.drn_pool_props(None, None) == -1
    # the wrapper refuses host tensors (no CPU fallback)
    from drn_amd import ops
    z = torch.zeros(4, 8)
    with pytest.raises(_lib.DrnError):
        ops.pool_props(z, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                       torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), 1, torch.zeros(1, 1, 8),
                       torch.zeros(1, 1, 2, dtype=torch.float64))
