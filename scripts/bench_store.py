#!/usr/bin/env python
"""Measures the device feature store (drn_amd.store) on the MI355X -> profiles/store_bench.json:

  kernel   drn_pool_props alone at B = 32, D = 4096, bf16, videos of 120 rows, runs of 8 / 16 / 32 / 64 rows (the reference's
           sliding-window scales at interval 8), T = 256 and T = 32: launch-inclusive microseconds per call over ~0.3 s windows and
           the ALGORITHMIC bytes (both outputs once + each clip's slab once) over that time, cache-warm and with rotating buffers;
  trainer  Trainer.train_epoch, graph mode, B = 32, T = 256, fed three ways in one process, interleaved, median over rounds:
           StoreLoader (the store feed), the same batches pre-built on the device, the same batches in pinned host memory (bf16) --
           the last two are the feeds the trainer had before the store;
  host     samples/s of DataLoader(CharadesSTA, num_workers = 8) + collate_data(bf16) on a synthetic on-disk dataset of the same
           geometry (written to a temporary directory), for context.

    python scripts/bench_store.py [--out profiles/store_bench.json] [--rounds 5] [--skip-host]"""
import argparse
import functools
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, D, S, NV, INTERVAL, WINDOW = 32, 4096, 120, 64, 8, 16
SCALES = (8, 16, 32, 64)          # rows per run
EPOCHS_PER_WINDOW = 4             # a timed trainer window: 4 epochs of 32 steps (~0.3 s)


def proposals_of(T, frames):
    """T (start, end) frame pairs: the four scales in equal parts, each sliding evenly over the video."""
    out = []
    per = T // len(SCALES)
    for rows in SCALES:
        length = rows * INTERVAL
        for i in range(per):
            start = (frames - length) * i // max(per - 1, 1)
            out.append((float(start), min(start + length, frames)))
    return out


def build_store(T, dtype, device, seed=0):
    from drn_amd.data import proposal_windows
    from drn_amd.store import FeatureStore
    g = torch.Generator().manual_seed(seed)
    frames = S * INTERVAL
    videos = []
    for v in range(NV):
        lo, hi, pse = proposal_windows(proposals_of(T, frames), frames, S, WINDOW, 1 - INTERVAL / WINDOW)
        videos.append(("V%03d" % v, torch.randn(S, D, generator=g), lo, hi, pse, frames))
    return FeatureStore.from_tensors(videos, device, dtype)


def bench_kernel(T, rounds, window_s=0.3):
    """Launch-inclusive times: windows of about window_s seconds of back-to-back launches from Python on one stream, device events
    around each window.  "warm": one output buffer and the same 32 videos every launch, so the slabs and (at T = 32) the output can
    stay in the 256 MB Infinity Cache.  "rotating": six output buffers (402 MB at T = 256) and both halves of the store in turn, so
    every launch writes lines that have left the cache.  Neither is a kernel-trace time: scripts/rocprof_kernels.py on a rocprofv3
    --kernel-trace run of `bench_store.py --kernel-only` gives that (profiles/store_kernel_trace.txt)."""
    from drn_amd import ops
    st = build_store(T, torch.bfloat16, "cuda:0")
    runs = (st.win[:, 1] - st.win[:, 0] + 1).float()
    vids = [torch.arange(B, dtype=torch.int32, device="cuda:0") + B * h for h in range(NV // B)]
    outs = [torch.empty((B, T, D), dtype=torch.bfloat16, device="cuda:0") for _ in range(6)]
    pse = torch.empty((B, T, 2), dtype=torch.float64, device="cuda:0")

    def window(reps, rotate):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            st.gather(vids[i % len(vids)] if rotate else vids[0], out=outs[i % len(outs)] if rotate else outs[0], out_pse=pse, T=T)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    window(20, True)
    reps = max(50, int(window_s / (window(200, False) * 1e-6)))
    times = {"warm": [], "rotating": []}
    for _ in range(rounds):                                                    # interleaved
        times["warm"].append(window(reps, False))
        times["rotating"].append(window(reps, True))
    algo = outs[0].numel() * 2 + pse.numel() * 8 + B * S * D * 2
    res = {"B": B, "T": T, "D": D, "dtype": "bf16", "rows_per_video": S, "run_rows_mean": float(runs.mean()), "run_rows": list(SCALES),
           "launches_per_window": reps, "algorithmic_bytes": algo, "lds_rows_limit": ops.pool_props_lds_rows(B, D, ops.BF16),
           "note": "launch-inclusive: back-to-back launches issued from Python on one stream; algorithmic bytes over that time is not "
                   "an HBM rate (warm: slabs and output may be served by the Infinity Cache)"}
    for kind, ts in times.items():
        us = statistics.median(ts)
        res[kind] = {"us_median": us, "us_rounds": ts, "algorithmic_bytes_per_s": algo / (us * 1e-6)}
    return res


class SyntheticQueries(object):
    """What StoreLoader needs of a dataset: len and meta(i) = (vid, tokens, gt, num_frames)."""

    def __init__(self, store, n, lq=8, seed=1):
        g = np.random.default_rng(seed)
        self.rows = []
        for i in range(n):
            s = float(g.uniform(0.0, 0.5))
            self.rows.append((store.names[int(g.integers(0, len(store)))], torch.from_numpy(g.integers(1, 1000, size=lq)),
                              (s, s + float(g.uniform(0.15, 0.5))), S * INTERVAL))

    def __len__(self):
        return len(self.rows)

    def meta(self, i):
        return self.rows[i]


def bench_trainer(T, rounds, nbatches=32):
    from drn_amd import trainer as TR
    from drn_amd.model import mainModel
    from drn_amd.store import StoreLoader
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict
    st = build_store(T, torch.bfloat16, "cuda:0")
    ds = SyntheticQueries(st, B * nbatches)
    feeds = {"store": StoreLoader(ds, st, B)}
    # the same nbatches batches three ways (2.1 GB resident on the device, and again in pinned host memory, at T = 256)
    feeds["device"] = list(StoreLoader(ds, st, B))
    feeds["pinned_host_bf16"] = [tuple(t.cpu().pin_memory() if torch.is_tensor(t) and t.is_cuda else t for t in b) for b in feeds["device"]]
    trainers = {}
    for name in feeds:
        m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("C3D", D, 1)), compute_dtype=torch.bfloat16)
        m.load_state_dict(seeded_state_dict(m, 0))
        trainers[name] = TR.Trainer(m.to("cuda:0"), 1, lr=1e-5, graph=True)
        for e in range(3):                                                     # warm-up, capture, replay
            trainers[name].train_epoch(feeds[name], e)
        torch.cuda.synchronize()
    times = {name: [] for name in feeds}
    for r in range(rounds):
        for name in feeds:                                                     # interleaved: every round times every feed once
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(EPOCHS_PER_WINDOW):
                trainers[name].train_epoch(feeds[name], 3 + r * EPOCHS_PER_WINDOW + k)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / (nbatches * EPOCHS_PER_WINDOW))
    res = {"B": B, "T": T, "D": D, "dtype": "bf16", "steps_per_epoch": nbatches, "epochs_per_window": EPOCHS_PER_WINDOW, "rounds": rounds, "store_bytes": st.nbytes,
           "store_videos": len(st), "feeds": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["feeds"][name] = {"ms_per_step_median": med, "ms_per_step_rounds": ts, "clips_per_s": B / (med * 1e-3)}
    return res


def write_dataset(root, T):
    """A Charades-STA-shaped dataset of the benchmarked geometry on disk: NV videos of S x D fp32 features, T proposals each."""
    base = os.path.join(root, "data", "dataset", "Charades")
    os.makedirs(base)
    os.makedirs(os.path.join(root, "features"))
    g = torch.Generator().manual_seed(0)
    frames = S * INTERVAL
    names = ["V%03d" % v for v in range(NV)]
    words = ["w%d" % i for i in range(50)]
    json.dump({w: i + 1 for i, w in enumerate(words)}, open(os.path.join(base, "Charades_word2id.json"), "w"))
    json.dump({n: 24.0 for n in names}, open(os.path.join(base, "Charades_fps_dict.json"), "w"))
    json.dump({n: frames / 24.0 for n in names}, open(os.path.join(base, "Charades_duration.json"), "w"))
    with open(os.path.join(base, "props.txt"), "w") as f:
        for n in names:
            f.write("# %s\n%s\n%d\n" % (n, n, frames))
            for s, e in proposals_of(T, frames):
                f.write("%d %d\n" % (s, e))
    with open(os.path.join(base, "Charades_sta_train.txt"), "w") as f:
        for i in range(NV * 8):
            f.write("%s 1.0 9.0##%s.\n" % (names[i % NV], " ".join(words[(i + k) % 50] for k in range(8))))
    for n in names:
        torch.save(torch.randn(S, D, generator=g), os.path.join(root, "features", "%s.pt" % n))
    return {"feature_type": "C3D", "C3D": {"feature_root": "./features", "feature_dim": D, "ft_window_size": WINDOW,
                                           "ft_overlap": 1 - INTERVAL / WINDOW}, "props_file_path": "./data/dataset/Charades/props.txt"}


def bench_host(T, workers=8, batches=8):
    from torch.utils.data import DataLoader
    from drn_amd.data import CharadesSTA, collate_data
    root = tempfile.mkdtemp(prefix="drn_store_bench_")
    try:
        cfg = write_dataset(root, T)
        ds = CharadesSTA(cfg, "train", root, lambda s: s.split())
        loader = DataLoader(ds, batch_size=B, shuffle=False, num_workers=workers,
                            collate_fn=functools.partial(collate_data, feature_dtype=torch.bfloat16))
        it = iter(loader)
        next(it)                                                               # worker start-up is not the pipeline's rate
        t0 = time.perf_counter()
        n = 0
        for _ in range(batches):
            n += len(next(it)[0])
        dt = time.perf_counter() - t0
        return {"B": B, "T": T, "D": D, "workers": workers, "samples": n, "samples_per_s": n / dt,
                "note": "files in the page cache of a temporary directory; no pinning, no copy to the device"}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="the kernel windows alone, short (for a rocprofv3 --kernel-trace run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_store.py measures on an MI355X; no GPU found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0)}

    def section(key, value):                                                   # the file is rewritten after every section
        res[key] = value
        print(json.dumps({key: value}), flush=True)
        json.dump(res, open(args.out, "w"), indent=1)
    if args.kernel_only:
        section("kernel", [bench_kernel(256, 1, window_s=0.02), bench_kernel(32, 1, window_s=0.02)])
        return
    section("kernel", [bench_kernel(256, args.rounds), bench_kernel(32, args.rounds)])
    if not args.skip_trainer:
        section("trainer", bench_trainer(256, args.rounds))
    if not args.skip_host:
        section("host_pipeline", bench_host(256))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
