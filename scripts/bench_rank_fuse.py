#!/usr/bin/env python
"""rank_fuse beside rank_fuse_reference on the same device tensors -- what a caller would write in torch without it.

    python scripts/bench_rank_fuse.py [--rounds 7] [--out profiles/rank_fuse_bench.json]

Shapes (M lists, C entries a list, S sentences) = (2, 128, 1), (2, 128, 64), (8, 1024, 1), (8, 1024, 64) over V = 100,000 videos,
fused to lists of n = C.  Per shape the fused list is first asserted equal, bit for bit, to rank_fuse_reference evaluated on the
host; whether the reference evaluated ON THE DEVICE gives the same bits is recorded, not required.  Then the two take turns inside every
round: a round times a window of back-to-back calls from the host clock to a device synchronise and divides by the calls; the medians
over the rounds are reported with their minimum and maximum.  No ratio is required: the numbers are what they are."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 100000
SHAPES = ((2, 128, 1), (2, 128, 64), (8, 1024, 1), (8, 1024, 64))      # (M, C, S)
WINDOW_S = 0.1                                                         # a timed window aims at this much work
DEV = "cuda:0"


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def overlapping_lists(M, C, S, seed):
    """M lists (S, C) int32 of distinct positions drawn from a shared pool of 4 C videos spread over [0, V): every list holds about a
    quarter of the pool, so most videos are held by some lists and not by others, as the shortlists of different encoders are."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    pool = 4 * C
    step = V // pool
    return [(torch.rand(S, pool, generator=g, device=DEV).argsort(dim=1)[:, :C] * step).to(torch.int32).contiguous() for _ in range(M)]


def window(run, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def bench_shape(M, C, S, rounds):
    from drn_amd import rank_fuse, rank_fuse_reference
    lists = torch.stack(overlapping_lists(M, C, S, seed=1000 * M + C + S))
    n = C
    w = torch.tensor([1.0, 0.5, 2.0, 0.25, 4.0, 0.125, 3.0, 1.5][:M], dtype=torch.float32, device=DEV)
    out = rank_fuse(lists, V, n, weights=w)
    host = rank_fuse_reference(lists.cpu(), V, n, weights=w.cpu())
    for f in ("ids", "scores", "n"):
        a, b = getattr(out, f).cpu(), getattr(host, f)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (M, C, S, f, "rank_fuse is not the definition's")
    on_device = rank_fuse_reference(lists, V, n, weights=w)
    device_equal = all(torch.equal(getattr(out, f).view(torch.int32), getattr(on_device, f).view(torch.int32)) for f in ("ids", "scores", "n"))
    runs = {"rank_fuse": lambda: rank_fuse(lists, V, n, weights=w, out=out), "reference": lambda: rank_fuse_reference(lists, V, n, weights=w)}
    reps = {}
    for name, run in runs.items():                          # warm, then size the window from one timed call
        run()
        reps[name] = max(1, min(2000, int(WINDOW_S * 1e6 / max(window(run, 3), 1.0))))
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, run in runs.items():
            times[name].append(window(run, reps[name]))
    ours, theirs = statistics.median(times["rank_fuse"]), statistics.median(times["reference"])
    return {"M": M, "C": C, "S": S, "V": V, "n": n, "sort_words": max(256, 1 << (M * C - 1).bit_length()), "calls_per_window": reps,
            "rank_fuse_us": spread(times["rank_fuse"]), "reference_on_device_us": spread(times["reference"]),
            "reference_over_rank_fuse": theirs / ours, "reference_on_device_gives_the_same_bits": device_equal,
            "candidates_per_sentence": {"min": int(out.n.min()), "max": int(out.n.max())}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="default profiles/rank_fuse_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_fuse: no GPU: a timing taken anywhere else says nothing (there is no CPU fallback)")
    out = args.out or os.path.join(ROOT, "profiles", "rank_fuse_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the lists resident, every shape warmed",
           "method": {"interleaved": True, "rounds": args.rounds,
                      "statistic": "median [min, max] over rounds; a round = the mean call time of one window of back-to-back calls (~%.1f s)" % WINDOW_S,
                      "clock": "host clock from before the first call of a window to after a device synchronise: launch-inclusive us per call",
                      "yardstick": "rank_fuse_reference on the same device tensors: per list a scatter_reduce_(amin) into (S, V + 1), a "
                                   "divide and an add over (S, V), then one stable sort of (S, V) float64 -- what a caller writes in "
                                   "torch today; it allocates its (S, V) temporaries inside the clock, rank_fuse writes into out=",
                      "lists": "distinct positions a list, drawn from a shared pool of 4 C videos: every list holds about a quarter of it",
                      "what_this_does_not_say": "no kernel-only time (no profiler run); the kernel's time is expected to be set by its two "
                                                "LDS sorts of `sort_words` words, one workgroup a sentence: S = 1 uses one CU of 256; no "
                                                "ratio is required of these numbers"},
           "shapes": []}
    for M, C, S in SHAPES:
        row = bench_shape(M, C, S, args.rounds)
        res["shapes"].append(row)
        print("M = %d, C = %d, S = %d: rank_fuse %.1f us, reference on the device %.1f us (x %.1f), same bits on the device: %s" % (
            M, C, S, row["rank_fuse_us"]["median"], row["reference_on_device_us"]["median"], row["reference_over_rank_fuse"],
            row["reference_on_device_gives_the_same_bits"]), flush=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
