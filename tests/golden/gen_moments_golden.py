#!/usr/bin/env python
"""Record what the REFERENCE evaluator picks -- its own sort, then its own temporal NMS -- on seeded lists of (start, end, score)
candidates: tests/golden/moments.json, the fixture of tests/test_grounding_cpu.py and tests/test_grounding_gpu.py.

The reference is imported (utils/evaluate_utils.PostProcessRunner), never copied: each case goes through
_postprocess_raw_results_no_merge (evaluate_utils.py:91-107) and nms_temporal (:186-212) and the picks are written down.  CPU only.

Every candidate travels as [start, end, original index, score]: the reference reads the boundaries from the front and the score from
the back of a prediction, so the index rides through its sort untouched and the recorded picks are positions in the INPUT list,
taken from the reference's own ordering (no re-implementation of its tie rule here).  Values are float32 numbers handed over as
numpy float64 scalars: what the device sees, widened as the host path widens them, and 0/0 between two empty segments is the NaN
numpy makes of it (never `<= overlap`: struck out) rather than the ZeroDivisionError plain Python floats raise there.

usage: python tests/golden/gen_moments_golden.py --reference <checkout of the reference>"""
import argparse
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OVERLAPS = (0.25, 0.45, 0.65)
KS = (1, 5, 100)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def random_list(rng, n, grid=None):
    """n segments inside [0, 1]; grid: boundaries and scores on multiples of 1 / grid (many exact coincidences)."""
    a, b = rng.random(n), rng.random(n)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    s = rng.random(n)
    if grid:
        lo, hi, s = np.round(lo * grid) / grid, np.round(hi * grid) / grid, np.round(s * grid) / grid
    return f32(lo), f32(hi), f32(s)


def families(rng):
    """(tag, starts, ends, scores) lists built to hit the rules one by one, then random ones of growing length."""
    out = []
    out.append(("single", f32([0.25]), f32([0.75]), f32([0.5])))
    out.append(("single_empty_segment", f32([0.5]), f32([0.5]), f32([0.9])))
    # exact score ties: all equal / pairs / ties between overlapping and between disjoint segments
    lo, hi, _ = random_list(rng, 12)
    out.append(("all_scores_equal", lo, hi, f32([0.5] * 12)))
    lo, hi, s = random_list(rng, 16)
    s[1::2] = s[::2]
    out.append(("score_ties_in_pairs", lo, hi, s))
    out.append(("ties_disjoint", f32([0.0, 0.3, 0.6, 0.8]), f32([0.2, 0.5, 0.7, 1.0]), f32([0.7, 0.7, 0.7, 0.7])))
    # duplicate segments, with equal and with different scores
    lo, hi, s = random_list(rng, 10)
    lo, hi = np.concatenate([lo, lo]), np.concatenate([hi, hi])
    out.append(("duplicates_same_score", lo, hi, np.concatenate([s, s])))
    out.append(("duplicates_other_score", lo, hi, np.concatenate([s, s[::-1].copy()])))
    # zero-length segments: 0/0 against each other (NaN), 0 / len against a real one
    out.append(("empty_segments_only", f32([0.1, 0.1, 0.5, 0.9]), f32([0.1, 0.1, 0.5, 0.9]), f32([0.4, 0.8, 0.6, 0.2])))
    lo, hi, s = random_list(rng, 14)
    hi[::3] = lo[::3]
    out.append(("empty_among_real", lo, hi, s))
    lo, hi, s = random_list(rng, 14)
    hi[::2] = lo[::2]
    s[:] = 0.25
    out.append(("empty_among_real_tied", lo, hi, s))
    # nested, disjoint, chained
    c = f32(np.linspace(0.02, 0.48, 12))
    out.append(("nested", c, f32(1.0) - c, f32(rng.random(12))))
    out.append(("nested_best_inside", c, f32(1.0) - c, f32(np.linspace(0.1, 0.9, 12))))
    e = f32(np.linspace(0.0, 1.0, 11))
    out.append(("disjoint_tiling", e[:-1], e[1:], f32(rng.random(10))))
    out.append(("chain_half_overlap", f32(np.linspace(0.0, 0.8, 17)), f32(np.linspace(0.0, 0.8, 17)) + f32(0.1), f32(rng.random(17))))
    # the post-processor's own fallback moment
    out.append(("whole_video", f32([0.0]), f32([1.0]), f32([1.0])))
    # more than one wave stride (64 lanes), up to what three pyramid levels of top-n candidates hold
    for n in (65, 96, 130, 200):
        out.append(("long_%d" % n,) + random_list(rng, n))
    out.append(("long_grid_150",) + random_list(rng, 150, grid=16))
    while len(out) < 24:
        n = int(rng.integers(2, 48))
        out.append(("random_%d" % n,) + random_list(rng, n, grid=(8 if len(out) % 2 else None)))
    return out


def reference_picks(runner_cls, lo, hi, s, overlap, k):
    preds = [[np.float64(a), np.float64(b), i, np.float64(c)] for i, (a, b, c) in enumerate(zip(lo, hi, s))]
    runner = runner_cls({"video": [{"query": "q", "gt": [0.0, 1.0], "node_predictions": preds, "level": [[0] * len(preds)]}]})
    runner._postprocess_raw_results_no_merge("")
    ordered = runner.processed_results["video"][0]["node_predictions"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                # (the 0/0 of two empty segments)
        picks = runner.nms_temporal([p[0] for p in ordered], [p[1] for p in ordered], [p[-1] for p in ordered], overlap)
    return [int(ordered[i][2]) for i in picks[:k]], len(picks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(HERE, "moments.json"))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    sys.path.insert(0, ref)
    os.chdir(ref)                                   # (its constructor opens a vocabulary file by a relative path)
    from utils.evaluate_utils import PostProcessRunner
    cases = []
    for rep in range(9):                            # 9 seeds x 24 lists, each with one (overlap, k) pair: every family meets every pair
        rng = np.random.default_rng(1000 + rep)
        for j, (tag, lo, hi, s) in enumerate(families(rng)):
            overlap, k = OVERLAPS[(rep + j) % 3], KS[((rep + j) // 3) % 3]
            picks, survivors = reference_picks(PostProcessRunner, lo, hi, s, overlap, k)
            # str(float32) is the shortest decimal that reads back as the same float32
            cases.append({"tag": "%s_r%d" % (tag, rep), "overlap": overlap, "k": k, "survivors": survivors, "picks": picks,
                          "preds": [[float(str(a)), float(str(b)), float(str(c))] for a, b, c in zip(lo, hi, s)]})
    with open(args.out, "w") as f:
        json.dump({"overlaps": list(OVERLAPS), "ks": list(KS), "cases": cases}, f, separators=(",", ":"))
    print("%d cases -> %s (%d bytes)" % (len(cases), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
