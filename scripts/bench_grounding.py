#!/usr/bin/env python
"""Queries per second of grounding without a ground truth (drn_amd.Grounder.ground: shared prop_fc, device post-processor, device
NMS) against the same queries through Trainer.evaluate(with_results=False) (every query its own clip, prop_fc with the gate fused,
loss + drn_eval_recall), in one process on one MI355X.

Shape: T = 256 proposals, D = 4096, bf16, Q = 32 queries per batch over V = Q / share videos, share = Q/V in {1, 2, 4}.  Both paths
read device-resident batches (no host -> device copy inside the window) and end in one device synchronise per timed window.  The
all variants (the eager ones, and `fused` / `graph` / `fused+graph` of each sharing factor) are run interleaved, `--rounds` rounds of `--iters` batches each after `--warmup` untimed batches per variant; the
figure reported is the median over rounds, with the min / max next to it.  evaluate() is timed on V = Q clips whatever the share
(it has no way to share a video), so its three figures are repeats of one measurement and show the spread.

Writes profiles/grounding_bench.json (or --out).  Needs the GPU: there is no CPU path to time."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--props", type=int, default=256)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--shares", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grounding.py measures on the GPU; none is visible")
    from drn_amd import Grounder
    from drn_amd import trainer as TR
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict, synthetic_batch
    dev = torch.device("cuda:0")
    Q, T, D = args.queries, args.props, args.dim
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    cfg = default_cfg("C3D" if D == 4096 else "SYN", D, 3)
    model = mainModel(VOCAB_SIZE, as_namespace(cfg), compute_dtype=dtype)
    model.load_state_dict(seeded_state_dict(model, 0))
    model = model.to(dev).eval()
    trainer = TR.Trainer(model, 3, lr=1e-4)
    grounder = Grounder(model, top_k=5, nms_overlap=0.45)
    engines = {"fused": Grounder(model, top_k=5, nms_overlap=0.45, fused=True),
               "graph": Grounder(model, top_k=5, nms_overlap=0.45, graph=True, max_graphs=8),
               "fused+graph": Grounder(model, top_k=5, nms_overlap=0.45, fused=True, graph=True, max_graphs=8)}
    tok, qlen, feats, pse, gt, nprops, nframes = synthetic_batch(Q, T, D, seed=11)
    tok, qlen, feats, pse, gt = (t.to(dev) for t in (tok, qlen, feats, pse, gt))
    names = ["v%d" % i for i in range(Q)]
    eval_batch = (names, pse, feats, gt, tok, qlen, nprops, nframes)

    variants = {}
    for share in args.shares:
        assert Q % share == 0
        V = Q // share
        vid = (torch.arange(Q) % V).to(dev)                  # every video asked `share` times, not sorted by video
        f, p = feats[:V].contiguous(), pse[:V].contiguous()
        index = None if share == 1 else vid
        variants["ground_share%d" % share] = (lambda f=f, p=p, index=index: grounder.ground(tok, qlen, f, p, index))
        # the opt-in paths, same inputs: one-launch eval conv blocks, hipGraph replay, both (the base is the eager variant above)
        for tag, g in engines.items():
            variants["ground_%s_share%d" % (tag, share)] = (lambda g=g, f=f, p=p, index=index: g.ground(tok, qlen, f, p, index))
    variants["evaluate"] = lambda: trainer.evaluate([eval_batch], with_results=False)

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for fn in variants.values():
        window(fn, args.warmup)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():                       # interleaved: a drift of the clock or the host hits all variants alike
            times[k].append(window(fn, args.iters))
    result = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, device-resident batches",
              "shape": {"queries": Q, "props": T, "dim": D, "dtype": args.dtype, "stage": 3},
              "method": {"iters_per_window": args.iters, "rounds": args.rounds, "warmup_batches": args.warmup, "interleaved": True,
                         "statistic": "median over rounds of the mean batch time of a window"},
              "variants": {}}
    for k, ts in times.items():
        med = statistics.median(ts)
        result["variants"][k] = {"ms_per_batch": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4),
                                 "queries_per_s": round(Q / med, 1)}
    base = result["variants"]["evaluate"]["ms_per_batch"]
    for k, v in result["variants"].items():
        v["speedup_vs_evaluate"] = round(base / v["ms_per_batch"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
