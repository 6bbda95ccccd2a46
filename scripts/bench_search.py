#!/usr/bin/env python
"""Measures Grounder.search on a resident FeatureStore and on a SearchIndex built from it, on the MI355X -> profiles/search_bench.json:

  search   ms per search of S in {1, 8} sentences against 64 videos (120 rows x 4096, bf16; bench_store.py's store), T = 256 and
           T = 32, four ways in one process, interleaved, median over rounds: the store path and the index path, each eager and by
           graph replay.  Host clock around windows of searches that end in a device synchronise; the default chunk (all 64 videos in
           one step).  The two paths' Hits are compared field for field at every shape;
  build    ms per SearchIndex.build of that store (synchronised), and nbytes of the store and of the index;
  kernel   drn_gate_gather_packed alone at the search's largest step (512 pairs) and at 64 pairs: launch-inclusive microseconds per
           call over ~0.3 s windows and the bytes it WRITES (Q T (C + P) elements) over that time.

    python scripts/bench_search.py [--out profiles/search_bench.json] [--rounds 5]

  --shortlist  instead of the above -> profiles/search_pairs_bench.json: S = 8 sentences, each with its own N random candidates of
           the 64 videos (N in {4, 16, 64 = all}), Grounder.search(candidates=) beside the full cartesian search of the same
           Grounders, on the store and on the index, eager and by graph replay; same store, same protocol.  At N = all the two
           searches do the same device work and their Hits are compared field for field.

  --evaluate   instead of the above -> profiles/search_eval_bench.json: one evaluation pass over 8 batches of S = 8 annotated sentences
           (drn_amd.evaluate_search: search, drn_search_recall on the Hits, ONE copy at the end of the pass) beside the same batches
           scored on the host (search, Hits.tolist(), metrics.search_first_hits, per batch), on the store and on the index, eager and
           by graph replay; same store, same protocol.  The two tables are compared.

  --quantized  instead of the above -> profiles/search_q8_bench.json: a SearchIndex built with quantize="mxfp8" (block-scaled FP8 codes,
           dequantised inside drn_gate_gather_packed_q8) beside the plain index of the same store, by the same Grounders in one process:
           nbytes of both (and SearchIndex.bytes_of, which they must equal), ms per build, ms per search (S in {1, 8}, T in {256, 32},
           eager and by graph replay), the two gather kernels alone at 512 and 64 pairs, and -- from evaluate_search on random
           annotations -- the two recall tables and the share of sentences whose first hit names the same video on both indexes.
           The quantised Hits are compared field for field with those of index.dequantized().

  --mx-conv0   instead of the above -> profiles/search_mx8conv_bench.json: the SAME quantised index searched by Grounder(conv0="mxfp8")
           (conv0 on block-scaled FP8 MFMAs straight from the codes, the sentence gate folded into quantised weights) beside the default
           Grounder (drn_gate_gather_packed_q8, then conv0 on bf16 MFMAs), in one process: ms per search (S in {1, 8}, T in {256, 32},
           eager and by graph replay), drn_conv0_mx8 alone beside gather + conv0 GEMM alone at 512 and 64 pairs, the once-per-search
           weights launch alone, the first-hit agreement and evaluate_search recalls of the two modes on random annotations, and the
           largest ratio of drn_conv0_mx8's error to its derived bound on the random case of tests/test_search_mx8conv_gpu.py.

  --mx-conv0-fused   instead of the above -> profiles/search_mx8conv_fused_bench.json, by --mx-conv0's protocol on one quantised index:
           Grounder(conv0="mxfp8", fused=True) (drn_conv0_mx8_bn: conv0 on LDS-staged FP8 tiles with BatchNorm, ReLU and the gate in its
           epilogue) beside Grounder(conv0="mxfp8") and the default Grounder(fused=True), ms per search (S in {1, 8}, T in {256, 32},
           eager and by graph replay); the launch alone at 512 and 64 pairs beside its yardsticks (a) drn_conv0_mx8 +
           bn_eval_scale_shift + bn_apply_multi back to back and (b) the gather + the one-launch conv0 block of the default fused path;
           the first-hit agreement of the fused and the unfused mode; the error / tolerance ratios of tests/test_search_mx8fused_gpu.py.

  --mx-conv0-tiles   instead of the above -> profiles/search_mx8conv_tiles_bench.json, by the same protocol on one quantised index: the
           fused launch behind bn_eval_scale_shift on every tile drn_conv0_mx8_bn_tile ships, on the tile the chooser picks ("auto") and
           on the wide tile through drn_conv0_mx8_bn, beside the default fused path's gather + one-launch conv0 block, at 512 and 64
           pairs x T in {256, 32}, at the grids between them on either side of the rule's two crossovers (W = 16 ... 56 and 80 ... 255 wide
           workgroups) and at a T = 32 shortlist step of 8 sentences x 4 candidates (as planned and shuffled); searches by
           graph replay (S in {1, 8}, T in {256, 32}) with the chooser as shipped, with the chooser held to the wide tile, and on the
           default Grounder(fused=True).  The chooser's rule rests on these numbers.

  --device-candidates   instead of the above -> profiles/search_device_candidates_bench.json, by the same protocol (64 videos x 120 x
           4096, bf16, T in {256, 32}, S = 8, median [min, max] of 5 interleaved rounds): (a) a two-stage search -- Shortlister.shortlist
           then Grounder.search(candidates=) -- with the shortlist's ids passed as the device tensor, beside the only way the parent of
           this feature has: the same shortlist read back with .tolist() and passed as host lists to the same kind of Grounder (N in
           {4, 16}, a plain and a quantised index, eager and by graph replay); (b) the shortlist launch alone (V = 64 and a synthetic
           65,536 x 512 bf16 table, S in {1, 8, 64}, n in {16, 128}) beside torch.matmul + torch.topk on the same tensors and beside
           the time to read the table once at the chip's bandwidth; (c) the plan launch alone at S * N = 32 and 512; the largest
           error / tolerance ratio of tests/test_shortlist_gpu.py's random case.  Random embeddings: nothing here says anything about
           recall.

  --segment-shortlist   instead of the above -> profiles/search_segment_shortlist_bench.json: Shortlister(offsets=).shortlist alone
           (drn_shortlist_segments_topn, all three launches) on R = 65,536 rows x 512 in bf16 laid out as 65,536 videos x 1 row, 4,096 x
           16 and 546 x 120 (the last video takes 136 rows, to make R), S in {1, 8, 64}, n in {16, 128}, launch-inclusive us, median
           [min, max] of 5 interleaved rounds, beside (a) the plain shortlist kernel on the same R rows as R videos and (b)
           torch.matmul + scatter_reduce_(amax) + torch.topk, with the read floor (R * E * 2 bytes per 16 sentences at 6.29 TB/s) beside
           every figure; the derived condition that the 16-row and 120-row layouts take no longer than the 1-row layout by more than
           its max - min, shape by shape; the largest error / tolerance ratio of tests/test_segment_shortlist_gpu.py's random case.
           Random embeddings: nothing here says anything about recall.

  --quantized-shortlist  instead of the above -> profiles/search_q8_shortlist_bench.json: Shortlister(quantize="mxfp8").shortlist
           (drn_shortlist_topn_q8 on 65,536 videos x 1 row, drn_shortlist_segments_topn_q8 on 4,096 x 16 and 546 x 120; R = 65,536 rows
           x 512, bf16 queries, S in {1, 8, 64}, n in {16, 128}, launch-inclusive us, median [min, max] of 5 interleaved rounds) beside
           the plain table over the SAME dequantised rows ranked by the plain kernels in the same process, with each table's read
           floor; the bytes of both tables (asserted equal to Shortlister.bytes_of); the time to quantise the table; whether the two
           answers are the same bits; the tolerance_ratio of tests/test_q8_shortlist_gpu.py's lossy case; and, on the random table, the
           share of sentences whose first video and whose n-list agree with those of the ORIGINAL unquantised table.  Random
           embeddings: nothing here says anything about recall.

  --filtered-shortlist  instead of the above -> profiles/search_filtered_shortlist_bench.json: Shortlister.shortlist(allow=) on R =
           65,536 rows x 512 (bf16 queries, n = 16, S in {1, 8, 64}; the plain table as 65,536 x 1, the ragged one as 4,096 x 16, the
           quantised plain table at S = 8), launch-inclusive us, median [min, max] of 5 interleaved rounds in one process, under five
           masks -- all ones, random 50 %, random 1 %, a contiguous 1/16 of the videos (15/16 of the blocks dark), a per-sentence random
           1 % -- beside (a) the unmasked launch on the same table, the parent's code unchanged, and (b), for the shared masks, the
           parent's only exact way: Shortlister(emb[keep].contiguous()), shortlist, keep[ids], with and without the construction.
           Two conditions are derived, not measured, and reported shape by shape: (C1) the all-ones mask costs the unmasked launch plus
           at most 128 (144 ragged) mask words per workgroup -- the difference against (a) is printed, in capitals where it exceeds (a)'s
           max - min; (C2) the contiguous-1/16 and the 1 % mask do no more work than the all-ones mask and may not take longer than it
           beyond its max - min.  Random embeddings: nothing here says anything about recall.

  --late-shortlist      instead of the above -> profiles/search_late_shortlist_bench.json: Shortlister.shortlist_late (drn_shortlist_late_topn,
           both launches) on R = 65,536 rows x 512 in bf16 laid out as 4,096 x 16 and 546 x 120, n = 16, S in {1, 8, 64}, with L = 8 all
           live, L = 16 all live, L = 16 with lengths 6 and L = 32 with lengths 16; launch-inclusive us, median [min, max] of 5
           interleaved rounds in one process, beside (a) what a caller can do without the feature -- torch.matmul on the flattened
           tokens, scatter_reduce_(amax), a masked sum, torch.topk -- at the shapes whose (S L, R) matrix and index stay below 512 rows, and
           (b) shortlist() on the same table with the S L flattened tokens as queries: another answer, the same MFMA work and table reads
           per 16 query rows.  Two conditions are derived, not measured, and reported shape by shape: (C1) L = 16 all live takes no longer
           than (b) at 16 S query rows beyond (b)'s max - min; (C2) L = 32 with lengths 16 takes no longer than L = 16 all live beyond the
           latter's max - min, with a control beside it: L = 16 all live once more on other random tokens.  The largest error / tolerance ratio of tests/test_late_shortlist_gpu.py's random case.  Random
           embeddings: nothing here says anything about recall.

  --rank                instead of the above -> profiles/search_rank_bench.json: Shortlister.rank (drn_shortlist_rank / _segments_rank, all
           three launches) on R = 65,536 rows x 512 in bf16 as 65,536 x 1 and 4,096 x 16, and rank_late (drn_shortlist_late_rank) at L = 16
           on the ragged layout, S in {1, 8, 64}; launch-inclusive us, median [min, max] of 5 interleaved rounds in one process, beside (a)
           the shortlist of n = 16 on the same table and queries, the parent's code path, and (b) what a caller does today for depth
           past 128: torch.matmul (plus scatter_reduce_(amax) when ragged, a sum over the tokens when late), two comparisons and sums.
           One condition is derived, not measured, and reported HOLDS / MISSED shape by shape: (C1) rank takes no longer than (a) beyond
           (a)'s max - min.  Agreement counts: whether every rank below 16 is the target's place in (a)'s list, and how many sentences
           equal (b) (near-ties in bf16 may differ).  Then evaluate_shortlist on PLANTED queries -- a target's row plus noise, no trained
           encoder -- on the plain table and on quantize="mxfp8" side by side: recall at 1 / 10 / 100 / 1000 and the median rank.

  --rerank              instead of the above -> profiles/search_rerank_bench.json: Shortlister.rerank_late (drn_shortlist_rerank, both
           launches) on R = 65,536 rows x 512 in bf16 laid out as 4,096 x 16 and 546 x 120, S in {1, 8, 64}, L = 16 all live, n = 16, on
           C = 128 and C = 32 distinct random candidates a sentence; launch-inclusive us, median [min, max] of 5 interleaved rounds in one
           process, beside (A) what the parent offers for the same answer -- pack_allow of the candidates' mask + shortlist_late(allow=),
           the fields asserted equal before timing -- and (B) the unmasked shortlist_late; and rerank (one query row) beside pack_allow +
           shortlist(allow=).  One condition is derived, not measured, and reported holds / MISSED shape by shape: (R1) rerank_late
           takes no longer than (A) beyond (A)'s max - min.  Random embeddings and candidates: nothing here says anything about recall.

  --sharded-shortlist   instead of the above -> profiles/search_sharded_shortlist_bench.json: ShardedShortlister.shortlist (every shard's
           entry, then drn_shortlist_merge_lists) on R = 65,536 rows x 512 in bf16 laid out as 65,536 x 1 and 4,096 x 16, cut into K = 1 /
           4 / 16 equal shards, S in {1, 8, 64}, n in {16, 128}; launch-inclusive us, median [min, max] of 5 interleaved rounds in one
           process, beside the single Shortlister over the same rows (every field asserted equal before timing) and the merge launch
           alone; one mixed object (half FP8, half bf16) and shortlist_late at 16 tokens on K = 4, each beside its single table.  One
           condition is derived, not measured, and reported HOLDS / MISSED shape by shape: (G1) adding 1,024 rows by append + shortlist
           takes less than torch.cat + Shortlister + shortlist on the same tensors by more than the latter's max - min.  Random
           embeddings: nothing here says anything about recall.

  --sharded-rank   instead of the above -> profiles/search_sharded_rank_bench.json: ShardedShortlister.rank, rerank (C = 128, n = 16) and --
           on the ragged layout -- rank_late (16 tokens) on the same two layouts and K = 1 / 4 / 16 equal shards, S in {1, 8, 64}, by the
           protocol of --sharded-shortlist, beside the single Shortlister over the same rows (every field asserted equal before timing);
           and append + rank beside torch.cat + Shortlister + rank on the same tensors, the gain judged against the latter's own
           max - min.  No time is required of the sharded calls (2 K + 3 launches against 3): the ratios are what is reported.

  --compact   instead of the above -> profiles/search_compact_bench.json: ShardedShortlister.compact on the same two layouts, all-bf16,
           all-FP8 and half / half shards (target plain), K = 4 and 16, all kept and a random 10 % dropped, beside the route the parent
           offers on the same shards and mask -- mx8_dequantize of the FP8 shards, torch.cat, index_select, Shortlister(...) -- by a host
           clock to a device synchronise, the two taking turns in every round, the result asserted equal to compact_reference byte for
           byte before timing.  (G1) compact() takes less than the route by more than the route's own max - min: HOLDS / DOES NOT HOLD
           per shape, no absolute time required.  Without a bar: the rows launches' bytes per second (bytes from the shapes, device
           events around each launch: launch-inclusive) against the HBM peak, and shortlist and rank at S = 8, n = 16 on the compacted
           table beside the K = 16 sharded object under the same mask.

  --pooled   instead of the above -> profiles/search_pooled_bench.json: Shortlister.pooled(how="mean") with group=None and group=4 on
           65,536 rows x 512 bf16 as 4,096 videos x 16 and as 5,120 videos of 1 / 3 / 0 / 17 / 43 rows, from a bf16 and from an FP8
           table (target "same"), beside the parent's only way to such a table, in torch on the device -- (mx8_dequantize,) an fp32
           index_add_, a divide, a cast, Shortlister(...) -- by a host clock to a device synchronise, the two taking turns in every
           round, every field asserted equal to pool_segments_reference (evaluated on the host) before timing.  The condition:
           pooled() takes no longer than that route beyond the route's own max - min, HOLDS / DOES NOT HOLD per shape, no absolute
           time required.  For orientation only: the bytes read and written over 8 TB/s.

  --fused-shortlist   instead of the above -> profiles/search_fused_shortlist_bench.json, on 65,536 rows x 512 bf16 at S = 1 / 8 / 64,
           launch-inclusive us from device events around windows of back-to-back calls, the variants taking turns in every round:
           (a) Shortlister.scores beside shortlist(q, 16) on the same table, 65,536 x 1 plain and 4,096 x 16 ragged -- the derived
           condition: scores() takes no longer than shortlist() beyond that launch's own max - min, HOLDS / MISSED per shape, no
           absolute time required; (b) FusedShortlister.shortlist at M = 2, the 4,096 x 16 ragged table and its pooled table, beside
           torch.matmul per table + scatter_reduce_(amax) + the weighted sum + torch.topk, the fused list asserted equal to
           fused_shortlist_reference of the tables' own scores() before timing."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

D, NV = 4096, 64
STATE = ("seg", "score", "video", "level", "rank", "n")


def make_model():
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("C3D", D, 3)), compute_dtype=torch.bfloat16)
    m.load_state_dict(seeded_state_dict(m, 0))
    m = m.to("cuda:0").eval()
    with torch.no_grad():                                  # a classifier that passes most locations: every pair has candidates
        m.fcos.head.cls_logits.bias.fill_(0.5)
    return m


def sentences(S, seed):
    from drn_amd.utils.synthetic import synthetic_batch
    tok, qlen = synthetic_batch(S, 32, 64, seed=seed)[:2]
    return tok.to("cuda:0"), qlen.to("cuda:0")


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def bench_search(model, store, index, T, S, rounds, window_s=0.3):
    from drn_amd import Grounder
    tok, qlen = sentences(S, 7)
    eager, graphed = Grounder(model, top_k=10), Grounder(model, top_k=10, graph=True)
    variants = {"store_eager": lambda: eager.search(tok, qlen, store, per_video=2),
                "index_eager": lambda: eager.search(tok, qlen, index, per_video=2),
                "store_graph": lambda: graphed.search(tok, qlen, store, per_video=2),
                "index_graph": lambda: graphed.search(tok, qlen, index, per_video=2)}
    hits = {k: fn() for k, fn in variants.items()}
    torch.cuda.synchronize()
    same = {k: all(torch.equal(getattr(hits[k], f), getattr(hits["store_eager"], f)) for f in STATE) for k in variants}
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():                     # interleaved: a drift of the clock or the host hits all variants alike
            times[k].append(window(fn, reps[k]))
    res = {"T": T, "S": S, "videos": len(store), "pairs_per_step": S * len(store), "top_k": 10, "per_video": 2, "rounds": rounds,
           "hits_equal_store_eager": same, "hits_min_n": int(hits["store_eager"].n.min()), "graph_captures": graphed.captures, "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_search_median": statistics.median(ts), "ms_per_search_rounds": ts, "searches_per_window": reps[k]}
    return res


def bench_shortlist(model, where, name, T, S, N, rounds, window_s=0.3):
    """Shortlists of N videos per sentence (drawn without replacement, seed N) beside the cartesian search of all NV videos: the same
    two Grounders (eager, graph) run both, interleaved."""
    import numpy as np
    from drn_amd import Grounder
    tok, qlen = sentences(S, 7)
    g = np.random.RandomState(N)
    lists = [sorted(int(v) for v in g.permutation(NV)[:N]) for _ in range(S)]
    eager, graphed = Grounder(model, top_k=10), Grounder(model, top_k=10, graph=True)
    variants = {"cartesian_eager": lambda: eager.search(tok, qlen, where, per_video=2),
                "shortlist_eager": lambda: eager.search(tok, qlen, where, per_video=2, candidates=lists),
                "cartesian_graph": lambda: graphed.search(tok, qlen, where, per_video=2),
                "shortlist_graph": lambda: graphed.search(tok, qlen, where, per_video=2, candidates=lists)}
    hits = {k: fn() for k, fn in variants.items()}
    torch.cuda.synchronize()
    same = lambda a, b: all(torch.equal(getattr(hits[a], f), getattr(hits[b], f)) for f in STATE)
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]))
    distinct = len(set(v for l in lists for v in l))
    res = {"resident": name, "T": T, "S": S, "videos": NV, "candidates_per_sentence": N, "pairs": S * N, "cartesian_pairs": S * NV,
           "distinct_candidate_videos": distinct, "top_k": 10, "per_video": 2, "rounds": rounds, "graph_captures": graphed.captures,
           "shortlist_graph_equals_eager": same("shortlist_graph", "shortlist_eager"),
           "shortlist_equals_cartesian": same("shortlist_eager", "cartesian_eager") if N == NV else None, "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_search_median": statistics.median(ts), "ms_per_search_min": min(ts), "ms_per_search_max": max(ts),
                              "ms_per_search_rounds": ts, "searches_per_window": reps[k]}
    med = lambda k: res["variants"][k]["ms_per_search_median"]
    res["shortlist_over_cartesian"] = {"eager": med("shortlist_eager") / med("cartesian_eager"),
                                       "graph": med("shortlist_graph") / med("cartesian_graph")}
    return res


def main_shortlist(args):
    from bench_store import build_store
    from drn_amd import SearchIndex
    out = args.out or os.path.join(ROOT, "profiles", "search_pairs_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, store and index resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s; min and max of the rounds beside it",
                      "clock": "host clock around searches ending in a device synchronise",
                      "what": "Grounder.search(candidates=) with N random videos per sentence beside Grounder.search over all videos"},
           "shortlist": []}
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        index = SearchIndex.build(model, store)
        for name, where in (("store", store), ("index", index)):
            for N in (4, 16, NV):
                res["shortlist"].append(bench_shortlist(model, where, name, T, 8, N, args.rounds))
                print(json.dumps({"shortlist": res["shortlist"][-1]}), flush=True)
                json.dump(res, open(out, "w"), indent=1)
        del store, index
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bench_evaluate(model, where, name, T, rounds, S=8, nbatches=8, window_s=0.3):
    """One pass = nbatches batches of S sentences, sentence q of batch b annotated in video (b * S + q) % NV with a random ground truth
    (host tensors, as search_batches yields them; the tokens are resident, as a caller that evaluates repeatedly keeps them).
    device: evaluate_search.  host: per batch search -> Hits.tolist() (a synchronise and six copies) -> metrics.search_first_hits."""
    import numpy as np
    from drn_amd import Grounder, evaluate_search
    from drn_amd.metrics import search_first_hits
    ious, K, kv = (0.5, 0.7), 10, 2
    g = torch.Generator().manual_seed(T)
    batches = []
    for b in range(nbatches):
        tok, qlen = sentences(S, 100 + b)
        start = torch.rand(S, generator=g, dtype=torch.float64) * 0.5
        gt = torch.stack([start, start + 0.1 + torch.rand(S, generator=g, dtype=torch.float64) * 0.4], dim=1)
        batches.append((["V%03d" % ((b * S + q) % NV) for q in range(S)], tok, qlen, gt))
    eager, graphed = Grounder(model, top_k=K), Grounder(model, top_k=K, graph=True)

    def on_host(grounder):
        parts = []
        for names, tok, qlen, gt in batches:
            rows = grounder.search(tok, qlen, where, top_k=K, per_video=kv).tolist()
            parts.append(search_first_hits(rows, [where.index[n] for n in names], gt.tolist(), ious, K))
        return np.concatenate(parts)
    on_device = lambda grounder: evaluate_search(grounder, batches, where, ious=ious, topks=(1, K), per_video=kv).first_hits
    variants = {"device_eager": lambda: on_device(eager), "host_eager": lambda: on_host(eager),
                "device_graph": lambda: on_device(graphed), "host_graph": lambda: on_host(graphed)}
    tables = {k: fn() for k, fn in variants.items()}
    torch.cuda.synchronize()
    reps = {}
    for k, fn in variants.items():
        window(fn, 2)
        reps[k] = max(3, int(window_s * 1e3 / window(fn, 3)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]) / nbatches)
    ref = tables["host_eager"]
    res = {"resident": name, "T": T, "S": S, "batches_per_pass": nbatches, "videos": NV, "pairs_per_step": S * NV, "top_k": K,
           "per_video": kv, "ious": list(ious), "rounds": rounds, "graph_captures": graphed.captures,
           "tables_equal_host_eager": {k: bool((tables[k] == ref).all()) for k in variants},
           "sentences_hit_at_any_depth": int((ref[:, :len(ious)] < K).any(axis=1).sum()),
           "videos_found": int((ref[:, len(ious)] < K).sum()), "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_batch_median": statistics.median(ts), "ms_per_batch_min": min(ts), "ms_per_batch_max": max(ts),
                              "ms_per_batch_rounds": ts, "passes_per_window": reps[k]}
    med = lambda k: res["variants"][k]["ms_per_batch_median"]
    res["device_over_host"] = {"eager": med("device_eager") / med("host_eager"), "graph": med("device_graph") / med("host_graph")}
    return res


def main_evaluate(args):
    from bench_store import build_store
    from drn_amd import SearchIndex
    out = args.out or os.path.join(ROOT, "profiles", "search_eval_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, store and index resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s of whole passes, per batch; "
                                                        "min and max of the rounds beside it",
                      "clock": "host clock around passes that end with the table on the host",
                      "what": "evaluate_search (drn_search_recall per batch, one copy per pass) beside search + Hits.tolist() + "
                              "metrics.search_first_hits per batch; synthetic weights: the recalls mean nothing"},
           "evaluate": []}
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        index = SearchIndex.build(model, store)
        for name, where in (("store", store), ("index", index)):
            res["evaluate"].append(bench_evaluate(model, where, name, T, args.rounds))
            print(json.dumps({"evaluate": res["evaluate"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        del store, index
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bench_build(model, store, rounds):
    from drn_amd import SearchIndex
    index = SearchIndex.build(model, store)
    ts = [window(lambda: SearchIndex.build(model, store), 1) for _ in range(max(rounds, 3))]
    return index, {"ms_per_build_median": statistics.median(ts), "ms_per_build_rounds": ts, "videos": len(store),
                   "proposals": int(store.nprops.sum()), "store_nbytes": store.nbytes, "index_nbytes": index.nbytes,
                   "row_width": index.Dp + index.P}


def bench_kernel(index, T, Q, rounds, window_s=0.3):
    """Launch-inclusive: back-to-back launches issued from Python on one stream, device events around each window.  Two output
    buffers in turn.  What is counted is what the kernel WRITES; it also reads every source row once per pair (mostly from L2 /
    Infinity Cache: 64 videos' rows are 143 MB at T = 256, 18 MB at T = 32)."""
    from drn_amd import ops
    dev = index.rows.device
    S = Q // NV
    gate = torch.randn(S, index.Dp, device=dev)
    pair = torch.arange(Q, dtype=torch.int32, device=dev)
    pq, pv = torch.div(pair, NV, rounding_mode="floor"), torch.remainder(pair, NV)
    vids = torch.arange(NV, dtype=torch.int32, device=dev)
    outs = [torch.empty((Q, T, index.Dp + index.P), dtype=index.dtype, device=dev) for _ in range(2)]

    def run(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            ops.gate_gather_packed(index.rows, index.pad_row, index.prop_off, gate, pq, pv, vids, outs[i & 1], T, index.Dp, index.P, ops.BF16)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    run(10)
    reps = max(20, int(window_s / (run(20) * 1e-6)))
    ts = [run(reps) for _ in range(rounds)]
    written = outs[0].numel() * outs[0].element_size()
    us = statistics.median(ts)
    return {"Q": Q, "T": T, "C": index.Dp, "P": index.P, "dtype": "bf16", "launches_per_window": reps, "bytes_written": written,
            "us_median": us, "us_rounds": ts, "written_bytes_per_s": written / (us * 1e-6),
            "note": "launch-inclusive; written bytes over that time.  At Q = 64, T = 32 the output (18 MB) fits the Infinity Cache: "
                    "that figure is not an HBM rate"}


def bench_q8_search(model, plain, q, ref, T, S, rounds, window_s=0.3):
    """The plain index (the code every search on an index runs without this option) and the quantised one, interleaved."""
    from drn_amd import Grounder
    tok, qlen = sentences(S, 7)
    eager, graphed = Grounder(model, top_k=10), Grounder(model, top_k=10, graph=True)
    variants = {"plain_eager": lambda: eager.search(tok, qlen, plain, per_video=2),
                "q8_eager": lambda: eager.search(tok, qlen, q, per_video=2),
                "plain_graph": lambda: graphed.search(tok, qlen, plain, per_video=2),
                "q8_graph": lambda: graphed.search(tok, qlen, q, per_video=2)}
    hits = {k: fn() for k, fn in variants.items()}
    twin = eager.search(tok, qlen, ref, per_video=2)
    torch.cuda.synchronize()
    same = lambda a, b: all(torch.equal(getattr(a, f), getattr(b, f)) for f in STATE)
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]))
    res = {"T": T, "S": S, "videos": len(plain), "pairs_per_step": S * len(plain), "top_k": 10, "per_video": 2, "rounds": rounds,
           "graph_captures": graphed.captures,
           "q8_hits_equal_dequantized_twin": {"eager": same(hits["q8_eager"], twin), "graph": same(hits["q8_graph"], twin)},
           "q8_hits_equal_plain": same(hits["q8_eager"], hits["plain_eager"]), "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_search_median": statistics.median(ts), "ms_per_search_min": min(ts), "ms_per_search_max": max(ts),
                              "ms_per_search_rounds": ts, "searches_per_window": reps[k]}
    v = res["variants"]
    for mode in ("eager", "graph"):
        diff = v["q8_" + mode]["ms_per_search_median"] - v["plain_" + mode]["ms_per_search_median"]
        spread = v["plain_" + mode]["ms_per_search_max"] - v["plain_" + mode]["ms_per_search_min"]
        res["q8_minus_plain_" + mode] = {"ms": diff, "plain_max_minus_min_ms": spread, "a_difference": abs(diff) > spread}
    return res


def bench_q8_build(model, store, rounds):
    from drn_amd import SearchIndex
    plain, q = SearchIndex.build(model, store), SearchIndex.build(model, store, quantize="mxfp8")
    ts = {"plain": [], "q8": []}
    for _ in range(max(rounds, 3)):
        ts["plain"].append(window(lambda: SearchIndex.build(model, store), 1))
        ts["q8"].append(window(lambda: SearchIndex.build(model, store, quantize="mxfp8"), 1))
    total, width = int(store.nprops.sum()), plain.Dp + plain.P
    item = torch.empty((), dtype=plain.dtype).element_size()
    res = {"videos": len(store), "proposals": total, "store_nbytes": store.nbytes, "Dp": plain.Dp, "P": plain.P,
           "plain_nbytes": plain.nbytes, "q8_nbytes": q.nbytes,
           "plain_bytes_of": SearchIndex.bytes_of(total, width, plain.dtype, len(store)),
           "q8_bytes_of": SearchIndex.bytes_of(total, width, plain.dtype, len(store), quantize="mxfp8", P=plain.P),
           "plain_row_bytes": width * item, "q8_row_bytes": plain.Dp + plain.Dp // 32 + plain.P * item,
           "q8_storage_nbytes": sum(t.untyped_storage().nbytes() for t in (q.codes, q.scales, q.pos, q.prop_off))}
    res["q8_over_plain_bytes"] = res["q8_nbytes"] / res["plain_nbytes"]
    for k in ts:
        res[k + "_ms_per_build_median"], res[k + "_ms_per_build_rounds"] = statistics.median(ts[k]), ts[k]
    return plain, q, res


def bench_q8_kernels(plain, q, T, Q, rounds, window_s=0.3):
    """bench_kernel's protocol for both gather kernels on the same pairs, interleaved round by round."""
    from drn_amd import ops
    dev = plain.rows.device
    S = Q // NV
    gate = torch.randn(S, plain.Dp, device=dev)
    pair = torch.arange(Q, dtype=torch.int32, device=dev)
    pq, pv = torch.div(pair, NV, rounding_mode="floor"), torch.remainder(pair, NV)
    vids = torch.arange(NV, dtype=torch.int32, device=dev)
    outs = [torch.empty((Q, T, plain.Dp + plain.P), dtype=plain.dtype, device=dev) for _ in range(2)]
    launch = {"gate_gather_packed": lambda o: ops.gate_gather_packed(plain.rows, plain.pad_row, plain.prop_off, gate, pq, pv, vids, o, T,
                                                                     plain.Dp, plain.P, ops.BF16),
              "gate_gather_packed_q8": lambda o: ops.gate_gather_packed_q8(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, gate, pq, pv,
                                                                           vids, o, T, q.Dp, q.P, ops.BF16)}

    def run(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(outs[i & 1])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    reps = {}
    for k, fn in launch.items():
        run(fn, 10)
        reps[k] = max(20, int(window_s / (run(fn, 20) * 1e-6)))
    ts = {k: [] for k in launch}
    for _ in range(rounds):
        for k, fn in launch.items():
            ts[k].append(run(fn, reps[k]))
    written = outs[0].numel() * outs[0].element_size()
    res = {"Q": Q, "T": T, "C": plain.Dp, "P": plain.P, "dtype": "bf16", "bytes_written": written,
           "note": "launch-inclusive; both kernels write the same bytes; the quantised one reads 4736 instead of 8704 bytes per source row"}
    for k in launch:
        us = statistics.median(ts[k])
        res[k] = {"us_median": us, "us_min": min(ts[k]), "us_max": max(ts[k]), "us_rounds": ts[k], "launches_per_window": reps[k],
                  "written_bytes_per_s": written / (us * 1e-6)}
    return res


def bench_q8_recall(model, plain, q, T, S=8, nbatches=8):
    """evaluate_search on both indexes over bench_evaluate's batches (random annotations, synthetic weights: the recalls say nothing
    about the model, only how far the two indexes' answers are apart), and the first hits' videos side by side."""
    from drn_amd import Grounder, evaluate_search
    ious, topks, kv = (0.5, 0.7), (1, 10), 2
    g = torch.Generator().manual_seed(T)
    batches = []
    for b in range(nbatches):
        tok, qlen = sentences(S, 100 + b)
        start = torch.rand(S, generator=g, dtype=torch.float64) * 0.5
        gt = torch.stack([start, start + 0.1 + torch.rand(S, generator=g, dtype=torch.float64) * 0.4], dim=1)
        batches.append((["V%03d" % ((b * S + i) % NV) for i in range(S)], tok, qlen, gt))
    grounder = Grounder(model, top_k=10)
    res = {"T": T, "sentences": S * nbatches, "ious": list(ious), "topks": list(topks), "per_video": kv,
           "note": "synthetic weights and random annotations: these recalls say nothing about the model"}
    tables = {}
    for name, where in (("plain", plain), ("q8", q)):
        r = evaluate_search(grounder, batches, where, ious=ious, topks=topks, per_video=kv)
        tables[name] = r.first_hits
        res[name] = {"moment": r.moment, "video": r.video}
    res["first_hit_rows_equal"] = float((tables["plain"] == tables["q8"]).all(axis=1).mean())
    same_video = same_top10 = 0
    for _, tok, qlen, _ in batches:
        a, b = grounder.search(tok, qlen, plain, per_video=kv), grounder.search(tok, qlen, q, per_video=kv)
        same_video += int((a.video[:, 0] == b.video[:, 0]).sum())
        same_top10 += int((a.video == b.video).all(dim=1).sum())
    res["first_hit_same_video_share"] = same_video / (S * nbatches)
    res["top10_same_videos_in_order_share"] = same_top10 / (S * nbatches)
    return res


def main_quantized(args):
    from bench_store import build_store
    out = args.out or os.path.join(ROOT, "profiles", "search_q8_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, both indexes resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s; min and max of the rounds beside it",
                      "clock": "host clock around searches ending in a device synchronise; device events for the kernel windows",
                      "what": "SearchIndex.build(quantize=\"mxfp8\") beside the plain SearchIndex of the same store; a difference smaller "
                              "than the plain index's own max - min across rounds is no difference"},
           "build": [], "search": [], "kernel": [], "recall": []}
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        plain, q, b = bench_q8_build(model, store, args.rounds)
        res["build"].append(dict(b, T=T))
        print(json.dumps({"build": res["build"][-1]}), flush=True)
        ref = q.dequantized()
        for S in (1, 8):
            res["search"].append(bench_q8_search(model, plain, q, ref, T, S, args.rounds))
            print(json.dumps({"search": res["search"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        del ref
        for Q in (512, 64):
            res["kernel"].append(bench_q8_kernels(plain, q, T, Q, args.rounds))
            print(json.dumps({"kernel": res["kernel"][-1]}), flush=True)
        res["recall"].append(bench_q8_recall(model, plain, q, T))
        print(json.dumps({"recall": res["recall"][-1]}), flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del store, plain, q
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bench_mx_search(model, q, T, S, rounds, window_s=0.3):
    """The default path on the quantised index (gather, then conv0 on bf16 MFMAs) and conv0="mxfp8" on the same index, interleaved."""
    from drn_amd import Grounder
    tok, qlen = sentences(S, 7)
    g = {"default_eager": Grounder(model, top_k=10), "mx_eager": Grounder(model, top_k=10, conv0="mxfp8"),
         "default_graph": Grounder(model, top_k=10, graph=True), "mx_graph": Grounder(model, top_k=10, graph=True, conv0="mxfp8")}
    variants = {k: (lambda gr=gr: gr.search(tok, qlen, q, per_video=2)) for k, gr in g.items()}
    hits = {k: fn() for k, fn in variants.items()}
    torch.cuda.synchronize()
    same = lambda a, b: all(torch.equal(getattr(hits[a], f), getattr(hits[b], f)) for f in STATE)
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]))
    res = {"T": T, "S": S, "videos": len(q), "pairs_per_step": S * len(q), "top_k": 10, "per_video": 2, "rounds": rounds,
           "mx_graph_equals_mx_eager": same("mx_graph", "mx_eager"), "mx_hits_equal_default": same("mx_eager", "default_eager"),
           "first_hit_same_video": int((hits["mx_eager"].video[:, 0] == hits["default_eager"].video[:, 0]).sum()), "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_search_median": statistics.median(ts), "ms_per_search_min": min(ts), "ms_per_search_max": max(ts),
                              "ms_per_search_rounds": ts, "searches_per_window": reps[k]}
    v = res["variants"]
    for mode in ("eager", "graph"):
        diff = v["mx_" + mode]["ms_per_search_median"] - v["default_" + mode]["ms_per_search_median"]
        spread = v["default_" + mode]["ms_per_search_max"] - v["default_" + mode]["ms_per_search_min"]
        res["mx_minus_default_" + mode] = {"ms": diff, "default_max_minus_min_ms": spread, "a_difference": abs(diff) > spread}
    return res


def bench_mx_kernels(model, q, T, Q, rounds, window_s=0.3):
    """bench_kernel's protocol, launch-inclusive, interleaved: drn_conv0_mx8 alone; the gather and the conv0 GEMM it replaces, each
    alone and back to back (the GEMM as conv_block launches it, on the gather's output); and the once-per-search weights launch."""
    from drn_amd import functional as DF, ops
    from drn_amd.model.basic_blocks import conv_bn
    dev = q.codes.device
    S = Q // NV
    conv, _ = conv_bn(model.backbone_net.forward_conv0, "bench")
    Cout = int(conv.weight.shape[0])
    gate = torch.randn(S, q.Dp, device=dev)
    pair = torch.arange(Q, dtype=torch.int32, device=dev)
    pq, pv = torch.div(pair, NV, rounding_mode="floor"), torch.remainder(pair, NV)
    vids = torch.arange(NV, dtype=torch.int32, device=dev)
    g0 = torch.empty((Q, T, q.Dp + q.P), dtype=q.dtype, device=dev)
    raws = [torch.empty((Q, T, Cout), dtype=q.dtype, device=dev) for _ in range(2)]
    with torch.no_grad():
        wq = DF.conv0_mx8_weights(conv.weight, gate, q.D, q.Dp)
        wp = DF.packed(conv.weight, (0, 2, 1), ops.BF16)
    gather = lambda o: ops.gate_gather_packed_q8(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, gate, pq, pv, vids, g0, T, q.Dp, q.P, ops.BF16)
    gemm = lambda o: ops.gemm_nt([ops.gemm_desc(g0, wp, o, Q * T, Cout, q.Dp + q.P, taps=3, stride=1, pad=1, Lout=T, Lsrc=T,
                                                lda=q.Dp + q.P)], ops.BF16)
    launch = {"conv0_mx8": lambda o: ops.conv0_mx8(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, wq[0], wq[1], wq[2], pq, pv, vids, o, T,
                                                   q.Dp, q.P),
              "gate_gather_packed_q8": gather, "conv0_gemm_bf16": gemm, "gather_then_gemm": lambda o: (gather(o), gemm(o)),
              "gate_quantize_weights_mx8": lambda o: ops.gate_quantize_weights_mx8(DF.packed(conv.weight, (2, 0, 1), ops.F32)[:, :, :q.D], gate,
                                                                                  q.D, q.Dp, wq[0], wq[1])}

    def run(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(raws[i & 1])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    reps = {}
    with torch.no_grad():
        for k, fn in launch.items():
            run(fn, 5)
            reps[k] = max(10, int(window_s / (run(fn, 10) * 1e-6)))
        ts = {k: [] for k in launch}
        for _ in range(rounds):
            for k, fn in launch.items():
                ts[k].append(run(fn, reps[k]))
    flop = 2.0 * Q * T * Cout * 3 * (q.Dp + q.P)
    res = {"Q": Q, "T": T, "S": S, "C": q.Dp, "P": q.P, "Cout": Cout, "flop": flop, "g0_bytes": g0.numel() * g0.element_size(),
           "gated_weight_bytes": int(wq[0].numel() + wq[1].numel()), "note": "launch-inclusive, device events around windows of ~0.3 s"}
    for k in launch:
        us = statistics.median(ts[k])
        res[k] = {"us_median": us, "us_min": min(ts[k]), "us_max": max(ts[k]), "us_rounds": ts[k], "launches_per_window": reps[k]}
    for k in ("conv0_mx8", "conv0_gemm_bf16"):
        res[k]["tflops"] = flop / (res[k]["us_median"] * 1e-6) / 1e12
    return res


def bench_mx_recall(model, q, T, S=8, nbatches=8):
    """bench_q8_recall's batches through both modes on the same quantised index (random annotations, synthetic weights: the recalls
    say nothing about the model, only how far the two modes' answers are apart)."""
    from drn_amd import Grounder, evaluate_search
    ious, topks, kv = (0.5, 0.7), (1, 10), 2
    g = torch.Generator().manual_seed(T)
    batches = []
    for b in range(nbatches):
        tok, qlen = sentences(S, 100 + b)
        start = torch.rand(S, generator=g, dtype=torch.float64) * 0.5
        gt = torch.stack([start, start + 0.1 + torch.rand(S, generator=g, dtype=torch.float64) * 0.4], dim=1)
        batches.append((["V%03d" % ((b * S + i) % NV) for i in range(S)], tok, qlen, gt))
    grounders = {"default": Grounder(model, top_k=10), "mx": Grounder(model, top_k=10, conv0="mxfp8")}
    res = {"T": T, "sentences": S * nbatches, "ious": list(ious), "topks": list(topks), "per_video": kv,
           "note": "synthetic weights and random annotations: these recalls say nothing about the model"}
    tables = {}
    for name, gr in grounders.items():
        r = evaluate_search(gr, batches, q, ious=ious, topks=topks, per_video=kv)
        tables[name] = r.first_hits
        res[name] = {"moment": r.moment, "video": r.video}
    res["first_hit_rows_equal"] = float((tables["default"] == tables["mx"]).all(axis=1).mean())
    same_video = same_top10 = 0
    worst = 0.0
    for _, tok, qlen, _ in batches:
        a, b = grounders["default"].search(tok, qlen, q, per_video=kv), grounders["mx"].search(tok, qlen, q, per_video=kv)
        same_video += int((a.video[:, 0] == b.video[:, 0]).sum())
        same_top10 += int((a.video == b.video).all(dim=1).sum())
        worst = max(worst, float((a.score[:, 0] - b.score[:, 0]).abs().max()))
    res["first_hit_same_video_share"] = same_video / (S * nbatches)
    res["top10_same_videos_in_order_share"] = same_top10 / (S * nbatches)
    res["first_hit_score_largest_abs_difference"] = worst
    return res


def mx_bound_ratio():
    """The random case of tests/test_search_mx8conv_gpu.py (Dp = 384, P = 256, Cout = 64, L = 40, raw in bf16): the largest
    |raw - ref| over its derived bound 2^-8 |ref| + K 2^-23 sum |a b|."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_search_mx8conv_gpu import random_case, raw_bound, run_conv0
    from drn_amd.index import mx8_conv0_reference
    case = random_case(384, 256, 64, 11)
    raw = run_conv0(*case, 40, torch.bfloat16)
    ref = mx8_conv0_reference(*case, 40)
    return {"Dp": 384, "P": 256, "Cout": 64, "L": 40, "raw": "bf16", "bound": "2^-8 |ref| + 3 (Dp + P) 2^-23 sum |a b|",
            "largest_error_over_bound": float(((raw.double().cpu() - ref).abs() / raw_bound(*case, 40, ref)).max())}


def main_mx_conv0(args):
    from bench_store import build_store
    from drn_amd import SearchIndex
    out = args.out or os.path.join(ROOT, "profiles", "search_mx8conv_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, one quantised index resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s; min and max of the rounds beside it",
                      "clock": "host clock around searches ending in a device synchronise; device events for the kernel windows",
                      "what": "Grounder(conv0=\"mxfp8\") beside the default Grounder on the same SearchIndex(quantize=\"mxfp8\"); a difference "
                              "smaller than the default path's own max - min across rounds is no difference"},
           "bound_ratio": mx_bound_ratio(), "search": [], "kernel": [], "recall": []}
    print(json.dumps({"bound_ratio": res["bound_ratio"]}), flush=True)
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        q = SearchIndex.build(model, store, quantize="mxfp8")
        del store
        for S in (1, 8):
            res["search"].append(bench_mx_search(model, q, T, S, args.rounds))
            print(json.dumps({"search": res["search"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        for Q in (512, 64):
            res["kernel"].append(bench_mx_kernels(model, q, T, Q, args.rounds))
            print(json.dumps({"kernel": res["kernel"][-1]}), flush=True)
        res["recall"].append(bench_mx_recall(model, q, T))
        print(json.dumps({"recall": res["recall"][-1]}), flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del q
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bench_mxf_search(model, q, T, S, rounds, window_s=0.3):
    """conv0="mxfp8" with fused=True (the new launch) beside conv0="mxfp8" unfused and the default fused path, interleaved."""
    from drn_amd import Grounder
    tok, qlen = sentences(S, 7)
    g = {}
    for mode, kw in (("eager", {}), ("graph", {"graph": True})):
        g["default_fused_" + mode] = Grounder(model, top_k=10, fused=True, **kw)
        g["mx_unfused_" + mode] = Grounder(model, top_k=10, conv0="mxfp8", **kw)
        g["mx_fused_" + mode] = Grounder(model, top_k=10, conv0="mxfp8", fused=True, **kw)
    variants = {k: (lambda gr=gr: gr.search(tok, qlen, q, per_video=2)) for k, gr in g.items()}
    hits = {k: fn() for k, fn in variants.items()}
    torch.cuda.synchronize()
    same = lambda a, b: all(torch.equal(getattr(hits[a], f), getattr(hits[b], f)) for f in STATE)
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]))
    res = {"T": T, "S": S, "videos": len(q), "pairs_per_step": S * len(q), "top_k": 10, "per_video": 2, "rounds": rounds,
           "mx_fused_graph_equals_mx_fused_eager": same("mx_fused_graph", "mx_fused_eager"),
           "mx_fused_hits_equal_mx_unfused": same("mx_fused_eager", "mx_unfused_eager"),
           "first_hit_same_video_as_mx_unfused": int((hits["mx_fused_eager"].video[:, 0] == hits["mx_unfused_eager"].video[:, 0]).sum()),
           "first_hit_score_largest_abs_difference_to_mx_unfused":
               float((hits["mx_fused_eager"].score[:, 0] - hits["mx_unfused_eager"].score[:, 0]).abs().max()),
           "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_search_median": statistics.median(ts), "ms_per_search_min": min(ts), "ms_per_search_max": max(ts),
                              "ms_per_search_rounds": ts, "searches_per_window": reps[k]}
    v = res["variants"]
    for mode in ("eager", "graph"):
        for other in ("mx_unfused_", "default_fused_"):
            diff = v["mx_fused_" + mode]["ms_per_search_median"] - v[other + mode]["ms_per_search_median"]
            spread = v[other + mode]["ms_per_search_max"] - v[other + mode]["ms_per_search_min"]
            res["mx_fused_minus_" + other + mode] = {"ms": diff, "other_max_minus_min_ms": spread, "a_difference": abs(diff) > spread}
    return res


def bench_mxf_kernels(model, q, T, Q, rounds, window_s=0.3):
    """bench_kernel's protocol, launch-inclusive, interleaved: drn_conv0_mx8_bn alone and behind bn_eval_scale_shift (what
    functional.conv0_mx8_block launches inside fused_eval()); yardstick (a), the unfused mode's three launches back to back; yardstick
    (b), the default fused path's gather + bn_eval_scale_shift + one-launch conv0 block (ops.conv_bn_eval); drn_conv0_mx8 alone."""
    from drn_amd import functional as DF, ops
    from drn_amd.model.basic_blocks import conv_bn
    dev = q.codes.device
    S = Q // NV
    conv, bn = conv_bn(model.backbone_net.forward_conv0, "bench")
    Cout = int(conv.weight.shape[0])
    gate = torch.randn(S, q.Dp, device=dev)
    pair = torch.arange(Q, dtype=torch.int32, device=dev)
    pq, pv = torch.div(pair, NV, rounding_mode="floor"), torch.remainder(pair, NV)
    vids = torch.arange(NV, dtype=torch.int32, device=dev)
    gate1 = torch.randn(S, Cout, device=dev).index_select(0, pq.long())
    g0 = torch.empty((Q, T, q.Dp + q.P), dtype=q.dtype, device=dev)
    raw = torch.empty((Q, T, Cout), dtype=q.dtype, device=dev)
    outs = [(torch.empty((Q, T, Cout), dtype=q.dtype, device=dev), torch.empty((Q, T, Cout), dtype=q.dtype, device=dev)) for _ in range(2)]
    ss = torch.empty((2, Cout), dtype=torch.float32, device=dev)
    with torch.no_grad():
        wq = DF.conv0_mx8_weights(conv.weight, gate, q.D, q.Dp)
        wp = DF.packed(conv.weight, (0, 2, 1), ops.BF16)
    scale_shift = lambda: ops.bn_eval_scale_shift(Cout, bn.weight, bn.bias, conv.bias, bn.running_mean, bn.running_var, bn.eps, ss)
    level = lambda o: dict(raw=raw, ld_raw=Cout, ss=ss, out=o[0], ld_out=Cout, M=Q * T, L=T, up=None, ld_up=0, gate=gate1, gated=o[1],
                           ld_gated=Cout)
    conv0 = lambda o: ops.conv0_mx8(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, wq[0], wq[1], wq[2], pq, pv, vids, raw, T, q.Dp, q.P)
    fused = lambda o: ops.conv0_mx8_bn(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, wq[0], wq[1], wq[2], pq, pv, vids, ss, gate1, o[0],
                                       o[1], T, q.Dp, q.P)
    gather = lambda o: ops.gate_gather_packed_q8(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, gate, pq, pv, vids, g0, T, q.Dp, q.P, ops.BF16)

    def block(o):
        desc = ops.gemm_desc(g0, wp, raw, Q * T, Cout, q.Dp + q.P, taps=3, stride=1, pad=1, Lout=T, Lsrc=T, lda=q.Dp + q.P)
        if not ops.conv_bn_eval([desc], [level(o)], ops.BF16, True):
            raise SystemExit("bench_search.py: ops.conv_bn_eval does not serve conv0 at these sizes")
    launch = {"conv0_mx8_bn": fused, "scale_shift_then_conv0_mx8_bn": lambda o: (scale_shift(), fused(o)),
              "a_conv0_mx8_scale_shift_bn_apply": lambda o: (conv0(o), scale_shift(), ops.bn_apply_multi([level(o)], Cout, ops.BF16, relu=True)),
              "b_gather_scale_shift_conv_bn_eval": lambda o: (gather(o), scale_shift(), block(o)),
              "conv0_mx8": conv0}

    def run(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(outs[i & 1])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    reps = {}
    with torch.no_grad():
        for k, fn in launch.items():
            run(fn, 5)
            reps[k] = max(10, int(window_s / (run(fn, 10) * 1e-6)))
        ts = {k: [] for k in launch}
        for _ in range(rounds):
            for k, fn in launch.items():
                ts[k].append(run(fn, reps[k]))
    flop = 2.0 * Q * T * Cout * 3 * (q.Dp + q.P)
    res = {"Q": Q, "T": T, "S": S, "C": q.Dp, "P": q.P, "Cout": Cout, "flop": flop,
           "note": "launch-inclusive, device events around windows of ~0.3 s; out and gated in bf16, a gate row per pair"}
    for k in launch:
        us = statistics.median(ts[k])
        res[k] = {"us_median": us, "us_min": min(ts[k]), "us_max": max(ts[k]), "us_rounds": ts[k], "launches_per_window": reps[k]}
    for k in ("conv0_mx8_bn", "conv0_mx8"):
        res[k]["tflops"] = flop / (res[k]["us_median"] * 1e-6) / 1e12
    a, b, new = res["a_conv0_mx8_scale_shift_bn_apply"], res["b_gather_scale_shift_conv_bn_eval"], res["scale_shift_then_conv0_mx8_bn"]
    res["new_minus_a_us"] = new["us_median"] - a["us_median"]
    res["a_max_minus_min_us"] = a["us_max"] - a["us_min"]
    res["faster_than_a_by_more_than_its_spread"] = a["us_median"] - new["us_median"] > res["a_max_minus_min_us"]
    res["new_minus_b_us"] = new["us_median"] - b["us_median"]
    res["faster_than_b_by_more_than_its_spread"] = b["us_median"] - new["us_median"] > b["us_max"] - b["us_min"]
    return res


def bench_mxf_agreement(model, q, T, S=8, nbatches=8):
    """bench_mx_recall's sentences through the fused and the unfused conv0="mxfp8" mode: how far the two modes' answers are apart."""
    from drn_amd import Grounder
    fused, unfused = Grounder(model, top_k=10, conv0="mxfp8", fused=True), Grounder(model, top_k=10, conv0="mxfp8")
    same_video = same_top10 = 0
    worst = 0.0
    for b in range(nbatches):
        tok, qlen = sentences(S, 100 + b)
        x, y = fused.search(tok, qlen, q, per_video=2), unfused.search(tok, qlen, q, per_video=2)
        same_video += int((x.video[:, 0] == y.video[:, 0]).sum())
        same_top10 += int((x.video == y.video).all(dim=1).sum())
        worst = max(worst, float((x.score[:, 0] - y.score[:, 0]).abs().max()))
    return {"T": T, "sentences": S * nbatches, "per_video": 2, "first_hit_same_video_share": same_video / (S * nbatches),
            "top10_same_videos_in_order_share": same_top10 / (S * nbatches), "first_hit_score_largest_abs_difference": worst,
            "note": "synthetic weights: this says how far the two modes are apart, nothing about recall on a trained checkpoint"}


def mxf_tolerance_ratio():
    """The random case of tests/test_search_mx8fused_gpu.py (Dp = 384, P = 256, Cout = 64, L = 40, bf16, scale / shift of mixed signs,
    a gate per pair): the largest |out - want| and |gated - want gate| over their derived tolerances."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_search_mx8conv_gpu import raw_bound
    from test_search_mx8fused_gpu import epilogue_case, run_bn
    from drn_amd.index import mx8_conv0_reference
    case, ss, gate = epilogue_case()
    out, gated, _ = run_bn(case, 40, torch.bfloat16, ss=ss, gate=gate)
    ref = mx8_conv0_reference(*case, 40)
    mag = raw_bound(*case, 40, ref) - 2.0 ** -8 * ref.abs()
    scale, shift = ss[0].double().cpu(), ss[1].double().cpu()
    want = torch.relu(ref * scale + shift)
    tol = scale.abs() * mag + 2.0 ** -8 * want.abs() + 2.0 ** -20 * ((ref * scale).abs() + shift.abs())
    g1 = gate.double().cpu()[:, None, :]
    tol_g = g1.abs() * tol * (1 + 2.0 ** -7) + 2.0 ** -8 * (want * g1).abs()
    return {"Dp": 384, "P": 256, "Cout": 64, "L": 40, "out": "bf16",
            "tolerance": "|scale| 3 (Dp + P) 2^-23 sum |a b| + 2^-8 |want| + 2^-20 (|ref scale| + |shift|)",
            "largest_error_over_tolerance_out": float(((out.double().cpu() - want).abs() / tol.clamp_min(1e-30)).max()),
            "largest_error_over_tolerance_gated": float(((gated.double().cpu() - want * g1).abs() / tol_g.clamp_min(1e-30)).max())}


def main_mx_conv0_fused(args):
    from bench_store import build_store
    from drn_amd import SearchIndex
    out = args.out or os.path.join(ROOT, "profiles", "search_mx8conv_fused_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, one quantised index resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s; min and max of the rounds beside it",
                      "clock": "host clock around searches ending in a device synchronise; device events for the kernel windows",
                      "what": "Grounder(conv0=\"mxfp8\", fused=True) beside Grounder(conv0=\"mxfp8\") and Grounder(fused=True) on the same "
                              "SearchIndex(quantize=\"mxfp8\"); a difference smaller than the other path's own max - min across rounds is "
                              "no difference"},
           "tolerance_ratio": mxf_tolerance_ratio(), "search": [], "kernel": [], "agreement": []}
    print(json.dumps({"tolerance_ratio": res["tolerance_ratio"]}), flush=True)
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        q = SearchIndex.build(model, store, quantize="mxfp8")
        del store
        for Q in (512, 64):
            res["kernel"].append(bench_mxf_kernels(model, q, T, Q, args.rounds))
            print(json.dumps({"kernel": res["kernel"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        for S in (1, 8):
            res["search"].append(bench_mxf_search(model, q, T, S, args.rounds))
            print(json.dumps({"search": res["search"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        res["agreement"].append(bench_mxf_agreement(model, q, T))
        print(json.dumps({"agreement": res["agreement"][-1]}), flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del q
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bench_mxt_kernels(model, q, T, S, pq, pv, vids, what, rounds, window_s=0.3):
    """bench_mxf_kernels' protocol on one list of pairs: bn_eval_scale_shift + drn_conv0_mx8_bn_tile on every shipped tile forced, on
    "auto", on the wide tile through drn_conv0_mx8_bn itself (the kernel before the narrow tiles, in the same process), and the default
    fused path's gather + bn_eval_scale_shift + one-launch conv0 block."""
    from drn_amd import functional as DF, ops
    from drn_amd.model.basic_blocks import conv_bn
    dev = q.codes.device
    Q = int(pq.numel())
    conv, bn = conv_bn(model.backbone_net.forward_conv0, "bench")
    Cout = int(conv.weight.shape[0])
    gate = torch.randn(S, q.Dp, device=dev)
    gate1 = torch.randn(S, Cout, device=dev).index_select(0, pq.long())
    g0 = torch.empty((Q, T, q.Dp + q.P), dtype=q.dtype, device=dev)
    raw = torch.empty((Q, T, Cout), dtype=q.dtype, device=dev)
    outs = [(torch.empty((Q, T, Cout), dtype=q.dtype, device=dev), torch.empty((Q, T, Cout), dtype=q.dtype, device=dev)) for _ in range(2)]
    ss = torch.empty((2, Cout), dtype=torch.float32, device=dev)
    with torch.no_grad():
        wq = DF.conv0_mx8_weights(conv.weight, gate, q.D, q.Dp)
        wp = DF.packed(conv.weight, (0, 2, 1), ops.BF16)
    scale_shift = lambda: ops.bn_eval_scale_shift(Cout, bn.weight, bn.bias, conv.bias, bn.running_mean, bn.running_var, bn.eps, ss)
    level = lambda o: dict(raw=raw, ld_raw=Cout, ss=ss, out=o[0], ld_out=Cout, M=Q * T, L=T, up=None, ld_up=0, gate=gate1, gated=o[1],
                           ld_gated=Cout)
    fused = lambda o, tile: ops.conv0_mx8_bn(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, wq[0], wq[1], wq[2], pq, pv, vids, ss, gate1,
                                             o[0], o[1], T, q.Dp, q.P, tile=tile)
    gather = lambda o: ops.gate_gather_packed_q8(q.codes, q.scales, q.pos, q.pad_row, q.prop_off, gate, pq, pv, vids, g0, T, q.Dp, q.P, ops.BF16)

    def block(o):
        desc = ops.gemm_desc(g0, wp, raw, Q * T, Cout, q.Dp + q.P, taps=3, stride=1, pad=1, Lout=T, Lsrc=T, lda=q.Dp + q.P)
        if not ops.conv_bn_eval([desc], [level(o)], ops.BF16, True):
            raise SystemExit("bench_search.py: ops.conv_bn_eval does not serve conv0 at these sizes")
    launch = {"wide": lambda o: (scale_shift(), fused(o, None)), "auto": lambda o: (scale_shift(), fused(o, "auto"))}
    for tile in ops.CONV0_MX8_TILES[1:]:
        launch["tile_%dx%d" % tile] = lambda o, tile=tile: (scale_shift(), fused(o, tile))
    launch["default_gather_scale_shift_conv_bn_eval"] = lambda o: (gather(o), scale_shift(), block(o))

    def run(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(outs[i & 1])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    reps, bits = {}, {}
    with torch.no_grad():
        for k, fn in launch.items():
            run(fn, 5)
            reps[k] = max(10, int(window_s / (run(fn, 10) * 1e-6)))
            fn(outs[0])
            bits[k] = (outs[0][0].clone(), outs[0][1].clone())
        ts = {k: [] for k in launch}
        for _ in range(rounds):
            for k, fn in launch.items():
                ts[k].append(run(fn, reps[k]))
    res = {"what": what, "Q": Q, "T": T, "S": S, "C": q.Dp, "P": q.P, "Cout": Cout, "auto_tile": list(ops.conv0_mx8_bn_tile(Q, T, Cout)),
           "wide_workgroups": -(-Q * T // 256) * -(-Cout // 256),
           "note": "launch-inclusive, device events around windows of ~0.3 s, each launch behind bn_eval_scale_shift; out and gated in bf16"}
    for k in launch:
        res[k] = {"us_median": statistics.median(ts[k]), "us_min": min(ts[k]), "us_max": max(ts[k]), "us_rounds": ts[k],
                  "launches_per_window": reps[k]}
        if k != "default_gather_scale_shift_conv_bn_eval":
            res[k]["bits_equal_wide"] = bool(torch.equal(bits[k][0], bits["wide"][0]) and torch.equal(bits[k][1], bits["wide"][1]))
    wide = res["wide"]
    spread = wide["us_max"] - wide["us_min"]
    res["wide_max_minus_min_us"] = spread
    for k in launch:
        if k not in ("wide", "default_gather_scale_shift_conv_bn_eval"):
            res[k]["faster_than_wide_by_more_than_its_spread"] = wide["us_median"] - res[k]["us_median"] > spread
            res[k]["slower_than_wide_by_more_than_its_spread"] = res[k]["us_median"] - wide["us_median"] > spread
    res["auto_minus_default_us"] = res["auto"]["us_median"] - res["default_gather_scale_shift_conv_bn_eval"]["us_median"]
    return res


def bench_mxt_search(model, q, T, S, rounds, window_s=0.3):
    """Searches by graph replay: conv0="mxfp8", fused=True with the chooser as shipped, the same with the chooser held to the wide tile
    (captured while ops.conv0_mx8_bn_tile is replaced), and the default fused path."""
    from drn_amd import Grounder, ops
    tok, qlen = sentences(S, 7)
    g = {"default_fused_graph": Grounder(model, top_k=10, fused=True, graph=True),
         "mx_fused_auto_graph": Grounder(model, top_k=10, conv0="mxfp8", fused=True, graph=True),
         "mx_fused_wide_graph": Grounder(model, top_k=10, conv0="mxfp8", fused=True, graph=True)}
    variants = {k: (lambda gr=gr: gr.search(tok, qlen, q, per_video=2)) for k, gr in g.items()}
    chooser, tiles = ops.conv0_mx8_bn_tile, []
    ops.conv0_mx8_bn_tile = lambda Q, L, Cout: tiles.append(chooser(Q, L, Cout)) or ops.CONV0_MX8_WIDE
    try:
        hits = {"mx_fused_wide_graph": variants["mx_fused_wide_graph"]()}                    # (the capture: the tile is part of it)
    finally:
        ops.conv0_mx8_bn_tile = chooser
    for k in ("default_fused_graph", "mx_fused_auto_graph"):
        hits[k] = variants[k]()
    torch.cuda.synchronize()
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]))
    res = {"T": T, "S": S, "videos": len(q), "pairs_per_step": S * len(q), "top_k": 10, "per_video": 2, "rounds": rounds,
           "auto_tiles": sorted(set(map(tuple, tiles))),
           "auto_hits_equal_wide_hits": all(torch.equal(getattr(hits["mx_fused_auto_graph"], f), getattr(hits["mx_fused_wide_graph"], f))
                                            for f in STATE),
           "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"ms_per_search_median": statistics.median(ts), "ms_per_search_min": min(ts), "ms_per_search_max": max(ts),
                              "ms_per_search_rounds": ts, "searches_per_window": reps[k]}
    v = res["variants"]
    for other in ("mx_fused_wide_graph", "default_fused_graph"):
        diff = v["mx_fused_auto_graph"]["ms_per_search_median"] - v[other]["ms_per_search_median"]
        spread = v[other]["ms_per_search_max"] - v[other]["ms_per_search_min"]
        res["auto_minus_" + other] = {"ms": diff, "other_max_minus_min_ms": spread, "a_difference": abs(diff) > spread}
    return res


CROSSOVER_PAIRS = {256: (80, 96, 112, 128, 129, 160, 192, 255), 32: (128, 256, 384, 392, 448)}


def main_mx_conv0_tiles(args):
    from bench_store import build_store
    from drn_amd import SearchIndex, ops
    from drn_amd.grounding import plan_pairs
    out = args.out or os.path.join(ROOT, "profiles", "search_mx8conv_tiles_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "measured_on": "MI355X, one process, one quantised index resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s; min and max of the rounds beside it",
                      "clock": "host clock around searches ending in a device synchronise; device events for the kernel windows",
                      "what": "drn_conv0_mx8_bn_tile on every shipped tile, on the chosen one and on the wide tile, beside the default fused "
                              "path, on the same SearchIndex(quantize=\"mxfp8\"); a difference smaller than the wide tile's own max - min "
                              "across rounds is no difference"},
           "tiles": [list(t) for t in ops.CONV0_MX8_TILES],
           "rule": {"W": "cdiv(Q L, 256) x cdiv(Cout, 256), the wide tile's workgroups",
                    "64x64": "16 W <= %d x compute units" % ops.CONV0_MX8_SMALL_UPTO_16THS,
                    "128x64": "else 16 W <= %d x compute units" % ops.CONV0_MX8_MID_UPTO_16THS, "wide": "above"},
           "kernel": [], "search": []}
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, dev)
        q = SearchIndex.build(model, store, quantize="mxfp8")
        del store
        vids = torch.arange(NV, dtype=torch.int32, device=dev)
        # the four grids of the README, then the grids between them that the rule's two crossovers are read from: W = 80 ... 255 wide
        # workgroups (T = 256: one per pair) on either side of 128 x 64 | wide, W = 16 ... 56 (T = 32: one per 8 pairs) of 64 x 64 | 128 x 64
        for Q, what in [(512, "cartesian"), (64, "cartesian")] + [(Q, "cartesian, crossover") for Q in CROSSOVER_PAIRS[T]]:
            pair = torch.arange(Q, dtype=torch.int32, device=dev)
            pq, pv = torch.div(pair, NV, rounding_mode="floor"), torch.remainder(pair, NV)
            res["kernel"].append(bench_mxt_kernels(model, q, T, -(-Q // NV), pq, pv, vids, what, args.rounds))
            print(json.dumps({"kernel": res["kernel"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        if T == 32:
            # a shortlist step: 8 sentences x 4 candidates each, one chunk of 32 pairs as plan_pairs emits it (sorted by sentence: a
            # 256-row tile holds two sentences), and the same pairs shuffled (up to eight sentences in a 256-row tile, two in a 64-row one)
            gen = torch.Generator().manual_seed(3)
            lists = [torch.randperm(NV, generator=gen)[:4].tolist() for _ in range(8)]
            plan = plan_pairs(lists, NV, 32, 32, 4)
            assert plan.pair_q.shape[0] == 1
            pq, pv = torch.from_numpy(plan.pair_q[0]).to(dev), torch.from_numpy(plan.pair_v[0]).to(dev)
            pvids = torch.from_numpy(plan.vids[0]).to(dev)
            perm = torch.randperm(32, generator=gen).to(dev)
            for what, a, b in (("shortlist 8 x 4, as planned", pq, pv), ("shortlist 8 x 4, shuffled", pq[perm].contiguous(), pv[perm].contiguous())):
                res["kernel"].append(bench_mxt_kernels(model, q, T, 8, a, b, pvids, what, args.rounds))
                print(json.dumps({"kernel": res["kernel"][-1]}), flush=True)
                json.dump(res, open(out, "w"), indent=1)
        for S in (1, 8):
            res["search"].append(bench_mxt_search(model, q, T, S, args.rounds))
            print(json.dumps({"search": res["search"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
        del q
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


HBM_PEAK_BYTES_PER_S, HBM_COPY_BYTES_PER_S = 8.0e12, 6.29e12          # MI355X: the spec and what a float4 copy reaches


def event_window(launch, rounds, window_s=0.2):
    """Launch-inclusive us per call: back-to-back calls issued from Python on one stream, device events around each window."""
    def run(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    run(5)
    reps = max(10, min(2000, int(window_s / (run(10) * 1e-6))))
    return [run(reps) for _ in range(rounds)], reps


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "rounds": ts}


def verdict(new, base):
    """new against base, both lists of rounds: a difference inside the baseline's own max - min is NO DIFFERENCE."""
    d = statistics.median(new) - statistics.median(base)
    if abs(d) <= max(base) - min(base):
        return "NO DIFFERENCE"
    return "SLOWER" if d > 0 else "faster"


def bench_two_stage(model, where, name, T, S, N, rounds, window_s=0.2):
    """(a): shortlist + search with the ids as a device tensor beside the same shortlist read back and passed as host lists."""
    from drn_amd import Grounder, Shortlister
    tok, qlen = sentences(S, 7)
    g = torch.Generator().manual_seed(N)
    sl = Shortlister(torch.randn(NV, 512, generator=g).to("cuda:0", torch.bfloat16).contiguous(), names=where.names)
    qe = torch.randn(S, 512, generator=g).to("cuda:0", torch.bfloat16).contiguous()
    gr = {k: Grounder(model, top_k=10, graph=k.endswith("graph")) for k in ("host_eager", "device_eager", "host_graph", "device_graph")}

    def host(grounder):
        short = sl.shortlist(qe, N)
        lists = [row[:k] for row, k in zip(short.ids.tolist(), short.n.tolist())]          # (the read-back: the search's only synchronise)
        return grounder.search(tok, qlen, where, per_video=2, candidates=lists)

    def device(grounder):
        return grounder.search(tok, qlen, where, per_video=2, candidates=sl.shortlist(qe, N).ids)
    variants = {k: (lambda k=k: (host if k.startswith("host") else device)(gr[k])) for k in gr}
    hits = {k: fn() for k, fn in variants.items()}
    torch.cuda.synchronize()
    same = lambda a, b: all(torch.equal(getattr(hits[a], f), getattr(hits[b], f)) for f in STATE)
    reps = {}
    for k, fn in variants.items():
        window(fn, 3)
        reps[k] = max(5, int(window_s * 1e3 / window(fn, 5)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, reps[k]))
    res = {"resident": name, "T": T, "index_T": int(where.T), "S": S, "videos": NV, "candidates_per_sentence": N, "pairs": S * N,
           "top_k": 10, "per_video": 2, "rounds": rounds, "graph_captures": {k: gr[k].captures for k in gr if k.endswith("graph")},
           "device_equals_host": {"eager": same("device_eager", "host_eager"), "graph": same("device_graph", "host_graph")},
           "variants": {k: dict(spread(ts), unit="ms per shortlist + search", searches_per_window=reps[k]) for k, ts in times.items()}}
    res["device_against_host"] = {m: {"ratio_of_medians": statistics.median(times["device_" + m]) / statistics.median(times["host_" + m]),
                                      "verdict": verdict(times["device_" + m], times["host_" + m])} for m in ("eager", "graph")}
    return res


def bench_shortlist_launch(V, S, n, rounds):
    """(b): drn_shortlist_topn alone beside torch.matmul + torch.topk on the same tensors (bf16 scores there, fp32 here) and beside the
    time to read the table once."""
    from drn_amd import Shortlist, Shortlister
    g = torch.Generator(device="cuda:0").manual_seed(V + S)
    emb = torch.randn(V, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    sl = Shortlister(emb)
    out = Shortlist(*sl.shortlist(q, n))
    k = min(n, V)
    ours, reps = event_window(lambda: sl.shortlist(q, n, out=out), rounds)
    theirs, _ = event_window(lambda: torch.topk(torch.matmul(q, emb.t()), k, dim=1), rounds)
    table = emb.numel() * emb.element_size()
    tiles, blocks, m = -(-S // 16), -(-V // 256), min(n, 256)
    res = {"V": V, "E": 512, "S": S, "n": n, "dtype": "bf16", "launches_per_window": reps, "table_bytes": table,
           "table_reads": tiles, "workspace_bytes_written_and_read": S * blocks * m * 8,
           "shortlist_us": spread(ours), "matmul_topk_us": spread(theirs),
           "table_once_us_at_8.0TB/s": table / HBM_PEAK_BYTES_PER_S * 1e6, "table_once_us_at_6.29TB/s": table / HBM_COPY_BYTES_PER_S * 1e6,
           "shortlist_over_matmul_topk": statistics.median(ours) / statistics.median(theirs),
           "shortlist_against_matmul_topk": verdict(ours, theirs),
           "shortlist_over_table_floor_6.29TB/s": statistics.median(ours) / (tiles * table / HBM_COPY_BYTES_PER_S * 1e6),
           "note": "launch-inclusive, both launches of the shortlist; the floor counts the table once per 16 sentences and nothing else"
                   + ("; 64 KB: the table lives in cache, the floor is not an HBM time" if V <= 64 else "")}
    del sl, emb
    return res


def bench_plan_launch(S, N, rounds):
    """(c): drn_plan_candidates alone."""
    from drn_amd import ops, plan_candidate_steps
    C = torch.randint(-2, NV, (S, N), dtype=torch.int32, device="cuda:0")
    plan = plan_candidate_steps(S, N, None, 1019)                      # cap of top_k = 10, per_video = 2
    steps = plan.pair_q.shape[0]
    table = torch.empty((steps, plan.pairs), dtype=torch.int32, device="cuda:0")
    ts, reps = event_window(lambda: ops.plan_candidates(C, NV, plan.Sc, plan.Nc, plan.pairs, steps, table), rounds)
    return {"S": S, "N": N, "pairs": plan.pairs, "steps": steps, "launches_per_window": reps, "plan_us": spread(ts)}


def shortlist_tolerance_ratio():
    """tests/test_shortlist_gpu.py's random case (E = 512, V = 300, S = 5, n = 16, bf16): the largest |returned score - float64 score|
    over tol = E * 2^-23 * sum |q * emb|."""
    from drn_amd import Shortlister
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(300, 512, generator=g).to("cuda:0", torch.bfloat16).contiguous()
    q = torch.randn(5, 512, generator=g).to("cuda:0", torch.bfloat16).contiguous()
    got = Shortlister(emb).shortlist(q, 16)
    ref = q.double() @ emb.double().t()
    tol = 512 * 2.0 ** -23 * (q.double().abs() @ emb.double().abs().t())
    ids = got.ids.long()
    return float(((got.scores.double() - torch.gather(ref, 1, ids)).abs() / torch.gather(tol, 1, ids)).max())


def main_device_candidates(args):
    from bench_store import build_store
    from drn_amd import SearchIndex
    out = args.out or os.path.join(ROOT, "profiles", "search_device_candidates_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, indexes resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "host clock around shortlist + search ending in a device synchronise; device events for the launch windows",
                      "baseline": "the same shortlist read back with .tolist() and passed as host lists: the only way before device "
                                  "candidates existed.  A difference inside the baseline's own max - min is NO DIFFERENCE",
                      "what_this_does_not_say": "synthetic weights and random embeddings: nothing here says anything about recall"},
           "tolerance_ratio": shortlist_tolerance_ratio(), "two_stage": [], "shortlist_launch": [], "plan_launch": []}
    for V in (NV, 65536):
        for S in (1, 8, 64):
            for n in (16, 128):
                res["shortlist_launch"].append(bench_shortlist_launch(V, S, n, args.rounds))
                print(json.dumps({"shortlist_launch": res["shortlist_launch"][-1]}), flush=True)
    torch.cuda.empty_cache()
    for S, N in ((8, 4), (8, 64)):
        res["plan_launch"].append(bench_plan_launch(S, N, args.rounds))
        print(json.dumps({"plan_launch": res["plan_launch"][-1]}), flush=True)
    json.dump(res, open(out, "w"), indent=1)
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        for name, kw in (("index", {}), ("index_mxfp8", {"quantize": "mxfp8"})):
            index = SearchIndex.build(model, store, **kw)
            for N in (4, 16):
                res["two_stage"].append(bench_two_stage(model, index, name, T, 8, N, args.rounds))
                print(json.dumps({"two_stage": res["two_stage"][-1]}), flush=True)
                json.dump(res, open(out, "w"), indent=1)
            del index
        del store
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


SEGMENT_LAYOUTS = (("65536x1", [1] * 65536), ("4096x16", [16] * 4096), ("546x120", [120] * 545 + [136]))     # R = 65,536 each: the
# bench store's 546 videos of 120 rows come to 65,520, so its last video takes the 16 rows that remain


def interleaved_windows(variants, rounds, window_s=0.2):
    """{name: launch} -> ({name: [us per call, one per round]}, {name: calls per window}): launch-inclusive, device events around windows
    of back-to-back calls, the variants taking turns inside every round."""
    def run(launch, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    reps = {}
    for k, launch in variants.items():
        run(launch, 5)
        reps[k] = max(10, min(2000, int(window_s / (run(launch, 10) * 1e-6))))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, launch in variants.items():
            times[k].append(run(launch, reps[k]))
    return times, reps


def bench_segment_shortlist(name, lens, emb, S, n, rounds):
    """drn_shortlist_segments_topn on R = 65,536 rows cut into videos by `lens`, beside (a) the plain kernel of the parent on the same R
    rows as R videos and (b) what a caller can do without the feature: torch.matmul, a segmented amax, torch.topk."""
    import numpy as np
    from drn_amd import SegmentShortlist, Shortlist, Shortlister
    R, V = int(emb.shape[0]), len(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    assert off[-1] == R
    g = torch.Generator(device="cuda:0").manual_seed(S + n)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    seg, plain = Shortlister(emb, offsets=off), Shortlister(emb)
    out_seg, out_plain = SegmentShortlist(*seg.shortlist(q, n)), Shortlist(*plain.shortlist(q, n))
    index = torch.repeat_interleave(torch.arange(V, device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(S, R).contiguous()
    best = torch.empty((S, V), dtype=torch.bfloat16, device="cuda:0")

    def torch_way():
        best.fill_(float("-inf"))
        best.scatter_reduce_(1, index, torch.matmul(q, emb.t()), "amax")
        return torch.topk(best, min(n, V), dim=1)
    times, reps = interleaved_windows({"segments": lambda: seg.shortlist(q, n, out=out_seg), "plain_rows": lambda: plain.shortlist(q, n, out=out_plain),
                                       "torch": torch_way}, rounds)
    table, tiles = emb.numel() * emb.element_size(), -(-S // 16)
    med = {k: statistics.median(ts) for k, ts in times.items()}
    return {"layout": name, "R": R, "V": V, "E": 512, "S": S, "n": n, "dtype": "bf16", "blocks": int(seg.plan.blk_vid.shape[0]) - 1,
            "launches_per_window": reps, "table_bytes": table, "table_reads": tiles,
            "segments_us": spread(times["segments"]), "plain_rows_us": spread(times["plain_rows"]), "matmul_amax_topk_us": spread(times["torch"]),
            "read_floor_us_at_6.29TB/s": tiles * table / HBM_COPY_BYTES_PER_S * 1e6, "table_once_us_at_8.0TB/s": table / HBM_PEAK_BYTES_PER_S * 1e6,
            "segments_over_plain_rows": med["segments"] / med["plain_rows"], "segments_against_plain_rows": verdict(times["segments"], times["plain_rows"]),
            "segments_over_matmul_amax_topk": med["segments"] / med["torch"], "segments_against_matmul_amax_topk": verdict(times["segments"], times["torch"]),
            "segments_over_read_floor": med["segments"] / (tiles * table / HBM_COPY_BYTES_PER_S * 1e6),
            "note": "launch-inclusive, all three launches of the segmented shortlist; plain_rows ranks the same R rows as R videos (another "
                    "answer: rows, not videos); torch scores in bf16, here fp32; the floor counts the table once per 16 sentences and nothing else"}


def segment_tolerance_ratio():
    """tests/test_segment_shortlist_gpu.py's random case (E = 512, run lengths 1, 3, 0, 17 twenty times, then 300 and 2; S = 5, n = 16,
    bf16): the largest |returned score - the video's float64 maximum| over tol = the largest E * 2^-23 * sum |q * emb_r| of its rows."""
    import numpy as np
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(sum(lens), 512, generator=g).to("cuda:0", torch.bfloat16).contiguous()
    q = torch.randn(17, 512, generator=g).to("cuda:0", torch.bfloat16)[:5].contiguous()
    got = Shortlister(emb, offsets=np.concatenate([[0], np.cumsum(lens)])).shortlist(q, 16)
    video = torch.repeat_interleave(torch.arange(len(lens), device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(5, -1)
    ref = torch.full((5, len(lens)), float("-inf"), dtype=torch.float64, device="cuda:0").scatter_reduce(1, video, q.double() @ emb.double().t(), "amax")
    tol = torch.zeros_like(ref).scatter_reduce(1, video, 512 * 2.0 ** -23 * (q.double().abs() @ emb.double().abs().t()), "amax")
    ids = got.ids.long()
    return float(((got.scores.double() - torch.gather(ref, 1, ids)).abs() / torch.gather(tol, 1, ids)).max())


def main_segment_shortlist(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_segment_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the table resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baselines": "plain_rows: the parent's drn_shortlist_topn on the same R rows, in the same process, its code unchanged; "
                                   "matmul_amax_topk: torch.matmul, scatter_reduce_(amax) over the videos' rows, torch.topk.  A difference "
                                   "inside the baseline's own max - min is NO DIFFERENCE",
                      "condition": "derived, not measured: at the same R the 16-row and 120-row layouts score the same rows with the same MFMAs "
                                   "and sort fewer keys than the 1-row layout, so neither may take longer than it by more than ITS max - min",
                      "what_this_does_not_say": "random embeddings: nothing here says anything about recall"},
           "tolerance_ratio": segment_tolerance_ratio(), "segment_shortlist": [], "condition": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for S in (1, 8, 64):
        for n in (16, 128):
            rows = {}
            for name, lens in SEGMENT_LAYOUTS:
                rows[name] = bench_segment_shortlist(name, lens, emb, S, n, args.rounds)
                res["segment_shortlist"].append(rows[name])
                print(json.dumps({"segment_shortlist": rows[name]}), flush=True)
            base = rows["65536x1"]["segments_us"]
            for name in ("4096x16", "546x120"):
                over = rows[name]["segments_us"]["median"] - base["median"]
                res["condition"].append({"S": S, "n": n, "layout": name, "median_minus_1row_median_us": over,
                                         "1row_max_minus_min_us": base["max"] - base["min"], "holds": over <= base["max"] - base["min"]})
                print(json.dumps({"condition": res["condition"][-1]}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bench_q8_shortlist(name, lens, emb, S, n, rounds):
    """Shortlister(quantize="mxfp8") on R = 65,536 rows (one row per video: the plain entry; otherwise the segmented one) beside the
    plain table over the SAME dequantised rows, in one process, and the agreement of its lists with those of the ORIGINAL table."""
    import numpy as np
    from drn_amd import Shortlister
    R, V = int(emb.shape[0]), len(lens)
    off = None if V == R else np.concatenate([[0], np.cumsum(lens)])
    g = torch.Generator(device="cuda:0").manual_seed(S + n)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    quant = Shortlister(emb, offsets=off, quantize="mxfp8")
    plain = quant.dequantized()
    assert quant.nbytes == Shortlister.bytes_of(R, 512, torch.bfloat16, "mxfp8") and plain.nbytes == Shortlister.bytes_of(R, 512, torch.bfloat16)
    out_q, out_p = quant.shortlist(q, n), plain.shortlist(q, n)
    times, reps = interleaved_windows({"quantized": lambda: quant.shortlist(q, n, out=out_q), "plain": lambda: plain.shortlist(q, n, out=out_p)},
                                      rounds)
    same = all(torch.equal(a, b) for a, b in zip(out_q, out_p))
    orig = Shortlister(emb, offsets=off).shortlist(q, n)
    first = float((orig.ids[:, 0] == out_q.ids[:, 0]).double().mean())
    lists = float((orig.ids == out_q.ids).all(dim=1).double().mean())
    common = float((orig.ids[:, :, None] == out_q.ids[:, None, :]).any(dim=2).double().mean())      # (every list here is full: n <= V)
    tiles = -(-S // 16)
    med = {k: statistics.median(ts) for k, ts in times.items()}
    return {"layout": name, "entry": "drn_shortlist_topn_q8" if off is None else "drn_shortlist_segments_topn_q8", "R": R, "V": V, "E": 512,
            "S": S, "n": n, "dtype": "bf16", "launches_per_window": reps, "quantized_table_bytes": quant.nbytes, "plain_table_bytes": plain.nbytes,
            "table_reads": tiles, "quantized_us": spread(times["quantized"]), "plain_us": spread(times["plain"]),
            "quantized_read_floor_us_at_6.29TB/s": tiles * quant.nbytes / HBM_COPY_BYTES_PER_S * 1e6,
            "plain_read_floor_us_at_6.29TB/s": tiles * plain.nbytes / HBM_COPY_BYTES_PER_S * 1e6,
            "quantized_over_plain": med["quantized"] / med["plain"], "quantized_against_plain": verdict(times["quantized"], times["plain"]),
            "equals_plain_over_dequantised_rows_bit_for_bit": same,
            "against_the_original_table": {"share_of_sentences_with_the_same_first_video": first, "share_of_sentences_with_the_same_n_list": lists,
                                           "mean_share_of_the_n_list_in_both": common},
            "note": "launch-inclusive, every launch of the entry; plain ranks mx8_dequantize of the same codes; the agreement is on RANDOM "
                    "embeddings against the table before quantising and says nothing about recall"}


def q8_tolerance_ratio():
    """tests/test_q8_shortlist_gpu.py's lossy case (E = 512, bf16, blocks of 32 columns scaled by 2^-3 .. 2^3, run lengths 1, 3, 0, 17
    twenty times, then 300 and 2; S = 5, n = 16 and 128, the rows as videos and as runs): the largest |quantised score - float64 score
    of the table BEFORE quantising| over drn_amd.retrieve.quantized_score_bound."""
    import numpy as np
    from drn_amd import Shortlister
    from drn_amd.retrieve import quantized_score_bound
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    R = sum(lens)
    g = torch.Generator().manual_seed(4 + 1000 * R + 512)
    emb = torch.randn(R, 512, generator=g) * torch.exp2(torch.randint(-3, 4, (R, 16), generator=g).float()).repeat_interleave(32, dim=1)
    q = torch.randn(17, 512, generator=g)
    emb, q = emb.to("cuda:0", torch.bfloat16).contiguous(), q.to("cuda:0", torch.bfloat16)[:5].contiguous()
    video = torch.repeat_interleave(torch.arange(len(lens), device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(5, -1)
    worst = 0.0
    for off in (None, np.concatenate([[0], np.cumsum(lens)])):
        sl = Shortlister(emb, offsets=off, quantize="mxfp8")
        ref, tol = q.double() @ emb.double().t(), quantized_score_bound(emb, sl.scales, q)
        if off is not None:
            ref = torch.full((5, len(lens)), float("-inf"), dtype=torch.float64, device="cuda:0").scatter_reduce(1, video, ref, "amax")
            tol = torch.zeros_like(ref).scatter_reduce(1, video, tol, "amax")
        for n in (16, 128):
            got = sl.shortlist(q, n)
            ids = got.ids.clamp(min=0).long()
            ratio = (got.scores.double() - torch.gather(ref, 1, ids)).abs() / torch.gather(tol, 1, ids)
            worst = max(worst, float(ratio[got.ids >= 0].max()))
    return worst


def main_q8_shortlist(args):
    from drn_amd import Shortlister, ops
    out = args.out or os.path.join(ROOT, "profiles", "search_q8_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    codes = torch.empty((65536, 512), dtype=torch.uint8, device="cuda:0")
    scales = torch.empty((65536, 16), dtype=torch.uint8, device="cuda:0")
    quantize_us, reps = event_window(lambda: ops.quantize_rows_mx8(emb, codes, scales), args.rounds)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, both tables resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baseline": "plain: Shortlister over mx8_dequantize of the SAME codes and scales (bf16), the plain kernels, their code "
                                  "unchanged, in the same process.  A difference inside the plain table's own max - min is NO DIFFERENCE",
                      "what_this_does_not_say": "random embeddings: nothing here says anything about recall"},
           "table": {"rows": 65536, "E": 512, "dtype": "bf16",
                     "quantized_bytes": Shortlister.bytes_of(65536, 512, torch.bfloat16, "mxfp8"), "plain_bytes": Shortlister.bytes_of(65536, 512, torch.bfloat16),
                     "float32_bytes": Shortlister.bytes_of(65536, 512, torch.float32),
                     "bytes_per_row": {"quantized": Shortlister.bytes_of(1, 512, torch.bfloat16, "mxfp8"), "bf16": 1024, "fp32": 2048},
                     "quantize_us": dict(spread(quantize_us), launches_per_window=reps, what="ops.quantize_rows_mx8 of the whole table, one launch")},
           "tolerance_ratio": q8_tolerance_ratio(), "q8_shortlist": []}
    del codes, scales
    for S in (1, 8, 64):
        for n in (16, 128):
            for name, lens in SEGMENT_LAYOUTS:
                row = bench_q8_shortlist(name, lens, emb, S, n, args.rounds)
                res["q8_shortlist"].append(row)
                print(json.dumps({"q8_shortlist": row}), flush=True)
            json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


FILTER_SHAPES = [("65536x1", [1] * 65536, None, S) for S in (1, 8, 64)] + [("4096x16", [16] * 4096, None, S) for S in (1, 8, 64)] \
    + [("65536x1", [1] * 65536, "mxfp8", 8)]
FILTER_MASKS = ("ones", "half", "one_pct", "sixteenth", "per_sentence_one_pct")


def bench_filtered_shortlist(name, lens, quantize, emb, S, n, rounds):
    """shortlist(allow=) under the five masks beside (a) the unmasked launch on the same table and (b) for the shared masks the
    sub-table way -- gather the kept rows, build a Shortlister over them, shortlist, map the ids back -- with and without the
    construction; the masked all-ones list against the unmasked one and every shared masked list against the sub-table's, bit for bit."""
    import numpy as np
    from drn_amd import Shortlister, pack_allow
    dev = "cuda:0"
    R, V = int(emb.shape[0]), len(lens)
    lens_np = np.asarray(lens, dtype=np.int64)
    off = None if V == R else np.concatenate([[0], np.cumsum(lens_np)])
    g = torch.Generator(device=dev).manual_seed(S + n)
    q = torch.randn(S, 512, generator=g, device=dev).to(torch.bfloat16).contiguous()
    sl = Shortlister(emb, offsets=off, quantize=quantize)
    lens_dev = torch.as_tensor(lens_np, device=dev)
    sixteenth = torch.zeros(V, dtype=torch.bool, device=dev)
    sixteenth[5 * V // 16:6 * V // 16] = True
    masks = {"ones": torch.ones(V, dtype=torch.bool, device=dev), "half": torch.rand(V, generator=g, device=dev) < 0.5,
             "one_pct": torch.rand(V, generator=g, device=dev) < 0.01, "sixteenth": sixteenth,
             "per_sentence_one_pct": torch.rand(S, V, generator=g, device=dev) < 0.01}
    assert tuple(masks) == FILTER_MASKS
    words = {k: pack_allow(m.contiguous()) for k, m in masks.items()}
    outs = {k: sl.shortlist(q, n, allow=w) for k, w in words.items()}
    out_plain = sl.shortlist(q, n)

    def sub_table(mask):
        keep = torch.nonzero(mask)[:, 0]
        if off is None:
            return Shortlister(emb[keep].contiguous(), quantize=quantize), keep
        sub_off = np.concatenate([[0], np.cumsum(lens_np[keep.cpu().numpy()])])
        return Shortlister(emb[torch.repeat_interleave(mask, lens_dev)].contiguous(), offsets=sub_off, quantize=quantize), keep

    def via(sub, keep, out=None):
        got = sub.shortlist(q, n, out=out)
        return got, torch.where(got.ids >= 0, keep[got.ids.clamp(min=0).long()].to(torch.int32), got.ids)
    variants = {"unmasked": lambda: sl.shortlist(q, n, out=out_plain)}
    for k in FILTER_MASKS:
        variants[k] = lambda k=k: sl.shortlist(q, n, out=outs[k], allow=words[k])
    same = {"ones_equals_unmasked_bit_for_bit": all(torch.equal(a, b) for a, b in zip(outs["ones"], out_plain))}
    shared = ("half", "one_pct", "sixteenth")
    for k in shared:
        sub, keep = sub_table(masks[k])
        got, ids = via(sub, keep)
        same[k + "_equals_sub_table_bit_for_bit"] = bool(torch.equal(ids, outs[k].ids) and torch.equal(got.scores, outs[k].scores)
                                                         and torch.equal(got.n, outs[k].n))
        variants["sub_table_" + k] = lambda sub=sub, keep=keep, out=got: via(sub, keep, out)
        variants["sub_table_built_" + k] = lambda k=k: via(*sub_table(masks[k]))
    times, reps = interleaved_windows(variants, rounds)
    med = {k: statistics.median(ts) for k, ts in times.items()}
    width = lambda ts: max(ts) - min(ts)
    row = {"layout": name, "quantize": quantize, "R": R, "V": V, "E": 512, "S": S, "n": n, "dtype": "bf16",
           "entry": "drn_shortlist_%stopn%s_allow" % ("" if off is None else "segments_", "" if quantize is None else "_q8"),
           "blocks": -(-V // 256) if off is None else int(sl.plan.blk_vid.shape[0]) - 1, "table_bytes": sl.nbytes, "table_reads": -(-S // 16),
           "allowed": {k: int(m.sum()) for k, m in masks.items()}, "launches_per_window": reps, "answers": same,
           "unmasked_us": spread(times["unmasked"]), "masked_us": {}, "sub_table_us": {},
           "read_floor_us_at_6.29TB/s": -(-S // 16) * sl.nbytes / HBM_COPY_BYTES_PER_S * 1e6}
    for k in FILTER_MASKS:
        row["masked_us"][k] = dict(spread(times[k]), over_unmasked=med[k] / med["unmasked"], against_unmasked=verdict(times[k], times["unmasked"]))
    for k in shared:
        a, b = times["sub_table_" + k], times["sub_table_built_" + k]
        row["sub_table_us"][k] = {"shortlist_and_remap": spread(a), "with_construction": spread(b),
                                  "masked_over_shortlist_and_remap": med[k] / statistics.median(a), "masked_against_shortlist_and_remap": verdict(times[k], a),
                                  "masked_over_with_construction": med[k] / statistics.median(b), "masked_against_with_construction": verdict(times[k], b)}
    d = med["ones"] - med["unmasked"]
    row["C1"] = {"ones_minus_unmasked_median_us": d, "unmasked_max_minus_min_us": width(times["unmasked"]), "holds": d <= width(times["unmasked"]),
                 "says": "inside the unmasked launch's own spread" if d <= width(times["unmasked"])
                 else "THE ALL-ONES MASK IS SLOWER THAN THE UNMASKED LAUNCH BY MORE THAN ITS max - min"}
    row["C2"] = {}
    for k in ("sixteenth", "one_pct"):
        d = med[k] - med["ones"]
        row["C2"][k] = {"median_minus_ones_median_us": d, "ones_max_minus_min_us": width(times["ones"]), "holds": d <= width(times["ones"]),
                        "says": "no longer than the all-ones mask beyond its spread" if d <= width(times["ones"])
                        else "SLOWER THAN THE ALL-ONES MASK BY MORE THAN ITS max - min"}
    row["note"] = ("launch-inclusive, every launch of the entry; the sub-table way gathers the kept rows, builds a Shortlister over them (one "
                   "synchronise and a finiteness pass; a ragged table also rebuilds its offsets on the host), shortlists and maps the ids "
                   "back; its construction is timed inside the same event windows")
    return row


def main_filtered_shortlist(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_filtered_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the tables resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baselines": "(a) unmasked: the parent's entry on the same table, its code unchanged; (b) sub_table: the parent's only "
                                   "exact way for a shared mask, Shortlister(emb[keep].contiguous()) + shortlist + keep[ids], with and "
                                   "without the construction.  A difference inside the baseline's own max - min is NO DIFFERENCE",
                      "conditions": "derived, not measured: (C1) the all-ones mask does the unmasked launch's work plus at most 128 (ragged: "
                                    "144) mask words per workgroup; (C2) on one table the contiguous-1/16 and the 1 % mask do no more work than "
                                    "the all-ones mask and may not take longer than it beyond ITS max - min",
                      "what_this_does_not_say": "random embeddings: nothing here says anything about recall; pack_allow and allow_of are not "
                                                "timed; no kernel-only times (no profiler run); n = 16 only"},
           "masks": {"ones": "every video", "half": "random 50 %", "one_pct": "random 1 %",
                     "sixteenth": "the videos [5 V / 16, 6 V / 16): 15/16 of the blocks dark", "per_sentence_one_pct": "a random 1 % per sentence, (S, W)"},
           "filtered_shortlist": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for name, lens, quantize, S in FILTER_SHAPES:
        row = bench_filtered_shortlist(name, lens, quantize, emb, S, 16, args.rounds)
        res["filtered_shortlist"].append(row)
        print(json.dumps({"filtered_shortlist": row}), flush=True)
        json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


LATE_TOKENS = (("L8", 8, 8), ("L16", 16, 16), ("L16_len6", 16, 6), ("L32_len16", 32, 16))        # (name, L, live tokens of every sentence)
LATE_TORCH_MAX_ROWS = 512                                   # (a) is measured where S L stays at or below it: a 256 MiB int64 index beside the matrix


def bench_late_shortlist(name, lens, emb, S, n, rounds):
    """drn_shortlist_late_topn on R = 65,536 rows cut into videos by `lens`, the four token shapes of one (layout, S) taking turns with
    (b) shortlist() on the flattened tokens and (a) matmul + amax + masked sum + topk inside every round."""
    import numpy as np
    from drn_amd import SegmentShortlist, Shortlist, Shortlister
    R, V = int(emb.shape[0]), len(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    assert off[-1] == R
    g = torch.Generator(device="cuda:0").manual_seed(S + n)
    seg = Shortlister(emb, offsets=off)
    variants, flops = {}, {}
    for tag, L, live in LATE_TOKENS:
        q = torch.randn(S, L, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
        lengths = torch.full((S,), live, dtype=torch.int32, device="cuda:0")
        out = Shortlist(*seg.shortlist_late(q, lengths, n))
        variants["late_" + tag] = (lambda q=q, lengths=lengths, out=out: seg.shortlist_late(q, lengths, n, out=out))
        flops[tag] = 2.0 * S * live * R * 512
        if live == L:                                       # (b) cannot skip padding: it is measured at the all-live shapes and at 32 S rows
            flat = q.reshape(S * L, 512)
            out_flat = SegmentShortlist(*seg.shortlist(flat, n))
            variants["flat_" + tag] = (lambda flat=flat, out_flat=out_flat: seg.shortlist(flat, n, out=out_flat))
        if S * L <= LATE_TORCH_MAX_ROWS:
            index = torch.repeat_interleave(torch.arange(V, device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(S * L, R).contiguous()
            best = torch.empty((S * L, V), dtype=torch.bfloat16, device="cuda:0")
            alive = (torch.arange(L, device="cuda:0")[None, :] < lengths[:, None])[:, :, None]

            def torch_way(q=q, index=index, best=best, alive=alive, L=L):
                best.fill_(float("-inf"))
                best.scatter_reduce_(1, index, torch.matmul(q.reshape(S * L, 512), emb.t()), "amax")
                sim = best.view(S, L, V).float()
                return torch.topk(torch.where(alive, sim, torch.zeros_like(sim)).sum(dim=1), min(n, V), dim=1)
            variants["torch_" + tag] = torch_way
    # a control for (C2): L = 16 all live once more, on other random tokens in another tensor -- what two inputs of ONE shape differ by
    q16b, l16b = torch.randn(S, 16, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous(), torch.full((S,), 16, dtype=torch.int32, device="cuda:0")
    out16b = Shortlist(*seg.shortlist_late(q16b, l16b, n))
    variants["late_L16_other_tokens"] = lambda: seg.shortlist_late(q16b, l16b, n, out=out16b)
    q32 = torch.randn(S * 32, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    out32 = SegmentShortlist(*seg.shortlist(q32, n))
    variants["flat_L32"] = lambda: seg.shortlist(q32, n, out=out32)
    times, reps = interleaved_windows(variants, rounds)
    row = {"layout": name, "R": R, "V": V, "E": 512, "S": S, "n": n, "dtype": "bf16", "blocks": int(seg.plan.blk_vid.shape[0]) - 1,
           "launches_per_window": reps, "table_bytes": emb.numel() * emb.element_size(), "shapes": []}
    for tag, L, live in LATE_TOKENS:
        late = times["late_" + tag]
        shape = {"tokens": tag, "L": L, "live": live, "late_us": spread(late), "flops": flops[tag],
                 "tflops": flops[tag] / (statistics.median(late) * 1e-6) / 1e12, "table_reads": S * -(-live // 16)}
        if "flat_" + tag in times:
            shape["flat_shortlist_us"] = spread(times["flat_" + tag])
            shape["late_against_flat_shortlist"] = verdict(late, times["flat_" + tag])
        if "torch_" + tag in times:
            shape["matmul_amax_sum_topk_us"] = spread(times["torch_" + tag])
            shape["late_over_matmul_amax_sum_topk"] = statistics.median(late) / statistics.median(times["torch_" + tag])
            shape["late_against_matmul_amax_sum_topk"] = verdict(late, times["torch_" + tag])
        row["shapes"].append(shape)
    row["flat_shortlist_32S_rows_us"] = spread(times["flat_L32"])
    b, l16, l32 = times["flat_L16"], times["late_L16"], times["late_L32_len16"]
    over1, over2 = statistics.median(l16) - statistics.median(b), statistics.median(l32) - statistics.median(l16)
    row["C1"] = {"late_L16_minus_flat_16S_rows_us": over1, "flat_max_minus_min_us": max(b) - min(b), "holds": over1 <= max(b) - min(b)}
    row["C2"] = {"late_L32_len16_minus_late_L16_us": over2, "late_L16_max_minus_min_us": max(l16) - min(l16), "holds": over2 <= max(l16) - min(l16),
                 "control_late_L16_other_tokens_minus_late_L16_us": statistics.median(times["late_L16_other_tokens"]) - statistics.median(l16)}
    row["late_L16_other_tokens_us"] = spread(times["late_L16_other_tokens"])
    row["note"] = ("launch-inclusive, both launches of the late shortlist; flat_shortlist ranks the S L tokens as S L sentences (another answer: "
                   "per-token lists, all three launches of the segmented shortlist); torch scores in bf16, here fp32; table_reads counts the "
                   "block rows read once per (sentence, token tile)")
    return row


def late_tolerance_ratio():
    """tests/test_late_shortlist_gpu.py's random case (E = 512, run lengths 1, 3, 0, 17 twenty times, then 300 and 2; S = 5, L = 33 with
    lengths 33, 1, 16, 17, 20, n = 16, bf16): the largest |returned score - the float64 score| over tol = sum over the live t of the
    largest E * 2^-23 * sum |q_t * emb_r| of the video's rows + L * 2^-23 * sum over the live t of |sim_t|."""
    import numpy as np
    from drn_amd import Shortlister
    lens = [1, 3, 0, 17] * 20 + [300, 2]
    V, L, E = len(lens), 33, 512
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(sum(lens), E, generator=g).to("cuda:0", torch.bfloat16).contiguous()
    q = torch.randn(17, 64, E, generator=g).to("cuda:0", torch.bfloat16)[:5, :L].contiguous()
    lengths = torch.tensor([33, 1, 16, 17, 20], dtype=torch.int32, device="cuda:0")
    got = Shortlister(emb, offsets=np.concatenate([[0], np.cumsum(lens)])).shortlist_late(q, lengths, 16)
    video = torch.repeat_interleave(torch.arange(V, device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(5 * L, -1)
    flat = q.double().reshape(5 * L, E)
    sim = torch.full((5 * L, V), float("-inf"), dtype=torch.float64, device="cuda:0").scatter_reduce(1, video, flat @ emb.double().t(), "amax")
    tol = torch.zeros_like(sim).scatter_reduce(1, video, E * 2.0 ** -23 * (flat.abs() @ emb.double().abs().t()), "amax")
    live = (torch.arange(L, device="cuda:0")[None] < lengths[:, None])[:, :, None] & (torch.as_tensor(lens, device="cuda:0") > 0)[None, None]
    sim = torch.where(live, sim.reshape(5, L, V), torch.zeros((), dtype=torch.float64, device="cuda:0"))
    tol = torch.where(live, tol.reshape(5, L, V), torch.zeros((), dtype=torch.float64, device="cuda:0")).sum(dim=1) + L * 2.0 ** -23 * sim.abs().sum(dim=1)
    ids = got.ids.long()
    return float(((got.scores.double() - torch.gather(sim.sum(dim=1), 1, ids)).abs() / torch.gather(tol, 1, ids)).max())


def main_late_shortlist(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_late_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the table resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baselines": "(a) matmul_amax_sum_topk: torch.matmul on the flattened tokens, scatter_reduce_(amax) over the videos' rows, "
                                   "a masked sum over the tokens, torch.topk -- where S L <= %d; (b) flat_shortlist: shortlist() of the same "
                                   "table on the S L flattened tokens, the parent's code unchanged.  A difference inside the baseline's own "
                                   "max - min is NO DIFFERENCE" % LATE_TORCH_MAX_ROWS,
                      "conditions": "derived, not measured: (C1) L = 16 all live runs the tiles of (b) at 16 S query rows, sorts one key row "
                                    "where (b) sorts 16 and merges S lists where (b) merges 16 S, so it may not take longer than (b) beyond "
                                    "(b)'s max - min; (C2) L = 32 with lengths 16 never enters its second tile and may not take longer than "
                                    "L = 16 all live beyond ITS max - min",
                      "what_this_does_not_say": "random embeddings: nothing here says anything about recall; no kernel-only times (no profiler "
                                                "run); n = 16 only"},
           "tolerance_ratio": late_tolerance_ratio(), "late_shortlist": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for S in (1, 8, 64):
        for name, lens in SEGMENT_LAYOUTS[1:]:
            row = bench_late_shortlist(name, lens, emb, S, 16, args.rounds)
            res["late_shortlist"].append(row)
            print(json.dumps({"late_shortlist": row}), flush=True)
            for c in ("C1", "C2"):
                print("%s %s S = %d: %s" % (c, name, S, "holds" if row[c]["holds"] else "MISSED"), flush=True)
            json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


RANK_NOISE = 6.0                                            # the planted queries: a target's row plus this many standard normals a column


def bench_rank(emb, S, rounds):
    """Shortlister.rank / rank_late on R = 65,536 rows as 65,536 x 1 (plain), 4,096 x 16 (ragged) and late interaction at L = 16 on the
    ragged layout, each beside (a) the shortlist of n = 16 on the same table and queries, the parent's code path, and (b) what a caller
    does today for depth past 128: torch.matmul (scatter_reduce_(amax) when ragged, a sum over the tokens when late), two comparisons
    and sums.  All variants of one S take turns inside every round."""
    import numpy as np
    from drn_amd import Shortlister, TargetRank
    R, E, n, L = int(emb.shape[0]), 512, 16, 16
    lens = dict(SEGMENT_LAYOUTS)["4096x16"]
    V2 = len(lens)
    g = torch.Generator(device="cuda:0").manual_seed(S)
    q = torch.randn(S, E, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    tok = torch.randn(S, L, E, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    lengths = torch.full((S,), L, dtype=torch.int32, device="cuda:0")
    plain, seg = Shortlister(emb), Shortlister(emb, offsets=np.concatenate([[0], np.cumsum(lens)]))
    index = torch.repeat_interleave(torch.arange(V2, device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))
    # targets: the first sentences take places 0 .. 15 of their own list, the rest any video
    lists = {"plain": plain.shortlist(q, n), "ragged": seg.shortlist(q, n), "late": seg.shortlist_late(tok, lengths, n)}
    targets = {}
    for kind, short in lists.items():
        V = R if kind == "plain" else V2
        t = torch.randint(0, V, (S,), generator=g, device="cuda:0", dtype=torch.int32)
        k = min(S, n)
        t[:k] = short.ids[torch.arange(k, device="cuda:0"), torch.arange(k, device="cuda:0")]
        targets[kind] = t.contiguous()
    outs = {kind: TargetRank(*(plain.rank(q, targets[kind]) if kind == "plain" else seg.rank(q, targets[kind]) if kind == "ragged"
                               else seg.rank_late(tok, lengths, targets[kind]))) for kind in lists}
    best = torch.empty((S, V2), dtype=torch.bfloat16, device="cuda:0")
    best_late = torch.empty((S * L, V2), dtype=torch.bfloat16, device="cuda:0")
    where = {"plain": torch.arange(R, device="cuda:0")[None, :], "ragged": torch.arange(V2, device="cuda:0")[None, :]}

    def counted(sc, t, ar):
        ts = torch.gather(sc, 1, t.long()[:, None])
        return ((sc > ts) | ((sc == ts) & (ar < t[:, None]))).sum(dim=1), torch.isfinite(sc).sum(dim=1)

    def torch_plain():
        return counted(torch.matmul(q, emb.t()), targets["plain"], where["plain"])

    def torch_ragged():
        best.fill_(float("-inf"))
        best.scatter_reduce_(1, index[None].expand(S, R), torch.matmul(q, emb.t()), "amax")
        return counted(best, targets["ragged"], where["ragged"])

    def torch_late():
        best_late.fill_(float("-inf"))
        best_late.scatter_reduce_(1, index[None].expand(S * L, R), torch.matmul(tok.reshape(S * L, E), emb.t()), "amax")
        return counted(best_late.view(S, L, V2).float().sum(dim=1), targets["late"], where["ragged"])
    variants = {
        "rank_plain": lambda: plain.rank(q, targets["plain"], out=outs["plain"]),
        "shortlist_plain": lambda: plain.shortlist(q, n, out=lists["plain"]),
        "torch_plain": torch_plain,
        "rank_ragged": lambda: seg.rank(q, targets["ragged"], out=outs["ragged"]),
        "shortlist_ragged": lambda: seg.shortlist(q, n, out=lists["ragged"]),
        "torch_ragged": torch_ragged,
        "rank_late": lambda: seg.rank_late(tok, lengths, targets["late"], out=outs["late"]),
        "shortlist_late": lambda: seg.shortlist_late(tok, lengths, n, out=lists["late"]),
        "torch_late": torch_late,
    }
    times, reps = interleaved_windows(variants, rounds)
    torch_counts = {"plain": torch_plain()[0], "ragged": torch_ragged()[0], "late": torch_late()[0]}
    rows = []
    for kind in ("plain", "ragged", "late"):
        r, a, b = times["rank_" + kind], times["shortlist_" + kind], times["torch_" + kind]
        over = statistics.median(r) - statistics.median(a)
        got, short, t = outs[kind].rank.tolist(), lists[kind].ids.tolist(), targets[kind].tolist()
        agree_a = all((short[s][k] == t[s]) if 0 <= k < n else (t[s] not in short[s]) for s, k in enumerate(got))
        agree_b = sum(int(x == y) for x, y in zip(got, torch_counts[kind].tolist()))
        rows.append({"ranking": kind, "layout": "65536x1" if kind == "plain" else "4096x16", "R": R, "V": R if kind == "plain" else V2, "E": E, "S": S,
                     "L": L if kind == "late" else None, "dtype": "bf16", "launches_per_window": {k: reps[k + "_" + kind] for k in ("rank", "shortlist", "torch")},
                     "rank_us": spread(r), "shortlist_n16_us": spread(a), "matmul_compare_sum_us": spread(b),
                     "C1": {"rank_minus_shortlist_us": over, "shortlist_max_minus_min_us": max(a) - min(a), "verdict": "HOLDS" if over <= max(a) - min(a) else "MISSED"},
                     "rank_over_shortlist_n16": statistics.median(r) / statistics.median(a),
                     "rank_over_matmul_compare_sum": statistics.median(r) / statistics.median(b),
                     "every_rank_below_16_is_the_lists_place": agree_a, "sentences_equal_to_matmul_compare_sum": agree_b,
                     "ranks_below_16": sum(1 for k in got if 0 <= k < n)})
    return rows


def rank_planted_recall(emb, sentences=256, batch=64):
    """evaluate_shortlist on PLANTED structure -- a query is its target's row plus RANK_NOISE standard normals a column; no trained encoder
    is involved -- on the plain table and on the same table quantised to block-scaled FP8, side by side."""
    from drn_amd import Shortlister, evaluate_shortlist
    R = int(emb.shape[0])
    names = ["v%05d" % v for v in range(R)]
    g = torch.Generator(device="cuda:0").manual_seed(1)
    t = torch.randint(0, R, (sentences,), generator=g, device="cuda:0")
    q = (emb[t].float() + RANK_NOISE * torch.randn(sentences, 512, generator=g, device="cuda:0")).to(torch.bfloat16).contiguous()
    host = t.tolist()
    batches = [([names[v] for v in host[a:a + batch]], q[a:a + batch].contiguous()) for a in range(0, sentences, batch)]
    res = {"sentences": sentences, "noise": RANK_NOISE, "what_this_is": "planted structure (a target's row plus noise), not a trained encoder"}
    ranks = {}
    for kind, sl in (("bf16", Shortlister(emb, names=names)), ("mxfp8", Shortlister(emb, names=names, quantize="mxfp8"))):
        got = evaluate_shortlist(sl, batches, topks=(1, 10, 100, 1000))
        ranks[kind] = got.ranks
        res[kind] = {"recall_at": dict(zip(("1", "10", "100", "1000"), got.recall)), "mrr": got.mrr, "median_rank": got.median_rank}
    d = ranks["mxfp8"].astype("int64") - ranks["bf16"].astype("int64")
    res["mxfp8_minus_bf16_places"] = {"mean": float(d.mean()), "largest_loss": int(d.max()), "largest_gain": int(-d.min()),
                                      "sentences_unchanged": int((d == 0).sum())}
    return res


def main_rank(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_rank_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the table resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baselines": "(a) shortlist_n16: shortlist() / shortlist_late() with n = 16 on the same table and queries, the parent's code "
                                   "unchanged; (b) matmul_compare_sum: torch.matmul (scatter_reduce_(amax) over the videos' rows when ragged, a sum "
                                   "over the tokens when late), two comparisons and sums -- what a caller does today for depth past 128",
                      "condition": "derived, not measured: (C1) rank does the reads and the MFMA chain of (a), counts where (a) sorts 256 keys a "
                                   "sentence and merges, and pays one more small launch, so it may not take longer than (a) beyond (a)'s max - min",
                      "what_this_does_not_say": "random embeddings: the timings say nothing about recall; planted_recall is planted structure, not "
                                                "a trained encoder; no kernel-only times (no profiler run)"},
           "rank": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for S in (1, 8, 64):
        for row in bench_rank(emb, S, args.rounds):
            res["rank"].append(row)
            print(json.dumps({"rank": row}), flush=True)
            print("C1 %s S = %d: %s (rank / (b) = %.3f)" % (row["ranking"], S, row["C1"]["verdict"], row["rank_over_matmul_compare_sum"]), flush=True)
        json.dump(res, open(out, "w"), indent=1)
    res["shapes_where_every_rank_below_16_is_the_lists_place"] = "%d of %d" % (sum(r["every_rank_below_16_is_the_lists_place"] for r in res["rank"]),
                                                                               len(res["rank"]))
    res["planted_recall"] = rank_planted_recall(emb)
    print(json.dumps({"planted_recall": res["planted_recall"]}), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


RERANK_WIDTHS = (128, 32)                                   # C: distinct random positions per sentence


def bench_rerank(name, lens, emb, S, n, rounds):
    """drn_shortlist_rerank on R = 65,536 rows cut into videos by `lens`, L = 16 all live: rerank_late at C = 128 and 32 taking turns with
    (A) pack_allow of the candidate mask + shortlist_late(allow=), the parent's way to the same answer, (B) the unmasked shortlist_late,
    and rerank (one query row a sentence) beside shortlist(allow=).  rerank_late's fields are asserted equal to (A)'s before timing."""
    import numpy as np
    from drn_amd import SegmentShortlist, Shortlist, Shortlister, candidates_mask, pack_allow
    R, V, L = int(emb.shape[0]), len(lens), 16
    off = np.concatenate([[0], np.cumsum(lens)])
    assert off[-1] == R
    g = torch.Generator(device="cuda:0").manual_seed(S + n)
    seg = Shortlister(emb, offsets=off)
    q = torch.randn(S, L, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    q1 = q[:, 0].contiguous()
    lengths = torch.full((S,), L, dtype=torch.int32, device="cuda:0")
    variants = {}
    out_b = Shortlist(*seg.shortlist_late(q, lengths, n))
    variants["late_unmasked"] = lambda: seg.shortlist_late(q, lengths, n, out=out_b)
    for C in RERANK_WIDTHS:
        cand = torch.stack([torch.randperm(V, generator=g, device="cuda:0")[:C] for _ in range(S)]).to(torch.int32).contiguous()
        mask = candidates_mask(cand, V)
        words = pack_allow(mask)
        out_r, out_a = Shortlist(*seg.rerank_late(cand, q, lengths, n)), Shortlist(*seg.shortlist_late(q, lengths, n, allow=words))
        for f in Shortlist._fields:
            assert torch.equal(getattr(out_r, f), getattr(out_a, f)), (name, S, C, f)
        out_r1, out_a1 = Shortlist(*seg.rerank(cand, q1, n)), SegmentShortlist(*seg.shortlist(q1, n, allow=words))
        for f in Shortlist._fields:
            assert torch.equal(getattr(out_r1, f), getattr(out_a1, f)), (name, S, C, f, "rerank")

        def masked_late(mask=mask, words=words, out_a=out_a):
            pack_allow(mask, out=words)
            return seg.shortlist_late(q, lengths, n, out=out_a, allow=words)

        def masked_segments(mask=mask, words=words, out_a1=out_a1):
            pack_allow(mask, out=words)
            return seg.shortlist(q1, n, out=out_a1, allow=words)
        variants["rerank_late_C%d" % C] = lambda cand=cand, out_r=out_r: seg.rerank_late(cand, q, lengths, n, out=out_r)
        variants["masked_late_C%d" % C] = masked_late
        variants["rerank_C%d" % C] = lambda cand=cand, out_r1=out_r1: seg.rerank(cand, q1, n, out=out_r1)
        variants["masked_segments_C%d" % C] = masked_segments
    times, reps = interleaved_windows(variants, rounds)
    row = {"layout": name, "R": R, "V": V, "E": 512, "S": S, "L": L, "n": n, "dtype": "bf16", "launches_per_window": reps,
           "late_unmasked_us": spread(times["late_unmasked"]), "widths": []}
    b = times["late_unmasked"]
    for C in RERANK_WIDTHS:
        r, a = times["rerank_late_C%d" % C], times["masked_late_C%d" % C]
        r1, a1 = times["rerank_C%d" % C], times["masked_segments_C%d" % C]
        over = statistics.median(r) - statistics.median(a)
        row["widths"].append({
            "C": C, "rows_scored_over_R": C * (R / V) / R, "rerank_late_us": spread(r), "A_pack_allow_plus_masked_late_us": spread(a),
            "rerank_late_over_A": statistics.median(r) / statistics.median(a), "rerank_late_over_B": statistics.median(r) / statistics.median(b),
            "R1": {"rerank_late_minus_A_us": over, "A_max_minus_min_us": max(a) - min(a), "holds": over <= max(a) - min(a)},
            "rerank_us": spread(r1), "pack_allow_plus_masked_segments_us": spread(a1),
            "rerank_over_masked_segments": statistics.median(r1) / statistics.median(a1), "rerank_against_masked_segments": verdict(r1, a1)})
    row["note"] = ("launch-inclusive: both launches of the rerank; (A) is three launches, pack_allow and the two of the masked late shortlist "
                   "(the mask itself is given: making it from the ids is not timed); (B) is the unmasked late shortlist; rerank / "
                   "masked_segments: one query row a sentence, best segment")
    return row


def main_rerank(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_rerank_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the table resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baselines": "(A) pack_allow of the candidates' mask + shortlist_late(allow=), the parent's way to the same answer, the "
                                   "fields asserted equal before timing; (B) the unmasked shortlist_late.  A difference inside the baseline's "
                                   "own max - min is NO DIFFERENCE",
                      "condition": "derived, not measured: (R1) rerank_late does a subset of (A)'s row reads and MFMAs, C * mean run / R of them, "
                                   "and one launch fewer, so it may not take longer than (A) beyond (A)'s max - min; at S = 1 both sit on their "
                                   "launches and may tie",
                      "what_this_does_not_say": "random embeddings and random candidates: nothing here says anything about recall, or about what "
                                                "depth a coarse stage needs; bf16 only: no fp32, no FP8 tables; C = 128 and 32 only, not C = "
                                                "1024; n = 16 and L = 16 only; no kernel-only times (no profiler run)"},
           "rerank": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for S in (1, 8, 64):
        for name, lens in SEGMENT_LAYOUTS[1:]:
            row = bench_rerank(name, lens, emb, S, 16, args.rounds)
            res["rerank"].append(row)
            print(json.dumps({"rerank": row}), flush=True)
            for w in row["widths"]:
                print("R1 %s S = %d C = %d: %s (rerank_late / A = %.3f, / B = %.3f)" % (name, S, w["C"], "holds" if w["R1"]["holds"] else "MISSED",
                                                                                        w["rerank_late_over_A"], w["rerank_late_over_B"]), flush=True)
            json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


SHARD_COUNTS = (1, 4, 16)                                   # K equal shards of the 65,536 rows
GROWTH_ROWS = 1024                                          # rows that arrive in (G1)


def equal_shards(emb, lens, K, quantize=()):
    """The table cut into K Shortlisters of R / K rows each over CLONED slices (V / K videos each; ragged when the layout is); the shards
    whose number is in `quantize` are kept in block-scaled FP8."""
    import numpy as np
    from drn_amd import Shortlister
    R, V = int(emb.shape[0]), len(lens)
    assert V % K == 0 and R % K == 0
    off = np.concatenate([[0], np.cumsum(lens)])
    shards = []
    for k in range(K):
        a, b = k * V // K, (k + 1) * V // K
        q8 = "mxfp8" if k in quantize else None
        rows = emb[int(off[a]):int(off[b])].clone()
        shards.append(Shortlister(rows, quantize=q8) if max(lens) == 1 else Shortlister(rows, offsets=off[a:b + 1] - off[a], quantize=q8))
    return shards


def same_fields(a, b, what):
    for f in a._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


def bench_sharded_shortlist(name, lens, emb, single, sharded, S, n, rounds):
    """ShardedShortlister.shortlist at K = 1 / 4 / 16 equal shards beside the single Shortlister over the same rows (the parent's code,
    unchanged) and the merge launch alone on the lists the call left; every field asserted equal to the single table's before timing."""
    from drn_amd import ops
    g = torch.Generator(device="cuda:0").manual_seed(S + n)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    out_single = single.shortlist(q, n)
    variants = {"single": lambda: single.shortlist(q, n, out=out_single)}
    for K, sh in sharded.items():
        out = sh.shortlist(q, n)
        same_fields(out, out_single, (name, K, S, n))
        lists = sh._lists(S, n)
        rows = (lists[3], out[3]) if len(out) == 4 else (None, None)
        variants["sharded_K%d" % K] = lambda sh=sh, out=out: sh.shortlist(q, n, out=out)
        variants["merge_K%d" % K] = lambda sh=sh, out=out, lists=lists, rows=rows: ops.shortlist_merge_lists(
            lists[0], lists[1], lists[2], rows[0], sh.bases_device, n, out[0], out[1], out[2], rows=rows[1])
    times, reps = interleaved_windows(variants, rounds)
    base = times["single"]
    row = {"layout": name, "R": int(emb.shape[0]), "V": len(lens), "E": 512, "S": S, "n": n, "dtype": "bf16", "launches_per_window": reps,
           "single_us": spread(base), "shards": []}
    for K in sharded:
        t, m = times["sharded_K%d" % K], times["merge_K%d" % K]
        row["shards"].append({"K": K, "sharded_us": spread(t), "merge_alone_us": spread(m),
                              "sharded_over_single": statistics.median(t) / statistics.median(base), "sharded_against_single": verdict(t, base),
                              "merge_share_of_sharded": statistics.median(m) / statistics.median(t)})
    row["note"] = ("launch-inclusive: K shards' entries one after the other on one stream (two launches each on the plain layout, three on the "
                   "ragged one) and the merge launch; merge_alone is the merge launch on the stacked lists the call left")
    return row


def bench_sharded_other(name, lens, emb, S, n, rounds):
    """A mixed object (half FP8, half bf16: K = 2) beside the single plain Shortlister over the same rows (the FP8 half dequantised), and
    -- on the ragged layout -- shortlist_late at 16 tokens on K = 4 shards beside the single table."""
    import numpy as np
    from drn_amd import ShardedShortlister, Shortlister
    g = torch.Generator(device="cuda:0").manual_seed(3 * S + n)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    ragged = max(lens) > 1
    off = np.concatenate([[0], np.cumsum(lens)])
    cold, hot = equal_shards(emb, lens, 2, quantize=(0,))
    rows = torch.cat([cold.dequantized().embeddings, hot.embeddings]).contiguous()
    single = Shortlister(rows, offsets=off) if ragged else Shortlister(rows)
    mixed = ShardedShortlister([cold, hot])
    out_s, out_m = single.shortlist(q, n), mixed.shortlist(q, n)
    same_fields(out_m, out_s, (name, "mixed", S, n))
    variants = {"single": lambda: single.shortlist(q, n, out=out_s), "mixed": lambda: mixed.shortlist(q, n, out=out_m)}
    if ragged:
        L = 16
        tok = torch.randn(S, L, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
        lengths = torch.full((S,), L, dtype=torch.int32, device="cuda:0")
        whole, four = Shortlister(emb, offsets=off), ShardedShortlister(equal_shards(emb, lens, 4))
        out_w, out_f = whole.shortlist_late(tok, lengths, n), four.shortlist_late(tok, lengths, n)
        same_fields(out_f, out_w, (name, "late", S, n))
        variants["late_single"] = lambda: whole.shortlist_late(tok, lengths, n, out=out_w)
        variants["late_K4"] = lambda: four.shortlist_late(tok, lengths, n, out=out_f)
    times, reps = interleaved_windows(variants, rounds)
    row = {"layout": name, "S": S, "n": n, "launches_per_window": reps, "table_bytes": {"single_bf16": single.nbytes, "mixed": mixed.nbytes},
           "single_plain_us": spread(times["single"]), "mixed_fp8_bf16_K2_us": spread(times["mixed"]),
           "mixed_over_single": statistics.median(times["mixed"]) / statistics.median(times["single"]),
           "mixed_against_single": verdict(times["mixed"], times["single"])}
    if ragged:
        row.update({"L": 16, "late_single_us": spread(times["late_single"]), "late_K4_us": spread(times["late_K4"]),
                    "late_K4_over_single": statistics.median(times["late_K4"]) / statistics.median(times["late_single"]),
                    "late_K4_against_single": verdict(times["late_K4"], times["late_single"])})
    return row


def bench_growth(name, lens, emb, new_rows, new_lens, S, n, rounds, iters=10):
    """(G1) two ways to add GROWTH_ROWS rows to the resident table and shortlist once: sharded.append(Shortlister(new_rows)) + shortlist
    beside torch.cat + Shortlister(...) + shortlist on the same tensors, the parent's only way.  Host clock from before the first call to
    after a device synchronise; the two take turns inside every round; a round is the mean of `iters` runs."""
    import numpy as np
    from drn_amd import ShardedShortlister, Shortlister
    ragged = max(lens) > 1
    off, new_off = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(new_lens)])
    both_off = np.concatenate([off, off[-1] + new_off[1:]])
    make = (lambda rows, o: Shortlister(rows, offsets=o)) if ragged else (lambda rows, o: Shortlister(rows))
    base = make(emb, off)
    g = torch.Generator(device="cuda:0").manual_seed(7 * S + n)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()

    def append_way():
        sh = ShardedShortlister([base])                      # (the resident object: not timed)
        sh.shortlist(q, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = sh.append(make(new_rows, new_off)).shortlist(q, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, got

    def rebuild_way():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = make(torch.cat([emb, new_rows]), both_off).shortlist(q, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, got
    same_fields(append_way()[1], rebuild_way()[1], (name, "growth", S, n))
    a, b = [], []
    for _ in range(rounds):
        a.append(statistics.mean(append_way()[0] for _ in range(iters)))
        b.append(statistics.mean(rebuild_way()[0] for _ in range(iters)))
    gain = statistics.median(b) - statistics.median(a)
    return {"layout": name, "S": S, "n": n, "resident_rows": int(emb.shape[0]), "new_rows": int(new_rows.shape[0]), "runs_per_round": iters,
            "append_plus_shortlist_us": spread(a), "cat_plus_rebuild_plus_shortlist_us": spread(b),
            "append_over_rebuild": statistics.median(a) / statistics.median(b),
            "G1": {"rebuild_minus_append_us": gain, "rebuild_max_minus_min_us": max(b) - min(b), "holds": gain > max(b) - min(b)}}


def main_sharded_shortlist(args):
    from drn_amd import ShardedShortlister, Shortlister
    import numpy as np
    out = args.out or os.path.join(ROOT, "profiles", "search_sharded_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the tables resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call; (G1): "
                               "host clock from before the first call to after a device synchronise, a round = the mean of 10 runs",
                      "baselines": "single: ONE Shortlister over the same rows, the parent's code unchanged, in the same process, every field "
                                   "asserted equal before timing.  A difference inside the baseline's own max - min is NO DIFFERENCE",
                      "condition": "derived, not measured: (G1) adding 1,024 rows by append + shortlist touches 1,024 new rows and launches K + 1 "
                                   "shards' entries and a merge; torch.cat + Shortlister + shortlist copies the whole table, checks all of it "
                                   "for finiteness with a synchronise and makes a new plan and workspaces, so the first must take less than "
                                   "the second by more than the second's own max - min",
                      "what_this_does_not_say": "random embeddings: nothing here says anything about recall; bf16 queries only; equal shards only "
                                                "(a small hot shard beside a large cold one is measured in (G1) alone); shards run one after "
                                                "the other on one stream: parallel streams are not tried; no kernel-only times (no profiler "
                                                "run); K = 64 is not measured"},
           "sharded_shortlist": [], "mixed_and_late": [], "growth": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    new_rows = torch.randn(GROWTH_ROWS, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()

    def save():
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for name, lens in SEGMENT_LAYOUTS[:2]:
        off = np.concatenate([[0], np.cumsum(lens)])
        single = Shortlister(emb) if max(lens) == 1 else Shortlister(emb, offsets=off)
        sharded = {K: ShardedShortlister(equal_shards(emb, lens, K)) for K in SHARD_COUNTS}
        for S in (1, 8, 64):
            for n in (16, 128):
                row = bench_sharded_shortlist(name, lens, emb, single, sharded, S, n, args.rounds)
                res["sharded_shortlist"].append(row)
                print(json.dumps({"sharded_shortlist": row}), flush=True)
                for k in row["shards"]:
                    print("%s S = %d n = %d K = %d: sharded / single = %.3f (%s), the merge alone %.1f us" % (
                        name, S, n, k["K"], k["sharded_over_single"], k["sharded_against_single"], k["merge_alone_us"]["median"]), flush=True)
                save()
        del sharded
        for S in (1, 8, 64):
            row = bench_sharded_other(name, lens, emb, S, 16, args.rounds)
            res["mixed_and_late"].append(row)
            print(json.dumps({"mixed_and_late": row}), flush=True)
            new_lens = [lens[0]] * (GROWTH_ROWS // lens[0])
            row = bench_growth(name, lens, emb, new_rows, new_lens, S, 16, args.rounds)
            res["growth"].append(row)
            print(json.dumps({"growth": row}), flush=True)
            print("G1 %s S = %d: %s (append / rebuild = %.3f)" % (name, S, "HOLDS" if row["G1"]["holds"] else "MISSED", row["append_over_rebuild"]),
                  flush=True)
            save()
    save()
    print("wrote", out)


def bench_sharded_rank(name, lens, emb, single, sharded, S, rounds):
    """ShardedShortlister.rank, rerank (C = 128, n = 16) and -- on the ragged layout -- rank_late (16 tokens) at K = 1 / 4 / 16 equal
    shards beside the single Shortlister over the same rows (the parent's code, unchanged); every field asserted equal to the single
    table's before timing."""
    g = torch.Generator(device="cuda:0").manual_seed(11 * S)
    V, ragged = len(lens), max(lens) > 1
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    targets = torch.randint(0, V, (S,), generator=g, device="cuda:0").to(torch.int32)
    cands = torch.randint(0, V, (S, 128), generator=g, device="cuda:0").to(torch.int32)
    calls = {"rank": lambda o, out=None: o.rank(q, targets, out=out), "rerank": lambda o, out=None: o.rerank(cands, q, 16, out=out)}
    if ragged:
        tok = torch.randn(S, 16, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
        lengths = torch.full((S,), 16, dtype=torch.int32, device="cuda:0")
        calls["rank_late"] = lambda o, out=None: o.rank_late(tok, lengths, targets, out=out)
    row = {"layout": name, "R": int(emb.shape[0]), "V": V, "E": 512, "S": S, "dtype": "bf16", "C": 128, "n": 16, "L_late": 16, "methods": {}}
    for method, call in calls.items():
        out_single = call(single)
        variants = {"single": lambda call=call, out=out_single: call(single, out)}
        for K, sh in sharded.items():
            out = call(sh)
            same_fields(out, out_single, (name, method, K, S))
            variants["sharded_K%d" % K] = lambda call=call, sh=sh, out=out: call(sh, out)
        times, reps = interleaved_windows(variants, rounds)
        base = times["single"]
        row["methods"][method] = {"launches_per_window": reps, "single_us": spread(base), "shards": [
            {"K": K, "sharded_us": spread(times["sharded_K%d" % K]),
             "sharded_over_single": statistics.median(times["sharded_K%d" % K]) / statistics.median(base),
             "sharded_against_single": verdict(times["sharded_K%d" % K], base)} for K in sharded]}
    row["note"] = ("launch-inclusive: a sharded rank is 2 K + 3 launches on one stream against the single table's 3, a sharded rerank "
                   "2 K + 2 against 2")
    return row


def bench_rank_growth(name, lens, emb, new_rows, new_lens, S, rounds, iters=10):
    """Two ways to add GROWTH_ROWS rows to the resident table and rank once: sharded.append(Shortlister(new_rows)) + rank beside torch.cat
    + Shortlister(...) + rank on the same tensors.  Host clock from before the first call to after a device synchronise; the two take
    turns inside every round; a round is the mean of `iters` runs."""
    import numpy as np
    from drn_amd import ShardedShortlister, Shortlister
    ragged = max(lens) > 1
    off, new_off = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(new_lens)])
    both_off = np.concatenate([off, off[-1] + new_off[1:]])
    make = (lambda rows, o: Shortlister(rows, offsets=o)) if ragged else (lambda rows, o: Shortlister(rows))
    base = make(emb, off)
    g = torch.Generator(device="cuda:0").manual_seed(13 * S)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    targets = torch.randint(0, len(lens) + len(new_lens), (S,), generator=g, device="cuda:0").to(torch.int32)

    def append_way():
        sh = ShardedShortlister([base])                      # (the resident object: not timed)
        sh.rank(q, targets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = sh.append(make(new_rows, new_off)).rank(q, targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, got

    def rebuild_way():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = make(torch.cat([emb, new_rows]), both_off).rank(q, targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, got
    same_fields(append_way()[1], rebuild_way()[1], (name, "growth", S))
    a, b = [], []
    for _ in range(rounds):
        a.append(statistics.mean(append_way()[0] for _ in range(iters)))
        b.append(statistics.mean(rebuild_way()[0] for _ in range(iters)))
    gain = statistics.median(b) - statistics.median(a)
    return {"layout": name, "S": S, "resident_rows": int(emb.shape[0]), "new_rows": int(new_rows.shape[0]), "runs_per_round": iters,
            "append_plus_rank_us": spread(a), "cat_plus_rebuild_plus_rank_us": spread(b), "append_over_rebuild": statistics.median(a) / statistics.median(b),
            "gain": {"rebuild_minus_append_us": gain, "rebuild_max_minus_min_us": max(b) - min(b), "beyond_the_baselines_spread": gain > max(b) - min(b)}}


def main_sharded_rank(args):
    from drn_amd import ShardedShortlister, Shortlister
    import numpy as np
    out = args.out or os.path.join(ROOT, "profiles", "search_sharded_rank_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the tables resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call; growth: "
                               "host clock from before the first call to after a device synchronise, a round = the mean of 10 runs",
                      "baselines": "single: ONE Shortlister over the same rows, the parent's code unchanged, in the same process, every field "
                                   "asserted equal before timing.  A difference inside the baseline's own max - min is NO DIFFERENCE",
                      "what_this_does_not_say": "no time is required of the sharded calls: 2 K + 3 launches stand against 3.  Random embeddings: "
                                                "nothing here says anything about recall; bf16 queries only; equal shards only (a small new "
                                                "shard beside a large resident one in growth alone); no mask; shards run one after the other "
                                                "on one stream; no kernel-only times (no profiler run); K = 64 and FP8 shards are not "
                                                "measured"},
           "sharded_rank": [], "growth": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    new_rows = torch.randn(GROWTH_ROWS, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()

    def save():
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for name, lens in SEGMENT_LAYOUTS[:2]:
        off = np.concatenate([[0], np.cumsum(lens)])
        single = Shortlister(emb) if max(lens) == 1 else Shortlister(emb, offsets=off)
        sharded = {K: ShardedShortlister(equal_shards(emb, lens, K)) for K in SHARD_COUNTS}
        for S in (1, 8, 64):
            row = bench_sharded_rank(name, lens, emb, single, sharded, S, args.rounds)
            res["sharded_rank"].append(row)
            print(json.dumps({"sharded_rank": row}), flush=True)
            for method, m in row["methods"].items():
                for k in m["shards"]:
                    print("%s %s S = %d K = %d: sharded / single = %.3f (%s), %.1f against %.1f us" % (
                        name, method, S, k["K"], k["sharded_over_single"], k["sharded_against_single"], k["sharded_us"]["median"],
                        m["single_us"]["median"]), flush=True)
            save()
        del sharded
        for S in (1, 8, 64):
            new_lens = [lens[0]] * (GROWTH_ROWS // lens[0])
            row = bench_rank_growth(name, lens, emb, new_rows, new_lens, S, args.rounds)
            res["growth"].append(row)
            print(json.dumps({"growth": row}), flush=True)
            print("growth %s S = %d: append / rebuild = %.3f (%s the rebuild's own spread)" % (
                name, S, row["append_over_rebuild"], "BEYOND" if row["gain"]["beyond_the_baselines_spread"] else "INSIDE"), flush=True)
            save()
    save()
    print("wrote", out)


HBM_PEAK_TBS = 8.0                                          # the MI355X's HBM3E peak by its data sheet (a float4 copy reaches about 6.3)
COMPACT_FORMATS = (("bf16", (), "same"), ("fp8", "all", "same"), ("half_fp8_to_plain", "even", None))


def compact_route(sh, mask_dev, mask_host, lens, lens_dev, target):
    """The way back to one table WITHOUT compact(): dequantise the FP8 shards in torch, torch.cat, index_select of the survivors, and a
    fresh Shortlister, whose constructor reads the whole table again for finiteness and quantises it when the target is FP8."""
    import numpy as np
    from drn_amd import Shortlister
    from drn_amd.index import mx8_dequantize
    rows = torch.cat([s.embeddings if s.quantize is None else mx8_dequantize(s.codes, s.scales, s.dtype) for s in sh.shards])
    if max(lens) == 1:
        return Shortlister(rows.index_select(0, mask_dev.nonzero().squeeze(1)), quantize=target)
    live = torch.repeat_interleave(mask_dev, lens_dev)
    off = np.concatenate([[0], np.cumsum(np.asarray(lens)[mask_host])])
    return Shortlister(rows.index_select(0, live.nonzero().squeeze(1)), offsets=off, quantize=target)


def compact_rows_bytes(sh, kept_rows, target, V):
    """Bytes the rows launches read plus bytes they write, from the shapes: every kept row once in its source format and once in the
    target's (512 columns: 1024 bytes in bf16, 528 in FP8), the positions of every video (4 bytes) and, on a ragged corpus, two source
    offsets a video and one new offset a kept video -- counted as 12 bytes a video, an upper bound."""
    read = sum(n * (1024 if s.quantize is None else 528) for s, n in zip(sh.shards, kept_rows))
    return read + sum(kept_rows) * (1024 if target is None else 528) + V * (4 if sh.shards[0]._seg is None else 16)


def bench_compact(name, lens, emb, fmt, K, mask_name, rounds, iters=5):
    """ShardedShortlister.compact beside compact_route on the same shards and mask: host clock from before the call to after a device
    synchronise, the two taking turns inside every round, a round = the mean of `iters` runs.  Before timing the result is asserted
    equal to compact_reference byte for byte, and to the route's table wherever the two are promised equal (a plain target)."""
    import numpy as np
    from drn_amd import ShardedShortlister, compact_reference, ops, pack_allow
    label, which, quantize = fmt
    q8 = range(K) if which == "all" else range(0, K, 2) if which == "even" else ()
    sh = ShardedShortlister(equal_shards(emb, lens, K, quantize=q8))
    V = len(sh)
    lens_dev = torch.tensor(lens, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(K)
    mask_dev = torch.ones(V, dtype=torch.bool, device="cuda:0") if mask_name == "all_kept" else torch.rand(V, generator=g, device="cuda:0") >= 0.1
    mask_host = mask_dev.cpu().numpy()
    keep = None if mask_name == "all_kept" else pack_allow(mask_dev)
    target = sh.shards[0].quantize if quantize == "same" else quantize
    got, want, route = sh.compact(keep, quantize=quantize), compact_reference(sh, keep=mask_dev.cpu(), quantize=quantize), \
        compact_route(sh, mask_dev, mask_host, lens, lens_dev, target)
    assert got.kept == want.kept and torch.equal(got.positions, want.positions)
    tensors = lambda t: (t.embeddings,) if t.quantize is None else (t.codes, t.scales)
    for a, b in zip(tensors(got.table), tensors(want.table)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, label, K, mask_name)
    route_equal = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(tensors(got.table), tensors(route)))
    assert route_equal or target is not None, (name, label, K, mask_name)     # (FP8 -> FP8 copies bytes; the route requantises: equality is not promised)
    if got.table._seg is not None:
        assert torch.equal(got.table.offsets, want.table.offsets) and torch.equal(got.table.offsets, route.offsets)
    del want, route

    def timed(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6
    ours, theirs, rows_us = [], [], []
    for _ in range(rounds):
        ours.append(statistics.mean(timed(lambda: sh.compact(keep, quantize=quantize)) for _ in range(iters)))
        theirs.append(statistics.mean(timed(lambda: compact_route(sh, mask_dev, mask_host, lens, lens_dev, target)) for _ in range(iters)))
        ops.kernel_timer = []
        sh.compact(keep, quantize=quantize)
        torch.cuda.synchronize()
        rows_us.append(sum(e0.elapsed_time(e1) for tag, _, e0, e1 in ops.kernel_timer if tag == "compact_rows") * 1e3)
        ops.kernel_timer = None
    off = np.concatenate([[0], np.cumsum(lens)])
    kept_rows = [int(np.asarray(lens)[a:b][mask_host[a:b]].sum()) for a, b in zip(sh.bases[:-1], sh.bases[1:])]
    nbytes = compact_rows_bytes(sh, kept_rows, target, V)
    gain = statistics.median(theirs) - statistics.median(ours)
    holds = gain > max(theirs) - min(theirs)                 # (less than the route by more than the route's own spread)
    return {"layout": name, "R": int(off[-1]), "V": V, "E": 512, "formats": label, "target": target or "plain", "K": K, "mask": mask_name,
            "kept_videos": got.kept, "kept_rows": sum(kept_rows), "runs_per_round": iters, "compact_us": spread(ours), "route_us": spread(theirs),
            "compact_over_route": statistics.median(ours) / statistics.median(theirs),
            "G1": {"route_minus_compact_us": gain, "route_max_minus_min_us": max(theirs) - min(theirs), "verdict": "HOLDS" if holds else "DOES NOT HOLD"},
            "route_bytes_equal": route_equal,
            "rows_launches": {"us": spread(rows_us), "bytes": nbytes, "TB_per_s": nbytes / (statistics.median(rows_us) * 1e-6) / 1e12,
                              "share_of_hbm_peak": nbytes / (statistics.median(rows_us) * 1e-6) / 1e12 / HBM_PEAK_TBS,
                              "note": "the K rows launches of one call, device events around each launch from Python: launch-inclusive, not "
                                      "a kernel-trace figure; set against the data sheet's %.1f TB/s" % HBM_PEAK_TBS}}


def bench_compact_buys(name, lens, emb, rounds, S=8, n=16, K=16):
    """What the compaction buys: shortlist and rank at S = 8, n = 16 on the compacted table beside the K = 16 sharded object under the
    same mask (a random 10 % dropped), every field asserted equal (ids and targets mapped through positions) before timing."""
    from drn_amd import ShardedShortlister, pack_allow
    sh = ShardedShortlister(equal_shards(emb, lens, K))
    V = len(sh)
    g = torch.Generator(device="cuda:0").manual_seed(99)
    mask = torch.rand(V, generator=g, device="cuda:0") >= 0.1
    keep = pack_allow(mask)
    done = sh.compact(keep)
    table, pos = done.table, done.positions
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    targets = torch.randint(0, V, (S,), generator=g, device="cuda:0").to(torch.int32)
    local = pos[targets.long()].contiguous()
    a, b = table.shortlist(q, n), sh.shortlist(q, n, allow=keep)
    assert torch.equal(a.ids, torch.where(b.ids >= 0, pos[b.ids.clamp(min=0).long()], b.ids)) and torch.equal(a.scores, b.scores) and torch.equal(a.n, b.n)
    same_fields(table.rank(q, local), sh.rank(q, targets, allow=keep), (name, "rank"))
    ra, rb = table.rank(q, local), sh.rank(q, targets, allow=keep)
    times, reps = interleaved_windows({
        "shortlist_compacted": lambda: table.shortlist(q, n, out=a), "shortlist_sharded": lambda: sh.shortlist(q, n, out=b, allow=keep),
        "rank_compacted": lambda: table.rank(q, local, out=ra), "rank_sharded": lambda: sh.rank(q, targets, out=rb, allow=keep)}, rounds)
    row = {"layout": name, "S": S, "n": n, "K": K, "mask": "random 10 % dropped", "kept_videos": done.kept, "launches_per_window": reps}
    for m in ("shortlist", "rank"):
        c, s = times[m + "_compacted"], times[m + "_sharded"]
        row[m] = {"compacted_us": spread(c), "sharded_masked_us": spread(s), "sharded_over_compacted": statistics.median(s) / statistics.median(c),
                  "compacted_against_sharded": verdict(c, s)}
    return row


def main_compact(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_compact_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the shards resident, every shape warmed",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds; a round = the mean of 5 runs",
                      "clock": "host clock from before the call to after a device synchronise (compact and the route); device events "
                               "around each rows launch (rows_launches); device events around windows of back-to-back calls (buys)",
                      "yardstick": "the route the parent offers: mx8_dequantize of the FP8 shards, torch.cat, index_select of the survivors, "
                                   "Shortlister(rows, offsets, quantize=target), in the same process on the same shards and mask",
                      "G1": "compact() takes less than the route, by more than the route's own max - min: HOLDS / DOES NOT HOLD per "
                            "shape; a shape where it does not hold is reported and not tuned; no absolute time is required",
                      "what_this_does_not_say": "random embeddings, bf16 queries, equal shards, E = 512 only; the route is given the mask as a "
                                                "bool tensor on the device and on the host, compact() its packed words; all-FP8 shards "
                                                "compact to FP8 by a byte copy where the route requantises (route_bytes_equal says whether "
                                                "the bytes came out equal all the same: it is not promised); no kernel-only times"},
           "compact": [], "buys": []}

    def save():
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for name, lens in SEGMENT_LAYOUTS[:2]:
        for fmt in COMPACT_FORMATS:
            for K in (4, 16):
                for mask_name in ("all_kept", "random_10pct_dropped"):
                    row = bench_compact(name, lens, emb, fmt, K, mask_name, args.rounds)
                    res["compact"].append(row)
                    print("compact %s %s K = %d %s: compact / route = %.3f, %.0f against %.0f us, (G1) %s; rows launches %.2f TB/s" % (
                        name, fmt[0], K, mask_name, row["compact_over_route"], row["compact_us"]["median"], row["route_us"]["median"],
                        row["G1"]["verdict"], row["rows_launches"]["TB_per_s"]), flush=True)
                    save()
        row = bench_compact_buys(name, lens, emb, args.rounds)
        res["buys"].append(row)
        print(json.dumps({"buys": row}), flush=True)
        save()
    print("wrote", out)


DEEP_DEPTHS = (128, 256, 512, 1024)
DEEP_LAYOUTS = (SEGMENT_LAYOUTS[0], SEGMENT_LAYOUTS[1])     # 65,536 x 1 as a plain table (no offsets), 4,096 x 16 ragged


def bench_deep_shortlist(name, lens, emb, S, rounds):
    """Shortlister.shortlist_deep on R = 65,536 rows: (a) at n = 128 beside shortlist(q, 128) on the same tensors, (b) at n = 256 / 512 /
    1024, (c) at n = 1024 beside the parent's only way to the same list under the same order -- eight rounds of shortlist(q, 128,
    allow=), each excluding the videos already listed by a device scatter into a bool mask and pack_allow -- and (d) torch.matmul (+ a
    segmented amax) + torch.topk(1024), for orientation only.  Every field is asserted equal before timing."""
    import numpy as np
    from drn_amd import Shortlister, pack_allow
    R, V = int(emb.shape[0]), len(lens)
    ragged = V != R
    off = np.concatenate([[0], np.cumsum(lens)])
    assert off[-1] == R and V >= 1024
    g = torch.Generator(device="cuda:0").manual_seed(S + 1024)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    sl = Shortlister(emb, offsets=off if ragged else None)
    kind = type(sl.shortlist(q, 1))
    out_s = kind(*sl.shortlist(q, 128))
    out_d = {n: kind(*sl.shortlist_deep(q, n)) for n in DEEP_DEPTHS}
    for f in kind._fields:
        assert torch.equal(getattr(out_d[128], f), getattr(out_s, f)), (name, S, f, "deep 128 == shortlist 128")
        for n in DEEP_DEPTHS[:-1]:
            deep, part = getattr(out_d[1024], f), getattr(out_d[n], f)
            assert torch.equal(deep[:, :n] if deep.dim() == 2 else deep.clamp(max=n), part), (name, S, n, f, "a prefix of the deep list")
    mask = torch.ones((S, V), dtype=torch.bool, device="cuda:0")
    words = pack_allow(mask)
    out_r = [kind(*sl.shortlist(q, 128, allow=words)) for _ in range(8)]

    def rounds8():
        mask.fill_(True)
        for r in range(8):
            pack_allow(mask, out=words)
            sl.shortlist(q, 128, out=out_r[r], allow=words)
            if r < 7:
                mask.scatter_(1, out_r[r].ids.long(), False)                  # (every list is full: V >= 1024 finite scores, asserted below)
    rounds8()
    assert bool((out_d[1024].n == 1024).all()) and all(bool((o.n == 128).all()) for o in out_r)
    for f in kind._fields:
        if f != "n":
            assert torch.equal(torch.cat([getattr(o, f) for o in out_r], dim=1), getattr(out_d[1024], f)), (name, S, f, "eight rounds == deep 1024")
    variants = {"shortlist_128": lambda: sl.shortlist(q, 128, out=out_s), "rounds8_1024": rounds8}
    for n in DEEP_DEPTHS:
        variants["deep_%d" % n] = lambda n=n: sl.shortlist_deep(q, n, out=out_d[n])
    if ragged:
        index = torch.repeat_interleave(torch.arange(V, device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(S, R).contiguous()
        best = torch.empty((S, V), dtype=torch.bfloat16, device="cuda:0")

        def torch_way():
            best.fill_(float("-inf"))
            best.scatter_reduce_(1, index, torch.matmul(q, emb.t()), "amax")
            return torch.topk(best, 1024, dim=1)
    else:
        torch_way = lambda: torch.topk(torch.matmul(q, emb.t()), 1024, dim=1)
    variants["torch_1024"] = torch_way
    times, reps = interleaved_windows(variants, rounds)
    med = {k: statistics.median(ts) for k, ts in times.items()}
    c, d = times["rounds8_1024"], times["deep_1024"]
    over = med["deep_1024"] - med["rounds8_1024"]
    table = emb.numel() * emb.element_size()
    row = {"layout": name, "R": R, "V": V, "E": 512, "S": S, "dtype": "bf16", "blocks": sl._nblocks(), "launches_per_window": reps,
           "table_once_us_at_8.0TB/s": table / HBM_PEAK_BYTES_PER_S * 1e6,
           "a": {"shortlist_128_us": spread(times["shortlist_128"]), "deep_128_us": spread(times["deep_128"]),
                 "deep_128_over_shortlist_128": med["deep_128"] / med["shortlist_128"],
                 "deep_128_against_shortlist_128": verdict(times["deep_128"], times["shortlist_128"])},
           "b": {"deep_%d_us" % n: spread(times["deep_%d" % n]) for n in DEEP_DEPTHS[1:]},
           "c": {"eight_rounds_us": spread(c), "deep_1024_over_eight_rounds": med["deep_1024"] / med["rounds8_1024"],
                 "deep_1024_minus_eight_rounds_us": over, "eight_rounds_max_minus_min_us": max(c) - min(c), "holds": over <= max(c) - min(c),
                 "deep_1024_against_eight_rounds": verdict(d, c)},
           "d": {"matmul_topk_1024_us": spread(times["torch_1024"]), "deep_1024_over_matmul_topk": med["deep_1024"] / med["torch_1024"],
                 "deep_1024_against_matmul_topk": verdict(d, times["torch_1024"])},
           "note": "launch-inclusive, every launch of a call: two (three on the ragged layout) for shortlist and shortlist_deep; the eight "
                   "rounds are a fill, eight pack_allow, eight masked shortlists and seven scatters; torch scores in bf16 with no defined tie "
                   "order: another answer, for orientation"}
    return row


def main_deep_shortlist(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_deep_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the table resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "baselines": "(a) shortlist(q, 128) on the same tensors; (c) eight rounds of shortlist(q, 128, allow=), each excluding "
                                   "the videos already listed (device scatter into a bool mask + pack_allow), the concatenation asserted equal "
                                   "to shortlist_deep(q, 1024) field for field before timing; (d) torch.matmul + torch.topk(1024).  A "
                                   "difference inside the baseline's own max - min is NO DIFFERENCE",
                      "condition": "derived, not measured: (c) reads the table eight times and runs eight merges and eight packs, so "
                                   "shortlist_deep at n = 1024 may not take longer than (c) beyond (c)'s max - min.  No number gates the change",
                      "what_this_does_not_say": "random embeddings: nothing here says anything about recall, or about what depth a coarse stage "
                                                "needs; bf16 only: no fp32, no FP8 tables, no masks; no kernel-only times (no profiler run); "
                                                "the two-level merge is not built, so nothing says what it would save at S = 1"},
           "deep_shortlist": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for S in (1, 8, 64):
        for name, lens in DEEP_LAYOUTS:
            row = bench_deep_shortlist(name, lens, emb, S, args.rounds)
            res["deep_shortlist"].append(row)
            print(json.dumps({"deep_shortlist": row}), flush=True)
            print("(a) %s S = %d: deep 128 / shortlist 128 = %.3f (%s)" % (name, S, row["a"]["deep_128_over_shortlist_128"],
                                                                         row["a"]["deep_128_against_shortlist_128"]), flush=True)
            print("(c) %s S = %d: %s (deep 1024 / eight rounds = %.3f)" % (name, S, "HOLDS" if row["c"]["holds"] else "MISSED",
                                                                          row["c"]["deep_1024_over_eight_rounds"]), flush=True)
            print("(d) %s S = %d: deep 1024 / matmul + topk = %.3f (%s)" % (name, S, row["d"]["deep_1024_over_matmul_topk"],
                                                                          row["d"]["deep_1024_against_matmul_topk"]), flush=True)
            json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


POOLED_LAYOUTS = (SEGMENT_LAYOUTS[1], ("5120x(1,3,0,17,43)", [1, 3, 0, 17, 43] * 1024))     # R = 65,536 each: 4,096 x 16, and an unequal one


def pooled_route(sl, index, counts, rows_out, out_off):
    """The way to a pooled table WITHOUT pooled(), in torch on the device: (dequantise,) an fp32 index_add_ -- whose add order nobody
    states --, a divide, a cast, and a fresh Shortlister, whose constructor reads the result again for finiteness (its host round
    trip) and quantises it when the source was FP8.  index (the pooled row of every source row) and counts are made outside the clock."""
    from drn_amd import Shortlister
    from drn_amd.index import mx8_dequantize
    rows = sl.embeddings if sl.quantize is None else mx8_dequantize(sl.codes, sl.scales, sl.dtype)
    acc = torch.zeros((rows_out, rows.shape[1]), dtype=torch.float32, device=rows.device).index_add_(0, index, rows.float())
    return Shortlister((acc / counts[:, None]).to(rows.dtype), offsets=out_off, quantize=sl.quantize)


def bench_pooled(name, lens, emb, fp8, group, rounds, iters=5):
    """Shortlister.pooled(how="mean", group=group) beside pooled_route on the same table: host clock from before the call to after a
    device synchronise (both synchronise by design), the two taking turns inside every round, a round = the mean of `iters` runs.
    Before timing every field of the result is asserted equal to pool_segments_reference, evaluated on the host."""
    import numpy as np
    from drn_amd import Shortlister, pool_offsets, pool_segments_reference
    from drn_amd.index import mx8_quantize
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R, V = int(off[-1]), len(lens)
    assert R == int(emb.shape[0])
    sl = Shortlister(emb, offsets=off, quantize="mxfp8" if fp8 else None)
    got, want = sl.pooled(group=group), pool_segments_reference(sl, how="mean", group=group)
    if fp8:
        codes, scales = mx8_quantize(want.rows)
        assert torch.equal(got.codes.cpu(), codes) and torch.equal(got.scales.cpu(), scales), (name, fp8, group)
    else:
        assert torch.equal(got.embeddings.cpu().view(torch.int16), want.rows.view(torch.int16)), (name, fp8, group)
    assert (got._seg is None) == (want.offsets is None) and (group is None or got.offsets.cpu().tolist() == want.offsets.tolist())
    out_off = pool_offsets(off, group)
    rows_out = V if group is None else int(out_off[-1])
    per = np.asarray(lens) if group is None else None
    if group is None:
        index, counts = np.repeat(np.arange(V), per), np.maximum(per, 1)
    else:
        within = np.arange(R) - np.repeat(off[:-1], lens)
        index = np.repeat(out_off[:-1], lens) + within // group
        counts = np.bincount(index, minlength=rows_out)
    index, counts = torch.from_numpy(index).to("cuda:0"), torch.from_numpy(counts).to("cuda:0", torch.float32)
    route = pooled_route(sl, index, counts, rows_out, out_off)
    tensors = lambda t: (t.embeddings,) if t.quantize is None else (t.codes, t.scales)
    route_equal = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(tensors(got), tensors(route)))
    del want, route

    def timed(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6
    ours, theirs = [], []
    for _ in range(rounds):
        ours.append(statistics.mean(timed(lambda: sl.pooled(group=group)) for _ in range(iters)))
        theirs.append(statistics.mean(timed(lambda: pooled_route(sl, index, counts, rows_out, out_off)) for _ in range(iters)))
    over = statistics.median(ours) - statistics.median(theirs)
    row_bytes = 528 if fp8 else 1024
    nbytes = R * row_bytes + 4 * (V + 1) * (1 if group is None else 2) + rows_out * (1024 + (1024 + 528 if fp8 else 0))
    return {"layout": name, "R": R, "V": V, "E": 512, "source": "mxfp8" if fp8 else "bf16", "target": "same", "how": "mean",
            "group": group, "pooled_rows": rows_out, "runs_per_round": iters, "pooled_us": spread(ours), "route_us": spread(theirs),
            "pooled_over_route": statistics.median(ours) / statistics.median(theirs),
            "condition": {"pooled_minus_route_us": over, "route_max_minus_min_us": max(theirs) - min(theirs),
                          "verdict": "HOLDS" if over <= max(theirs) - min(theirs) else "DOES NOT HOLD"},
            "route_bytes_equal": route_equal,
            "bytes": {"read_and_written": nbytes, "us_at_8.0TB/s": nbytes / HBM_PEAK_BYTES_PER_S * 1e6,
                      "note": "for orientation only: every source row once in its format, the offsets, every pooled row written in bf16 "
                              "and, for an FP8 result, read again by the quantiser and written as codes and scales"}}


def main_pooled(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_pooled_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the table resident, every shape warmed",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds; a round = the mean of 5 runs",
                      "clock": "host clock from before the call to after a device synchronise: launch-inclusive us per call, the "
                               "synchronise of pooled() and of the route's constructor included",
                      "yardstick": "the parent's only way to a pooled table, in torch on the device: (mx8_dequantize of an FP8 table,) an "
                                   "fp32 index_add_, a divide, a cast and Shortlister(rows, offsets, quantize=) -- in the same rounds, on "
                                   "the same table; its index and counts are made outside the clock",
                      "condition": "derived, not measured: pooled() reads the table once and writes the pooled rows once, the route "
                                   "writes and reads an fp32 copy besides, so pooled() may not take longer than the route beyond the "
                                   "route's own max - min: HOLDS / DOES NOT HOLD per shape; no absolute time is required",
                      "what_this_does_not_say": "no kernel-only time (no profiler run); bf16 only, no fp32; no long runs on few videos, "
                                                "where one wavefront a pooled row fills little of the chip; how=\"mean\" only; random "
                                                "embeddings: nothing here says anything about recall of a pooled table"},
           "pooled": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for name, lens in POOLED_LAYOUTS:
        for fp8 in (False, True):
            for group in (None, 4):
                row = bench_pooled(name, lens, emb, fp8, group, args.rounds)
                res["pooled"].append(row)
                print("pooled %s %s group = %s: pooled / route = %.3f, %.0f against %.0f us, condition %s" % (
                    name, row["source"], group, row["pooled_over_route"], row["pooled_us"]["median"], row["route_us"]["median"],
                    row["condition"]["verdict"]), flush=True)
                with open(out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
    print("wrote", out)


def bench_fused_shortlist(emb, S, rounds, n=16):
    """(a) Shortlister.scores beside shortlist(q, n) on the same table, plain (65,536 x 1) and ragged (4,096 x 16); (b)
    FusedShortlister.shortlist at M = 2 -- the 4,096 x 16 ragged table and its pooled table over the same 4,096 videos -- beside what a
    caller can do without it: torch.matmul per table, scatter_reduce_(amax), the weighted sum, torch.topk.  The fused list is asserted
    equal to fused_shortlist_reference of the tables' own scores() before timing."""
    import numpy as np
    from drn_amd import FusedShortlister, Shortlister, fused_shortlist_reference
    R = int(emb.shape[0])
    g = torch.Generator(device="cuda:0").manual_seed(S + 4096)
    q = torch.randn(S, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    rows = []
    tables = {}
    for name, lens in (SEGMENT_LAYOUTS[0], SEGMENT_LAYOUTS[1]):
        V = len(lens)
        sl = Shortlister(emb, offsets=np.concatenate([[0], np.cumsum(lens)]) if V != R else None)
        tables[name] = sl
        out_l = type(sl.shortlist(q, 1))(*sl.shortlist(q, n))
        out_s = sl.scores(q)
        assert torch.equal(torch.gather(out_s, 1, out_l.ids.long()).view(torch.int32), out_l.scores.view(torch.int32)), (name, S)
        times, reps = interleaved_windows({"shortlist": lambda: sl.shortlist(q, n, out=out_l), "scores": lambda: sl.scores(q, out=out_s)}, rounds)
        base, new = times["shortlist"], times["scores"]
        over = statistics.median(new) - statistics.median(base)
        rows.append({"report": "a", "layout": name, "R": R, "V": V, "E": 512, "S": S, "n": n, "dtype": "bf16", "launches_per_window": reps,
                     "shortlist_us": spread(base), "scores_us": spread(new), "scores_bytes_written": 4 * S * V,
                     "scores_over_shortlist": statistics.median(new) / statistics.median(base), "scores_minus_shortlist_us": over,
                     "shortlist_max_minus_min_us": max(base) - min(base), "holds": over <= max(base) - min(base),
                     "scores_against_shortlist": verdict(new, base)})
    fine = tables[SEGMENT_LAYOUTS[1][0]]
    coarse = fine.pooled()
    V, lens = len(fine), SEGMENT_LAYOUTS[1][1]
    w = [1.0, 0.5]
    fused = FusedShortlister([fine, coarse], weights=w)
    out_f = fused.shortlist([q, q], n)
    want = fused_shortlist_reference(torch.stack([fine.scores(q), coarse.scores(q)]), w, n)
    for f in ("ids", "scores", "n"):
        assert torch.equal(getattr(out_f, f), getattr(want, f)), (S, f, "the fused list is the definition's")
    index = torch.repeat_interleave(torch.arange(V, device="cuda:0"), torch.as_tensor(lens, device="cuda:0"))[None].expand(S, R).contiguous()
    best = torch.empty((S, V), dtype=torch.bfloat16, device="cuda:0")
    pooled = coarse.embeddings

    def torch_way():
        best.fill_(float("-inf"))
        best.scatter_reduce_(1, index, torch.matmul(q, emb.t()), "amax")
        return torch.topk(w[0] * best + w[1] * torch.matmul(q, pooled.t()), n, dim=1)
    times, reps = interleaved_windows({"fused": lambda: fused.shortlist([q, q], n, out=out_f), "torch": torch_way}, rounds)
    rows.append({"report": "b", "tables": "4096x16 ragged bf16 + its pooled 4096x1 bf16", "M": 2, "V": V, "E": 512, "S": S, "n": n,
                 "launches_per_window": reps, "fused_us": spread(times["fused"]), "matmul_amax_sum_topk_us": spread(times["torch"]),
                 "fused_over_torch": statistics.median(times["fused"]) / statistics.median(times["torch"]),
                 "fused_against_torch": verdict(times["fused"], times["torch"]),
                 "note": "the fused call is two score launches and the two launches of drn_shortlist_fuse_topn; torch scores in bf16, sums "
                         "in bf16 and has no defined tie order: another answer, for orientation"})
    return rows


def main_fused_shortlist(args):
    out = args.out or os.path.join(ROOT, "profiles", "search_fused_shortlist_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, the tables resident",
           "method": {"interleaved": True, "statistic": "median [min, max] over rounds of the mean time of a window of ~0.2 s",
                      "clock": "device events around windows of back-to-back calls issued from Python: launch-inclusive us per call",
                      "condition": "derived, not measured: scores() does the reads and the MFMA chain of shortlist() and writes 4 * S * V bytes "
                                   "where the other sorts and merges, so (a) scores() may not take longer than shortlist(q, 16) on the same "
                                   "table beyond that launch's own max - min.  No number gates the change; a miss is a finding",
                      "what_this_does_not_say": "random embeddings say nothing about recall; bf16 only: no fp32, no FP8 tables, no masks, no "
                                                "late interaction; no kernel-only times (no profiler run)"},
           "fused_shortlist": []}
    g = torch.Generator(device="cuda:0").manual_seed(65536)
    emb = torch.randn(65536, 512, generator=g, device="cuda:0").to(torch.bfloat16).contiguous()
    for S in (1, 8, 64):
        for row in bench_fused_shortlist(emb, S, args.rounds):
            res["fused_shortlist"].append(row)
            print(json.dumps({"fused_shortlist": row}), flush=True)
            if row["report"] == "a":
                print("(a) %s S = %d: %s (scores / shortlist = %.3f, %s)" % (row["layout"], S, "HOLDS" if row["holds"] else "MISSED",
                                                                           row["scores_over_shortlist"], row["scores_against_shortlist"]), flush=True)
            else:
                print("(b) S = %d: fused / matmul + amax + sum + topk = %.3f (%s)" % (S, row["fused_over_torch"], row["fused_against_torch"]),
                      flush=True)
        json.dump(res, open(out, "w"), indent=1)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/search_bench.json (search_pairs_bench.json with --shortlist, search_eval_bench.json with --evaluate, "
                                            "search_q8_bench.json with --quantized, search_q8_shortlist_bench.json with --quantized-shortlist, "
                                            "search_filtered_shortlist_bench.json with --filtered-shortlist, search_late_shortlist_bench.json with "
                                            "--late-shortlist, search_rank_bench.json with --rank, search_rerank_bench.json with --rerank, "
                                            "search_sharded_shortlist_bench.json with --sharded-shortlist, search_sharded_rank_bench.json with "
                                            "--sharded-rank, search_compact_bench.json with --compact)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shortlist", action="store_true", help="measure Grounder.search(candidates=) beside the cartesian search")
    ap.add_argument("--evaluate", action="store_true", help="measure evaluate_search beside scoring Hits.tolist() on the host")
    ap.add_argument("--quantized", action="store_true", help="measure a SearchIndex built with quantize=\"mxfp8\" beside the plain index")
    ap.add_argument("--mx-conv0", action="store_true", help="measure Grounder(conv0=\"mxfp8\") beside the default path on one quantised index")
    ap.add_argument("--mx-conv0-fused", action="store_true", help="measure Grounder(conv0=\"mxfp8\", fused=True) beside the unfused mode and "
                                                                  "the default fused path on one quantised index")
    ap.add_argument("--mx-conv0-tiles", action="store_true", help="measure the narrow tiles of the fused FP8 conv0 and the chooser beside the "
                                                                  "wide tile and the default fused path on one quantised index")
    ap.add_argument("--device-candidates", action="store_true", help="measure Shortlister.shortlist + Grounder.search(candidates= a device "
                                                                     "tensor) beside the shortlist read back as host lists")
    ap.add_argument("--segment-shortlist", action="store_true", help="measure Shortlister(offsets=).shortlist on 65,536 rows in three layouts "
                                                                     "beside the plain kernel on the same rows and matmul + amax + topk")
    ap.add_argument("--quantized-shortlist", action="store_true", help="measure Shortlister(quantize=\"mxfp8\").shortlist on 65,536 rows in three "
                                                                       "layouts beside the plain table over the same dequantised rows")
    ap.add_argument("--filtered-shortlist", action="store_true", help="measure Shortlister.shortlist(allow=) under five masks beside the unmasked "
                                                                      "launch and the sub-table way")
    ap.add_argument("--late-shortlist", action="store_true", help="measure Shortlister.shortlist_late at four token shapes beside shortlist() on "
                                                                  "the flattened tokens and matmul + amax + sum + topk")
    ap.add_argument("--rank", action="store_true", help="measure Shortlister.rank / rank_late beside the shortlist of n = 16 and matmul + "
                                                        "comparisons + sums, and evaluate_shortlist on planted queries, plain and FP8")
    ap.add_argument("--rerank", action="store_true", help="measure Shortlister.rerank_late / rerank on 128 and 32 candidates a sentence beside "
                                                          "pack_allow + the masked full shortlists and the unmasked late shortlist")
    ap.add_argument("--sharded-shortlist", action="store_true", help="measure ShardedShortlister.shortlist on 1 / 4 / 16 equal shards beside the "
                                                                     "single table, the merge launch alone, a mixed FP8 / bf16 object, "
                                                                     "shortlist_late, and append beside torch.cat + rebuild")
    ap.add_argument("--sharded-rank", action="store_true", help="measure ShardedShortlister.rank, rank_late and rerank on 1 / 4 / 16 equal shards "
                                                                "beside the single table, and append + rank beside torch.cat + rebuild + rank")
    ap.add_argument("--compact", action="store_true", help="measure ShardedShortlister.compact beside dequantise + torch.cat + index_select + "
                                                           "Shortlister on the same shards, the rows launches' bytes per second, and "
                                                           "what the compacted table buys against K = 16 shards under the same mask")
    ap.add_argument("--deep-shortlist", action="store_true", help="measure Shortlister.shortlist_deep at n = 128 / 256 / 512 / 1024 beside "
                                                                  "shortlist() at 128, eight masked rounds of it and matmul + topk "
                                                                  "(writes profiles/search_deep_shortlist_bench.json)")
    ap.add_argument("--pooled", action="store_true", help="measure Shortlister.pooled (mean, one row a video and one per 4 rows, bf16 and FP8 "
                                                          "sources) beside index_add_ + divide + cast + Shortlister in torch "
                                                          "(writes profiles/search_pooled_bench.json)")
    ap.add_argument("--fused-shortlist", action="store_true", help="measure Shortlister.scores beside shortlist(q, 16), and "
                                                                   "FusedShortlister.shortlist over a ragged table and its pooled table beside "
                                                                   "matmul + amax + weighted sum + topk in torch "
                                                                   "(writes profiles/search_fused_shortlist_bench.json)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_search.py measures on an MI355X; no GPU found")
    if args.fused_shortlist:
        return main_fused_shortlist(args)
    if args.pooled:
        return main_pooled(args)
    if args.deep_shortlist:
        return main_deep_shortlist(args)
    if args.compact:
        return main_compact(args)
    if args.sharded_rank:
        return main_sharded_rank(args)
    if args.sharded_shortlist:
        return main_sharded_shortlist(args)
    if args.rerank:
        return main_rerank(args)
    if args.rank:
        return main_rank(args)
    if args.late_shortlist:
        return main_late_shortlist(args)
    if args.filtered_shortlist:
        return main_filtered_shortlist(args)
    if args.quantized_shortlist:
        return main_q8_shortlist(args)
    if args.segment_shortlist:
        return main_segment_shortlist(args)
    if args.device_candidates:
        return main_device_candidates(args)
    if args.shortlist:
        return main_shortlist(args)
    if args.evaluate:
        return main_evaluate(args)
    if args.quantized:
        return main_quantized(args)
    if args.mx_conv0:
        return main_mx_conv0(args)
    if args.mx_conv0_fused:
        return main_mx_conv0_fused(args)
    if args.mx_conv0_tiles:
        return main_mx_conv0_tiles(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "search_bench.json")
    from bench_store import build_store
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on": "MI355X, one process, store and index resident",
           "store": {"videos": NV, "rows_per_video": 120, "dim": D, "dtype": "bf16"},
           "method": {"interleaved": True, "statistic": "median over rounds of the mean time of a window of ~0.3 s",
                      "clock": "host clock around searches ending in a device synchronise; device events for the kernel windows"},
           "build": [], "search": [], "kernel": []}
    model = make_model()
    for T in (256, 32):
        store = build_store(T, torch.bfloat16, "cuda:0")
        index, b = bench_build(model, store, args.rounds)
        res["build"].append(dict(b, T=T))
        print(json.dumps({"build": res["build"][-1]}), flush=True)
        for S in (1, 8):
            res["search"].append(bench_search(model, store, index, T, S, args.rounds))
            print(json.dumps({"search": res["search"][-1]}), flush=True)
            json.dump(res, open(args.out, "w"), indent=1)
        for Q in (512, 64):
            res["kernel"].append(bench_kernel(index, T, Q, args.rounds))
            print(json.dumps({"kernel": res["kernel"][-1]}), flush=True)
        json.dump(res, open(args.out, "w"), indent=1)
        del store, index
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
