// Rank and rerank over a corpus kept as several tables (drn_amd/retrieve.py, ShardedShortlister.rank / rank_late / rerank /
// rerank_late): the three small launches that stand between the shards' own kernels.
//   drn_shard_positions               corpus positions -> each shard's local positions (-1 outside the shard), one launch;
//   drn_shortlist_rank_thresholds     the K shards' target keys -> the K shards' counting thresholds and the target's key, one launch;
//   drn_shortlist_rank_reduce_shards  the K shards' block counts -> rank, score, total, one launch.
// (The kernels live here and not in retrieve_shard.hip / retrieve_rank.hip, whose kernel lists are pinned by their resource tests.)
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// WHY THE RANK IS EXACT.  A key is sl_key(score, position) = (sl_word(score) << 32) | ~position and "precedes" is key > the target's
// key.  A score's bits do not depend on the table that holds the video (retrieve.hip), so shard k's kernels make, for the video at
// its position i, the key of the corpus's video bases[k] + i except for the position bits.  Let the target lie in shard kt with the
// LOCAL key tk (the phase-1 launch of retrieve_rank.hip on the local position, -1 in every other shard: key 0 there), tw = tk >> 32
// its score's word; a finite score's word is never 0, so tw >= 1.  Inside shard k:
//   k == kt: local order is corpus order inside a shard: a video precedes iff key > tk;
//   k <  kt: every equal score lies at a lower corpus position: a video precedes iff its word >= tw, i.e. key > (tw << 32) - 1
//            (the keys of the word tw - 1 end at (tw << 32) - 1, those of tw start at tw << 32);
//   k >  kt: every equal score lies at a higher corpus position: it precedes iff its word > tw, i.e. key > (tw << 32) | 0xffffffff.
// So the phase-2 launch of retrieve_rank.hip, handed thr[k][s] in the place of tkey[s], counts exactly the corpus's videos of shard k
// that precede the target; the counts are integers, the target is counted nowhere (its own key equals thr[kt][s]), total is the sum of
// the shards' totals and the score is sl_score(tk).  Where no shard holds a candidate target every key is 0: the thresholds are all
// ones, nothing counts as above, rank = -1, score = 0, and total is still counted.
// No atomics, no workspace beyond what is passed, nothing read on the host.

// positions [S][C] -> out [K][S][C]: out[k] = positions - bases[k] where bases[k] <= positions < bases[k + 1], else -1.  One thread per
// output word, bases in LDS, each clamped at 0; compared and subtracted in 64 bits, so INT_MIN and INT_MAX land in no shard.
__global__ __launch_bounds__(256) void shard_positions_kernel(const int* __restrict__ positions, const int* __restrict__ bases_g, const int K,
                                                              const long per, int* __restrict__ out) {
  __shared__ int bases[DRN_SHARDS_MAX + 1];
  const int tid = threadIdx.x;
  for (int i = tid; i <= K; i += 256) bases[i] = max(bases_g[i], 0);
  __syncthreads();
  const long at = (long)blockIdx.x * 256 + tid;
  if (at >= K * per) return;
  const int k = (int)(at / per);
  const long p = positions[at - k * per], lo = bases[k], hi = bases[k + 1];
  out[at] = (p >= lo && p < hi) ? (int)(p - lo) : -1;
}

// keys [K][S] -> thr [K][S], key [S].  One wavefront per sentence, lane = shard (K <= DRN_SHARDS_MAX = 64 lanes): a ballot finds the
// shards whose key is not 0 and the LOWEST wins, should two claim the target; its key travels by one shuffle.
static_assert(DRN_SHARDS_MAX <= 64, "one lane per shard");
__global__ __launch_bounds__(256) void rank_thresholds_kernel(const sl_key_t* __restrict__ keys, const int K, const int S,
                                                              sl_key_t* __restrict__ thr, sl_key_t* __restrict__ key) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;                                         // (wave-uniform)
  const sl_key_t mine = lane < K ? keys[(long)lane * S + s] : 0ull;
  const unsigned long long has = __ballot(mine != 0ull);
  const int kt = has != 0ull ? __ffsll(has) - 1 : -1;
  const sl_key_t tk = __shfl(mine, max(kt, 0), 64), top = (tk >> 32) << 32;
  const sl_key_t t = kt < 0 ? ~0ull : lane < kt ? top - 1ull : lane == kt ? tk : top | 0xffffffffull;
  if (lane < K) thr[(long)lane * S + s] = t;
  if (lane == 0) key[s] = kt < 0 ? 0ull : tk;
}

// The reduce of retrieve_rank.hip over K count regions back to back: region k is cnt_k [S][nb_k] pairs from pair S * blk_off[k], nb_k =
// blk_off[k + 1] - blk_off[k]; nb = blk_off[K] as the host knows it.  One wavefront per sentence walks the nb blocks of the corpus; a
// block's shard is found by bisection of blk_off in LDS.  Every value of blk_off is clamped into [0, nb] and a region's end to its
// start at least, so whatever the device's table holds the pair read lies at S lo + s (hi - lo) + (j - lo) < S hi <= S nb.
__global__ __launch_bounds__(256) void rank_reduce_shards_kernel(const sl_key_t* __restrict__ key, const int2* __restrict__ cnt,
                                                                 const int* __restrict__ blk_off, const int K, const int S, const int nb,
                                                                 int* __restrict__ rank, float* __restrict__ score,
                                                                 int* __restrict__ total) {
  __shared__ int off[DRN_SHARDS_MAX + 1];
  for (int i = threadIdx.x; i <= K; i += 256) off[i] = min(max(blk_off[i], 0), nb);
  __syncthreads();
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;                                         // (wave-uniform)
  int above = 0, any = 0;
  for (int j = lane; j < nb; j += 64) {
    int k = 0;
    for (int step = 32; step > 0; step >>= 1)                 // the last region that starts at or before block j (K <= 64)
      if (k + step < K && off[k + step] <= j) k += step;
    const int lo = off[k], hi = max(off[k + 1], lo);
    if (j >= lo && j < hi) {
      const int2 c = cnt[(long)S * lo + (long)s * (hi - lo) + (j - lo)];
      above += c.x;
      any += c.y;
    }
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    above += __shfl_xor(above, w, 64);
    any += __shfl_xor(any, w, 64);
  }
  if (lane == 0) {
    const sl_key_t k = key[s];
    rank[s] = k != 0ull ? above : -1;
    score[s] = k != 0ull ? sl_score(k) : 0.f;
    total[s] = any;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The entries: every check answers before anything is launched.

extern "C" int drn_shard_positions(const int32_t* positions, const int32_t* bases, int K, int S, int C, int32_t* out, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(positions && bases && out, "drn_shard_positions: null pointer");
  DRN_CHECK_ARG(K >= 1 && K <= DRN_SHARDS_MAX, "drn_shard_positions: K = %d shards outside [1, %d]", K, DRN_SHARDS_MAX);
  DRN_CHECK_ARG(S >= 1, "drn_shard_positions: bad args (S = %d sentences)", S);
  DRN_CHECK_ARG(C >= 1 && C <= DRN_RERANK_MAX_CANDIDATES, "drn_shard_positions: C = %d positions a sentence outside [1, %d]", C,
                DRN_RERANK_MAX_CANDIDATES);
  DRN_CHECK_ARG((((uintptr_t)positions | (uintptr_t)bases | (uintptr_t)out) & 3) == 0, "drn_shard_positions: every buffer must be 4-byte aligned");
  const long per = (long)S * C, elems = per * K;
  DRN_CHECK_ARG(elems <= 0x7fffffffL, "drn_shard_positions: %d shards of %d x %d positions are more than 2^31 words", K, S, C);
  shard_positions_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, (hipStream_t)stream>>>(positions, bases, K, per, out);
  return drn_launch_status("drn_shard_positions");
}

extern "C" int drn_shortlist_rank_thresholds(const void* keys, int K, int S, void* thresholds, void* key, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(keys && thresholds && key, "drn_shortlist_rank_thresholds: null pointer");
  DRN_CHECK_ARG(K >= 1 && K <= DRN_SHARDS_MAX, "drn_shortlist_rank_thresholds: K = %d shards outside [1, %d]", K, DRN_SHARDS_MAX);
  DRN_CHECK_ARG(S >= 1 && (long)K * S <= 0x7fffffffL / 8, "drn_shortlist_rank_thresholds: bad args (S = %d sentences)", S);
  DRN_CHECK_ARG((((uintptr_t)keys | (uintptr_t)thresholds | (uintptr_t)key) & 7) == 0,
                "drn_shortlist_rank_thresholds: every buffer must be 8-byte aligned");
  rank_thresholds_kernel<<<cdiv(S, 4), 256, 0, (hipStream_t)stream>>>((const sl_key_t*)keys, K, S, (sl_key_t*)thresholds, (sl_key_t*)key);
  return drn_launch_status("drn_shortlist_rank_thresholds");
}

extern "C" int drn_shortlist_rank_reduce_shards(const void* key, const void* cnt, int cnt_bytes, const int32_t* blk_off, int K, int S,
                                                int blocks, int32_t* rank, float* score, int32_t* total, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(key && cnt && blk_off && rank && score && total, "drn_shortlist_rank_reduce_shards: null pointer");
  DRN_CHECK_ARG(K >= 1 && K <= DRN_SHARDS_MAX, "drn_shortlist_rank_reduce_shards: K = %d shards outside [1, %d]", K, DRN_SHARDS_MAX);
  DRN_CHECK_ARG(S >= 1, "drn_shortlist_rank_reduce_shards: bad args (S = %d sentences)", S);
  DRN_CHECK_ARG(blocks >= K, "drn_shortlist_rank_reduce_shards: %d blocks for K = %d shards of one block at least", blocks, K);
  DRN_CHECK_ARG((((uintptr_t)key | (uintptr_t)cnt) & 7) == 0, "drn_shortlist_rank_reduce_shards: the key and the counts must be 8-byte aligned");
  DRN_CHECK_ARG((((uintptr_t)blk_off | (uintptr_t)rank | (uintptr_t)score | (uintptr_t)total) & 3) == 0,
                "drn_shortlist_rank_reduce_shards: blk_off and the results must be 4-byte aligned");
  const long need = 8L * S * blocks;
  DRN_CHECK_ARG(need <= 0x7fffffffL && cnt_bytes >= need, "drn_shortlist_rank_reduce_shards: the counts hold %d bytes, %ld are needed (8 * S * blocks)",
                cnt_bytes, need);
  rank_reduce_shards_kernel<<<cdiv(S, 4), 256, 0, (hipStream_t)stream>>>((const sl_key_t*)key, (const int2*)cnt, blk_off, K, S, blocks, rank,
                                                                         score, total);
  return drn_launch_status("drn_shortlist_rank_reduce_shards");
}
