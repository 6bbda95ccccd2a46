// A corpus kept as several tables (drn_amd/retrieve.py, ShardedShortlister): every shard ranks itself with its own entry, unchanged, and
//   drn_shortlist_merge_lists   merges the K per-shard lists of each sentence into the list of the whole corpus, one launch;
//   drn_allow_slices            cuts a packed allow mask over the whole corpus into the K shards' own packed masks, one launch.
// (Rank and rerank over the shards -- local positions, counting thresholds, the sum of the shards' counts -- are retrieve_shard_rank.hip.)
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// WHY THE MERGE IS EXACT.  A score's bits depend on the sentence and the video's rows alone (retrieve.hip), so shard k gives video v
// of the corpus -- its position bases[k] + id -- the score the whole table would; and every list is cut under one total order, score
// descending then position ascending, which adding a shard's base to its positions preserves inside the shard and which the key
// sl_key(score, bases[k] + id) states across shards.  The best n of a set are among the best n of each of its parts, so the best n of
// the K lists ARE the whole table's list, bit for bit.
//
// One wavefront per sentence, as shortlist_merge_kernel: entry (k, i) is rebuilt as a key in registers -- 0, "no candidate", unless
// i < min(counts[k], n_in), 0 <= id < bases[k + 1] - bases[k] and the score is finite, so an id out of range never becomes a position --
// ML_PRE lists in flight, two entries a lane; the keys above the current n-th best are compacted (a ballot and the count of the lanes
// below) into the staging half of the 2 * SL_MAX_N LDS buffer, which is folded by sl_sort_desc whenever it would overflow and at the
// end.  The shipped entries write sorted lists, where those keys are a prefix; the compaction does not need that, and no list is
// read past n_in.
//
// rows (the ragged shards' winning segments) do not ride through the sort.  After it the wavefront walks the lists once more: an
// entry belongs to the answer iff its key is not 0 and not below the n-th best, its place is found by bisection of the sorted keys
// in LDS (they are distinct), and its row is copied there.  Only the instantiation with rows pays for the second walk.
// No atomics, no workspace, no scratch.
#define SL_MAX_N DRN_SHORTLIST_MAX
#define ML_PRE 8            // lists the merge keeps in flight

struct MlLists {
  const int* ids;             // [K][S][n_in]
  const float* scores;        // [K][S][n_in]
  const int* counts;          // [K][S]
  const int* rows;            // [K][S][n_in] or null
};

// the keys of the entries `lane` and `lane + 64` of sentence s's list k; every load is independent of the others
__device__ __forceinline__ void ml_keys(const MlLists& in, const int* bases, const int k, const int S, const int s, const int n_in,
                                        const int lane, sl_key_t& k0, sl_key_t& k1) {
  const long at = ((long)k * S + s) * n_in;
  const bool h0 = lane < n_in, h1 = lane + 64 < n_in;
  const int id0 = h0 ? in.ids[at + lane] : -1, id1 = h1 ? in.ids[at + lane + 64] : -1;
  const float s0 = h0 ? in.scores[at + lane] : 0.f, s1 = h1 ? in.scores[at + lane + 64] : 0.f;
  const int cnt = in.counts[(long)k * S + s];
  const int base = bases[k], len = bases[k + 1] - base;
  k0 = (lane < cnt && id0 >= 0 && id0 < len) ? sl_key(s0, base + id0) : 0ull;
  k1 = (lane + 64 < cnt && id1 >= 0 && id1 < len) ? sl_key(s1, base + id1) : 0ull;
}

template <bool ROWS>
__global__ __launch_bounds__(64) void shortlist_merge_lists_kernel(const MlLists in, const int* __restrict__ bases_g, const int K,
                                                                   const int S, const int n_in, const int n, int* __restrict__ ids,
                                                                   float* __restrict__ scores, int* __restrict__ counts,
                                                                   int* __restrict__ rows) {
  __shared__ sl_key_t buf[2 * SL_MAX_N];                      // [0, SL_MAX_N): the best so far, sorted; [SL_MAX_N, ..): staging
  __shared__ int bases[DRN_SHARDS_MAX + 1];
  const int s = blockIdx.x, lane = threadIdx.x;
  for (int i = lane; i < 2 * SL_MAX_N; i += 64) buf[i] = 0ull;
  for (int i = lane; i <= K; i += 64) bases[i] = bases_g[i];
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;     // the lanes before this one
  sl_key_t thr = 0ull;                                        // the n-th best so far: only keys above it can enter the list
  int staged = 0;
  for (int b0 = 0; b0 < K; b0 += ML_PRE) {
    sl_key_t k0[ML_PRE], k1[ML_PRE];
#pragma unroll
    for (int u = 0; u < ML_PRE; ++u) {
      ml_keys(in, bases, min(b0 + u, K - 1), S, s, n_in, lane, k0[u], k1[u]);
      if (b0 + u >= K) k0[u] = k1[u] = 0ull;
    }
#pragma unroll
    for (int u = 0; u < ML_PRE; ++u) {
      const unsigned long long m0 = __ballot(k0[u] > thr), m1 = __ballot(k1[u] > thr);
      const int p0 = __popcll(m0), p = p0 + __popcll(m1);     // (<= 2 * 64 = SL_MAX_N)
      if (p == 0) continue;
      if (staged + p > SL_MAX_N) {                            // (wave-uniform) make room: fold the staging half in
        __syncthreads();
        sl_sort_desc<2 * SL_MAX_N, 64>(buf, 1, lane);
        for (int i = SL_MAX_N + lane; i < 2 * SL_MAX_N; i += 64) buf[i] = 0ull;
        thr = buf[n - 1];
        staged = 0;
        __syncthreads();
      }
      // (keys at or below a threshold that has just risen are staged all the same: the sort drops them)
      if ((m0 >> lane) & 1ull) buf[SL_MAX_N + staged + __popcll(m0 & below)] = k0[u];
      if ((m1 >> lane) & 1ull) buf[SL_MAX_N + staged + p0 + __popcll(m1 & below)] = k1[u];
      staged += p;
    }
  }
  __syncthreads();
  sl_sort_desc<2 * SL_MAX_N, 64>(buf, 1, lane);
  int cnt = 0;
  for (int i = lane; i < n; i += 64) {
    const sl_key_t k = buf[i];
    const bool ok = k != 0ull;
    ids[(long)s * n + i] = ok ? sl_video(k) : -1;
    scores[(long)s * n + i] = ok ? sl_score(k) : 0.f;
    if (ROWS && !ok) rows[(long)s * n + i] = -1;
    cnt += ok;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) cnt += __shfl_xor(cnt, w, 64);
  if (lane == 0) counts[s] = cnt;
  if (!ROWS) return;
  // the second walk: the row of every entry that made the list, to the place of its key
  const sl_key_t last = buf[n - 1];                           // (0 while the list is not full: then every candidate is in it)
  for (int k = 0; k < K; ++k) {
    sl_key_t key[2];
    ml_keys(in, bases, k, S, s, n_in, lane, key[0], key[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (key[h] == 0ull || key[h] < last) continue;
      int lo = 0, hi = n - 1;                                 // the first place whose key is not above this one
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (buf[mid] > key[h]) lo = mid + 1; else hi = mid;
      }
      if (buf[lo] == key[h]) rows[(long)s * n + lo] = in.rows[((long)k * S + s) * n_in + lane + 64 * h];
    }
  }
}

extern "C" int drn_shortlist_merge_lists(const int32_t* in_ids, const float* in_scores, const int32_t* in_counts, const int32_t* in_rows,
                                         const int32_t* bases, int K, int S, int n_in, int n, int32_t* ids, float* scores,
                                         int32_t* counts, int32_t* rows, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(in_ids && in_scores && in_counts && bases && ids && scores && counts, "drn_shortlist_merge_lists: null pointer");
  DRN_CHECK_ARG((in_rows == nullptr) == (rows == nullptr),
                "drn_shortlist_merge_lists: rows must be given on both sides (the lists of ragged shards) or on neither");
  DRN_CHECK_ARG(K >= 1 && K <= DRN_SHARDS_MAX, "drn_shortlist_merge_lists: K = %d lists a sentence outside [1, %d]", K, DRN_SHARDS_MAX);
  DRN_CHECK_ARG(S >= 1, "drn_shortlist_merge_lists: bad args (S = %d sentences)", S);
  DRN_CHECK_ARG(n_in >= 1 && n_in <= SL_MAX_N, "drn_shortlist_merge_lists: n_in = %d outside [1, %d]", n_in, SL_MAX_N);
  DRN_CHECK_ARG(n >= 1 && n <= SL_MAX_N, "drn_shortlist_merge_lists: n = %d outside [1, %d]", n, SL_MAX_N);
  DRN_CHECK_ARG((((uintptr_t)in_ids | (uintptr_t)in_scores | (uintptr_t)in_counts | (uintptr_t)in_rows | (uintptr_t)bases | (uintptr_t)ids |
                  (uintptr_t)scores | (uintptr_t)counts | (uintptr_t)rows) & 3) == 0,
                "drn_shortlist_merge_lists: every buffer must be 4-byte aligned");
  const MlLists in{in_ids, in_scores, in_counts, in_rows};
  if (rows)
    shortlist_merge_lists_kernel<true><<<S, 64, 0, (hipStream_t)stream>>>(in, bases, K, S, n_in, n, ids, scores, counts, rows);
  else
    shortlist_merge_lists_kernel<false><<<S, 64, 0, (hipStream_t)stream>>>(in, bases, K, S, n_in, n, ids, scores, counts, rows);
  return drn_launch_status("drn_shortlist_merge_lists");
}

// ---------------------------------------------------------------------------------------------------------------------------
// Mask slices.  words [rows][W], W = ceil(V / 32), is a packed mask over the whole corpus; shard k's own mask is the bits
// [bases[k], bases[k + 1]) moved down to bit 0: word w of its row holds the corpus bits bases[k] + 32 w .. + 31 -- two neighbouring
// words of the input through a funnel shift, a base need not be a multiple of 32 -- with the bits at or past V_k = bases[k + 1] -
// bases[k] zero, pack_allow's convention.  The pieces lie back to back in `out`: piece k is [rows][W_k], W_k = ceil(V_k / 32), from word
// rows * (W_0 + ... + W_(k-1)).  Each workgroup makes the running sums of W_k from bases (one wavefront, a shuffle scan) and writes
// nothing unless they end at `total`, the words a row the caller sized `out` by: bad bases give no access outside the buffers.
// One thread per output word.
__global__ __launch_bounds__(256) void allow_slices_kernel(const int* __restrict__ words, const int nrows, const int W,
                                                           const int* __restrict__ bases_g, const int K, const int total,
                                                           int* __restrict__ out) {
  __shared__ int bases[DRN_SHARDS_MAX + 1], first[DRN_SHARDS_MAX + 1];      // first[k]: the words a row before piece k
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int lo = tid < K ? bases_g[tid] : 0, hi = tid < K ? bases_g[tid + 1] : 0;
    const int wk = hi > lo ? (int)(((long)hi - lo + 31) >> 5) : 0;
    long sum = wk;                                            // (inclusive scan; 64 bits: bad bases may not wrap into `total`)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long up = __shfl_up(sum, d, 64);
      if (tid >= d) sum += up;
    }
    if (tid < K) {
      bases[tid] = lo;
      first[tid + 1] = sum > 0x7fffffffL ? -1 : (int)sum;
    }
    if (tid == 0) first[0] = 0;
    if (tid == K - 1) bases[K] = hi;
  }
  __syncthreads();
  if (first[K] != total) return;                              // (workgroup-uniform)
  const long at = (long)blockIdx.x * 256 + tid;
  if (at >= (long)nrows * total) return;
  const int r = (int)(at / total), t = (int)(at - (long)r * total);
  int k = 0;
  for (int step = 32; step > 0; step >>= 1)                   // the last piece that starts at or before word t (K <= 64)
    if (k + step < K && first[k + step] <= t) k += step;
  const int w = t - first[k], Wk = first[k + 1] - first[k];
  const long g = (long)bases[k] + 32L * w;                    // the corpus bit of bit 0 of this word
  const long gw = g >> 5;
  const int sh = (int)(g & 31);
  const unsigned lo = (g >= 0 && gw < W) ? (unsigned)words[(long)r * W + gw] : 0u;
  const unsigned hi = (g >= 0 && gw + 1 < W) ? (unsigned)words[(long)r * W + gw + 1] : 0u;
  unsigned v = (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
  const long left = (long)bases[k + 1] - g;                   // the shard's bits from this word on (>= 1)
  if (left < 32) v &= (1u << left) - 1u;
  out[(long)nrows * first[k] + (long)r * Wk + w] = (int)v;
}

extern "C" int drn_allow_slices(const int32_t* words, int rows, int V, const int32_t* bases, int K, int total_words, int32_t* out,
                                void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(words && bases && out, "drn_allow_slices: null pointer");
  DRN_CHECK_ARG(rows >= 1 && V >= 1, "drn_allow_slices: bad args (rows = %d, V = %d videos)", rows, V);
  DRN_CHECK_ARG(K >= 1 && K <= DRN_SHARDS_MAX, "drn_allow_slices: K = %d shards outside [1, %d]", K, DRN_SHARDS_MAX);
  const int W = cdiv(V, 32);
  DRN_CHECK_ARG(total_words >= W && (long)total_words <= (long)W + K - 1,
                "drn_allow_slices: %d words a row for the pieces; K = %d shards of V = %d videos come to between %d and %ld", total_words, K, V,
                W, (long)W + K - 1);
  DRN_CHECK_ARG((((uintptr_t)words | (uintptr_t)bases | (uintptr_t)out) & 3) == 0, "drn_allow_slices: every buffer must be 4-byte aligned");
  const long elems = (long)rows * total_words;
  DRN_CHECK_ARG(elems <= 0x7fffffffL, "drn_allow_slices: %d rows of %d words are more than 2^31 words", rows, total_words);
  allow_slices_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, (hipStream_t)stream>>>(words, rows, W, bases, K, total_words, out);
  return drn_launch_status("drn_allow_slices");
}
