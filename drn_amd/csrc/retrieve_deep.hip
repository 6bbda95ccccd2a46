// Deep shortlists (drn_amd/retrieve.py, Shortlister.shortlist_deep): the merge of drn_shortlist_deep (retrieve_allow.hip), lists of up
// to DRN_SHORTLIST_DEEP_MAX = 1024 videos a sentence -- the width drn_shortlist_rerank and drn_plan_candidates take.
//   shortlist_merge_deep_kernel<CAP>   shortlist_merge_kernel's contract (retrieve.hip) at depth, CAP in {256, 512, 1024};
//   sl_launch_merge_deep               its launch, declared in shortlist.h beside sl_launch_merge.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// Phase one is not here: the masked phase-one kernels of retrieve_allow.hip write m = min(n, 256) sorted keys per (sentence, block),
// and a block holds at most 256 videos, so at n >= 256 a block's list is complete.
//
// The merge: sentence s merges its nblocks lists ws[s][b][0..m), each sorted descending with key 0 = no candidate and all keys of a
// sentence distinct, into ids, scores [S][n] and counts [S].  ONE workgroup of 256 threads per sentence walks the lists FOUR at a
// time, one per wave, up to four keys of a list per lane (m <= 256); the next four are loaded before the current four are staged.
// The keys above the current n-th best are a prefix of a sorted list: a wave counts them with ballots, the four counts cross LDS
// (cnt, two sets used in turn: one barrier a round), and every thread walks the four counts in list order -- so where a list lands
// in the staging half depends on the lists before it alone, and the best n of a set of distinct keys do not depend on how they are
// found.  When staging would overflow, and once at the end, sl_sort_desc<2 * CAP, 256> folds it in; keys staged under a threshold
// that has just risen are dropped by that sort.  No atomics, no tickets, no workgroup waits on another.
//
// Bounds: 1 <= m <= min(n, 256) and n <= CAP (sl_launch_merge_deep picks the smallest such CAP; the entry checks n).  A list stages
// p <= m <= CAP keys at staged + i, i < p, and staged + p <= CAP holds after the fold that makes room, so every store lies in buf.
#define DP_THREADS 256
#define DP_WAVES 4          // lists in flight: one per wave
#define DP_PER_LANE 4       // keys of a list per lane: 64 * 4 = 256 >= m

// Static LDS: buf 2 * CAP keys of 8 bytes and cnt 2 * 4 words = 16 * CAP + 32 bytes: 4,128 / 8,224 / 16,416 B at CAP = 256 / 512 / 1024.
template <int CAP>
__global__ __launch_bounds__(DP_THREADS) void shortlist_merge_deep_kernel(const sl_key_t* __restrict__ ws, const int n, const int m,
                                                                          const int nblocks, int* __restrict__ ids,
                                                                          float* __restrict__ scores, int* __restrict__ counts) {
  __shared__ sl_key_t buf[2 * CAP];                           // [0, CAP): the best so far, sorted; [CAP, 2 CAP): staging
  __shared__ int cnt[2][DP_WAVES];                            // each wave's keys above the threshold, of this round and the last
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 2 * CAP; i += DP_THREADS) buf[i] = 0ull;
  const sl_key_t* mine = ws + (long)s * nblocks * m;
  sl_key_t thr = 0ull;                                        // the n-th best so far: only keys above it can enter the list
  int staged = 0;
  sl_key_t next[DP_PER_LANE];
#pragma unroll
  for (int j = 0; j < DP_PER_LANE; ++j) next[j] = (wave < nblocks && lane + 64 * j < m) ? mine[(long)wave * m + lane + 64 * j] : 0ull;
  __syncthreads();
  for (int b0 = 0, round = 0; b0 < nblocks; b0 += DP_WAVES, ++round) {
    sl_key_t k[DP_PER_LANE];
#pragma unroll
    for (int j = 0; j < DP_PER_LANE; ++j) k[j] = next[j];
    const int nb = b0 + DP_WAVES + wave;                      // (wave-uniform) the list this wave stages in the next round
#pragma unroll
    for (int j = 0; j < DP_PER_LANE; ++j) next[j] = (nb < nblocks && lane + 64 * j < m) ? mine[(long)nb * m + lane + 64 * j] : 0ull;
    // (a list is sorted, so the keys above thr are a prefix of it: key lane + 64 j has place lane + 64 j)
    int p = 0;
#pragma unroll
    for (int j = 0; j < DP_PER_LANE; ++j) p += __popcll(__ballot(k[j] > thr));
    if (lane == 0) cnt[round & 1][wave] = p;
    __syncthreads();
    int c[DP_WAVES];
#pragma unroll
    for (int u = 0; u < DP_WAVES; ++u) c[u] = cnt[round & 1][u];
#pragma unroll
    for (int u = 0; u < DP_WAVES; ++u) {
      if (c[u] == 0) continue;                                // (workgroup-uniform, as everything below but the stores)
      if (staged + c[u] > CAP) {                              // make room: fold the staging half in
        __syncthreads();
        sl_sort_desc<2 * CAP, DP_THREADS>(buf, 1, tid);
        thr = buf[n - 1];
        for (int i = CAP + tid; i < 2 * CAP; i += DP_THREADS) buf[i] = 0ull;
        staged = 0;
        __syncthreads();
      }
      // (keys at or below a threshold that has just risen are staged all the same: the sort drops them)
      if (wave == u) {
#pragma unroll
        for (int j = 0; j < DP_PER_LANE; ++j)
          if (lane + 64 * j < c[u]) buf[CAP + staged + lane + 64 * j] = k[j];
      }
      staged += c[u];
    }
  }
  __syncthreads();
  sl_sort_desc<2 * CAP, DP_THREADS>(buf, 1, tid);
  // the list is a prefix of buf: the place whose successor is empty (or past n) knows the count
  for (int i = tid; i < n; i += DP_THREADS) {
    const sl_key_t key = buf[i], after = i + 1 < n ? buf[i + 1] : 0ull;
    const bool ok = key != 0ull;
    ids[(long)s * n + i] = ok ? sl_video(key) : -1;
    scores[(long)s * n + i] = ok ? sl_score(key) : 0.f;
    if (ok && after == 0ull) counts[s] = i + 1;
    if (i == 0 && !ok) counts[s] = 0;
  }
}

// (declared in shortlist.h; not part of the C ABI.  The caller has checked 1 <= m <= min(n, 256) and n <= DRN_SHORTLIST_DEEP_MAX)
void sl_launch_merge_deep(const sl_key_t* ws, int S, int n, int m, int nblocks, int32_t* ids, float* scores, int32_t* counts,
                          hipStream_t stream) {
  static_assert(DRN_SHORTLIST_DEEP_MAX == 1024, "the largest CAP below is the deepest list");
  if (n <= 256) shortlist_merge_deep_kernel<256><<<S, DP_THREADS, 0, stream>>>(ws, n, m, nblocks, ids, scores, counts);
  else if (n <= 512) shortlist_merge_deep_kernel<512><<<S, DP_THREADS, 0, stream>>>(ws, n, m, nblocks, ids, scores, counts);
  else shortlist_merge_deep_kernel<1024><<<S, DP_THREADS, 0, stream>>>(ws, n, m, nblocks, ids, scores, counts);
}
