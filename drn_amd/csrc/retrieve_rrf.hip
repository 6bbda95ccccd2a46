// RANK FUSION (drn_amd/retrieve.py: rank_fuse, rank_fuse_rank, RankFusedShortlister): reciprocal-rank fusion of M finished id lists.
//   drn_rank_fuse_topn   each sentence's best n videos by the sum of their votes w[m] / (k0 + rank in list m + 1), one total order;
//   drn_rank_fuse_rank   the place of a named video in that order (drn_shortlist_rank's three fields).
// drn_amd.retrieve.rank_fuse_reference and rank_fuse_rank_reference are the definitions.  Only the lists are read: no table, no dense
// score matrix, no workspace in global memory, no atomics.  ONE launch, one workgroup per sentence.
#include "common.h"
#include "shortlist.h"
#include "fuse.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// THE KERNEL.  A sentence's M * C entries become 64-bit words in LDS, LEN of them (a power of two >= M * C, at most 8192: 64 KiB).
//   1. entry (list m, column j) holding id -> the word (id << 32) | (m << 16) | j, stored COMPLEMENTED, so that sl_sort_desc sorts the
//      words themselves ascending: by id, then list, then column.  An id outside [0, V) and the padding up to LEN are stored as 0, which
//      no complemented word equals (an id in [0, V) has a clear top bit) and which sorts last.
//   2. after the sort the first word of an (id, m) run is list m's FIRST occurrence of the video and its low 16 bits are the rank; the
//      first word of an id run OWNS the video.
//   3. the owner folds the votes of the lists that hold the video in the sorted order, which is m ascending: acc = +0, acc = acc +
//      w[m] / (k0 + float(j + 1)), one fp32 add, one correctly rounded division and one more add a term, nothing contracted.  It steps
//      from list to list by binary search for the first word at or above (id, m + 1, 0): at most M searches of log2(LEN) reads each,
//      however often the row repeats one id.
//   4. the owner's sl_key(acc, id) -- 0 where the fold is not finite, the mask bit is clear or (drop) a list does not hold the video --
//      is kept in a register across a barrier and written back over the sorted row; every other word becomes 0.
//   5. topn: the same sort, now of candidate keys; the best n are written, and the number of keys that are not 0 is the place of the
//      last one.  rank: the owner of targets[s] publishes its key, and every thread counts, from its registers, the keys above it.
// Every index into LDS is below LEN by construction, every read of the lists lies at m < M, j < C of row s, a mask word is read only
// for an id already known to lie in [0, V), and targets[s] is compared, never used as an index.
#define RF_LIST_SHIFT 16
#define RF_LOW_MASK 0xffffull

__device__ __forceinline__ bool rf_allowed(const int* __restrict__ allow, const int stride, const int s, const int v) {
  return allow == nullptr || ((allow[(long)s * stride + (v >> 5)] >> (v & 31)) & 1);
}

// the candidate key of the video that the sorted word at p owns (0: p owns none, or the video is no candidate)
template <int LEN>
__device__ __forceinline__ sl_key_t rf_owner_key(const sl_key_t* keys, const int p, const float* __restrict__ weights, const float k0,
                                                 const int M, const int mode, const int* __restrict__ allow, const int allow_stride,
                                                 const int s) {
  const sl_key_t c = keys[p];
  if (c == 0ull) return 0ull;
  const unsigned id = (unsigned)(~c >> 32);
  if (p > 0 && (unsigned)(~keys[p - 1] >> 32) == id) return 0ull;               // (an earlier word of the same video owns it)
  float acc = 0.f;
  int held = 0, at = p;
  for (int step = 0; step < DRN_RANK_FUSE_MAX_LISTS; ++step) {                   // (m rises with every step: at most M <= 8 of them)
    const sl_key_t cur = ~keys[at];
    const int m = (int)((cur >> RF_LIST_SHIFT) & RF_LOW_MASK), j = (int)(cur & RF_LOW_MASK);
    acc = fu_add(acc, __fdiv_rn(weights[m], fu_add(k0, (float)(j + 1))));
    ++held;
    if (m + 1 >= M) break;
    // the first word after `at` that is at or above (id, m + 1, 0): complemented, the first stored word <= want
    const sl_key_t want = ~(((sl_key_t)id << 32) | ((sl_key_t)(m + 1) << RF_LIST_SHIFT));
    int lo = at + 1;
    if (lo < LEN && keys[lo] > want) {                                           // (not the neighbour: a repeat inside list m)
      int hi = LEN;
      ++lo;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] <= want) hi = mid;
        else lo = mid + 1;
      }
    }
    if (lo >= LEN) break;
    const sl_key_t next = keys[lo];
    if (next == 0ull || (unsigned)(~next >> 32) != id) break;                    // (the video's run has ended)
    at = lo;
  }
  const bool ok = (mode == DRN_FUSE_SKIP || held == M) && rf_allowed(allow, allow_stride, s, (int)id);
  return ok ? sl_key(acc, (int)id) : 0ull;
}

template <int LEN, int NT, bool RANK>
__global__ __launch_bounds__(NT) void rank_fuse_kernel(const int* __restrict__ lists, const long stride_m, const long ld, const int C,
                                                       const int M, const int V, const float* __restrict__ weights, const float k0,
                                                       const int mode, const int* __restrict__ allow, const int allow_stride, const int n,
                                                       int* __restrict__ ids, float* __restrict__ scores, int* __restrict__ counts,
                                                       const int* __restrict__ targets, int* __restrict__ rank, float* __restrict__ score,
                                                       int* __restrict__ total) {
  constexpr int PER = LEN / NT;                               // words a thread owns: p = tid + i * NT
  __shared__ sl_key_t keys[LEN];
  __shared__ sl_key_t tkey;                                   // rank: the target's key
  __shared__ int wa[NT / 64], wn[NT / 64];                    // rank: each wave's counts
  const int tid = threadIdx.x, s = blockIdx.x;
  const int entries = M * C;                                  // (<= LEN: the entry picks LEN)
  for (int p = tid; p < LEN; p += NT) {
    sl_key_t word = 0ull;
    if (p < entries) {
      const int m = p / C, j = p - m * C;
      const int id = lists[m * stride_m + s * ld + j];
      if (id >= 0 && id < V) word = ~(((sl_key_t)(unsigned)id << 32) | ((sl_key_t)m << RF_LIST_SHIFT) | (sl_key_t)j);
    }
    keys[p] = word;
  }
  if (RANK && tid == 0) tkey = 0ull;
  __syncthreads();
  sl_sort_desc<LEN, NT>(keys, 1, tid);                        // (ends in a barrier)
  sl_key_t mine[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) mine[i] = rf_owner_key<LEN>(keys, tid + i * NT, weights, k0, M, mode, allow, allow_stride, s);
  if constexpr (RANK) {
    const int t = targets[s];
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if (mine[i] != 0ull && sl_video(mine[i]) == t) tkey = mine[i];             // (one owner a video: one writer at most)
    __syncthreads();
    const sl_key_t tk = tkey;
    int above = 0, any = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      above += mine[i] > tk;
      any += mine[i] != 0ull;
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
      above += __shfl_xor(above, w, 64);
      any += __shfl_xor(any, w, 64);
    }
    if ((tid & 63) == 0) {
      wa[tid >> 6] = above;
      wn[tid >> 6] = any;
    }
    __syncthreads();
    if (tid == 0) {
      int a = 0, c = 0;
      for (int w = 0; w < NT / 64; ++w) {
        a += wa[w];
        c += wn[w];
      }
      rank[s] = tk != 0ull ? a : -1;
      score[s] = tk != 0ull ? sl_score(tk) : 0.f;
      total[s] = c;
    }
  } else {
    __syncthreads();                                          // (every read of the sorted row is done)
#pragma unroll
    for (int i = 0; i < PER; ++i) keys[tid + i * NT] = mine[i];
    __syncthreads();
    sl_sort_desc<LEN, NT>(keys, 1, tid);
    for (int i = tid; i < n; i += NT) {
      const sl_key_t k = i < LEN ? keys[i] : 0ull;
      ids[(long)s * n + i] = k != 0ull ? sl_video(k) : -1;
      scores[(long)s * n + i] = k != 0ull ? sl_score(k) : 0.f;
    }
    // the keys that are not 0 stand first: the last of them says how many they are
    for (int p = tid; p < LEN; p += NT)
      if (keys[p] != 0ull && (p == LEN - 1 || keys[p + 1] == 0ull)) counts[s] = min(p + 1, n);
    if (tid == 0 && keys[0] == 0ull) counts[s] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The entries.

struct RfArgs {
  const int32_t* lists;
  long stride_m, ld;
  int C, M, V;
  const float* weights;
  float k0;
  int mode;
  const int32_t* allow;
  int allow_stride, S, n;
  int32_t* ids;
  float* scores;
  int32_t* counts;
  const int32_t* targets;
  int32_t* rank;
  float* score;
  int32_t* total;
};

template <int LEN, int NT, bool RANK>
static void rf_launch_len(const RfArgs& a, hipStream_t stream) {
  rank_fuse_kernel<LEN, NT, RANK><<<a.S, NT, 0, stream>>>(a.lists, a.stride_m, a.ld, a.C, a.M, a.V, a.weights, a.k0, a.mode, a.allow,
                                                          a.allow ? a.allow_stride : 0, a.n, a.ids, a.scores, a.counts, a.targets, a.rank,
                                                          a.score, a.total);
}

// the sort length is the power of two at or above M * C, 256 at the least: a 2 x 128 fusion does not sort 8192 words
template <bool RANK>
static void rf_launch(const RfArgs& a, hipStream_t stream) {
  const int entries = a.M * a.C;
  if (entries <= 256) rf_launch_len<256, 256, RANK>(a, stream);
  else if (entries <= 512) rf_launch_len<512, 256, RANK>(a, stream);
  else if (entries <= 1024) rf_launch_len<1024, 256, RANK>(a, stream);
  else if (entries <= 2048) rf_launch_len<2048, 1024, RANK>(a, stream);
  else if (entries <= 4096) rf_launch_len<4096, 1024, RANK>(a, stream);
  else rf_launch_len<8192, 1024, RANK>(a, stream);
}

static int rf_check(const char* what, const int32_t* lists, long long stride_m, int ld, int C, int M, int V, const float* weights, float k0,
                    int mode, const int32_t* allow, int allow_stride, int S) {
  DRN_CHECK_ARG(lists && weights, "%s: null pointer", what);
  DRN_CHECK_ARG(V >= 1 && S >= 1, "%s: bad args (V = %d videos, S = %d sentences)", what, V, S);
  DRN_CHECK_ARG(M >= 1 && M <= DRN_RANK_FUSE_MAX_LISTS, "%s: M = %d lists outside [1, %d]", what, M, DRN_RANK_FUSE_MAX_LISTS);
  DRN_CHECK_ARG(C >= 1 && C <= DRN_SHORTLIST_DEEP_MAX, "%s: C = %d entries a list outside [1, %d]", what, C, DRN_SHORTLIST_DEEP_MAX);
  DRN_CHECK_ARG(mode == DRN_FUSE_DROP || mode == DRN_FUSE_SKIP, "%s: mode = %d is neither %d (drop) nor %d (skip)", what, mode, DRN_FUSE_DROP,
                DRN_FUSE_SKIP);
  DRN_CHECK_ARG(k0 >= 0.f && k0 <= 3.402823466e38f, "%s: k0 = %g is not a finite number >= 0", what, (double)k0);
  DRN_CHECK_ARG(ld >= C, "%s: ld = %d below C = %d", what, ld, C);
  DRN_CHECK_ARG(M == 1 || stride_m >= (long long)(S - 1) * ld + C,
                "%s: stride_m = %lld below the (S - 1) * ld + C = %lld elements of one list", what, stride_m, (long long)(S - 1) * ld + C);
  DRN_CHECK_ARG(((uintptr_t)lists & 3) == 0 && ((uintptr_t)weights & 3) == 0, "%s: lists and weights must be 4-byte aligned", what);
  DRN_CHECK_ARG(S <= 65535, "%s: S = %d, more than 65535 sentences", what, S);
  return fu_check_allow(what, allow, allow_stride, V);
}

extern "C" int drn_rank_fuse_topn(const int32_t* lists, long long stride_m, int ld, int C, int M, int V, const float* weights, float k0,
                                  int mode, const int32_t* allow, int allow_stride, int S, int n, int32_t* ids, float* scores,
                                  int32_t* counts, void* stream) {
  const char* what = "drn_rank_fuse_topn";
  drn_clear_status();
  if (const int rc = rf_check(what, lists, stride_m, ld, C, M, V, weights, k0, mode, allow, allow_stride, S)) return rc;
  DRN_CHECK_ARG(ids && scores && counts, "%s: null pointer", what);
  DRN_CHECK_ARG(n >= 1 && n <= DRN_SHORTLIST_DEEP_MAX, "%s: n = %d outside [1, %d]", what, n, DRN_SHORTLIST_DEEP_MAX);
  DRN_CHECK_ARG(((uintptr_t)ids & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)counts & 3) == 0,
                "%s: ids, scores and counts must be 4-byte aligned", what);
  const RfArgs a = {lists, (long)stride_m, (long)ld, C, M, V, weights, k0, mode, allow, allow_stride, S, n, ids, scores, counts,
                    nullptr, nullptr, nullptr, nullptr};
  rf_launch<false>(a, (hipStream_t)stream);
  return drn_launch_status(what);
}

extern "C" int drn_rank_fuse_rank(const int32_t* lists, long long stride_m, int ld, int C, int M, int V, const float* weights, float k0,
                                  int mode, const int32_t* allow, int allow_stride, int S, const int32_t* targets, int32_t* rank,
                                  float* score, int32_t* total, void* stream) {
  const char* what = "drn_rank_fuse_rank";
  drn_clear_status();
  if (const int rc = rf_check(what, lists, stride_m, ld, C, M, V, weights, k0, mode, allow, allow_stride, S)) return rc;
  DRN_CHECK_ARG(targets && rank && score && total, "%s: null pointer", what);
  DRN_CHECK_ARG(((uintptr_t)targets & 3) == 0 && ((uintptr_t)rank & 3) == 0 && ((uintptr_t)score & 3) == 0 && ((uintptr_t)total & 3) == 0,
                "%s: targets, rank, score and total must be 4-byte aligned", what);
  const RfArgs a = {lists, (long)stride_m, (long)ld, C, M, V, weights, k0, mode, allow, allow_stride, S, 0, nullptr, nullptr, nullptr,
                    targets, rank, score, total};
  rf_launch<true>(a, (hipStream_t)stream);
  return drn_launch_status(what);
}
