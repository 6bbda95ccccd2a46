// The first stage of a two-stage search, on the device (drn_amd/retrieve.py, Grounder.search(candidates=device tensor)):
//   drn_shortlist_topn   each sentence's best n videos of a (V, E) embedding table by dot product, under a TOTAL order;
//   drn_plan_candidates  a (S, N) table of candidate positions -> the pair_video rows of the search's steps.
#include "common.h"
#include "shortlist.h"
#include "../../include/drn_hip.h"

// ---------------------------------------------------------------------------------------------------------------------------
// Shortlist.  score[s][v] = sum_e q[s][e] * emb[v][e], accumulated in fp32 on MFMAs; sentence s lists the videos whose score is
// finite, by score descending, then position ascending.
//
// ONE (s, v) score is one accumulator element of a chain of MFMAs over the K-steps 0, 1, ... of E in ascending order: bf16 on
// v_mfma_f32_16x16x32_bf16 (32 columns per step, lane group g = lane >> 4 holds columns 32 k + 8 g .. + 7 of both operands), fp32 on
// v_mfma_f32_16x16x4_f32 (16 columns per four MFMAs: lane group g loads columns 16 k + 4 g .. + 3 and MFMA i takes element i, so MFMA
// i sums the columns 16 k + 4 g + i over g).  Columns past E are zeros.  Which tile, workgroup or row of the tile a pair falls in
// changes neither the steps nor their order, so a score's bits do not depend on V, S, n or the grid.
//
// A candidate is ONE 64-bit key: the score as an unsigned word that orders as the float does (-0 folded into +0) above the
// complement of the position.  Larger key = earlier in the list; 0 = no candidate (a finite score's word is never 0).  The total
// order is one integer comparison, all keys of a sentence are distinct, and so the best n of a set do not depend on how they are found.
//
// Phase one (shortlist_block_kernel): workgroup (b, t) scores the SL_BLOCK videos of block b against the 16 sentences of tile t -- four
// waves, four 16-video MFMA tiles each, fragments straight from memory, the table read ONCE per 16 sentences -- sorts each sentence's
// SL_BLOCK keys in LDS (bitonic, descending) and writes the first m = min(n, SL_BLOCK) to ws[s][b][0..m).
// Phase two (shortlist_merge_kernel): one wavefront per sentence walks its blocks' lists; keys above the current n-th best are
// appended to a staging half of a 2 * SL_MAX_N LDS buffer, which is sorted whenever it would overflow and at the end.
// No atomics, no tickets: two launches.
#define SL_BLOCK 256
#define SL_MAX_N DRN_SHORTLIST_MAX
#define SL_PRE 8            // lists phase two keeps in flight

// (the key, the sort, the fragment loaders and the MFMA step: shortlist.h, shared with retrieve_seg.hip)

template <typename T>
__global__ __launch_bounds__(256) void shortlist_block_kernel(const T* __restrict__ emb, const T* __restrict__ q, const int V,
                                                              const int E, const int S, const int m, const int nblocks,
                                                              sl_key_t* __restrict__ ws) {
  __shared__ sl_key_t keys[16 * SL_BLOCK];                    // 32 KiB: [sentence of the tile][video of the block]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, s0 = blockIdx.y * 16, v0 = b * SL_BLOCK + wave * 64;
  const int r = lane & 15, g = lane >> 4;
  // (a row past S or V reads the last row instead: its scores become no keys below)
  const T* qrow = q + (long)min(s0 + r, S - 1) * E;
  const T* erow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) erow[j] = emb + (long)min(v0 + 16 * j + r, V - 1) * E;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int COLS = SlStep<T>::COLS, PER_LANE = SlStep<T>::PER_LANE;
  // whole steps on 16-byte loads where every row starts on a 16-byte boundary (the tables are 16-byte aligned), then the rest
  const int whole = E % PER_LANE == 0 ? E / COLS * COLS : 0;
  int c = 0;
  for (; c < whole; c += COLS) {
    const int c0 = c + g * PER_LANE;
    const auto a = sl_frag(qrow, c0);
    decltype(sl_frag(qrow, c0)) bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = sl_frag(erow[j], c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a, bv[j], acc[j]);
  }
  for (; c < E; c += COLS) {
    const int c0 = c + g * PER_LANE;
    const auto a = sl_frag_tail(qrow, c0, E);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = sl_mfma(a, sl_frag_tail(erow[j], c0, E), acc[j]);
  }
  // C/D: column (video) lane & 15, row (sentence) 4 (lane >> 4) + i
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + 16 * j + r, sl = 4 * g + i;
      keys[sl * SL_BLOCK + wave * 64 + 16 * j + r] = (v < V && s0 + sl < S) ? sl_key(acc[j][i], v) : 0ull;
    }
  __syncthreads();
  sl_sort_desc<SL_BLOCK, 256>(keys, 16, tid);
  const int rows = min(16, S - s0);
  for (int p = tid; p < rows * m; p += 256) {
    const int sl = p / m, i = p - sl * m;
    ws[((long)(s0 + sl) * nblocks + b) * m + i] = keys[sl * SL_BLOCK + i];
  }
}

__global__ __launch_bounds__(64) void shortlist_merge_kernel(const sl_key_t* __restrict__ ws, const int n, const int m,
                                                             const int nblocks, int* __restrict__ ids, float* __restrict__ scores,
                                                             int* __restrict__ counts) {
  __shared__ sl_key_t buf[2 * SL_MAX_N];                      // [0, SL_MAX_N): the best so far, sorted; [SL_MAX_N, ..): staging
  const int s = blockIdx.x, lane = threadIdx.x;
  for (int i = lane; i < 2 * SL_MAX_N; i += 64) buf[i] = 0ull;
  __syncthreads();
  const sl_key_t* mine = ws + (long)s * nblocks * m;
  const bool two = m > 64;                                    // (m <= SL_MAX_N = 128: at most two keys of a list per lane)
  sl_key_t thr = 0ull;                                        // the n-th best so far: only keys above it can enter the list
  int staged = 0;
  for (int b0 = 0; b0 < nblocks; b0 += SL_PRE) {
    sl_key_t k0[SL_PRE], k1[SL_PRE];
#pragma unroll
    for (int u = 0; u < SL_PRE; ++u) {
      const bool live = b0 + u < nblocks;
      const sl_key_t* list = mine + (long)(b0 + u) * m;
      k0[u] = (live && lane < m) ? list[lane] : 0ull;
      k1[u] = (live && two && lane + 64 < m) ? list[lane + 64] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < SL_PRE; ++u) {
      // (a list is sorted, so the keys above thr are a prefix of it: p0 of the first 64, then p1 of the rest)
      const int p0 = __popcll(__ballot(k0[u] > thr)), p1 = __popcll(__ballot(k1[u] > thr));
      const int p = p0 + p1;                                  // (<= m <= SL_MAX_N)
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
      if (lane < p0) buf[SL_MAX_N + staged + lane] = k0[u];
      if (lane < p1) buf[SL_MAX_N + staged + p0 + lane] = k1[u];
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
    cnt += ok;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) cnt += __shfl_xor(cnt, w, 64);
  if (lane == 0) counts[s] = cnt;
}

// (declared in shortlist.h: retrieve_seg.hip's lists are merged by the same kernel; not part of the C ABI)
void sl_launch_merge(const sl_key_t* ws, int S, int n, int m, int nblocks, int32_t* ids, float* scores, int32_t* counts, hipStream_t stream) {
  shortlist_merge_kernel<<<S, 64, 0, stream>>>(ws, n, m, nblocks, ids, scores, counts);
}

extern "C" int drn_shortlist_topn(const void* emb, const void* queries, int V, int E, int S, int n, int dtype, void* ws, int ws_keys,
                                  int32_t* ids, float* scores, int32_t* counts, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(emb && queries && ws && ids && scores && counts, "drn_shortlist_topn: null pointer");
  DRN_CHECK_ARG(V >= 1 && E >= 1 && S >= 1, "drn_shortlist_topn: bad args (V = %d videos, E = %d columns, S = %d sentences)", V, E, S);
  DRN_CHECK_ARG(n >= 1 && n <= SL_MAX_N, "drn_shortlist_topn: n = %d outside [1, %d]", n, SL_MAX_N);
  DRN_CHECK_ARG(dtype == DRN_F32 || dtype == DRN_BF16, "drn_shortlist_topn: dtype %d (float32 / bfloat16 only)", dtype);
  DRN_CHECK_ARG(((uintptr_t)emb & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)ws & 7) == 0,
                "drn_shortlist_topn: the table and the queries must be 16-byte aligned, the workspace 8-byte aligned");
  const int m = n < SL_BLOCK ? n : SL_BLOCK, nblocks = cdiv(V, SL_BLOCK), tiles = cdiv(S, 16);
  const long need = (long)S * nblocks * m;
  DRN_CHECK_ARG(need <= 0x7fffffffL && ws_keys >= need, "drn_shortlist_topn: the workspace holds %d keys, %ld are needed (S * ceil(V / %d) * min(n, %d))",
                ws_keys, need, SL_BLOCK, SL_BLOCK);
  DRN_CHECK_ARG(tiles <= 65535, "drn_shortlist_topn: S = %d, more than 65535 tiles of 16 sentences", S);
  const dim3 grid(nblocks, tiles);
  if (dtype == DRN_BF16)
    shortlist_block_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)emb, (const bf16_t*)queries, V, E, S, m, nblocks,
                                                                          (sl_key_t*)ws);
  else
    shortlist_block_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)emb, (const float*)queries, V, E, S, m, nblocks,
                                                                         (sl_key_t*)ws);
  sl_launch_merge((const sl_key_t*)ws, S, n, m, nblocks, ids, scores, counts, (hipStream_t)stream);
  return drn_launch_status("drn_shortlist_topn");
}

// ---------------------------------------------------------------------------------------------------------------------------
// The data half of a search over device candidates.  cand [S][N] int32: row s is sentence s's set of store positions; an entry outside
// [0, Nv) is no candidate and of a position repeated in a row only the first occurrence counts -- across the WHOLE row, or a repeat in
// another column block would be ranked twice by a later merge step.  The steps are a function of the shapes alone
// (grounding.plan_candidate_steps): step sb * ncb + cb holds the sentences [sb * Sc, + Sc) and the columns [cb * Nc, + Nc), pair
// sl * Nc + jl = (sentence sb * Sc + sl, column cb * Nc + jl).  table [steps][pairs] gets the pair's store position or -1 (no
// candidate, a sentence or column past S or N, a pair past Sc * Nc).  One workgroup per sentence slot of the grid (nsb * Sc of them)
// holds its row in LDS; the slot with sl == 0 also writes its steps' tails.  Every element of the table is written exactly once.
#define PLAN_MAX_N DRN_CANDIDATES_MAX

__global__ __launch_bounds__(256) void plan_candidates_kernel(const int* __restrict__ cand, const int S, const int N, const int Nv,
                                                              const int Sc, const int Nc, const int ncb, const int pairs,
                                                              int* __restrict__ table) {
  __shared__ int row[PLAN_MAX_N];
  const int s = blockIdx.x, sb = s / Sc, sl = s - sb * Sc, tid = threadIdx.x;
  if (s < S)
    for (int j = tid; j < N; j += 256) row[j] = cand[(long)s * N + j];
  __syncthreads();
  for (int j = tid; j < ncb * Nc; j += 256) {
    int v = -1;
    if (s < S && j < N) {
      v = row[j];
      if (v < 0 || v >= Nv) v = -1;
      for (int i = 0; v >= 0 && i < j; ++i)
        if (row[i] == v) v = -1;
    }
    const int cb = j / Nc, jl = j - cb * Nc;
    table[(long)(sb * ncb + cb) * pairs + sl * Nc + jl] = v;
  }
  if (sl == 0) {
    const int tail = pairs - Sc * Nc;
    for (int p = tid; p < ncb * tail; p += 256) {
      const int cb = p / tail, i = p - cb * tail;
      table[(long)(sb * ncb + cb) * pairs + Sc * Nc + i] = -1;
    }
  }
}

extern "C" int drn_plan_candidates(const int32_t* cand, int S, int N, int Nv, int Sc, int Nc, int pairs, int steps, int32_t* table,
                                   void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(cand && table, "drn_plan_candidates: null pointer");
  DRN_CHECK_ARG(S >= 1 && N >= 1 && N <= PLAN_MAX_N && Nv >= 0, "drn_plan_candidates: bad args (S = %d sentences, N = %d columns of at most %d, Nv = %d videos)",
                S, N, PLAN_MAX_N, Nv);
  DRN_CHECK_ARG(Sc >= 1 && Sc <= S && Nc >= 1 && Nc <= N && pairs >= 1 && (long)Sc * Nc <= pairs,
                "drn_plan_candidates: a step of %d sentences x %d columns does not fit %d pairs", Sc, Nc, pairs);
  const int nsb = cdiv(S, Sc), ncb = cdiv(N, Nc);
  DRN_CHECK_ARG((long)nsb * ncb == steps, "drn_plan_candidates: %d steps given, the shapes make %ld", steps, (long)nsb * ncb);
  DRN_CHECK_ARG((long)steps * pairs <= 0x7fffffffL, "drn_plan_candidates: more than 2^31 table entries");
  plan_candidates_kernel<<<nsb * Sc, 256, 0, (hipStream_t)stream>>>(cand, S, N, Nv, Sc, Nc, ncb, pairs, table);
  return drn_launch_status("drn_plan_candidates");
}
