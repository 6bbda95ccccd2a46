// Eval-time post-processor of the dense heads (model/inference.py:51-120,166-199), one workgroup per clip:
//   candidates  sigmoid(logit) > thr        (tested BEFORE the IoU-score product, inference.py:71-79)
//   score       sigmoid(logit) [* sigmoid(iou)]   (second / third stage)
//   per level   keep the top_n scores (torch.topk(sorted=False): any order -- kept here in location order)
//   decode      ((loc - reg0)/32, (loc + reg1)/32) clamped to [0,1], score = sqrt(score), location = loc/32
// Kept candidates of a clip are written level after level (the order select_over_all_levels concatenates), counts per
// (clip, level) tell the host how to slice them: ONE device->host copy per batch instead of the reference's
// nonzero / tolist round trips per clip and level.  reg = exp(.) > 0, so the reference's min_size = 0 filter never fires.
#include "common.h"
#include "../../include/drn_hip.h"

#define PP_THREADS 256
#define PP_MAX_L 2048

struct PostParams {
  int nlevels, B, rows_per_clip;
  int row_start[DRN_MAX_GROUPS], L[DRN_MAX_GROUPS];
  float stride[DRN_MAX_GROUPS];
  float thr, downsample;
  int top_n, use_iou;
};

__device__ __forceinline__ float sigmoid_pp(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(PP_THREADS) void postprocess_kernel(const PostParams P, const float* __restrict__ logits,
                                                                 const float* __restrict__ reg, const float* __restrict__ iou,
                                                                 float* __restrict__ det, float* __restrict__ scores,
                                                                 float* __restrict__ locs, int* __restrict__ counts) {
  __shared__ float sc[PP_MAX_L];            // score of candidates, -1 for the rest
  __shared__ unsigned char keep[PP_MAX_L];
  __shared__ int wsum[PP_THREADS / 64], s_total;
  const int b = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  int out_base = 0;                         // kept candidates of the previous levels of this clip
  for (int l = 0; l < P.nlevels; ++l) {
    const int L = P.L[l];
    const long r0 = P.row_start[l] + (long)b * L;
    for (int t = tid; t < L; t += PP_THREADS) {
      const float c = sigmoid_pp(logits[r0 + t]);
      float s = -1.f;
      if (c > P.thr) s = P.use_iou ? c * sigmoid_pp(iou[r0 + t]) : c;
      sc[t] = s;
    }
    __syncthreads();
    // how many candidates?  (block count through ballots)
    int n_c = 0;
    for (int t0 = 0; t0 < L; t0 += PP_THREADS) {
      const int t = t0 + tid;
      const unsigned long long m = __ballot(t < L && sc[t] >= 0.f);
      if (lane == 0) wsum[wv] = __popcll(m);
      __syncthreads();
      n_c += wsum[0] + wsum[1] + wsum[2] + wsum[3];
      __syncthreads();
    }
    // top_n by rank (ties: earlier location first) when there are more candidates than that
    for (int t = tid; t < L; t += PP_THREADS) {
      const float s = sc[t];
      bool k = s >= 0.f;
      if (k && n_c > P.top_n) {
        int rank = 0;
        for (int j = 0; j < L; ++j) {
          const float o = sc[j];
          rank += (o > s) || (o == s && j < t);
        }
        k = rank < P.top_n;
      }
      keep[t] = k;
    }
    __syncthreads();
    // ordered compaction
    int level_kept = 0;
    for (int t0 = 0; t0 < L; t0 += PP_THREADS) {
      const int t = t0 + tid;
      const bool k = t < L && keep[t];
      const unsigned long long m = __ballot(k);
      if (lane == 0) wsum[wv] = __popcll(m);
      __syncthreads();
      int before = __popcll(m & ((1ull << lane) - 1ull));
      for (int q = 0; q < wv; ++q) before += wsum[q];
      const int chunk = wsum[0] + wsum[1] + wsum[2] + wsum[3];
      if (k) {
        const long o = (long)b * P.rows_per_clip + out_base + level_kept + before;
        const float loc = (float)t * P.stride[l] + P.stride[l] * 0.5f;      // model/fcos.py:204-211
        const float d0 = (loc - reg[(r0 + t) * 2 + 0]) / P.downsample, d1 = (loc + reg[(r0 + t) * 2 + 1]) / P.downsample;
        det[o * 2 + 0] = fminf(fmaxf(d0, 0.f), 1.f);
        det[o * 2 + 1] = fminf(fmaxf(d1, 0.f), 1.f);
        scores[o] = sqrtf(sc[t]);
        locs[o] = loc / 32.f;
      }
      level_kept += chunk;
      __syncthreads();
    }
    if (tid == 0) counts[b * P.nlevels + l] = level_kept;
    out_base += level_kept;
    __syncthreads();
  }
}

extern "C" int drn_postprocess(const DrnLossLevel* levels, int nlevels, int B, const float* logits, const float* reg, const float* iou,
                               float thr, int top_n, float downsample, float* det, float* scores, float* locs, int* counts,
                               void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(levels && nlevels >= 1 && nlevels <= DRN_MAX_GROUPS && B > 0, "drn_postprocess: bad level table");
  DRN_CHECK_ARG(logits && reg && det && scores && locs && counts && top_n > 0 && downsample > 0.f, "drn_postprocess: bad args");
  PostParams P;
  memset(&P, 0, sizeof(P));
  P.nlevels = nlevels; P.B = B; P.thr = thr; P.top_n = top_n; P.downsample = downsample; P.use_iou = iou != nullptr;
  int rows = 0, per_clip = 0;
  for (int l = 0; l < nlevels; ++l) {
    DRN_CHECK_ARG(levels[l].L > 0 && levels[l].L <= PP_MAX_L, "drn_postprocess: level %d has %d locations (max %d)", l, levels[l].L, PP_MAX_L);
    P.row_start[l] = rows; P.L[l] = levels[l].L; P.stride[l] = levels[l].stride;
    rows += B * levels[l].L;
    per_clip += levels[l].L;
  }
  P.rows_per_clip = per_clip;
  postprocess_kernel<<<B, PP_THREADS, 0, (hipStream_t)stream>>>(P, logits, reg, iou, det, scores, locs, counts);
  return drn_launch_status("drn_postprocess");
}

// ---------------------------------------------------------------------------------------------------------------------------
// Recall@k at temporal-IoU thresholds with temporal NMS, on the device (utils/evaluate_utils.py:131-215 as driven by
// main.py:324-364): one wavefront per (clip, IoU threshold).  The host evaluator sorts a clip's predictions by score (stable),
// runs a greedy NMS at threshold iou - 0.05 from the highest score down -- score ties go to the LATER prediction -- and counts
// the clip when one of the first k survivors overlaps the ground truth by >= iou (un-clamped IoU).  Only the first
// K = max(k) survivors matter, so no sort is needed: K times, the best candidate still alive is found with a wave reduction
// over (score, index), tested against the ground truth, and everything it suppresses is struck out.  All arithmetic in
// double on the float32 detections, exactly the numbers the host path sees after .tolist().
// out[b][q] = position of the first survivor that hits (0-based), or K when none of the first K does.
// every level table drn_postprocess accepts fits: DRN_MAX_GROUPS levels of at most PP_MAX_L locations
#define ER_MAX_CAND (DRN_MAX_GROUPS * PP_MAX_L)

// The pick loop both wave-per-clip kernels below run: up to K times, find the best candidate still alive -- highest score, ties to
// the LATER index -- call on_pick(p, index, score, x1, x2) with wave-uniform arguments, and strike out everything it suppresses at
// `overlap` (and itself).  `empty`: the clip has no candidates and stands for the single fallback detection (0, 1) with score 1
// (model/inference.py:192-197); n is then 1 and d / s are not read.  Returns the number of picks made.
template <typename F>
__device__ __forceinline__ int nms_pick_loop(unsigned char* alive, const float* __restrict__ d, const float* __restrict__ s, int n,
                                             const bool empty, const double overlap, const int K, const int lane, F on_pick) {
  for (int j = lane; j < n; j += 64) alive[j] = 1;
  __syncthreads();
  int p = 0;
  for (; p < K; ++p) {
    float bs = -1.f;
    int bj = -1;
    for (int j = lane; j < n; j += 64)
      if (alive[j]) {
        const float sj = empty ? 1.f : s[j];
        if (bj < 0 || sj > bs || (sj == bs && j > bj)) { bs = sj; bj = j; }
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oj = __shfl_xor(bj, o, 64);
      if (oj >= 0 && (bj < 0 || os > bs || (os == bs && oj > bj))) { bs = os; bj = oj; }
    }
    if (bj < 0) break;                        // nothing left
    const double x1 = empty ? 0.0 : (double)d[bj * 2], x2 = empty ? 1.0 : (double)d[bj * 2 + 1];
    on_pick(p, bj, bs, x1, x2);
    const double len = x2 - x1;
    for (int j = lane; j < n; j += 64)
      if (alive[j]) {
        const double y1 = (double)d[j * 2], y2 = (double)d[j * 2 + 1];
        const double inter = fmax(0.0, fmin(x2, y2) - fmax(x1, y1));
        const double o = inter / (len + (y2 - y1) - inter);
        if (!(o <= overlap) || j == bj) alive[j] = 0;     // (0/0 = NaN is not <= overlap: struck out, as in the reference)
      }
    __syncthreads();
  }
  return p;
}

__global__ __launch_bounds__(64) void eval_recall_kernel(const float* __restrict__ det, const float* __restrict__ scores,
                                                         const int* __restrict__ counts, int nlevels, int rows_per_clip,
                                                         const void* __restrict__ gt, int gt_f64, const double* __restrict__ ious,
                                                         int K, int* __restrict__ out, int n_iou) {
  __shared__ unsigned char alive[ER_MAX_CAND];
  const int b = blockIdx.x, q = blockIdx.y, lane = threadIdx.x;
  int n = 0;
  for (int l = 0; l < nlevels; ++l) n += counts[b * nlevels + l];
  const float* __restrict__ d = det + (long)b * rows_per_clip * 2;
  const float* __restrict__ s = scores + (long)b * rows_per_clip;
  const double iou_thr = ious[q], overlap = ious[q] - 0.05;
  const double g0 = gt_f64 ? ((const double*)gt)[b * 2] : (double)((const float*)gt)[b * 2];
  const double g1 = gt_f64 ? ((const double*)gt)[b * 2 + 1] : (double)((const float*)gt)[b * 2 + 1];
  const bool empty = n == 0;                 // model/inference.py:192-197: one detection (0, 1) with score 1
  if (empty) n = 1;
  int first_hit = K;
  nms_pick_loop(alive, d, s, n, empty, overlap, K, lane, [&](int p, int, float, double x1, double x2) {
    if (first_hit == K) {
      const double iou = (fmin(g1, x2) - fmax(g0, x1)) / (fmax(g1, x2) - fmin(g0, x1));      // evaluate_utils.py:228-232
      if (iou >= iou_thr) first_hit = p;
    }
  });
  if (lane == 0) out[b * n_iou + q] = first_hit;
}

extern "C" int drn_eval_recall(const float* det, const float* scores, const int32_t* counts, int B, int nlevels, int rows_per_clip,
                               const void* gt, int gt_is_f64, const double* ious, int n_iou, int max_topk, int32_t* first_hit,
                               void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(det && scores && counts && gt && ious && first_hit && B > 0 && nlevels >= 1 && n_iou >= 1 && max_topk >= 1,
                "drn_eval_recall: bad args");
  DRN_CHECK_ARG(rows_per_clip > 0 && rows_per_clip <= ER_MAX_CAND, "drn_eval_recall: %d candidate slots per clip (max %d)", rows_per_clip, ER_MAX_CAND);
  eval_recall_kernel<<<dim3(B, n_iou), 64, 0, (hipStream_t)stream>>>(det, scores, counts, nlevels, rows_per_clip, gt, gt_is_f64, ious,
                                                                     max_topk, first_hit, n_iou);
  return drn_launch_status("drn_eval_recall");
}

// ---------------------------------------------------------------------------------------------------------------------------
// The moments themselves: the first K survivors of that same NMS, best first, one wavefront per clip
// (utils/evaluate_utils.py:91-107 sort + :186-212 nms_temporal; the fallback moment of model/inference.py:192-197 for a clip without
// candidates).  The detections are copied, not recomputed; `level` comes from the running sum of the clip's per-level counts.
__global__ __launch_bounds__(64) void select_moments_kernel(const float* __restrict__ det, const float* __restrict__ scores,
                                                            const int* __restrict__ counts, int nlevels, int rows_per_clip,
                                                            double overlap, int K, float* __restrict__ seg, float* __restrict__ score,
                                                            int* __restrict__ level, int* __restrict__ index, int* __restrict__ n_out) {
  __shared__ unsigned char alive[ER_MAX_CAND];
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = 0;
  for (int l = 0; l < nlevels; ++l) n += counts[b * nlevels + l];
  n = min(n, rows_per_clip);                 // (counts are the post-processor's; a corrupt table must not reach past the clip's slots)
  const float* __restrict__ d = det + (long)b * rows_per_clip * 2;
  const float* __restrict__ s = scores + (long)b * rows_per_clip;
  const bool empty = n <= 0;
  if (empty) n = 1;
  const long o = (long)b * K;
  const int np = nms_pick_loop(alive, d, s, n, empty, overlap, K, lane, [&](int p, int j, float sj, double, double) {
    if (lane != 0) return;
    int lv = -1;
    if (!empty) {
      int end = 0;
      for (lv = 0; lv < nlevels - 1; ++lv) {
        end += counts[b * nlevels + lv];
        if (j < end) break;
      }
    }
    seg[(o + p) * 2 + 0] = empty ? 0.f : d[j * 2];
    seg[(o + p) * 2 + 1] = empty ? 1.f : d[j * 2 + 1];
    score[o + p] = sj;
    level[o + p] = lv;
    index[o + p] = empty ? -1 : j;
  });
  for (int p = np + lane; p < K; p += 64) {
    seg[(o + p) * 2 + 0] = 0.f;
    seg[(o + p) * 2 + 1] = 0.f;
    score[o + p] = 0.f;
    level[o + p] = -1;
    index[o + p] = -1;
  }
  if (lane == 0) n_out[b] = np;
}

extern "C" int drn_select_moments(const float* det, const float* scores, const int32_t* counts, int B, int nlevels, int rows_per_clip,
                                  double overlap, int K, float* seg, float* score, int32_t* level, int32_t* index, int32_t* n,
                                  void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(det && scores && counts && seg && score && level && index && n && B > 0 && nlevels >= 1 && K >= 1,
                "drn_select_moments: bad args");
  DRN_CHECK_ARG(rows_per_clip > 0 && rows_per_clip <= ER_MAX_CAND, "drn_select_moments: %d candidate slots per clip (max %d)", rows_per_clip, ER_MAX_CAND);
  select_moments_kernel<<<B, 64, 0, (hipStream_t)stream>>>(det, scores, counts, nlevels, rows_per_clip, overlap, K, seg, score, level,
                                                           index, n);
  return drn_launch_status("drn_select_moments");
}

// ---------------------------------------------------------------------------------------------------------------------------
// The best K moments of a sentence across videos, streamed chunk by chunk (Grounder.search): one wavefront per sentence merges one
// chunk's select_moments outputs into the sentence's running state, in place.  The K state entries and the chunk's Vc * kv entries
// are staged in LDS -- everything the state holds is read before anything is written -- then, as in nms_pick_loop, up to K times
// the best candidate still alive is found with a wave reduction and struck out.  The order is total: score descending (the stored
// floats), video position ascending, rank ascending (and the staging slot, for a video listed twice), so the result does not
// depend on how the videos were cut into chunks.  No candidates: padded chunk slots (vids outside [0, Nv)), the fallback moment
// (index < 0, score 1: it would top every ranking), entries past n[p], scores that are not finite.
#define MM_MAX_CAND DRN_MERGE_MAX_CAND

// does candidate (s1, v1, r1, i1) come before (s2, v2, r2, i2)?  i < 0: no candidate
__device__ __forceinline__ bool mm_before(float s1, int v1, int r1, int i1, float s2, int v2, int r2, int i2) {
  if (i1 < 0) return false;
  if (i2 < 0) return true;
  if (s1 != s2) return s1 > s2;
  if (v1 != v2) return v1 < v2;
  if (r1 != r2) return r1 < r2;
  return i1 < i2;
}

// LDS of one merging wavefront: the staged candidates' score, segment, video position, level and rank, and who is still alive.
struct MmLds {
  float *score, *seg;
  int *video, *level, *rank;
  unsigned char* alive;
};
#define MM_LDS_DECL(L)                                                                   \
  __shared__ float mm_score[MM_MAX_CAND], mm_seg[MM_MAX_CAND * 2];                       \
  __shared__ int mm_video[MM_MAX_CAND], mm_level[MM_MAX_CAND], mm_rank[MM_MAX_CAND];     \
  __shared__ unsigned char mm_alive[MM_MAX_CAND];                                        \
  const MmLds L = {mm_score, mm_seg, mm_video, mm_level, mm_rank, mm_alive}

// What both merge kernels run for sentence s: stage its K state entries and the cnt * kv entries of its cnt pairs, then pick.
// pair_of(slot, p, v): the chunk's pair index and the store position of the sentence's slot-th pair.  K + cnt * kv <= MM_MAX_CAND is
// the caller's to guarantee.
template <typename PairOf>
__device__ __forceinline__ void mm_merge_sentence(const MmLds c, const float* __restrict__ seg, const float* __restrict__ score,
                                                  const int* __restrict__ level, const int* __restrict__ index,
                                                  const int* __restrict__ n_in, const int s, const int cnt, const int kv, const int Nv,
                                                  const int K, const bool fresh, float* st_seg, float* st_score, int* st_video,
                                                  int* st_level, int* st_rank, int* st_n, const int lane, PairOf pair_of) {
  const long o = (long)s * K;
  const int ns = fresh ? 0 : min(max(st_n[s], 0), K);
  const int N = K + cnt * kv;
  for (int i = lane; i < N; i += 64) {
    bool ok;
    long src = 0;
    int v = -1, r = 0;
    if (i < K) {
      ok = i < ns;
      src = o + i;
      if (ok) { v = st_video[src]; r = st_rank[src]; }
    } else {
      const int e = i - K, slot = e / kv;
      r = e - slot * kv;
      long p;
      pair_of(slot, p, v);
      src = p * kv + r;
      ok = v >= 0 && v < Nv && r < n_in[p] && index[src] >= 0;
    }
    float sc = 0.f;
    if (ok) {
      sc = i < K ? st_score[src] : score[src];
      ok = isfinite(sc);
    }
    if (ok) {
      c.score[i] = sc;
      c.video[i] = v;
      c.rank[i] = r;
      c.seg[i * 2 + 0] = i < K ? st_seg[src * 2 + 0] : seg[src * 2 + 0];
      c.seg[i * 2 + 1] = i < K ? st_seg[src * 2 + 1] : seg[src * 2 + 1];
      c.level[i] = i < K ? st_level[src] : level[src];
    }
    c.alive[i] = ok;
  }
  __syncthreads();
  int np = 0;
  for (; np < K; ++np) {
    float bs = 0.f;
    int bv = 0, br = 0, bi = -1;
    for (int i = lane; i < N; i += 64)
      if (c.alive[i] && mm_before(c.score[i], c.video[i], c.rank[i], i, bs, bv, br, bi)) {
        bs = c.score[i]; bv = c.video[i]; br = c.rank[i]; bi = i;
      }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
      const float os = __shfl_xor(bs, w, 64);
      const int ov = __shfl_xor(bv, w, 64), orr = __shfl_xor(br, w, 64), oi = __shfl_xor(bi, w, 64);
      if (mm_before(os, ov, orr, oi, bs, bv, br, bi)) { bs = os; bv = ov; br = orr; bi = oi; }
    }
    if (bi < 0) break;                        // nothing left
    if (lane == 0) {
      st_seg[(o + np) * 2 + 0] = c.seg[bi * 2 + 0];
      st_seg[(o + np) * 2 + 1] = c.seg[bi * 2 + 1];
      st_score[o + np] = bs;
      st_video[o + np] = bv;
      st_level[o + np] = c.level[bi];
      st_rank[o + np] = br;
      c.alive[bi] = 0;
    }
    __syncthreads();
  }
  for (int p = np + lane; p < K; p += 64) {
    st_seg[(o + p) * 2 + 0] = 0.f;
    st_seg[(o + p) * 2 + 1] = 0.f;
    st_score[o + p] = 0.f;
    st_video[o + p] = -1;
    st_level[o + p] = -1;
    st_rank[o + p] = -1;
  }
  if (lane == 0) st_n[s] = np;
}

__global__ __launch_bounds__(64) void merge_moments_kernel(const float* __restrict__ seg, const float* __restrict__ score,
                                                           const int* __restrict__ level, const int* __restrict__ index,
                                                           const int* __restrict__ n_in, int Vc, int kv, const int* __restrict__ vids,
                                                           int Nv, int K, int first, const int* __restrict__ first_dev,
                                                           float* st_seg, float* st_score, int* st_video, int* st_level, int* st_rank,
                                                           int* st_n) {
  MM_LDS_DECL(c);
  const int s = blockIdx.x;
  const bool fresh = first_dev ? first_dev[0] != 0 : first != 0;
  // (K + Vc * kv <= MM_MAX_CAND: checked by the host)
  mm_merge_sentence(c, seg, score, level, index, n_in, s, Vc, kv, Nv, K, fresh, st_seg, st_score, st_video, st_level, st_rank, st_n,
                    threadIdx.x, [&](int slot, long& p, int& v) {
                      p = (long)s * Vc + slot;
                      v = vids[slot];
                    });
}

extern "C" int drn_merge_moments(const float* seg, const float* score, const int32_t* level, const int32_t* index, const int32_t* n,
                                 int S, int Vc, int kv, const int32_t* vids, int Nv, int K, int first, const int32_t* first_dev,
                                 float* st_seg, float* st_score, int32_t* st_video, int32_t* st_level, int32_t* st_rank, int32_t* st_n,
                                 void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(seg && score && level && index && n && vids && st_seg && st_score && st_video && st_level && st_rank && st_n,
                "drn_merge_moments: null pointer");
  DRN_CHECK_ARG(S > 0 && Vc > 0 && Nv >= 0, "drn_merge_moments: bad args (S = %d sentences, Vc = %d chunk slots, Nv = %d videos)", S, Vc, Nv);
  DRN_CHECK_ARG(K >= 1, "drn_merge_moments: K = %d, at least 1 moment per sentence", K);
  DRN_CHECK_ARG(kv >= 1, "drn_merge_moments: kv = %d, at least 1 slot per pair", kv);
  DRN_CHECK_ARG((long)K + (long)Vc * kv <= MM_MAX_CAND, "drn_merge_moments: K + Vc * kv = %ld candidates per sentence (max %d)",
                (long)K + (long)Vc * kv, MM_MAX_CAND);
  DRN_CHECK_ARG((long)S * Vc * kv <= 0x7fffffffL, "drn_merge_moments: more than 2^31 chunk entries");
  merge_moments_kernel<<<S, 64, 0, (hipStream_t)stream>>>(seg, score, level, index, n, Vc, kv, vids, Nv, K, first, first_dev, st_seg,
                                                          st_score, st_video, st_level, st_rank, st_n);
  return drn_launch_status("drn_merge_moments");
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same ranking for a chunk of P pairs in ANY assignment to sentences (Grounder.search(candidates=)): sentence s owns the pairs
// [pair_off[s], pair_off[s + 1]) of the chunk and pair p is the video at store position pair_video[p].  Nothing read from pair_off is
// trusted: the offsets are clamped to [0, P], a negative or decreasing range is empty and a range longer than the LDS holds is cut,
// so a bad table ranks the wrong pairs but indexes nothing outside LDS or the inputs.  A sentence without a pair in the chunk re-ranks
// its own state, which is the identity.
__global__ __launch_bounds__(64) void merge_moments_ragged_kernel(const float* __restrict__ seg, const float* __restrict__ score,
                                                                  const int* __restrict__ level, const int* __restrict__ index,
                                                                  const int* __restrict__ n_in, int P, int kv,
                                                                  const int* __restrict__ pair_video, const int* __restrict__ pair_off,
                                                                  int Nv, int K, int first, const int* __restrict__ first_dev,
                                                                  float* st_seg, float* st_score, int* st_video, int* st_level,
                                                                  int* st_rank, int* st_n) {
  MM_LDS_DECL(c);
  const int s = blockIdx.x;
  const bool fresh = first_dev ? first_dev[0] != 0 : first != 0;
  const int lo = min(max(pair_off[s], 0), P), hi = min(max(pair_off[s + 1], 0), P);
  const int cnt = min(max(hi - lo, 0), (MM_MAX_CAND - K) / kv);          // (K + kv <= MM_MAX_CAND: checked by the host)
  mm_merge_sentence(c, seg, score, level, index, n_in, s, cnt, kv, Nv, K, fresh, st_seg, st_score, st_video, st_level, st_rank, st_n,
                    threadIdx.x, [&](int slot, long& p, int& v) {
                      p = lo + slot;                                     // (< lo + cnt <= hi <= P)
                      v = pair_video[p];
                    });
}

extern "C" int drn_merge_moments_ragged(const float* seg, const float* score, const int32_t* level, const int32_t* index,
                                        const int32_t* n, int S, int P, int kv, const int32_t* pair_video, const int32_t* pair_off, int Nv,
                                        int K, int first, const int32_t* first_dev, float* st_seg, float* st_score, int32_t* st_video,
                                        int32_t* st_level, int32_t* st_rank, int32_t* st_n, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(seg && score && level && index && n && pair_video && pair_off && st_seg && st_score && st_video && st_level &&
                    st_rank && st_n,
                "drn_merge_moments_ragged: null pointer");
  DRN_CHECK_ARG(S > 0 && P > 0 && Nv >= 0, "drn_merge_moments_ragged: bad args (S = %d sentences, P = %d pairs, Nv = %d videos)", S, P, Nv);
  DRN_CHECK_ARG(K >= 1, "drn_merge_moments_ragged: K = %d, at least 1 moment per sentence", K);
  DRN_CHECK_ARG(kv >= 1, "drn_merge_moments_ragged: kv = %d, at least 1 slot per pair", kv);
  DRN_CHECK_ARG((long)K + (long)kv <= MM_MAX_CAND, "drn_merge_moments_ragged: K + kv = %ld candidates for one pair (max %d)",
                (long)K + (long)kv, MM_MAX_CAND);
  DRN_CHECK_ARG((long)P * kv <= 0x7fffffffL, "drn_merge_moments_ragged: more than 2^31 chunk entries");
  merge_moments_ragged_kernel<<<S, 64, 0, (hipStream_t)stream>>>(seg, score, level, index, n, P, kv, pair_video, pair_off, Nv, K, first,
                                                                 first_dev, st_seg, st_score, st_video, st_level, st_rank, st_n);
  return drn_launch_status("drn_merge_moments_ragged");
}

// ---------------------------------------------------------------------------------------------------------------------------
// Corpus recall of a search: where, in a sentence's Hits, does the right moment of the right video first appear?  One wavefront
// per sentence; only the first m = min(max(n[s], 0), K) entries are read.  Column i < I: the first position whose video is the
// ground truth's and whose un-clamped tIoU with the ground truth (eval_recall_kernel's expression, in double on the float32
// segment) is >= ious[i]; a NaN among the four bounds is no hit (fmin / fmax would drop it and call the pair identical).  Column I:
// the number of DISTINCT videos ranked before the first entry of the ground truth's video -- its position in the video ranking,
// whatever per_video was.  K where there is none.  The video column is staged in LDS for the distinct count.
__global__ __launch_bounds__(64) void search_recall_kernel(const float* __restrict__ seg, const int* __restrict__ video,
                                                           const int* __restrict__ n, const int* __restrict__ gt_video,
                                                           const void* __restrict__ gt, int gt_f64, const double* __restrict__ ious,
                                                           int K, int I, int* __restrict__ out) {
  __shared__ int vcol[MM_MAX_CAND];
  const int s = blockIdx.x, lane = threadIdx.x;
  const long o = (long)s * K;
  const int m = min(max(n[s], 0), K);          // (K <= MM_MAX_CAND: checked by the host)
  const int gv = gt_video[s];
  for (int p = lane; p < m; p += 64) vcol[p] = video[o + p];
  __syncthreads();
  const double g0 = gt_f64 ? ((const double*)gt)[s * 2] : (double)((const float*)gt)[s * 2];
  const double g1 = gt_f64 ? ((const double*)gt)[s * 2 + 1] : (double)((const float*)gt)[s * 2 + 1];
  const bool gt_ok = gv >= 0 && !(g0 != g0) && !(g1 != g1);
  int* __restrict__ row = out + (long)s * (I + 1);
  for (int i = 0; i < I; ++i) {
    const double thr = ious[i];
    int first = K;
    if (gt_ok)
      for (int p = lane; p < m; p += 64) {
        if (vcol[p] != gv) continue;
        const double x1 = (double)seg[(o + p) * 2], x2 = (double)seg[(o + p) * 2 + 1];
        if (x1 != x1 || x2 != x2) continue;
        const double iou = (fmin(g1, x2) - fmax(g0, x1)) / (fmax(g1, x2) - fmin(g0, x1));
        if (iou >= thr) { first = p; break; }  // (a lane's positions ascend: its first hit is its smallest)
      }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) first = min(first, __shfl_xor(first, w, 64));
    if (lane == 0) row[i] = first;
  }
  int p0 = m;
  if (gv >= 0)
    for (int p = lane; p < m; p += 64)
      if (vcol[p] == gv) { p0 = p; break; }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) p0 = min(p0, __shfl_xor(p0, w, 64));
  const bool found = p0 < m;                   // (wave-uniform; gv < 0 leaves p0 = m)
  int distinct = 0;                            // entries before p0 that are the first of their video
  for (int p = lane; found && p < p0; p += 64) {
    const int v = vcol[p];
    bool seen = false;
    for (int j = 0; j < p && !seen; ++j) seen = vcol[j] == v;
    distinct += !seen;
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) distinct += __shfl_xor(distinct, w, 64);
  if (lane == 0) row[I] = found ? distinct : K;
}

extern "C" int drn_search_recall(const float* seg, const int32_t* video, const int32_t* n, const int32_t* gt_video, const void* gt,
                                 int gt_is_f64, const double* ious, int S, int K, int I, int32_t* first_hit, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(S >= 1, "drn_search_recall: S = %d, at least 1 sentence", S);
  DRN_CHECK_ARG(K >= 1, "drn_search_recall: K = %d, at least 1 hit slot per sentence", K);
  DRN_CHECK_ARG(I >= 1, "drn_search_recall: I = %d, at least 1 IoU threshold", I);
  DRN_CHECK_ARG(K <= MM_MAX_CAND, "drn_search_recall: K = %d hit slots per sentence (max %d)", K, MM_MAX_CAND);
  DRN_CHECK_ARG(seg && video && n && gt_video && gt && ious && first_hit, "drn_search_recall: null pointer");
  search_recall_kernel<<<S, 64, 0, (hipStream_t)stream>>>(seg, video, n, gt_video, gt, gt_is_f64, ious, K, I, first_hit);
  return drn_launch_status("drn_search_recall");
}
