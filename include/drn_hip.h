/* libdrn_hip.so -- C-ABI of the MI355X (gfx950) DRN hot path.
 *
 * The reference (Alvin-Zeng/DRN) has no FFI on this path except the third-party
 * pybind extension fcos_core._C (model/layers/sigmoid_focal_loss.py:18,31); every
 * other entry point below replaces a stock ATen/cuDNN call made from the
 * reference's Python modules (file:line cited per function).  Conventions:
 *   - extern "C", plain pointers/ints, no torch types; caller owns every buffer
 *     (including workspaces); raw DEVICE pointers unless a parameter says "host";
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream);
 *     kernels are asynchronous on it, never synchronise, never allocate;
 *   - return 0 on success, negative on error (see drn_last_error()); never
 *     throws or aborts across the ABI; re-entrant (one process per GPU).
 *   - dtype: 0 = float32 (exact f32 MFMA, parity mode), 1 = bfloat16 storage
 *     with fp32 accumulation.  Activations are channels-last ("NLC"): row
 *     m = (sequence, t), C contiguous, explicit row stride in elements.
 */
#ifndef DRN_HIP_H
#define DRN_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRN_ABI_VERSION 9
#define DRN_MAX_GROUPS 4

int drn_abi_version(void);
/* TEST / EXPERIMENT switches, process-wide; nothing on the product path (drn_amd/*.py outside tests) calls this.  They let tests reach
 * kernels their shapes would not select: "tn3_minrows" (fewest rows for the fused-tap weight-gradient kernel, default 4096), "tn_fused"
 * (0 switches that kernel off), "nt_w4" (0: drn_gemm_nt runs the general 8-wave kernel also for the large plain bf16 products that
 * gemm_nt_w4_kernel takes by default; results are bit-identical either way), "nt_w4c" / "nt_w4h" (the same for the k = 3 convolutions on
 * 256x256 tiles and the 256x128-tile kernel), "nt_deep*", "bn1_maxwg", "w4h_tapil", "exp0".."exp4" (launch heuristics, 0 = shipped).
 * Per-launch behaviour (the split-K exchange's confirmation, deferred weight-gradient reduces) is NOT here: it travels in the call's own
 * arguments (DRN_KSPLIT_CONFIRM_*, DrnWgradPending).  The library never reads the environment. */
int drn_tune(const char* key, int value);
const char* drn_last_error(void); /* thread-local, valid until the next failing call on this thread */

/* One problem of a grouped implicit-GEMM launch:  C[M][N] (+)= A'(M x K) * B[N][K]^T
 * where K = taps*Cin and A' is the im2col view of a channels-last tensor A:
 *   mode 0 (forward, model/basic_blocks.py:9-18 Conv1d / nn.Linear when taps==1):
 *       row m=(seq,t), column (tap,c) reads A[seq*Lsrc + t*stride + tap - pad][c]
 *   mode 1 (data gradient of the same conv):
 *       reads A[seq*Lsrc + (t + pad - tap)/stride][c] when divisible and in range
 *   out-of-range taps read zero.  B is [N][taps*Cin] (K contiguous).
 * Epilogue: + bias[n];  optional second output C2 = value before gating;
 *   * gate[(m / Lout)*ldg + n]  (query gating, model/backbone.py:28-30);
 *   per-128-row-slab BatchNorm statistics in (sum, M2) form: stats[(slab*2 + 0)*N + n] = sum of the slab's rows,
 *   stats[(slab*2 + 1)*N + n] = sum of squared deviations from the SLAB mean (merged by drn_bn_finalize with the
 *   parallel-variance formula: no E[x^2]-E[x]^2 cancellation) -- deterministic, no atomics.
 */
typedef struct DrnGemmDesc {
  const void* A;
  const void* B;
  void* C;
  void* C2;          /* optional pre-gate copy of C (row stride ldc2), or NULL */
  const float* bias; /* [N] fp32 or NULL */
  const float* gate; /* [(M/Lout)][ldg] fp32 or NULL */
  float* stats;      /* [ceil(M/128)][2][N] fp32 or NULL */
  int32_t M, N;
  int32_t Cin, taps, stride, pad, mode;
  int32_t Lout, Lsrc;
  int32_t lda, ldb, ldc, ldg;
  int32_t accumulate; /* 1: C += result */
  int32_t ldc2;       /* row stride of C2 */
  int32_t out_f32;    /* 1: C is fp32 [M][ldc] regardless of dtype (no C2 / gate / stats): weight gradients as an NT product */
  float* sumsq;       /* or NULL.  out_f32 launches on gemm_nt_w4_kernel only (drn_gemm_nt_plan says DRN_NT_KIND_W4; no bias / accumulate):
                       * sumsq[t] = sum of the squares of output tile t's values (256x256 tiles in launch order, (M/256)*(N/256) floats):
                       * the gradient's contribution to the global norm without reading it again (drn_sumsq_finalize2) */
  /* gb_act != NULL: a data gradient (mode 1, k = 3 / stride 1) whose consumer is the input stage's gate backward (drn_gate_bwd_t;
   * model/backbone.py:28-30 on prop_fc's output): C is NOT written; with g = the product rounded to dtype, s = m / Lout,
   *   gb_dct[c][m] = dtype(g[m][c] * gate[s][c])   (row stride gb_ldt: the K-major operand of prop_fc's weight gradient),
   *   gb_dgate[s][c] = sum_t g * gb_act[m][c]       ([M / Lout][N] fp32; gb_act: the pre-gate activation, row stride gb_ld_act),
   *   gb_dsum[s][c]  = sum_t g * gate[s][c]         ([M / Lout][N] fp32: per-clip column sums, the bias gradient's partials).
   * bf16 launches on gemm_nt_w4c_kernel only (drn_gemm_nt_plan says DRN_NT_KIND_W4C), Lout in {32, 64, 128, 256}, gate set,
   * no bias / C2 / stats / accumulate; one problem per launch. */
  const void* gb_act;
  void* gb_dct;
  float* gb_dgate;
  float* gb_dsum;
  int32_t gb_ld_act, gb_ldt;
} DrnGemmDesc;

/* Grouped NT implicit GEMM on MFMA (conv1d fwd / dgrad, linear fwd / dgrad).
 * Replaces nn.Linear (model/main_model.py:59), nn.Conv1d (model/basic_blocks.py:9,
 * model/fcos.py:33,37,59,65) forward and their input gradients. */
int drn_gemm_nt(const DrnGemmDesc* descs /*host*/, int ngroups, int dtype, void* stream);
/* Which kernel drn_gemm_nt would run these problems on (no launch; arguments validated the same way): >= 0 one of the kinds
 * below, < 0 an error code.  For callers that schedule around a launch (functional.input_prep pre-touches the prop_fc weight
 * only when the general kernel runs) instead of re-deriving the library's rule. */
#define DRN_NT_KIND_TILE128 0  /* conv_gemm_nt_kernel, 128x128 tiles */
#define DRN_NT_KIND_TILE256 1  /* conv_gemm_nt_kernel, 256x256 tiles */
#define DRN_NT_KIND_W4 2       /* gemm_nt_w4_kernel: large plain bf16 products, 4 waves, 5-slot ring */
#define DRN_NT_KIND_W4C 3      /* gemm_nt_w4c_kernel: the same loop for k = 3 / stride 1 convolutions */
#define DRN_NT_KIND_W4H 4      /* gemm_nt_w4h_kernel: the same loop on 256x128 tiles (N too narrow to fill the chip with 256x256) */
int drn_gemm_nt_plan(const DrnGemmDesc* descs /*host*/, int ngroups, int dtype);
/* ... and which kernel drn_gemm_nt_splitk / _grouped would run them on with the K loop split ksplit ways. */
int drn_gemm_nt_splitk_plan(const DrnGemmDesc* descs /*host*/, int ngroups, int ksplit, int dtype);
/* Same for ONE problem with the K loop split `ksplit` ways (few output tiles: conv0, the coarse pyramid levels), in ONE
 * launch: every split publishes its fp32 partial tile in ws (drn_gemm_nt_splitk_ws_elems floats, 16-byte aligned), the
 * split that arrives last at a tile adds them in split order (deterministic) and runs the epilogue.  counters: >= one int32
 * per 128x128 output tile (<= DRN_QD_COUNTERS), zero on entry, left zero (the buffer drn_skinny_group uses will do). */
/* `ksplit` = the split count (1..64) in the low 16 bits, optionally OR-ed with ONE of the bits below: how a split confirms its
 * write-through partial-tile stores before it takes the tile's ticket.  No bit (what drn_amd.ops passes): an sc1 load of every stored
 * 64-byte request -- needed whenever a kernel of another queue may run beside the launch (a copy stream, a second graph branch, RCCL),
 * which the library cannot rule out; + 12 us per training step at T = 256.  _ATOMIC: a returning agent-scope read-modify-write per
 * request instead (+ 76 us per step).  _NONE: nothing -- only for a caller that owns the device's every queue (experiments, stress
 * tests).  Values are identical in every mode. */
#define DRN_KSPLIT_CONFIRM_ATOMIC 0x20000
#define DRN_KSPLIT_CONFIRM_NONE   0x80000
int64_t drn_gemm_nt_splitk_ws_elems(int M, int N, int ksplit);
int drn_gemm_nt_splitk(const DrnGemmDesc* desc /*host*/, int ksplit, float* ws, int32_t* counters, int dtype, void* stream);
/* ... and for a grouped launch: every problem's K loop is split ksplit ways; ws >= ksplit * (sum over the problems of their
 * 128x128 output tiles) * 16384 floats, one counter per tile of the launch. */
int drn_gemm_nt_splitk_grouped(const DrnGemmDesc* descs /*host*/, int ngroups, int ksplit, float* ws, int32_t* counters, int dtype,
                               void* stream);

/* ... and for ONE long-K k = 3 / stride 1 convolution with few output tiles (conv0's forward) on full-width 256x256 tiles in two
 * launches: every split writes its fp32 partial product as plane `split` of ws (drn_gemm_nt_splitk256_ws_elems floats), a second
 * kernel adds the planes in split order (+ bias), writes C and the per-128-row-slab BatchNorm statistics.  bf16 only, M and N
 * multiples of 256, Cin of 64, at least 2 K-steps of 64 per split; no gate / C2 / accumulate / out_f32 (DRN_ERR_UNSUPPORTED). */
int64_t drn_gemm_nt_splitk256_ws_elems(int M, int N, int ksplit);
int drn_gemm_nt_splitk256(const DrnGemmDesc* desc /*host*/, int ksplit, float* ws, int dtype, void* stream);

/* Weight gradient:  dW[n][tap][c] (fp32) = sum_m dY[m][n] * X[src(m,tap)][c]   (mode-0 addressing of X).
 * dW is written as [N][taps][Cin] when w_layout==0 or [N][Cin][taps] (the nn.Conv1d parameter layout) when 1.
 * Grouped: the same dW accumulates over all groups (shared-weight heads, model/fcos.py:93-102).
 * `ws` is an fp32 workspace of drn_wgrad_ws_elems(...) elements (split over rows, reduced deterministically). */
typedef struct DrnWgradDesc {
  const void* dY; /* [M][N] */
  const void* X;  /* channels-last source */
  int32_t M, Lout, Lsrc;
  int32_t ldy, ldx;
} DrnWgradDesc;
/* bf16, taps == 3, stride == 1, pad == 1, Lsrc == Lout and >= 4096 rows run the fused-tap kernel (one staged X block
 * feeds all three taps); everything else the per-tap kernel.  Same results to fp32 rounding (the split points differ).
 * drn_tune("tn_fused", 0) disables the fused-tap kernel, "tn3_minrows" sets its row threshold (tests). */
int64_t drn_wgrad_ws_elems(int M_total, int N, int Cin, int taps);

/* Deferred reduce passes.  A weight-gradient launch that splits its rows ends with a reduce launch of its own -- unless the caller hands
 * it a DrnWgradPending list (HOST memory the caller owns; all-zero = empty; nothing about it lives in the library, so two models or two
 * threads use two lists): the launch then only RECORDS its reduce, and drn_wgrad_reduce_pending() runs every recorded one in ONE launch
 * (same summation order over the splits: same bits) and empties the list.  The caller keeps the workspaces alive until then and flushes
 * before anything reads the gradients.  Not recorded (reduced at once, as with pend = NULL): an accumulating reduce (it reads `out`), and
 * anything once the list holds DRN_WGRAD_PEND_MAX items.  An output that ALREADY has a reduce recorded in the list is an error
 * (DRN_ERR_ARG before anything is launched): flush in between. */
#define DRN_WGRAD_PEND_MAX 24
typedef struct DrnWgradPendItem {
  const float* ws; /* [nsplit][N][taps][Cin] partials */
  float* out;      /* the gradient */
  int32_t nsplit, N, Cin, taps, w_layout, accumulate;
} DrnWgradPendItem;
typedef struct DrnWgradPending {
  DrnWgradPendItem it[DRN_WGRAD_PEND_MAX];
  int32_t blk_start[DRN_WGRAD_PEND_MAX + 1]; /* filled by the library when it plans the flush */
  int32_t n;                                  /* items recorded */
  float* sumsq;                               /* set for the duration of a flush */
} DrnWgradPending;

int drn_gemm_wgrad(const DrnWgradDesc* descs /*host*/, int ngroups, float* dW, int N, int Cin, int taps, int stride,
                   int pad, int w_layout, int accumulate, float* ws, int dtype, DrnWgradPending* pend /*host or NULL*/, void* stream);

/* n independent weight gradients of equal N / taps / stride / pad (different weights, different row counts: the FPN level
 * convs) in one launch; dWs is a HOST array of n device pointers; ws >= n * drn_wgrad_ws_elems(max M, N, Cin, taps).
 * Cins (host, or NULL): the problems' own input-channel counts when they differ (the FPN 1x1 laterals: 256 / 512 / 1024 -> 512);
 * Cin is then the largest of them. */
int drn_gemm_wgrad_multi(const DrnWgradDesc* problems /*host*/, int n, float* const* dWs /*host*/, int N, int Cin,
                         const int32_t* Cins /*host*/, int taps, int stride, int pad, int w_layout, int accumulate, float* ws,
                         int dtype, DrnWgradPending* pend /*host or NULL*/, void* stream);
/* The flush: one launch on `stream`; sumsq (device, drn_wgrad_pending_blocks(pend) floats, or NULL) receives one partial per workgroup of
 * the squared sums of what it wrote.  drn_wgrad_pending_bytes: partials read + gradients written by that flush (its HBM roofline
 * denominator). */
int drn_wgrad_pending_blocks(DrnWgradPending* pend);
int64_t drn_wgrad_pending_bytes(const DrnWgradPending* pend);
int drn_wgrad_reduce_pending(DrnWgradPending* pend, float* sumsq, void* stream);

/* ---- HBM-bound helpers (drn_amd/csrc/elementwise.hip) -------------------------------------------------- */
/* fp32 -> dtype cast of n contiguous elements (feature tensor / weights; the reference is fp32-only). */
int drn_cast(const float* in, void* out, int64_t n, int dtype, void* stream);
/* out[a][b][c] (dtype) = in[a*sa + b*sb + c*sc] (fp32): re-lays nn.Conv1d weights (Cout,Cin,k) as the GEMM's
 * B operands [Cout][k][Cin] (forward) and [Cin][k][Cout] (data gradient). */
/* out[k][m] = in[m][k] for a row-major M x K matrix of dtype elements (row strides ld_in / ld_out): K-major copies of the
 * operands let the largest weight gradient run as an NT product (see drn_amd/functional.py, _InputStageFn). */
/* out[m][k] = outT[k][m] = (dtype) in[m][k] for a contiguous fp32 M x K matrix: cast and K-major copy in one pass. */
int drn_cast_transpose(const float* in, void* out, void* outT, int M, int K, int dtype, void* stream);
/* The same pass with at most max_workgroups workgroups resident (a grid-stride loop over the tiles): for schedules that run it
 * BESIDE latency-bound launches of another branch (drn_amd.graph.ForkedStep: the query encoder's forward), which a full-rate
 * streaming pass next to them stretches 2-3 x. */
int drn_cast_transpose_throttled(const float* in, void* out, void* outT, int M, int K, int dtype, int max_workgroups, void* stream);
int drn_transpose2d(const void* in, int ld_in, void* out, int ld_out, int M, int K, int dtype, void* stream);
int drn_pack_weight(const float* in, void* out, int A, int B, int C, int64_t sa, int64_t sb, int64_t sc, int dtype, void* stream);
/* The same for n weights in one launch (all GEMM operands of the model after an optimizer step; the reference's cuDNN
 * re-lays its filters inside every call). */
typedef struct {
  const float* in;
  void* out;
  int64_t sa, sb, sc;
  int32_t A, B, C;
  int64_t ldo; /* elements between consecutive (a,b) rows of out; 0 = contiguous (C) */
} DrnPackDesc;
int drn_pack_weights(const DrnPackDesc* items /*host*/, int n, int dtype, void* stream);
/* Read `bytes` (16-byte aligned buffer) through the caches and discard: warms an operand that was written long ago (the
 * bf16 weight copy of prop_fc) right before the GEMM that streams it. */
int drn_touch(const void* p, int64_t bytes, void* stream);
/* n <= DRN_COPY_MAX device byte ranges copied dst[i] <- src[i] (src[i] NULL: zero-filled) in ONE launch: the refill of a captured
 * step's static input buffers between two hipGraph replays (drn_amd.trainer; replaces the reference loop's per-tensor .cuda()
 * copies, main.py:214-217, on device-resident batches).  Ranges must not overlap. */
#define DRN_COPY_MAX 8
/* rows2d (host, 3 ints per range, or NULL): {row_bytes, src_pitch, dst_pitch} > 0 makes range i two-dimensional -- bytes[i] =
 * rows * dst_pitch bytes of dst are written, the first row_bytes of every row from src rows src_pitch apart, the rest zero (a
 * token matrix padded out to the captured step's query length). */
int drn_copy_multi(const void* const* srcs /*host array of device ptrs*/, void* const* dsts, const int64_t* bytes /*host*/,
                   const int32_t* rows2d /*host or NULL*/, int n, void* stream);
/* feat[m][3] = (float)[start, end, end - start] from props_start_end (M x 2, fp64 or fp32): the position features of
 * model/main_model.py:51-55 in one launch (the reference: subtraction, torch.cat, .float()). */
int drn_pos_feat(const void* start_end, int is_f64, float* feat, int M, void* stream);
/* position_transform = nn.Linear(3,256) on [start,end,duration] (model/main_model.py:34,51-55), written straight
 * into the channel slice of conv0's input (replaces torch.cat at model/backbone.py:31-32). */
int drn_pos_embed_fwd(const float* feat /*[M][3]*/, const float* W /*[C][3]*/, const float* b, void* out, int ld_out, int M, int C,
                      int dtype, void* stream);
int drn_pos_embed_bwd(const void* dout, int ld, const float* feat, int M, int C, float* dW, float* db, int accumulate,
                      float* ws /* >= 1024*C floats */, int dtype, void* stream);
/* The same two gradients taken THROUGH the convolution that reads the embedding as the last P of its Cin input channels
 * (model/backbone.py:31-32 cat -> forward_conv0), from the gradient dY (B*Lo rows x Cout) at that conv's output, so that the conv's
 * input-gradient product can leave those P columns out:  Q[tap][j][o] = sum_rows dY[s,to,o] * f[s*L + to*stride - pad + tap][j]
 * (f[.][3] = 1, rows outside [0, L) skipped), dW[c][j] = sum_{tap,o} Wd[c][tap*Cout + o] * Q[tap][j][o], db[c] = column j = 3.
 * Wd: row Cin-P of the (Cin, k, Cout) copy of the conv weight in `dtype` (ldw elements between rows); k = 1 or 3;
 * ws >= drn_conv_tail_bwd_ws_elems(B*Lo, k, Cout) floats. */
int64_t drn_conv_tail_bwd_ws_elems(int M, int k, int Cout);
int drn_conv_tail_bwd(const void* dY, int ld_dy, int B, int Lo, int Cout, const void* Wd, int64_t ldw, int k, int stride, int pad,
                      const float* feat /*[B*L][3]*/, int L, int P, float* dW /*[P][3]*/, float* db /*[P]*/, int accumulate,
                      float* ws, int dtype, void* stream);
/* backward of F.interpolate(nearest, x2) + add (model/FPN.py:63-68): dst[s,t] += src[s,2t] + src[s,2t+1] */
int drn_pairsum_add(void* dst, int ld_dst, const void* src, int ld_src, int Mdst, int C, int accumulate, int dtype, void* stream);
/* out-of-place form: dst[s,t] = base[s,t] + src[s,2t] + src[s,2t+1] (base = the level's own incoming gradient) */
int drn_pairsum_add_to(void* dst, int ld_dst, const void* base, int ld_base, const void* src, int ld_src, int Mdst, int C,
                       int dtype, void* stream);
/* both steps of a three-level pyramid in one launch: d1 = own1 + pairs(d0) (M1 rows), d2 = own2 + pairs(d1) (M1 / 2 rows); the bits
 * of two drn_pairsum_add_to launches */
int drn_pairsum_chain3(const void* d0, int ld0, const void* own1, int ldo1, void* d1, int ld1, const void* own2, int ldo2, void* d2,
                       int ld2, int M1, int C, int dtype, void* stream);
/* out[s,t,c] = z[s,t,c] * gate[s,c]: the level-0 query gate (model/backbone.py:28-30 on prop_fc's output) as its own pass, for
 * the schedule that runs the query encoder beside the prop_fc GEMM (otherwise drn_gemm_nt's epilogue applies the gate). */
int drn_gate_fwd(const void* z, int ld_z, const float* gate, int ldg, void* out, int ld_out, int nseq, int L, int C, int dtype,
                 void* stream);
/* drn_gate_fwd with a video indirection, for Q queries that share V <= Q videos (each (query, video) pair is one clip of
 * model/main_model.py:51-59,67 + model/backbone.py:28-32): out[q*L+t][c] = dtype(float(z[vid[q]*L+t][c]) * gate[q][c]) for c < C and
 * out[q*L+t][C+p] = pos[vid[q]*L+t][p] for p < P (the video's position-embedding columns; pos NULL with P = 0).  vid: device array
 * of Q indices in [0, V); the kernel clamps an index outside that range and writes zeros for its rows.  vid_host: an optional host
 * copy of vid -- when given, an index outside [0, V) is DRN_ERR_ARG before anything is launched.  vid = identity: drn_gate_fwd's
 * bits. */
int drn_gate_gather_fwd(const void* z, int ld_z, const float* gate, int ldg, const void* pos, int ld_pos, const int32_t* vid,
                        const int32_t* vid_host /*host, may be NULL*/, int V, void* out, int ld_out, int Q, int L, int C, int P,
                        int dtype, void* stream);
/* The same gate + position columns read from a PACKED, projected index (drn_amd.SearchIndex) instead of a chunk's (V, L, .) buffers:
 * rows (n_rows, C + P) holds per proposal [prop_fc output | position embedding], video v owning rows prop_off[v] .. prop_off[v+1]
 * (prop_off: Nv + 1 device int32), and pad_row is the row of a padded proposal.  Pair p < Q is (sentence pq[p], chunk slot pv[p]),
 * its video v = vids[pv[p]] (vids: Vc device int32 store positions):
 *   src = (0 <= v < Nv && t < prop_off[v+1] - prop_off[v]) ? prop_off[v] + t : pad_row          for t < L
 *   out[p*L+t][c] = dtype(float(rows[src][c]) * gate[pq[p]][c]) for c < C      out[p*L+t][C+j] = rows[src][C+j] for j < P
 * One launch writes conv0's whole (Q, L, C+P) input; pq, pv and vids are read on the device at every launch (a captured graph serves
 * every chunk).  A slot outside [0, Vc) or a video outside [0, Nv) reads the pad row; pq is clamped to [0, S) for the loads and is
 * the caller's to keep in range.  pq_host: an optional host copy of pq -- when given, an entry outside [0, S) is DRN_ERR_ARG before
 * anything is launched.  P may be 0. */
int drn_gate_gather_packed(const void* rows, int ld_rows, int n_rows, int pad_row, const int32_t* prop_off, int Nv, const float* gate,
                           int ldg, int S, const int32_t* pq, const int32_t* pq_host /*host, may be NULL*/, const int32_t* pv,
                           const int32_t* vids, int Vc, void* out, int ld_out, int Q, int L, int C, int P, int dtype, void* stream);
/* Rows in block-scaled FP8 (drn_amd/csrc/qindex.hip; the MX layout: OCP e4m3fn codes, one power-of-two scale per 32 columns).
 * x (n, C) in `dtype`, unit column stride, C % 32 == 0 -> codes (n, C) and scales (n, C / 32), both uint8.  Per block of 32 columns:
 *   amax = max |x| in fp32 = m * 2^k with m in [0.5, 1);  e = k - 9 if m <= 0.875 else k - 8 (the smallest e with amax <= 448 * 2^e),
 *   e = -110 for a zero block, e clamped to [-110, 127];  scales[.] = e + 127 (an e8m0 exponent = the fp32 exponent field of 2^e);
 *   codes[.] = e4m3fn(x * 2^-e), round to nearest even, the sign kept where the value rounds to zero;  value = float(code) * 2^e,
 * which is exact in fp32 and in bf16.  drn_amd.index.mx8_quantize is the same definition on the host.  x and codes 16-byte aligned
 * with row strides that are 16-byte multiples; bytes of codes / scales past a row's width are not written.  One launch, no workspace. */
int drn_quantize_rows_mx8(const void* x, int ld_x, int n, int C, uint8_t* codes, int ld_codes, uint8_t* scales, int ld_scales, int dtype,
                          void* stream);
/* drn_gate_gather_packed on a quantised index: the C gated columns of row src are codes[src] / scales[src] as drn_quantize_rows_mx8
 * writes them, the P position columns pos[src] in `dtype` (pos NULL with P = 0); pairs, slots, videos, the pad row, the clamps and
 * pq_host as there:
 *   out[p*L+t][c] = dtype(float(codes[src][c]) * 2^(scales[src][c/32] - 127) * gate[pq[p]][c]) for c < C
 *   out[p*L+t][C+j] = pos[src][j] for j < P
 * -- bit for bit drn_gate_gather_packed on rows that hold the dequantised values.  C % 32 == 0; ld_codes a multiple of 16. */
int drn_gate_gather_packed_q8(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos,
                              int n_rows, int pad_row, const int32_t* prop_off, int Nv, const float* gate, int ldg, int S,
                              const int32_t* pq, const int32_t* pq_host /*host, may be NULL*/, const int32_t* pv, const int32_t* vids,
                              int Vc, void* out, int ld_out, int Q, int L, int C, int P, int dtype, void* stream);
/* conv0 on a quantised index without the gather (csrc/qconv.hip): the sentence gate multiplies conv0's WEIGHT instead of its input,
 * (z * g) W = z (diag(g) W), and the gated weights are quantised to the index's own format.
 * drn_gate_quantize_weights_mx8: w (3, Cout, >= D) fp32, tap-major (w[tap][n][c] = conv0.weight[n][c][tap], row stride ld_w), gate
 * (S, >= D) fp32 ->
 *   wcodes (S, 3, Cout, Dp) / wscales (S, 3, Cout, Dp/32) = drn_quantize_rows_mx8's format of the fp32 products gate[s][c] * w[tap][n][c],
 * columns [D, Dp) zero -- byte for byte drn_amd.index.mx8_gate_weights.  Dp % 32 == 0, D <= Dp; ld_wcodes a multiple of 16 and wcodes
 * 16-byte aligned (row strides of the (S*3*Cout) rows; bytes past a row's width are not written).  One launch for all S sentences. */
int drn_gate_quantize_weights_mx8(const float* w, int ld_w, const float* gate, int ldg, int S, int Cout, int D, int Dp, uint8_t* wcodes,
                                  int ld_wcodes, uint8_t* wscales, int ld_wscales, void* stream);
/* drn_conv0_mx8: the k = 3, stride 1, pad 1 convolution of the (Q, L, C + P) input drn_gate_gather_packed_q8 would have written,
 * straight from the index (the same tables, clamps and pq_host refusal), as an implicit GEMM over the three taps:
 *   raw[p*L+t][n] = sum_tap sum_c  dq(codes, scales)[src(p, t+tap-1)][c] * dq(wcodes, wscales)[pq[p]][tap][n][c]
 *                 + sum_tap sum_j  pos[src(p, t+tap-1)][j] * wpos[tap][n][j]
 * the feature part on v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, the scale bytes as they lie), the position part on
 * v_mfma_f32_16x16x32_bf16 into the same fp32 accumulators; a tap outside [0, L) contributes zero.  No bias, no split-K, no atomics:
 * a row's value does not depend on which other pairs share the launch.  wcodes (S, 3, Cout, C) / wscales (S, 3, Cout, C/32) contiguous;
 * pos (n_rows, >= P) and wpos (3, Cout, P) bf16 (NULL with P = 0); raw (Q*L, >= Cout) bf16, or fp32 with out_f32.
 * C % 32 == 0, P % 32 == 0, Cout % 16 == 0; codes / pos rows 16-byte aligned. */
int drn_conv0_mx8(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos, int n_rows,
                  int pad_row, const int32_t* prop_off, int Nv, const uint8_t* wcodes, const uint8_t* wscales, const void* wpos, int S,
                  const int32_t* pq, const int32_t* pq_host /*host, may be NULL*/, const int32_t* pv, const int32_t* vids, int Vc,
                  void* raw, int ld_raw, int out_f32, int Q, int L, int C, int P, int Cout, void* stream);
/* drn_conv0_mx8_bn: drn_conv0_mx8 -> eval BatchNorm -> ReLU -> gate in ONE launch, raw never written (Grounder(conv0="mxfp8",
 * fused=True)).  The same operands, tables, clamps and pq_host refusal, the same sum per output element (a row's value does not depend on
 * which other pairs share the launch, nor on their order; no split-K, no atomics), computed from LDS-staged tiles of 256 rows of the
 * flattened (pair, t) output x up to 256 channels -- a tile may hold several pairs and sentences; the grid depends on (Q, L, Cout)
 * only.  With acc the fp32 accumulator and (sc, sh) = ss[n], ss[Cout + n], the table drn_bn_eval_scale_shift writes:
 *   v = max(fmaf(acc, sc, sh), 0)          (ss NULL: v = acc, the bare convolution)
 *   out[(p*L+t)*ld_out + n] = dtype(v);   with gate: gated[(p*L+t)*ld_gated + n] = dtype(v * gate[p*ldg + n])  -- gate (Q, >= Cout)
 *   fp32, one row per PAIR, multiplied into the unrounded v as drn_bn_apply_multi does; gate and gated come together or not at all.
 * out / gated bf16, or fp32 with out_f32; elements past Cout in a row are not written.  The other constraints are drn_conv0_mx8's. */
int drn_conv0_mx8_bn(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos, int n_rows,
                     int pad_row, const int32_t* prop_off, int Nv, const uint8_t* wcodes, const uint8_t* wscales, const void* wpos, int S,
                     const int32_t* pq, const int32_t* pq_host /*host, may be NULL*/, const int32_t* pv, const int32_t* vids, int Vc,
                     const float* ss, const float* gate, int ldg, void* out, int ld_out, void* gated, int ld_gated, int out_f32, int Q,
                     int L, int C, int P, int Cout, void* stream);
/* drn_conv0_mx8_bn_tile: drn_conv0_mx8_bn on a tile of tile_rows x tile_cols (rows of the flattened (pair, t) output x channels): 256 x 256
 * is drn_conv0_mx8_bn itself; 128 x 64 and 64 x 64 put 8 and 16 times as many workgroups on the chip, for grids that do not fill it.  The
 * same arguments, the same checks, and bit for bit the same out / gated for every tile: an output element sums its own K in the same
 * fixed order whatever the tile (no split-K, no atomics).  tile_rows = tile_cols = 0: the tile drn_conv0_mx8_bn_choose names.  Any other
 * shape is refused before the launch. */
int drn_conv0_mx8_bn_tile(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos, int n_rows,
                          int pad_row, const int32_t* prop_off, int Nv, const uint8_t* wcodes, const uint8_t* wscales, const void* wpos,
                          int S, const int32_t* pq, const int32_t* pq_host /*host, may be NULL*/, const int32_t* pv, const int32_t* vids,
                          int Vc, const float* ss, const float* gate, int ldg, void* out, int ld_out, void* gated, int ld_gated,
                          int out_f32, int Q, int L, int C, int P, int Cout, int tile_rows, int tile_cols, void* stream);
/* drn_conv0_mx8_bn_choose: the tile drn_conv0_mx8_bn_tile(..., 0, 0, ...) takes -> *rows, *cols.  A function of Q * L, Cout and the
 * current device's compute-unit count alone (never of the pairs: a captured launch replays with other pairs): with W = ceil(Q L / 256) x
 * ceil(Cout / 256) wide-tile workgroups, 64 x 64 while 16 W <= 3 compute units, 128 x 64 while 16 W <= 8 compute units (W up to half the
 * compute units), the wide tile above.  Without a device: the wide tile.  A pending HIP error of earlier work is left in place. */
int drn_conv0_mx8_bn_choose(int Q, int L, int Cout, int* rows, int* cols);
/* backward of the query gating x = q[:, :, None] * x (model/backbone.py:28-30):
 * dC = (add ? add : 0) + dG * gate[seq] (skipped when dC is NULL); dgate[seq][c] = sum_t dG*act;
 * dsum (optional, [nseq][C]) = sum_t dG * gate[seq]: per-clip column sums of dC's gated term (bias-gradient partials) */
int drn_gate_bwd(const void* dG, int ld_dg, const void* act, int ld_act, const float* gate, int ldg, const void* add, int ld_add,
                 void* dC, int ld_dc, float* dgate, int ld_dgate, float* dsum, int nseq, int L, int C, int dtype, void* stream);
/* Input-stage variant: the gated gradient is written only TRANSPOSED, dCT[c][seq*L + t] (row stride ldt), as the K-major
 * operand of the prop_fc weight gradient; dgate / dsum as above.  L % 32 == 0. */
int drn_gate_bwd_t(const void* dG, int ld_dg, const void* act, int ld_act, const float* gate, int ldg, void* dCT, int64_t ldt,
                   float* dgate, int ld_dgate, float* dsum, int nseq, int L, int C, int dtype, void* stream);
/* out[c] (+)= sum_m X[m][c]  (bias gradients) */
int drn_colsum(const void* X, int ld, int M, int C, float* out, int accumulate, float* ws /* >= 64*C floats */, int dtype,
               void* stream);

/* ---- BatchNorm1d(+ReLU) (drn_amd/csrc/bn.hip; model/basic_blocks.py:23-26, model/fcos.py:34,38,60,66) ---- */
typedef struct DrnBnGroup {
  const float* stats; /* [tiles][2][C] from drn_gemm_nt */
  int32_t tiles, M;
  float* scale_shift; /* out [2][C] */
  float* save;        /* out [2][C]: mean, invstd (for backward) */
} DrnBnGroup;
/* Train mode: batch statistics -> scale/shift; running stats updated once per group IN ORDER (shared head modules
 * are applied once per pyramid level, model/fcos.py:93-102).  conv_bias (or NULL) only shifts running_mean. */
int drn_bn_finalize(const DrnBnGroup* groups /*host*/, int ngroups, int C, const float* gamma, const float* beta,
                    const float* conv_bias, float* running_mean, float* running_var, float momentum, float eps, void* stream);
int drn_bn_eval_scale_shift(int C, const float* gamma, const float* beta, const float* conv_bias, const float* running_mean,
                            const float* running_var, float eps, float* scale_shift, void* stream);
/* The same with per-group parameters, for groups that belong to different BatchNorm modules (the FPN levels) as well as
 * groups sharing one (pass the same pointers: they are updated in order). */
typedef struct DrnBnFinDesc {
  const float* stats;
  int32_t tiles, M;
  float* scale_shift;
  float* save;
  const float* gamma;
  const float* beta;
  const float* conv_bias;  /* or NULL */
  float* running_mean;     /* or NULL */
  float* running_var;      /* or NULL */
  float momentum, eps;
} DrnBnFinDesc;
int drn_bn_finalize_multi(const DrnBnFinDesc* descs /*host*/, int n, int C, void* stream);
/* out = [relu](raw*scale+shift) [+ up[seq, t/2]] ; gated = out*gate[seq]  (fused consumers' prologues) */
int drn_bn_apply(const void* raw, int ld_raw, const float* scale_shift, void* out, int ld_out, int M, int C, int L, const void* up,
                 int ld_up, const float* gate, int ldg, void* gated, int ld_gated, int relu, int dtype, void* stream);
/* ... for up to DRN_MAX_GROUPS pyramid levels of equal C in ONE launch (independent levels only). */
typedef struct DrnBnApplyDesc {
  const void* raw;
  const float* scale_shift;
  void* out;
  const void* up;     /* or NULL */
  const float* gate;  /* or NULL (with gated) */
  void* gated;
  int32_t ld_raw, ld_out, ld_up, ldg, ld_gated, M, L;
} DrnBnApplyDesc;
int drn_bn_apply_multi(const DrnBnApplyDesc* descs /*host*/, int n, int C, int relu, int dtype, void* stream);
/* Conv1d -> BatchNorm1d (eval) -> [ReLU] in ONE launch: drn_gemm_nt + drn_bn_apply_multi without the raw tensor.  Eval BatchNorm is a
 * per-channel affine map, so it runs in the GEMM epilogue: no statistics, no exchange, no second pass over the output.
 * Per group g, with acc[m][n] the fp32 accumulator of problem gemm[g] (mode 0; any taps / stride / pad drn_gemm_nt serves) and
 * (sc, sh) = bn[g].scale_shift[n], scale_shift[N + n] -- the table drn_bn_eval_scale_shift writes, conv bias folded into sh:
 *   v = fmaf(acc, sc, sh);  v = fmaxf(v, 0) when relu;
 *   out[m*ld_out + n] = dtype(v);
 *   with bn[g].gate: gated[m*ld_gated + n] = dtype(v * gate[(m / L)*ldg + n])  -- from the unrounded v, as drn_bn_apply_multi does.
 * In fp32 the results are bit-identical to drn_gemm_nt followed by drn_bn_apply_multi (the raw fp32 tensor IS the accumulator); in
 * bf16 they skip the rounding of the raw tensor.  gemm[g].C is not written and may be NULL; bn[g].raw is ignored; bn[g].M / L must
 * equal gemm[g].M / Lout.
 * DRN_ERR_UNSUPPORTED -- nothing launched, drn_last_error() says why, run the separate launches: bn[g].up set (the FPN top-down chain
 * needs a finished coarser level); any of gemm[g].C2 / bias / gate / stats / accumulate / out_f32 / sumsq / gb_*; mode 1; groups with
 * different N; outputs that are not 16-byte aligned with 16-byte row strides; a launch drn_gemm_nt_plan puts on DRN_NT_KIND_W4
 * (gemm_nt_w4_kernel has no such epilogue).
 * Kernel selection is drn_gemm_nt's / drn_gemm_nt_splitk's own (same tile rule, same drn_tune keys, same K order): a convolution runs
 * on the kernel kind it runs on without the fusion; the _plan entry points report that kind (or an error code) without launching.
 * _splitk serves ONE problem (conv0); ws / counters as for drn_gemm_nt_splitk; OR DRN_KSPLIT_EVAL_RELU into ksplit for the ReLU.  The
 * grouped K-split has no fused form. */
#define DRN_KSPLIT_EVAL_RELU 0x1000000
int drn_conv_bn_eval(const DrnGemmDesc* gemm /*host*/, const DrnBnApplyDesc* bn /*host*/, int ngroups, int relu, int dtype, void* stream);
int drn_conv_bn_eval_plan(const DrnGemmDesc* gemm /*host*/, const DrnBnApplyDesc* bn /*host*/, int ngroups, int dtype);
int drn_conv_bn_eval_splitk(const DrnGemmDesc* gemm /*host*/, const DrnBnApplyDesc* bn /*host*/, int ksplit, float* ws, int32_t* counters,
                            int dtype, void* stream);
int drn_conv_bn_eval_splitk_plan(const DrnGemmDesc* gemm /*host*/, const DrnBnApplyDesc* bn /*host*/, int ksplit, int dtype);
/* Train-mode forward in ONE launch (C % 64 == 0): statistics merge + running-statistics update + apply.  Each workgroup of the
 * apply pass merges the slab statistics of its own 64 channels; scale_shift / save / the running statistics are written once
 * per channel, groups in order (groups may share a BatchNorm module: model/fcos.py:93-102).  Replaces drn_bn_finalize(_multi)
 * + drn_bn_apply_multi for nn.BatchNorm1d + ReLU in training (model/basic_blocks.py:23-26). */
typedef struct DrnBnTrainDesc {
  const float* stats; /* [tiles][2][C] from drn_gemm_nt, tiles = ceil(M/128) */
  float* scale_shift; /* out [2][C] */
  float* save;        /* out [2][C]: mean, invstd */
  const float* gamma;
  const float* beta;
  const float* conv_bias; /* or NULL */
  float* running_mean;    /* or NULL */
  float* running_var;     /* or NULL */
  const void* raw;
  void* out;
  const void* up;    /* or NULL */
  const float* gate; /* or NULL (with gated) */
  void* gated;
  float momentum, eps;
  int32_t tiles, ld_raw, ld_out, ld_up, ldg, ld_gated, M, L;
} DrnBnTrainDesc;
int drn_bn_train_apply(const DrnBnTrainDesc* descs /*host*/, int n, int C, int relu, int dtype, void* stream);
/* Conv1d -> BatchNorm1d (training) -> ReLU in ONE launch (model/basic_blocks.py:9-31; FPN laterals / output convs
 * model/FPN.py:54-69; head towers model/fcos.py:33-69 with statistics per level call, fcos.py:93-102): drn_gemm_nt +
 * drn_bn_train_apply without the second launch and without re-reading the raw conv output.  gemm[i] / bn[i] describe group i
 * (bn[i].raw == gemm[i].C; the raw output is still written: backward reads it; gemm[i].stats / bn[i].stats are ignored).
 * Every workgroup keeps its raw tile in registers, publishes its per-slab statistics as 64-bit {value, generation} pairs in
 * tagged_ws, merges the pairs of its tile column -- polling them until they carry this launch's generation -- exactly as
 * drn_bn_train_apply merges (same bits), and stores the normalised tile.  up_group (host, or NULL): up_group[i] = j > i makes
 * out_i += nearest_x2(out_j) (the FPN top-down chain), recomputed from group j's raw rows inside the launch; -1 = none.
 * tagged_ws: >= drn_conv_bn_train_ws_bytes() bytes, 8-byte aligned, ZERO when first used and afterwards written by this entry
 * point only; generation: one int32, zero at first, advanced by the kernel (one pair of buffers per stream).
 * Returns DRN_ERR_UNSUPPORTED -- nothing launched, call the two-launch path -- when the groups' N differ or are not a
 * multiple of the tile width, an epilogue option of drn_gemm_nt is requested, or the grid exceeds what the chip holds at once
 * (the wait needs every workgroup resident; the device must not be shared with another process that also waits).  */
int64_t drn_conv_bn_train_ws_bytes(const DrnGemmDesc* gemm /*host*/, int ngroups);
int drn_conv_bn_train(const DrnGemmDesc* gemm /*host*/, const DrnBnTrainDesc* bn /*host*/, int ngroups, int relu,
                      const int32_t* up_group /*host or NULL*/, void* tagged_ws, int64_t ws_bytes, int32_t* generation, int dtype,
                      void* stream);
/* Watchdog of that wait: workgroups that gave up after 2 s since the last reset (their launch's results are invalid).
 * Synchronises the device; -1 on error. */
int drn_conv_bn_train_timeouts(int reset);
/* dRaw, dgamma, dbeta from dOut; ReLU mask recomputed from raw; draw may alias dout. */
int drn_bn_bwd(const void* dout, int ld_dout, const void* raw, int ld_raw, const float* scale_shift, const float* save,
               const float* gamma, void* draw, int ld_draw, float* dgamma, float* dbeta, int accumulate, int M, int C, int relu,
               float* ws /* >= 515*C floats */, int dtype, void* stream);
/* ... for up to DRN_MAX_GROUPS levels of equal C in three launches; levels sharing one module pass the same dgamma/dbeta
 * with accumulate = 1 from the second level on (summed in level order).  ws >= n*515*C floats. */
typedef struct DrnBnBwdDesc {
  const void* dout;
  const void* raw;
  const float* scale_shift;
  const float* save;
  const float* gamma;
  void* draw;
  float* dgamma;
  float* dbeta;
  int32_t ld_dout, ld_raw, ld_draw, accumulate, M;
  /* drn_bn_bwd_one only.  gb_dg != NULL: the layer's output was also consumed GATED by the query (model/backbone.py:28-30,
   * gated = out * gate[clip]); gb_dg [M][gb_ld_dg] is the gradient of the gated output, dout (or NULL) the gradient of the plain one.
   * The launch does drn_gate_bwd's work on the rows it loads: dout_eff = dtype(dout + gb_dg * gb_gate[m / gb_L]) feeds the BatchNorm
   * backward (bit-identical to the two launches), gb_dgate[clip][c] ([M / gb_L][C] fp32) = sum_t gb_dg * out with `out` recomputed from
   * raw.  Needs gb_L a multiple of 32 rows (bf16; 16 in fp32) that divides the launch's row block: drn_bn_bwd_one_ws_bytes() says 0
   * otherwise, and the caller runs drn_gate_bwd itself. */
  const void* gb_dg;
  const float* gb_gate;
  float* gb_dgate;
  int32_t gb_ld_dg, gb_ldg, gb_L;
} DrnBnBwdDesc;
int drn_bn_bwd_multi(const DrnBnBwdDesc* descs /*host*/, int n, int C, int relu, float* ws, int dtype, void* stream);
/* The same in ONE launch: every workgroup keeps its rows of dout and raw in registers between the sums and the apply half and
 * meets the other row blocks of its channel tile through tagged pairs in `tagged_ws` (64-byte aligned, >=
 * drn_bn_bwd_one_ws_bytes() bytes, ZERO before its first use and then left to the library: it carries the launch generation;
 * one launch at a time per workspace).  Needs C % 64 == 0 and a grid the chip holds at once: DRN_ERR_UNSUPPORTED (nothing
 * launched) / 0 bytes otherwise -- the caller then takes drn_bn_bwd_multi.  Per-row-block partial sums are formed over
 * different row blocks than drn_bn_bwd_multi's, so the two agree to rounding, not bit for bit.
 * drn_bn_bwd_one_timeouts: workgroups that gave up waiting (2 s watchdog; 0 in a healthy run); synchronises the device. */
int64_t drn_bn_bwd_one_ws_bytes(const DrnBnBwdDesc* descs /*host*/, int n, int C, int dtype);
int drn_bn_bwd_one(const DrnBnBwdDesc* descs /*host*/, int n, int C, int relu, void* tagged_ws, int64_t ws_bytes, int dtype, void* stream);
int drn_bn_bwd_one_timeouts(int reset);

/* ---- 1-2 channel output heads (drn_amd/csrc/heads.hip; model/fcos.py:43-49,68,96-102) ------------------- */
typedef struct DrnHeadGroup {
  const void* X; /* level activations, channels-last (may be a column slice) */
  void* dX;      /* backward: gradient buffer, same geometry */
  int32_t ldx, M, L;
  const float* scale; /* exp mode: scales[l].scale (1 float) */
} DrnHeadGroup;
/* out[r][n] = bias[n] + conv(X, W)[r][n]; exp_mode: z = that, out = exp(scale_l*z).  `W` is the nn.Conv1d weight (N,C,taps)
 * RE-LAID as [N][taps][C] fp32 (what drn_pack_weight(perm 0,2,1) / drn_adam_tiled's kind-1 copy produce); dW comes back in the
 * parameter's own (N,C,taps) layout. */
int drn_head_out_fwd(const DrnHeadGroup* groups /*host*/, int ngroups, const float* W, const float* bias, int N, int C, int taps,
                     int exp_mode, float* out, float* z, int dtype, void* stream);
/* dout is the gradient w.r.t. `out`; exp_mode applies d out/d z = scale*out and accumulates dscale[l];
 * dX (+)= conv^T(dz), dW/dbias/dscale (+)= ... over all levels. */
int drn_head_out_bwd(const DrnHeadGroup* groups /*host*/, int ngroups, const float* W, const float* dout, const float* out,
                     const float* z, int N, int C, int taps, int exp_mode, int accumulate_dx, float* dW, float* dbias,
                     float* dscale, int accumulate_dw, float* ws /* >= drn_heads_ws_elems(sum of M, N, C, taps) floats */, int dtype, void* stream);

/* Up to 2 heads per launch (cls_logits + bbox_pred read the two halves of one tower output: side by side they fill the chip).
 * One DrnHeadCall = the arguments of drn_head_out_fwd / _bwd for one head; forward uses groups, W, bias, out, z; backward
 * groups (with dX), W, dout, out, z, dW, dbias, dscale (+ dscale_stride), ws (>= drn_heads_ws_elems() floats each), accumulate flags.
 * Backward is two launches: data gradient + weight-gradient partials side by side, then the reduction of the partials. */
typedef struct DrnHeadCall {
  const DrnHeadGroup* groups; /* host */
  int32_t ngroups, N, C, taps, exp_mode, accumulate_dx, accumulate_dw;
  int32_t dscale_stride; /* elements between dscale[l] and dscale[l+1] (0 = 1) */
  const float* W;
  const float* bias;
  float* out;
  float* z;
  const float* dout;
  float* dW;
  float* dbias;
  float* dscale;
  float* ws;
} DrnHeadCall;
int64_t drn_heads_ws_elems(int total_rows, int N, int C, int taps); /* fp32 workspace of one head's backward */
int drn_heads_fwd(const DrnHeadCall* calls /*host*/, int ncalls, int dtype, void* stream);
int drn_heads_bwd(const DrnHeadCall* calls /*host*/, int ncalls, int dtype, void* stream);

/* ---- losses (drn_amd/csrc/loss.hip; model/loss.py:40-239, model/layers/{iou_loss,sigmoid_focal_loss}.py) -- */
typedef struct DrnLossLevel {
  int32_t L;    /* locations per clip on this level */
  float stride; /* fpn_stride: location = t*stride + stride/2 (model/fcos.py:204-211) */
  float lo, hi; /* object_sizes_of_interest (model/loss.py:47-51) */
} DrnLossLevel;
/* logits [R], reg [R][2], iou [R] are fp32 over R = B*sum(L) rows ordered level-first, clip-major (the reference's
 * flatten order, model/loss.py:150-166).  gt [B][2] is fp32, or fp64 with gt_f64 = 1 (cast on load, main_model.py:74).
 * out6 = {loss_cls, loss_reg, loss_iou, n_pos, n_iou_pos, loss_cls + loss_reg + loss_iou (main.py:225)}.
 * bumps (host array, may be NULL): int64 device counters (BatchNorm num_batches_tracked) incremented by the same launch.
 * Replaces FCOSLossComputation.__call__ incl. fcos_core._C.sigmoid_focalloss_forward/backward + IOULoss +
 * segment_tiou/SmoothL1. */
#define DRN_LOSS_MAX_BUMPS 32
typedef struct DrnCounterBump {
  void* counter; /* int64 on the device */
  int32_t inc;
} DrnCounterBump;
int drn_fcos_loss_fwd(const DrnLossLevel* levels /*host*/, int nlevels, int B, const float* logits, const float* reg,
                      const float* iou, const void* gt /*[B][2]*/, int gt_f64, float gamma, float alpha, float target_scale,
                      int iou_stage, float* out6, float* labels /*[R] or NULL*/, float* ws /* >= 5*ceil(R/256) floats */,
                      int32_t* ticket /* one zeroed int32 (left zero), or NULL: the final summation as a second launch */,
                      const DrnCounterBump* bumps /*host*/, int nbumps, void* stream);
int drn_fcos_loss_bwd(const DrnLossLevel* levels /*host*/, int nlevels, int B, const float* logits, const float* reg,
                      const float* iou, const void* gt, int gt_f64, float gamma, float alpha, float target_scale, int iou_stage,
                      const float* fwd_out6, const float* g_cls, const float* g_reg, const float* g_iou /* 1 float each, NULL = 0 */,
                      float* dlogits, float* dreg, float* diou, void* stream);

/* The reference's ONE real FFI on this path, 1:1: fcos_core._C.sigmoid_focalloss_forward(logits, targets, num_classes, gamma,
 * alpha) -> losses and sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha) -> d_logits
 * (model/layers/sigmoid_focal_loss.py:18-20,31-33).  logits / losses / d_losses / d_logits are fp32 [N][num_classes],
 * targets int32 [N]: 0 = background, c in 1..num_classes = foreground class c, negative = ignored (loss and gradient 0).
 * Element-wise (the caller sums, sigmoid_focal_loss.py:68); any num_classes; finite for any finite logit. */
int drn_focal_fwd(const float* logits, const int32_t* targets, int64_t N, int num_classes, float gamma, float alpha, float* losses,
                  void* stream);
int drn_focal_bwd(const float* logits, const int32_t* targets, const float* d_losses, int64_t N, int num_classes, float gamma,
                  float alpha, float* d_logits, void* stream);

/* Stand-alone IOULoss (model/layers/iou_loss.py:5-24, exported by model/layers/__init__.py): pred / target fp32 [N][2] =
 * (left, right) distances, weight fp32 [N] or NULL.  out2[0] = sum(l_i w_i) / sum(w) when weight != NULL and sum(w) > 0, else
 * mean(l_i), l_i = -log((min(pr,tr) + min(pl,tl) + 1e-8) / (union + 1e-8)); out2[1] = the divisor, negative for the plain mean
 * (backward reads the mode there: no host sync).  N == 0 is an error (the reference asserts).  Backward: gout = upstream
 * gradient (1 float, NULL = 1); dpred / dtarget [N][2], either may be NULL; ties in min() split evenly. */
int drn_iou_loss_fwd(const float* pred, const float* target, const float* weight, int64_t N, float* out2, void* stream);
int drn_iou_loss_bwd(const float* pred, const float* target, const float* weight, int64_t N, const float* out2, const float* gout,
                     float* dpred, float* dtarget, void* stream);

/* ---- eval post-processor (drn_amd/csrc/postproc.hip; model/inference.py:51-120,166-199) ------------------------
 * Per clip and level: candidates sigmoid(logit) > thr, score = sigmoid(logit)[*sigmoid(iou)] (iou NULL in the first stage),
 * top_n per level, segments ((loc-reg0)/downsample, (loc+reg1)/downsample) clamped to [0,1], score = sqrt(.), loc/32.
 * Inputs are the head outputs in the loss layout (rows level-first / clip-major).  Outputs are padded per clip:
 * det [B][sum L][2], scores / locs [B][sum L], counts [B][nlevels] = kept candidates per level, written level after level. */
int drn_postprocess(const DrnLossLevel* levels /*host*/, int nlevels, int B, const float* logits, const float* reg, const float* iou,
                    float thr, int top_n, float downsample, float* det, float* scores, float* locs, int32_t* counts, void* stream);
/* Recall@k with temporal NMS on the device, straight from drn_postprocess's outputs (utils/evaluate_utils.py:131-215: stable
 * sort by score, greedy NMS at IoU threshold iou - 0.05 visiting score ties from the later prediction, hit = one of the first
 * k survivors overlaps gt by >= iou, un-clamped IoU; double arithmetic on the float32 detections, as the host path).
 * first_hit[b][q] = 0-based position among the NMS survivors of the first one that hits at ious[q], or max_topk when none of the
 * first max_topk does: recall@k counts first_hit < k.  gt: (B, 2) fp64 or fp32; ious: device array of n_iou doubles. */
int drn_eval_recall(const float* det, const float* scores, const int32_t* counts, int B, int nlevels, int rows_per_clip,
                    const void* gt, int gt_is_f64, const double* ious /*device*/, int n_iou, int max_topk, int32_t* first_hit,
                    void* stream);
/* The moments of each clip, straight from drn_postprocess's outputs: the first K survivors of that same temporal NMS, best first
 * (utils/evaluate_utils.py:91-107 stable sort by score, :186-212 nms_temporal at `overlap` -- the evaluator's value is iou - 0.05 --
 * score ties to the later candidate, a candidate struck out unless inter / (len_i + len_j - inter) <= overlap in double, 0/0 struck
 * out).  seg [B][K][2] = the detections, copied; score [B][K]; level [B][K] = pyramid level of the candidate (running sum of
 * counts); index [B][K] = its position in the clip's candidate list; n [B] = valid entries.  Entries past n: 0 / -1.  A clip
 * without candidates yields the fallback moment of model/inference.py:192-197: (0, 1), score 1, level -1, index -1, n = 1.  One
 * wavefront per clip, no host synchronisation. */
int drn_select_moments(const float* det, const float* scores, const int32_t* counts, int B, int nlevels, int rows_per_clip,
                       double overlap, int K, float* seg, float* score, int32_t* level, int32_t* index, int32_t* n, void* stream);
/* The best K moments of S sentences ACROSS videos, streamed chunk by chunk: one call merges one chunk's drn_select_moments outputs --
 * P = S * Vc pairs of kv slots each, pair p = (sentence p / Vc, chunk slot p % Vc), vids [Vc] = the slots' positions in a store of Nv
 * videos -- into the running state of each sentence, in place: st_seg [S][K][2], st_score [S][K], st_video [S][K] (store position),
 * st_level [S][K], st_rank [S][K] (the moment's position among its pair's survivors), st_n [S]; slots past st_n are written 0 / -1.
 * Candidates of sentence s: its st_n[s] state entries and the entries r < n[p] of its pairs, EXCEPT pairs whose vids[slot] is outside
 * [0, Nv) (the padded tail of the last chunk), fallback entries (index < 0: a video without a candidate is no hit) and entries whose
 * score is not finite.  Order, total, so that the result does not depend on how the videos were cut into chunks: score descending
 * (the stored floats compared, nothing recomputed), then video position ascending, then rank ascending.
 * The incoming state is ignored (never read) when `first` is non-zero; first_dev, when not NULL, is a DEVICE word read instead of
 * `first`, so that a captured graph serves the first chunk and the later ones.  One wavefront per sentence stages the K + Vc * kv
 * candidates in LDS: K + Vc * kv <= DRN_MERGE_MAX_CAND, refused otherwise.  No host synchronisation. */
#define DRN_MERGE_MAX_CAND 2048
int drn_merge_moments(const float* seg, const float* score, const int32_t* level, const int32_t* index, const int32_t* n, int S, int Vc,
                      int kv, const int32_t* vids, int Nv, int K, int first, const int32_t* first_dev, float* st_seg, float* st_score,
                      int32_t* st_video, int32_t* st_level, int32_t* st_rank, int32_t* st_n, void* stream);
/* drn_merge_moments for a chunk of P pairs in ANY assignment to sentences (a shortlist of videos per sentence): pair_video [P] = the
 * store position of pair p's video (outside [0, Nv): a padded pair, skipped), pair_off [S + 1] = sentence s owns the pairs
 * [pair_off[s], pair_off[s + 1]) of the chunk; both on the device.  Pairs outside every range take no part.  Same candidates, same
 * exceptions, same total order (a pair's position in its sentence's range standing in for the chunk slot), same state and same
 * first / first_dev as drn_merge_moments.  A sentence without a pair in the chunk keeps its state bit for bit (first == 0) or is left
 * empty (first != 0).  Nothing read from pair_off is trusted: offsets are clamped to [0, P], a negative or decreasing range is empty,
 * and at most (DRN_MERGE_MAX_CAND - K) / kv pairs of a range are read -- a caller that wants every pair ranked keeps its ranges within
 * that.  K + kv <= DRN_MERGE_MAX_CAND, refused otherwise.  One wavefront per sentence, no host synchronisation. */
int drn_merge_moments_ragged(const float* seg, const float* score, const int32_t* level, const int32_t* index, const int32_t* n, int S,
                             int P, int kv, const int32_t* pair_video, const int32_t* pair_off, int Nv, int K, int first,
                             const int32_t* first_dev, float* st_seg, float* st_score, int32_t* st_video, int32_t* st_level,
                             int32_t* st_rank, int32_t* st_n, void* stream);
/* Corpus recall of a search, on the device: scores the Hits of S sentences (drn_merge_moments' state: seg [S][K][2], video [S][K],
 * n [S]) against ground truth -- gt_video [S] = store position of the annotated video, gt [S][2] = start and end as fractions of it,
 * fp64 or fp32 (gt_is_f64); ious: device array of I doubles.  first_hit [S][I + 1], with m = min(max(n[s], 0), K):
 *   column i < I  the smallest position p in [0, m) with video[s][p] == gt_video[s] and tIoU(seg[s][p], gt[s]) >= ious[i], K when none;
 *                 tIoU is drn_eval_recall's un-clamped (min(g1, x2) - max(g0, x1)) / (max(g1, x2) - min(g0, x1)) in double on the
 *                 float32 segment -- a disjoint pair is negative, 0/0 and a NaN bound are no hit;
 *   column I      the number of DISTINCT videos among video[s][0:p0], p0 = the smallest position in [0, m) of gt_video[s]'s video, K
 *                 when there is none: the ground-truth video's place in the VIDEO ranking, whatever per_video was.
 * Entries at or past n[s] are not read.  A gt_video that is negative or names no video of the row yields K in every column.
 * recall@k counts first_hit < k.  K <= DRN_MERGE_MAX_CAND (a Hits table cannot be larger), refused otherwise.  One wavefront per
 * sentence, no host synchronisation. */
int drn_search_recall(const float* seg, const int32_t* video, const int32_t* n, const int32_t* gt_video, const void* gt, int gt_is_f64,
                      const double* ious /*device*/, int S, int K, int I, int32_t* first_hit, void* stream);
/* The first stage of a two-stage search (drn_amd/csrc/retrieve.hip): each of S sentences' best n videos of an embedding table, by
 * dot product.  emb [V][E] and queries [S][E], contiguous, both float32 or both bfloat16 (dtype), 16-byte aligned.
 * score[s][v] = sum_e queries[s][e] * emb[v][e], accumulated in fp32 on MFMAs in ONE fixed order per score: its bits do not depend on
 * V, S, n or how the grid cuts the table.  Sentence s lists the videos whose score is finite, ordered by score descending, then
 * position ascending -- a total order -- cut to n: ids [S][n], scores [S][n], counts [S] = the list's length; past it ids = -1 and
 * scores = 0.  1 <= n <= DRN_SHORTLIST_MAX (a choice, not a measurement: two lists of that many 8-byte keys are the 2 KiB one merging
 * wavefront sorts in LDS).  ws: ws_keys >= S * ceil(V / 256) * min(n, 256) 8-byte keys of workspace, 8-byte aligned, written by the
 * first of the two launches (each workgroup ranks 256 videos for 16 sentences) and read by the second (one wavefront per sentence
 * merges its lists).  No atomics, no host synchronisation. */
#define DRN_SHORTLIST_MAX 128
int drn_shortlist_topn(const void* emb, const void* queries, int V, int E, int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids,
                       float* scores, int32_t* counts, void* stream);
/* The shortlist over a RAGGED table (drn_amd/csrc/retrieve_seg.hip): emb [R][E] holds segment embeddings, video v owns the rows
 * offsets[v] .. offsets[v + 1] - 1 (offsets [V + 1] int32 on the device, non-decreasing from 0 to R; a video may own no row).
 * score[s][v] = the maximum over v's rows of drn_shortlist_topn's score of that row -- the same MFMA chain per (sentence, row), so a
 * row's bits depend on the row and the query alone, and with one row per video the scores are drn_shortlist_topn's.  Sentence s lists
 * the videos that own a row and whose score is finite, under the same total order, cut to n; rows [S][n] = the lowest segment number
 * (row - offsets[v]) that reaches the video's score, -1 past the list.  blk_vid [nblocks + 1] and vid_blk [V], int32 on the device,
 * are the caller's block plan: block b holds the videos blk_vid[b] .. blk_vid[b + 1] - 1, at most 256, blk_vid[0] = 0 and
 * blk_vid[nblocks] = V, and vid_blk[v] is v's block.  The three tables are NOT read on the host; every index taken from them is
 * clamped, so a bad table gives a wrong list and no access outside the buffers.  ws: ws_keys >= K + ceil(K / 2) 8-byte keys, K = S *
 * nblocks * min(n, 256) (each block's lists, then their winning segments as int32).  Three launches (rank the blocks, the merge of
 * drn_shortlist_topn, look the segments up); no atomics, no host synchronisation. */
int drn_shortlist_segments_topn(const void* emb, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                                const int32_t* vid_blk, int R, int V, int nblocks, int E, int S, int n, int dtype, void* ws, int ws_keys,
                                int32_t* ids, float* scores, int32_t* counts, int32_t* rows, void* stream);
/* drn_shortlist_topn and drn_shortlist_segments_topn over a table kept in block-scaled FP8 (drn_amd/csrc/retrieve_q8.hip): codes
 * [V or R][E] uint8 (OCP e4m3fn) and scales [V or R][E / 32] uint8 (e8m0, one power-of-two scale per 32 columns), contiguous, as
 * drn_quantize_rows_mx8 writes them, codes 16-byte aligned; E % 32 == 0, refused otherwise (there is no tail).  dtype is that of the
 * QUERIES (float32 or bfloat16) and chooses the MFMA chain.  A table value is float(code) * 2^(scale - 127), exact in both dtypes,
 * built in registers from 8 (bfloat16) or 4 (float32) code bytes and the scale byte of their block; the K-steps, their order and the
 * MFMAs per (sentence, row) are the plain entries', so the lists are BIT FOR BIT those of the plain entry over the dequantised table.
 * The table is not checked here: a NaN code (0x7f / 0xff) or a scale byte of 255 makes scores that are not finite and are not listed.
 * Everything else -- the order, the padding, the workspace and its size, the block plan, the clamps, the launches (two and three) -- is
 * the plain twin's. */
int drn_shortlist_topn_q8(const uint8_t* codes, const uint8_t* scales, const void* queries, int V, int E, int S, int n, int dtype, void* ws,
                          int ws_keys, int32_t* ids, float* scores, int32_t* counts, void* stream);
int drn_shortlist_segments_topn_q8(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                   const int32_t* blk_vid, const int32_t* vid_blk, int R, int V, int nblocks, int E, int S, int n, int dtype,
                                   void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows, void* stream);
/* The four shortlist entries above with a packed ALLOW MASK (drn_amd/csrc/retrieve_allow.hip): each takes its twin's arguments plus
 * allow and allow_stride.  A packed mask is W = ceil(V / 32) int32 words a row on the device, 4-byte aligned: bit v & 31 of word v >> 5
 * set = video v may be listed; bits at or past V are ignored.  allow_stride = 0: allow [W], one mask for every sentence; allow_stride =
 * W: allow [S][W], row s for sentence s; any other stride is refused.  A video whose bit is clear is no candidate for that sentence,
 * exactly like a video whose score is not finite: the list is the twin's definition applied to the allowed videos (on a ragged table
 * the mask is over VIDEOS, not rows), and a listed score has the bits the twin gives it -- the same MFMA chain.  Everything else -- the
 * order, the padding, the workspace and its size, the block plan, the clamps, the checks, the launches (two and three) -- is the twin's.
 * A workgroup whose block holds no allowed video for any sentence of its tile reads no row of the table.  The mask is not read on the
 * host; its contents may change between replays of a captured graph. */
int drn_shortlist_topn_allow(const void* emb, const void* queries, const int32_t* allow, int allow_stride, int V, int E, int S, int n,
                             int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, void* stream);
int drn_shortlist_segments_topn_allow(const void* emb, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                                      const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S,
                                      int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows,
                                      void* stream);
int drn_shortlist_topn_q8_allow(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* allow, int allow_stride,
                                int V, int E, int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts,
                                void* stream);
int drn_shortlist_segments_topn_q8_allow(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                         const int32_t* blk_vid, const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V,
                                         int nblocks, int E, int S, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores,
                                         int32_t* counts, int32_t* rows, void* stream);
/* The DEEP shortlist (drn_amd/csrc/retrieve_allow.hip, the merge in drn_amd/csrc/retrieve_deep.hip): the four *_allow entries above
 * behind one name, with 1 <= n <= DRN_SHORTLIST_DEEP_MAX = DRN_RERANK_MAX_CANDIDATES = DRN_CANDIDATES_MAX -- the width
 * drn_shortlist_rerank and drn_plan_candidates take, so a coarse table can fill the second stage of a cascade.  table is emb, or the
 * codes of a block-scaled FP8 table with scales beside them (scales == NULL: a plain table; E % 32 == 0 with scales); dtype is that of
 * the queries.  offsets == NULL: one row per video -- blk_vid, vid_blk and rows must then be NULL too, and R and nblocks are ignored;
 * otherwise all four are given, with the checks of drn_shortlist_segments_topn.  allow is REQUIRED: a packed mask with stride 0 or
 * ceil(V / 32), 4-byte aligned (a caller without a filter passes one row of all-ones words with stride 0).  The definition, the
 * scores' bits, the order, the padding and the clamps are the *_allow entries': at n <= DRN_SHORTLIST_MAX every field equals theirs.
 * ws: ws_keys >= S * blocks * min(n, 256) 8-byte keys, times 1.5 on a ragged table, as the twins'.  Two launches on a plain table, three
 * on a ragged one: the twin's phase one (a block holds at most 256 videos, so at n >= 256 its list is complete), one workgroup per
 * sentence that merges the lists four at a time in 2 * CAP keys of LDS, CAP = 256 / 512 / 1024 the smallest >= n, and the twin's
 * segment look-up.  No atomics, no host synchronisation; the queries and the mask may change between replays of a captured graph. */
#define DRN_SHORTLIST_DEEP_MAX 1024
int drn_shortlist_deep(const void* table, const uint8_t* scales, const void* queries, const int32_t* offsets, const int32_t* blk_vid,
                       const int32_t* vid_blk, const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S, int n,
                       int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows, void* stream);
/* The BINARY shortlist (drn_amd/csrc/retrieve_bin.hip): a table of 1-bit SIGN CODES ranked by Hamming distance.  codes [rows][W] int32,
 * W = ceil(E / 32): bit e & 31 of word e >> 5 is 1 unless x[row][e] < 0 (+0 and -0 give 1), bits at or past E are 0 -- a packed allow
 * mask's convention, and drn_pack_allow over ~(x < 0) is the quantiser.  queries [S][E] are floats of `dtype`; the launch binarises
 * them by the same rule, and a row with an element that is not finite lists nothing.  score[s][r] = E - 2 popcount(code(q_s) xor
 * codes[r]) over the E real bits = sum_e sign(q_e) sign(x_e), an integer that is exact as a float: 1 <= E <= DRN_BINARY_MAX_E (a CHOICE:
 * 16 sentences' query codes are 8 KiB of LDS).  The conventions are drn_shortlist_deep's: offsets == NULL is one row per video --
 * blk_vid, vid_blk and rows must then be NULL too, and R and nblocks are ignored; otherwise all four are given, a video is scored by
 * its best row and rows names the lowest row that reaches it.  allow is REQUIRED: a packed mask over the videos with stride 0 or
 * ceil(V / 32), 4-byte aligned (a caller without a filter passes one row of all-ones words with stride 0).  1 <= n <=
 * DRN_SHORTLIST_DEEP_MAX; the total order, the -1 / 0 / -1 padding and the clamps of every index read from the device tables are those
 * of drn_shortlist_topn and drn_shortlist_segments_topn.  ws: ws_keys >= S * blocks * min(n, 256) 8-byte keys, times 1.5 on a ragged
 * table.  Two launches on a plain table, three on a ragged one: the XOR / popcount phase one (one table row per thread, 16-byte loads
 * when W % 4 == 0), then the merge of drn_shortlist_deep at every n, and the segment look-up.  No
 * atomics, no host synchronisation; the queries and the mask may change between replays of a captured graph. */
#define DRN_BINARY_MAX_E 4096
int drn_shortlist_bin(const int32_t* codes, const void* queries, const int32_t* offsets, const int32_t* blk_vid, const int32_t* vid_blk,
                      const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S, int n, int dtype, void* ws, int ws_keys,
                      int32_t* ids, float* scores, int32_t* counts, int32_t* rows, void* stream);
/* The ASYMMETRIC binary shortlist (drn_amd/csrc/retrieve_bin_asym.hip): FLOAT queries against the same table of sign codes.  score[s][r] =
 * sum_e q[s][e] * (codes[r] bit e set ? +1 : -1): the queries keep their magnitudes, the table stays one bit a column.  It IS
 * drn_shortlist_deep over the (rows, E) table of +-1 in `dtype` that the codes stand for, bit for bit in every field: phase one runs
 * that entry's MFMA chain (the same K-steps in ascending order, 32 columns a step in bf16 and 16 in fp32) with its table operand built
 * from the code bits in registers, a column at or past E zero on both sides.  A score that is not finite is not listed, so a query row
 * that holds an element that is not finite lists nothing.  The argument list, the argument checks, the conventions (offsets == NULL is
 * one row per video), the REQUIRED mask, 1 <= n <= DRN_SHORTLIST_DEEP_MAX, 1 <= E <= DRN_BINARY_MAX_E, the workspace, the order, the
 * padding and the clamps are drn_shortlist_bin's.  Two launches on a plain table, three on a ragged one: phase one (16-byte loads of a
 * row's words when W % 4 == 0), then the merge of drn_shortlist_deep at every n, and the segment look-up.  No atomics, no host
 * synchronisation; the queries and the mask may change between replays of a captured graph. */
int drn_shortlist_bin_asym(const int32_t* codes, const void* queries, const int32_t* offsets, const int32_t* blk_vid, const int32_t* vid_blk,
                           const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S, int n, int dtype, void* ws,
                           int ws_keys, int32_t* ids, float* scores, int32_t* counts, int32_t* rows, void* stream);
/* The shortlist by LATE INTERACTION over a ragged table (drn_amd/csrc/retrieve_late.hip): queries [S][L][E] holds L token vectors a
 * sentence, lengths [S] int32 on the device says how many of them are live -- clamped into [0, L] on the device, never read on the host;
 * the contents of a token at or past it are not read.  sim[s][t][v] = drn_shortlist_segments_topn's score of (query row (s, t), video
 * v) -- the same MFMA chain per (token, row) and the same segmented maximum, so its bits are that entry's -- and score[s][v] = ((0 +
 * sim[s][0][v]) + sim[s][1][v]) + ... over the live tokens in ascending order, plain fp32 adds: it depends on the sentence's live tokens
 * and the video's rows alone, not on S, L, the padding, V, n, the other videos' offsets, the mask or the grid.  Sentence s lists the
 * videos that own a row, whose score is finite (a NaN or an infinity among the terms carries through) and whose mask bit is set, under
 * the total order of drn_shortlist_topn, cut to n; a sentence without live tokens lists nothing.  1 <= L <= DRN_LATE_MAX_TOKENS (a
 * choice that bounds one workgroup's time, not a measurement).  offsets, blk_vid, R, V, nblocks: the table and the block plan of
 * drn_shortlist_segments_topn (vid_blk is not needed: no segment is looked up).  allow: a packed mask as in the *_allow entries, or NULL
 * for none (allow_stride is then ignored).  ws: ws_keys >= S * nblocks * min(n, 256) 8-byte keys.  Two launches -- workgroup (block,
 * sentence) walks the sentence's live tokens in tiles of 16 against its block's rows, then the merge of drn_shortlist_topn -- no atomics,
 * no host synchronisation; lengths, the queries and the mask may change between replays of a captured graph.  The _q8 twin takes the
 * table as codes and scales (drn_shortlist_segments_topn_q8 says how) and answers bit for bit like the plain entry over the dequantised
 * table. */
#define DRN_LATE_MAX_TOKENS 64
int drn_shortlist_late_topn(const void* emb, const void* queries, const int32_t* lengths, const int32_t* offsets, const int32_t* blk_vid,
                            const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S, int L, int n, int dtype,
                            void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, void* stream);
int drn_shortlist_late_topn_q8(const uint8_t* codes, const uint8_t* scales, const void* queries, const int32_t* lengths,
                               const int32_t* offsets, const int32_t* blk_vid, const int32_t* allow, int allow_stride, int R, int V,
                               int nblocks, int E, int S, int L, int n, int dtype, void* ws, int ws_keys, int32_t* ids, float* scores,
                               int32_t* counts, void* stream);
/* The RANK OF A NAMED VIDEO in the full order of the three shortlists above (drn_amd/csrc/retrieve_rank.hip): targets [S] int32 on the
 * device, never read on the host; with t = targets[s], a CANDIDATE of sentence s being a video the matching *_topn entry could list
 * (it owns a row, its score is finite, its mask bit is set and -- late -- the sentence has a live token):
 *   total[s] = the number of candidates of s (the length of the list, were n unbounded);
 *   rank[s]  = the number of candidates that precede t under the total order of drn_shortlist_topn (score descending, then position
 *              ascending), score[s] = t's score, where 0 <= t < V and t is a candidate; rank[s] = -1 and score[s] = 0 otherwise (a value
 *              outside [0, V) is legal, is clamped for every read and means "no target").
 * So rank[s] = k >= 0 exactly when the entry's list with any n > k holds t at place k, with score[s] there, bit for bit: the scores
 * come from the same MFMA chain.  Counted over the WHOLE table: no cap at DRN_SHORTLIST_MAX, no list, no sort.  table is emb, or the
 * codes of a block-scaled FP8 table with scales beside them (scales == NULL: a plain table; E % 32 == 0 with scales); dtype is that
 * of the queries.  allow: a packed mask as in the *_allow entries, or NULL for none (allow_stride is then ignored).  queries [S][E],
 * or [S][L][E] with lengths [S] for drn_shortlist_late_rank; offsets, blk_vid, R, V, nblocks as in drn_shortlist_segments_topn.  ws:
 * ws_bytes >= 8 * S * (1 + blocks) bytes, 8-byte aligned, blocks = ceil(V / 256) on the plain table and nblocks on a ragged one (each
 * sentence's target key, then two int32 counts per (sentence, block)).  Three launches -- the target keys, the block counts, one
 * wavefront per sentence sums them -- no atomics, no host synchronisation; an answer depends on the sentence, its target, the table and
 * the mask alone, and targets, the queries, lengths and the mask may change between replays of a captured graph. */
int drn_shortlist_rank(const void* table, const uint8_t* scales, const void* queries, const int32_t* targets, const int32_t* allow,
                       int allow_stride, int V, int E, int S, int dtype, void* ws, int ws_bytes, int32_t* rank, float* score,
                       int32_t* total, void* stream);
int drn_shortlist_segments_rank(const void* table, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                const int32_t* blk_vid, const int32_t* targets, const int32_t* allow, int allow_stride, int R, int V,
                                int nblocks, int E, int S, int dtype, void* ws, int ws_bytes, int32_t* rank, float* score, int32_t* total,
                                void* stream);
int drn_shortlist_late_rank(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths, const int32_t* offsets,
                            const int32_t* blk_vid, const int32_t* targets, const int32_t* allow, int allow_stride, int R, int V,
                            int nblocks, int E, int S, int L, int dtype, void* ws, int ws_bytes, int32_t* rank, float* score,
                            int32_t* total, void* stream);
/* The rank entries OPENED INTO THEIR PHASES, for a corpus kept as several tables (below): the arguments of the matching entry above up
 * to dtype, then phase, keys, cnt, cnt_bytes.  phase 1 runs the entry's first launch alone: keys [S] = the 64-bit key of (s, targets[s])
 * in THIS table, 0 where the target is no candidate (cnt is not used and may be NULL).  phase 2 runs its second launch alone, reading
 * keys [S] as THRESHOLDS in the place of the target keys: cnt [S][blocks] pairs of int32 -- the candidates of the block whose key is
 * above keys[s], and its candidates -- blocks as in the entry's ws, cnt_bytes >= 8 * S * blocks (targets is not used and may be NULL).
 * keys and cnt are 8-byte aligned.  Any other phase is refused.  One launch; the kernels, and so every bit, are the entries' own. */
int drn_shortlist_rank_phase(const void* table, const uint8_t* scales, const void* queries, const int32_t* targets, const int32_t* allow,
                             int allow_stride, int V, int E, int S, int dtype, int phase, void* keys, void* cnt, int cnt_bytes,
                             void* stream);
int drn_shortlist_segments_rank_phase(const void* table, const uint8_t* scales, const void* queries, const int32_t* offsets,
                                      const int32_t* blk_vid, const int32_t* targets, const int32_t* allow, int allow_stride, int R, int V,
                                      int nblocks, int E, int S, int dtype, int phase, void* keys, void* cnt, int cnt_bytes, void* stream);
int drn_shortlist_late_rank_phase(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths,
                                  const int32_t* offsets, const int32_t* blk_vid, const int32_t* targets, const int32_t* allow,
                                  int allow_stride, int R, int V, int nblocks, int E, int S, int L, int dtype, int phase, void* keys,
                                  void* cnt, int cnt_bytes, void* stream);
/* RERANK A CANDIDATE LIST (drn_amd/csrc/retrieve_rerank.hip): candidates [S][C] int32 on the device, never read on the host, row s =
 * sentence s's SET of store positions: an entry outside [0, V) is no candidate (the -1 padding of a shortlist is one), and of a position
 * repeated in a row the first occurrence counts, across the whole row.  Only the listed (sentence, video) pairs are scored -- the rows
 * of the listed videos are the only table rows read -- and the answer is, field for field and bit for bit, what the matching *_topn
 * entry gives over the whole table under the mask "listed, and allowed": score[s][v] is drn_shortlist_late_topn's (the sum over the live
 * tokens, in ascending order, of the token's best row of v; with L = 1 that is drn_shortlist_segments_topn's score, and on a table of
 * one row per video drn_shortlist_topn's), a candidate owns a row, has a finite score and a set mask bit, the sentence has a live token,
 * and the order is drn_shortlist_topn's total order by STORE POSITION: the place of a video in the list means nothing.  table is emb,
 * or the codes of a block-scaled FP8 table with scales beside them (scales == NULL: a plain table; E % 32 == 0 with scales); dtype is
 * that of the queries [S][L][E].  lengths [S] as in drn_shortlist_late_topn, or NULL: every token is live.  offsets [V + 1] as in
 * drn_shortlist_segments_topn, or NULL: row v is video v (R == V).  allow: a packed mask as in the *_allow entries, or NULL for none
 * (allow_stride is then ignored).  1 <= C <= DRN_RERANK_MAX_CANDIDATES (a choice: the width of the candidates tensor
 * drn_plan_candidates takes, one row in 4 KiB of LDS), 1 <= n <= DRN_SHORTLIST_MAX (n > C is legal: the rest is padding).  ws: ws_keys >=
 * S * ceil(C / DRN_RERANK_GROUP) * min(n, DRN_RERANK_GROUP) 8-byte keys.  Two launches -- workgroup (group, sentence) scores the
 * DRN_RERANK_GROUP slots of its group (a choice, not a measurement), then the merge of drn_shortlist_topn -- no atomics, no host
 * synchronisation; an answer depends on the sentence, the set of its valid candidates, the table and the mask alone, and candidates,
 * the queries, lengths and the mask may change between replays of a captured graph. */
#define DRN_RERANK_MAX_CANDIDATES 1024
#define DRN_RERANK_GROUP 16
int drn_shortlist_rerank(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths, const int32_t* offsets,
                         const int32_t* candidates, const int32_t* allow, int allow_stride, int R, int V, int E, int S, int L, int C, int n,
                         int dtype, void* ws, int ws_keys, int32_t* ids, float* scores, int32_t* counts, void* stream);
/* THE SCORES OF THE LISTED PAIRS, the listed-pairs counterpart of drn_shortlist_scores: out[s * ld_out + j], fp32, for s < S and j < C,
 * ld_out >= C -- exactly those elements, and nothing past column C of a row -- column j beside candidates[s][j].  Every argument means
 * what it means in drn_shortlist_rerank, and the refusals are its own without n and ws; out is 4-byte aligned.  Slot j is LIVE under
 * exactly that entry's rule: its id lies in [0, V), no earlier slot of the whole row holds the same id, the mask bit is set, the video
 * owns a row and the sentence has a live token.  A live slot whose sum is finite gets the score drn_shortlist_rerank would list for the
 * pair -- the same kernel up to the sums: the same bits, a -0 written as +0 as the key folds it -- and EVERY other slot gets -inf: finite
 * <=> candidate, and no NaN is ever written.  inside_only != 0: a slot whose id lies outside [0, V) is LEFT UNTOUCHED instead, which is
 * what lets the K shards of a corpus write one matrix -- each the slots drn_shard_positions gave it -- in stream order.  ONE launch,
 * workgroup (group of DRN_RERANK_GROUP slots, sentence); no workspace, no atomics, no host synchronisation; the rows of videos that are
 * not listed are never read, and candidates, the queries, lengths and the mask may change between replays of a captured graph. */
int drn_shortlist_rerank_scores(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths,
                                const int32_t* offsets, const int32_t* candidates, const int32_t* allow, int allow_stride, int R, int V,
                                int E, int S, int L, int C, int dtype, int inside_only, float* out, int ld_out, void* stream);
/* mask [S][V], one byte a video (a torch.bool tensor: non-zero = allowed) -> words [S][ceil(V / 32)], the packed mask above: every
 * word written, bits at or past V zero.  S = 1 packs a mask shared by all sentences.  One launch, nothing read back. */
int drn_pack_allow(const uint8_t* mask, int S, int V, int32_t* words, void* stream);
/* A CORPUS KEPT AS K TABLES (drn_amd/csrc/retrieve_shard.hip): corpus position = bases[k] + position in shard k, bases [K + 1] int32 on
 * the device, the running sums of the shards' videos from 0; 1 <= K <= DRN_SHARDS_MAX (a choice, not a measurement).  Each shard is
 * ranked by its own *_topn entry; drn_shortlist_merge_lists merges the K lists of every sentence, stacked as in_ids, in_scores
 * [K][S][n_in], in_counts [K][S] and -- the lists of ragged shards -- in_rows [K][S][n_in], into ids, scores [S][n], counts [S] and rows
 * [S][n]; rows is given exactly when in_rows is (both NULL otherwise).  Entry (k, s, i) is a candidate iff i < min(in_counts[k][s],
 * n_in), 0 <= in_ids[k][s][i] < bases[k + 1] - bases[k] and its score is finite; sentence s lists its candidates by score descending,
 * then corpus position bases[k] + id ascending -- the total order of drn_shortlist_topn -- cut to n, a row travelling with its entry;
 * past the list ids = -1, scores = 0, rows = -1.  A score's bits do not depend on the table it was computed in and every shard cuts
 * its list under the same order, so with n_in >= n the result IS the list of the concatenated table, bit for bit.  Both n_in and n lie
 * in [1, DRN_SHORTLIST_MAX].  PRECONDITION: the ids of one list are distinct, as every shipped entry writes them (sorted, too; the
 * order of an input list is not relied on).  On other input the content of the list is unspecified; even then nothing outside the
 * outputs is written, nothing past n_in is read, and an id out of range never becomes a position.  One launch, one wavefront per
 * sentence; no atomics, no workspace, no host synchronisation; nothing is read on the host, so everything may change between replays
 * of a captured graph.  Lists gathered from other devices merge through the same entry. */
#define DRN_SHARDS_MAX 64
int drn_shortlist_merge_lists(const int32_t* in_ids, const float* in_scores, const int32_t* in_counts, const int32_t* in_rows,
                              const int32_t* bases, int K, int S, int n_in, int n, int32_t* ids, float* scores, int32_t* counts,
                              int32_t* rows, void* stream);
/* words [rows][ceil(V / 32)], a packed mask over the whole corpus (rows = 1: shared by all sentences) -> the K shards' own packed
 * masks, back to back in out: piece k is [rows][W_k], W_k = ceil(V_k / 32), V_k = bases[k + 1] - bases[k], from word rows * (W_0 + ... +
 * W_(k-1)); word w of a row holds the corpus bits bases[k] + 32 w .. + 31 (a base need not be a multiple of 32), the bits at or past
 * V_k zero.  Each piece is a legal allow argument of its shard's *_allow entry, 4-byte aligned.  total_words = W_0 + ... + W_(K-1), the
 * words a row `out` holds, computed by the caller from its host copy of bases; when the device's bases do not come to it nothing is
 * written.  bases as in drn_shortlist_merge_lists, not read on the host.  One launch, nothing read back. */
int drn_allow_slices(const int32_t* words, int rows, int V, const int32_t* bases, int K, int total_words, int32_t* out, void* stream);
/* RANK AND RERANK OVER THE K TABLES (drn_amd/csrc/retrieve_shard_rank.hip), every field bit for bit the single table's.
 * drn_shard_positions: positions [S][C] int32 on the device, corpus positions (targets: C = 1; candidate lists: C <=
 * DRN_RERANK_MAX_CANDIDATES) -> out [K][S][C]: out[k] = positions - bases[k] where bases[k] <= positions < bases[k + 1], else -1,
 * compared and subtracted in 64 bits (INT_MIN and INT_MAX land in no shard); every value read from bases is clamped at 0.  Slice [k] is
 * a legal targets / candidates argument of shard k's entries.  A rerank is then each shard's drn_shortlist_rerank on its slice and
 * drn_shortlist_merge_lists. */
int drn_shard_positions(const int32_t* positions, const int32_t* bases, int K, int S, int C, int32_t* out, void* stream);
/* keys [K][S], the target keys phase 1 of the *_rank_phase entries wrote in each shard for the local targets of drn_shard_positions
 * (at most one per column is not 0) -> thresholds [K][S] for phase 2 and key [S].  With kt the LOWEST shard whose key tk is not 0 and
 * tw = tk >> 32: thresholds[k][s] = (tw << 32) - 1 for k < kt (an equal score there lies at a lower corpus position and precedes), tk
 * for k == kt, (tw << 32) | 0xffffffff for k > kt (an equal score there follows), and key[s] = tk; where every key is 0 the
 * thresholds are all ones and key[s] = 0.  All 8-byte aligned.  One launch, one wavefront per sentence. */
int drn_shortlist_rank_thresholds(const void* keys, int K, int S, void* thresholds, void* key, void* stream);
/* key [S] and the K shards' phase-2 counts back to back in cnt -- region k is [S][blk_off[k + 1] - blk_off[k]] pairs from pair
 * S * blk_off[k]; blk_off [K + 1] int32 on the device, the running sums of the shards' blocks from 0, blocks = blk_off[K] as the host
 * knows it (every value read from blk_off is clamped into [0, blocks]), cnt_bytes >= 8 * S * blocks -> rank, score, total [S] as in
 * drn_shortlist_rank: the sums over all blocks, rank = -1 and score = 0 where key[s] == 0, else score = the key's.  One launch, one
 * wavefront per sentence.  All three: no atomics, no workspace beyond what is passed, nothing read on the host. */
int drn_shortlist_rank_reduce_shards(const void* key, const void* cnt, int cnt_bytes, const int32_t* blk_off, int K, int S, int blocks,
                                     int32_t* rank, float* score, int32_t* total, void* stream);
/* COMPACTING THE K TABLES INTO ONE (drn_amd/csrc/retrieve_compact.hip; drn_amd.retrieve.compact_reference is the definition): the
 * videos a packed mask keeps, in corpus order, in a new table.  drn_compact_plan is launched once per shard, k = 0 .. K - 1, IN STREAM
 * ORDER: keep [ceil(V / 32)] is the shard's own piece of the mask as drn_allow_slices cuts it (NULL: every video is kept), offsets
 * [V + 1] the shard's own on a ragged shard (NULL: one row a video), V the shard's videos.  carry [K + 1][2] int32 holds (videos kept,
 * rows kept) BEFORE each shard: launch k reads carry[k] -- launch 0 writes it, zeros -- and writes carry[k + 1], so carry[K] is (V',
 * R') of the new table and the launches need nothing else from each other.  positions [V] is the SHARD'S slice of the corpus's map:
 * the new position of each video, -1 where it is dropped.  new_offsets [cap] (given exactly when offsets is) gets, at the new position
 * of every kept video, the rows kept before it, and at carry[k + 1].videos the rows kept so far: after launch K - 1 its first V' + 1
 * entries are the new table's offsets; an index at or past cap is never written (cap = the corpus's videos + 1 is always enough).  An
 * exclusive scan by ONE workgroup a launch: no workgroup waits on another, no flag, no atomics, no workspace, nothing read on the host. */
int drn_compact_plan(const int32_t* keep, const int32_t* offsets, int V, int k, int K, int cap, int32_t* carry, int32_t* positions,
                     int32_t* new_offsets, void* stream);
/* One launch per shard: the kept rows of the shard to their places.  src is the shard's plain rows [src_rows][E] in `dtype`, or its
 * codes [src_rows][E] u8 with src_scales [src_rows][E / 32] (src_format DRN_COMPACT_MX8); src_offsets and positions as the shard gave
 * them to drn_compact_plan and as it wrote them; dst_offsets [dst_videos + 1] the new table's offsets (given exactly when src_offsets
 * is), dst_videos = V'.  Video v with p = positions[v] in [0, dst_videos) owns the source rows src_offsets[v] .. src_offsets[v + 1] - 1
 * (row v) and its row j goes to row dst_offsets[p] + j (row p) of the new table; dst (and dst_scales) is a WINDOW of that table or a
 * staging buffer for it, holding its rows [dst_row0, dst_row0 + dst_rows): a row outside the window is not written, and nothing else
 * is.  The pairs: plain -> plain, the values as they are; FP8 -> FP8, codes and scale bytes byte for byte (nothing is requantised);
 * FP8 -> plain, float(code) * 2^(scale - 127) in `dtype`, exact.  plain -> FP8 is REFUSED: the caller stages plain rows and runs
 * drn_quantize_rows_mx8, the one quantiser.  E % 32 == 0 with an FP8 side; dtype is that of the plain side (of the queries when there
 * is none).  16-byte accesses when every base pointer and row pitch allows it, one element a lane otherwise; 64-bit row addresses; a
 * bounded grid.  No atomics, no workspace, nothing read on the host. */
#define DRN_COMPACT_PLAIN 0
#define DRN_COMPACT_MX8 1
int drn_compact_rows(const void* src, const uint8_t* src_scales, const int32_t* src_offsets, const int32_t* positions,
                     const int32_t* dst_offsets, int V, int src_rows, int E, int src_format, int dst_format, int dtype, int dst_videos,
                     int dst_row0, int dst_rows, void* dst, uint8_t* dst_scales, void* stream);
/* POOLING A RAGGED TABLE'S SEGMENTS INTO A COARSE TABLE (drn_amd/csrc/retrieve_pool.hip; drn_amd.retrieve.pool_segments_reference is the
 * definition, bit for bit).  table is the plain rows [R][E] in `dtype`, or the codes [R][E] u8 of a block-scaled FP8 table with scales
 * [R][E / 32] beside them (scales == NULL: a plain table; E % 32 == 0 with scales); offsets [V + 1] the table's own.  out [R_out][E] is
 * ALWAYS plain rows in `dtype` (a caller that wants FP8 runs drn_quantize_rows_mx8, the one quantiser, over them) and a WINDOW of the
 * pooled table: its rows [out_row0, out_row0 + R_out) -- the whole table with out_row0 = 0, or a staging buffer's chunk of it.
 *   group == 0, out_offsets == NULL: one row a video, out_row0 + R_out <= V; row v pools the rows offsets[v] .. offsets[v + 1] - 1, and a video
 *     without rows gives a row of +0;
 *   group = g >= 1, out_offsets [V + 1] given: video v owns the output rows out_offsets[v] .. out_offsets[v + 1] - 1 (the caller made
 *     them: ceil(len_v / g) each, running sums from 0), and its row j pools the source rows offsets[v] + j g .. + g - 1, cut at
 *     offsets[v + 1].
 * how = DRN_POOL_MEAN: an fp32 accumulator from +0, the group's rows added in ASCENDING row order, one fp32 add a row, one correctly
 * rounded fp32 division by float(count), one rounding to `dtype` (nearest even); DRN_POOL_MAX: the first row, then acc = x > acc ? x :
 * acc in ascending order -- the maximum, exact, and of two zeros of either sign the earlier row's.  A source value of an FP8 table is
 * float(code) * 2^(scale - 127), exact.  So a row's bits depend on its group's rows alone, not on V, the grid or the other videos.
 * The table and out are 16-byte aligned, 1 <= R_out < 2^31; every index read from offsets and out_offsets is clamped, and nothing is
 * written outside out's R_out * E elements, every one of which is.  One launch: one wavefront per (output row, slab of 512 bf16 / 256
 * fp32 columns), so few videos with very long runs fill little of the chip.  No atomics, no LDS, no workspace, nothing read on the host. */
#define DRN_POOL_MEAN 0
#define DRN_POOL_MAX 1
int drn_pool_segments(const void* table, const uint8_t* scales, const int32_t* offsets, const int32_t* out_offsets, int R, int V, int R_out,
                      int out_row0, int E, int group, int how, int dtype, void* out, void* stream);
/* DENSE SCORES AND FUSED SHORTLISTS (drn_amd/csrc/retrieve_fuse.hip; drn_amd.retrieve.scores_reference, fuse_scores_reference,
 * fused_shortlist_reference and fused_rank_reference are the definitions).
 *
 * drn_shortlist_scores writes the WHOLE score matrix the shortlist entries rank and throw away: out[s * ld_out + v], fp32, for s < S and
 * v < V, ld_out >= V -- exactly those elements and nothing else.  table is emb, or the codes of a block-scaled FP8 table with scales
 * beside them (scales == NULL: a plain table; E % 32 == 0 with scales); dtype is that of the queries.  offsets == NULL: one row per
 * video -- blk_vid and lengths must then be NULL too, R and nblocks are ignored and L must be 1; otherwise offsets and blk_vid are the
 * table and block plan of drn_shortlist_segments_topn.  lengths == NULL: queries [S][E], L must be 1; otherwise late interaction,
 * queries [S][L][E] and lengths [S] as in drn_shortlist_late_topn.  allow: a packed mask as in the *_allow entries, or NULL for none.
 * out[s][v] is the score the matching *_topn entry gives the pair -- the same MFMA chain, the same segmented maximum, the same token
 * fold: its bits are the listed score's, a -0 written as +0 as the key folds it -- and -inf where the video is NO CANDIDATE: it owns no
 * row, its score is not finite, its mask bit is clear or (late) the sentence has no live token.  So finite <=> candidate, and no NaN
 * is ever written.  A block whose mask words are all clear for the tile reads no table row and writes its -inf all the same.  Every
 * index read from a device table is clamped.  out is 4-byte aligned.  ONE launch, no workspace, no atomics, no host synchronisation;
 * the queries, lengths and the mask may change between replays of a captured graph. */
int drn_shortlist_scores(const void* table, const uint8_t* scales, const void* queries, const int32_t* lengths, const int32_t* offsets,
                         const int32_t* blk_vid, const int32_t* allow, int allow_stride, int R, int V, int nblocks, int E, int S, int L,
                         int dtype, float* out, int ld_out, void* stream);
/* The FUSED score of M stacked score matrices, element (m, s, v) at scores[m * stride_m + s * ld + v], ld >= V, under weights [M] fp32
 * ON THE DEVICE (never read on the host), 1 <= M <= DRN_FUSE_MAX_TABLES (a CHOICE, not a measurement: the tables a sentence's score
 * is folded over), in a FIXED order, in fp32, two roundings a term (a multiply, then an add: no FMA):
 *   acc = +0;  for m = 0 .. M - 1 ascending:  present = isfinite(scores[m][s][v]);
 *     mode DRN_FUSE_DROP:  acc = acc + (w[m] * scores[m][s][v]);      DRN_FUSE_SKIP:  if present: acc = acc + (w[m] * scores[m][s][v]);
 *   candidate = isfinite(acc) and allowed(s, v) and (DROP: every m present | SKIP: some m present).
 * drn_shortlist_fuse_topn lists each sentence's candidates by fused score descending, then position ascending, cut to n, 1 <= n <=
 * DRN_SHORTLIST_DEEP_MAX, into ids / out_scores [S][n] and counts [S] with the -1 / 0 padding of drn_shortlist_topn.  ws: ws_keys >= S *
 * ceil(V / 256) * min(n, 256) 8-byte keys.  Two launches: workgroup (block of 256 videos, sentence) fuses, sorts and writes min(n, 256)
 * keys; then the merge of drn_shortlist_topn (n <= DRN_SHORTLIST_MAX) or of drn_shortlist_deep (above).  With M = 1 and w = 1 this
 * ranks ANY score matrix under the total order: 0 + 1 * s is exact.
 * drn_shortlist_fuse_rank answers drn_shortlist_rank's three fields under the fused score: targets [S] int32 on the device (a value
 * outside [0, V) means "no target" and is clamped for every read), rank = the candidates whose fused key precedes the target's (-1
 * where the target is no candidate), score = the target's fused score (0 beside -1), total = the candidates.  ONE launch, one
 * workgroup per sentence walks the V videos; no workspace.
 * allow: a packed mask as in the *_allow entries, or NULL.  scores and weights are 4-byte aligned.  No atomics, no host
 * synchronisation; the matrices, the weights, the targets and the mask may change between replays of a captured graph. */
#define DRN_FUSE_MAX_TABLES 8
#define DRN_FUSE_DROP 0
#define DRN_FUSE_SKIP 1
int drn_shortlist_fuse_topn(const float* scores, long long stride_m, int ld, const float* weights, int M, int mode, const int32_t* allow,
                            int allow_stride, int V, int S, int n, void* ws, int ws_keys, int32_t* ids, float* out_scores, int32_t* counts,
                            void* stream);
int drn_shortlist_fuse_rank(const float* scores, long long stride_m, int ld, const float* weights, int M, int mode, const int32_t* targets,
                            const int32_t* allow, int allow_stride, int V, int S, int32_t* rank, float* score, int32_t* total, void* stream);
/* THE FUSED RERANK: drn_shortlist_fuse_topn over LISTED pairs.  scores holds M stacked [S][C] matrices, element (m, s, j) at
 * scores[m * stride_m + s * ld + j], ld >= C, column j belonging to the video candidates[s][j] -- what drn_shortlist_rerank_scores writes,
 * though ANY matrices are safe: candidates [S][C] int32 on the device as in drn_shortlist_rerank, 1 <= C <= DRN_RERANK_MAX_CANDIDATES, and
 * slot j is LISTED, by this entry's own reading of the row, when its id lies in [0, V), no earlier slot of the row holds the same id and
 * its mask bit is set (a mask word is read only for an id already known to lie in [0, V)).  The fold, the modes and the presence rule
 * are drn_shortlist_fuse_topn's, statement for statement; a slot is a candidate when it is listed, its acc is finite and it passes the
 * mode's rule.  The key carries the REAL store position, so the order among the listed is the full fused shortlist's total order and
 * the place of a video in the list means nothing: the answer is drn_shortlist_fuse_topn's over [S][V] matrices under the mask "listed,
 * and allowed".  1 <= n <= DRN_SHORTLIST_DEEP_MAX (n > C is legal: the rest is padding); ws: ws_keys >= S * ceil(C / 256) * min(n, 256)
 * 8-byte keys.  Two launches: workgroup (block of 256 slots, sentence) fuses, sorts and writes min(n, 256) keys; then the merge of
 * drn_shortlist_topn (n <= DRN_SHORTLIST_MAX) or of drn_shortlist_deep (above), whose premise -- no video twice -- the rule above keeps.
 * No atomics, no host synchronisation; the matrices, the weights, candidates and the mask may change between replays of a captured
 * graph. */
int drn_shortlist_fuse_rerank(const float* scores, long long stride_m, int ld, const float* weights, int M, int mode,
                              const int32_t* candidates, const int32_t* allow, int allow_stride, int V, int C, int S, int n, void* ws,
                              int ws_keys, int32_t* ids, float* out_scores, int32_t* counts, void* stream);
/* RANK FUSION (drn_amd/csrc/retrieve_rrf.hip; drn_amd.retrieve.rank_fuse_reference and rank_fuse_rank_reference are the definitions):
 * reciprocal-rank fusion of M finished id lists over the same V videos, for tables whose scores share no scale.  lists holds M stacked
 * [S][C] int32 matrices ON THE DEVICE, element (m, s, j) at lists[m * stride_m + s * ld + j], ld >= C, 1 <= M <= DRN_RANK_FUSE_MAX_LISTS (a
 * CHOICE: M * C words of 8 bytes fill 64 KiB of LDS), 1 <= C <= DRN_SHORTLIST_DEEP_MAX -- other shortlists' ids as they lie on the device.
 * An entry outside [0, V) means nothing (-1, V, INT_MIN, INT_MAX), and of a position repeated in one row of one list the first
 * occurrence counts; the RANK of video v in list m is the column j of that first occurrence.  weights [M] fp32 ON THE DEVICE (never read
 * on the host); k0 >= 0 and finite.  In fp32, nothing contracted:
 *   acc = +0;  for m ascending over the lists that hold v:  acc = acc + w[m] / (k0 + float(j + 1))      (the division correctly rounded)
 *   candidate = isfinite(acc) and allowed(s, v) and (DRN_FUSE_SKIP: some list holds v | DRN_FUSE_DROP: every list holds v).
 * drn_rank_fuse_topn lists each sentence's candidates by acc descending, then position ascending, cut to n, 1 <= n <=
 * DRN_SHORTLIST_DEEP_MAX, into ids / scores [S][n] and counts [S] with the -1 / 0 padding of drn_shortlist_topn.  drn_rank_fuse_rank
 * answers drn_shortlist_rank's three fields in that order: targets [S] int32 on the device (a value outside [0, V) means "no target"; it
 * is compared, never used as an index), rank = the candidates that precede the target (-1 where it is no candidate), score = its acc (0
 * beside -1), total = the candidates.  allow: a packed mask as in the *_allow entries, or NULL; a mask word is read only for an id
 * already known to lie in [0, V).  Every pointer is 4-byte aligned.  ONE launch each, one workgroup per sentence: the entries are sorted
 * in LDS (a power of two >= M * C words, 256 to 8192), folded, and the candidates sorted again; no workspace, no atomics, no host
 * synchronisation; the lists, the weights, the targets and the mask may change between replays of a captured graph. */
#define DRN_RANK_FUSE_MAX_LISTS 8
int drn_rank_fuse_topn(const int32_t* lists, long long stride_m, int ld, int C, int M, int V, const float* weights, float k0, int mode,
                       const int32_t* allow, int allow_stride, int S, int n, int32_t* ids, float* scores, int32_t* counts, void* stream);
int drn_rank_fuse_rank(const int32_t* lists, long long stride_m, int ld, int C, int M, int V, const float* weights, float k0, int mode,
                       const int32_t* allow, int allow_stride, int S, const int32_t* targets, int32_t* rank, float* score, int32_t* total,
                       void* stream);
/* The data half of Grounder.search(candidates= a device tensor): cand [S][N] int32 on the device, row s = sentence s's set of
 * positions in a store of Nv videos (an entry outside [0, Nv) is no candidate; of a position repeated in a row the first occurrence
 * counts, across the whole row), 1 <= N <= DRN_CANDIDATES_MAX (a choice: one row is held in 4 KiB of LDS) -> table [steps][pairs], the
 * pair_video rows drn_merge_moments_ragged reads: step sb * ceil(N / Nc) + cb holds the sentences [sb * Sc, + Sc) and the columns
 * [cb * Nc, + Nc), its pair sl * Nc + jl is (sentence sb * Sc + sl, column cb * Nc + jl) and gets that entry's position, or -1 for no
 * candidate, a sentence or column past S or N, or a pair at or past Sc * Nc.  1 <= Sc <= S, 1 <= Nc <= N, Sc * Nc <= pairs and
 * steps == ceil(S / Sc) * ceil(N / Nc), refused otherwise.  Every element of the table is written; one launch, nothing read back. */
#define DRN_CANDIDATES_MAX 1024
int drn_plan_candidates(const int32_t* cand, int S, int N, int Nv, int Sc, int Nc, int pairs, int steps, int32_t* table, void* stream);

/* ---- query-encoder glue (drn_amd/csrc/qenc.hip; model/language_module.py:17-63), all fp32 ----------------------
 * Word embedding lookup written time-major (L, B, E) and its dense gradient (row padding_idx stays zero). */
int drn_qe_embed_fwd(const int64_t* tokens /*[B][L]*/, const float* table /*[V][E]*/, float* out_tm, int B, int L, int E, void* stream);
int drn_qe_embed_bwd(const int64_t* tokens, const float* demb_tm, float* dtable /*[V][E], fully written*/, int B, int L, int E, int V,
                     int padding_idx, void* stream);
/* q_vector = [output[b][0] ; output[b][len_b-1]] (language_module.py:48-54); bwd ADDS into dout (B, L, C). */
int drn_qe_qvec_fwd(const float* out /*[B][L][C]*/, const int64_t* lengths, float* qvec /*[B][2C]*/, int B, int L, int C, void* stream);
int drn_qe_qvec_bwd(const float* dqvec, const int64_t* lengths, float* dout, int B, int L, int C, void* stream);
/* The three attention "commands" (language_module.py:17-36): logits = cmd_inter2logits(q_cmd[:,None,:] * output),
 * softmax over the words of each query (padding masked), cmd = att @ output.  qcmd (B,3,C), att (B,3,L), cmds (3,B,C).
 * bwd: dcmd0..2 (B,C) each or NULL; writes dqcmd (B,3,C), dout (B,L,C) and per-clip partials dw_part (B,C), dbias_part (B)
 * of the cmd_inter2logits weight / bias gradients (sum them over B). */
int drn_qe_attn_fwd(const float* out, const float* qcmd, const float* w /*[C]*/, const float* bias /*[1]*/, const int64_t* lengths,
                    float* att, float* cmds, int B, int L, int C, void* stream);
int drn_qe_attn_bwd(const float* dcmd0, const float* dcmd1, const float* dcmd2, const float* att, const float* out, const float* qcmd,
                    const float* w, const int64_t* lengths, float* dqcmd, float* dout, float* dw_part, float* dbias_part, int B, int L,
                    int C, void* stream);
/* dst_s[j] = sum_m X[m][col0_s + j] for up to DRN_COLSEG_MAX column ranges of one fp32 matrix (bias gradients). */
#define DRN_COLSEG_MAX 8
typedef struct {
  float* dst;
  int32_t col0, n;
} DrnColSeg;
int drn_colsum_segs(const float* X, int ld, int M, const DrnColSeg* segs /*host*/, int nsegs, void* stream);

/* ---- batch-sized dense layers of the query side (drn_amd/csrc/qdense.hip; model/language_module.py:13-23,38-63,
 * model/main_model.py:36-50), fp32, exact-fp32 MFMA, GROUPED: one launch serves up to DRN_QD_MAX problems.
 * drn_skinny_group:  Y[M][N] = X[M][K] * W[N][K]^T (+ bias[N]) (ReLU) (zeroed where mask[m][n] <= 0), M <= 64 rows, any N,
 *   K % 4 == 0: qInput* / the gate projections / the LSTM input projection forward, and -- through cached transposed
 *   weight copies -- their input gradients (mask = the ReLU of the layer in front).  Long K is split over workgroups; the
 *   last-arriving workgroup of a column tile adds the partial tiles in a fixed order (deterministic, no second launch):
 *   ws >= drn_skinny_group_ws_elems() floats, counters = DRN_QD_COUNTERS int32 zeros owned by the caller (the kernel
 *   leaves them zero).
 * drn_outer_wgrad:  dW[N][K] = sum_m dY[m][N] * X[m][K] (row stride ldw), db[N] = db2[N] = sum_m dY[m][N] (optional):
 *   the weight / bias gradients of the same layers (M = clips, or clips x words for the LSTM weights).  A problem with
 *   dW == NULL only produces the column sums.  dtype DRN_F32: exact-fp32 MFMA; DRN_BF16 (the bf16 model): the fp32 operands are
 *   rounded to bf16 as they enter the MFMA (fp32 accumulation, fp32 results; the column sums stay exact). */
#define DRN_QD_MAX 16
#define DRN_QD_COUNTERS 2048
typedef struct DrnSkinnyDesc {
  const void* X;     /* fp32 rows, or bf16 rows when x_dtype == DRN_BF16 (K % 8 == 0, ldx % 8 == 0 elements): the weights are then
                        rounded to bf16 on load and the product accumulates in fp32 on the bf16 MFMA */
  const float* W;
  const float* bias; /* or NULL */
  const float* mask; /* or NULL; [M][ldm] */
  float* Y;
  int32_t ldx, ldy, ldm, M, N, K, relu;
  int32_t x_dtype;   /* DRN_F32 (0) or DRN_BF16; the same for every problem of a launch */
} DrnSkinnyDesc;
int64_t drn_skinny_group_ws_elems(const DrnSkinnyDesc* descs /*host*/, int n);
int drn_skinny_group(const DrnSkinnyDesc* descs /*host*/, int n, float* ws, int32_t* counters, void* stream);
typedef struct DrnOuterDesc {
  const float* dY;
  const float* X;
  float* dW;
  float* db;  /* or NULL */
  float* db2; /* or NULL */
  int32_t ldy, ldx, ldw, M, N, K;
} DrnOuterDesc;
int drn_outer_wgrad(const DrnOuterDesc* descs /*host*/, int n, int dtype, void* stream);

/* ---- language-guided pooling (drn_amd/csrc/lgp.hip; model/LGP.py:29-51) ---------------------------------------
 * x (B, t, C) channels-last, qn (B, C) fp32 = BN(conv1x1(query)) prepared by the caller, out (B, t/2, C),
 * att (B, t/2, 2) fp32 (saved for backward).  C <= 2048 (bf16) / 1024 (f32). */
int drn_lgp_fwd(const void* x, int ldx, const float* qn, void* out, int ld_out, float* att, int B, int t, int C, int dtype,
                void* stream);
/* dx (B, t, C) and dqn (B, C) = gradient w.r.t. qn; ws >= B*ceil(t/8)*C floats. */
int drn_lgp_bwd(const void* x, int ldx, const float* qn, const float* att, const void* dout, int ld_dout, void* dx, int ld_dx,
                float* dqn, float* ws, int B, int t, int C, int dtype, void* stream);

/* ---- query-encoder BiLSTM recurrence (drn_amd/csrc/lstm.hip; model/language_module.py:13-15,38-45) ------------
 * One launch per time step for both directions; sequence lengths (int64) on the device (replaces pack_padded_sequence +
 * the cuDNN/MIOpen RNN).  fp32, gate order i,f,g,o.  xproj / gates / dgates are [L][B][2][4H] indexed by time and
 * direction (one (L*B) x 8H matrix); xproj = x_t W_ih^T without biases (b_ih + b_hh are added here); hseq/cseq
 * [2][L+1][B][H] by step (slot 0 is never read: zero initial state); hprev_t [L][B][2][H] = hidden state that entered
 * time t (operand of the W_hh gradient); out [B][L][2H].  Step s handles t = s (forward direction) and t = L-1-s
 * (reverse).  B <= 64, H % 64 == 0.  w_dtype: DRN_F32 (exact-fp32 MFMA, the parity mode) or DRN_BF16 (Whh_* / WhhT_* are bf16
 * copies in the same element order, H % 128 == 0: the hidden state / gate gradients are rounded to bf16 as they are loaded,
 * products accumulate in fp32; states, gates and every output stay fp32).  qvec (optional, [B][4H]): the sentence vector [out[b][0][:] ; out[b][len_b-1][:]]
 * (language_module.py:48-54), each half-row written by the step that produces it -- no gather launch after the recurrence.
 * hseq16 (optional, fp16 [2][L+1][B][H], with fp32 weights and H % 128 == 0): every step also writes its state there and reads the
 * previous one from there; the recurrent product then runs on the fp16 MFMA (W_hh rounded in registers, fp32 accumulation). */
int drn_lstm_step_fwd(const float* xproj, const void* Whh_f, const void* Whh_r, int w_dtype, const float* b_ih_f, const float* b_hh_f,
                      const float* b_ih_r, const float* b_hh_r, float* hseq, float* cseq, float* gates, float* out, float* hprev_t,
                      float* qvec, void* hseq16, const int64_t* lengths, int B, int L, int H, int s, void* stream);
/* The hseq16 forward with ALL steps in ONE launch (the bits of L drn_lstm_step_fwd launches): workgroups stay for the whole sequence and
 * hand the hidden state over through xch_ws -- 64-byte aligned, >= drn_lstm_seq_fwd_ws_bytes(B, L, H) bytes, ZERO before its first use and
 * then left to the library (one buffer per (B, L, H); launches on it are stream-ordered).  H % 128 == 0, fp32 W_hh.  DRN_ERR_UNSUPPORTED
 * (nothing launched) when the grid does not fit the chip at once.  drn_lstm_seq_fwd_timeouts: workgroups that gave up waiting (2 s
 * watchdog; 0 in a healthy run); synchronises the device. */
int64_t drn_lstm_seq_fwd_ws_bytes(int B, int L, int H);
int drn_lstm_seq_fwd(const float* xproj, const void* Whh_f, const void* Whh_r, const float* b_ih_f, const float* b_hh_f, const float* b_ih_r,
                     const float* b_hh_r, float* hseq, float* cseq, float* gates, float* out, float* hprev_t, float* qvec, void* xch_ws,
                     int64_t ws_bytes, const int64_t* lengths, int B, int L, int H, void* stream);
int drn_lstm_seq_fwd_timeouts(int reset);
/* Backward: drn_lstm_bwd_first does the cell backward of the last step (s = L-1) from dout [B][L][2H] alone; then
 * drn_lstm_step_bwd for s = L-1 .. 1 propagates through W_hh of step s (dgates[t(s)] x Whh) and applies the cell backward
 * of step s-1 in its epilogue (the recurrent dL/dh never goes to memory).  dgates is the operand of the weight-gradient
 * GEMMs; dc / dh_pass are [2][B][H] running state.  WhhT_* = Whh^T as [H][4H].  dqvec (optional, [B][4H]): gradient of the
 * sentence vector, added to dout rows 0 and len_b-1 as they are read (dout itself is not modified).  dgates16 (optional, with
 * w_dtype DRN_BF16): a bf16 buffer shaped like dgates; the cell backward writes a rounded copy of every gate gradient there and the
 * recurrent product reads that copy (half the bytes) -- dgates itself stays fp32 for the weight / input-gradient products. */
int drn_lstm_bwd_first(const float* dout, const float* gates, const float* cseq, float* dgates, float* dc, float* dh_pass,
                       const float* dqvec, void* dgates16, const int64_t* lengths, int B, int L, int H, void* stream);
int drn_lstm_step_bwd(const float* dout, const float* gates, const float* cseq, const void* WhhT_f, const void* WhhT_r, int w_dtype,
                      float* dgates, float* dc, float* dh_pass, const float* dqvec, void* dgates16, const int64_t* lengths, int B, int L,
                      int H, int s, void* stream);

/* ---- fused clip_grad_norm_ + Adam over flat gradient buckets (drn_amd/csrc/optim.hip; main.py:140,238-243) ---- */
int64_t drn_opt_nblocks(int64_t n); /* partial sums produced by drn_sumsq_partials for n elements */
/* partials[b] = sum of g^2 over block b; step_counter (device int, or NULL) is incremented once per call. */
int drn_sumsq_partials(const float* g, int64_t n, float* partials, int* step_counter, void* stream);
/* total_sumsq[0] = grad_scale^2 * sum of ALL buckets' partials, one workgroup, fixed order: the squared global norm of the
 * gradients the Adam kernels see, grad_scale * g (grad_scale = 1/world when the buckets hold the all-reduced SUM; 1 otherwise). */
int drn_sumsq_finalize(const float* partials, int npartials, float* total_sumsq, float grad_scale, void* stream);
/* The norm pass WITHOUT the gradients whose squared sums the producing kernels left behind (one process only: after an all-reduce
 * the producers' sums are stale).  drn_sumsq_partials_skip: elements in the nskip <= DRN_SUMSQ_MAX_SKIP ranges [skip_lo[i],
 * skip_hi[i]) (host arrays, element offsets into g) are not read.  drn_sumsq_finalize2 adds next <= DRN_SUMSQ_MAX_EXT external
 * partial arrays (host arrays of device pointers / lengths: DrnGemmDesc::sumsq of the prop_fc weight gradient,
 * drn_wgrad_reduce_pending's sumsq) to the pass's own partials, everything in a fixed order. */
#define DRN_SUMSQ_MAX_SKIP 16
#define DRN_SUMSQ_MAX_EXT 8
int drn_sumsq_partials_skip(const float* g, int64_t n, float* partials, int* step_counter, const int64_t* skip_lo /*host*/,
                            const int64_t* skip_hi /*host*/, int nskip, const unsigned char* block_classes /*device or NULL*/, void* stream);
/* Host helper: block_classes[b] for the drn_opt_nblocks(n) blocks of that pass (0 = clear of every range, 1 = inside one, 2 = on a
 * boundary); uploaded once per range set, it spares every block the walk over the ranges. */
int drn_sumsq_block_classes(int64_t n, const int64_t* skip_lo /*host*/, const int64_t* skip_hi /*host*/, int nskip, unsigned char* classes /*host*/);
int drn_sumsq_finalize2(const float* partials, int npartials, const float* const* ext /*host*/, const int32_t* ext_n /*host*/, int next,
                        float* total_sumsq, float grad_scale, void* stream);
/* One bucket: g/m/v flat [n]; tensor i covers [seg_start[i], seg_start[i+1]) and lives at p_ptr[i] (both tables on the
 * device).  blk_seg (device, drn_opt_nblocks(n) ints, or NULL): index of the tensor holding element 4096*b, so a block
 * does not search the table.  mirror_dev (device table of nseg pointers, or NULL; entries may be NULL): a bf16 copy of tensor
 * i in the same element order (the GEMM operand of a Linear / 1x1 conv), rewritten from the updated value in the same pass.
 * Every gradient is read as grad_scale * g; clip coef = min(1, max_norm/(sqrt(total_sumsq)+1e-6)) (max_norm<=0: off). */
int drn_adam_bucket(const float* g, float* m, float* v, int64_t n, const int64_t* seg_start_dev, float* const* p_ptr_dev, int nseg,
                    const int32_t* blk_seg, void* const* mirror_dev, const float* total_sumsq, const int* step_counter, float lr,
                    float beta1, float beta2, float eps, float max_norm, float grad_scale, void* stream);

/* The same update for tensors whose GEMM operands are RE-LAID copies (conv weights (Cout, Cin, k) as [Cout][k][Cin] and
 * [Cin][k][Cout]; Linear weights transposed): the tensor is walked in 64 x 64-channel tiles instead of linearly, each tile's
 * updated values pass through LDS and leave as 16-byte pieces of BOTH copies -- the per-step drn_pack_weights launches over
 * these tensors (76 us per step) disappear.  items: DEVICE array; blk_item / blk_tile: device, one int per workgroup (which
 * item, which tile of it), nblocks of them.  The caller leaves these tensors out of drn_adam_bucket (NULL in p_ptr_dev). */
typedef struct DrnAdamTiledItem {
  float* p;        /* parameter, R x (C*k) row-major fp32 */
  int64_t off;     /* its offset inside the flat g / m / v buffers */
  void* m1;        /* copy [r][tap][c]: element (r, c, tap) at m1[(r*k + tap)*ld1 + c], or NULL */
  void* m2;        /* copy [c][tap][r]: element (r, c, tap) at m2[(c*k + tap)*ld2 + r], or NULL */
  int64_t ld1, ld2;
  int32_t R, C, k;
  int32_t code1, code2; /* dtype of m1 / m2: DRN_F32 or DRN_BF16 */
  int32_t tiles_c;      /* ceil(C / 64) */
} DrnAdamTiledItem;
int drn_adam_tiled(const float* g, float* m, float* v, const DrnAdamTiledItem* items_dev, const int32_t* blk_item_dev,
                   const int32_t* blk_tile_dev, int nblocks, const float* total_sumsq, const int* step_counter, float lr, float beta1,
                   float beta2, float eps, float max_norm, float grad_scale, void* stream);

/* Proposal features from a device-resident feature store (drn_amd.store; replaces the reference's per-sample host loop,
 * dataset.py:118-154 + the collate padding 180-224, on the device): for clip b with video v = vids[b], n = prop_off[v+1] - prop_off[v]
 * and proposal t < n with [lo, hi] = win[prop_off[v] + t],
 *   out[b][t][:]  = element-wise max over rows seg_off[v] + lo .. seg_off[v] + hi of feats     out_pse[b][t] = pse[prop_off[v] + t]
 * and rows t >= n are zero in both.  Every element of out (B, T, D) and out_pse (B, T, 2) is written exactly once (no clearing by the
 * caller); the running maximum starts from the first row of the run (features are signed) and is an exact order comparison of the stored
 * bits (-0 < +0); the store holds finite values only.  A vids[b] outside [0, Nv) (or a video of no rows) reads nothing and has its rows
 * written as zeros; lo / hi are clamped to the video's rows and n to T, so a bad table cannot read outside feats.
 * One workgroup owns one clip x one column block: it stages the video's rows of that block in LDS once (videos of at most
 * drn_pool_props_lds_rows() rows; longer ones are read through L2), its lanes own 16-byte column chunks.  Rows whose byte length
 * is not a multiple of 16 (or unaligned bases) take an element-wise path.  Host checks, DRN_ERR_ARG before anything is launched:
 * null pointers, negative counts, a vids_host entry outside [0, Nv), T < a counts_host entry, dtype; pse / out_pse 16-byte aligned. */
typedef struct DrnPoolProps {
  const void* feats;         /* (R, D) row-major, `dtype` */
  const int64_t* seg_off;    /* (Nv + 1) first row of each video */
  const int32_t* prop_off;   /* (Nv + 1) first proposal of each video in win / pse */
  const int32_t* win;        /* (Ptot, 2) [lo, hi], inclusive, local to the video */
  const double* pse;         /* (Ptot, 2) */
  const int32_t* vids;       /* (B) device */
  const int32_t* vids_host;  /* (B) host copy of vids, or NULL */
  const int32_t* counts_host;/* (B) host: proposals of each clip, or NULL */
  void* out;                 /* (B, T, D) `dtype` */
  double* out_pse;           /* (B, T, 2) */
  int32_t Nv, B, T, D, dtype;
  int32_t max_rows;          /* rows of the longest video when the caller knows them (sizes the LDS request), else 0 */
} DrnPoolProps;
int drn_pool_props(const DrnPoolProps* d /*host*/, void* stream);
/* rows of one video the LDS path of drn_pool_props holds for B clips of D elements (0: that geometry takes the element-wise path) */
int64_t drn_pool_props_lds_rows(int B, int D, int dtype);

/* MEASUREMENT infrastructure (bench.py; nothing on the product path calls it): what this chip sustains on bf16 MFMA with operands that
 * toggle like data.  MI355X clocks to its power budget: a register-only v_mfma_f32_32x32x16_bf16 loop at the issue floor (32 cycles per
 * MFMA and SIMD, 256 workgroups x 4 waves, no LDS or memory traffic) runs at ~2.3 GHz on zeros and ~1.7-1.8 GHz on random bf16 operands.
 * Launches on `stream`, waits for it, returns TFLOP/s, the effective clock (shader cycles / wall time) and cycles per MFMA.
 * ws: drn_diag_mfma_ws_bytes() bytes of device memory.  iters: 8 MFMAs per wave each (20000 ~ 3 ms). */
long drn_diag_mfma_ws_bytes(void);
int drn_diag_mfma_sustained(void* ws, int iters, int zero_operands, double* tflops, double* clock_ghz, double* cycles_per_mfma, void* stream);

#ifdef __cplusplus
}
#endif
#endif
