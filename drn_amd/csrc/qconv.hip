// conv0 of a search on a quantised index WITHOUT the gather (drn_amd.Grounder(conv0="mxfp8")): the block-scaled FP8 codes of the index
// are conv0's A operand as they lie -- the 32-column blocks run along conv0's K dimension -- and the sentence gate, which the gather
// kernel multiplies into the activations, multiplies conv0's weight instead:  (z * g) W = z (diag(g) W).
//   drn_gate_quantize_weights_mx8  once per search: the S gated copies of conv0's feature weights in the index's own format
//   drn_conv0_mx8                  per chunk: the implicit GEMM over three taps, reading index rows and gated weights from memory
// drn_amd/index.py has both definitions in plain torch (mx8_gate_weights, mx8_conv0_reference).
#include "mx8.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- gated weights
// quantize_rows_mx8_kernel (qindex.hip) on rows that are products: row (s, tap, n) of Dp columns, column c = gate[s][c] * w[tap][n][c]
// for c < D (ONE fp32 multiply) and zero for D <= c < Dp.  The same lane / block assignment and the same arithmetic (mx8.h).
__global__ __launch_bounds__(256) void gate_quantize_weights_mx8_kernel(const float* __restrict__ w, int ld_w, const float* __restrict__ gate,
                                                                        int ldg, int rows_per_s /* 3 * Cout */, int D, long total,
                                                                        int gpr /* Dp / 16 */, uint8_t* __restrict__ codes, int ld_codes,
                                                                        uint8_t* __restrict__ scales, int ld_scales) {
  for (long b = (long)blockIdx.x * 256; b < total; b += (long)gridDim.x * 256) {
    const long i = b + threadIdx.x;
    const bool active = i < total;
    const long row = active ? i / gpr : 0;
    const int g = active ? (int)(i - row * gpr) : 0;
    const int s = (int)(row / rows_per_s), wr = (int)(row - (long)s * rows_per_s);
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = g * 16 + k;
      const int cc = min(c, D - 1);
      const float prod = gate[(long)s * ldg + cc] * w[(long)wr * ld_w + cc];
      v[k] = (active && c < D) ? prod : 0.f;
    }
    u32x4 q;
    const int e = mx8_quantize16(v, q);
    if (!active) continue;
    *(u32x4*)(codes + row * ld_codes + g * 16) = q;
    if ((g & 1) == 0) scales[row * ld_scales + (g >> 1)] = (uint8_t)(e + 127);
  }
}

extern "C" int drn_gate_quantize_weights_mx8(const float* w, int ld_w, const float* gate, int ldg, int S, int Cout, int D, int Dp,
                                             uint8_t* wcodes, int ld_wcodes, uint8_t* wscales, int ld_wscales, void* stream) {
  drn_clear_status();
  DRN_CHECK_ARG(w && gate && wcodes && wscales, "drn_gate_quantize_weights_mx8: null pointer");
  DRN_CHECK_ARG(S > 0 && Cout > 0 && D > 0 && Dp >= D, "drn_gate_quantize_weights_mx8: bad args (S %d, Cout %d, D %d, Dp %d)", S, Cout, D, Dp);
  DRN_CHECK_ARG(Dp % MX8_BLOCK == 0, "drn_gate_quantize_weights_mx8: Dp = %d is not a multiple of the block of %d columns", Dp, MX8_BLOCK);
  DRN_CHECK_ARG(ld_w >= D && ldg >= D && ld_wcodes >= Dp && ld_wscales >= Dp / MX8_BLOCK,
                "drn_gate_quantize_weights_mx8: a row stride is shorter than its row");
  DRN_CHECK_ARG(ld_wcodes % 16 == 0 && (((uintptr_t)wcodes) & 15) == 0,
                "drn_gate_quantize_weights_mx8: wcodes and its row stride must be 16-byte multiples");
  DRN_CHECK_ARG((long)S * 3 * Cout <= 0x7fffffffL, "drn_gate_quantize_weights_mx8: more than 2^31 rows");
  const long total = (long)S * 3 * Cout * (Dp / 16);
  gate_quantize_weights_mx8_kernel<<<ew_blocks(total, 256, 8192), 256, 0, (hipStream_t)stream>>>(w, ld_w, gate, ldg, 3 * Cout, D, total, Dp / 16,
                                                                                             wcodes, ld_wcodes, wscales, ld_wscales);
  return drn_launch_status("drn_gate_quantize_weights_mx8");
}

// ---------------------------------------------------------------- conv0 on the codes: operands, checks
// The operands of every conv0 entry below, filled once per entry, checked by one function and unpacked by one launch function per
// kernel family.  drn_conv0_mx8 writes its raw output through out / ld_out and leaves ss, gate and gated null.  (The kernels keep their
// flat parameter lists and their own bodies.  Both ways of folding the two LDS-staged kernels were built with this struct as the kernel
// argument and measured: one template on all three tiles was 1 to 2 % slower at 256 x 256, two kernels made of shared device functions
// 1 to 3 % slower on every tile -- DESIGN.md section 3, profiles/search_mx8conv_onetemplate_bench.json.)
struct Conv0Mx8Args {
  const uint8_t *codes, *scales;                         // the index: rows of C codes, C / 32 scale bytes, P position values
  const bf16_t* pos;
  const int* prop_off;
  const uint8_t *wcodes, *wscales;                       // the gated weights [S][3][Cout][C], [..][C / 32], the position weights [3][Cout][P]
  const bf16_t* wpos;
  const int *pq, *pv, *vids;
  const float *ss, *gate;                                // the epilogue of the fused entries
  void *out, *gated;
  int ld_codes, ld_scales, ld_pos, n_rows, pad_row, Nv, S, Vc, ldg, ld_out, ld_gated, Q, L, C, P, Cout;
};
// (by the parameter names that the three entries share)
#define CONV0_MX8_ARGS(ss, gate, ldg, out, ld_out, gated, ld_gated)                                                                         \
  Conv0Mx8Args {                                                                                                                            \
    codes, scales, (const bf16_t*)pos, prop_off, wcodes, wscales, (const bf16_t*)wpos, pq, pv, vids, ss, gate, out, gated, ld_codes,        \
        ld_scales, ld_pos, n_rows, pad_row, Nv, S, Vc, ldg, ld_out, ld_gated, Q, L, C, P, Cout                                              \
  }

// The rows of the widest LDS tile: the fused kernels compute a tile's first row + its rows in int, so Q L stays that far below 2^31.
#define MXT_ROWS 256

// The argument checks of all three entries, the messages under the caller's name.  fused: the entries with the epilogue, whose
// kernels index a weight plane in 32 bits and walk tiles of up to MXT_ROWS rows.
static int conv0_mx8_check(const char* entry, const Conv0Mx8Args& a, const int32_t* pq_host, bool fused) {
  const int Q = a.Q, L = a.L, C = a.C, P = a.P, Cout = a.Cout;
  DRN_CHECK_ARG(a.codes && a.scales && a.prop_off && a.wcodes && a.wscales && a.pq && a.pv && a.vids && a.out && (P == 0 || (a.pos && a.wpos)),
                "%s: null pointer", entry);
  if (fused) DRN_CHECK_ARG((a.gate != nullptr) == (a.gated != nullptr), "%s: gate and gated must come together", entry);
  DRN_CHECK_ARG(a.n_rows > 0 && a.pad_row >= 0 && a.pad_row < a.n_rows && a.Nv > 0 && a.S > 0 && a.Vc > 0 && Q > 0 && L > 0 && C > 0 && P >= 0 &&
                    Cout > 0,
                "%s: bad args (n_rows %d, pad_row %d, Nv %d, S %d, Vc %d, Q %d, L %d, C %d, P %d, Cout %d)", entry, a.n_rows, a.pad_row, a.Nv,
                a.S, a.Vc, Q, L, C, P, Cout);
  DRN_CHECK_ARG(C % MX8_BLOCK == 0, "%s: C = %d is not a multiple of the block of %d columns", entry, C, MX8_BLOCK);
  DRN_CHECK_ARG(P % 32 == 0, "%s: P = %d is not a multiple of the 32 columns of a position step", entry, P);
  DRN_CHECK_ARG(Cout % 16 == 0, "%s: Cout = %d is not a multiple of 16", entry, Cout);
  if (fused) {
    DRN_CHECK_ARG((long)Cout * C <= 0x7fffffffL && 3L * Cout * P <= 0x7fffffffL, "%s: a weight plane of %d x %d is beyond 2^31", entry, Cout,
                  C + P);
    DRN_CHECK_ARG((long)Q * L <= 0x7fffffffL - MXT_ROWS &&
                      ((long)Q * L + MXT_ROWS - 1) / MXT_ROWS * cdiv(Cout, 256) <= 0x7fffffffL,
                  "%s: more than 2^31 rows", entry);
  } else {
    DRN_CHECK_ARG((long)Q * L <= 0x7fffffffL && (long)Q * cdiv(L, 16) * cdiv(Cout, 256) <= 0x7fffffffL, "%s: more than 2^31 rows", entry);
  }
  DRN_CHECK_ARG(a.ld_codes >= C && a.ld_scales >= C / MX8_BLOCK && (P == 0 || a.ld_pos >= P) && a.ld_out >= Cout &&
                    (!a.gated || (a.ld_gated >= Cout && a.ldg >= Cout)),
                "%s: a row stride is shorter than its row", entry);
  DRN_CHECK_ARG(a.ld_codes % 16 == 0 && (P == 0 || a.ld_pos % 8 == 0) &&
                    ((((uintptr_t)a.codes) | ((uintptr_t)a.wcodes) | ((uintptr_t)(P ? a.pos : nullptr)) | ((uintptr_t)(P ? a.wpos : nullptr))) & 15) == 0,
                "%s: codes / wcodes / pos / wpos and their row strides must be 16-byte multiples", entry);
  if (pq_host)
    for (int p = 0; p < Q; ++p)
      DRN_CHECK_ARG(pq_host[p] >= 0 && pq_host[p] < a.S, "%s: pair %d reads sentence %d of %d", entry, p, (int)pq_host[p], a.S);
  return DRN_OK;
}

// ---------------------------------------------------------------- conv0 on the codes
// One workgroup = 4 waves = 16 * MI output rows of ONE pair (an M tile never spans two pairs: they may belong to different sentences) x
// up to 256 output channels, wave w owning channels [64 w, 64 w + 64) as 4 fragments of 16.  No LDS: both operands of
// v_mfma_scale_f32_16x16x128_f8f6f4 come from memory directly, a lane's A fragment from one index row (row l & 15 of the fragment), its B
// fragment from one gated-weight row (channel l & 15); the four waves read the same index rows and meet in the vector cache.
// The operand map of the instruction, ESTABLISHED with one-hot probes on an MI355X and held by the exact-integer test
// (tests/test_search_mx8conv_gpu.py) -- it is NOT "32 contiguous K per lane": with g = l >> 4, registers 0-3 of a lane's fragment hold
// k = 16 g + 0..15 and registers 4-7 hold k = 64 + 16 g + 0..15 (two 16-byte loads 64 columns apart), while the lane's scale byte
// (byte 0 of the scale register, op_sel 0) applies to K block g, k in [32 g, 32 g + 32), of row / column l & 15 -- values that OTHER
// lanes hold (groups 2 (g & 1), 2 (g & 1) + 1, registers 0-3 for g < 2, registers 4-7 for g >= 2).
// K runs tap by tap over ceil(C / 128) steps -- a 16-byte half or a block past C is zero codes (with scale byte 127: byte 0 would be
// 2^-127, not zero, and 255 is NaN) -- then over P / 32 steps of
// v_mfma_f32_16x16x32_bf16 on the position columns into the same accumulators (C/D: column l & 15, row 4 (l >> 4) + i, whatever the
// operand format).  A tap row outside [0, L) is zero codes / zero position values.  No split-K, no atomics: an accumulator sums its K in
// one fixed order, whatever else the launch holds.
// Every address is a function of the tables and the work-item number, clamped as in gate_gather_packed_q8_kernel (pq into [0, S), the
// slot and the video to the pad row, src into [0, n_rows), the channel into [0, Cout), the columns into [0, C)): a masked fragment is
// loaded from its clamped address and then replaced by zeros, so no activation value and no mask moves an access.
template <int MI, typename OUT>
__global__ __launch_bounds__(256) void conv0_mx8_kernel(const uint8_t* __restrict__ codes, int ld_codes, const uint8_t* __restrict__ scales,
                                                        int ld_scales, const bf16_t* __restrict__ pos, int ld_pos, int n_rows, int pad_row,
                                                        const int* __restrict__ prop_off, int Nv, const uint8_t* __restrict__ wcodes,
                                                        const uint8_t* __restrict__ wscales, const bf16_t* __restrict__ wpos, int S,
                                                        const int* __restrict__ pq, const int* __restrict__ pv, const int* __restrict__ vids,
                                                        int Vc, OUT* __restrict__ raw, int ld_raw, int Q, int L, int C, int P, int Cout) {
  constexpr int NJ = 4;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mtiles = (L + 16 * MI - 1) / (16 * MI), ngroups = (Cout + 255) / 256;
  int b = blockIdx.x;
  const int ng = b % ngroups;
  b /= ngroups;
  const int mt = b % mtiles, p = b / mtiles;
  const int n0 = ng * 256 + wave * 64;
  if (p >= Q || n0 >= Cout) return;                     // (wave-uniform; the kernel has no barrier)
  const int q = min(max(pq[p], 0), S - 1), slot = pv[p];
  const int vd = (slot >= 0 && slot < Vc) ? vids[slot] : -1;
  int base = 0, cnt = 0;
  if (vd >= 0 && vd < Nv) {
    base = prop_off[vd];
    cnt = prop_off[vd + 1] - base;
  }
  const int r = lane & 15, kq = lane >> 4;
  const int t0 = mt * 16 * MI;
  const int cblocks = C / MX8_BLOCK;
  long ncol[NJ];                                         // this lane's weight row inside a (sentence, tap) plane, clamped
#pragma unroll
  for (int j = 0; j < NJ; ++j) ncol[j] = min(n0 + 16 * j + r, Cout - 1);
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tap = 0; tap < 3; ++tap) {
    long src[MI];
    bool live[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int u = t0 + 16 * i + r + tap - 1;
      live[i] = u >= 0 && u < L;
      src[i] = min(max(u >= 0 && u < cnt ? base + u : pad_row, 0), n_rows - 1);
    }
    const long plane = ((long)q * 3 + tap) * Cout;
    const uint8_t* wc = wcodes + plane * C;
    const uint8_t* ws = wscales + plane * cblocks;
    for (int k0 = 0; k0 < C; k0 += 128) {
      const int c_lo = k0 + 16 * kq, c_hi = c_lo + 64;   // this lane's two runs of 16 columns ...
      const int kb = k0 / MX8_BLOCK + kq;                // ... and the block of 32 columns its scale byte speaks for
      const bool lo_in = c_lo < C, hi_in = c_hi < C, kin = kb < cblocks;
      const int c_lo_c = min(c_lo, C - 16), c_hi_c = min(c_hi, C - 16), kbc = min(kb, cblocks - 1);
      const u32x4 zero = {0u, 0u, 0u, 0u};
      i32x8 a[MI], bw[NJ];
      int sa[MI], sb[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const uint8_t* ap = codes + src[i] * ld_codes;
        u32x4 lo = *(const u32x4*)(ap + c_lo_c), hi = *(const u32x4*)(ap + c_hi_c);
        const unsigned sc = scales[src[i] * ld_scales + kbc];
        lo = (lo_in && live[i]) ? lo : zero;
        hi = (hi_in && live[i]) ? hi : zero;
        a[i] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        sa[i] = (kin && live[i]) ? (int)sc : 127;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const uint8_t* bp = wc + ncol[j] * C;
        u32x4 lo = *(const u32x4*)(bp + c_lo_c), hi = *(const u32x4*)(bp + c_hi_c);
        const unsigned sc = ws[ncol[j] * cblocks + kbc];
        lo = lo_in ? lo : zero;
        hi = hi_in ? hi : zero;
        bw[j] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        sb[j] = kin ? (int)sc : 127;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (n0 + 16 * j >= Cout) break;                  // (wave-uniform)
#pragma unroll
        for (int i = 0; i < MI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], bw[j], acc[i][j], 0 /* cbsz: A is e4m3 */, 0 /* blgp: B is e4m3 */,
                                                                       0, sa[i], 0, sb[j]);
      }
    }
    for (int j0 = 0; j0 < P; j0 += 32) {
      bf16x8 a[MI], bw[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const bf16x8 v = *(const bf16x8*)(pos + src[i] * ld_pos + j0 + 8 * kq);
        a[i] = live[i] ? v : bf16x8{};
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) bw[j] = *(const bf16x8*)(wpos + ((long)tap * Cout + ncol[j]) * P + j0 + 8 * kq);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (n0 + 16 * j >= Cout) break;
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bw[j], acc[i][j], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = n0 + 16 * j + r;
      if (n >= Cout) continue;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int t = t0 + 16 * i + 4 * kq + x;
        if (t < L) raw[((long)p * L + t) * ld_raw + n] = (OUT)acc[i][j][x];
      }
    }
}

// The argument list that all three kernels begin with, from the operand struct.
#define CONV0_MX8_OPERANDS                                                                                                                    \
  a.codes, a.ld_codes, a.scales, a.ld_scales, a.pos, a.ld_pos, a.n_rows, a.pad_row, a.prop_off, a.Nv, a.wcodes, a.wscales, a.wpos, a.S, a.pq, \
      a.pv, a.vids, a.Vc
template <typename OUT>
static void launch_conv0_mx8(const Conv0Mx8Args& a, hipStream_t st) {
  const long per_mtile = (long)a.Q * cdiv(a.Cout, 256);
#define CONV0_MX8_LAUNCH(MI)                                                                                                             \
  conv0_mx8_kernel<MI, OUT><<<(unsigned)(per_mtile * cdiv(a.L, 16 * MI)), 256, 0, st>>>(CONV0_MX8_OPERANDS, (OUT*)a.out, a.ld_out, a.Q, a.L, \
                                                                                         a.C, a.P, a.Cout)
  // rows of one pair per workgroup: as many as the sequence fills, up to 64
  if (a.L <= 16) CONV0_MX8_LAUNCH(1);
  else if (a.L <= 32) CONV0_MX8_LAUNCH(2);
  else CONV0_MX8_LAUNCH(4);
#undef CONV0_MX8_LAUNCH
}

extern "C" int drn_conv0_mx8(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos, int n_rows,
                             int pad_row, const int32_t* prop_off, int Nv, const uint8_t* wcodes, const uint8_t* wscales, const void* wpos,
                             int S, const int32_t* pq, const int32_t* pq_host, const int32_t* pv, const int32_t* vids, int Vc, void* raw,
                             int ld_raw, int out_f32, int Q, int L, int C, int P, int Cout, void* stream) {
  drn_clear_status();
  const Conv0Mx8Args a = CONV0_MX8_ARGS(nullptr, nullptr, 0, raw, ld_raw, nullptr, 0);
  if (const int rc = conv0_mx8_check("drn_conv0_mx8", a, pq_host, false)) return rc;
  if (out_f32) launch_conv0_mx8<float>(a, (hipStream_t)stream);
  else launch_conv0_mx8<bf16_t>(a, (hipStream_t)stream);
  return drn_launch_status("drn_conv0_mx8");
}

// ---------------------------------------------------------------- conv0 on the codes, LDS-staged, with BatchNorm / ReLU / gate in the epilogue
// drn_conv0_mx8_bn (Grounder(conv0="mxfp8", fused=True)).  One workgroup = 8 waves = MXT_ROWS = 256 rows of the FLATTENED (pair, t) output
// x up to 256 output channels; wave w owns rows [64 (w & 3), +64) x channels [128 (w >> 2), +128) as 4 x 8 fragments of 16 x 16.  At small
// L a tile spans several pairs (8 at L = 32); a pair longer than the tile spans several tiles.  The grid, cdiv(Q L, 256) x cdiv(Cout, 256),
// and the tile -> pair map are functions of (Q, L, Cout) alone.
// K runs tap-outer: step s = (tap, k0) stages a 256 x 128-byte tile of index codes (row i = the source row of output row i at this tap,
// zeros where the tap falls outside [0, L)) and a 256 x 128-byte tile of the sentence's gated weights, with one dword of four scale bytes
// per row, into one of TWO LDS stages (2 x (32 + 32 + 1 + 1) KB = 132 KB, + the 4 KB row table + the 1 KB sentence list = 140,288 bytes:
// ONE workgroup per CU, two waves per SIMD).  The global
// loads of step s + 1 are issued into registers before the MFMAs of step s and written to the other stage after them: one barrier per
// step.  The operand map of the instruction (above) makes a staged tile a plain row copy.  128-byte rows would put rows r and r + 2 on
// the same banks for ds_read_b128, so the 16-byte slot c of row r lies at slot c ^ ((r >> 1) & 7): each of the instruction's four lane
// groups (microarchitecture: {0-3, 12-15, 20-27}, ...) then covers all 64 banks once, and the 8 lanes that write one row still cover
// 128 contiguous bytes.
// Sentences: all rows of one MFMA share B, so the tile makes one pass of the whole K loop per DISTINCT sentence among its pairs (in the
// order of first appearance; wave-uniform, found from pq in LDS), staging only that sentence's weights; rows of other sentences are
// staged as zero codes with scale byte 127 and add +0 to their accumulators.
// An accumulator therefore sums its own sentence's K in one fixed order -- taps 0..2 x the 128-column steps, then taps 0..2 x the
// 32-column position steps on v_mfma_f32_16x16x32_bf16 (fragments from memory, as conv0_mx8_kernel) -- whatever else the tile or the
// launch holds, and whatever the order of the pairs.  (A NaN weight code, or a weight scale byte 255 -- the e8m0 NaN --, of ANOTHER
// sentence in the same tile is the one exception: 0 x NaN; the quantiser writes neither, its scale bytes end at 254.)  No split-K, no atomics.
// Addresses: clamped exactly as in conv0_mx8_kernel; a masked row is loaded from its clamped address and then zeroed.
// Epilogue, from the fp32 accumulator: v = relu(fmaf(acc, scale, shift)) with (scale, shift) = ss[n], ss[Cout + n]
// (bn_eval_scale_shift's table; ss NULL: v = acc), out = OUT(v), gated = OUT(v * gate[pair][n]) from the UNROUNDED v, as bn_apply_kernel.
#define MXT_TILE (MXT_ROWS * 128)
// The order of the K loop's memory operations IS its schedule (loads of the next step, then per channel fragment two LDS reads and four
// MFMAs, then the LDS writes of the next step); left alone, the compiler reads all eight B fragments first (64 registers more, which
// spill) and writes the next stage before the MFMAs (which waits for the loads just issued).  Nothing moves across this.
#define MXT_FENCE()                        \
  do {                                     \
    asm volatile("" ::: "memory");         \
    __builtin_amdgcn_sched_barrier(0);     \
  } while (0)

template <typename OUT>
__global__ __launch_bounds__(512) void conv0_mx8_tiled_kernel(const uint8_t* __restrict__ codes, int ld_codes, const uint8_t* __restrict__ scales,
                                                              int ld_scales, const bf16_t* __restrict__ pos, int ld_pos, int n_rows, int pad_row,
                                                              const int* __restrict__ prop_off, int Nv, const uint8_t* __restrict__ wcodes,
                                                              const uint8_t* __restrict__ wscales, const bf16_t* __restrict__ wpos, int S,
                                                              const int* __restrict__ pq, const int* __restrict__ pv, const int* __restrict__ vids,
                                                              int Vc, const float* __restrict__ ss, const float* __restrict__ gate, int ldg,
                                                              OUT* __restrict__ out, int ld_out, OUT* __restrict__ gated, int ld_gated, int Q, int L,
                                                              int C, int P, int Cout) {
  __shared__ __attribute__((aligned(16))) uint8_t tA[2][MXT_TILE];
  __shared__ __attribute__((aligned(16))) uint8_t tB[2][MXT_TILE];
  __shared__ unsigned sA[2][MXT_ROWS], sB[2][MXT_ROWS];
  __shared__ int qs[MXT_ROWS];                           // the (clamped) sentences of the tile's pairs; -1 once their pass is done
  __shared__ i32x4 rinfo[MXT_ROWS];                      // per tile row: t, its video's first row and row count, its sentence (-1: past M)
  constexpr int MI = 4, NJ = 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ngroups = (Cout + 255) / 256;
  const int ng = blockIdx.x % ngroups;
  const int M = Q * L, m0 = (int)(blockIdx.x / ngroups) * MXT_ROWS;            // (the entry refuses Q L + 256 > 2^31 - 1)
  const int p0 = m0 / L, p1 = min((m0 + MXT_ROWS - 1) / L, Q - 1), npairs = p1 - p0 + 1;   // (<= 256: L >= 1)
  const int cblocks = C / MX8_BLOCK, ksteps = (C + 127) / 128, nsteps = 3 * ksteps;
  const int r = lane & 15, kq = lane >> 4;

  if (tid < MXT_ROWS) {
    const int m = m0 + tid, p = min(m / L, Q - 1);
    const int slot = pv[p];
    const int vd = (slot >= 0 && slot < Vc) ? vids[slot] : -1;
    int base = 0, cnt = 0;
    if (vd >= 0 && vd < Nv) {
      base = prop_off[vd];
      cnt = prop_off[vd + 1] - base;
    }
    rinfo[tid] = i32x4{m - p * L, base, cnt, m < M ? min(max(pq[p], 0), S - 1) : -1};
  }
  for (int i = tid; i < npairs; i += 512) qs[i] = min(max(pq[p0 + i], 0), S - 1);
  __syncthreads();
  // the source row of tile row R at offset u of its video, clamped; whether it is a row of sentence q with tap u inside [0, L)
  auto src_of = [&](const i32x4 R, int u) { return (long)min(max(u >= 0 && u < R[2] ? R[1] + u : pad_row, 0), n_rows - 1); };
  auto live_of = [&](const i32x4 R, int u, int q) { return R[3] == q && u >= 0 && u < L; };

  // staging: thread -> the 16-byte slot (tid & 7) of rows (tid >> 3) + 64 k, k < 4, of both tiles; one scale dword of row tid & 255 of
  // A (waves 0-3) or of B (waves 4-7)
  const int srow0 = tid >> 3, sslot = tid & 7;
  const int dst0 = srow0 * 128 + ((sslot ^ ((srow0 >> 1) & 7)) << 4);          // ((row >> 1) & 7 is the same for rows 64 apart)
  const bool scaleA = wave < 4;                          // (wave-uniform)
  const int scrow = tid & 255;
  // this wave's fragments
  const int wr = (wave & 3) * 64, n0 = ng * 256 + (wave >> 2) * 128;

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int pi = 0; pi < npairs; ++pi) {
    const int q = qs[pi];                                // (one address for the whole workgroup)
    if (q < 0) continue;                                 // (uniform: a sentence that had its pass)
    // fetch: the global loads of a step into registers, nothing consuming them (no wait); stage: mask them and write them to LDS
    u32x4 ra[4], rb[4];
    unsigned rsb[4], keep;                               // keep: bit k = A row k is live, bit 4 = the scale row is live
    auto fetch = [&](int step) {
      const int tap = step / ksteps, k0 = (step - tap * ksteps) * 128;
      const unsigned colc = (unsigned)min(k0 + 16 * sslot, C - 16);
      const uint8_t* wc = wcodes + ((long)q * 3 + tap) * Cout * C;             // (uniform)
      keep = 0;
      int srow = srow0, scr = scrow;                     // (opaque: offsets made of them are computed here, not kept -- and spilled -- across
      asm volatile("" : "+v"(srow), "+v"(scr));          //  the whole K loop)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const i32x4 R = rinfo[srow + 64 * k];
        const int u = R[0] + tap - 1;
        ra[k] = *(const u32x4*)(codes + src_of(R, u) * ld_codes + colc);
        keep |= (live_of(R, u, q) ? 1u : 0u) << k;
        rb[k] = *(const u32x4*)(wc + ((unsigned)min(ng * 256 + srow + 64 * k, Cout - 1) * (unsigned)C + colc));
      }
      const uint8_t* sp;
      if (scaleA) {
        const i32x4 R = rinfo[scr];
        const int u = R[0] + tap - 1;
        keep |= (live_of(R, u, q) ? 1u : 0u) << 4;
        sp = scales + src_of(R, u) * ld_scales;
      } else {
        keep |= 1u << 4;
        sp = wscales + (((long)q * 3 + tap) * Cout + min(ng * 256 + scr, Cout - 1)) * cblocks;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) rsb[g] = sp[min(k0 / MX8_BLOCK + g, cblocks - 1)];
    };
    auto stage = [&](int step, int buf) {
      const int k0 = (step % ksteps) * 128;
      const bool col_in = k0 + 16 * sslot < C;
      const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        *(u32x4*)(&tA[buf][dst0 + 64 * 128 * k]) = (col_in && ((keep >> k) & 1)) ? ra[k] : zero;
        *(u32x4*)(&tB[buf][dst0 + 64 * 128 * k]) = col_in ? rb[k] : zero;
      }
      unsigned rs = 0;
#pragma unroll
      for (int g = 0; g < 4; ++g) rs |= ((((keep >> 4) & 1) && k0 / MX8_BLOCK + g < cblocks) ? rsb[g] : 127u) << (8 * g);
      (scaleA ? sA[buf] : sB[buf])[scrow] = rs;
    };

    fetch(0);
    stage(0, 0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
      const int buf = step & 1;
      if (step + 1 < nsteps) fetch(step + 1);
      MXT_FENCE();
      i32x8 a[MI];
      int sa[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wr + 16 * i + r, sw = (row >> 1) & 7;
        const u32x4 lo = *(const u32x4*)(&tA[buf][row * 128 + ((kq ^ sw) << 4)]);
        const u32x4 hi = *(const u32x4*)(&tA[buf][row * 128 + (((kq + 4) ^ sw) << 4)]);
        a[i] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        sa[i] = (int)((sA[buf][row] >> (8 * kq)) & 0xffu);
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {                     // (fragments past Cout read clamped rows and are not stored)
        const int row = (wave >> 2) * 128 + 16 * j + r, sw = (row >> 1) & 7;
        const u32x4 lo = *(const u32x4*)(&tB[buf][row * 128 + ((kq ^ sw) << 4)]);
        const u32x4 hi = *(const u32x4*)(&tB[buf][row * 128 + (((kq + 4) ^ sw) << 4)]);
        const i32x8 bw = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        const int sb = (int)((sB[buf][row] >> (8 * kq)) & 0xffu);
#pragma unroll
        for (int i = 0; i < MI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], bw, acc[i][j], 0 /* cbsz: A is e4m3 */, 0 /* blgp: B is e4m3 */, 0,
                                                                       sa[i], 0, sb);
        asm volatile("" : "+v"(acc[0][j]), "+v"(acc[1][j]), "+v"(acc[2][j]), "+v"(acc[3][j])::"memory");
        __builtin_amdgcn_sched_barrier(0);
      }
      if (step + 1 < nsteps) stage(step + 1, buf ^ 1);
      __syncthreads();
    }
    // the position columns, fragments from memory
    if (n0 < Cout) {
      int rr = r, kk = kq;                               // (opaque, as in fetch)
      asm volatile("" : "+v"(rr), "+v"(kk));
      for (int tap = 0; tap < 3; ++tap) {
        long src[MI];
        bool live[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const i32x4 R = rinfo[wr + 16 * i + rr];
          const int u = R[0] + tap - 1;
          src[i] = src_of(R, u);
          live[i] = live_of(R, u, q);
        }
        for (int j0 = 0; j0 < P; j0 += 32) {
          bf16x8 a[MI];
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            const bf16x8 v = *(const bf16x8*)(pos + src[i] * ld_pos + j0 + 8 * kk);
            a[i] = live[i] ? v : bf16x8{};
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const bf16x8 bw = *(const bf16x8*)(wpos + (unsigned)((tap * Cout + min(n0 + 16 * j + rr, Cout - 1)) * P + j0 + 8 * kk));
#pragma unroll
            for (int i = 0; i < MI; ++i)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bw, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    // this sentence is done: strike it from the list (every wave has read qs[pi]: the K loop's barriers lie in between)
    for (int i = tid; i < npairs; i += 512)
      if (qs[i] == q) qs[i] = -1;
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int m = m0 + wr + 16 * i + 4 * kq + x;
      if (m >= M) continue;
      const float* gp = gated ? gate + (long)(m / L) * ldg : nullptr;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + 16 * j + r;
        if (n >= Cout) continue;
        float v = acc[i][j][x];
        if (ss) v = fmaxf(fmaf(v, ss[n], ss[Cout + n]), 0.f);
        out[(long)m * ld_out + n] = (OUT)v;
        if (gated) gated[(long)m * ld_gated + n] = (OUT)(v * gp[n]);
      }
    }
}

// ---------------------------------------------------------------- the same launch on narrow tiles, for grids that do not fill the chip
// drn_conv0_mx8_bn_tile.  conv0_mx8_tiled_kernel's one tile shape puts cdiv(Q L, 256) x cdiv(Cout, 256) workgroups on the chip, each
// walking its 3 (C / 128) K steps alone: 64 pairs x T = 32 are 8 workgroups on 256 CUs.  conv0_mx8_narrow_kernel<OUT, ROWS, COLS> is the
// same computation on ROWS x COLS tiles (128 x 64, 64 x 64), 4 waves: wave w owns rows [16 MI (w % WR), +16 MI) x channels
// [16 NJ (w / WR), +16 NJ) of the tile.  Everything that defines a value is the wide kernel's: the flattened (pair, t) rows and the row
// table, the clamped addresses and the zeroing at the LDS write, the swizzle and the operand map, one pass per distinct sentence in the
// order of first appearance, the tap-outer steps, the position columns after them, the epilogue from the unrounded fp32 value.  An
// accumulator depends on its own row of A, its own column of B and the order of its K steps alone, and the passes of other sentences
// add +0: each output element is bit for bit the wide kernel's (tests/test_search_mx8tiles_gpu.py).  No split-K, no atomics.
// LDS: two stages of (ROWS + COLS) x (128 + 4) bytes + the row table and the sentence list: 52.0 KB at 128 x 64 (two workgroups per
// CU: <= 256 registers), 34.3 KB at 64 x 64 (three per CU: <= 168 registers; the launch bound asks for that occupancy by ROWS).  The
// grids a narrow tile is chosen for hold at most three 64 x 64 workgroups per CU, all resident at once, or at most four 128 x 64
// workgroups per CU in two resident rounds (conv0_mx8_choose); registers beyond that go to a second set of prefetched loads.
#define MXN_THREADS 256
template <typename OUT, int ROWS, int COLS>
__global__ __launch_bounds__(MXN_THREADS, ROWS == 64 ? 3 : 2) void conv0_mx8_narrow_kernel(
    const uint8_t* __restrict__ codes, int ld_codes, const uint8_t* __restrict__ scales, int ld_scales, const bf16_t* __restrict__ pos,
    int ld_pos, int n_rows, int pad_row, const int* __restrict__ prop_off, int Nv, const uint8_t* __restrict__ wcodes,
    const uint8_t* __restrict__ wscales, const bf16_t* __restrict__ wpos, int S, const int* __restrict__ pq, const int* __restrict__ pv,
    const int* __restrict__ vids, int Vc, const float* __restrict__ ss, const float* __restrict__ gate, int ldg, OUT* __restrict__ out,
    int ld_out, OUT* __restrict__ gated, int ld_gated, int Q, int L, int C, int P, int Cout) {
  static_assert(ROWS % 64 == 0 && COLS % 64 == 0 && ROWS + COLS <= MXN_THREADS, "one scale row per thread, whole waves on either side");
  constexpr int WR = 2, WC = 2, MI = ROWS / WR / 16, NJ = COLS / WC / 16, KA = ROWS / 32, KB = COLS / 32;
  __shared__ __attribute__((aligned(16))) uint8_t tA[2][ROWS * 128];
  __shared__ __attribute__((aligned(16))) uint8_t tB[2][COLS * 128];
  __shared__ unsigned sA[2][ROWS], sB[2][COLS];
  __shared__ int qs[ROWS];                               // the (clamped) sentences of the tile's pairs; -1 once their pass is done
  __shared__ i32x4 rinfo[ROWS];                          // per tile row: t, its video's first row and row count, its sentence (-1: past M)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ngroups = (Cout + COLS - 1) / COLS;
  const int ng = blockIdx.x % ngroups;
  const int M = Q * L, m0 = (int)(blockIdx.x / ngroups) * ROWS;                // (the entry refuses Q L + 256 > 2^31 - 1)
  const int p0 = m0 / L, p1 = min((m0 + ROWS - 1) / L, Q - 1), npairs = p1 - p0 + 1;       // (<= ROWS: L >= 1)
  const int cblocks = C / MX8_BLOCK, ksteps = (C + 127) / 128, nsteps = 3 * ksteps;
  const int r = lane & 15, kq = lane >> 4;

  if (tid < ROWS) {
    const int m = m0 + tid, p = min(m / L, Q - 1);
    const int slot = pv[p];
    const int vd = (slot >= 0 && slot < Vc) ? vids[slot] : -1;
    int base = 0, cnt = 0;
    if (vd >= 0 && vd < Nv) {
      base = prop_off[vd];
      cnt = prop_off[vd + 1] - base;
    }
    rinfo[tid] = i32x4{m - p * L, base, cnt, m < M ? min(max(pq[p], 0), S - 1) : -1};
  }
  for (int i = tid; i < npairs; i += MXN_THREADS) qs[i] = min(max(pq[p0 + i], 0), S - 1);
  __syncthreads();
  auto src_of = [&](const i32x4 R, int u) { return (long)min(max(u >= 0 && u < R[2] ? R[1] + u : pad_row, 0), n_rows - 1); };
  auto live_of = [&](const i32x4 R, int u, int q) { return R[3] == q && u >= 0 && u < L; };

  // staging: thread -> the 16-byte slot (tid & 7) of rows (tid >> 3) + 32 k of A (k < KA) and of B (k < KB); one scale dword of row tid
  // of A (tid < ROWS) or of row tid - ROWS of B (the next COLS threads): whole waves either way
  const int srow0 = tid >> 3, sslot = tid & 7;
  const int dst0 = srow0 * 128 + ((sslot ^ ((srow0 >> 1) & 7)) << 4);          // ((row >> 1) & 7 is the same for rows 32 apart)
  const bool scaleA = tid < ROWS, scaleB = !scaleA && tid < ROWS + COLS;       // (wave-uniform)
  const int scrow = scaleA ? tid : min(tid - ROWS, COLS - 1);
  const int wr = (wave % WR) * 16 * MI, wc = (wave / WR) * 16 * NJ, n0 = ng * COLS + wc;

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int pi = 0; pi < npairs; ++pi) {
    const int q = qs[pi];
    if (q < 0) continue;                                 // (uniform: a sentence that had its pass)
    // fetch: the global loads of a step into one of TWO register sets, nothing consuming them (no wait); stage: mask them and write
    // them to LDS.  The loads of step s + 2 are issued before the MFMAs of step s, and step s + 1 -- loaded a whole step earlier -- is
    // written to the other LDS stage after them: a narrow tile has few MFMAs per step to hide a load behind, and the registers to spare.
    struct Regs {
      u32x4 ra[KA], rb[KB];
      unsigned rsb[4], keep;                             // keep: bit k = A row k is live, bit 8 = the scale row is live
    } set0, set1;
    auto fetch = [&](int step, Regs& R_) {
      u32x4(&ra)[KA] = R_.ra;
      u32x4(&rb)[KB] = R_.rb;
      unsigned(&rsb)[4] = R_.rsb;
      unsigned& keep = R_.keep;
      const int tap = step / ksteps, k0 = (step - tap * ksteps) * 128;
      const unsigned colc = (unsigned)min(k0 + 16 * sslot, C - 16);
      const uint8_t* wcp = wcodes + ((long)q * 3 + tap) * Cout * C;            // (uniform)
      keep = 0;
      int srow = srow0, scr = scrow;                     // (opaque, as in the wide kernel: offsets made of them are computed here, not kept
      asm volatile("" : "+v"(srow), "+v"(scr));          //  across the whole K loop)
#pragma unroll
      for (int k = 0; k < KA; ++k) {
        const i32x4 R = rinfo[srow + 32 * k];
        const int u = R[0] + tap - 1;
        ra[k] = *(const u32x4*)(codes + src_of(R, u) * ld_codes + colc);
        keep |= (live_of(R, u, q) ? 1u : 0u) << k;
      }
#pragma unroll
      for (int k = 0; k < KB; ++k)
        rb[k] = *(const u32x4*)(wcp + ((unsigned)min(ng * COLS + srow + 32 * k, Cout - 1) * (unsigned)C + colc));
      {                                                  // (every thread, idle ones too: the number of loads in flight is one
        const i32x4 R = rinfo[scaleA ? scr : 0];         //  number, so the wait before the LDS writes can leave the newer loads out)
        const int u = R[0] + tap - 1;
        keep |= ((!scaleA || live_of(R, u, q)) ? 1u : 0u) << 8;
        const uint8_t* sp = scaleA ? scales + src_of(R, u) * ld_scales
                                   : wscales + (((long)q * 3 + tap) * Cout + min(ng * COLS + scr, Cout - 1)) * cblocks;
#pragma unroll
        for (int g = 0; g < 4; ++g) rsb[g] = sp[min(k0 / MX8_BLOCK + g, cblocks - 1)];
      }
    };
    auto stage = [&](int step, int buf, const Regs& R_) {
      const u32x4(&ra)[KA] = R_.ra;
      const u32x4(&rb)[KB] = R_.rb;
      const unsigned(&rsb)[4] = R_.rsb;
      const unsigned keep = R_.keep;
      const int k0 = (step % ksteps) * 128;
      const bool col_in = k0 + 16 * sslot < C;
      const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < KA; ++k) *(u32x4*)(&tA[buf][dst0 + 32 * 128 * k]) = (col_in && ((keep >> k) & 1)) ? ra[k] : zero;
#pragma unroll
      for (int k = 0; k < KB; ++k) *(u32x4*)(&tB[buf][dst0 + 32 * 128 * k]) = col_in ? rb[k] : zero;
      if (scaleA || scaleB) {
        unsigned rs = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) rs |= ((((keep >> 8) & 1) && k0 / MX8_BLOCK + g < cblocks) ? rsb[g] : 127u) << (8 * g);
        (scaleA ? sA[buf] : sB[buf])[scrow] = rs;
      }
    };

    // one K step: F takes the loads of step + 2, G holds those of step + 1
    auto kstep = [&](int step, Regs& F, const Regs& G) {
      const int buf = step & 1;
      if (step + 2 < nsteps) fetch(step + 2, F);
      MXT_FENCE();
      i32x8 a[MI];
      int sa[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wr + 16 * i + r, sw = (row >> 1) & 7;
        const u32x4 lo = *(const u32x4*)(&tA[buf][row * 128 + ((kq ^ sw) << 4)]);
        const u32x4 hi = *(const u32x4*)(&tA[buf][row * 128 + (((kq + 4) ^ sw) << 4)]);
        a[i] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        sa[i] = (int)((sA[buf][row] >> (8 * kq)) & 0xffu);
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {                     // (fragments past Cout read clamped rows and are not stored)
        const int row = wc + 16 * j + r, sw = (row >> 1) & 7;
        const u32x4 lo = *(const u32x4*)(&tB[buf][row * 128 + ((kq ^ sw) << 4)]);
        const u32x4 hi = *(const u32x4*)(&tB[buf][row * 128 + (((kq + 4) ^ sw) << 4)]);
        const i32x8 bw = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        const int sb = (int)((sB[buf][row] >> (8 * kq)) & 0xffu);
#pragma unroll
        for (int i = 0; i < MI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], bw, acc[i][j], 0 /* cbsz: A is e4m3 */, 0 /* blgp: B is e4m3 */, 0,
                                                                       sa[i], 0, sb);
#pragma unroll
        for (int i = 0; i < MI; ++i) asm volatile("" : "+v"(acc[i][j])::"memory");          // (the MFMAs stay before the LDS writes)
        __builtin_amdgcn_sched_barrier(0);
      }
      if (step + 1 < nsteps) stage(step + 1, buf ^ 1, G);
      __syncthreads();
    };
    fetch(0, set0);
    stage(0, 0, set0);
    fetch(1, set1);                                      // (nsteps >= 3)
    __syncthreads();
    for (int step = 0; step < nsteps; step += 2) {
      kstep(step, set0, set1);
      if (step + 1 < nsteps) kstep(step + 1, set1, set0);
    }
    // the position columns, fragments from memory
    if (n0 < Cout) {
      int rr = r, kk = kq;                               // (opaque, as in fetch)
      asm volatile("" : "+v"(rr), "+v"(kk));
      for (int tap = 0; tap < 3; ++tap) {
        long src[MI];
        bool live[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const i32x4 R = rinfo[wr + 16 * i + rr];
          const int u = R[0] + tap - 1;
          src[i] = src_of(R, u);
          live[i] = live_of(R, u, q);
        }
        for (int j0 = 0; j0 < P; j0 += 32) {
          bf16x8 a[MI];
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            const bf16x8 v = *(const bf16x8*)(pos + src[i] * ld_pos + j0 + 8 * kk);
            a[i] = live[i] ? v : bf16x8{};
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const bf16x8 bw = *(const bf16x8*)(wpos + (unsigned)((tap * Cout + min(n0 + 16 * j + rr, Cout - 1)) * P + j0 + 8 * kk));
#pragma unroll
            for (int i = 0; i < MI; ++i)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bw, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    // this sentence is done: strike it from the list (every wave has read qs[pi]: the K loop's barriers lie in between)
    for (int i = tid; i < npairs; i += MXN_THREADS)
      if (qs[i] == q) qs[i] = -1;
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int m = m0 + wr + 16 * i + 4 * kq + x;
      if (m >= M) continue;
      const float* gp = gated ? gate + (long)(m / L) * ldg : nullptr;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + 16 * j + r;
        if (n >= Cout) continue;
        float v = acc[i][j][x];
        if (ss) v = fmaxf(fmaf(v, ss[n], ss[Cout + n]), 0.f);
        out[(long)m * ld_out + n] = (OUT)v;
        if (gated) gated[(long)m * ld_gated + n] = (OUT)(v * gp[n]);
      }
    }
}

// A shipped tile's launch: its kernel, its thread count, its grid.
template <typename OUT, int ROWS, int COLS>
static void launch_conv0_mx8_tile(const Conv0Mx8Args& a, hipStream_t st) {
  const unsigned grid = (unsigned)(((long)a.Q * a.L + ROWS - 1) / ROWS * cdiv(a.Cout, COLS));
#define CONV0_MX8_BN_OPERANDS \
  CONV0_MX8_OPERANDS, a.ss, a.gate, a.ldg, (OUT*)a.out, a.ld_out, (OUT*)a.gated, a.ld_gated, a.Q, a.L, a.C, a.P, a.Cout
  if constexpr (ROWS == MXT_ROWS) conv0_mx8_tiled_kernel<OUT><<<grid, 512, 0, st>>>(CONV0_MX8_BN_OPERANDS);
  else conv0_mx8_narrow_kernel<OUT, ROWS, COLS><<<grid, MXN_THREADS, 0, st>>>(CONV0_MX8_BN_OPERANDS);
#undef CONV0_MX8_BN_OPERANDS
}


// Check, then launch a shipped tile (by its rows: 256 x 256, 128 x 64, 64 x 64), under the name of the entry that the caller is or
// stands for.
static int conv0_mx8_bn_run(const char* entry, const Conv0Mx8Args& a, const int32_t* pq_host, int out_f32, int tile_rows, void* stream) {
  drn_clear_status();
  if (const int rc = conv0_mx8_check(entry, a, pq_host, true)) return rc;
  hipStream_t st = (hipStream_t)stream;
  switch (2 * tile_rows + (out_f32 ? 1 : 0)) {
    case 2 * 256 + 1: launch_conv0_mx8_tile<float, 256, 256>(a, st); break;
    case 2 * 256: launch_conv0_mx8_tile<bf16_t, 256, 256>(a, st); break;
    case 2 * 128 + 1: launch_conv0_mx8_tile<float, 128, 64>(a, st); break;
    case 2 * 128: launch_conv0_mx8_tile<bf16_t, 128, 64>(a, st); break;
    case 2 * 64 + 1: launch_conv0_mx8_tile<float, 64, 64>(a, st); break;
    case 2 * 64: launch_conv0_mx8_tile<bf16_t, 64, 64>(a, st); break;
    default: DRN_CHECK_ARG(false, "%s: no tile of %d rows", entry, tile_rows);
  }
  return drn_launch_status(entry);
}

extern "C" int drn_conv0_mx8_bn(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos, int n_rows,
                                int pad_row, const int32_t* prop_off, int Nv, const uint8_t* wcodes, const uint8_t* wscales, const void* wpos,
                                int S, const int32_t* pq, const int32_t* pq_host, const int32_t* pv, const int32_t* vids, int Vc, const float* ss,
                                const float* gate, int ldg, void* out, int ld_out, void* gated, int ld_gated, int out_f32, int Q, int L, int C,
                                int P, int Cout, void* stream) {
  return conv0_mx8_bn_run("drn_conv0_mx8_bn", CONV0_MX8_ARGS(ss, gate, ldg, out, ld_out, gated, ld_gated), pq_host, out_f32, 256, stream);
}

// The tile "choose" picks: a function of (Q L, Cout) and the device's CU count alone -- never of pq / pv / vids, so a captured launch
// replays with other pairs.  W = the wide tile's workgroups, cdiv(Q L, 256) x cdiv(Cout, 256); a wide tile is 16 64 x 64 tiles or 8
// 128 x 64 tiles at Cout = 256:
//   16 W <= MXN_SMALL_UPTO_16THS x CUs                   ->  64 x 64  (3/16: its workgroups are resident at once, three per CU)
//   else 16 W <= MXN_MID_UPTO_16THS x CUs                -> 128 x 64  (8/16: at most two resident rounds of two workgroups per CU)
//   else                                                 -> 256 x 256 (the wide kernel: a third round of 128 x 64 costs more than it)
// (the crossovers as measured: DESIGN.md section 3, profiles/search_mx8conv_tiles_bench.json).  No device: wide.
#define MXN_SMALL_UPTO_16THS 3
#define MXN_MID_UPTO_16THS 8
static int conv0_mx8_cus() {                             // (as nt_resident_capacity, gemm_nt_bn.hip)
  int dev = 0;                                           // A query that fails (a box without a device) answers 0 and takes its OWN error
  if (hipGetDevice(&dev) != hipSuccess) {                // off the thread's sticky slot; one that succeeds touches nothing, so a pending
    (void)hipGetLastError();                             // error of earlier work stays for whoever asks for it.
    return 0;
  }
  static int cus[64];
  if (dev < 0 || dev >= 64) return 0;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    cus[dev] = n;
  }
  return cus[dev];
}

static void conv0_mx8_choose(long M, int Cout, int* rows, int* cols) {
  const long W = (M + 255) / 256 * cdiv(Cout, 256), cus = conv0_mx8_cus();
  if (cus <= 0 || 16 * W > MXN_MID_UPTO_16THS * cus) *rows = 256, *cols = 256;
  else if (16 * W > MXN_SMALL_UPTO_16THS * cus) *rows = 128, *cols = 64;
  else *rows = 64, *cols = 64;
}

extern "C" int drn_conv0_mx8_bn_choose(int Q, int L, int Cout, int* rows, int* cols) {
  DRN_CHECK_ARG(rows && cols, "drn_conv0_mx8_bn_choose: null pointer");
  DRN_CHECK_ARG(Q > 0 && L > 0 && Cout > 0 && (long)Q * L <= 0x7fffffffL - MXT_ROWS, "drn_conv0_mx8_bn_choose: bad args (Q %d, L %d, Cout %d)", Q,
                L, Cout);
  conv0_mx8_choose((long)Q * L, Cout, rows, cols);       // (a box without a device answers "wide": conv0_mx8_cus)
  return DRN_OK;
}

extern "C" int drn_conv0_mx8_bn_tile(const uint8_t* codes, int ld_codes, const uint8_t* scales, int ld_scales, const void* pos, int ld_pos,
                                     int n_rows, int pad_row, const int32_t* prop_off, int Nv, const uint8_t* wcodes, const uint8_t* wscales,
                                     const void* wpos, int S, const int32_t* pq, const int32_t* pq_host, const int32_t* pv, const int32_t* vids,
                                     int Vc, const float* ss, const float* gate, int ldg, void* out, int ld_out, void* gated, int ld_gated,
                                     int out_f32, int Q, int L, int C, int P, int Cout, int tile_rows, int tile_cols, void* stream) {
  const bool choose = tile_rows == 0 && tile_cols == 0;
  DRN_CHECK_ARG(choose || (tile_rows == 256 && tile_cols == 256) || (tile_rows == 128 && tile_cols == 64) || (tile_rows == 64 && tile_cols == 64),
                "drn_conv0_mx8_bn_tile: no %d x %d tile (256 x 256, 128 x 64, 64 x 64; 0, 0: choose)", tile_rows, tile_cols);
  DRN_CHECK_ARG(Q > 0 && L > 0 && Cout > 0 && (long)Q * L <= 0x7fffffffL - MXT_ROWS &&
                    ((long)Q * L + 63) / 64 * cdiv(Cout, 64) <= 0x7fffffffL,
                "drn_conv0_mx8_bn_tile: bad args (Q %d, L %d, Cout %d), or more than 2^31 rows or workgroups", Q, L, Cout);
  if (choose) conv0_mx8_choose((long)Q * L, Cout, &tile_rows, &tile_cols);
  // (the wide tile: drn_conv0_mx8_bn's launch, under its name)
  return conv0_mx8_bn_run(tile_rows == 256 ? "drn_conv0_mx8_bn" : "drn_conv0_mx8_bn_tile", CONV0_MX8_ARGS(ss, gate, ldg, out, ld_out, gated, ld_gated),
                          pq_host, out_f32, tile_rows, stream);
}
