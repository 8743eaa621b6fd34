// Compact prefill GEMMs (opt-in: MLA.predict_action_diff(prefill="compact"), mla_amd/infer.py). One observation is ~545 prefix rows; the
// training GEMM's 256-row tiles (built for 17 536 rows) turn that into 3 row tiles of which 2.13 hold work and, for the two N = 4096
// projections, 48 workgroups on 256 CUs. This family is sized for 1 <= M <= 1024 rows instead:
//   out[M, N] = x[M, K] . W^T, W [N, K] row-major as the projections are stored, fp32 accumulation, ONE rounding to bf16;
//   tile 64 x rows by 128 W rows by one 128-byte K tile row per workgroup of 4 waves (wave w: W rows [32 w, 32 w + 32) against all 64 x
//   rows, 8 accumulators), operands staged through registers into two LDS buffers of 8 + 16 KiB (one barrier per K tile), 16-B chunk c of
//   row r stored at slot c ^ ((r >> 1) & 7) of its 128-B row: the 16-lane groups of ds_read_b128 then touch 16 different 16-B slots of the
//   256-B bank row;
//   split-K (plan: until tiles x split >= 2 x 256 CUs, at least 8 K tiles per slice): slice s of tile (tm, tn) writes its fp32 partial
//   tile to the caller's workspace [split][ceil(M / 64) * 64][N]; reduce_kernel adds the slices in the order s = 0, 1, ... and runs the
//   epilogue. No atomics, no counters: the same inputs give the same bits on every run.
// Three forms share the main loop (FORM):
//   plain    + optional residual; rows addressed like the skinny / suffix kernels (ldo, out_batch_stride, rows_per_batch)
//   rope     the rotary embedding of columns [0, rope_cols) in the epilogue (a 128-column tile is one head: channel d and its partner
//            d + 64 sit in the same tile), on the fp32 sums
//   swiglu   W = packed gate|up [2 I, K]; tile column c < 64 is gate channel 64 tn + c, c >= 64 up channel 64 tn + c - 64; the epilogue
//            writes silu(gate) * up (swiglu_fwd_elem on the fp32 sums) to act [M, I] only
// Workgroup id -> tile: one contiguous chunk of the (tn major, tm minor) order per XCD (id % 8), so the row tiles that share a W tile
// run next to each other on one XCD's L2.
// Two operand kinds share all of the above (OP):
//   OpBf16   bf16 x and W, a K tile of 64 elements in two steps of v_mfma_f32_16x16x32_bf16 (lane group g reads chunk 4 kk + g of its
//            row); K % 32 == 0, the last K tile predicated per 16-B chunk
//   OpF8     (prefill_precision="fp8") e4m3fn codes of BOTH operands with one fp32 scale per row, exactly what mla_quant_fp8_rows writes;
//            a K tile of 128 codes in one v_mfma_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3 x e4m3; the builtin with constant zero scale
//            operands is the non-scaled instruction), 4 x the k of the bf16 MFMA in twice its cycles; K % 128 == 0, every K tile whole.
//            Lane (g = l >> 4, li = l & 15) of BOTH operands holds bytes [32 g, 32 g + 32) of its row's K tile in byte order. Whatever k
//            the hardware assigns to (g, byte j), it is the same k in A and in B, so every product pairs xq[m, k] with Wq[n, k] and the
//            sum over the tile is complete (tests/test_prefill_f8_gemm_gpu.py proves it with exact integer sums). The sums run over the
//            unscaled codes; the epilogue forms v = (sum * x_scale[m]) * w_scale[n] in fp32 BEFORE the rotation (the partner channel
//            n ^ 64 with ITS scale), before swiglu_fwd_elem (gate and up with the scales of their own rows of the packed matrix) and
//            before the residual; one rounding.
// The wide-row FP8 family (opt-in: MLA.predict_action_diff_batch(batch_prefill="fp8"), the B x S_p prefix rows of a batched call;
// mla_gemm_prefill_f8_wide*): OpF8's contract for 1 <= M <= 65536. Main loop, epilogues and reduction launch are templated on the row tile
// BMT (Geo<BMT>); plan_wide chooses it:
//   BMT  64  the compact instantiation and split rule; always for M <= 1024, where the wide entry points launch what the compact ones
//            launch (same bits), and beyond while 128-row tiles alone would not give three workgroups per CU
//   BMT 128  M > 1024 and ceil(M / 128) * (N / 128) >= 3 x 256: a 2 x 2 grid of waves, wave (wn, wm) W rows [64 wn, 64 wn + 64) against x
//            rows [64 wm, 64 wm + 64), 16 accumulators; per K tile a wave reads (64 + 64) x 128 B of LDS for 64 . 64 . 128 MACs -- 32 per
//            byte against the 64-row tile's 21; two stages of 16 + 16 KiB, x staged 4 rows per thread; the swizzle is conflict-free as
//            before (a fragment's rows are 16 i + li on both tiles). Such a plan never splits: the split rule stops at two per CU.
//   Measured at the 7B widths, M = 1090 .. 4360 (profiles/batch_prefill_fp8_infer_latency.txt): 0.64-0.88 x the time of the 64-row kernel
//   run in slices of <= 1024 rows, up to 1.49 PFLOP/s; the threshold (three per CU, not the two it started with) follows that table.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

constexpr int BM = 64, BM_WIDE = 128, BN = 128; // row tiles: the compact family's, and the wide family's second choice
constexpr int ROWB = 128;                       // bytes of a K tile row, both operand kinds
constexpr int MMAX = 1024, MMAX_WIDE = 65536;
constexpr int CUS = 256;                        // the launcher plans for the MI355X's 256 CUs (no device query, no state)
constexpr int MAX_SPLIT = 16, MIN_KTILES = 8;
constexpr int CT_LD = BN + 4;                   // fp32 row pitch of the finished tile in LDS (16-B aligned rows)
enum { PLAIN = 0, ROPE = 1, SWIGLU = 2 };

// The 4 waves of a workgroup over a BMT x 128 tile: WAVES_N x WAVES_M waves of WN W rows (NT fragments of 16) by 64 x rows (4 fragments).
//   BMT  64: 4 x 1 waves of 32 x 64,  8 accumulators; a wave reads (32 + 64) x 128 B of LDS per K tile for 32 . 64 . 128 MACs (21 / B)
//   BMT 128: 2 x 2 waves of 64 x 64, 16 accumulators; (64 + 64) x 128 B for 64 . 64 . 128 MACs (32 / B)
template <int BMT>
struct Geo {
  static_assert(BMT == 64 || BMT == 128, "row tile");
  static constexpr int WAVES_M = BMT / 64, WAVES_N = 4 / WAVES_M, WN = BN / WAVES_N, NT = WN / 16;
};

// An operand kind: element, K tile (BK elements = ROWB bytes), K granularity (KGRAN < BK: the last K tile is predicated per chunk),
// elements per 16-B chunk (= the alignment of ldx / ldw), whether per-row scales exist, and mma<NT>(): the MFMAs of one staged K tile --
// xs / wsm the wave's first x / W row in the swizzled tiles in LDS (64 x rows, 16 NT W rows), fsw the swizzle of the lane's fragment rows.
struct OpBf16 {
  typedef bf16_t elem;
  static constexpr int BK = 64, KGRAN = 32, CHUNK = 8;
  static constexpr bool SCALED = false;
  template <int NT>
  static __device__ __forceinline__ void mma(const char* xs, const char* wsm, int g, int li, int fsw, f32x4_t (&acc)[NT][4]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = ((kk * 4 + g) ^ fsw) << 4;
      u32x4_t af[NT], bfr[4];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) af[nt] = *(const u32x4_t*)(wsm + (nt * 16 + li) * ROWB + off);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) bfr[mb] = *(const u32x4_t*)(xs + (mb * 16 + li) * ROWB + off);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
          acc[nt][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[nt]), __builtin_bit_cast(bf16x8_t, bfr[mb]),
                                                                acc[nt][mb], 0, 0, 0);
    }
  }
};

struct OpF8 {
  typedef uint8_t elem;
  static constexpr int BK = 128, KGRAN = 128, CHUNK = 16;
  static constexpr bool SCALED = true;
  static __device__ __forceinline__ i32x8_t frag(const char* row, int off0, int off1) {
    const u32x4_t lo = *(const u32x4_t*)(row + off0), hi = *(const u32x4_t*)(row + off1);
    return i32x8_t{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  }
  template <int NT>
  static __device__ __forceinline__ void mma(const char* xs, const char* wsm, int g, int li, int fsw, f32x4_t (&acc)[NT][4]) {
    const int off0 = ((2 * g) ^ fsw) << 4, off1 = ((2 * g + 1) ^ fsw) << 4;      // lane group g takes chunks 2 g and 2 g + 1 of the row
    i32x8_t af[NT], bfr[4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) af[nt] = frag(wsm + (nt * 16 + li) * ROWB, off0, off1);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) bfr[mb] = frag(xs + (mb * 16 + li) * ROWB, off0, off1);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        acc[nt][mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[nt], bfr[mb], acc[nt][mb], 0, 0, 0, 0, 0, 0);
  }
};

template <class OP>
struct Args {
  const typename OP::elem* x; long long ldx;
  const typename OP::elem* W; long long ldw;
  const float* xs; const float* wsc;             // OpF8: the scale of every x row / W row; null otherwise
  bf16_t* out; long long ldo, out_bs; int rpb;
  const bf16_t* res; long long ld_res;
  int M, N, K;                                   // N: W rows (2 I in the SwiGLU form)
  const float* rope_cos; const float* rope_sin; int rope_cols;
  float* ws; int split, sps;                     // sps: K tiles per slice
};

struct Plan { int bm, mt, nt, split, sps, wgs; long long ws_bytes; };

// tiles x split >= 2 x cus where K allows (two workgroups per CU: 4 waves each hide little on their own)
template <class OP>
inline Plan plan(int M, int N, int K, int cus, int bm = BM) {
  Plan p;
  p.bm = bm;
  p.mt = (M + bm - 1) / bm;
  p.nt = N / BN;
  const int tiles = p.mt * p.nt, ktiles = (K + OP::BK - 1) / OP::BK;
  p.split = 1;
  while (tiles * p.split < 2 * cus && p.split < MAX_SPLIT && ktiles / (p.split * 2) >= MIN_KTILES) p.split *= 2;
  p.sps = (ktiles + p.split - 1) / p.split;
  p.wgs = tiles * p.split;
  p.ws_bytes = p.split > 1 ? (long long)p.split * p.mt * bm * N * 4 : 0;
  return p;
}

// The wide family's plan: for M <= 1024 the compact family's plan -- tile, split and therefore bits; beyond, 128-row tiles once they
// alone give THREE workgroups per CU, 64-row tiles with the compact split rule below that. The rule started at two per CU; the measured
// table moved it (profiles/batch_prefill_fp8_infer_latency.txt): with 576 tiles of 128 rows on the 512 slots of two workgroups per CU
// (o and down at M = 2180) the second round runs one-eighth full and one launch of 1120 64-row tiles is 8-13 % faster, while from 864
// tiles on the 128-row tile wins every cell (by 7-15 %; 1-4 % at 1120). A 128-row plan never splits -- the split rule stops at two
// workgroups per CU --, so the launcher has no reduce launch for that tile (a rule that splits on it has to add the launch and its test).
constexpr int WIDE_WGS_PER_CU = 3;
template <class OP>
inline Plan plan_wide(int M, int N, int K, int cus) {
  const long long tiles128 = (long long)((M + BM_WIDE - 1) / BM_WIDE) * (N / BN);
  return plan<OP>(M, N, K, cus, M > MMAX && tiles128 >= (long long)WIDE_WGS_PER_CU * cus ? BM_WIDE : BM);
}

template <class OP>
inline bool shape_ok(int M, int N, int K, int mmax = MMAX) {
  return M >= 1 && M <= mmax && N >= BN && N % BN == 0 && K >= OP::KGRAN && K % OP::KGRAN == 0;
}

// workgroup id -> work item: XCD x (= id % 8) walks items [x * per, (x + 1) * per) in order; the remainder keeps its id
__device__ __forceinline__ int item(int id, int total) {
  const int per = total >> 3;
  return id < per * 8 ? (id & 7) * per + (id >> 3) : id;
}

// W row (= output-scale index) of tile column c
template <int FORM>
__device__ __forceinline__ long long wrow(int tn, int c, int N) {
  if (FORM == SWIGLU) return c < 64 ? tn * 64 + c : (N >> 1) + tn * 64 + (c - 64);
  return tn * BN + c;
}

// The epilogue of tile (tm, tn): sum8(ml, cl, f) yields the 8 finished fp32 sums of tile row ml, tile columns cl .. cl + 7; OpF8's are
// scaled here, per row and per W row, in front of everything else.
template <class OP, int FORM, int BMT, class L>
__device__ __forceinline__ void epilogue(const Args<OP>& a, int tm, int tn, L sum8) {
  constexpr int CH = FORM == SWIGLU ? 8 : 16;              // 8-column output chunks per tile row
  for (int e = threadIdx.x; e < BMT * CH; e += 256) {
    const int ml = e / CH, ch = e % CH, m = tm * BMT + ml;
    if (m >= a.M) continue;
    [[maybe_unused]] float sx = 0.f;
    if constexpr (OP::SCALED) sx = a.xs[m];
    auto load8 = [&](int cl, float* f) {
      sum8(ml, cl, f);
      if constexpr (OP::SCALED) {
        const float* sw = a.wsc + wrow<FORM>(tn, cl, a.N);  // 8 columns from a multiple of 8 stay inside one half of a SwiGLU tile
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (f[j] * sx) * sw[j];
      }
    };
    float v[8];
    int ncol;
    if (FORM == SWIGLU) {
      float gt[8], up[8];
      load8(ch * 8, gt);
      load8(64 + ch * 8, up);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = swiglu_fwd_elem(gt[j], up[j]);
      ncol = tn * 64 + ch * 8;
    } else {
      load8(ch * 8, v);
      ncol = tn * BN + ch * 8;
      if (FORM == ROPE && ncol < a.rope_cols) {
        // apply_rotary_pos_emb (modeling_llama.py:184-208) per head of 128: a' = a cos - b sin, b' = b cos + a sin, b = a's channel + 64
        float o[8];
        load8((ch * 8) ^ 64, o);
        const int d = (ch * 8) & 63, pos = m % a.rpb;
        const float* cp = a.rope_cos + (long long)pos * 64 + d;
        const float* sp = a.rope_sin + (long long)pos * 64 + d;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ch < 8 ? fmaf(v[j], cp[j], -(o[j] * sp[j])) : fmaf(v[j], cp[j], o[j] * sp[j]);
      }
      if (FORM == PLAIN && a.res) {
        float r[8];
        unpack8(*(const u32x4_t*)(a.res + (long long)m * a.ld_res + ncol), r);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += r[j];
      }
    }
    *(u32x4_t*)(a.out + (long long)(m / a.rpb) * a.out_bs + (long long)(m % a.rpb) * a.ldo + ncol) = pack8(v);
  }
}

template <class OP, int FORM, int BMT>
__global__ __launch_bounds__(256) void kernel(const Args<OP> a) {
  static_assert(OP::BK * sizeof(typename OP::elem) == ROWB && OP::CHUNK * sizeof(typename OP::elem) == 16, "a K tile row is 8 16-B chunks");
  typedef Geo<BMT> G;
  constexpr int XJ = BMT / 32;                                                         // x rows a thread stages per K tile
  constexpr int XB = BMT * ROWB, WB = BN * ROWB, STAGE = XB + WB;                      // 8 | 16 + 16 KiB per stage
  // the finished tile reuses the staging buffers (BMT 128: 2 KiB more than the two 32-KiB stages; two workgroups still share a CU's LDS)
  constexpr int SMEM = 2 * STAGE > BMT * CT_LD * 4 ? 2 * STAGE : BMT * CT_LD * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int wn = wave % G::WAVES_N, wm = wave / G::WAVES_N;                            // the wave's W rows [WN wn, ..), x rows [64 wm, ..)
  const int ntn = a.N / BN, ntm = (a.M + BMT - 1) / BMT, tiles = ntm * ntn;
  const int it = item(blockIdx.x, tiles * a.split);
  const int sp = it / tiles, t = it - sp * tiles, tn = t / ntm, tm = t - tn * ntm;
  const int ktiles = (a.K + OP::BK - 1) / OP::BK;
  const int kt0 = sp * a.sps, kt1 = kt0 + a.sps < ktiles ? kt0 + a.sps : ktiles;
  // staging: thread -> 16-B chunk c of rows r0 + 32 j (x: j < BMT / 32, W: j < 4); (r >> 1) & 7 does not depend on j
  const int c = tid & 7, r0 = tid >> 3;
  const int sw = ((c ^ ((r0 >> 1) & 7)) << 4) + r0 * ROWB;
  const typename OP::elem* xp[XJ];
  bool xok[XJ];
  const typename OP::elem* wp[4];
#pragma unroll
  for (int j = 0; j < XJ; ++j) {
    const int m = tm * BMT + r0 + 32 * j;
    xok[j] = m < a.M;
    xp[j] = a.x + (long long)(xok[j] ? m : 0) * a.ldx + c * OP::CHUNK;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) wp[j] = a.W + wrow<FORM>(tn, r0 + 32 * j, a.N) * a.ldw + c * OP::CHUNK;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  u32x4_t rx[XJ], rw[4];
  f32x4_t acc[G::NT][4];
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[nt][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto gload = [&](int kt) {
    const int k = kt * OP::BK;                     // < K: 32-bit (a 64-bit k costs both kinds address arithmetic in the loop)
    bool ok = true;                                // K % CHUNK == 0: a chunk is inside K or beyond it as a whole
    if constexpr (OP::KGRAN < OP::BK) ok = k + c * OP::CHUNK < a.K;
#pragma unroll
    for (int j = 0; j < XJ; ++j) rx[j] = ok && xok[j] ? *(const u32x4_t*)(xp[j] + k) : zero;
#pragma unroll
    for (int j = 0; j < 4; ++j) rw[j] = ok ? *(const u32x4_t*)(wp[j] + k) : zero;
  };
  auto lstore = [&](int buf) {
    char* xs = smem + buf * STAGE;
#pragma unroll
    for (int j = 0; j < XJ; ++j) *(u32x4_t*)(xs + sw + j * 32 * ROWB) = rx[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) *(u32x4_t*)(xs + XB + sw + j * 32 * ROWB) = rw[j];
  };
  if (kt0 < kt1) {
    gload(kt0);
    lstore(0);
  }
  __syncthreads();
  const int fsw = (li >> 1) & 7;                   // swizzle of a fragment row: rows 16 i + li, (row >> 1) & 7 = (li >> 1) & 7
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;                // block-uniform
    if (more) gload(kt + 1);
    const char* xs = smem + buf * STAGE;
    OP::template mma<G::NT>(xs + wm * 64 * ROWB, xs + XB + wn * G::WN * ROWB, g, li, fsw, acc);
    if (more) lstore(buf ^ 1);
    __syncthreads();
  }
  // D[n][m] of (nt, mb): W row WN wn + 16 nt + 4 g + reg, x row 64 wm + 16 mb + li -> 4 consecutive tile columns per lane
  const int trow = wm * 64 + li, tcol = wn * G::WN + g * 4;
  if (a.split > 1) {
    const long long mpad = (long long)ntm * BMT;
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        *(f32x4_t*)(a.ws + ((long long)sp * mpad + tm * BMT + mb * 16 + trow) * a.N + tn * BN + tcol + nt * 16) = acc[nt][mb];
    return;
  }
  float* ct = (float*)smem;                        // every wave is behind the loop's last barrier: the staging buffers are free
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) *(f32x4_t*)(ct + (mb * 16 + trow) * CT_LD + tcol + nt * 16) = acc[nt][mb];
  __syncthreads();
  epilogue<OP, FORM, BMT>(a, tm, tn, [&](int ml, int cl, float* f) {
    const f32x4_t lo = *(const f32x4_t*)(ct + ml * CT_LD + cl), hi = *(const f32x4_t*)(ct + ml * CT_LD + cl + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
  });
}

// one workgroup per tile: the slices' partial tiles added in the order s = 0, 1, ..., then the epilogue
template <class OP, int FORM, int BMT>
__global__ __launch_bounds__(256) void reduce_kernel(const Args<OP> a) {
  const int ntm = (a.M + BMT - 1) / BMT;
  const int tn = blockIdx.x / ntm, tm = blockIdx.x - tn * ntm;
  const long long slice = (long long)ntm * BMT * a.N;
  epilogue<OP, FORM, BMT>(a, tm, tn, [&](int ml, int cl, float* f) {
    const float* p = a.ws + (long long)(tm * BMT + ml) * a.N + tn * BN + cl;
    f32x4_t lo = *(const f32x4_t*)p, hi = *(const f32x4_t*)(p + 4);
    for (int s = 1; s < a.split; ++s) {
      lo += *(const f32x4_t*)(p + s * slice);
      hi += *(const f32x4_t*)(p + s * slice + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
  });
}

#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)
#define SHAPE_MSG "%s: 1 <= M <= 1024, N %% 128 == 0, K %% %d == 0 required (M %d, N %d, K %d)"
#define SHAPE_MSG_WIDE "%s: 1 <= M <= 65536, N %% 128 == 0, K %% %d == 0 required (M %d, N %d, K %d)"

// WIDE: the entry points that accept up to 65 536 rows and let the plan choose the row tile (plan_wide)
template <class OP, int FORM, bool WIDE = false>
int entry(const char* name, const void* x, long long ldx, const float* x_scale, const void* W, long long ldw, const float* w_scale, void* out,
          long long ldo, long long out_bs, int rpb, const void* res, long long ld_res, int M, int N, int K, const float* rope_cos,
          const float* rope_sin, int rope_cols, void* ws, size_t ws_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(x && W && out && (!OP::SCALED || (x_scale && w_scale)), "%s: null pointer", name);
  MLA_CHECK_ARG(shape_ok<OP>(M, N, K, WIDE ? MMAX_WIDE : MMAX) && rpb >= 1, WIDE ? SHAPE_MSG_WIDE : SHAPE_MSG, name, OP::KGRAN, M, N, K);
  MLA_CHECK_ARG(AL16(x) && AL16(W) && AL16(out) && ldx % OP::CHUNK == 0 && ldw % OP::CHUNK == 0 && ldo % 8 == 0 && out_bs % 8 == 0 &&
                    ldx >= K && ldw >= K,
                "%s: %s / out rows must be 16-B aligned", name, OP::SCALED ? "xq / Wq" : "x / W");
  MLA_CHECK_ARG(!res || (AL16(res) && ld_res % 8 == 0), "%s: residual rows must be 16-B aligned", name);
  if (FORM == ROPE)
    MLA_CHECK_ARG(rope_cos && rope_sin && AL16(rope_cos) && AL16(rope_sin) && rope_cols > 0 && rope_cols % 128 == 0 && rope_cols <= N,
                  "%s: the RoPE epilogue needs both tables (16-B aligned) and rope_cols a multiple of 128 (head_dim 128) and <= N", name);
  const Plan p = WIDE ? plan_wide<OP>(M, N, K, CUS) : plan<OP>(M, N, K, CUS);
  MLA_CHECK_ARG(p.split == 1 || (ws && AL16(ws) && (long long)ws_bytes >= p.ws_bytes),
                "%s: workspace of %lld bytes (16-B aligned) needed for split-K %d, got %lld", name, p.ws_bytes, p.split, (long long)ws_bytes);
  Args<OP> a;
  a.x = (const typename OP::elem*)x; a.ldx = ldx; a.W = (const typename OP::elem*)W; a.ldw = ldw;
  a.xs = x_scale; a.wsc = w_scale;
  a.out = (bf16_t*)out; a.ldo = ldo; a.out_bs = out_bs; a.rpb = rpb;
  a.res = (const bf16_t*)res; a.ld_res = ld_res;
  a.M = M; a.N = N; a.K = K;
  a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.rope_cols = rope_cols;
  a.ws = (float*)ws; a.split = p.split; a.sps = p.sps;
  bool wide_tile = false;
  if constexpr (WIDE) {
    wide_tile = p.bm == BM_WIDE;
    MLA_CHECK_ARG(!wide_tile || p.split == 1, "%s: a 128-row plan does not split (plan_wide)", name);     // no reduce launch on this tile
    if (wide_tile) hipLaunchKernelGGL((kernel<OP, FORM, BM_WIDE>), dim3(p.wgs), dim3(256), 0, stream, a);
  }
  if (!wide_tile) {
    hipLaunchKernelGGL((kernel<OP, FORM, BM>), dim3(p.wgs), dim3(256), 0, stream, a);
    if (p.split > 1) hipLaunchKernelGGL((reduce_kernel<OP, FORM, BM>), dim3(p.mt * p.nt), dim3(256), 0, stream, a);
  }
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  mla_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
  return (int)e;
}

template <class OP, bool WIDE = false>
int plan_entry(const char* name, int M, int N, int K, int cus, int* out4) {
  MLA_CHECK_ARG(out4, "%s: null pointer", name);
  MLA_CHECK_ARG(shape_ok<OP>(M, N, K, WIDE ? MMAX_WIDE : MMAX) && cus >= 1, WIDE ? SHAPE_MSG_WIDE : SHAPE_MSG, name, OP::KGRAN, M, N, K);
  const Plan p = WIDE ? plan_wide<OP>(M, N, K, cus) : plan<OP>(M, N, K, cus);
  out4[0] = p.bm; out4[1] = BN; out4[2] = p.split; out4[3] = p.wgs;
  return 0;
}

template <class OP, bool WIDE = false>
long long ws_bytes_entry(const char* name, int M, int N, int K) {
  MLA_CHECK_ARG(shape_ok<OP>(M, N, K, WIDE ? MMAX_WIDE : MMAX), WIDE ? SHAPE_MSG_WIDE : SHAPE_MSG, name, OP::KGRAN, M, N, K);
  return (WIDE ? plan_wide<OP>(M, N, K, CUS) : plan<OP>(M, N, K, CUS)).ws_bytes;
}

}  // namespace

extern "C" int mla_gemm_prefill_plan(int M, int N, int K, int cus, int* out4) {
  return plan_entry<OpBf16>("mla_gemm_prefill_plan", M, N, K, cus, out4);
}

extern "C" int mla_gemm_prefill_f8_plan(int M, int N, int K, int cus, int* out4) {
  return plan_entry<OpF8>("mla_gemm_prefill_f8_plan", M, N, K, cus, out4);
}

extern "C" long long mla_gemm_prefill_ws_bytes(int M, int N, int K) { return ws_bytes_entry<OpBf16>("mla_gemm_prefill_ws_bytes", M, N, K); }

extern "C" long long mla_gemm_prefill_f8_ws_bytes(int M, int N, int K) { return ws_bytes_entry<OpF8>("mla_gemm_prefill_f8_ws_bytes", M, N, K); }

extern "C" int mla_gemm_prefill_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                                     int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, void* workspace,
                                     size_t workspace_bytes, hipStream_t stream) {
  return entry<OpBf16, PLAIN>("mla_gemm_prefill_bf16", x, ldx, nullptr, W, ldw, nullptr, out, ldo, out_batch_stride, rows_per_batch, residual,
                              ld_res, M, N, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw, const float* w_scale,
                                   void* out, long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual,
                                   long long ld_res, int M, int N, int K, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return entry<OpF8, PLAIN>("mla_gemm_prefill_f8", xq, ldx, x_scale, Wq, ldw, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual,
                            ld_res, M, N, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_qkv_rope(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo,
                                         long long out_batch_stride, int rows_per_batch, int M, int N, int K, const float* rope_cos,
                                         const float* rope_sin, int rope_cols, int head_dim, void* workspace, size_t workspace_bytes,
                                         hipStream_t stream) {
  MLA_CHECK_ARG(head_dim == 128, "mla_gemm_prefill_qkv_rope: head_dim must be 128 (got %d)", head_dim);
  return entry<OpBf16, ROPE>("mla_gemm_prefill_qkv_rope", x, ldx, nullptr, W, ldw, nullptr, out, ldo, out_batch_stride, rows_per_batch, nullptr,
                             0, M, N, K, rope_cos, rope_sin, rope_cols, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8_qkv_rope(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw,
                                            const float* w_scale, void* out, long long ldo, long long out_batch_stride, int rows_per_batch,
                                            int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols, int head_dim,
                                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(head_dim == 128, "mla_gemm_prefill_f8_qkv_rope: head_dim must be 128 (got %d)", head_dim);
  return entry<OpF8, ROPE>("mla_gemm_prefill_f8_qkv_rope", xq, ldx, x_scale, Wq, ldw, w_scale, out, ldo, out_batch_stride, rows_per_batch,
                           nullptr, 0, M, N, K, rope_cos, rope_sin, rope_cols, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_gateup_swiglu(const void* x, long long ldx, const void* wgu, long long ldw, void* act, long long ldo,
                                              long long out_batch_stride, int rows_per_batch, int M, int I, int K, void* workspace,
                                              size_t workspace_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(I >= 64 && I % 64 == 0 && I <= (1 << 29), "mla_gemm_prefill_gateup_swiglu: I %% 64 == 0 required (I %d)", I);
  return entry<OpBf16, SWIGLU>("mla_gemm_prefill_gateup_swiglu", x, ldx, nullptr, wgu, ldw, nullptr, act, ldo, out_batch_stride, rows_per_batch,
                               nullptr, 0, M, 2 * I, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8_gateup_swiglu(const void* xq, long long ldx, const float* x_scale, const void* wgu_q, long long ldw,
                                                 const float* w_scale, void* act, long long ldo, long long out_batch_stride,
                                                 int rows_per_batch, int M, int I, int K, void* workspace, size_t workspace_bytes,
                                                 hipStream_t stream) {
  MLA_CHECK_ARG(I >= 64 && I % 64 == 0 && I <= (1 << 29), "mla_gemm_prefill_f8_gateup_swiglu: I %% 64 == 0 required (I %d)", I);
  return entry<OpF8, SWIGLU>("mla_gemm_prefill_f8_gateup_swiglu", xq, ldx, x_scale, wgu_q, ldw, w_scale, act, ldo, out_batch_stride,
                             rows_per_batch, nullptr, 0, M, 2 * I, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

// ---- the wide-row FP8 family: the contract of mla_gemm_prefill_f8* for 1 <= M <= 65536, the row tile (64 | 128) chosen by plan_wide
extern "C" int mla_gemm_prefill_f8_wide_plan(int M, int N, int K, int cus, int* out4) {
  return plan_entry<OpF8, true>("mla_gemm_prefill_f8_wide_plan", M, N, K, cus, out4);
}

extern "C" long long mla_gemm_prefill_f8_wide_ws_bytes(int M, int N, int K) {
  return ws_bytes_entry<OpF8, true>("mla_gemm_prefill_f8_wide_ws_bytes", M, N, K);
}

extern "C" int mla_gemm_prefill_f8_wide(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw,
                                        const float* w_scale, void* out, long long ldo, long long out_batch_stride, int rows_per_batch,
                                        const void* residual, long long ld_res, int M, int N, int K, void* workspace, size_t workspace_bytes,
                                        hipStream_t stream) {
  return entry<OpF8, PLAIN, true>("mla_gemm_prefill_f8_wide", xq, ldx, x_scale, Wq, ldw, w_scale, out, ldo, out_batch_stride, rows_per_batch,
                                  residual, ld_res, M, N, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8_wide_qkv_rope(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw,
                                                 const float* w_scale, void* out, long long ldo, long long out_batch_stride,
                                                 int rows_per_batch, int M, int N, int K, const float* rope_cos, const float* rope_sin,
                                                 int rope_cols, int head_dim, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(head_dim == 128, "mla_gemm_prefill_f8_wide_qkv_rope: head_dim must be 128 (got %d)", head_dim);
  return entry<OpF8, ROPE, true>("mla_gemm_prefill_f8_wide_qkv_rope", xq, ldx, x_scale, Wq, ldw, w_scale, out, ldo, out_batch_stride,
                                 rows_per_batch, nullptr, 0, M, N, K, rope_cos, rope_sin, rope_cols, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8_wide_gateup_swiglu(const void* xq, long long ldx, const float* x_scale, const void* wgu_q, long long ldw,
                                                      const float* w_scale, void* act, long long ldo, long long out_batch_stride,
                                                      int rows_per_batch, int M, int I, int K, void* workspace, size_t workspace_bytes,
                                                      hipStream_t stream) {
  MLA_CHECK_ARG(I >= 64 && I % 64 == 0 && I <= (1 << 29), "mla_gemm_prefill_f8_wide_gateup_swiglu: I %% 64 == 0 required (I %d)", I);
  return entry<OpF8, SWIGLU, true>("mla_gemm_prefill_f8_wide_gateup_swiglu", xq, ldx, x_scale, wgu_q, ldw, w_scale, act, ldo,
                                   out_batch_stride, rows_per_batch, nullptr, 0, M, 2 * I, K, nullptr, nullptr, 0, workspace,
                                   workspace_bytes, stream);
}
