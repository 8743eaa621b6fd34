// Compact prefill GEMMs (opt-in: MLA.predict_action_diff(prefill="compact"), mla_amd/infer.py). One observation is ~545 prefix rows; the
// training GEMM's 256-row tiles (built for 17 536 rows) turn that into 3 row tiles of which 2.13 hold work and, for the two N = 4096
// projections, 48 workgroups on 256 CUs. This family is sized for 1 <= M <= 1024 rows instead:
//   out[M, N] = x[M, K] . W^T, W [N, K] row-major as the projections are stored, fp32 accumulation, ONE rounding to bf16;
//   tile 64 x rows by 128 W rows by 64 k per workgroup of 4 waves (wave w: W rows [32 w, 32 w + 32) against all 64 x rows, 8 accumulators
//   of v_mfma_f32_16x16x32_bf16), operands staged through registers into two LDS buffers (one barrier per K tile), 16-B chunk c of row r
//   stored at slot c ^ ((r >> 1) & 7) of its 128-B row: the 16-lane groups of ds_read_b128 then touch 16 different 16-B slots of the
//   256-B bank row;
//   split-K (prefill_plan: until tiles x split >= 2 x 256 CUs, at least 8 K tiles per slice): slice s of tile (tm, tn) writes its fp32
//   partial tile to the caller's workspace [split][ceil(M / 64) * 64][N]; gemm_prefill_reduce_kernel adds the slices in the order
//   s = 0, 1, ... and runs the epilogue. No atomics, no counters: the same inputs give the same bits on every run.
// Three forms share the main loop (FORM):
//   plain    + optional residual; rows addressed like the skinny / suffix kernels (ldo, out_batch_stride, rows_per_batch)
//   rope     the rotary embedding of columns [0, rope_cols) in the epilogue (a 128-column tile is one head: channel d and its partner
//            d + 64 sit in the same tile), on the fp32 sums
//   swiglu   W = packed gate|up [2 I, K]; tile column c < 64 is gate channel 64 tn + c, c >= 64 up channel 64 tn + c - 64; the epilogue
//            writes silu(gate) * up (swiglu_fwd_elem on the fp32 sums) to act [M, I] only
// Workgroup id -> tile: one contiguous chunk of the (tn major, tm minor) order per XCD (id % 8), so the row tiles that share a W tile
// run next to each other on one XCD's L2.
#include "common.h"

namespace {

constexpr int PF_BM = 64, PF_BN = 128, PF_BK = 64;
constexpr int PF_MMAX = 1024;
constexpr int PF_CUS = 256;                     // the launcher plans for the MI355X's 256 CUs (no device query, no state)
constexpr int PF_MAX_SPLIT = 16, PF_MIN_KTILES = 8;
constexpr int PF_CT_LD = PF_BN + 4;             // fp32 row pitch of the finished tile in LDS (16-B aligned rows)
enum { PF_PLAIN = 0, PF_ROPE = 1, PF_SWIGLU = 2 };

struct PrefillArgs {
  const bf16_t* x; long long ldx;
  const bf16_t* W; long long ldw;
  bf16_t* out; long long ldo, out_bs; int rpb;
  const bf16_t* res; long long ld_res;
  int M, N, K;                                   // N: W rows (2 I in the SwiGLU form)
  const float* rope_cos; const float* rope_sin; int rope_cols;
  float* ws; int split, sps;                     // sps: K tiles per slice
};

struct PrefillPlan { int mt, nt, split, sps, wgs; long long ws_bytes; };

// tiles x split >= 2 x cus where K allows (two workgroups per CU: 4 waves each hide little on their own)
inline PrefillPlan prefill_plan(int M, int N, int K, int cus) {
  PrefillPlan p;
  p.mt = (M + PF_BM - 1) / PF_BM;
  p.nt = N / PF_BN;
  const int tiles = p.mt * p.nt, ktiles = (K + PF_BK - 1) / PF_BK;
  p.split = 1;
  while (tiles * p.split < 2 * cus && p.split < PF_MAX_SPLIT && ktiles / (p.split * 2) >= PF_MIN_KTILES) p.split *= 2;
  p.sps = (ktiles + p.split - 1) / p.split;
  p.wgs = tiles * p.split;
  p.ws_bytes = p.split > 1 ? (long long)p.split * p.mt * PF_BM * N * 4 : 0;
  return p;
}

// workgroup id -> work item: XCD x (= id % 8) walks items [x * per, (x + 1) * per) in order; the remainder keeps its id
__device__ __forceinline__ int pf_item(int id, int total) {
  const int per = total >> 3;
  return id < per * 8 ? (id & 7) * per + (id >> 3) : id;
}

template <int FORM>
__device__ __forceinline__ long long pf_wrow(int tn, int c, int N) {
  if (FORM == PF_SWIGLU) return c < 64 ? tn * 64 + c : (N >> 1) + tn * 64 + (c - 64);
  return tn * PF_BN + c;
}

// The epilogue of tile (tm, tn): load8(ml, cl, f) yields the 8 finished fp32 sums of tile row ml, tile columns cl .. cl + 7.
template <int FORM, class L>
__device__ __forceinline__ void pf_epilogue(const PrefillArgs& a, int tm, int tn, L load8) {
  constexpr int CH = FORM == PF_SWIGLU ? 8 : 16;           // 8-column output chunks per tile row
  for (int e = threadIdx.x; e < PF_BM * CH; e += 256) {
    const int ml = e / CH, ch = e % CH, m = tm * PF_BM + ml;
    if (m >= a.M) continue;
    float v[8];
    int ncol;
    if (FORM == PF_SWIGLU) {
      float gt[8], up[8];
      load8(ml, ch * 8, gt);
      load8(ml, 64 + ch * 8, up);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = swiglu_fwd_elem(gt[j], up[j]);
      ncol = tn * 64 + ch * 8;
    } else {
      load8(ml, ch * 8, v);
      ncol = tn * PF_BN + ch * 8;
      if (FORM == PF_ROPE && ncol < a.rope_cols) {
        // apply_rotary_pos_emb (modeling_llama.py:184-208) per head of 128: a' = a cos - b sin, b' = b cos + a sin, b = a's channel + 64
        float o[8];
        load8(ml, (ch * 8) ^ 64, o);
        const int d = (ch * 8) & 63, pos = m % a.rpb;
        const float* cp = a.rope_cos + (long long)pos * 64 + d;
        const float* sp = a.rope_sin + (long long)pos * 64 + d;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ch < 8 ? fmaf(v[j], cp[j], -(o[j] * sp[j])) : fmaf(v[j], cp[j], o[j] * sp[j]);
      }
      if (FORM == PF_PLAIN && a.res) {
        float r[8];
        unpack8(*(const u32x4_t*)(a.res + (long long)m * a.ld_res + ncol), r);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += r[j];
      }
    }
    *(u32x4_t*)(a.out + (long long)(m / a.rpb) * a.out_bs + (long long)(m % a.rpb) * a.ldo + ncol) = pack8(v);
  }
}

template <int FORM>
__global__ __launch_bounds__(256) void gemm_prefill_kernel(const PrefillArgs a) {
  constexpr int XB = PF_BM * PF_BK * 2, WB = PF_BN * PF_BK * 2, STAGE = XB + WB;      // 8 + 16 KiB per stage
  static_assert(PF_BM * PF_CT_LD * 4 <= 2 * STAGE, "the finished tile reuses the staging buffers");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int ntn = a.N / PF_BN, ntm = (a.M + PF_BM - 1) / PF_BM, tiles = ntm * ntn;
  const int item = pf_item(blockIdx.x, tiles * a.split);
  const int sp = item / tiles, t = item - sp * tiles, tn = t / ntm, tm = t - tn * ntm;
  const int ktiles = (a.K + PF_BK - 1) / PF_BK;
  const int kt0 = sp * a.sps, kt1 = kt0 + a.sps < ktiles ? kt0 + a.sps : ktiles;
  // staging: thread -> chunk c of rows r0 + 32 j (x: j < 2, W: j < 4); (r >> 1) & 7 does not depend on j
  const int c = tid & 7, r0 = tid >> 3;
  const int sw = ((c ^ ((r0 >> 1) & 7)) << 4) + r0 * 128;
  const bf16_t* xp[2];
  bool xok[2];
  const bf16_t* wp[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = tm * PF_BM + r0 + 32 * j;
    xok[j] = m < a.M;
    xp[j] = a.x + (long long)(xok[j] ? m : 0) * a.ldx + c * 8;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) wp[j] = a.W + pf_wrow<FORM>(tn, r0 + 32 * j, a.N) * a.ldw + c * 8;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  u32x4_t rx[2], rw[4];
  f32x4_t acc[2][4];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[nt][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#define PF_GLOAD(KT)                                                                           \
  {                                                                                            \
    const int k = (KT) * PF_BK;                                                                \
    const bool ok = k + c * 8 < a.K;              /* K % 8 == 0: a chunk is inside K or beyond it as a whole */ \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) rx[j] = ok && xok[j] ? *(const u32x4_t*)(xp[j] + k) : zero; \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) rw[j] = ok ? *(const u32x4_t*)(wp[j] + k) : zero;           \
  }
#define PF_LSTORE(BUF)                                                                         \
  {                                                                                            \
    char* xs = smem + (BUF) * STAGE;                                                           \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) *(u32x4_t*)(xs + sw + j * 32 * 128) = rx[j]; \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) *(u32x4_t*)(xs + XB + sw + j * 32 * 128) = rw[j]; \
  }
  if (kt0 < kt1) {
    PF_GLOAD(kt0)
    PF_LSTORE(0)
  }
  __syncthreads();
  const int fsw = (li >> 1) & 7;                   // swizzle of a fragment row: rows 16 i + li, (row >> 1) & 7 = (li >> 1) & 7
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;                // block-uniform
    if (more) PF_GLOAD(kt + 1)
    const char* xs = smem + buf * STAGE;
    const char* wsm = xs + XB;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = ((kk * 4 + g) ^ fsw) << 4;
      u32x4_t af[2], bfr[4];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) af[nt] = *(const u32x4_t*)(wsm + (wave * 32 + nt * 16 + li) * 128 + off);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) bfr[mb] = *(const u32x4_t*)(xs + (mb * 16 + li) * 128 + off);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
          acc[nt][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[nt]), __builtin_bit_cast(bf16x8_t, bfr[mb]),
                                                                acc[nt][mb], 0, 0, 0);
    }
    if (more) PF_LSTORE(buf ^ 1)
    __syncthreads();
  }
#undef PF_GLOAD
#undef PF_LSTORE
  // D[n][m] of (nt, mb): W row 32 wave + 16 nt + 4 g + reg, x row 16 mb + li -> 4 consecutive tile columns per lane
  if (a.split > 1) {
    const long long mpad = (long long)ntm * PF_BM;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        *(f32x4_t*)(a.ws + ((long long)sp * mpad + tm * PF_BM + mb * 16 + li) * a.N + tn * PF_BN + wave * 32 + nt * 16 + g * 4) = acc[nt][mb];
    return;
  }
  float* ct = (float*)smem;                        // every wave is behind the loop's last barrier: the staging buffers are free
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) *(f32x4_t*)(ct + (mb * 16 + li) * PF_CT_LD + wave * 32 + nt * 16 + g * 4) = acc[nt][mb];
  __syncthreads();
  pf_epilogue<FORM>(a, tm, tn, [&](int ml, int cl, float* f) {
    const f32x4_t lo = *(const f32x4_t*)(ct + ml * PF_CT_LD + cl), hi = *(const f32x4_t*)(ct + ml * PF_CT_LD + cl + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
  });
}

// one workgroup per tile: the slices' partial tiles added in the order s = 0, 1, ..., then the epilogue
template <int FORM>
__global__ __launch_bounds__(256) void gemm_prefill_reduce_kernel(const PrefillArgs a) {
  const int ntn = a.N / PF_BN, ntm = (a.M + PF_BM - 1) / PF_BM;
  const int tn = blockIdx.x / ntm, tm = blockIdx.x - tn * ntm;
  const long long slice = (long long)ntm * PF_BM * a.N;
  pf_epilogue<FORM>(a, tm, tn, [&](int ml, int cl, float* f) {
    const float* p = a.ws + (long long)(tm * PF_BM + ml) * a.N + tn * PF_BN + cl;
    f32x4_t lo = *(const f32x4_t*)p, hi = *(const f32x4_t*)(p + 4);
    for (int s = 1; s < a.split; ++s) {
      lo += *(const f32x4_t*)(p + s * slice);
      hi += *(const f32x4_t*)(p + s * slice + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
  });
  (void)ntn;
}

#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

template <int FORM>
int prefill_entry(const char* name, const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_bs,
                  int rpb, const void* res, long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                  void* ws, size_t ws_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(x && W && out, "%s: null pointer", name);
  MLA_CHECK_ARG(M >= 1 && M <= PF_MMAX && N >= PF_BN && N % PF_BN == 0 && K >= 32 && K % 32 == 0 && rpb >= 1,
                "%s: 1 <= M <= 1024, N %% 128 == 0, K %% 32 == 0 required (M %d, N %d, K %d)", name, M, N, K);
  MLA_CHECK_ARG(AL16(x) && AL16(W) && AL16(out) && ldx % 8 == 0 && ldw % 8 == 0 && ldo % 8 == 0 && out_bs % 8 == 0 && ldx >= K && ldw >= K,
                "%s: x / W / out rows must be 16-B aligned", name);
  MLA_CHECK_ARG(!res || (AL16(res) && ld_res % 8 == 0), "%s: residual rows must be 16-B aligned", name);
  if (FORM == PF_ROPE)
    MLA_CHECK_ARG(rope_cos && rope_sin && AL16(rope_cos) && AL16(rope_sin) && rope_cols > 0 && rope_cols % 128 == 0 && rope_cols <= N,
                  "%s: the RoPE epilogue needs both tables (16-B aligned) and rope_cols a multiple of 128 (head_dim 128) and <= N", name);
  const PrefillPlan p = prefill_plan(M, N, K, PF_CUS);
  MLA_CHECK_ARG(p.split == 1 || (ws && AL16(ws) && (long long)ws_bytes >= p.ws_bytes),
                "%s: workspace of %lld bytes (16-B aligned) needed for split-K %d, got %lld", name, p.ws_bytes, p.split, (long long)ws_bytes);
  PrefillArgs a;
  a.x = (const bf16_t*)x; a.ldx = ldx; a.W = (const bf16_t*)W; a.ldw = ldw;
  a.out = (bf16_t*)out; a.ldo = ldo; a.out_bs = out_bs; a.rpb = rpb;
  a.res = (const bf16_t*)res; a.ld_res = ld_res;
  a.M = M; a.N = N; a.K = K;
  a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.rope_cols = rope_cols;
  a.ws = (float*)ws; a.split = p.split; a.sps = p.sps;
  hipLaunchKernelGGL((gemm_prefill_kernel<FORM>), dim3(p.wgs), dim3(256), 0, stream, a);
  if (p.split > 1) hipLaunchKernelGGL((gemm_prefill_reduce_kernel<FORM>), dim3(p.mt * p.nt), dim3(256), 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  mla_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
  return (int)e;
}

}  // namespace

extern "C" int mla_gemm_prefill_plan(int M, int N, int K, int cus, int* out4) {
  MLA_CHECK_ARG(out4, "mla_gemm_prefill_plan: null pointer");
  MLA_CHECK_ARG(M >= 1 && M <= PF_MMAX && N >= PF_BN && N % PF_BN == 0 && K >= 32 && K % 32 == 0 && cus >= 1,
                "mla_gemm_prefill_plan: 1 <= M <= 1024, N %% 128 == 0, K %% 32 == 0 required (M %d, N %d, K %d)", M, N, K);
  const PrefillPlan p = prefill_plan(M, N, K, cus);
  out4[0] = PF_BM; out4[1] = PF_BN; out4[2] = p.split; out4[3] = p.wgs;
  return 0;
}

extern "C" long long mla_gemm_prefill_ws_bytes(int M, int N, int K) {
  if (!(M >= 1 && M <= PF_MMAX && N >= PF_BN && N % PF_BN == 0 && K >= 32 && K % 32 == 0)) {
    mla_set_error("mla_gemm_prefill_ws_bytes: 1 <= M <= 1024, N %% 128 == 0, K %% 32 == 0 required (M %d, N %d, K %d)", M, N, K);
    return -1;
  }
  return prefill_plan(M, N, K, PF_CUS).ws_bytes;
}

extern "C" int mla_gemm_prefill_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                                     int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, void* workspace,
                                     size_t workspace_bytes, hipStream_t stream) {
  return prefill_entry<PF_PLAIN>("mla_gemm_prefill_bf16", x, ldx, W, ldw, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res, M, N, K,
                                 nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_qkv_rope(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo,
                                         long long out_batch_stride, int rows_per_batch, int M, int N, int K, const float* rope_cos,
                                         const float* rope_sin, int rope_cols, int head_dim, void* workspace, size_t workspace_bytes,
                                         hipStream_t stream) {
  MLA_CHECK_ARG(head_dim == 128, "mla_gemm_prefill_qkv_rope: head_dim must be 128 (got %d)", head_dim);
  return prefill_entry<PF_ROPE>("mla_gemm_prefill_qkv_rope", x, ldx, W, ldw, out, ldo, out_batch_stride, rows_per_batch, nullptr, 0, M, N, K,
                                rope_cos, rope_sin, rope_cols, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_gateup_swiglu(const void* x, long long ldx, const void* wgu, long long ldw, void* act, long long ldo,
                                              long long out_batch_stride, int rows_per_batch, int M, int I, int K, void* workspace,
                                              size_t workspace_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(I >= 64 && I % 64 == 0 && I <= (1 << 29), "mla_gemm_prefill_gateup_swiglu: I %% 64 == 0 required (I %d)", I);
  return prefill_entry<PF_SWIGLU>("mla_gemm_prefill_gateup_swiglu", x, ldx, wgu, ldw, act, ldo, out_batch_stride, rows_per_batch, nullptr, 0, M,
                                  2 * I, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}
