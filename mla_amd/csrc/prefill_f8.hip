// FP8 compact prefill GEMMs (opt-in: MLA.predict_action_diff(prefill="compact", prefill_precision="fp8"), mla_amd/infer.py). The W8A8 twin
// of prefill.hip: both operands are e4m3fn codes with one fp32 scale per row, exactly what mla_quant_fp8_rows writes --
//   out[m, n] = bf16((sum_k xq[m, k] Wq[n, k]) * x_scale[m] * w_scale[n])   1 <= M <= 1024, N % 128 == 0, K % 128 == 0
//   the sums run over the unscaled codes in fp32 on v_mfma_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3 x e4m3; the builtin with constant
//   zero scale operands is the non-scaled instruction), 4 x the k of the bf16 MFMA in twice its cycles;
//   tile 64 x rows by 128 W rows by 128 k per workgroup of 4 waves. A 128-code K tile row is 128 bytes like prefill.hip's 64 bf16, so the
//   staging (registers -> two LDS buffers of 8 + 16 KiB, one barrier per K tile) and the XOR swizzle (16-B chunk c of row r at slot
//   c ^ ((r >> 1) & 7)) are that kernel's byte for byte;
//   fragments: lane (g = l >> 4, li = l & 15) of BOTH operands holds bytes [32 g, 32 g + 32) of its row's K tile in byte order. Whatever k
//   the hardware assigns to (g, byte j), it is the same k in A and in B, so every product pairs xq[m, k] with Wq[n, k] and the sum over
//   the tile is complete (tests/test_prefill_f8_gemm_gpu.py proves it with exact integer sums);
//   epilogue: v = (sum * x_scale[m]) * w_scale[n] in fp32 BEFORE the rotation (the partner channel n ^ 64 with ITS scale), before
//   swiglu_fwd_elem (gate and up with the scales of their own rows of the packed [2 I, K] matrix) and before the residual; one rounding;
//   split-K, workgroup order, workspace layout and the reduction launch as in prefill.hip (prefill_plan's rule on K tiles of 128): no
//   atomics, no counters, the same inputs give the same bits on every run.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

constexpr int F8_BM = 64, F8_BN = 128, F8_BK = 128;
constexpr int F8_MMAX = 1024;
constexpr int F8_CUS = 256;                     // the launcher plans for the MI355X's 256 CUs (no device query, no state)
constexpr int F8_MAX_SPLIT = 16, F8_MIN_KTILES = 8;
constexpr int F8_CT_LD = F8_BN + 4;             // fp32 row pitch of the finished tile in LDS (16-B aligned rows)
enum { F8_PLAIN = 0, F8_ROPE = 1, F8_SWIGLU = 2 };

struct F8Args {
  const uint8_t* x; long long ldx; const float* xs;
  const uint8_t* W; long long ldw; const float* wsc;
  bf16_t* out; long long ldo, out_bs; int rpb;
  const bf16_t* res; long long ld_res;
  int M, N, K;                                   // N: W rows (2 I in the SwiGLU form)
  const float* rope_cos; const float* rope_sin; int rope_cols;
  float* ws; int split, sps;                     // sps: K tiles per slice
};

struct F8Plan { int mt, nt, split, sps, wgs; long long ws_bytes; };

// prefill.hip's rule: tiles x split >= 2 x cus where K allows, a slice keeps at least 8 K tiles (of 128 here)
inline F8Plan f8_plan(int M, int N, int K, int cus) {
  F8Plan p;
  p.mt = (M + F8_BM - 1) / F8_BM;
  p.nt = N / F8_BN;
  const int tiles = p.mt * p.nt, ktiles = K / F8_BK;
  p.split = 1;
  while (tiles * p.split < 2 * cus && p.split < F8_MAX_SPLIT && ktiles / (p.split * 2) >= F8_MIN_KTILES) p.split *= 2;
  p.sps = (ktiles + p.split - 1) / p.split;
  p.wgs = tiles * p.split;
  p.ws_bytes = p.split > 1 ? (long long)p.split * p.mt * F8_BM * N * 4 : 0;
  return p;
}

inline bool f8_shape_ok(int M, int N, int K) {
  return M >= 1 && M <= F8_MMAX && N >= F8_BN && N % F8_BN == 0 && K >= F8_BK && K % F8_BK == 0;
}

// workgroup id -> work item: XCD x (= id % 8) walks items [x * per, (x + 1) * per) in order; the remainder keeps its id
__device__ __forceinline__ int f8_item(int id, int total) {
  const int per = total >> 3;
  return id < per * 8 ? (id & 7) * per + (id >> 3) : id;
}

// W row (= output-scale index) of tile column c
template <int FORM>
__device__ __forceinline__ long long f8_wrow(int tn, int c, int N) {
  if (FORM == F8_SWIGLU) return c < 64 ? tn * 64 + c : (N >> 1) + tn * 64 + (c - 64);
  return tn * F8_BN + c;
}

// The epilogue of tile (tm, tn): sum8(ml, cl, f) yields the 8 finished fp32 code sums of tile row ml, tile columns cl .. cl + 7; they are
// scaled here, per row and per W row, in front of everything else.
template <int FORM, class L>
__device__ __forceinline__ void f8_epilogue(const F8Args& a, int tm, int tn, L sum8) {
  constexpr int CH = FORM == F8_SWIGLU ? 8 : 16;           // 8-column output chunks per tile row
  for (int e = threadIdx.x; e < F8_BM * CH; e += 256) {
    const int ml = e / CH, ch = e % CH, m = tm * F8_BM + ml;
    if (m >= a.M) continue;
    const float sx = a.xs[m];
    auto load8 = [&](int cl, float* f) {
      sum8(ml, cl, f);
      const float* sw = a.wsc + f8_wrow<FORM>(tn, cl, a.N);  // 8 columns from a multiple of 8 stay inside one half of a SwiGLU tile
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = (f[j] * sx) * sw[j];
    };
    float v[8];
    int ncol;
    if (FORM == F8_SWIGLU) {
      float gt[8], up[8];
      load8(ch * 8, gt);
      load8(64 + ch * 8, up);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = swiglu_fwd_elem(gt[j], up[j]);
      ncol = tn * 64 + ch * 8;
    } else {
      load8(ch * 8, v);
      ncol = tn * F8_BN + ch * 8;
      if (FORM == F8_ROPE && ncol < a.rope_cols) {
        // apply_rotary_pos_emb (modeling_llama.py:184-208) per head of 128: a' = a cos - b sin, b' = b cos + a sin, b = a's channel + 64
        float o[8];
        load8((ch * 8) ^ 64, o);
        const int d = (ch * 8) & 63, pos = m % a.rpb;
        const float* cp = a.rope_cos + (long long)pos * 64 + d;
        const float* sp = a.rope_sin + (long long)pos * 64 + d;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ch < 8 ? fmaf(v[j], cp[j], -(o[j] * sp[j])) : fmaf(v[j], cp[j], o[j] * sp[j]);
      }
      if (FORM == F8_PLAIN && a.res) {
        float r[8];
        unpack8(*(const u32x4_t*)(a.res + (long long)m * a.ld_res + ncol), r);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += r[j];
      }
    }
    *(u32x4_t*)(a.out + (long long)(m / a.rpb) * a.out_bs + (long long)(m % a.rpb) * a.ldo + ncol) = pack8(v);
  }
}

__device__ __forceinline__ i32x8_t f8_frag(const char* row, int off0, int off1) {
  const u32x4_t lo = *(const u32x4_t*)(row + off0), hi = *(const u32x4_t*)(row + off1);
  return i32x8_t{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

template <int FORM>
__global__ __launch_bounds__(256) void gemm_prefill_f8_kernel(const F8Args a) {
  constexpr int XB = F8_BM * F8_BK, WB = F8_BN * F8_BK, STAGE = XB + WB;               // 8 + 16 KiB per stage
  static_assert(F8_BM * F8_CT_LD * 4 <= 2 * STAGE, "the finished tile reuses the staging buffers");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int ntn = a.N / F8_BN, ntm = (a.M + F8_BM - 1) / F8_BM, tiles = ntm * ntn;
  const int item = f8_item(blockIdx.x, tiles * a.split);
  const int sp = item / tiles, t = item - sp * tiles, tn = t / ntm, tm = t - tn * ntm;
  const int ktiles = a.K / F8_BK;
  const int kt0 = sp * a.sps, kt1 = kt0 + a.sps < ktiles ? kt0 + a.sps : ktiles;
  // staging: thread -> 16-B chunk c of rows r0 + 32 j (x: j < 2, W: j < 4); (r >> 1) & 7 does not depend on j
  const int c = tid & 7, r0 = tid >> 3;
  const int sw = ((c ^ ((r0 >> 1) & 7)) << 4) + r0 * 128;
  const uint8_t* xp[2];
  bool xok[2];
  const uint8_t* wp[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = tm * F8_BM + r0 + 32 * j;
    xok[j] = m < a.M;
    xp[j] = a.x + (long long)(xok[j] ? m : 0) * a.ldx + c * 16;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) wp[j] = a.W + f8_wrow<FORM>(tn, r0 + 32 * j, a.N) * a.ldw + c * 16;
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  u32x4_t rx[2], rw[4];
  f32x4_t acc[2][4];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[nt][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#define F8_GLOAD(KT)                                                                           \
  {                                                                                            \
    const long long k = (long long)(KT) * F8_BK;  /* K % 128 == 0: every K tile is whole */    \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) rx[j] = xok[j] ? *(const u32x4_t*)(xp[j] + k) : zero; \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) rw[j] = *(const u32x4_t*)(wp[j] + k);        \
  }
#define F8_LSTORE(BUF)                                                                         \
  {                                                                                            \
    char* xs = smem + (BUF) * STAGE;                                                           \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) *(u32x4_t*)(xs + sw + j * 32 * 128) = rx[j]; \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) *(u32x4_t*)(xs + XB + sw + j * 32 * 128) = rw[j]; \
  }
  if (kt0 < kt1) {
    F8_GLOAD(kt0)
    F8_LSTORE(0)
  }
  __syncthreads();
  // a fragment row is 16 i + li: its swizzle (row >> 1) & 7 = (li >> 1) & 7; lane group g takes chunks 2 g and 2 g + 1 of the row
  const int fsw = (li >> 1) & 7;
  const int off0 = ((2 * g) ^ fsw) << 4, off1 = ((2 * g + 1) ^ fsw) << 4;
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;                // block-uniform
    if (more) F8_GLOAD(kt + 1)
    const char* xs = smem + buf * STAGE;
    const char* wsm = xs + XB;
    i32x8_t af[2], bfr[4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) af[nt] = f8_frag(wsm + (wave * 32 + nt * 16 + li) * 128, off0, off1);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) bfr[mb] = f8_frag(xs + (mb * 16 + li) * 128, off0, off1);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        acc[nt][mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[nt], bfr[mb], acc[nt][mb], 0, 0, 0, 0, 0, 0);
    if (more) F8_LSTORE(buf ^ 1)
    __syncthreads();
  }
#undef F8_GLOAD
#undef F8_LSTORE
  // D[n][m] of (nt, mb): W row 32 wave + 16 nt + 4 g + reg, x row 16 mb + li -> 4 consecutive tile columns per lane
  if (a.split > 1) {
    const long long mpad = (long long)ntm * F8_BM;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        *(f32x4_t*)(a.ws + ((long long)sp * mpad + tm * F8_BM + mb * 16 + li) * a.N + tn * F8_BN + wave * 32 + nt * 16 + g * 4) = acc[nt][mb];
    return;
  }
  float* ct = (float*)smem;                        // every wave is behind the loop's last barrier: the staging buffers are free
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) *(f32x4_t*)(ct + (mb * 16 + li) * F8_CT_LD + wave * 32 + nt * 16 + g * 4) = acc[nt][mb];
  __syncthreads();
  f8_epilogue<FORM>(a, tm, tn, [&](int ml, int cl, float* f) {
    const f32x4_t lo = *(const f32x4_t*)(ct + ml * F8_CT_LD + cl), hi = *(const f32x4_t*)(ct + ml * F8_CT_LD + cl + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
  });
}

// one workgroup per tile: the slices' partial tiles added in the order s = 0, 1, ..., then the scaled epilogue
template <int FORM>
__global__ __launch_bounds__(256) void gemm_prefill_f8_reduce_kernel(const F8Args a) {
  const int ntm = (a.M + F8_BM - 1) / F8_BM;
  const int tn = blockIdx.x / ntm, tm = blockIdx.x - tn * ntm;
  const long long slice = (long long)ntm * F8_BM * a.N;
  f8_epilogue<FORM>(a, tm, tn, [&](int ml, int cl, float* f) {
    const float* p = a.ws + (long long)(tm * F8_BM + ml) * a.N + tn * F8_BN + cl;
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

template <int FORM>
int f8_entry(const char* name, const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw, const float* w_scale,
             void* out, long long ldo, long long out_bs, int rpb, const void* res, long long ld_res, int M, int N, int K,
             const float* rope_cos, const float* rope_sin, int rope_cols, void* ws, size_t ws_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(xq && x_scale && Wq && w_scale && out, "%s: null pointer", name);
  MLA_CHECK_ARG(f8_shape_ok(M, N, K) && rpb >= 1, "%s: 1 <= M <= 1024, N %% 128 == 0, K %% 128 == 0 required (M %d, N %d, K %d)", name, M, N,
                K);
  MLA_CHECK_ARG(AL16(xq) && AL16(Wq) && AL16(out) && ldx % 16 == 0 && ldw % 16 == 0 && ldo % 8 == 0 && out_bs % 8 == 0 && ldx >= K &&
                    ldw >= K,
                "%s: xq / Wq / out rows must be 16-B aligned", name);
  MLA_CHECK_ARG(!res || (AL16(res) && ld_res % 8 == 0), "%s: residual rows must be 16-B aligned", name);
  if (FORM == F8_ROPE)
    MLA_CHECK_ARG(rope_cos && rope_sin && AL16(rope_cos) && AL16(rope_sin) && rope_cols > 0 && rope_cols % 128 == 0 && rope_cols <= N,
                  "%s: the RoPE epilogue needs both tables (16-B aligned) and rope_cols a multiple of 128 (head_dim 128) and <= N", name);
  const F8Plan p = f8_plan(M, N, K, F8_CUS);
  MLA_CHECK_ARG(p.split == 1 || (ws && AL16(ws) && (long long)ws_bytes >= p.ws_bytes),
                "%s: workspace of %lld bytes (16-B aligned) needed for split-K %d, got %lld", name, p.ws_bytes, p.split, (long long)ws_bytes);
  F8Args a;
  a.x = (const uint8_t*)xq; a.ldx = ldx; a.xs = x_scale; a.W = (const uint8_t*)Wq; a.ldw = ldw; a.wsc = w_scale;
  a.out = (bf16_t*)out; a.ldo = ldo; a.out_bs = out_bs; a.rpb = rpb;
  a.res = (const bf16_t*)res; a.ld_res = ld_res;
  a.M = M; a.N = N; a.K = K;
  a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.rope_cols = rope_cols;
  a.ws = (float*)ws; a.split = p.split; a.sps = p.sps;
  hipLaunchKernelGGL((gemm_prefill_f8_kernel<FORM>), dim3(p.wgs), dim3(256), 0, stream, a);
  if (p.split > 1) hipLaunchKernelGGL((gemm_prefill_f8_reduce_kernel<FORM>), dim3(p.mt * p.nt), dim3(256), 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  mla_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
  return (int)e;
}

}  // namespace

extern "C" int mla_gemm_prefill_f8_plan(int M, int N, int K, int cus, int* out4) {
  MLA_CHECK_ARG(out4, "mla_gemm_prefill_f8_plan: null pointer");
  MLA_CHECK_ARG(f8_shape_ok(M, N, K) && cus >= 1,
                "mla_gemm_prefill_f8_plan: 1 <= M <= 1024, N %% 128 == 0, K %% 128 == 0 required (M %d, N %d, K %d)", M, N, K);
  const F8Plan p = f8_plan(M, N, K, cus);
  out4[0] = F8_BM; out4[1] = F8_BN; out4[2] = p.split; out4[3] = p.wgs;
  return 0;
}

extern "C" long long mla_gemm_prefill_f8_ws_bytes(int M, int N, int K) {
  if (!f8_shape_ok(M, N, K)) {
    mla_set_error("mla_gemm_prefill_f8_ws_bytes: 1 <= M <= 1024, N %% 128 == 0, K %% 128 == 0 required (M %d, N %d, K %d)", M, N, K);
    return -1;
  }
  return f8_plan(M, N, K, F8_CUS).ws_bytes;
}

extern "C" int mla_gemm_prefill_f8(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw, const float* w_scale,
                                   void* out, long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual,
                                   long long ld_res, int M, int N, int K, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return f8_entry<F8_PLAIN>("mla_gemm_prefill_f8", xq, ldx, x_scale, Wq, ldw, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual,
                            ld_res, M, N, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8_qkv_rope(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw,
                                            const float* w_scale, void* out, long long ldo, long long out_batch_stride, int rows_per_batch,
                                            int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols, int head_dim,
                                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
  MLA_CHECK_ARG(head_dim == 128, "mla_gemm_prefill_f8_qkv_rope: head_dim must be 128 (got %d)", head_dim);
  return f8_entry<F8_ROPE>("mla_gemm_prefill_f8_qkv_rope", xq, ldx, x_scale, Wq, ldw, w_scale, out, ldo, out_batch_stride, rows_per_batch,
                           nullptr, 0, M, N, K, rope_cos, rope_sin, rope_cols, workspace, workspace_bytes, stream);
}

extern "C" int mla_gemm_prefill_f8_gateup_swiglu(const void* xq, long long ldx, const float* x_scale, const void* wgu_q, long long ldw,
                                                 const float* w_scale, void* act, long long ldo, long long out_batch_stride,
                                                 int rows_per_batch, int M, int I, int K, void* workspace, size_t workspace_bytes,
                                                 hipStream_t stream) {
  MLA_CHECK_ARG(I >= 64 && I % 64 == 0 && I <= (1 << 29), "mla_gemm_prefill_f8_gateup_swiglu: I %% 64 == 0 required (I %d)", I);
  return f8_entry<F8_SWIGLU>("mla_gemm_prefill_f8_gateup_swiglu", xq, ldx, x_scale, wgu_q, ldw, w_scale, act, ldo, out_batch_stride,
                             rows_per_batch, nullptr, 0, M, 2 * I, K, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}
