// Inference-side kernels (round 6; SURVEY 8f rank 2: predict_action_diff, models/mla/model_mla.py:592-775 +
// models/diffusion/gaussian_diffusion.py:608-688). The reference re-runs the WHOLE 548-token forward for each of the 8 DDIM steps
// although everything in front of the [t, x] tokens is identical in all of them. mla_amd/infer.py runs one prefill that keeps the packed
// post-RoPE q|k|v rows of every layer, then 8 passes over the 2 suffix rows per sample. Those passes are weight-streaming
// (13.5 GB of bf16 weights per pass, ~2.5 ms at HBM rate), not MFMA work:
//   mla_gemv_bf16      out[m, n] = sum_k x[m, k] W[n, k] (+ residual), M <= 8 rows: every W row is read once, 16 B per lane, non-temporal,
//                      one wave per row pair, 256 B per lane in flight; x lives in LDS as bf16; fp32 accumulation.
//   mla_attn_decode    R <= 8 new query rows per (sample, head) against the cached keys / values [0, S_kv - R + r]: scores -> LDS,
//                      softmax per query, P V with 4 key slices per block; head_dim 128.
//   mla_gemm_skinny_bf16  the gemv contract for 1 <= M <= 64 rows and any K: W straight into MFMA A operands, x rows as B operands, no
//                      staging; 8 waves split K per 16-row tile.
//   mla_attn_chunk     the decode contract for 1 <= R <= 64 rows and any S_kv: online softmax over 64-key tiles, MFMA QK^T / PV.
//   mla_gemm_suffix_bf16  plain-input projection for 1 <= M <= 256 rows of a batch of samples: the skinny kernel's fragments with 1 / 2 / 4
//                      W tiles per workgroup, per-sample cache slots and rotary positions read from a device array.
//   mla_attn_chunk_ragged  mla_attn_chunk with one key count per sample, read from a device array.
//   mla_attn_chunk_groups  mla_attn_chunk for G groups of R query rows that share ONE sample's prefix rows (N action chunks drawn for one
//                      observation): every group sees the prefix and, causally, its own rows only.
//   mla_gemv_w8 / mla_gemm_skinny_w8  the first two projection contracts over weight-only FP8: W is [N, K] OCP e4m3fn bytes with one fp32
//                      scale per row (mla_quant_fp8_rows writes both); same kernels, W8 = true: half the bytes per weight, decoded in
//                      registers (v_cvt_pk_f32_fp8 / v_cvt_scalef32_pk_bf16_fp8), fp32 sum over the UNSCALED codes, one multiply by the
//                      row scale behind the finished sum.
//   mla_gemm_suffix_w8  the third projection contract (1 <= M <= 256 plain rows, ragged / groups slot addressing) over the same FP8 weights:
//                      gemm_suffix_kernel with W8 = true -- the skinny W8 kernel's 64-wide K steps, wave split and summation order, so every
//                      64-row slice is bit for bit mla_gemm_skinny_w8's output; serves N action chunks per observation (SampleGroupsEps).
//   mla_attn_chunk_ragged_groups  mla_attn_chunk_groups for B samples, each with its own prefix length read from a device array;
//                      mla_gemm_suffix_bf16_pos / _w8_pos write its rows: the cache row and the rotary position come from two arrays
//                      (N action chunks for each of B observations, BatchedSampleGroupsEps).
//   mla_gemm_skinny_gateup_swiglu_bf16 / _w8  the skinny kernel on the packed gate|up matrix with SwiGLU in the epilogue: a workgroup's
//                      tile is 8 gate rows and their 8 up rows, out [M, I] = silu(gate) * up; bit for bit mla_swiglu_fwd of the plain
//                      form's [M, 2 I] rows, which never reach memory (suffix_operand="once").
//   mla_gemv_w4 / mla_gemm_skinny_w4 / mla_gemm_skinny_gateup_swiglu_w4 / mla_gemm_suffix_w4(_pos)  the same five contracts over weight-only
//                      OCP MXFP4 (e2m1 codes, one e8m0 scale byte per 32 k of a row; mla_quant_mxfp4_rows writes both): same kernels,
//                      WFmt = WF_W4 -- a quarter of the bf16 bytes per weight, decoded WITH the block scale in registers
//                      (v_cvt_scalef32_pk_f32_fp4 / v_cvt_scalef32_pk_bf16_fp4), exactly: no scale multiply behind the sum. The MFMA
//                      forms keep the W8 forms' K steps, wave split and summation order (suffix_mx="fp4").
// infer.py keeps gemv / decode for every shape they accept and uses the other two beyond (action chunks of 8..63 steps); the last two
// serve batched sampling (B observations with prompts of different lengths on one pass).
// All are HBM-bound by construction: algorithmic bytes = the weight matrix (gemv) / the K and V rows of the head (decode).
#include "common.h"
#include "attn_suffix_tile.h"

namespace {

constexpr int GEMV_MMAX = 8;
constexpr int GEMV_ROWS = 2;          // W rows per wave
constexpr int GEMV_UNR = 8;           // K steps (64 lanes x 16 B each) whose loads are all issued before the first use

// x: [M, K] bf16 rows (ldx); W: [N, K] bf16, k-contiguous (ldw); out row m lives at out + (m / rpb) * out_bs + (m % rpb) * ldo
// (rpb rows per sample: lets the q|k|v rows of the suffix land directly in the per-sample cache slots); residual addressed like x
// with ld_res. K % 8 == 0, 16-B aligned rows.
// A 7B projection is only 33-90 MB: the kernel lives for a few microseconds and what it reaches is decided by the bytes in flight
// (Little's law: ~8 TB/s x ~2 us of loaded latency = 16 MB chip-wide), not by a loop. Lane map: 64 lanes per W row (a wave reads 1 KiB
// of a row per instruction), GEMV_ROWS rows per wave, the loads of GEMV_UNR K steps issued back to back into registers
// (2 x 8 x 16 B = 256 B per lane in flight) before the first FMA, one wave per row pair so that N = 4096 already puts 2 048 waves on the
// chip. Measured on the 7B suffix pass (12.95 GB of weights): 64 lanes per row with 4 rows per wave and no explicit batching 7.3 ms;
// 16 lanes per row / 8 rows per wave (four times fewer waves) 10.4 ms; this form 4.9 ms, 10-17 us per 33 MB projection (requesting the
// first row pair's weights BEFORE the input staging, to hide the staging / fused-RMSNorm prologue, cost 224 registers and was slower:
// 22.9 vs 16.8 us); profiles/r6_infer_latency.txt.
// PRE: what happens to the input rows on their way into LDS (every workgroup does it for itself -- M x K elements, a few KB -- instead
// of a separate launch in front of every projection: a pass over the suffix rows is launch-gap-bound once the weights stream at HBM rate)
//   0  nothing          1  LlamaRMSNorm (modeling_llama.py:76-90, same arithmetic and cast order as rmsnorm_fwd_kernel)
//   2  SwiGLU: x is the packed gate|up row [2 K], the GEMV input is silu(gate) * up (swiglu_fwd_elem, common.h)
__device__ __forceinline__ void unpack8f(const u32x4_t v, float* f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[2 * j] = bflo(v[j]); f[2 * j + 1] = bfhi(v[j]); }
}
__device__ __forceinline__ u32x4_t pack8f(const float* f) {
  u32x4_t v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = pack2bf(f[2 * j], f[2 * j + 1]);
  return v;
}
// W8: the weight operand is OCP e4m3fn (one byte per element, ldw in elements = bytes) with one fp32 scale per W row. Every e4m3 value is
// a bf16 value, so decoding loses nothing; the scale multiplies the FINISHED fp32 sum (never a partial one), in front of the residual add /
// the rotation and the one bf16 rounding. 16 B per lane and load as in the bf16 form = 16 weights instead of 8: K % 16 == 0.
// W4: the weight operand is OCP MXFP4 -- e2m1 codes, two per byte (element 2 j in the low nibble of byte j; ldw in BYTES), with one e8m0
// scale byte per block of 32 consecutive k of a row (w_scale.p [N, ld]: byte = e + 127, the block's values are code * 2^e). Every e2m1
// value has at most two significant bits and the scale is a power of two within [2^-125, 2^125], so the decode WITH its scale
// (v_cvt_scalef32_pk_f32_fp4 / v_cvt_scalef32_pk_bf16_fp4) is exact in bf16: the kernels are the bf16 kernels on the dequantised matrix up
// to summation order, with no scale multiply behind the sum and no new rounding point. K % 32 == 0: blocks never cross a row's end.
enum WFmt { WF_BF16 = 0, WF_W8 = 1, WF_W4 = 2 };
struct w4_scales { const uint8_t* p; long long ld; };
template <WFmt F> struct welem { typedef bf16_t t; typedef const float* __restrict__ scale_t; };
template <> struct welem<WF_W8> { typedef uint8_t t; typedef const float* __restrict__ scale_t; typedef u32x4_t load_t; };
template <> struct welem<WF_W4> { typedef uint8_t t; typedef w4_scales scale_t; typedef u32x2_t load_t; };
// the scale of an e8m0 byte as the fp32 operand of the scaled conversions: 2^(byte - 127), bytes 1 .. 254
__device__ __forceinline__ float e8m0_to_f32(const uint8_t b) { return __builtin_bit_cast(float, (uint32_t)b << 23); }
// the 4 codes of one 32-bit word -> floats (v_cvt_pk_f32_fp8: bytes 0, 1 / bytes 2, 3)
__device__ __forceinline__ void fp8x4_to_f32(const uint32_t w, float* f) {
  const mla_f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  f[0] = lo[0]; f[1] = lo[1]; f[2] = hi[0]; f[3] = hi[1];
}
// 8 codes (two words) -> one bf16 MFMA fragment, element order = byte order (v_cvt_scalef32_pk_bf16_fp8 at scale 1: exact)
__device__ __forceinline__ u32x4_t fp8x8_to_bf16(const uint32_t w0, const uint32_t w1) {
  u32x4_t v;
  v[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  v[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  v[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  v[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return v;
}
// 8 e2m1 codes (one word, element order = nibble order from the low end) times the block scale -> one bf16 MFMA fragment
__device__ __forceinline__ u32x4_t fp4x8_to_bf16(const uint32_t w, const float scale) {
  u32x4_t v;
  v[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  v[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  v[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  v[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return v;
}
// the 8 codes of one word times the block scale -> floats (v_cvt_scalef32_pk_f32_fp4: byte 0 .. 3, low nibble first)
__device__ __forceinline__ void fp4x8_to_f32(const uint32_t w, const float scale, float* f) {
  const mla_f32x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 1);
  const mla_f32x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 3);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}
// half h (codes 8 h .. 8 h + 7) of a lane's 16 codes of a 64-wide K step -> the A fragment of one MFMA: W8 two words at scale 1, W4 one word
// at the block's scale
template <WFmt F>
__device__ __forceinline__ u32x4_t wq_frag(const typename welem<F>::load_t a, const int h, const float scale) {
  if constexpr (F == WF_W4) return fp4x8_to_bf16(a[h], scale);
  else return fp8x8_to_bf16(a[2 * h], a[2 * h + 1]);
}
// The W8 form of gemv_kernel's K loop for one wave's GEMV_ROWS rows: a lane's 16 B are the codes of k = 16 c .. 16 c + 15, i.e. the x chunks
// 2 c and 2 c + 1 of xs ([M][kc] chunks of 8 bf16); a K step is 64 lanes x 16 = 1024 weights. Same batching as the bf16 loop: the loads of
// GEMV_UNR steps are issued before the first use.
// W4: a lane's 16 B are the 32 codes of ONE scale block, k = 32 c .. 32 c + 31 = the x chunks 4 c .. 4 c + 3, decoded with the block's scale
// (its byte is fetched with the codes); a K step is 2048 weights, the bytes in flight per lane are the W8 form's.
template <int M, WFmt F>
__device__ __forceinline__ void gemv_wq_rows(const uint8_t* const* wr, const uint8_t* const* sr, const u32x4_t* xs, int kc, int lane,
                                             float (*acc)[M]) {
  constexpr int XC = F == WF_W4 ? 4 : 2;                // x chunks of 8 per lane and load
  const int kc16 = kc >> (F == WF_W4 ? 2 : 1);          // 16-B loads per row
  for (int s0 = 0; s0 < ((kc16 + 63) >> 6); s0 += GEMV_UNR) {
    u32x4_t w[GEMV_UNR][GEMV_ROWS];
    float sc[GEMV_UNR][GEMV_ROWS];
#pragma unroll
    for (int u = 0; u < GEMV_UNR; ++u) {
      const int c = (s0 + u) * 64 + lane;
#pragma unroll
      for (int r = 0; r < GEMV_ROWS; ++r) {
        w[u][r] = c < kc16 ? __builtin_nontemporal_load((const u32x4_t*)(wr[r] + c * 16)) : u32x4_t{0u, 0u, 0u, 0u};   // code 0 = +0
        if constexpr (F == WF_W4) sc[u][r] = c < kc16 ? e8m0_to_f32(sr[r][c]) : 1.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < GEMV_UNR; ++u) {
      const int c = (s0 + u) * 64 + lane;
      if ((s0 + u) * 64 < kc16) {                       // (wave-uniform: whole steps beyond K are skipped)
        const int cc = c < kc16 ? c : kc16 - 1;          // lanes past the end read valid chunks against their zero weights
        float wf[GEMV_ROWS][8 * XC];
#pragma unroll
        for (int r = 0; r < GEMV_ROWS; ++r)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if constexpr (F == WF_W4) fp4x8_to_f32(w[u][r][j], sc[u][r], &wf[r][8 * j]);
            else fp8x4_to_f32(w[u][r][j], &wf[r][4 * j]);
          }
#pragma unroll
        for (int m = 0; m < M; ++m) {
#pragma unroll
          for (int h = 0; h < XC; ++h) {
            const u32x4_t xv = xs[m * kc + XC * cc + h];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float xl = bflo(xv[j]), xh = bfhi(xv[j]);
#pragma unroll
              for (int r = 0; r < GEMV_ROWS; ++r)
                acc[r][m] = fmaf(wf[r][8 * h + 2 * j + 1], xh, fmaf(wf[r][8 * h + 2 * j], xl, acc[r][m]));
            }
          }
        }
      }
    }
  }
}
template <int M, int PRE, WFmt F>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16_t* __restrict__ x, long long ldx, const typename welem<F>::t* __restrict__ W,
                                                   long long ldw, typename welem<F>::scale_t w_scale, bf16_t* __restrict__ out, long long ldo,
                                                   long long out_bs, int rpb, const bf16_t* __restrict__ res, long long ld_res, int N, int K,
                                                   const bf16_t* __restrict__ pre_w, float eps, const float* __restrict__ rope_cos,
                                                   const float* __restrict__ rope_sin, int rope_cols) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int kc = K >> 3;
  u32x4_t* xs = (u32x4_t*)smem;                       // [M][K / 8] chunks of 8 bf16
  float* scratch = (float*)(smem + (size_t)M * K * 2);   // 16 floats behind the rows (block reductions of the fused RMSNorm)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sets = (N + GEMV_ROWS - 1) / GEMV_ROWS;
  const int steps = (kc + 63) >> 6;                   // K steps of 64 chunks
  // input rows -> LDS, four independent 16-B loads per thread in flight (one load per loop trip cost a dependent round trip each:
  // ~6 us in front of every projection)
  for (int i0 = threadIdx.x; i0 < M * kc; i0 += 256 * 4) {
    u32x4_t a[4], b2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = i0 + t * 256;
      const int ii = i < M * kc ? i : M * kc - 1;
      const int m = ii / kc, c = ii - m * kc;
      a[t] = *(const u32x4_t*)(x + (long long)m * ldx + c * 8);
      if (PRE == 2) b2[t] = *(const u32x4_t*)(x + (long long)m * ldx + K + c * 8);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = i0 + t * 256;
      if (i < M * kc) {
        if (PRE == 2) {
          float g[8], u[8], o[8];
          unpack8f(a[t], g);
          unpack8f(b2[t], u);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = swiglu_fwd_elem(g[j], u[j]);
          xs[i] = pack8f(o);
        } else {
          xs[i] = a[t];
        }
      }
    }
  }
  __syncthreads();
  if (PRE == 1) {
    float rstd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float ss = 0.f;
      for (int c = threadIdx.x; c < kc; c += 256) {
        float f[8];
        unpack8f(xs[m * kc + c], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
      }
      ss = block_sum(ss, scratch);
      rstd[m] = 1.0f / sqrtf(ss / (float)K + eps);
    }
    for (int c = threadIdx.x; c < kc; c += 256) {
      float wv[8];
      unpack8f(*(const u32x4_t*)(pre_w + c * 8), wv);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float f[8], o[8];
        unpack8f(xs[m * kc + c], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = wv[j] * bf2f(f2bf(f[j] * rstd[m]));
        xs[m * kc + c] = pack8f(o);
      }
    }
    __syncthreads();
  }
  for (int set = blockIdx.x * 4 + wave; set < sets; set += gridDim.x * 4) {
    // rows of this wave: a consecutive pair -- or, in the rotary columns [0, rope_cols) of a fused q|k|v projection, channel d of a head
    // and its rotation partner d + 64 (apply_rotary_pos_emb, modeling_llama.py:184-208), so that the epilogue can rotate them
    const bool rot = rope_cos != nullptr && set * GEMV_ROWS < rope_cols;
    const int n0 = rot ? (set >> 6) * 128 + (set & 63) : set * GEMV_ROWS;
    const int nstep = rot ? 64 : 1;
    float acc[GEMV_ROWS][M];
    const typename welem<F>::t* wr[GEMV_ROWS];
    const uint8_t* sr[GEMV_ROWS];                         // W4: the rows' scale bytes
#pragma unroll
    for (int r = 0; r < GEMV_ROWS; ++r) {
      wr[r] = W + (long long)(n0 + r * nstep < N ? n0 + r * nstep : N - 1) * ldw;
      if constexpr (F == WF_W4) sr[r] = w_scale.p + (long long)(n0 + r * nstep < N ? n0 + r * nstep : N - 1) * w_scale.ld;
      else sr[r] = nullptr;
#pragma unroll
      for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
    }
    if constexpr (F != WF_BF16) gemv_wq_rows<M, F>(wr, sr, xs, kc, lane, acc);
    else
    for (int s0 = 0; s0 < steps; s0 += GEMV_UNR) {
      u32x4_t w[GEMV_UNR][GEMV_ROWS];
#pragma unroll
      for (int u = 0; u < GEMV_UNR; ++u) {
        const int c = (s0 + u) * 64 + lane;
#pragma unroll
        for (int r = 0; r < GEMV_ROWS; ++r)
          w[u][r] = c < kc ? __builtin_nontemporal_load((const u32x4_t*)(wr[r] + c * 8)) : u32x4_t{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int u = 0; u < GEMV_UNR; ++u) {
        const int c = (s0 + u) * 64 + lane;
        if ((s0 + u) * 64 < kc) {                     // (wave-uniform: whole steps beyond K are skipped)
          const int cc = c < kc ? c : kc - 1;          // lanes past the end read a valid chunk against their zero weights
#pragma unroll
          for (int m = 0; m < M; ++m) {
            const u32x4_t xv = xs[m * kc + cc];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float xl = bflo(xv[j]), xh = bfhi(xv[j]);
#pragma unroll
              for (int r = 0; r < GEMV_ROWS; ++r) acc[r][m] = fmaf(bfhi(w[u][r][j]), xh, fmaf(bflo(w[u][r][j]), xl, acc[r][m]));
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < GEMV_ROWS; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[r][m] = wave_sum(acc[r][m]);
    if (lane < GEMV_ROWS * M) {
      const int r = lane / M, m = lane - r * M;
      if (n0 + r * nstep < N) {
        float v = 0.f, partner = 0.f;
#pragma unroll
        for (int rr = 0; rr < GEMV_ROWS; ++rr)
#pragma unroll
          for (int mm = 0; mm < M; ++mm) {
            v = (rr == r && mm == m) ? acc[rr][mm] : v;
            partner = (rr != r && mm == m) ? acc[rr][mm] : partner;
          }
        if constexpr (F == WF_W8) {
          v = __fmul_rn(v, w_scale[n0 + r * nstep]);
          if (rot) partner = __fmul_rn(partner, w_scale[n0 + (1 - r) * nstep]);
        }
        if (res) v += bf2f(res[(long long)m * ld_res + n0 + r * nstep]);
        if (rot) {
          // the arithmetic of rope_kernel (elementwise.hip) on the bf16-rounded projection: a' = a cos - b sin, b' = b cos + a sin
          const int d = n0 & 63, pos = m % rpb;                    // table row = the row's index inside its sample's block of new rows
          const float c = rope_cos[pos * 64 + d], sn = rope_sin[pos * 64 + d];
          const float me = bf2f(f2bf(v)), other = bf2f(f2bf(partner));
          v = r == 0 ? fmaf(me, c, -(other * sn)) : fmaf(me, c, other * sn);
        }
        out[(long long)(m / rpb) * out_bs + (long long)(m % rpb) * ldo + n0 + r * nstep] = f2bf(v);
      }
    }
  }
}

// One block per (sample, head): 4 waves. q rows: q + (b * bs + (S_kv - R + r) * ld) + h * 128 (the new rows are the LAST R rows of the
// cache); query r sees keys [0, S_kv - R + r]. scale applied to the scores; softmax in fp32; o: [B * R, H * 128] bf16.
// Both passes over the keys map 16 lanes to one key row (8 channels = 16 B per lane) and 16 keys to one block step, and issue the
// loads of DEC_U steps before the first use: the first version (one dependent 16-B load per step in the score loop, one 4-B load per
// key in the P V loop) took 110 us per call at S_kv = 547 -- 35 + 138 serial round trips -- against ~15 us of the head's 281 KB at the
// rate one CU streams.
constexpr int DEC_RMAX = 8;
constexpr int DEC_U = 6;
constexpr int DEC_NW = 8;                              // waves per block: 32 keys per block step
__global__ __launch_bounds__(64 * DEC_NW) void attn_decode_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                                  bf16_t* __restrict__ o, int H, int S_kv, int R, long long ld, long long bs,
                                                                  long long ld_o, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = (float*)smem;                            // [R][S_kv] scores -> probabilities
  float* part = sc + (size_t)R * S_kv;                 // [DEC_NW waves][R][128] partial outputs
  const int h = blockIdx.x % H, b = blockIdx.x / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bf16_t* kb = k + b * bs + h * 128;
  const bf16_t* vb = v + b * bs + h * 128;
  const bf16_t* qb = q + b * bs + (long long)(S_kv - R) * ld + h * 128;
  const int sub = lane & 15, kg = wave * 4 + (lane >> 4);
  constexpr int KSTEP = 4 * DEC_NW;
  // ---- scores
  float qf[DEC_RMAX][8];
#pragma unroll
  for (int r = 0; r < DEC_RMAX; ++r) {
    if (r < R) {
      const u32x4_t qv = *(const u32x4_t*)(qb + (long long)r * ld + sub * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) { qf[r][2 * j] = bflo(qv[j]); qf[r][2 * j + 1] = bfhi(qv[j]); }
    }
  }
  for (int j0 = 0; j0 < S_kv; j0 += KSTEP * DEC_U) {
    u32x4_t kv[DEC_U];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int j = j0 + u * KSTEP + kg;
      kv[u] = *(const u32x4_t*)(kb + (long long)(j < S_kv ? j : S_kv - 1) * ld + sub * 8);
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int j = j0 + u * KSTEP + kg;
      float kf[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { kf[2 * e] = bflo(kv[u][e]); kf[2 * e + 1] = bfhi(kv[u][e]); }
#pragma unroll
      for (int r = 0; r < DEC_RMAX; ++r) {
        if (r < R) {
          float s = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) s = fmaf(qf[r][e], kf[e], s);
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
          if (sub == 0 && j < S_kv) sc[r * S_kv + j] = (j <= S_kv - R + r) ? s * scale : -INFINITY;
        }
      }
    }
  }
  // the first batch of V rows is requested before the softmax: it depends on nothing computed here
  u32x4_t vv0[DEC_U];
#pragma unroll
  for (int u = 0; u < DEC_U; ++u) {
    const int j = u * KSTEP + kg;
    vv0[u] = *(const u32x4_t*)(vb + (long long)(j < S_kv ? j : S_kv - 1) * ld + sub * 8);
  }
  __syncthreads();
  // ---- softmax: wave w normalises queries w, w + DEC_NW
  for (int r = wave; r < R; r += DEC_NW) {
    float m = -INFINITY;
    for (int j = lane; j < S_kv; j += 64) m = fmaxf(m, sc[r * S_kv + j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < S_kv; j += 64) { const float e = __expf(sc[r * S_kv + j] - m); sc[r * S_kv + j] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int j = lane; j < S_kv; j += 64) sc[r * S_kv + j] = bf2f(f2bf(sc[r * S_kv + j] * inv));   // P feeds the P V product as bf16, like the flash kernel's
  }
  __syncthreads();
  // ---- P V: lane owns channels sub * 8 .. + 7 of the keys of its group
  float acc[DEC_RMAX][8];
#pragma unroll
  for (int r = 0; r < DEC_RMAX; ++r)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
  for (int j0 = 0; j0 < S_kv; j0 += KSTEP * DEC_U) {
    u32x4_t vv[DEC_U];
    if (j0 == 0) {
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) vv[u] = vv0[u];
    } else {
#pragma unroll
      for (int u = 0; u < DEC_U; ++u) {
        const int j = j0 + u * KSTEP + kg;
        vv[u] = *(const u32x4_t*)(vb + (long long)(j < S_kv ? j : S_kv - 1) * ld + sub * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int j = j0 + u * KSTEP + kg;
      if (j < S_kv) {
        float vf[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { vf[2 * e] = bflo(vv[u][e]); vf[2 * e + 1] = bfhi(vv[u][e]); }
#pragma unroll
        for (int r = 0; r < DEC_RMAX; ++r)
          if (r < R) {
            const float p = sc[r * S_kv + j];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[r][e] = fmaf(p, vf[e], acc[r][e]);
          }
      }
    }
  }
  // the four key groups of a wave first (lanes l, l ^ 16, l ^ 32, l ^ 48), then the waves through LDS
#pragma unroll
  for (int r = 0; r < DEC_RMAX; ++r)
    if (r < R) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = acc[r][e];
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        if (lane < 16) part[(wave * R + r) * 128 + sub * 8 + e] = a;
      }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < R * 128; i += 64 * DEC_NW) {
    const int r = i >> 7, c = i & 127;
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < DEC_NW; ++g) s += part[(g * R + r) * 128 + c];
    o[(long long)(b * R + r) * ld_o + h * 128 + c] = f2bf(s);
  }
}

// ---- skinny GEMM for 1 <= M <= 64 rows (the suffix pass of an action chunk of up to 63 rows): same contract as gemv_kernel.
// One workgroup per 16-row W tile, SK_NW waves splitting K into contiguous ranges of 32-wide steps; per step and lane one 16-B
// non-temporal load of W straight into the A fragment of v_mfma_f32_16x16x32_bf16 (lane l: W row l & 15, k = 8 (l >> 4) .. + 7) and one
// 16-B load of each 16-row block of x into the B fragment (x row l & 15 of the block, the same k), so every W byte is read once per pass
// and nothing of x is staged: LDS holds only the waves' partial tiles (fixed-order sum over the waves), the rstd of the fused RMSNorm and
// its reduction scratch, whatever K is. x is re-read once per tile from L2 (M / 16 times the W bytes).
// PRE 1 computes each row's rstd in a prologue in rmsnorm_fwd_kernel's exact order (256 "threads" x 8-element chunks, wave sums,
// wave partials summed in order), PRE 2 forms silu(gate) * up per element with swiglu_fwd_elem: the B fragments hold the same bf16
// values the separate kernels would write. In the rotary columns a tile is rows d .. d + 7 and d + 64 .. d + 71 of one head (d = 8 j),
// so that the epilogue holds both halves of every rotate-half pair.
constexpr int SK_MMAX = 64;
constexpr int SK_NW = 8;
// W8 (e4m3fn weights, see gemv_kernel): a lane's 16-B load is 16 codes, k = 64 s + 16 (l >> 4) .. + 15 of a 64-wide step, decoded to bf16 into
// the A fragments of TWO MFMAs (codes 0-7, then 8-15); the B fragments are the x elements of the same k, so the k order inside a step is a
// permutation of the bf16 form's -- the sum is the same set of products. The conversions do not depend on M. K % 16 == 0: a lane's chunk is
// inside K or beyond it as a whole.
// GU (mla_gemm_skinny_gateup_swiglu_*; PRE 0, no residual, no rotary columns): W is the packed gate|up matrix [2 N, K] and workgroup t
// owns gate rows 8 t .. 8 t + 7 and up rows N + 8 t .. N + 8 t + 7 as the 16 rows of its A fragment -- the rotary columns' device of
// holding both halves of a pair in one tile. The K loop is the same code; the epilogue sums both halves in the same wave order, rounds
// each to bf16 (what the plain form would store), applies swiglu_fwd_elem and stores out [M, N]: a weight row's sum depends only on
// the row, the K split and the order, so the result is swiglu_fwd of the plain form's output bit for bit, and the packed rows never
// reach memory.
template <int MB, int PRE, WFmt F, bool GU = false>
__global__ __launch_bounds__(64 * SK_NW) void gemm_skinny_kernel(const bf16_t* __restrict__ x, long long ldx, const typename welem<F>::t* __restrict__ W,
                                                                 long long ldw, typename welem<F>::scale_t w_scale, bf16_t* __restrict__ out,
                                                                 long long ldo, long long out_bs, int rpb,
                                                                 const bf16_t* __restrict__ res, long long ld_res, int M, int N, int K,
                                                                 const bf16_t* __restrict__ pre_w, float eps, const float* __restrict__ rope_cos,
                                                                 const float* __restrict__ rope_sin, int rope_cols) {
  constexpr int NB = MB * (PRE == 2 ? 2 : 1);                        // x loads per K step
  constexpr int U = NB <= 2 ? 8 : (NB <= 4 ? 4 : 2);                 // K steps whose loads are issued before the first MFMA
  __shared__ __attribute__((aligned(16))) float lds[SK_NW * MB * 256 + SK_MMAX + 32];   // ONE array: partial tiles | rstd | scratch
  float* rstd = lds + SK_NW * MB * 256;
  float* scr = rstd + SK_MMAX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  if (PRE == 1) {
    // two rows at a time per 8-row round (threads 0-255 and 256-511 each play rmsnorm_fwd_kernel's 256 threads on one row)
    const int half = threadIdx.x >> 8, vt = threadIdx.x & 255, kc = K >> 3;
    for (int m0 = 0; m0 < M; m0 += 8) {
      float ss[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = vt; c < kc; c += 256) {
        u32x4_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m0 + half + 2 * i;
          v[i] = *(const u32x4_t*)(x + (long long)(m < M ? m : M - 1) * ldx + c * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float f[8];
          unpack8f(v[i], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) ss[i] += f[j] * f[j];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) ss[i] = wave_sum(ss[i]);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) scr[(i * 2 + half) * 4 + (vt >> 6)] = ss[i];
      }
      __syncthreads();
      if (threadIdx.x < 8) {
        const int i = threadIdx.x >> 1, hh = threadIdx.x & 1, m = m0 + hh + 2 * i;
        if (m < M) {
          float r = 0.f;
          for (int w = 0; w < 4; ++w) r += scr[(i * 2 + hh) * 4 + w];
          rstd[m] = 1.0f / sqrtf(r / (float)K + eps);
        }
      }
      __syncthreads();
    }
  }
  const int tile = blockIdx.x;
  const bool rot = !GU && rope_cos != nullptr && tile * 16 < rope_cols;
  const int nrows = GU ? 2 * N : N;                                  // rows of W
  const int nrow = GU ? ((li & 8) ? N : 0) + tile * 8 + (li & 7)
                      : (rot ? (tile >> 3) * 128 + ((li & 8) ? 64 : 0) + (tile & 7) * 8 + (li & 7) : tile * 16 + li);
  const typename welem<F>::t* wr = W + (long long)(nrow < nrows ? nrow : nrows - 1) * ldw;
  const uint8_t* sr = nullptr;                                       // W4: the row's scale bytes
  if constexpr (F == WF_W4) sr = w_scale.p + (long long)(nrow < nrows ? nrow : nrows - 1) * w_scale.ld;
  const bf16_t* xr[MB];
  bool xok[MB];
  float xrs[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + li;
    xok[mb] = m < M;
    xr[mb] = x + (long long)(xok[mb] ? m : 0) * ldx;
    xrs[mb] = (PRE == 1 && xok[mb]) ? rstd[m] : 0.f;
  }
  const int steps = F != WF_BF16 ? (K + 63) >> 6 : (K + 31) >> 5, spw = (steps + SK_NW - 1) / SK_NW;
  const int s_beg = wave * spw, s_end = s_beg + spw < steps ? s_beg + spw : steps;
  f32x4_t acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  if constexpr (F != WF_BF16) {
    // the W loads of UW steps are issued first (the bytes in flight per lane of the bf16 form at MB <= 2), the x / norm-weight loads
    // (L2 hits, twice as many per W load as in the bf16 form) in rounds of UX steps behind them
    // W4: the same 64-wide step and lane map -- a lane's 16 codes are 8 B inside ONE scale block (k >> 5), whose byte is fetched with them
    constexpr int UW = 8, UX = NB <= 1 ? 8 : (NB <= 2 ? 4 : (NB <= 4 ? 2 : 1));
    typedef typename welem<F>::load_t wload_t;
    for (int s0 = s_beg; s0 < s_end; s0 += UW) {
      wload_t a[UW];
      float sc[UW];
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        const int k = (s0 + u) * 64 + g * 16;
        const bool ok = s0 + u < s_end && k < K;
        a[u] = ok ? __builtin_nontemporal_load((const wload_t*)(wr + (F == WF_W4 ? k >> 1 : k))) : wload_t{};   // code 0 = +0
        if constexpr (F == WF_W4) sc[u] = ok ? e8m0_to_f32(sr[k >> 5]) : 1.0f;
        else sc[u] = 1.0f;
      }
#pragma unroll
      for (int u0 = 0; u0 < UW; u0 += UX) {
        u32x4_t b[UX][2][NB], nw[UX][2];
#pragma unroll
        for (int u = 0; u < UX; ++u) {
          const int k = (s0 + u0 + u) * 64 + g * 16;
          const bool ok = s0 + u0 + u < s_end && k < K;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              b[u][h][mb] = ok && xok[mb] ? *(const u32x4_t*)(xr[mb] + k + 8 * h) : zero;
              if (PRE == 2) b[u][h][MB + mb] = ok && xok[mb] ? *(const u32x4_t*)(xr[mb] + K + k + 8 * h) : zero;
            }
            if (PRE == 1) nw[u][h] = ok ? *(const u32x4_t*)(pre_w + k + 8 * h) : zero;
          }
        }
#pragma unroll
        for (int u = 0; u < UX; ++u) {
          if (s0 + u0 + u < s_end) {                                   // wave-uniform
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const u32x4_t af = wq_frag<F>(a[u0 + u], h, sc[u0 + u]);
              float wv[8];
              if (PRE == 1) unpack8f(nw[u][h], wv);
#pragma unroll
              for (int mb = 0; mb < MB; ++mb) {
                u32x4_t bv = b[u][h][mb];
                if (PRE == 1) {
                  float f[8], o[8];
                  unpack8f(bv, f);
#pragma unroll
                  for (int j = 0; j < 8; ++j) o[j] = wv[j] * bf2f(f2bf(f[j] * xrs[mb]));
                  bv = pack8f(o);
                } else if (PRE == 2) {
                  float gg[8], uu[8], o[8];
                  unpack8f(bv, gg);
                  unpack8f(b[u][h][MB + mb], uu);
#pragma unroll
                  for (int j = 0; j < 8; ++j) o[j] = swiglu_fwd_elem(gg[j], uu[j]);
                  bv = pack8f(o);
                }
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af), as_frag(bv), acc[mb], 0, 0, 0);
              }
            }
          }
        }
      }
    }
  } else
  for (int s0 = s_beg; s0 < s_end; s0 += U) {
    u32x4_t a[U], b[U][NB], nw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = (s0 + u) * 32 + g * 8;
      const bool ok = s0 + u < s_end && k < K;
      a[u] = ok ? __builtin_nontemporal_load((const u32x4_t*)(wr + k)) : zero;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        b[u][mb] = ok && xok[mb] ? *(const u32x4_t*)(xr[mb] + k) : zero;
        if (PRE == 2) b[u][MB + mb] = ok && xok[mb] ? *(const u32x4_t*)(xr[mb] + K + k) : zero;
      }
      if (PRE == 1) nw[u] = ok ? *(const u32x4_t*)(pre_w + k) : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < s_end) {                                          // wave-uniform
        float wv[8];
        if (PRE == 1) unpack8f(nw[u], wv);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          u32x4_t bv = b[u][mb];
          if (PRE == 1) {
            float f[8], o[8];
            unpack8f(bv, f);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = wv[j] * bf2f(f2bf(f[j] * xrs[mb]));
            bv = pack8f(o);
          } else if (PRE == 2) {
            float gg[8], uu[8], o[8];
            unpack8f(bv, gg);
            unpack8f(b[u][MB + mb], uu);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = swiglu_fwd_elem(gg[j], uu[j]);
            bv = pack8f(o);
          }
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a[u]), as_frag(bv), acc[mb], 0, 0, 0);
        }
      }
    }
  }
  // partial tiles -> LDS; D[n][m] of block mb sits in lane (n >> 2) * 16 + (m & 15), register n & 3
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[((wave * MB + mb) * 4 + r) * 64 + lane] = acc[mb][r];
  __syncthreads();
  if constexpr (GU) {
    // tile row i = gate column n, tile row i + 8 = its up column; n fastest, so 8 threads store 16 contiguous bytes of a row
    for (int e = threadIdx.x; e < 8 * MB * 16; e += 64 * SK_NW) {
      const int i = e & 7, m = e >> 3, n = tile * 8 + i;
      if (m >= M || n >= N) continue;
      const int mb = m >> 4, col = m & 15, iu = i + 8;
      float gs = 0.f, us = 0.f;
#pragma unroll
      for (int w = 0; w < SK_NW; ++w) gs += lds[((w * MB + mb) * 4 + (i & 3)) * 64 + (i >> 2) * 16 + col];
#pragma unroll
      for (int w = 0; w < SK_NW; ++w) us += lds[((w * MB + mb) * 4 + (iu & 3)) * 64 + (iu >> 2) * 16 + col];
      if constexpr (F == WF_W8) {
        gs = __fmul_rn(gs, w_scale[n]);
        us = __fmul_rn(us, w_scale[N + n]);
      }
      out[(long long)m * ldo + n] = f2bf(swiglu_fwd_elem(bf2f(f2bf(gs)), bf2f(f2bf(us))));
    }
    return;
  }
  for (int e = threadIdx.x; e < 16 * MB * 16; e += 64 * SK_NW) {
    const int m = e % (MB * 16), i = e / (MB * 16);
    const int n = rot ? (tile >> 3) * 128 + ((i & 8) ? 64 : 0) + (tile & 7) * 8 + (i & 7) : tile * 16 + i;
    if (m >= M || n >= N) continue;
    const int mb = m >> 4, col = m & 15;
    float v = 0.f, partner = 0.f;
#pragma unroll
    for (int w = 0; w < SK_NW; ++w) v += lds[((w * MB + mb) * 4 + (i & 3)) * 64 + (i >> 2) * 16 + col];
    if constexpr (F == WF_W8) v = __fmul_rn(v, w_scale[n]);
    if (res) v += bf2f(res[(long long)m * ld_res + n]);
    if (rot) {
      const int ip = i ^ 8;
#pragma unroll
      for (int w = 0; w < SK_NW; ++w) partner += lds[((w * MB + mb) * 4 + (ip & 3)) * 64 + (ip >> 2) * 16 + col];
      if constexpr (F == WF_W8) partner = __fmul_rn(partner, w_scale[n ^ 64]);  // the rotation partner's row: d <-> d + 64 of the same head
      // gemv_kernel's epilogue: rope_kernel's arithmetic on the bf16-rounded projection
      const int d = n & 63, pos = m % rpb;
      const float c = rope_cos[pos * 64 + d], sn = rope_sin[pos * 64 + d];
      const float me = bf2f(f2bf(v)), other = bf2f(f2bf(partner));
      v = i < 8 ? fmaf(me, c, -(other * sn)) : fmaf(me, c, other * sn);
    }
    out[(long long)(m / rpb) * out_bs + (long long)(m % rpb) * ldo + n] = f2bf(v);
  }
}

// ---- suffix GEMM for 1 <= M <= 256 rows of a BATCH of samples (plain input: the batched pass forms RMSNorm / SwiGLU once per projection
// with the stand-alone kernels): gemm_skinny_kernel's fragments and K loop -- 8 waves split K, every wave holds the whole tile -- with
//   NT  16-row W tiles per workgroup (NT A fragments per K step: x is re-read from L2 once per NT * 16 W rows instead of once per 16),
//   MB  16-row x blocks (up to 16: 256 rows),
//   ragged addressing: row m is row p = m % rpb of sample b = m / rpb and goes to cache row slot[b] + p of that sample (out + b * out_bs +
//   (slot[b] + p) * ldo), rotated with table row slot[b] + p (or rope_pos[b] + p where the rotary position is not the cache row: the
//   groups of several samples, BatchedSampleGroupsEps); slot and rope_pos live on the device, so a captured graph serves any mix of prefix
//   lengths. Rows outside [0, cap_rows), and positions outside [0, rope_rows), are not written.
// Every W fragment is loaded by exactly one wave of one workgroup: each weight byte is requested once per call.
// NT = 1 (M <= 64) is gemm_skinny_kernel<MB, 0>'s arithmetic: the same K ranges per wave, the same MFMA order inside a wave, the same
// fixed-order sum over the 8 waves -> bit-identical outputs. The partial tiles go through LDS one W tile and at most 8 x blocks at a
// time (64 KiB at most).
// W8 (e4m3fn weights, see gemm_skinny_kernel): a 64-wide K step, a lane's 16-B load = the 16 codes k = 64 s + 16 (l >> 4) .. + 15 of every W tile,
// decoded at scale 1 into the A fragments of two MFMAs per tile (h = 0: codes 0-7, h = 1: codes 8-15) against the x elements at k + 8 h; an
// x load round holds at most 16 loads -- HX half steps of MX <= 8 blocks; at MB = 16 a half step takes two rounds of 8 blocks (32 registers:
// all 16 at once spilled; the decode of its A fragments is common to both rounds and compiled once: 16 conversions per 64 MFMAs of a
// K step in the gfx950 code) --, the W loads of UW steps are issued in front of them. Per accumulator the MFMA order is (s, h) ascending over gemm_skinny_kernel<MB, 0, true>'s K ranges, the
// waves are summed in its order and w_scale[n] multiplies the finished sum: every 64-row slice is bit for bit that kernel's output.
template <int NT, int MB, WFmt F>
__global__ __launch_bounds__(64 * SK_NW) void gemm_suffix_kernel(const bf16_t* __restrict__ x, long long ldx, const typename welem<F>::t* __restrict__ W,
                                                                 long long ldw, typename welem<F>::scale_t w_scale,
                                                                 bf16_t* __restrict__ out, long long ldo, long long out_bs, int rpb,
                                                                 const int* __restrict__ slot, int cap_rows, const bf16_t* __restrict__ res,
                                                                 long long ld_res, int M, int N, int K, const float* __restrict__ rope_cos,
                                                                 const float* __restrict__ rope_sin, int rope_cols,
                                                                 const int* __restrict__ rope_pos, int rope_rows) {
  constexpr int NL = NT + MB;                                          // 16-B loads per lane and K step
  constexpr int U = NL <= 3 ? 8 : (NL <= 5 ? 4 : (NL <= 10 ? 2 : 1));  // K steps whose loads are issued before the first MFMA
  constexpr int MG = MB < 8 ? MB : 8;                                  // x blocks per epilogue round
  static_assert(MB % MG == 0, "x blocks come in whole epilogue rounds");
  __shared__ __attribute__((aligned(16))) float lds[SK_NW * MG * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  const int tile0 = blockIdx.x * NT;
  const typename welem<F>::t* wr[NT];
  const uint8_t* sr[NT];                                               // W4: the rows' scale bytes
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int tile = tile0 + nt;
    const bool rot = rope_cos != nullptr && tile * 16 < rope_cols;
    const int nrow = rot ? (tile >> 3) * 128 + ((li & 8) ? 64 : 0) + (tile & 7) * 8 + (li & 7) : tile * 16 + li;
    wr[nt] = W + (long long)(nrow < N ? nrow : N - 1) * ldw;
    if constexpr (F == WF_W4) sr[nt] = w_scale.p + (long long)(nrow < N ? nrow : N - 1) * w_scale.ld;
    else sr[nt] = nullptr;
  }
  const bf16_t* xr[MB];
  bool xok[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + li;
    xok[mb] = m < M;
    xr[mb] = x + (long long)(xok[mb] ? m : 0) * ldx;
  }
  const int steps = F != WF_BF16 ? (K + 63) >> 6 : (K + 31) >> 5, spw = (steps + SK_NW - 1) / SK_NW;
  const int s_beg = wave * spw, s_end = s_beg + spw < steps ? s_beg + spw : steps;
  f32x4_t acc[NT][MB];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[nt][mb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  if constexpr (F != WF_BF16) {
    typedef typename welem<F>::load_t wload_t;                         // gemm_skinny_kernel's: 16 B (W8) / 8 B inside one scale block (W4)
    constexpr int UW = U;                                              // the bf16 form's W bytes in flight per lane
    constexpr int HX = MB <= 1 ? 16 : (MB <= 2 ? 8 : (MB <= 4 ? 4 : (MB <= 8 ? 2 : 1)));   // half steps per x load round: <= 16 loads
    constexpr int MX = MB <= 8 ? MB : 8;                               // x blocks per load round (16 blocks: two rounds per half step)
    static_assert((2 * UW) % HX == 0 && HX <= 2 * UW && MB % MX == 0, "x load rounds tile the W batch");
    for (int s0 = s_beg; s0 < s_end; s0 += UW) {
      wload_t a[UW][NT];
      float sc[UW][NT];                                                // W4: the block's scale, fetched with the codes
#pragma unroll
      for (int u = 0; u < UW; ++u) {
        const int k = (s0 + u) * 64 + g * 16;
        const bool ok = s0 + u < s_end && k < K;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          a[u][nt] = ok ? __builtin_nontemporal_load((const wload_t*)(wr[nt] + (F == WF_W4 ? k >> 1 : k))) : wload_t{};   // code 0 = +0
          if constexpr (F == WF_W4) sc[u][nt] = ok ? e8m0_to_f32(sr[nt][k >> 5]) : 1.0f;
          else sc[u][nt] = 1.0f;
        }
      }
#pragma unroll
      for (int q0 = 0; q0 < 2 * UW; q0 += HX) {
#pragma unroll
        for (int m0 = 0; m0 < MB; m0 += MX) {
          u32x4_t b[HX][MX];
#pragma unroll
          for (int j = 0; j < HX; ++j) {
            const int u = (q0 + j) >> 1, h = (q0 + j) & 1;
            const int k = (s0 + u) * 64 + g * 16;
            const bool ok = s0 + u < s_end && k < K;
#pragma unroll
            for (int mb = 0; mb < MX; ++mb) b[j][mb] = ok && xok[m0 + mb] ? *(const u32x4_t*)(xr[m0 + mb] + k + 8 * h) : zero;
          }
#pragma unroll
          for (int j = 0; j < HX; ++j) {
            const int u = (q0 + j) >> 1, h = (q0 + j) & 1;
            if (s0 + u < s_end) {                                      // wave-uniform
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) {
                const u32x4_t af = wq_frag<F>(a[u][nt], h, sc[u][nt]);
#pragma unroll
                for (int mb = 0; mb < MX; ++mb)
                  acc[nt][m0 + mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af), as_frag(b[j][mb]), acc[nt][m0 + mb], 0, 0, 0);
              }
            }
          }
        }
      }
    }
  } else
  for (int s0 = s_beg; s0 < s_end; s0 += U) {
    u32x4_t a[U][NT], b[U][MB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = (s0 + u) * 32 + g * 8;
      const bool ok = s0 + u < s_end && k < K;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) a[u][nt] = ok ? __builtin_nontemporal_load((const u32x4_t*)(wr[nt] + k)) : zero;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) b[u][mb] = ok && xok[mb] ? *(const u32x4_t*)(xr[mb] + k) : zero;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < s_end) {                                            // wave-uniform
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
            acc[nt][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a[u][nt]), as_frag(b[u][mb]), acc[nt][mb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int tile = tile0 + nt;
    const bool rot = rope_cos != nullptr && tile * 16 < rope_cols;
#pragma unroll
    for (int mg = 0; mg < MB; mg += MG) {
      // partial tiles of W tile nt, x blocks mg .. mg + MG - 1 -> LDS; D[n][m] of a block sits in lane (n >> 2) * 16 + (m & 15), register n & 3
#pragma unroll
      for (int mb = 0; mb < MG; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[((wave * MG + mb) * 4 + r) * 64 + lane] = acc[nt][mg + mb][r];
      __syncthreads();
      for (int e = threadIdx.x; e < 16 * MG * 16; e += 64 * SK_NW) {
        const int ml = e % (MG * 16), i = e / (MG * 16);
        const int m = mg * 16 + ml;
        const int n = rot ? (tile >> 3) * 128 + ((i & 8) ? 64 : 0) + (tile & 7) * 8 + (i & 7) : tile * 16 + i;
        if (m >= M || n >= N) continue;
        const int mb = ml >> 4, col = ml & 15;
        const int sb = m / rpb, p = m - sb * rpb;
        const int row = (slot ? slot[sb] : 0) + p;
        if (row < 0 || row >= cap_rows) continue;
        // rope_pos (the _pos entry points): the table row is rope_pos[sb] + p instead of the cache row -- several groups of suffix rows
        // behind one prefix sit at different rows but share their positions; a position outside the tables writes nothing
        const int pos = rope_pos ? rope_pos[sb] + p : row;
        if (rope_pos && (pos < 0 || pos >= rope_rows)) continue;
        float v = 0.f, partner = 0.f;
#pragma unroll
        for (int w = 0; w < SK_NW; ++w) v += lds[((w * MG + mb) * 4 + (i & 3)) * 64 + (i >> 2) * 16 + col];
        if constexpr (F == WF_W8) v = __fmul_rn(v, w_scale[n]);
        if (res) v += bf2f(res[(long long)m * ld_res + n]);
        if (rot) {
          const int ip = i ^ 8;
#pragma unroll
          for (int w = 0; w < SK_NW; ++w) partner += lds[((w * MG + mb) * 4 + (ip & 3)) * 64 + (ip >> 2) * 16 + col];
          if constexpr (F == WF_W8) partner = __fmul_rn(partner, w_scale[n ^ 64]);   // the rotation partner's row: d <-> d + 64 of the same head
          // gemv_kernel's epilogue: rope_kernel's arithmetic on the bf16-rounded projection, at the row's position in its sample
          const int d = n & 63;
          const float c = rope_cos[(long long)pos * 64 + d], sn = rope_sin[(long long)pos * 64 + d];
          const float me = bf2f(f2bf(v)), other = bf2f(f2bf(partner));
          v = i < 8 ? fmaf(me, c, -(other * sn)) : fmaf(me, c, other * sn);
        }
        out[(long long)sb * out_bs + (long long)row * ldo + n] = f2bf(v);
      }
      if (nt + 1 < NT || mg + MG < MB) __syncthreads();
    }
  }
}

// ---- suffix attention for 1 <= R <= 64 query rows: one workgroup per (sample, head, block of 16 queries), SUF_NW waves taking the key
// tiles of 64 in turn: tile t on wave t % 4 in iteration t / 4. The tile step, the fragment layout and the fixed-order merge of the
// waves' states are attn_suffix_tile.h's.
// RAGGED (mla_attn_chunk_ragged): the sample's key count comes from kv_len[b] on the device (clamped to [R, S_cap], the rows the caller owns)
// instead of the launch argument; everything behind that line is the same code, so a sample's output is the B = 1 launch's bit for bit
// (the waves' tile assignment starts at key 0 either way), and a captured graph serves any mix of lengths.
template <bool RAGGED>
__global__ __launch_bounds__(64 * SUF_NW) void attn_chunk_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                                bf16_t* __restrict__ o, int H, int S_kv, int R, long long ld, long long bs,
                                                                long long ld_o, float scale, const int* __restrict__ kv_len) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int QB = (R + 15) >> 4;
  const int qb = blockIdx.x % QB, bh = blockIdx.x / QB, h = bh % H, b = bh / H;
  if (RAGGED) {
    const int n = kv_len[b];
    S_kv = n < R ? R : (n > S_kv ? S_kv : n);                            // S_kv arrives as the capacity S_cap
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  bf16_t* vt = (bf16_t*)smem + wave * 128 * SUF_VP;                   // this wave's V tile, transposed
  const bf16_t* kb = k + b * bs + h * 128;
  const bf16_t* vb = v + b * bs + h * 128;
  const int r = qb * 16 + li;
  const bool qok = r < R;
  const int qpos = S_kv - R + (qok ? r : R - 1);                       // last key this query sees (padding queries: the last row's)
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  bf16x8_t qf[4];
  {
    const bf16_t* qr = q + b * bs + (long long)(S_kv - R + (qok ? r : 0)) * ld + h * 128;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) qf[ds] = as_frag(qok ? *(const u32x4_t*)(qr + ds * 32 + g * 8) : zero);
  }
  const float sc2 = scale * 1.4426950408889634f;
  f32x4_t ot[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ot[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int ntiles = (S_kv + 63) >> 6, iters = (ntiles + SUF_NW - 1) / SUF_NW;
  for (int it = 0; it < iters; ++it) {                                  // same trip count in every wave: the barriers below are uniform
    const int j0 = (it * SUF_NW + wave) * 64;                           // beyond S_kv: clamped loads, every score masked
    u32x4_t kf[4][4], vv[16];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int j = j0 + f * 16 + li;
      const bf16_t* kr = kb + (long long)(j < S_kv ? j : S_kv - 1) * ld + g * 8;
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) kf[f][ds] = *(const u32x4_t*)(kr + ds * 32);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int j = j0 + u * 4 + g;
      vv[u] = *(const u32x4_t*)(vb + (long long)(j < S_kv ? j : S_kv - 1) * ld + li * 8);
    }
    f32x4_t st[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      st[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) st[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(kf[f][ds]), qf[ds], st[f], 0, 0, 0);
    }
    // S^T[key][query]: lane holds query li, keys j0 + 16 f + 4 g + reg; key j visible iff j <= qpos (< S_kv)
    float mx = -INFINITY;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        if (j0 + f * 16 + g * 4 + rr > qpos) st[f][rr] = -INFINITY;
        mx = fmaxf(mx, st[f][rr]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mnew = fmaxf(m, mx * sc2);
    const float msafe = mnew == -INFINITY ? 0.f : mnew;
    const float alpha = __builtin_amdgcn_exp2f(m - msafe);
    float ps = 0.f;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        st[f][rr] = __builtin_amdgcn_exp2f(fmaf(st[f][rr], sc2, -msafe));
        ps += st[f][rr];
      }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mnew;
#pragma unroll
    for (int i = 0; i < 8; ++i) ot[i] *= alpha;
    const bf16x8_t pf0 = pack_pfrag(st[0], st[1]), pf1 = pack_pfrag(st[2], st[3]);
    // V tile -> LDS transposed (lane: key 4 u + g, channels 8 li .. + 7)
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vt[(li * 8 + 2 * e) * SUF_VP + u * 4 + g] = (bf16_t)(vv[u][e] & 0xffffu);
        vt[(li * 8 + 2 * e + 1) * SUF_VP + u * 4 + g] = (bf16_t)(vv[u][e] >> 16);
      }
    __syncthreads();
#pragma unroll
    for (int fd = 0; fd < 8; ++fd) {
      const bf16_t* vr = vt + (fd * 16 + li) * SUF_VP + g * 4;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x2_t lo = *(const u32x2_t*)(vr + ks * 32), hi = *(const u32x2_t*)(vr + ks * 32 + 16);
        const u32x4_t av = {lo[0], lo[1], hi[0], hi[1]};
        ot[fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(av), ks ? pf1 : pf0, ot[fd], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  float* mo = (float*)smem;                                             // [SUF_NW][128][16]
  float* ml = mo + SUF_NW * 128 * 16;                                   // [SUF_NW][16] max, then [SUF_NW][16] sum
#pragma unroll
  for (int fd = 0; fd < 8; ++fd)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) mo[(wave * 128 + fd * 16 + g * 4 + rr) * 16 + li] = ot[fd][rr];
  if (g == 0) { ml[wave * 16 + li] = m; ml[SUF_NW * 16 + wave * 16 + li] = l; }
  __syncthreads();
  for (int e = threadIdx.x; e < 128 * 16; e += 64 * SUF_NW) {
    const int qq = e & 15, d = e >> 4, rq = qb * 16 + qq;
    if (rq >= R) continue;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < SUF_NW; ++w) mm = fmaxf(mm, ml[w * 16 + qq]);    // finite: wave 0's first tile holds key 0, seen by every query
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < SUF_NW; ++w) {
      const float fw = __builtin_amdgcn_exp2f(ml[w * 16 + qq] - mm);
      L += fw * ml[SUF_NW * 16 + w * 16 + qq];
      O += fw * mo[(w * 128 + d) * 16 + qq];
    }
    o[(long long)(b * R + rq) * ld_o + h * 128 + d] = f2bf(O / L);
  }
}

// ---- suffix attention for G groups of R query rows on ONE sample's cache (mla_attn_chunk_groups): rows [0, S_p) are the prefix every
// group sees, row S_p + g R + p is suffix row p of group g. Query (g, p) sees the logical keys 0 .. S_p + p; logical key j is memory row
// j (j < S_p) or j + g R (the group's own rows). attn_chunk_kernel's arithmetic over the logical key sequence of every group -- tiles of
// 64 logical keys from key 0, tile t on wave t % 4 in iteration t / 4, the same online softmax, P rounding and fixed-order merge -- so
// group g's rows are bit for bit mla_attn_chunk (B = 1, S_kv = S_p + R) on cat(cache[:S_p], cache[S_p + g R : S_p + (g + 1) R]).
// One workgroup serves one head, one block of 16 query rows and GW groups: a tile that lies wholly inside the prefix (64 (t + 1) <= S_p)
// has its K fragments loaded and its V tile transposed into LDS ONCE for the GW query blocks (state per block: qf 16, ot 32, m, l
// registers); tiles that hold logical keys >= S_p are loaded per group. Masked-key and padding loads clamp to the last logical key of
// the query's OWN group, so no output depends on another group's rows. Groups beyond G (G % GW != 0) recompute group G - 1 and store nothing.
constexpr int ATTN_GROUPS_GW = 1;                                      // groups per workgroup mla_attn_chunk_groups launches
constexpr int ATTN_GROUPS_XCD_CHUNKS = 0;                              // its work order: 0 as dispatched, 1 one chunk of the grid per XCD
// RAGGED (mla_attn_chunk_ragged_groups): B samples of G groups each, [B, S_cap, 3H] with sample stride bs; the work order gets the sample
// as its slowest index and S_p comes from prefix_len[b] on the device, clamped to [0, S_cap - G R] (the rows the caller owns). One
// workgroup serves one sample, so the clamped S_p -- and with it the trip count, the barrier count and `shared` -- is the same in every
// wave (readfirstlane keeps it in a scalar register). Everything behind that line is the same code: sample b's rows are bit for bit the
// plain launch on its slice with S_p = S_p[b], the grid does not depend on the lengths and a captured graph serves any mix of them.
template <int GW, bool RAGGED>
__global__ __launch_bounds__(64 * SUF_NW) void attn_chunk_groups_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                       const bf16_t* __restrict__ v, bf16_t* __restrict__ o, int G, int H,
                                                                       int S_p, int R, long long ld, long long ld_o, float scale, int xcd_chunks,
                                                                       const int* __restrict__ prefix_len, int S_cap, long long bs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int QB = (R + 15) >> 4, NGB = (G + GW - 1) / GW;
  // head-major work order: the workgroups of one head (its 2 S_p x 128 prefix K / V elements) are neighbours. Blocks are dealt out
  // round-robin over the 8 XCDs (observed, not a contract: only speed depends on it), so with xcd_chunks (host: grid % 8 == 0) block b
  // takes work item (b % 8) * (grid / 8) + b / 8 -- a bijection -- and the neighbours share one XCD's L2 instead of eight.
  const int bid = xcd_chunks ? (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int qb = bid % QB, gb = (bid / QB) % NGB, h = RAGGED ? (bid / (QB * NGB)) % H : bid / (QB * NGB);
  const int b = RAGGED ? bid / (QB * NGB * H) : 0;
  if (RAGGED) {
    const int n = prefix_len[b], room = S_cap - G * R;                  // host: room >= 0
    S_p = __builtin_amdgcn_readfirstlane(n < 0 ? 0 : (n > room ? room : n));
    q += b * bs; k += b * bs; v += b * bs;
  }
  const int S_kv = S_p + R;                                             // logical keys of a group
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  bf16_t* vt = (bf16_t*)smem + wave * 128 * SUF_VP;
  const bf16_t* kb = k + h * 128;
  const bf16_t* vb = v + h * 128;
  const int r = qb * 16 + li;
  const bool qok = r < R;
  const int qpos = S_kv - R + (qok ? r : R - 1);
  const u32x4_t zero = {0u, 0u, 0u, 0u};
  int goff[GW];                                                         // memory row of logical key j >= S_p: j + goff
  bf16x8_t qf[GW][4];
#pragma unroll
  for (int gi = 0; gi < GW; ++gi) {
    const int gg = gb * GW + gi;
    goff[gi] = (gg < G ? gg : G - 1) * R;
    const bf16_t* qr = q + (long long)(S_p + goff[gi] + (qok ? r : 0)) * ld + h * 128;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) qf[gi][ds] = as_frag(qok ? *(const u32x4_t*)(qr + ds * 32 + g * 8) : zero);
  }
  const float sc2 = scale * 1.4426950408889634f;
  f32x4_t ot[GW][8];
  float m[GW], l[GW];
#pragma unroll
  for (int gi = 0; gi < GW; ++gi) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ot[gi][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    m[gi] = -INFINITY;
    l[gi] = 0.f;
  }
  const int ntiles = (S_kv + 63) >> 6, iters = (ntiles + SUF_NW - 1) / SUF_NW;
  for (int it = 0; it < iters; ++it) {                                  // same trip count and barrier count in every wave
    const int j0 = (it * SUF_NW + wave) * 64;
    const bool shared = j0 + 64 <= S_p;                                 // wave-uniform: the tile holds prefix rows only
    u32x4_t kf[4][4];
#pragma unroll
    for (int gi = 0; gi < GW; ++gi) {
      const bool fresh = gi == 0 || !shared;                            // load K / V and rebuild the V tile, or reuse group 0's
      u32x4_t vv[16];
      if (fresh) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const int j = j0 + f * 16 + li, jc = j < S_kv ? j : S_kv - 1;
          const bf16_t* kr = kb + (long long)(jc < S_p ? jc : jc + goff[gi]) * ld + g * 8;
#pragma unroll
          for (int ds = 0; ds < 4; ++ds) kf[f][ds] = *(const u32x4_t*)(kr + ds * 32);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int j = j0 + u * 4 + g, jc = j < S_kv ? j : S_kv - 1;
          vv[u] = *(const u32x4_t*)(vb + (long long)(jc < S_p ? jc : jc + goff[gi]) * ld + li * 8);
        }
      }
      f32x4_t st[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        st[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) st[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(kf[f][ds]), qf[gi][ds], st[f], 0, 0, 0);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          if (j0 + f * 16 + g * 4 + rr > qpos) st[f][rr] = -INFINITY;
          mx = fmaxf(mx, st[f][rr]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m[gi], mx * sc2);
      const float msafe = mnew == -INFINITY ? 0.f : mnew;
      const float alpha = __builtin_amdgcn_exp2f(m[gi] - msafe);
      float ps = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          st[f][rr] = __builtin_amdgcn_exp2f(fmaf(st[f][rr], sc2, -msafe));
          ps += st[f][rr];
        }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l[gi] = l[gi] * alpha + ps;
      m[gi] = mnew;
#pragma unroll
      for (int i = 0; i < 8; ++i) ot[gi][i] *= alpha;
      const bf16x8_t pf0 = pack_pfrag(st[0], st[1]), pf1 = pack_pfrag(st[2], st[3]);
      if (fresh) {
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            vt[(li * 8 + 2 * e) * SUF_VP + u * 4 + g] = (bf16_t)(vv[u][e] & 0xffffu);
            vt[(li * 8 + 2 * e + 1) * SUF_VP + u * 4 + g] = (bf16_t)(vv[u][e] >> 16);
          }
      }
      __syncthreads();
#pragma unroll
      for (int fd = 0; fd < 8; ++fd) {
        const bf16_t* vr = vt + (fd * 16 + li) * SUF_VP + g * 4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const u32x2_t lo = *(const u32x2_t*)(vr + ks * 32), hi = *(const u32x2_t*)(vr + ks * 32 + 16);
          const u32x4_t av = {lo[0], lo[1], hi[0], hi[1]};
          ot[gi][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(av), ks ? pf1 : pf0, ot[gi][fd], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  // attn_chunk_kernel's merge, one group after the other through the same buffers
  float* mo = (float*)smem;                                             // [SUF_NW][128][16]
  float* ml = mo + SUF_NW * 128 * 16;                                   // [SUF_NW][16] max, then [SUF_NW][16] sum
#pragma unroll
  for (int gi = 0; gi < GW; ++gi) {
    const int gg = gb * GW + gi;
#pragma unroll
    for (int fd = 0; fd < 8; ++fd)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) mo[(wave * 128 + fd * 16 + g * 4 + rr) * 16 + li] = ot[gi][fd][rr];
    if (g == 0) { ml[wave * 16 + li] = m[gi]; ml[SUF_NW * 16 + wave * 16 + li] = l[gi]; }
    __syncthreads();
    for (int e = threadIdx.x; e < 128 * 16; e += 64 * SUF_NW) {
      const int qq = e & 15, d = e >> 4, rq = qb * 16 + qq;
      if (rq >= R || gg >= G) continue;
      float mm = -INFINITY;
#pragma unroll
      for (int w = 0; w < SUF_NW; ++w) mm = fmaxf(mm, ml[w * 16 + qq]);
      float L = 0.f, O = 0.f;
#pragma unroll
      for (int w = 0; w < SUF_NW; ++w) {
        const float fw = __builtin_amdgcn_exp2f(ml[w * 16 + qq] - mm);
        L += fw * ml[SUF_NW * 16 + w * 16 + qq];
        O += fw * mo[(w * 128 + d) * 16 + qq];
      }
      o[(long long)((b * G + gg) * R + rq) * ld_o + h * 128 + d] = f2bf(O / L);
    }
    if (gi + 1 < GW) __syncthreads();
  }
}

// ---- weight quantiser for the W8 projections: one workgroup per row of W [N, K] bf16.
//   amax = max_k |W[n, k]|;  scale[n] = amax / 448 (1 when the row is all zero);  q[n, k] = e4m3fn_rne(clamp(W[n, k] / scale[n], -448, 448))
// Both divisions are IEEE fp32 divisions (__fdiv_rn: no v_rcp, no multiply by a reciprocal), so that
// (W.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn) on the CPU gives the same bytes. The clamp is in front of the
// conversion: v_cvt_pk_fp8_f32 never sees a value beyond 448, so no NaN code can come out of finite input. Non-finite input is not
// supported. Two passes over the row (the second one hits L2); fixed-order max, no atomics, no workspace.
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const bf16_t* __restrict__ W, long long ldw, uint8_t* __restrict__ q, long long ldq,
                                                             float* __restrict__ scale, int K) {
  __shared__ float scratch[16];
  const bf16_t* wr = W + (long long)blockIdx.x * ldw;
  uint8_t* qr = q + (long long)blockIdx.x * ldq;
  const int kc16 = K >> 4;
  float amax = 0.f;
  for (int c = threadIdx.x; c < kc16; c += 256) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float f[8];
      unpack8f(*(const u32x4_t*)(wr + c * 16 + h * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
    }
  }
  amax = block_max(amax, scratch);
  const float s = amax == 0.f ? 1.0f : __fdiv_rn(amax, 448.0f);
  if (threadIdx.x == 0) scale[blockIdx.x] = s;
  for (int c = threadIdx.x; c < kc16; c += 256) {
    u32x4_t o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float f[8];
      unpack8f(*(const u32x4_t*)(wr + c * 16 + h * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = fminf(fmaxf(__fdiv_rn(f[j], s), -448.0f), 448.0f);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * j], f[4 * j + 1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * j + 2], f[4 * j + 3], w, true);
        o[2 * h + j] = (uint32_t)w;
      }
    }
    *(u32x4_t*)(qr + c * 16) = o;
  }
}

// ---- weight quantiser for the W4 projections (OCP MXFP4): one workgroup per row of W [N, K] bf16, one thread per block of 32 elements
// (64 B in, 16 B of codes + one scale byte out). Everything is integer work on the bf16 bits or an exact fp32 product, so the CPU
// statement gives the same bytes:
//   amax = the block's largest |w|, E = its exponent field - 127;  e = clamp(E - 2, -125, 125);  scale byte = e + 127
//   code = sign | index of round-to-nearest(|w| / 2^e) on {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even mantissa bit, saturating at 6
// |w| * 2^-e is exact in fp32 (a power-of-two factor; what underflows is far below the first threshold 0.25). An all-zero block gives
// byte 127 and codes +0. Non-finite input is not supported. No reduction across threads, no atomics: two runs give the same bytes.
__device__ __forceinline__ uint32_t e2m1_index(const float a) {
  // thresholds with their ties: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
  return a <= 0.25f ? 0u : (a < 0.75f ? 1u : (a <= 1.25f ? 2u : (a < 1.75f ? 3u : (a <= 2.5f ? 4u : (a < 3.5f ? 5u : (a <= 5.0f ? 6u : 7u))))));
}
__global__ __launch_bounds__(256) void quant_mxfp4_rows_kernel(const bf16_t* __restrict__ W, long long ldw, uint8_t* __restrict__ q, long long ldq,
                                                               uint8_t* __restrict__ s, long long lds, int K) {
  const bf16_t* wr = W + (long long)blockIdx.x * ldw;
  uint8_t* qr = q + (long long)blockIdx.x * ldq;
  uint8_t* sr = s + (long long)blockIdx.x * lds;
  for (int b = threadIdx.x; b < (K >> 5); b += 256) {
    u32x4_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *(const u32x4_t*)(wr + b * 32 + i * 8);
    uint32_t amax = 0u;                                  // bf16 bits without the sign: ordered like the magnitudes
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = v[i][j] & 0x7fffu, hi = (v[i][j] >> 16) & 0x7fffu;
        amax = amax > lo ? amax : lo;
        amax = amax > hi ? amax : hi;
      }
    int e = (int)(amax >> 7) - 127 - 2;
    e = e < -125 ? -125 : (e > 125 ? 125 : e);
    if (amax == 0u) e = 0;
    const float inv = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);     // 2^-e
    u32x4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t word = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = v[i][j] & 0xffffu, hi = v[i][j] >> 16;
        const uint32_t cl = e2m1_index(__builtin_bit_cast(float, (lo & 0x7fffu) << 16) * inv) | ((lo >> 12) & 8u);
        const uint32_t ch = e2m1_index(__builtin_bit_cast(float, (hi & 0x7fffu) << 16) * inv) | ((hi >> 12) & 8u);
        word |= (cl | (ch << 4)) << (8 * j);
      }
      o[i] = amax == 0u ? 0u : word;
    }
    *(u32x4_t*)(qr + b * 16) = o;
    sr[b] = (uint8_t)(e + 127);
  }
}

}  // namespace

// launch epilogue of the entry points that serve two exported names (MLA_LAUNCH_CHECK reports __func__)
static int launch_status(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  mla_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
  return (int)e;
}

#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

// What the entry points check and pass per weight format: K must be a multiple of KQ (bf16: a 16-B load; W8: a lane's 16 codes; W4: a
// scale block), ldw (elements of W's type: bf16 elements, or bytes) a multiple of LQ (16-B aligned rows), a W4 row holds K / 2 bytes and
// its scale row K / 32
template <WFmt F> struct wfmt_args {
  static constexpr int KQ = F == WF_W4 ? 32 : (F == WF_W8 ? 16 : 8), LQ = F == WF_BF16 ? 8 : 16;
  static bool scale_ok(const void* w_scale, long long ld_scale, int K) { return F == WF_BF16 || (w_scale && (F != WF_W4 || ld_scale >= K / 32)); }
  static bool row_ok(long long ldw, int K) { return ldw % LQ == 0 && (F != WF_W4 || ldw >= K / 2); }
  static typename welem<F>::scale_t scale(const void* w_scale, long long ld_scale) {
    if constexpr (F == WF_W4) return w4_scales{(const uint8_t*)w_scale, ld_scale};
    else return (const float*)w_scale;
  }
};

// mla_gemv_bf16 / mla_gemv_w8: one validation + launch path, W8 selects the weight format (ldw in elements of it)
template <WFmt F>
static int gemv_entry(const char* name, const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out, long long ldo,
                      long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre,
                      const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols, hipStream_t stream) {
  constexpr int KQ = wfmt_args<F>::KQ;
  MLA_CHECK_ARG(x && W && out && wfmt_args<F>::scale_ok(w_scale, ld_scale, K > 0 ? K : 0), "%s: null pointer (or a W4 scale row shorter than K / 32)", name);
  MLA_CHECK_ARG((rope_cos == nullptr) == (rope_sin == nullptr) && (!rope_cos || (rope_cols > 0 && rope_cols % 128 == 0 && rope_cols <= N && !residual)),
                "%s: the RoPE epilogue needs both tables, rope_cols a multiple of 128 and <= N, and no residual", name);
  MLA_CHECK_ARG(pre >= 0 && pre <= 2 && (pre != 1 || (pre_w && AL16(pre_w))), "%s: pre must be 0, 1 (RMSNorm: 16-B aligned weight needed) or 2 (SwiGLU)", name);
  MLA_CHECK_ARG(M >= 1 && M <= GEMV_MMAX && N >= 1 && K >= KQ && K % KQ == 0 && rows_per_batch >= 1, "%s: 1 <= M <= 8, K %% %d == 0 required (M %d, N %d, K %d)", name, KQ, M, N, K);
  MLA_CHECK_ARG(AL16(x) && AL16(W) && ldx % 8 == 0 && wfmt_args<F>::row_ok(ldw, K), "%s: x / W rows must be 16-B aligned", name);
  const size_t lds = (size_t)M * K * 2 + 64;
  MLA_CHECK_ARG(lds <= 160 * 1024, "%s: M x K x 2 bytes of input rows (+ 64) must fit the 160 KiB of LDS (M %d, K %d)", name, M, K);
  static int cus = 0;
  if (!cus) { hipDeviceProp_t p; int d = 0; (void)hipGetDevice(&d); cus = (hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }
  const int sets = (N + GEMV_ROWS - 1) / GEMV_ROWS;
  int blocks = (sets + 3) / 4;
  int per_cu = (int)((160 * 1024) / (lds > 20 * 1024 ? lds : 20 * 1024));      // resident workgroups per CU: LDS for x, at most 32 waves
  per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
  const int cap = cus * per_cu;
  if (blocks > cap) blocks = cap;
#define MLA_GEMV_LAUNCH(MM, PP)                                                                                                        \
  {                                                                                                                                    \
    static bool attr = false;                                                                                                          \
    if (!attr) { (void)hipFuncSetAttribute((const void*)gemv_kernel<MM, PP, F>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
    hipLaunchKernelGGL((gemv_kernel<MM, PP, F>), dim3(blocks), dim3(256), lds, stream, (const bf16_t*)x, ldx, (const typename welem<F>::t*)W, ldw, \
                       wfmt_args<F>::scale(w_scale, ld_scale), (bf16_t*)out, ldo, out_batch_stride, rows_per_batch, (const bf16_t*)residual, ld_res, N, K, (const bf16_t*)pre_w, eps, \
                       rope_cos, rope_sin, rope_cos ? rope_cols : 0);                                                                  \
  }
#define MLA_GEMV_CASE(MM)                                                                                                              \
  case MM:                                                                                                                             \
    if (pre == 0) MLA_GEMV_LAUNCH(MM, 0) else if (pre == 1) MLA_GEMV_LAUNCH(MM, 1) else MLA_GEMV_LAUNCH(MM, 2)                          \
    break;
  switch (M) {
    MLA_GEMV_CASE(1) MLA_GEMV_CASE(2) MLA_GEMV_CASE(3) MLA_GEMV_CASE(4) MLA_GEMV_CASE(5) MLA_GEMV_CASE(6) MLA_GEMV_CASE(7) MLA_GEMV_CASE(8)
  }
#undef MLA_GEMV_CASE
#undef MLA_GEMV_LAUNCH
  return launch_status(name);
}

extern "C" int mla_gemv_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                             int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre, const void* pre_w, float eps,
                             const float* rope_cos, const float* rope_sin, int rope_cols, hipStream_t stream) {
  return gemv_entry<WF_BF16>("mla_gemv_bf16", x, ldx, W, ldw, nullptr, 0, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res, M, N, K, pre, pre_w,
                           eps, rope_cos, rope_sin, rope_cols, stream);
}

extern "C" int mla_gemv_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                           long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre,
                           const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols, hipStream_t stream) {
  return gemv_entry<WF_W8>("mla_gemv_w8", x, ldx, W, ldw, w_scale, 0, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res, M, N, K, pre, pre_w,
                           eps, rope_cos, rope_sin, rope_cols, stream);
}

extern "C" int mla_gemv_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                           long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N,
                           int K, int pre, const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols,
                           hipStream_t stream) {
  return gemv_entry<WF_W4>("mla_gemv_w4", x, ldx, W, ldw, w_scale, ld_scale, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res, M, N, K,
                           pre, pre_w, eps, rope_cos, rope_sin, rope_cols, stream);
}

extern "C" int mla_attn_decode(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, int S_kv, int R, long long ld,
                               long long batch_stride, long long ld_o, float scale, hipStream_t stream) {
  MLA_CHECK_ARG(q && k && v && o, "mla_attn_decode: null pointer");
  MLA_CHECK_ARG(head_dim == 128, "mla_attn_decode: head_dim must be 128 (got %d)", head_dim);
  MLA_CHECK_ARG(B >= 1 && H >= 1 && R >= 1 && R <= DEC_RMAX && S_kv >= R, "mla_attn_decode: 1 <= R <= 8 <= S_kv required (R %d, S_kv %d)", R, S_kv);
  MLA_CHECK_ARG(AL16(q) && AL16(k) && AL16(v) && ld % 8 == 0 && batch_stride % 8 == 0 && ld_o % 2 == 0, "mla_attn_decode: 16-B aligned rows required");
  const size_t lds = ((size_t)R * S_kv + DEC_NW * (size_t)R * 128) * 4;
  MLA_CHECK_ARG(lds <= 160 * 1024, "mla_attn_decode: R x S_kv scores do not fit LDS (R %d, S_kv %d)", R, S_kv);
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)attn_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; }
  hipLaunchKernelGGL(attn_decode_kernel, dim3(B * H), dim3(64 * DEC_NW), lds, stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, H, S_kv,
                     R, ld, batch_stride, ld_o, scale);
  MLA_LAUNCH_CHECK();
}

// mla_gemm_skinny_bf16 / mla_gemm_skinny_w8: one validation + launch path, W8 selects the weight format
template <WFmt F>
static int skinny_entry(const char* name, const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out, long long ldo,
                        long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre,
                        const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols, hipStream_t stream) {
  constexpr int KQ = wfmt_args<F>::KQ;
  MLA_CHECK_ARG(x && W && out && wfmt_args<F>::scale_ok(w_scale, ld_scale, K > 0 ? K : 0), "%s: null pointer (or a W4 scale row shorter than K / 32)", name);
  MLA_CHECK_ARG((rope_cos == nullptr) == (rope_sin == nullptr) && (!rope_cos || (rope_cols > 0 && rope_cols % 128 == 0 && rope_cols <= N && !residual)),
                "%s: the RoPE epilogue needs both tables, rope_cols a multiple of 128 and <= N, and no residual", name);
  MLA_CHECK_ARG(pre >= 0 && pre <= 2 && (pre != 1 || (pre_w && AL16(pre_w))),
                "%s: pre must be 0, 1 (RMSNorm: 16-B aligned weight needed) or 2 (SwiGLU)", name);
  MLA_CHECK_ARG(M >= 1 && M <= SK_MMAX && N >= 1 && K >= KQ && K % KQ == 0 && rows_per_batch >= 1,
                "%s: 1 <= M <= 64, K %% %d == 0 required (M %d, N %d, K %d)", name, KQ, M, N, K);
  MLA_CHECK_ARG(AL16(x) && AL16(W) && ldx % 8 == 0 && wfmt_args<F>::row_ok(ldw, K), "%s: x / W rows must be 16-B aligned", name);
  const int tiles = (N + 15) / 16;
#define MLA_SK_LAUNCH(MB, PP)                                                                                                          \
  hipLaunchKernelGGL((gemm_skinny_kernel<MB, PP, F>), dim3(tiles), dim3(64 * SK_NW), 0, stream, (const bf16_t*)x, ldx,                  \
                     (const typename welem<F>::t*)W, ldw, wfmt_args<F>::scale(w_scale, ld_scale), (bf16_t*)out, ldo, out_batch_stride, rows_per_batch,                \
                     (const bf16_t*)residual, ld_res, M, N, K, (const bf16_t*)pre_w, eps, rope_cos, rope_sin, rope_cos ? rope_cols : 0)
#define MLA_SK_CASE(MB)                                                                                                                \
  case MB:                                                                                                                             \
    if (pre == 0) MLA_SK_LAUNCH(MB, 0); else if (pre == 1) MLA_SK_LAUNCH(MB, 1); else MLA_SK_LAUNCH(MB, 2);                              \
    break;
  switch ((M + 15) / 16) { MLA_SK_CASE(1) MLA_SK_CASE(2) MLA_SK_CASE(3) MLA_SK_CASE(4) }
#undef MLA_SK_CASE
#undef MLA_SK_LAUNCH
  return launch_status(name);
}

extern "C" int mla_gemm_skinny_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                                    int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre, const void* pre_w,
                                    float eps, const float* rope_cos, const float* rope_sin, int rope_cols, hipStream_t stream) {
  return skinny_entry<WF_BF16>("mla_gemm_skinny_bf16", x, ldx, W, ldw, nullptr, 0, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res, M, N, K,
                             pre, pre_w, eps, rope_cos, rope_sin, rope_cols, stream);
}

extern "C" int mla_gemm_skinny_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                                  long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K,
                                  int pre, const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols,
                                  hipStream_t stream) {
  return skinny_entry<WF_W8>("mla_gemm_skinny_w8", x, ldx, W, ldw, w_scale, 0, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res, M, N, K,
                             pre, pre_w, eps, rope_cos, rope_sin, rope_cols, stream);
}

extern "C" int mla_gemm_skinny_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                                  long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M,
                                  int N, int K, int pre, const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols,
                                  hipStream_t stream) {
  return skinny_entry<WF_W4>("mla_gemm_skinny_w4", x, ldx, W, ldw, w_scale, ld_scale, out, ldo, out_batch_stride, rows_per_batch, residual, ld_res,
                             M, N, K, pre, pre_w, eps, rope_cos, rope_sin, rope_cols, stream);
}

// mla_gemm_skinny_gateup_swiglu_bf16 / _w8: gemm_skinny_kernel's GU form (gate|up projection with the SwiGLU epilogue)
template <WFmt F>
static int skinny_gateup_entry(const char* name, const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                               long long ldo, int M, int I, int K, hipStream_t stream) {
  constexpr int KQ = wfmt_args<F>::KQ;
  MLA_CHECK_ARG(x && W && out && wfmt_args<F>::scale_ok(w_scale, ld_scale, K > 0 ? K : 0), "%s: null pointer (or a W4 scale row shorter than K / 32)", name);
  MLA_CHECK_ARG(M >= 1 && M <= SK_MMAX && I >= 8 && I % 8 == 0 && K >= KQ && K % KQ == 0,
                "%s: 1 <= M <= 64, I %% 8 == 0, K %% %d == 0 required (M %d, I %d, K %d)", name, KQ, M, I, K);
  MLA_CHECK_ARG(AL16(x) && AL16(W) && ldx % 8 == 0 && wfmt_args<F>::row_ok(ldw, K) && ldx >= K && (F == WF_W4 || ldw >= K),
                "%s: x / W rows must be 16-B aligned and hold K elements", name);
  MLA_CHECK_ARG(ldo >= I, "%s: ldo %lld < I %d", name, ldo, I);
#define MLA_SKGU_CASE(MB)                                                                                                              \
  case MB:                                                                                                                             \
    hipLaunchKernelGGL((gemm_skinny_kernel<MB, 0, F, true>), dim3(I / 8), dim3(64 * SK_NW), 0, stream, (const bf16_t*)x, ldx,           \
                       (const typename welem<F>::t*)W, ldw, wfmt_args<F>::scale(w_scale, ld_scale), (bf16_t*)out, ldo, 0LL, M, (const bf16_t*)nullptr, 0LL, M, I, K,  \
                       (const bf16_t*)nullptr, 0.f, (const float*)nullptr, (const float*)nullptr, 0);                                  \
    break;
  switch ((M + 15) / 16) { MLA_SKGU_CASE(1) MLA_SKGU_CASE(2) MLA_SKGU_CASE(3) MLA_SKGU_CASE(4) }
#undef MLA_SKGU_CASE
  return launch_status(name);
}

extern "C" int mla_gemm_skinny_gateup_swiglu_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, int M,
                                                  int I, int K, hipStream_t stream) {
  return skinny_gateup_entry<WF_BF16>("mla_gemm_skinny_gateup_swiglu_bf16", x, ldx, W, ldw, nullptr, 0, out, ldo, M, I, K, stream);
}

extern "C" int mla_gemm_skinny_gateup_swiglu_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out,
                                                long long ldo, int M, int I, int K, hipStream_t stream) {
  return skinny_gateup_entry<WF_W8>("mla_gemm_skinny_gateup_swiglu_w8", x, ldx, W, ldw, w_scale, 0, out, ldo, M, I, K, stream);
}

extern "C" int mla_gemm_skinny_gateup_swiglu_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale,
                                                void* out, long long ldo, int M, int I, int K, hipStream_t stream) {
  return skinny_gateup_entry<WF_W4>("mla_gemm_skinny_gateup_swiglu_w4", x, ldx, W, ldw, w_scale, ld_scale, out, ldo, M, I, K, stream);
}

// W [N, K] bf16 (ldw) -> q [N, K] e4m3fn codes (ldq, bytes) + scale [N] fp32; see quant_fp8_rows_kernel
extern "C" int mla_quant_fp8_rows(const void* W, long long ldw, void* q, long long ldq, float* scale, int N, int K, hipStream_t stream) {
  MLA_CHECK_ARG(W && q && scale, "mla_quant_fp8_rows: null pointer");
  MLA_CHECK_ARG(N >= 1 && K >= 16 && K % 16 == 0, "mla_quant_fp8_rows: N >= 1, K %% 16 == 0 required (N %d, K %d)", N, K);
  MLA_CHECK_ARG(AL16(W) && AL16(q) && ldw % 8 == 0 && ldq % 16 == 0 && ldw >= K && ldq >= K, "mla_quant_fp8_rows: W / q rows must be 16-B aligned and hold K elements");
  hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3(N), dim3(256), 0, stream, (const bf16_t*)W, ldw, (uint8_t*)q, ldq, scale, K);
  MLA_LAUNCH_CHECK();
}

// W [N, K] bf16 (ldw) -> q [N, K / 2] e2m1 code pairs (ldq, bytes) + s [N, K / 32] e8m0 scale bytes (lds, bytes); see quant_mxfp4_rows_kernel
extern "C" int mla_quant_mxfp4_rows(const void* W, long long ldw, void* q, long long ldq, void* s, long long lds, int N, int K, hipStream_t stream) {
  MLA_CHECK_ARG(W && q && s, "mla_quant_mxfp4_rows: null pointer");
  MLA_CHECK_ARG(N >= 1 && K >= 32 && K % 32 == 0, "mla_quant_mxfp4_rows: N >= 1, K %% 32 == 0 required (N %d, K %d)", N, K);
  MLA_CHECK_ARG(AL16(W) && AL16(q) && ldw % 8 == 0 && ldq % 16 == 0 && ldw >= K && ldq >= K / 2 && lds >= K / 32,
                "mla_quant_mxfp4_rows: W / q rows must be 16-B aligned and hold K elements, a scale row K / 32 bytes");
  hipLaunchKernelGGL(quant_mxfp4_rows_kernel, dim3(N), dim3(256), 0, stream, (const bf16_t*)W, ldw, (uint8_t*)q, ldq, (uint8_t*)s, lds, K);
  MLA_LAUNCH_CHECK();
}

extern "C" int mla_attn_chunk(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, int S_kv, int R, long long ld,
                              long long batch_stride, long long ld_o, float scale, hipStream_t stream) {
  MLA_CHECK_ARG(q && k && v && o, "mla_attn_chunk: null pointer");
  MLA_CHECK_ARG(head_dim == 128, "mla_attn_chunk: head_dim must be 128 (got %d)", head_dim);
  MLA_CHECK_ARG(B >= 1 && H >= 1 && R >= 1 && R <= SUF_RMAX && S_kv >= R, "mla_attn_chunk: 1 <= R <= 64, R <= S_kv required (R %d, S_kv %d)", R, S_kv);
  MLA_CHECK_ARG(AL16(q) && AL16(k) && AL16(v) && ld % 8 == 0 && batch_stride % 8 == 0 && ld_o % 2 == 0, "mla_attn_chunk: 16-B aligned rows required");
  const size_t lds = SUF_LDS_BYTES;
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)attn_chunk_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; }
  hipLaunchKernelGGL(attn_chunk_kernel<false>, dim3(B * H * ((R + 15) / 16)), dim3(64 * SUF_NW), lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                     (const bf16_t*)v, (bf16_t*)o, H, S_kv, R, ld, batch_stride, ld_o, scale, (const int*)nullptr);
  MLA_LAUNCH_CHECK();
}

extern "C" int mla_attn_chunk_ragged(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, const int* kv_len, int S_cap,
                                     int R, long long ld, long long batch_stride, long long ld_o, float scale, hipStream_t stream) {
  MLA_CHECK_ARG(q && k && v && o && kv_len, "mla_attn_chunk_ragged: null pointer");
  MLA_CHECK_ARG(head_dim == 128, "mla_attn_chunk_ragged: head_dim must be 128 (got %d)", head_dim);
  MLA_CHECK_ARG(B >= 1 && H >= 1 && R >= 1 && R <= SUF_RMAX && S_cap >= R, "mla_attn_chunk_ragged: 1 <= R <= 64, R <= S_cap required (R %d, S_cap %d)", R, S_cap);
  MLA_CHECK_ARG(AL16(q) && AL16(k) && AL16(v) && ld % 8 == 0 && batch_stride % 8 == 0 && ld_o % 2 == 0, "mla_attn_chunk_ragged: 16-B aligned rows required");
  const size_t lds = SUF_LDS_BYTES;
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)attn_chunk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; }
  hipLaunchKernelGGL(attn_chunk_kernel<true>, dim3(B * H * ((R + 15) / 16)), dim3(64 * SUF_NW), lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                     (const bf16_t*)v, (bf16_t*)o, H, S_cap, R, ld, batch_stride, ld_o, scale, kv_len);
  MLA_LAUNCH_CHECK();
}

// mla_attn_chunk_groups(_gw) / mla_attn_chunk_ragged_groups(_gw): one validation + launch path; gw = groups per workgroup (0: the library's
// choice). prefix_len != nullptr selects the ragged form: B samples, S_p_or_cap is then S_cap, the rows per sample.
static int attn_groups_entry(const char* name, const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim,
                             const int* prefix_len, int S_p_or_cap, int R, long long ld, long long bs, long long ld_o, float scale, int gw,
                             int order, hipStream_t stream) {
  const bool ragged = prefix_len != nullptr;
  MLA_CHECK_ARG(q && k && v && o, "%s: null pointer", name);
  MLA_CHECK_ARG(head_dim == 128, "%s: head_dim must be 128 (got %d)", name, head_dim);
  MLA_CHECK_ARG(B >= 1 && G >= 1 && H >= 1 && R >= 1 && R <= SUF_RMAX, "%s: B >= 1, G >= 1, 1 <= R <= 64 required (B %d, G %d, R %d)", name, B, G, R);
  if (ragged) {
    MLA_CHECK_ARG((long long)G * R <= (long long)S_p_or_cap, "%s: S_cap (%d) must hold the G * R suffix rows of a sample (G %d, R %d)", name,
                  S_p_or_cap, G, R);
    MLA_CHECK_ARG((long long)B * G * R <= 0x7fffffffLL && bs % 8 == 0, "%s: B * G * R output rows exceed the int range, or the sample stride is not 16-B aligned", name);
  } else {
    MLA_CHECK_ARG(S_p_or_cap >= 0, "%s: S_p >= 0 required (S_p %d)", name, S_p_or_cap);
    MLA_CHECK_ARG((long long)S_p_or_cap + (long long)G * R <= 0x7fffffffLL, "%s: S_p + G * R rows exceed the int range (G %d, R %d, S_p %d)", name, G, R, S_p_or_cap);
  }
  MLA_CHECK_ARG(AL16(q) && AL16(k) && AL16(v) && ld % 8 == 0 && ld_o % 2 == 0, "%s: 16-B aligned rows required", name);
  MLA_CHECK_ARG(gw == 0 || gw == 1 || gw == 2 || gw == 4, "%s: groups per workgroup must be 0 (default), 1, 2 or 4 (got %d)", name, gw);
  MLA_CHECK_ARG(order >= -1 && order <= 1, "%s: order must be -1 (default), 0 (as dispatched) or 1 (one chunk of the grid per XCD) (got %d)", name, order);
  if (gw == 0) gw = ATTN_GROUPS_GW;
  if (order < 0) order = ATTN_GROUPS_XCD_CHUNKS;
  const size_t lds = SUF_LDS_BYTES;
  const int QB = (R + 15) / 16;
  const long long grid = (long long)B * H * ((G + gw - 1) / gw) * QB;
  MLA_CHECK_ARG(grid <= 0x7fffffffLL, "%s: %lld workgroups exceed the grid range", name, grid);
  const int xcd_chunks = order == 1 && grid % 8 == 0;
#define MLA_AG_LAUNCH(GW, RG)                                                                                                          \
  {                                                                                                                                    \
    static bool attr = false;                                                                                                          \
    if (!attr) { (void)hipFuncSetAttribute((const void*)attn_chunk_groups_kernel<GW, RG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; } \
    hipLaunchKernelGGL((attn_chunk_groups_kernel<GW, RG>), dim3((unsigned)grid), dim3(64 * SUF_NW), lds, stream, (const bf16_t*)q,       \
                       (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, G, H, RG ? 0 : S_p_or_cap, R, ld, ld_o, scale, xcd_chunks,         \
                       prefix_len, RG ? S_p_or_cap : 0, RG ? bs : 0LL);                                                                 \
  }
  if (ragged) {
    if (gw == 1) MLA_AG_LAUNCH(1, true) else if (gw == 2) MLA_AG_LAUNCH(2, true) else MLA_AG_LAUNCH(4, true)
  } else {
    if (gw == 1) MLA_AG_LAUNCH(1, false) else if (gw == 2) MLA_AG_LAUNCH(2, false) else MLA_AG_LAUNCH(4, false)
  }
#undef MLA_AG_LAUNCH
  return launch_status(name);
}

extern "C" int mla_attn_chunk_groups(const void* q, const void* k, const void* v, void* o, int G, int H, int head_dim, int S_p, int R, long long ld,
                                     long long ld_o, float scale, hipStream_t stream) {
  return attn_groups_entry("mla_attn_chunk_groups", q, k, v, o, 1, G, H, head_dim, nullptr, S_p, R, ld, 0, ld_o, scale, 0, -1, stream);
}

extern "C" int mla_attn_chunk_groups_gw(const void* q, const void* k, const void* v, void* o, int G, int H, int head_dim, int S_p, int R,
                                        long long ld, long long ld_o, float scale, int gw, int order, hipStream_t stream) {
  return attn_groups_entry("mla_attn_chunk_groups_gw", q, k, v, o, 1, G, H, head_dim, nullptr, S_p, R, ld, 0, ld_o, scale, gw, order, stream);
}

extern "C" int mla_attn_chunk_ragged_groups(const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim,
                                            const int* prefix_len, int S_cap, int R, long long ld, long long batch_stride, long long ld_o,
                                            float scale, hipStream_t stream) {
  MLA_CHECK_ARG(prefix_len, "mla_attn_chunk_ragged_groups: null pointer");
  return attn_groups_entry("mla_attn_chunk_ragged_groups", q, k, v, o, B, G, H, head_dim, prefix_len, S_cap, R, ld, batch_stride, ld_o, scale, 0,
                           -1, stream);
}

extern "C" int mla_attn_chunk_ragged_groups_gw(const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim,
                                               const int* prefix_len, int S_cap, int R, long long ld, long long batch_stride, long long ld_o,
                                               float scale, int gw, int order, hipStream_t stream) {
  MLA_CHECK_ARG(prefix_len, "mla_attn_chunk_ragged_groups_gw: null pointer");
  return attn_groups_entry("mla_attn_chunk_ragged_groups_gw", q, k, v, o, B, G, H, head_dim, prefix_len, S_cap, R, ld, batch_stride, ld_o, scale,
                           gw, order, stream);
}

// mla_gemm_suffix_bf16(_pos) / mla_gemm_suffix_w8(_pos): one validation + launch path, W8 selects the weight format; rope_pos == nullptr
// is the form without a separate rotary position (the table row is the cache row)
template <WFmt F>
static int suffix_entry(const char* name, const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out, long long ldo,
                        long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual, long long ld_res,
                        int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols, const int* rope_pos, int rope_rows,
                        hipStream_t stream) {
  constexpr int KQ = wfmt_args<F>::KQ;
  MLA_CHECK_ARG(x && W && out && wfmt_args<F>::scale_ok(w_scale, ld_scale, K > 0 ? K : 0), "%s: null pointer (or a W4 scale row shorter than K / 32)", name);
  MLA_CHECK_ARG((rope_cos == nullptr) == (rope_sin == nullptr) && (!rope_cos || (rope_cols > 0 && rope_cols % 128 == 0 && rope_cols <= N && !residual)),
                "%s: the RoPE epilogue needs both tables, rope_cols a multiple of 128 and <= N, and no residual", name);
  MLA_CHECK_ARG(M >= 1 && M <= 256 && N >= 1 && K >= KQ && K % KQ == 0 && rows_per_batch >= 1,
                "%s: 1 <= M <= 256, K %% %d == 0 required (M %d, N %d, K %d)", name, KQ, M, N, K);
  MLA_CHECK_ARG(!slot || cap_rows >= rows_per_batch, "%s: cap_rows (%d) must hold the %d rows of a sample", name, cap_rows, rows_per_batch);
  MLA_CHECK_ARG(!rope_pos || (rope_cos && rope_rows >= 1), "%s: rope_pos needs the RoPE tables and rope_rows >= 1 (got %d)", name, rope_rows);
  MLA_CHECK_ARG(AL16(x) && AL16(W) && ldx % 8 == 0 && wfmt_args<F>::row_ok(ldw, K), "%s: x / W rows must be 16-B aligned", name);
  if (!slot) cap_rows = rows_per_batch;
  const int tiles = (N + 15) / 16, blocks = (M + 15) / 16;
#define MLA_SX_LAUNCH(NT, MB)                                                                                                          \
  hipLaunchKernelGGL((gemm_suffix_kernel<NT, MB, F>), dim3((tiles + NT - 1) / NT), dim3(64 * SK_NW), 0, stream, (const bf16_t*)x, ldx,   \
                     (const typename welem<F>::t*)W, ldw, wfmt_args<F>::scale(w_scale, ld_scale), (bf16_t*)out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows, \
                     (const bf16_t*)residual, ld_res, M, N, K, rope_cos, rope_sin, rope_cos ? rope_cols : 0, rope_pos, rope_rows)
  if (blocks <= 1) MLA_SX_LAUNCH(1, 1);
  else if (blocks == 2) MLA_SX_LAUNCH(1, 2);
  else if (blocks == 3) MLA_SX_LAUNCH(1, 3);
  else if (blocks == 4) MLA_SX_LAUNCH(1, 4);
  else if (blocks <= 6) MLA_SX_LAUNCH(2, 6);
  else if (blocks <= 8) MLA_SX_LAUNCH(2, 8);
  else MLA_SX_LAUNCH(2, 16);
#undef MLA_SX_LAUNCH
  return launch_status(name);
}

extern "C" int mla_gemm_suffix_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                                    int rows_per_batch, const int* slot, int cap_rows, const void* residual, long long ld_res, int M, int N, int K,
                                    const float* rope_cos, const float* rope_sin, int rope_cols, hipStream_t stream) {
  return suffix_entry<WF_BF16>("mla_gemm_suffix_bf16", x, ldx, W, ldw, nullptr, 0, out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows, residual,
                             ld_res, M, N, K, rope_cos, rope_sin, rope_cols, nullptr, 0, stream);
}

extern "C" int mla_gemm_suffix_bf16_pos(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo,
                                        long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                                        long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                                        const int* rope_pos, int rope_rows, hipStream_t stream) {
  return suffix_entry<WF_BF16>("mla_gemm_suffix_bf16_pos", x, ldx, W, ldw, nullptr, 0, out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows,
                             residual, ld_res, M, N, K, rope_cos, rope_sin, rope_cols, rope_pos, rope_rows, stream);
}

extern "C" int mla_gemm_suffix_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                                  long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                                  long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                                  hipStream_t stream) {
  return suffix_entry<WF_W8>("mla_gemm_suffix_w8", x, ldx, W, ldw, w_scale, 0, out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows, residual,
                            ld_res, M, N, K, rope_cos, rope_sin, rope_cols, nullptr, 0, stream);
}

extern "C" int mla_gemm_suffix_w8_pos(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                                      long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                                      long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                                      const int* rope_pos, int rope_rows, hipStream_t stream) {
  return suffix_entry<WF_W8>("mla_gemm_suffix_w8_pos", x, ldx, W, ldw, w_scale, 0, out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows,
                            residual, ld_res, M, N, K, rope_cos, rope_sin, rope_cols, rope_pos, rope_rows, stream);
}

extern "C" int mla_gemm_suffix_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                                  long long ldo, long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                                  long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                                  hipStream_t stream) {
  return suffix_entry<WF_W4>("mla_gemm_suffix_w4", x, ldx, W, ldw, w_scale, ld_scale, out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows,
                             residual, ld_res, M, N, K, rope_cos, rope_sin, rope_cols, nullptr, 0, stream);
}

extern "C" int mla_gemm_suffix_w4_pos(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                                      long long ldo, long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows,
                                      const void* residual, long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin,
                                      int rope_cols, const int* rope_pos, int rope_rows, hipStream_t stream) {
  return suffix_entry<WF_W4>("mla_gemm_suffix_w4_pos", x, ldx, W, ldw, w_scale, ld_scale, out, ldo, out_batch_stride, rows_per_batch, slot, cap_rows,
                             residual, ld_res, M, N, K, rope_cos, rope_sin, rope_cols, rope_pos, rope_rows, stream);
}
