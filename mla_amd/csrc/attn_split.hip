// Split-key suffix attention (opt-in: MLA.predict_action_diff(suffix_attention="split")): mla_attn_chunk's contract with each head's key
// range cut over several workgroups, so that a sampler step's attention reads its cache with most of the chip instead of B x H x ceil(R/16)
// CUs (32 of 256 at 7B, batch 1, one action row).
//
//   mla_attn_chunk_split   launch 1: workgroup (b, h, block of 16 queries, s) runs attn_chunk_kernel's arithmetic (infer.hip) over the
//                          s-th contiguous range of the 64-key tiles and writes the un-normalised softmax state (m, l, 128 fp32 sums) of
//                          its valid query rows into the caller's workspace. launch 2: one wave per (b, h, query) merges the states in the
//                          order s = 0, 1, ..., divides once, rounds once. No counters, no atomics, no workgroup waits on another: the
//                          dependency is the kernel boundary (~1.2 us), which in-launch combines measured dearer than.
//                          splits == 1: launch 1 alone in its finishing form -- no workspace access, and mla_attn_chunk's bits.
//   mla_attn_chunk_split_plan / _ws_bytes   pure host functions: the launcher's choice of splits, and the workspace it needs.
//
// Nothing here allocates, keeps state between calls or reads a workspace word this call did not write: graph-capturable, deterministic.
#include "common.h"

namespace {

constexpr int SP_RMAX = 64;
constexpr int SP_NW = 4;                        // waves per workgroup: wave w takes tiles t0 + w, t0 + w + 4, ... of its range
constexpr int SP_VP = 68;                       // V^T row pitch in keys (136 B: 8-B aligned, staggered banks), as in attn_chunk_kernel
constexpr int SP_CUS = 256;                     // the launcher plans for the MI355X's 256 CUs (no device query, no state)
constexpr int SP_STATE = 130;                   // fp32 words per (b, h, query, s): 128 sums in the first array, (m, l) in the second
constexpr int SP_CW = 4;                        // combine launch: waves (= states merged) per workgroup

__device__ __forceinline__ bf16x8_t as_frag(const u32x4_t v) { return __builtin_bit_cast(bf16x8_t, v); }
__device__ __forceinline__ bf16x8_t pack_pfrag(const f32x4_t lo, const f32x4_t hi) {
  u32x4_t u;
  u[0] = pack2bf(lo[0], lo[1]); u[1] = pack2bf(lo[2], lo[3]);
  u[2] = pack2bf(hi[0], hi[1]); u[3] = pack2bf(hi[2], hi[3]);
  return as_frag(u);
}
// the one normalisation both forms end in: one division, one bf16 rounding
__device__ __forceinline__ bf16_t sp_finish(float O, float L) { return f2bf(O / L); }

struct SplitPlan { int nT, splits, tps, wgs, cwgs; long long ws_bytes; };

inline long long sp_ws_bytes(int B, int H, int R, int splits) {
  return splits > 1 ? (long long)B * H * R * splits * SP_STATE * 4 : 0;
}
// splits grows by one while launch 1 still fits one workgroup per CU (measured: a second round of workgroups costs more than it saves),
// splits < nT, and the largest range has more than SP_NW tiles: a workgroup's time is its passes over its range, four tiles per pass, and
// cutting below one pass saves nothing but adds states to merge (measured at 9 tiles: 3 ranges 12.3 us, 4: 12.5, 9: 14.0 per launch
// pair). Every range so keeps at least 2 tiles. 1 when twice the unsplit grid no longer fits the chip.
inline SplitPlan sp_plan(int B, int H, int R, int S_kv, int cus, int forced) {
  SplitPlan p;
  const long long base = (long long)B * H * ((R + 15) / 16);
  p.nT = (S_kv + 63) / 64;
  p.splits = 1;
  if (forced > 0) p.splits = forced;
  else
    while (base * (p.splits + 1) <= cus && p.splits < p.nT && (p.nT + p.splits - 1) / p.splits > SP_NW) ++p.splits;
  p.tps = (p.nT + p.splits - 1) / p.splits;
  const long long wgs = base * p.splits;
  p.wgs = wgs > 0x7fffffffLL ? -1 : (int)wgs;
  p.cwgs = p.splits > 1 ? (int)(((long long)B * H * R + SP_CW - 1) / SP_CW) : 0;
  p.ws_bytes = sp_ws_bytes(B, H, R, p.splits);
  return p;
}

// attn_chunk_kernel over the tile range [t0, t0 + cnt) of split s = blockIdx.x % splits (ranges differ by at most one tile: the first
// nT % splits ranges take one more). FINISH (splits == 1): the range is every tile, the trip count, the masks and the merge are
// attn_chunk_kernel's, and so is every bit of o. Otherwise a wave whose tile lies behind the range skips the tile (it still meets the
// barriers), and the merged, un-normalised state goes to ws: sums [(b H + h) R + r][s][128], then (m, l) [(b H + h) R + r][s][2].
template <bool FINISH>
__global__ __launch_bounds__(64 * SP_NW) void attn_chunk_split_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                      const bf16_t* __restrict__ v, bf16_t* __restrict__ o, int H, int S_kv,
                                                                      int R, long long ld, long long bs, long long ld_o, float scale,
                                                                      int splits, float* __restrict__ ws, long long nstates) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int QB = (R + 15) >> 4;
  const int s = FINISH ? 0 : (int)(blockIdx.x % splits);
  const int wg = FINISH ? (int)blockIdx.x : (int)(blockIdx.x / splits);
  const int qb = wg % QB, bh = wg / QB, h = bh % H, b = bh / H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  bf16_t* vt = (bf16_t*)smem + wave * 128 * SP_VP;                    // this wave's V tile, transposed: [128 channels][SP_VP keys]
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
  const int ntiles = (S_kv + 63) >> 6;
  const int tbase = ntiles / splits, trem = ntiles % splits;
  const int t0 = s * tbase + (s < trem ? s : trem), cnt = tbase + (s < trem ? 1 : 0);
  const int iters = (cnt + SP_NW - 1) / SP_NW;
  for (int it = 0; it < iters; ++it) {                                  // same trip count in every wave: the barriers below are uniform
    const int tl = it * SP_NW + wave;                                   // tile of the range; behind it (FINISH: beyond S_kv): nothing visible
    const bool live = tl < cnt;
    const int j0 = (t0 + tl) * 64;
    bf16x8_t pf0, pf1;
    if (FINISH || live) {
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
      pf0 = pack_pfrag(st[0], st[1]);
      pf1 = pack_pfrag(st[2], st[3]);
      // V tile -> LDS transposed (lane: key 4 u + g, channels 8 li .. + 7)
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vt[(li * 8 + 2 * e) * SP_VP + u * 4 + g] = (bf16_t)(vv[u][e] & 0xffffu);
          vt[(li * 8 + 2 * e + 1) * SP_VP + u * 4 + g] = (bf16_t)(vv[u][e] >> 16);
        }
    }
    __syncthreads();
    if (FINISH || live) {
#pragma unroll
      for (int fd = 0; fd < 8; ++fd) {
        const bf16_t* vr = vt + (fd * 16 + li) * SP_VP + g * 4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const u32x2_t lo = *(const u32x2_t*)(vr + ks * 32), hi = *(const u32x2_t*)(vr + ks * 32 + 16);
          const u32x4_t av = {lo[0], lo[1], hi[0], hi[1]};
          ot[fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(av), ks ? pf1 : pf0, ot[fd], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // merge the waves' (max, sum, O^T) in wave order; O^T[d][query] of wave w: lane (d & 15) >> 2 ... as the MFMA left it. The split form
  // pads the query pitch to 17 words: its read-out below walks d on the lanes (coalesced state rows)
  constexpr int QP = FINISH ? 16 : 17;
  float* mo = (float*)smem;                                             // [SP_NW][128][QP]
  float* ml = mo + SP_NW * 128 * QP;                                    // [SP_NW][16] max, then [SP_NW][16] sum
#pragma unroll
  for (int fd = 0; fd < 8; ++fd)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) mo[(wave * 128 + fd * 16 + g * 4 + rr) * QP + li] = ot[fd][rr];
  if (g == 0) { ml[wave * 16 + li] = m; ml[SP_NW * 16 + wave * 16 + li] = l; }
  __syncthreads();
  for (int e = threadIdx.x; e < 128 * 16; e += 64 * SP_NW) {
    const int qq = FINISH ? (e & 15) : (e >> 7), d = FINISH ? (e >> 4) : (e & 127), rq = qb * 16 + qq;
    if (rq >= R) continue;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < SP_NW; ++w) mm = fmaxf(mm, ml[w * 16 + qq]);    // FINISH: finite -- wave 0's first tile holds key 0, seen by every query
    if (!FINISH && mm == -INFINITY) mm = 0.f;                           // a range wholly behind the query's causal limit: every weight exp2(-inf) = 0
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < SP_NW; ++w) {
      const float fw = __builtin_amdgcn_exp2f(ml[w * 16 + qq] - mm);
      L += fw * ml[SP_NW * 16 + w * 16 + qq];
      O += fw * mo[(w * 128 + d) * QP + qq];
    }
    if (FINISH) {
      o[(long long)(b * R + rq) * ld_o + h * 128 + d] = sp_finish(O, L);
    } else {
      const long long st = ((long long)bh * R + rq) * splits + s;
      ws[st * 128 + d] = O;                                             // the empty state: O = 0, l = 0, m = -inf
      if (d == 0) {
        float mw = -INFINITY;
#pragma unroll
        for (int w = 0; w < SP_NW; ++w) mw = fmaxf(mw, ml[w * 16 + qq]);
        ws[nstates * 128 + st * 2] = mw;
        ws[nstates * 128 + st * 2 + 1] = L;
      }
    }
  }
}

// one wave per (b, h, query): M = max_s m_s, numerator and denominator summed over s = 0, 1, ... with the weight exp2(m_s - M); an empty
// state (m = -inf) is skipped, i.e. contributes exactly zero and no inf - inf is formed. M is finite: range 0 holds key 0, which every
// query sees. Lane i owns channels 2 i, 2 i + 1.
__global__ __launch_bounds__(64 * SP_CW) void attn_split_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ o, int H, int R,
                                                                        long long ld_o, int splits, long long nrows) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * SP_CW + (threadIdx.x >> 6);   // (b H + h) R + r
  if (row >= nrows) return;
  const float* so = ws + row * splits * 128 + lane * 2;
  const float* sm = ws + nrows * splits * 128 + row * splits * 2;
  float M = -INFINITY;
  for (int s = 0; s < splits; ++s) M = fmaxf(M, sm[s * 2]);
  float L = 0.f, O0 = 0.f, O1 = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float ms = sm[s * 2];
    if (ms == -INFINITY) continue;
    const float fw = __builtin_amdgcn_exp2f(ms - M);
    const mla_f32x2_t ov = *(const mla_f32x2_t*)(so + (long long)s * 128);
    L += fw * sm[s * 2 + 1];
    O0 += fw * ov[0];
    O1 += fw * ov[1];
  }
  const long long bh = row / R;
  const int r = (int)(row - bh * R), h = (int)(bh % H);
  const long long b = bh / H;
  const uint32_t pk = (uint32_t)sp_finish(O0, L) | ((uint32_t)sp_finish(O1, L) << 16);
  *(uint32_t*)(o + (b * R + r) * ld_o + h * 128 + lane * 2) = pk;
}

#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

inline bool sp_shape_ok(int B, int H, int R, int S_kv) { return B >= 1 && H >= 1 && R >= 1 && R <= SP_RMAX && S_kv >= R; }

}  // namespace

extern "C" int mla_attn_chunk_split_plan(int B, int H, int R, int S_kv, int cus, int* out4) {
  MLA_CHECK_ARG(out4, "mla_attn_chunk_split_plan: null pointer");
  MLA_CHECK_ARG(sp_shape_ok(B, H, R, S_kv) && cus >= 1, "mla_attn_chunk_split_plan: B, H, cus >= 1 and 1 <= R <= 64, R <= S_kv required (B %d, H %d, R %d, S_kv %d, cus %d)",
                B, H, R, S_kv, cus);
  const SplitPlan p = sp_plan(B, H, R, S_kv, cus, 0);
  MLA_CHECK_ARG(p.wgs > 0, "mla_attn_chunk_split_plan: grid too large (B %d, H %d)", B, H);
  out4[0] = p.splits; out4[1] = p.tps; out4[2] = p.wgs; out4[3] = p.cwgs;
  return 0;
}

extern "C" long long mla_attn_chunk_split_ws_bytes(int B, int H, int R, int S_kv, int splits) {
  if (!sp_shape_ok(B, H, R, S_kv) || splits < 0 || splits > (S_kv + 63) / 64) {
    mla_set_error("mla_attn_chunk_split_ws_bytes: B, H >= 1, 1 <= R <= 64, R <= S_kv and 0 <= splits <= ceil(S_kv / 64) required (B %d, H %d, R %d, S_kv %d, "
                  "splits %d)", B, H, R, S_kv, splits);
    return -1;
  }
  return sp_plan(B, H, R, S_kv, SP_CUS, splits).ws_bytes;
}

extern "C" int mla_attn_chunk_split(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, int S_kv, int R,
                                    long long ld, long long batch_stride, long long ld_o, float scale, int splits, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
  MLA_CHECK_ARG(q && k && v && o, "mla_attn_chunk_split: null pointer");
  MLA_CHECK_ARG(head_dim == 128, "mla_attn_chunk_split: head_dim must be 128 (got %d)", head_dim);
  MLA_CHECK_ARG(sp_shape_ok(B, H, R, S_kv), "mla_attn_chunk_split: 1 <= R <= 64, R <= S_kv required (R %d, S_kv %d)", R, S_kv);
  MLA_CHECK_ARG(AL16(q) && AL16(k) && AL16(v) && ld % 8 == 0 && batch_stride % 8 == 0 && ld_o % 2 == 0 && (((uintptr_t)o) & 3) == 0,
                "mla_attn_chunk_split: 16-B aligned rows required");
  const int nT = (S_kv + 63) / 64;
  MLA_CHECK_ARG(splits >= 0 && splits <= nT, "mla_attn_chunk_split: splits must be in [0, %d] (0 = the plan's) for S_kv %d, got %d", nT, S_kv, splits);
  const SplitPlan p = sp_plan(B, H, R, S_kv, SP_CUS, splits);
  MLA_CHECK_ARG(p.wgs > 0, "mla_attn_chunk_split: grid too large (B %d, H %d, splits %d)", B, H, p.splits);
  if (p.splits > 1) {
    MLA_CHECK_ARG(ws, "mla_attn_chunk_split: splits %d needs a workspace (null)", p.splits);
    MLA_CHECK_ARG(AL16(ws) && (long long)ws_bytes >= p.ws_bytes, "mla_attn_chunk_split: workspace of %lld bytes (16-B aligned) needed for splits %d, got %lld",
                  p.ws_bytes, p.splits, (long long)ws_bytes);
  }
  const size_t lds = (size_t)SP_NW * 128 * SP_VP * 2;                  // >= the merge buffers ([4][128][17] + 128 floats)
  if (p.splits == 1) {
    (void)hipFuncSetAttribute((const void*)attn_chunk_split_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(attn_chunk_split_kernel<true>, dim3(p.wgs), dim3(64 * SP_NW), lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (bf16_t*)o, H, S_kv, R, ld, batch_stride, ld_o, scale, 1, (float*)nullptr, 0LL);
  } else {
    const long long nrows = (long long)B * H * R;
    (void)hipFuncSetAttribute((const void*)attn_chunk_split_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(attn_chunk_split_kernel<false>, dim3(p.wgs), dim3(64 * SP_NW), lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (bf16_t*)o, H, S_kv, R, ld, batch_stride, ld_o, scale, p.splits, (float*)ws, nrows * p.splits);
    hipLaunchKernelGGL(attn_split_combine_kernel, dim3(p.cwgs), dim3(64 * SP_CW), 0, stream, (const float*)ws, (bf16_t*)o, H, R, ld_o, p.splits,
                       nrows);
  }
  MLA_LAUNCH_CHECK();
}
