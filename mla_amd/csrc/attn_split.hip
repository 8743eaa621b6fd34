// Split-key suffix attention (opt-in: MLA.predict_action_diff(suffix_attention="split")): mla_attn_chunk's contract with each head's key
// range cut over several workgroups, so that a sampler step's attention reads its cache with most of the chip instead of B x H x ceil(R/16)
// CUs (32 of 256 at 7B, batch 1, one action row).
//
//   mla_attn_chunk_split   launch 1: workgroup (b, h, block of 16 queries, s) runs attn_chunk_kernel's arithmetic (infer.hip) over the
//                          s-th contiguous range of the 64-key tiles and writes the un-normalised softmax state (m, l, 128 fp32 sums) of
//                          its valid query rows into the caller's workspace. launch 2: one wave per (b, h, query) merges the states in the
//                          order s = 0, 1, ..., divides once, rounds once. No counters, no atomics, no workgroup waits on another: the
//                          dependency is the kernel boundary (~1.2 us), which in-launch combines measured dearer than.
//                          splits == 1: mla_attn_chunk itself -- no workspace access, no second launch.
//   mla_attn_groups_split  the same two launches under the addressing of mla_attn_chunk_groups / mla_attn_chunk_ragged_groups (G groups of R
//                          rows behind one prefix per sample, the prefix length optionally read on the device): opt-in
//                          groups_attention="split" of the batched and N-sample calls. One split is the head form's own launch.
//   mla_attn_chunk_split_plan / _ws_bytes   pure host functions: the launcher's choice of splits, and the workspace it needs.
//
// Nothing here allocates, keeps state between calls or reads a workspace word this call did not write: graph-capturable, deterministic.
#include "common.h"
#include "attn_suffix_tile.h"
#include "../../include/mla_hip.h"              // the head forms a single split resolves to (infer.hip), and this file's own entry points

namespace {

constexpr int SP_CUS = 256;                     // the launcher plans for the MI355X's 256 CUs (no device query, no state)
constexpr int SP_STATE = 130;                   // fp32 words per (b, h, query, s): 128 sums in the first array, (m, l) in the second
constexpr int SP_CW = 4;                        // combine launch: waves (= states merged) per workgroup

struct SplitPlan { int nT, splits, tps, wgs, cwgs; long long ws_bytes; };

inline long long sp_ws_bytes(int B, int H, int R, int splits) {
  return splits > 1 ? (long long)B * H * R * splits * SP_STATE * 4 : 0;
}
// splits grows by one while launch 1 still fits one workgroup per CU (measured: a second round of workgroups costs more than it saves),
// splits < nT, and the largest range has more than SUF_NW tiles: a workgroup's time is its passes over its range, four tiles per pass, and
// cutting below one pass saves nothing but adds states to merge (measured at 9 tiles: 3 ranges 12.3 us, 4: 12.5, 9: 14.0 per launch
// pair). Every range so keeps at least 2 tiles. 1 when twice the unsplit grid no longer fits the chip.
inline SplitPlan sp_plan(int B, int H, int R, int S_kv, int cus, int forced) {
  SplitPlan p;
  const long long base = (long long)B * H * ((R + 15) / 16);
  p.nT = (S_kv + 63) / 64;
  p.splits = 1;
  if (forced > 0) p.splits = forced;
  else
    while (base * (p.splits + 1) <= cus && p.splits < p.nT && (p.nT + p.splits - 1) / p.splits > SUF_NW) ++p.splits;
  p.tps = (p.nT + p.splits - 1) / p.splits;
  const long long wgs = base * p.splits;
  p.wgs = wgs > 0x7fffffffLL ? -1 : (int)wgs;
  p.cwgs = p.splits > 1 ? (int)(((long long)B * H * R + SP_CW - 1) / SP_CW) : 0;
  p.ws_bytes = sp_ws_bytes(B, H, R, p.splits);
  return p;
}

// Launch 1 (splits > 1 only): attn_chunk_kernel's tile step (infer.hip; written out here, attn_suffix_tile.h says why) over the tile
// range [t0, t0 + cnt) of split s = blockIdx.x % splits (ranges differ by at most one tile: the first nT % splits ranges take one
// more). Wave w takes tiles t0 + w, t0 + w + 4, ... of its range; a wave whose tile lies behind the range skips the tile (it still
// meets the barriers), and the merged, un-normalised state goes to ws: sums [(b H + h) R + r][s][128], then (m, l)
// [(b H + h) R + r][s][2].
// GROUPS (mla_attn_groups_split): attn_chunk_groups_kernel's addressing (infer.hip) under the same arithmetic. The launch's "samples"
// are the B G (sample, group) pairs, S_kv arrives as S_p -- or, with prefix_len, is read from prefix_len[b] and clamped to
// [0, S_cap - G R], one value per workgroup (readfirstlane), so trip and barrier counts stay uniform -- and a group's S_p + R logical
// keys are tiled from key 0: logical key j is memory row j (j < S_p) or j + g R. ntiles then depends on the sample: a range behind the
// sample's last tile has cnt == 0, skips the loop and writes the empty state. State and output rows need no map: (b G + g) is the sample
// index of the layout above, and of the combine launch. The groups form is a kernel of its own over the same text
// (attn_split_body.inc): each keeps its argument list, and its code.
template <bool GROUPS>
struct SpRows {                                                         // memory row of logical key j: j, or behind the prefix j + g R
  int S_p, goff;
  __device__ __forceinline__ int operator()(int j) const { return j >= S_p ? j + goff : j; }
};
template <>
struct SpRows<false> {
  int S_p, goff;
  __device__ __forceinline__ int operator()(int j) const { return j; }
};

__global__ __launch_bounds__(64 * SUF_NW) void attn_chunk_split_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                       const bf16_t* __restrict__ v, bf16_t* __restrict__ o, int H, int S_kv,
                                                                       int R, long long ld, long long bs, long long ld_o, float scale,
                                                                       int splits, float* __restrict__ ws, long long nstates) {
  constexpr bool GROUPS = false;                                        // o and ld_o are the combine launch's
  constexpr int G = 1, S_cap = 0;
  const int* const prefix_len = nullptr;
#include "attn_split_body.inc"
}

// launch 1 of mla_attn_groups_split; S_kv is S_p without prefix_len
__global__ __launch_bounds__(64 * SUF_NW) void attn_groups_split_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                        const bf16_t* __restrict__ v, int G, int H, int S_kv, int R,
                                                                        long long ld, long long bs, float scale, int splits,
                                                                        float* __restrict__ ws, long long nstates,
                                                                        const int* __restrict__ prefix_len, int S_cap) {
  constexpr bool GROUPS = true;
#include "attn_split_body.inc"
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
  const uint32_t pk = (uint32_t)f2bf(O0 / L) | ((uint32_t)f2bf(O1 / L) << 16);      // the head forms' finish: one division, one rounding
  *(uint32_t*)(o + (b * R + r) * ld_o + h * 128 + lane * 2) = pk;
}

#define AL16(p) ((((uintptr_t)(p)) & 15) == 0)

inline bool sp_shape_ok(int B, int H, int R, int S_kv) { return B >= 1 && H >= 1 && R >= 1 && R <= SUF_RMAX && S_kv >= R; }

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
  if (p.splits == 1)                                                    // the head form itself: no workspace access, no second launch
    return mla_attn_chunk(q, k, v, o, B, H, head_dim, S_kv, R, ld, batch_stride, ld_o, scale, stream);
  MLA_CHECK_ARG(ws, "mla_attn_chunk_split: splits %d needs a workspace (null)", p.splits);
  MLA_CHECK_ARG(AL16(ws) && (long long)ws_bytes >= p.ws_bytes, "mla_attn_chunk_split: workspace of %lld bytes (16-B aligned) needed for splits %d, got %lld",
                p.ws_bytes, p.splits, (long long)ws_bytes);
  const long long nrows = (long long)B * H * R;
  (void)hipFuncSetAttribute((const void*)attn_chunk_split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SUF_LDS_BYTES);
  hipLaunchKernelGGL(attn_chunk_split_kernel, dim3(p.wgs), dim3(64 * SUF_NW), SUF_LDS_BYTES, stream, (const bf16_t*)q, (const bf16_t*)k,
                     (const bf16_t*)v, (bf16_t*)o, H, S_kv, R, ld, batch_stride, ld_o, scale, p.splits, (float*)ws, nrows * p.splits);
  hipLaunchKernelGGL(attn_split_combine_kernel, dim3(p.cwgs), dim3(64 * SP_CW), 0, stream, (const float*)ws, (bf16_t*)o, H, R, ld_o, p.splits, nrows);
  MLA_LAUNCH_CHECK();
}

// mla_attn_chunk_groups' (prefix_len == nullptr: B == 1, S_p_or_cap = S_p) or mla_attn_chunk_ragged_groups' contract with the split of
// mla_attn_chunk_split per (sample, group). Plan and workspace are mla_attn_chunk_split's at (B G, H, R, S_max), S_max the most logical keys
// a group can have: the grid, the LDS and the workspace do not depend on the lengths in device memory.
extern "C" int mla_attn_groups_split(const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim,
                                     const int* prefix_len, int S_p_or_cap, int R, long long ld, long long batch_stride, long long ld_o,
                                     float scale, int splits, void* ws, size_t ws_bytes, hipStream_t stream) {
  const bool ragged = prefix_len != nullptr;
  MLA_CHECK_ARG(q && k && v && o, "mla_attn_groups_split: null pointer");
  MLA_CHECK_ARG(head_dim == 128, "mla_attn_groups_split: head_dim must be 128 (got %d)", head_dim);
  MLA_CHECK_ARG(B >= 1 && G >= 1 && H >= 1 && R >= 1 && R <= SUF_RMAX, "mla_attn_groups_split: B >= 1, G >= 1, 1 <= R <= 64 required (B %d, G %d, R %d)",
                B, G, R);
  MLA_CHECK_ARG((long long)B * G * R <= 0x7fffffffLL, "mla_attn_groups_split: B * G * R output rows exceed the int range (B %d, G %d, R %d)", B, G, R);
  long long smax;
  if (ragged) {
    MLA_CHECK_ARG((long long)G * R <= (long long)S_p_or_cap, "mla_attn_groups_split: S_cap (%d) must hold the G * R suffix rows of a sample (G %d, R %d)",
                  S_p_or_cap, G, R);
    MLA_CHECK_ARG(batch_stride % 8 == 0, "mla_attn_groups_split: the sample stride is not 16-B aligned");
    smax = (long long)S_p_or_cap - (long long)(G - 1) * R;
  } else {
    MLA_CHECK_ARG(B == 1, "mla_attn_groups_split: one sample without prefix_len (B %d)", B);
    MLA_CHECK_ARG(S_p_or_cap >= 0, "mla_attn_groups_split: S_p >= 0 required (S_p %d)", S_p_or_cap);
    MLA_CHECK_ARG((long long)S_p_or_cap + (long long)G * R <= 0x7fffffffLL, "mla_attn_groups_split: S_p + G * R rows exceed the int range (G %d, R %d, S_p %d)",
                  G, R, S_p_or_cap);
    smax = (long long)S_p_or_cap + R;
  }
  MLA_CHECK_ARG(AL16(q) && AL16(k) && AL16(v) && ld % 8 == 0 && ld_o % 2 == 0 && (((uintptr_t)o) & 3) == 0,
                "mla_attn_groups_split: 16-B aligned rows required");
  const int S_max = (int)smax, nT = (S_max + 63) / 64;
  MLA_CHECK_ARG(splits >= 0 && splits <= nT, "mla_attn_groups_split: splits must be in [0, %d] (0 = the plan's) for at most %d keys per group, got %d", nT,
                S_max, splits);
  const SplitPlan p = sp_plan(B * G, H, R, S_max, SP_CUS, splits);
  MLA_CHECK_ARG(p.wgs > 0, "mla_attn_groups_split: grid too large (B %d, G %d, H %d, splits %d)", B, G, H, p.splits);
  if (p.splits == 1)                                                    // the head form itself: no workspace access, no second launch
    return ragged ? mla_attn_chunk_ragged_groups(q, k, v, o, B, G, H, head_dim, prefix_len, S_p_or_cap, R, ld, batch_stride, ld_o, scale, stream)
                  : mla_attn_chunk_groups(q, k, v, o, G, H, head_dim, S_p_or_cap, R, ld, ld_o, scale, stream);
  MLA_CHECK_ARG(ws, "mla_attn_groups_split: splits %d needs a workspace (null)", p.splits);
  MLA_CHECK_ARG(AL16(ws) && (long long)ws_bytes >= p.ws_bytes, "mla_attn_groups_split: workspace of %lld bytes (16-B aligned) needed for splits %d, got %lld",
                p.ws_bytes, p.splits, (long long)ws_bytes);
  const long long nrows = (long long)B * G * H * R;
  (void)hipFuncSetAttribute((const void*)attn_groups_split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SUF_LDS_BYTES);
  hipLaunchKernelGGL(attn_groups_split_kernel, dim3(p.wgs), dim3(64 * SUF_NW), SUF_LDS_BYTES, stream, (const bf16_t*)q, (const bf16_t*)k,
                     (const bf16_t*)v, G, H, ragged ? 0 : S_p_or_cap, R, ld, ragged ? batch_stride : 0LL, scale, p.splits, (float*)ws,
                     nrows * p.splits, prefix_len, ragged ? S_p_or_cap : 0);
  hipLaunchKernelGGL(attn_split_combine_kernel, dim3(p.cwgs), dim3(64 * SP_CW), 0, stream, (const float*)ws, (bf16_t*)o, H, R, ld_o, p.splits, nrows);
  MLA_LAUNCH_CHECK();
}
