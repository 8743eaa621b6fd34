// What the cached-prefix sampler's suffix-attention kernels share: attn_chunk_kernel / attn_chunk_groups_kernel (infer.hip) and
// attn_chunk_split_kernel / attn_groups_split_kernel (attn_split.hip, one text: attn_split_body.inc). Every form's contract is bit
// identity with attn_chunk_kernel: they differ in how a logical key maps to a memory row, in which tiles a wave visits and in what
// happens to the merged state.
//
// One workgroup is SUF_NW waves; wave w takes key tiles of 64 in turn, each with its own online softmax (running max / sum per query,
// exp2 with the scale folded in); the waves' states are merged in a fixed order at the end, so LDS does not grow with S_kv. The forward
// flash kernel's fragment layout: S^T = K Q^T (K rows straight from global memory into the A fragments, Q in registers as the B
// fragments), P^T packed from the score registers as they are (attention.hip's pack_frag key order), O^T = V^T P^T with V^T read from
// a per-wave LDS transpose of the 64-row V tile. Lane l = 16 g + li owns query li of the block: the softmax needs two cross-lane steps
// per tile.
//
// Shared here: the launch constants and the fragment casts. NOT shared: the tile step itself (Q load, K / V loads, QK MFMAs, mask,
// online softmax, P packing, V-transpose store, PV MFMAs, wave merge) stays written out three times -- the two kernels of infer.hip
// and attn_split_body.inc. As inlined functions it keeps the bits but compiles to slower loops
// (profiles/suffix_attn_one_tile_step.txt). Whoever changes one copy changes all three; the torch.equal tests between the forms and
// tools/exp_suffix_attn_bits.py, which compares and times two builds, notice a missed one.
#pragma once
#include "common.h"

constexpr int SUF_RMAX = 64;                                           // query rows per sample (four blocks of 16)
constexpr int SUF_NW = 4;                                              // waves per workgroup
constexpr int SUF_VP = 68;                                             // V^T row pitch in keys (136 B: 8-B aligned, staggered banks)
constexpr size_t SUF_LDS_BYTES = (size_t)SUF_NW * 128 * SUF_VP * 2;    // the waves' V^T slabs; >= the merge buffers ([4][128][17] + 128 floats)

__device__ __forceinline__ bf16x8_t as_frag(const u32x4_t v) { return __builtin_bit_cast(bf16x8_t, v); }
__device__ __forceinline__ bf16x8_t pack_pfrag(const f32x4_t lo, const f32x4_t hi) {
  u32x4_t u;
  u[0] = pack2bf(lo[0], lo[1]); u[1] = pack2bf(lo[2], lo[3]);
  u[2] = pack2bf(hi[0], hi[1]); u[3] = pack2bf(hi[2], hi[3]);
  return as_frag(u);
}
