/* mla_hip_optim.h -- sibling of mla_hip.h: the optimizer entry points of libmla_hip.so added after the ABI pin.
 *
 * Why a second header: tests/test_abi.py pins the SET of symbols derived from include/mla_hip.h to the 153 names of
 * tests/golden/abi_signatures.json (the binding the hand-written ctypes tables gave, kept as the record of that hand-over). A new
 * entry point declared there would change the pinned set, so new optimizer entry points are declared here instead. This header is
 * treated exactly like the first: build.sh force-includes it into every translation unit (a declaration that disagrees with its
 * extern "C" definition is a compile error, an object older than it is rebuilt), mla_amd/hip.py derives a second ctypes table
 * from it with mla_amd/abi.py, and lib() sets argtypes and restypes from both. No name may be declared in both headers
 * (tests/test_abi_optim.py). The contract of mla_hip.h (caller-owned buffers, launch-only on `stream`, return codes) holds here.
 */
#ifndef MLA_HIP_OPTIM_H
#define MLA_HIP_OPTIM_H

#include "mla_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- AdamW with bf16 moments, stochastically rounded (opt-in; no counterpart in the reference: torch.optim.AdamW keeps fp32) ----
 * mla_adamw_step_groups / mla_adamw_ema_step_groups with exp_avg and exp_avg_sq stored as bf16 bit patterns: 22 B per element
 * instead of 30 (38 -> 30 with the average). m16, v16: bf16 [n], read and written; ema: fp32 [n] or NULL (no average; the two
 * factors are then ignored); p16: bf16 [n] or NULL. Elements [0, n_decay) are weight-decayed (n_decay = n: one group).
 *
 * One element: m = float(m16 << 16), v = float(v16 << 16); the update is adamw_elem of the fp32 step, every contraction as there;
 * p is updated from the UNROUNDED fp32 moments; the stored moments are rounded stochastically,
 *   m16' = sr16(m', r & 0xffff), v16' = sr16(v', r >> 16), sr16(x, r16) = (bits(x) + r16) >> 16 for finite x (a carry into the
 *   exponent is the correct round-up), round-to-nearest-even for inf / NaN,
 * which is unbiased: round-to-nearest cannot hold exp_avg_sq (bf16(0.999 v) == v, the second moment would never decay).
 * r for the element with global index e = index_base + i is word (e & 3) of Philox4x32-10 (multipliers 0xD2511F53 0xCD9E8D57, key
 * increments 0x9E3779B9 0xBB67AE85) with counter (lo32(e >> 2), hi32(e >> 2), (uint32)step, 0) and key (lo32(seed), hi32(seed)):
 * a function of (seed, step, e) alone, so one launch over [0, n) equals any split of it into consecutive launches with matching
 * index_base, and a rerun with the same seed is bit-identical.
 *
 * The 16-byte kernel (one Philox call per four elements) runs when p, g (and ema) are 16-B aligned, m16, v16, p16 8-B aligned,
 * index_base % 4 == 0 and n_decay % 4 == 0; everything else, and the n % 4 tail, goes through the scalar kernel. Both give the same
 * bits for the same e. Bias corrections are formed in double on the host, as in mla_adamw_step.
 * Returns -1 (nothing launched) for a null p / g / m16 / v16, n < 0, step < 1, n_decay outside [0, n], index_base < 0, or -- with
 * ema != NULL -- a factor outside [0, 1] or NaN. n == 0 is a valid no-op. */
int mla_adamw_m16_step(float* p, const float* g, void* m16, void* v16, float* ema, void* p16, long long n, long long n_decay,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale,
                       float ema_decay, float ema_one_minus_decay, unsigned long long seed, long long index_base, mla_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MLA_HIP_OPTIM_H */
