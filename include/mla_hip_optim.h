/* mla_hip_optim.h -- sibling of mla_hip.h: the entry points of libmla_hip.so added after the ABI pin (the optimizer's, and the
 * DPM-Solver++(2M) sampler step).
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

/* ---- Skip the optimizer step on a non-finite gradient norm (opt-in; no counterpart in the reference: clip_grad_norm_ with
 * error_if_nonfinite=False followed by torch.optim.AdamW lets the NaN through) ----
 * mla_clip_coef plus a device-side verdict. Finite sumsq[0]: coef[0] and norm_out[0] are bit for bit what mla_clip_coef writes and
 * skip[0] = 0. sumsq[0] = +inf or NaN (exponent bits all ones; a finite gradient whose sum of squares overflows fp32 counts too):
 * skip[0] = 1, coef[0] = 0, norm_out[0] = sqrt(sumsq[0]), the non-finite norm itself, for the log. norm_out may be NULL.
 * One thread, ordinary stores. Returns -1 (nothing launched) for a null sumsq, coef or skip. */
int mla_clip_coef_guard(const float* sumsq, float max_norm, float* coef, float* norm_out, int* skip, mla_stream_t stream);

/* Every form of the AdamW pass behind the verdict above: moments_bf16 = 0: m, v fp32 [n] (mla_adamw_step_groups, or
 * mla_adamw_ema_step_groups with ema != NULL; seed and index_base are unused); moments_bf16 = 1: m, v bf16 [n]
 * (mla_adamw_m16_step). ema: fp32 [n] or NULL; p16: bf16 [n] or NULL; elements [0, n_decay) are weight-decayed.
 * skip: one int on the device, read ONCE by every workgroup before anything else (a wave-uniform load). skip[0] != 0: the launch
 * returns without reading or writing p, g, m, v, ema, p16 or grad_scale -- the step did not happen. skip[0] == 0: every output is
 * bit for bit that of the entry point named above for the same arguments (the guarded kernels are further instances of the same
 * two templates; 16-byte or scalar kernel by the same alignment / n_decay / index_base rules, the n % 4 tail through the scalar one).
 * Bias corrections are formed in double on the host. Returns -1 (nothing launched) for what mla_adamw_m16_step refuses (null p / g
 * / m / v, n < 0, step < 1, n_decay outside [0, n], index_base < 0, with ema a factor outside [0, 1] or NaN), a null skip, or
 * moments_bf16 outside {0, 1}. n == 0 is a valid no-op. */
int mla_adamw_guard_step(float* p, const float* g, void* m, void* v, float* ema, void* p16, long long n, long long n_decay, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale, float ema_decay,
                         float ema_one_minus_decay, int moments_bf16, unsigned long long seed, long long index_base, const int* skip,
                         mla_stream_t stream);

/* ---- DPM-Solver++(2M) step of the device-resident sampler loop (opt-in solver="dpmpp2m"; no counterpart in the reference, whose only
 * deterministic solver is first-order DDIM; mla_amd/csrc/sampler.hip, mla_amd/infer.py _CachedEpsBase.sample_dpmpp2m) ----
 * mla_ddim_step's form and counter protocol (mla_hip.h) for the second-order multistep solver on the respaced process. s = *step; for
 * 0 <= s < steps, with coef[s] = {a, b, kx, k0, k1} ([steps, 5] fp32, GaussianDiffusion.dpmpp2m_tables: a, b as in mla_ddim_step's
 * table, kx, k0, k1 formed in double and rounded once) and hist [n] fp32, the previous step's x0 prediction:
 *   ax = a x; be = b eps; D = ax - be; t0 = kx x; t1 = k0 D; t2 = k1 hist; x = (t0 + t1) + t2; hist = D,
 * every operation rounded on its own (no FMA contraction): the bits of GaussianDiffusion.dpmpp2m_sample_loop. D is mla_ddim_step's x0
 * prediction bit for bit. x [n] fp32 and hist [n] fp32 are updated in place, eps [n] bf16, x_bf16 [n] = bf16_rne(x) is written; with
 * `advance` the counter then becomes s - 1 (thread 0, behind a workgroup barrier). Any other s: nothing is written (hist included),
 * the counter stays. hist is always read, also where k1 = 0 (the first step): the caller zeroes it in front of a loop, a stale
 * non-finite value would reach x through 0 * hist. One workgroup; 1 <= n <= 65 536.
 * mla_dpmpp2m_step_pin: the same step with known [n] fp32 and pin [n] uint8 (non-zero = pinned): D = pin[i] ? known[i] : D right behind
 * D = ax - be, in front of every use of D and of the store into hist -- the bits of the host loop with denoised_fn =
 * where(pin, known, D). pin all zero: the bits of mla_dpmpp2m_step. At the last step (s = 0: kx = 0, k0 = 1, k1 = 0) a pinned
 * x == known for finite x, eps and hist.
 * Stateless, no allocation, no host access, on `stream`, graph-capturable. Return -1 (nothing launched) for a null pointer (known and
 * pin count for the pinned form only), n outside [1, 65 536] or steps < 1. */
int mla_dpmpp2m_step(float* x, const void* eps, void* x_bf16, float* hist, const float* coef, int* step, int n, int steps, int advance,
                     mla_stream_t stream);
int mla_dpmpp2m_step_pin(float* x, const void* eps, void* x_bf16, float* hist, const float* coef, const float* known,
                         const unsigned char* pin, int* step, int n, int steps, int advance, mla_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MLA_HIP_OPTIM_H */
