// The samplers' glue on the device (mla_amd/infer.py:_CachedEpsBase.sample_ddim / sample_ddpm / sample_dpmpp2m): the per-step update of the
// action chunk (DDIM at eta = 0, the DDPM posterior step with its noise read from a table the host filled beforehand, or the
// DPM-Solver++(2M) step with the previous x0 prediction kept in device memory) and the assembly of the suffix
// pass's input rows. The step index lives in device memory and is counted down by the update kernel, so a sampler step depends on
// nothing the host knows: the host enqueues `steps` replays of one captured step and reads the result.
// All kernels are stateless, allocate nothing, launch on the caller's stream and are graph-capturable.
#include "common.h"

namespace {

// GaussianDiffusion.ddim_sample at eta = 0, clip_denoised = False (models/diffusion/gaussian_diffusion.py:520-568) with the four per-step
// values coef[s] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, sqrt(alphas_cumprod_prev), sqrt(1 - alphas_cumprod_prev)}:
//   ax = a x;  px = ax - b eps;  e2 = (ax - px) / b;  x' = px c + d e2
// every product, difference, quotient and sum rounded on its own, as the sampler's one-operation-per-kernel torch expressions round them:
// the result is the host loop's, bit for bit. Contraction is switched off for the function (hipcc would fuse a x - b eps into an FMA; the
// __f*_rn spellings are plain operators in this toolchain and would be fused just the same).
// ONE workgroup: the counter is read by every thread in front of the barrier and written by thread 0 behind it.
// PIN (mla_ddim_step_pin / mla_ddpm_step_pin): the reference's denoised_fn hook (gaussian_diffusion.py:318-321) as replacement inpainting --
// px <- known[i] where pin[i], right behind px = ax - b eps and in front of everything that reads px; the rest of the step is unchanged.
// PIN = false compiles the select away and never reads known / pin (null there).
template <bool PIN>
__global__ __launch_bounds__(256) void ddim_step_kernel(float* __restrict__ x, const bf16_t* __restrict__ eps, bf16_t* __restrict__ x_bf16,
                                                        const float* __restrict__ coef, const float* __restrict__ known,
                                                        const uint8_t* __restrict__ pin, int* step, int n, int steps, int advance) {
#pragma clang fp contract(off)
  const int s = *(const volatile int*)step;
  const bool live = s >= 0 && s < steps;                                      // a stale counter never indexes outside the table
  if (live) {
    const float a = coef[4 * s + 0], b = coef[4 * s + 1], c = coef[4 * s + 2], d = coef[4 * s + 3];
    for (int i = threadIdx.x; i < n; i += 256) {
      const float e = bf2f(eps[i]);
      const float ax = a * x[i];
      const float be = b * e;
      float px = ax - be;
      if (PIN && pin[i]) px = known[i];
      const float df = ax - px;
      const float e2 = df / b;
      const float pc = px * c;
      const float de = d * e2;
      const float out = pc + de;
      x[i] = out;
      x_bf16[i] = f2bf(out);
    }
  }
  __syncthreads();
  if (live && advance && threadIdx.x == 0) *step = s - 1;
}

// GaussianDiffusion.p_sample at clip_denoised = False with the fixed-small posterior variance (models/diffusion/gaussian_diffusion.py:395-440)
// and the five per-step values coef[s] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1,
// posterior_mean_coef2, (s != 0) exp(0.5 posterior_log_variance_clipped)}, the step's normal variates in row s of noise [steps, n]:
//   ax = a x;  px = ax - b eps;  mean = c1 px + c2 x;  x' = mean + sig noise
// every operation rounded on its own, as in ddim_step_kernel (contraction off: c1 px + c2 x and mean + sig noise would become FMAs). At
// s = 0 sig is 0 and the product 0 * noise is still formed and added, as the host loop does: the sign of a zero result is the host's.
// The counter protocol and PIN are ddim_step_kernel's.
template <bool PIN>
__global__ __launch_bounds__(256) void ddpm_step_kernel(float* __restrict__ x, const bf16_t* __restrict__ eps, bf16_t* __restrict__ x_bf16,
                                                        const float* __restrict__ coef, const float* __restrict__ noise,
                                                        const float* __restrict__ known, const uint8_t* __restrict__ pin, int* step, int n,
                                                        int steps, int advance) {
#pragma clang fp contract(off)
  const int s = *(const volatile int*)step;
  const bool live = s >= 0 && s < steps;                                      // a stale counter never indexes outside the tables
  if (live) {
    const float a = coef[5 * s + 0], b = coef[5 * s + 1], c1 = coef[5 * s + 2], c2 = coef[5 * s + 3], sig = coef[5 * s + 4];
    const float* __restrict__ z = noise + (size_t)s * n;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float e = bf2f(eps[i]);
      const float xi = x[i];
      const float ax = a * xi;
      const float be = b * e;
      float px = ax - be;
      if (PIN && pin[i]) px = known[i];
      const float m1 = c1 * px;
      const float m2 = c2 * xi;
      const float mean = m1 + m2;
      const float sn = sig * z[i];
      const float out = mean + sn;
      x[i] = out;
      x_bf16[i] = f2bf(out);
    }
  }
  __syncthreads();
  if (live && advance && threadIdx.x == 0) *step = s - 1;
}

// DPM-Solver++(2M) (Lu et al. 2022, the data-prediction multistep form; no counterpart in the reference) on the respaced process, with the
// five per-step values coef[s] = {sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, kx, k0, k1} (GaussianDiffusion.dpmpp2m_tables)
// and the previous step's x0 prediction in hist [n] fp32, read and written in place:
//   ax = a x;  D = ax - b eps;  x' = (kx x + k0 D) + k1 hist;  hist <- D
// every operation rounded on its own, as in ddim_step_kernel (contraction off). D is ddim_step_kernel's px bit for bit. At the first step
// k1 is 0 and the product 0 * hist is still formed and added, as the host loop does: the loop zeroes hist at every reset, so the product
// is a zero. At s = 0 the row is {., ., 0, 1, 0}: x' is the x0 prediction. The counter protocol and PIN are ddim_step_kernel's; the pin
// replaces D in front of every use and of the store into hist. A stale counter leaves hist alone too.
template <bool PIN>
__global__ __launch_bounds__(256) void dpmpp2m_step_kernel(float* __restrict__ x, const bf16_t* __restrict__ eps, bf16_t* __restrict__ x_bf16,
                                                           float* __restrict__ hist, const float* __restrict__ coef,
                                                           const float* __restrict__ known, const uint8_t* __restrict__ pin, int* step, int n,
                                                           int steps, int advance) {
#pragma clang fp contract(off)
  const int s = *(const volatile int*)step;
  const bool live = s >= 0 && s < steps;                                      // a stale counter never indexes outside the table
  if (live) {
    const float a = coef[5 * s + 0], b = coef[5 * s + 1], kx = coef[5 * s + 2], k0 = coef[5 * s + 3], k1 = coef[5 * s + 4];
    for (int i = threadIdx.x; i < n; i += 256) {
      const float e = bf2f(eps[i]);
      const float xi = x[i];
      const float ax = a * xi;
      const float be = b * e;
      float px = ax - be;
      if (PIN && pin[i]) px = known[i];
      const float t0 = kx * xi;
      const float t1 = k0 * px;
      const float t2 = k1 * hist[i];
      const float t01 = t0 + t1;
      const float out = t01 + t2;
      x[i] = out;
      x_bf16[i] = f2bf(out);
      hist[i] = px;
    }
  }
  __syncthreads();
  if (live && advance && threadIdx.x == 0) *step = s - 1;
}

// h_in row g R <- t_table[*step], rows g R + 1 + p <- x_e[g T + p] (R = 1 + T): cat([t_e, x_e], 1).reshape(G R, H) of the sampler's
// model call, with the timestep embedding looked up instead of recomputed. One workgroup per row, 16 B per lane.
__global__ __launch_bounds__(256) void sampler_rows_kernel(bf16_t* __restrict__ h_in, const bf16_t* __restrict__ t_table,
                                                           const bf16_t* __restrict__ x_e, const int* __restrict__ step, int T, int H,
                                                           int steps) {
  const int s = *step;
  if (s < 0 || s >= steps) return;
  const int R = 1 + T, row = blockIdx.x, g = row / R, p = row - g * R;
  const bf16_t* src = p == 0 ? t_table + (size_t)s * H : x_e + ((size_t)g * T + (p - 1)) * H;
  bf16_t* dst = h_in + (size_t)row * H;
  for (int ch = threadIdx.x; ch < (H >> 3); ch += 256) *(u32x4_t*)(dst + ch * 8) = *(const u32x4_t*)(src + ch * 8);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The checks and the launch of mla_ddim_step / mla_ddim_step_pin (`who` names the export in the messages).
template <bool PIN>
int ddim_step_launch(const char* who, float* x, const void* eps, void* x_bf16, const float* coef, const float* known, const uint8_t* pin,
                     int* step, int n, int steps, int advance, hipStream_t stream) {
  MLA_CHECK_ARG(x && eps && x_bf16 && coef && step && (!PIN || (known && pin)), "%s: null pointer", who);
  MLA_CHECK_ARG(n >= 1 && n <= 65536, "%s: n = %d outside [1, 65536] (one workgroup walks the chunk)", who, n);
  MLA_CHECK_ARG(steps >= 1, "%s: steps = %d", who, steps);
  hipLaunchKernelGGL(ddim_step_kernel<PIN>, dim3(1), dim3(256), 0, stream, x, (const bf16_t*)eps, (bf16_t*)x_bf16, coef, known, pin, step, n,
                     steps, advance ? 1 : 0);
  MLA_LAUNCH_CHECK();
}

template <bool PIN>
int ddpm_step_launch(const char* who, float* x, const void* eps, void* x_bf16, const float* coef, const float* noise, const float* known,
                     const uint8_t* pin, int* step, int n, int steps, int advance, hipStream_t stream) {
  MLA_CHECK_ARG(x && eps && x_bf16 && coef && noise && step && (!PIN || (known && pin)), "%s: null pointer", who);
  MLA_CHECK_ARG(n >= 1 && n <= 65536, "%s: n = %d outside [1, 65536] (one workgroup walks the chunk)", who, n);
  MLA_CHECK_ARG(steps >= 1, "%s: steps = %d", who, steps);
  hipLaunchKernelGGL(ddpm_step_kernel<PIN>, dim3(1), dim3(256), 0, stream, x, (const bf16_t*)eps, (bf16_t*)x_bf16, coef, noise, known, pin,
                     step, n, steps, advance ? 1 : 0);
  MLA_LAUNCH_CHECK();
}

template <bool PIN>
int dpmpp2m_step_launch(const char* who, float* x, const void* eps, void* x_bf16, float* hist, const float* coef, const float* known,
                        const uint8_t* pin, int* step, int n, int steps, int advance, hipStream_t stream) {
  MLA_CHECK_ARG(x && eps && x_bf16 && hist && coef && step && (!PIN || (known && pin)), "%s: null pointer", who);
  MLA_CHECK_ARG(n >= 1 && n <= 65536, "%s: n = %d outside [1, 65536] (one workgroup walks the chunk)", who, n);
  MLA_CHECK_ARG(steps >= 1, "%s: steps = %d", who, steps);
  hipLaunchKernelGGL(dpmpp2m_step_kernel<PIN>, dim3(1), dim3(256), 0, stream, x, (const bf16_t*)eps, (bf16_t*)x_bf16, hist, coef, known, pin,
                     step, n, steps, advance ? 1 : 0);
  MLA_LAUNCH_CHECK();
}

}  // namespace

extern "C" int mla_ddim_step(float* x, const void* eps, void* x_bf16, const float* coef, int* step, int n, int steps, int advance,
                             hipStream_t stream) {
  return ddim_step_launch<false>("mla_ddim_step", x, eps, x_bf16, coef, nullptr, nullptr, step, n, steps, advance, stream);
}

extern "C" int mla_ddim_step_pin(float* x, const void* eps, void* x_bf16, const float* coef, const float* known, const unsigned char* pin,
                                 int* step, int n, int steps, int advance, hipStream_t stream) {
  return ddim_step_launch<true>("mla_ddim_step_pin", x, eps, x_bf16, coef, known, pin, step, n, steps, advance, stream);
}

extern "C" int mla_ddpm_step(float* x, const void* eps, void* x_bf16, const float* coef, const float* noise, int* step, int n, int steps,
                             int advance, hipStream_t stream) {
  return ddpm_step_launch<false>("mla_ddpm_step", x, eps, x_bf16, coef, noise, nullptr, nullptr, step, n, steps, advance, stream);
}

extern "C" int mla_ddpm_step_pin(float* x, const void* eps, void* x_bf16, const float* coef, const float* noise, const float* known,
                                 const unsigned char* pin, int* step, int n, int steps, int advance, hipStream_t stream) {
  return ddpm_step_launch<true>("mla_ddpm_step_pin", x, eps, x_bf16, coef, noise, known, pin, step, n, steps, advance, stream);
}

extern "C" int mla_dpmpp2m_step(float* x, const void* eps, void* x_bf16, float* hist, const float* coef, int* step, int n, int steps,
                                int advance, hipStream_t stream) {
  return dpmpp2m_step_launch<false>("mla_dpmpp2m_step", x, eps, x_bf16, hist, coef, nullptr, nullptr, step, n, steps, advance, stream);
}

extern "C" int mla_dpmpp2m_step_pin(float* x, const void* eps, void* x_bf16, float* hist, const float* coef, const float* known,
                                    const unsigned char* pin, int* step, int n, int steps, int advance, hipStream_t stream) {
  return dpmpp2m_step_launch<true>("mla_dpmpp2m_step_pin", x, eps, x_bf16, hist, coef, known, pin, step, n, steps, advance, stream);
}

extern "C" int mla_sampler_rows(void* h_in, const void* t_table, const void* x_e, const int* step, int G, int T, int H, int steps,
                                hipStream_t stream) {
  MLA_CHECK_ARG(h_in && t_table && x_e && step, "mla_sampler_rows: null pointer");
  MLA_CHECK_ARG(G >= 1 && T >= 1 && steps >= 1 && (long long)G * (1 + T) <= 65536, "mla_sampler_rows: G = %d, T = %d, steps = %d", G, T,
                steps);
  MLA_CHECK_ARG(H >= 8 && H % 8 == 0 && al16(h_in) && al16(t_table) && al16(x_e),
                "mla_sampler_rows: H = %d must be a multiple of 8 and the rows 16-byte aligned", H);
  hipLaunchKernelGGL(sampler_rows_kernel, dim3(G * (1 + T)), dim3(256), 0, stream, (bf16_t*)h_in, (const bf16_t*)t_table,
                     (const bf16_t*)x_e, step, T, H, steps);
  MLA_LAUNCH_CHECK();
}
