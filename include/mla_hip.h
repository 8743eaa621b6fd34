/* mla_hip.h -- C ABI of libmla_hip.so: the MI355X (gfx950) kernels behind the MLA-Llama2-7B training hot path.
 *
 * There is no FFI in the reference (ZhuoyangLiu2005/MLA is pure PyTorch + the flash_attn wheel); each entry point
 * replaces the PyTorch / flash-attn call sites cited next to it (paths relative to the reference root). The Python
 * binding a maintainer would add is shown in INTEGRATION.md and implemented in mla_amd/hip.py (ctypes).
 *
 * Contract
 *  - plain pointers + sizes only; every buffer (inputs, outputs, workspace) is allocated and owned by the caller
 *    (PyTorch); kernels never allocate, free or retain pointers past the call;
 *  - launch-only on `stream`, never synchronise, never touch the default stream; re-entrant, no global mutable state
 *    (forward runs on the main thread, backward on autograd worker threads);
 *  - return 0 on success, a negative value for argument / shape / alignment violations (checked on the host before
 *    launch), a positive hipError_t if the launch failed; mla_last_error() returns a thread-local message;
 *  - bf16 tensors are raw uint16 bit patterns, row-major, unit inner stride; statistics, losses and master gradients
 *    are fp32; indices are int64 as torch provides them (int32 where noted).
 */
#ifndef MLA_HIP_H
#define MLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mla_stream_t; /* == hipStream_t */

/* ---- library ---- */
const char* mla_last_error(void);
int mla_query(int what); /* 0: ABI version, 1: compiled gfx arch (950), 2: wavefront size (64), 3: 1 if the opt-in experiment kernels are compiled in */
/* sha256[:16] over the gemm256 kernel family's sources, stamped at build time (build.sh): bench.py compares it with the id recorded
 * next to the PMC traffic figures in profiles/ and reports roofline.traffic_stale when they differ */
const char* mla_gemm_source_id(void);
/* hardware-assumption self test (ds_read_b64_tr_b16 lane map, global_load_lds destination order) */
int mla_selftest(const void* src_1k, int* out_tr_256, void* out_glds_1k, mla_stream_t stream);
/* box calibration (bench.py's `box` block): `blocks` workgroups x 8 waves issue v_mfma_f32_16x16x32_bf16 back to back on the caller's
 * operands (512 x 24 x 8 bf16 = 196 608 bytes, 16-B aligned, e.g. N(0, 1)) for `iters` x 64 MFMAs per wave -- no LDS, no memory traffic:
 * what the matrix cores of this box sustain on random data under its power cap. out: blocks x 512 floats (sink);
 * *flops_per_launch (may be NULL) = blocks x 8 x iters x 64 x 16 384. Time it with events around the launches. */
int mla_calib_mfma(const void* operands, float* out, int blocks, int iters, double* flops_per_launch, mla_stream_t stream);
/* dispatch probe for the one-launch attention backward (mla_attn_bwd with head_sync): `blocks` workgroups of that kernel's shape each
 * take a start ticket from out[0] (caller zeroes `out`, 1 + 2 * blocks ints), stay resident ~hold_us, and record out[1 + 2 L] = ticket,
 * out[2 + 2 L] = HW_REG_XCC_ID of workgroup L. The caller decides: 8 XCDs, XCC_ID == L & 7, start order == id order per XCD. */
int mla_dispatch_probe(int* out, int blocks, int hold_us, mla_stream_t stream);

/* ---- GEMM: every nn.Linear forward / dgrad / wgrad on the path --------------------------------------------------
 * transformers/models/llama/modeling_llama.py:240 (gate/up/down), :351-353 (q/k/v), :390 (o_proj), :1254 (lm_head);
 * util/nn_utils.py:21-34; models/diffusion/models.py:112-123,173-189; models/mla/fuser/contrastive.py:173-183,208.
 * C[M,N] = alpha * sum_k Aop(m,k) Bop(n,k) (+ bias[n]) (+ R[m,n]) (+ C when accumulate).
 * a_mode/b_mode: 0 = operand stored [rows][K] (k contiguous), 1 = stored [K][rows] (reduction-major).
 * forward y = x W^T: (0,0); dgrad dx = dy W: (0,1); wgrad dW = dy^T x: (1,1). out_fp32: C is float (else bf16). */
int mla_gemm_bf16(const void* A, const void* B, void* C, const void* R, const void* bias, int M, int N, int K, int lda, int ldb,
                  int ldc, int ldr, int a_mode, int b_mode, int out_fp32, int accumulate, float alpha, int force_generic,
                  mla_stream_t stream);
/* same contract + a caller-owned scratch buffer (>= 64 MiB for full effect): the 256x256 kernel then cuts the tiles of its last,
 * partially filled round of workgroups into K-slices (fp32 partials in the workspace, fix-up pass); deterministic */
int mla_gemm_bf16_ws(const void* A, const void* B, void* C, const void* R, const void* bias, int M, int N, int K, int lda, int ldb,
                     int ldc, int ldr, int a_mode, int b_mode, int out_fp32, int accumulate, float alpha, int force_generic,
                     float* workspace, size_t workspace_bytes, mla_stream_t stream);
/* mla_gemm_bf16_ws with fp32 output (no bias / residual) that ALSO leaves sum(C^2) of the final values -- after `accumulate` -- as
 * *sq_slots partial sums in sq_out (capacity in floats >= mla_gemm_sq_slots(M, N, K, workspace_bytes)): the contribution of a
 * weight gradient to the clipping norm (training/strategies/fsdp.py:308-310) without a second pass over the fp32 gradient buffer.
 * Fixed partial order, deterministic. Shapes of the 256x256 kernel only (M, N >= 256, K % 64 == 0, N % 8 == 0): error otherwise. */
int mla_gemm_sq_slots(int M, int N, int K, size_t workspace_bytes);   /* partials the launch below writes; -1 = shape not supported */
/* Main loop of the 256x256 kernel (k-contiguous instantiations, all fused forms included, and the plain kernel on reduction-major
 * operands): 1 = hand-scheduled assembly (default; needs
 * K % 128 == 0 and the whole-row epilogue, otherwise the launch uses the other one by itself), 0 = compiler-scheduled; any other value
 * only queries. Returns the mode in force. Results are bit-identical either way -- the switch exists for A/B measurements and tests.
 * Environment MLA_GEMM_KLOOP=0 sets the initial mode. */
int mla_gemm_kloop(int mode);
/* CUs the GEMM launches plan their rounds for (split-K tail of the last, partially filled round): n >= 8 and a multiple of 8 = plan
 * for n CUs (multi-GPU runs: the CUs RCCL's kernels leave free), 0 = the device's count (default; also MLA_GEMM_CUS in the
 * environment), n < 0 = query. Returns the setting in force, -1 for a bad argument. It only changes which tiles are split along K:
 * results agree to fp32 rounding across settings and are deterministic for a given one (K-slices are summed in a fixed order). */
int mla_gemm_cus(int n);
int mla_gemm_bf16_ws_sq(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int accumulate,
                        float alpha, float* workspace, size_t workspace_bytes, float* sq_out, int sq_capacity, int* sq_slots,
                        mla_stream_t stream);
/* the same launch with the operand layouts of mla_gemm_bf16 (a_mode / b_mode 1 = stored [K][rows]): the wgrad dW = dy^T x on row-major
 * dy and x, without transposed copies of either; M % 8 == 0 / N % 8 == 0 for a reduction-major A / B */
int mla_gemm_bf16_ws_sq_rm(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int a_mode, int b_mode,
                           int accumulate, float alpha, float* workspace, size_t workspace_bytes, float* sq_out, int sq_capacity,
                           int* sq_slots, mla_stream_t stream);

/* fused q|k|v projection + rotary embedding (LlamaAttention.forward modeling_llama.py:351-361 + apply_rotary_pos_emb :184-208):
 * C[M, N] = A[M, K] B[N, K]^T in bf16 with columns [0, rope_cols) rotated per head of 128 (position = row % S, tables [S, 64]
 * fp32) in the GEMM epilogue; bit-identical to mla_gemm_bf16 followed by mla_rope_inplace. M, N >= 256, K % 64 == 0. */
int mla_gemm_qkv_rope(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, const float* rope_cos,
                      const float* rope_sin, int S, int rope_cols, mla_stream_t stream);

/* fused gate|up projection + SwiGLU (LlamaMLP.forward modeling_llama.py:240): gu[M, 2I] = x[M, K] wgu[2I, K]^T (wgu = gate rows then up
 * rows), act[M, I] = silu(gate) * up and, if actT != NULL, actT[I, ldt] = act^T, all from one GEMM launch; bit-identical to
 * mla_gemm_bf16 followed by mla_swiglu_fwd_dual. M >= 256, I % 128 == 0, K % 64 == 0. act may be NULL when actT is given (the
 * recomputation of a checkpointed layer needs the product in the wgrad layout only), gu may be NULL when act is given (the forward of a
 * checkpointed layer keeps nothing but its input). */
int mla_gemm_gateup_swiglu(const void* x, const void* wgu, void* gu, void* act, void* actT, int M, int I, int K, int lda, int ldb,
                           long long ldt, mla_stream_t stream);
/* fused down-projection dgrad + SwiGLU backward (autograd of LlamaMLP.forward modeling_llama.py:240): d(act) = dy[M, K] wT[I, K]^T is
 * consumed in the GEMM epilogue -- gate|up (gu [M, 2I]) is read there and d(gate|up) is written in both layouts, dgu [M, 2I] and
 * dguT [2I, ldt]; bit-identical to mla_gemm_bf16 followed by mla_swiglu_bwd_t. M, I >= 256, K % 64 == 0, M % 8 == 0. dguT may be NULL
 * (the wgrad then reads dgu as a reduction-major operand): the transposed strip and its LDS staging are skipped. */
int mla_gemm_dact_swiglu_bwd(const void* dy, const void* wT, const void* gu, void* dgu, void* dguT, int M, int I, int K, int lda,
                             int ldb, long long ldt, mla_stream_t stream);
/* the same launch on the down-projection weight AS STORED: w [K, I] row-major (K = hidden size, row stride ldb >= I, a reduction-major B
 * operand like b_mode 1 of mla_gemm_bf16), so the caller keeps no W^T copy. Same K order and accumulation order per output:
 * bit-identical to mla_gemm_dact_swiglu_bwd on transpose(w). Same shape contract; I % 8 == 0, ldb % 8 == 0. */
int mla_gemm_dact_swiglu_bwd_rm(const void* dy, const void* w, const void* gu, void* dgu, void* dguT, int M, int I, int K, int lda,
                                int ldb, long long ldt, mla_stream_t stream);

/* ---- RMSNorm folded into the projections (round 6): fused RMSNorm + QKV + RoPE and fused RMSNorm + gate|up + SwiGLU, one launch each.
 * LlamaRMSNorm (modeling_llama.py:76-90) feeds only projections (:351-353 q/k/v, :240 gate/up), and y W^T with y = g * (x * rstd)
 * equals rstd (.) ((x * g) W^T): the row scale commutes with the product. The GEMM that PRODUCES the residual-stream rows x
 * (LlamaDecoderLayer :744 / :750: o_proj / down_proj + residual) leaves, besides C = x, xg = bf16(x * g) with g = the NEXT norm's weight
 * and ss [M, N / 256] = one fp32 partial of sum(x^2) per row and 256-column tile (mla_gemm_res_norm; N % 256 == 0; deterministic; split-K
 * tail through `workspace` like mla_gemm_bf16_ws). The projection that CONSUMES them (the _rs forms; A = xg) multiplies its fp32
 * accumulator rows by rstd[m] = 1 / sqrt(sum_j ss[m, j] / K + eps) before the single rounding to bf16 the fused RoPE / SwiGLU epilogues
 * start from, and stores rstd [M] for the backward; with ss == NULL it reads rstd [M] instead. mla_rmsnorm_prep makes xg and rstd for rows
 * that do not come out of a GEMM (first layer, recomputation). The stand-alone norm pass disappears from the forward; the backward is
 * unchanged (it needs x and rstd only). Rounding points: x * g is rounded once where the reference rounds x * rstd and then g * that. */
int mla_gemm_res_norm(const void* A, const void* B, void* C, const void* R, const void* g, void* xg, float* ss, int M, int N, int K,
                      int lda, int ldb, int ldc, int ldr, float* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_gemm_qkv_rope_rs(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, const float* rope_cos,
                         const float* rope_sin, int S, int rope_cols, const float* ss, int parts, float eps, float* rstd,
                         mla_stream_t stream);
int mla_gemm_gateup_swiglu_rs(const void* x, const void* wgu, void* gu, void* act, void* actT, int M, int I, int K, int lda, int ldb,
                              long long ldt, const float* ss, int parts, float eps, float* rstd, mla_stream_t stream);
int mla_rmsnorm_prep(const void* x, const void* w, void* xg, float* rstd, int rows, int H, float eps, mla_stream_t stream);

/* ---- RMSNorm: LlamaRMSNorm.forward modeling_llama.py:76-90; timm RmsNorm in FinalLayer (models/diffusion/models.py:177) */
int mla_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int rows, int H, float eps, mla_stream_t stream);
/* y [rows, H] = w * bf16(x * rstd[row]) with the rstd a forward saved: the normalised input rebuilt row-major, bit for bit what
 * mla_rmsnorm_fwd wrote (the row-major twin of mla_rmsnorm_apply_t, for the wgrad on reduction-major operands). H % 8 == 0. */
int mla_rmsnorm_apply(const void* x, const void* w, const float* rstd, void* y, long long rows, int H, mla_stream_t stream);
int mla_rmsnorm_bwd_blocks(int rows);
/* dx = dres + d(rmsnorm)/dx ; dw (+)= sum_rows dy * x_hat ; workspace >= mla_rmsnorm_bwd_blocks(rows)*H floats */
int mla_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx, float* dw,
                    int dw_accumulate, int rows, int H, float* workspace, size_t workspace_bytes, mla_stream_t stream);
/* ---- timm==0.9.10 RmsNorm (FinalLayer.norm_final, models/diffusion/models.py:18,177; pin pyproject.toml:44): timm v0.9.10
 * timm/layers/fast_norm.py::rms_norm computes v = torch.var(x, dim=-1, keepdim=True) (unbiased, mean-subtracted) and returns
 * x * rsqrt(v + eps) * weight -- not the mean-of-squares norm above. mean/rstd [rows] fp32 are saved for the backward. */
int mla_timm_rmsnorm_fwd(const void* x, const void* w, void* y, float* mean, float* rstd, int rows, int H, float eps,
                         mla_stream_t stream);
/* dx = d(timm rms_norm)/dx ; dw (+)= sum_rows dy * x * rstd ; workspace >= mla_rmsnorm_bwd_blocks(rows)*H floats */
int mla_timm_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, void* dx, float* dw,
                         int dw_accumulate, int rows, int H, float* workspace, size_t workspace_bytes, mla_stream_t stream);
/* bias gradients of every nn.Linear with a bias on the path (autograd of util/nn_utils.py:21-34, models/diffusion/models.py:112-123):
 * out[n] (+)= sum_r dy[r][n]; workspace >= mla_colsum_blocks(rows)*N floats */
int mla_colsum_blocks(int rows);
int mla_colsum_bf16(const void* dy, float* out, int accumulate, int rows, int N, int ld, float* workspace, size_t workspace_bytes,
                    mla_stream_t stream);
/* nn.LayerNorm forward in the frozen vision tokenizer: models/mla/image/vision_tokenizer.py:21-24 */
int mla_layernorm_fwd(const void* x, const void* w, const void* b, void* y, int rows, int H, float eps, mla_stream_t stream);

/* ---- RoPE in place on the q and k slices of a packed qkv buffer: apply_rotary_pos_emb modeling_llama.py:184-208 */
int mla_rope_inplace(void* buf, const float* cos_t, const float* sin_t, long long tokens, int S, int nheads, int D, int ld,
                     int q_off, int k_off, int backward, mla_stream_t stream);

/* ---- SwiGLU: LlamaMLP.forward modeling_llama.py:240; gu = [gate | up] per row
 * Limit: sigmoid(gate) comes from the hardware exponential and reciprocal (1 ulp each), and the reciprocal flushes a result below 2^-126
 * to 0. For gate < -87.3 the outputs (act, dgu) are therefore exactly 0 where the exact values are of magnitude 87 x 2^-126 x up. The
 * fused GEMM epilogues share the definition (common.h) and the limit. */
int mla_swiglu_fwd(const void* gu, void* act, long long rows, int I, mla_stream_t stream);
int mla_swiglu_bwd(const void* dact, const void* gu, void* dgu, void* act_out, long long rows, int I, mla_stream_t stream);
/* ---- activations of the small heads: kind 0 GELU(erf) (MLPProjector util/nn_utils.py:21-34), 1 GELU(tanh) (timm Mlp in ActionEmbedder /
 * FinalLayer, models/diffusion/models.py:112-123,173-189), 2 ReLU (contrastive heads models/mla/fuser/contrastive.py:173-183; Point-PN
 * Point_PN.py:179,209,218), 3 SiLU (TimestepEmbedder models/diffusion/models.py:34-38) */
int mla_act_fwd(const void* x, void* y, long long n, int kind, mla_stream_t stream);
int mla_act_bwd(const void* dy, const void* x, void* dx, long long n, int kind, mla_stream_t stream);

/* ---- casts / adds / row gathers (sequence assembly of PrismaticVLM.forward models/vlm/prismatic.py:981-1038) */
int mla_cast_f32_to_bf16(const float* x, void* y, long long n, mla_stream_t stream);
int mla_cast_bf16_to_f32(const void* x, float* y, long long n, mla_stream_t stream);
int mla_add_bf16(const void* a, const void* b, void* y, long long n, mla_stream_t stream);
int mla_gather_rows_bf16(const void* src, const long long* idx, void* out, long long rows, int H, int scatter, mla_stream_t stream);

/* ---- tile transposes feeding the all-NT backward GEMMs (dx = dy W and dW = dy^T x of every Linear on the decoder path,
 * i.e. autograd of modeling_llama.py:240,351-353,390): dst[c][r] = src[r][c]; the two fused forms recompute the
 * normalised input (modeling_llama.py:85-90 with the saved rstd) / the SwiGLU product (:240) straight into [C, R]. */
int mla_transpose_bf16(const void* src, void* dst, long long R, int C, long long ld, long long ldt, mla_stream_t stream);
int mla_rmsnorm_apply_t(const void* x, const void* w, const float* rstd, void* dst, long long rows, int H, long long ldt,
                        mla_stream_t stream);
int mla_swiglu_fwd_t(const void* gu, void* dst, long long rows, int I, long long ldt, mla_stream_t stream);
/* SwiGLU forward (LlamaMLP.forward modeling_llama.py:240) writing the product in both layouts in one pass: act [rows, I] for the
 * down projection and actT [I, ldt] kept for the backward's wgrad GEMM (instead of recomputing it from gu there) */
int mla_swiglu_fwd_dual(const void* gu, void* act, void* actT, long long rows, int I, long long ldt, mla_stream_t stream);
/* SwiGLU backward writing both layouts in one pass: dgu [rows, 2I] for the dgrad GEMM and dguT [2I, ldt] for the wgrad GEMM
 * (modeling_llama.py:241 LlamaMLP backward; saves re-reading the 2I-wide gradient for a separate transpose) */
int mla_swiglu_bwd_t(const void* dact, const void* gu, void* dgu, void* dguT, long long rows, int I, long long ldt, mla_stream_t stream);

/* ---- embedding: LlamaModel.embed_tokens modeling_llama.py:975-976 (deterministic, atomics-free backward).
 * bwd: grad[ids[t]] += dy[t] in ascending token order. workspace: fp32 [tokens / 64, H] scratch or NULL; with it, every aligned
 * batch of 64 tokens that carries one id (padding) is summed first by its own workgroup and enters the walk as one row. */
int mla_embedding_fwd(const long long* ids, const void* table, void* out, long long tokens, int H, int vocab, mla_stream_t stream);
int mla_embedding_bwd(const long long* ids, const void* dy, float* grad, float* workspace, long long tokens, int H, int vocab,
                      mla_stream_t stream);

/* ---- optimizer: AdamW (training/strategies/fsdp.py:257) over the local fp32 shard + bf16 compute copy; clip (:308-310)
 * The bias corrections 1 - beta^step are formed in double on the host and cast once (as torch.optim.AdamW does); the element update is
 * fp32 with p16 = bf16(p). grad_scale (device scalar or null) multiplies g before both moments. */
int mla_adamw_step(float* p, const float* g, float* m, float* v, void* p16, long long n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, const float* grad_scale, mla_stream_t stream);
/* the same update over a flat range laid out [weight-decayed | not decayed]: elements [0, n_decay) get weight_decay, the rest none --
 * both AdamW parameter groups of a sharding unit (training/strategies/fsdp.py:231-257) in one launch */
int mla_adamw_step_groups(float* p, const float* g, float* m, float* v, void* p16, long long n, long long n_decay, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int step, const float* grad_scale, mla_stream_t stream);
/* ---- weight average (EMA) of the fp32 masters (update_ema, training/strategies/base_strategy_mla.py:33-41: ema.mul_(decay).add_(param,
 * alpha=1 - decay)). The two steps above with one more fp32 stream ema [n]: after the update, ema = ema_one_minus_decay * p_new +
 * ema_decay * ema, the product rounded and the sum one fma, on the fp32 master (never the bf16 copy). p, m, v, p16 come out as from
 * the plain step, bit for bit. The caller forms both factors: decay cast to fp32, 1 - decay formed in double and cast once (the
 * convention of the bias corrections above). ema == NULL, n < 0 or a factor outside [0, 1]: invalid argument, never a plain step. */
int mla_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, void* p16, long long n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, const float* grad_scale, float ema_decay,
                       float ema_one_minus_decay, mla_stream_t stream);
int mla_adamw_ema_step_groups(float* p, const float* g, float* m, float* v, float* ema, void* p16, long long n, long long n_decay, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale,
                              float ema_decay, float ema_one_minus_decay, mla_stream_t stream);
/* the same average as a pass of its own, for weights held outside the optimizer: ema = one_minus_decay * p + decay * ema over fp32 [n] */
int mla_ema_update(float* ema, const float* p, long long n, float decay, float one_minus_decay, mla_stream_t stream);
int mla_sumsq_f32(const float* x, long long n, float* out, int accumulate, float* workspace, size_t workspace_bytes,
                  mla_stream_t stream);
/* out[0] (+)= sum(partial[0 .. n)), fixed order: second stage of the gradient norm over mla_gemm_bf16_ws_sq partials */
int mla_sum_partials(const float* partial, int n, float* out, int accumulate, mla_stream_t stream);
int mla_clip_coef(const float* sumsq, float max_norm, float* coef, float* norm_out, mla_stream_t stream);

/* ---- diffusion: GaussianDiffusion.q_sample models/diffusion/gaussian_diffusion.py:214-229 */
int mla_q_sample(const float* x0, const float* noise, const long long* t, const float* sqrt_ac, const float* sqrt_1mac, float* out,
                 int batch, int per, int nsteps, mla_stream_t stream);

/* ---- causal attention (replaces flash_attn 2.5.5: modeling_llama.py:420-597; math :371-380). head_dim 128.
 * q/k/v: first element of each slice of the packed [B*S, ld_qkv] buffer; o / dout: [B*S, ld_o]; lse, delta: [B,H,S].
 * seqlens (int32 [B] or NULL): right-padded rows q >= seqlens[b] give zero output / zero gradients. */
int mla_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int* seqlens, int B, int S, int H,
                 int head_dim, long long ld_qkv, long long ld_o, float scale, mla_stream_t stream);
/* Shared-prefix sequences (round 6, opt-in; models/mla/model_mla.py:148-180 tiles every sample R times although, without a point cloud,
 * the R copies differ only in their last rows [t, x, </s>]): one sequence [prefix | R suffix groups of grp_len rows]. Rows >= grp_start
 * belong to group (row - grp_start) / grp_len; a query attends to the prefix and, causally, to its OWN group. The RoPE positions of the
 * suffix rows come from the caller's tables (row s of rope_cos / rope_sin is the table row of position pos(s)). grp_len == 0: plain causal.
 * grp_starts (int32 [B] on the device, or NULL): a first suffix row per sample for ragged prompts (valid rows of sample b: [0, seqlens[b])).
 * mla_attn_bwd_g = mla_attn_bwd_t (transposed copies and head_sync optional) with the same grouping; rope_per_sample = 1: the tables are
 * [B * S, 64], one block of S rows per sample (per-sample positions), instead of one [S, 64] table. */
int mla_attn_fwd_g(const void* q, const void* k, const void* v, void* o, float* lse, const int* seqlens, int B, int S, int H,
                   int head_dim, long long ld_qkv, long long ld_o, float scale, int grp_start, int grp_len, const int* grp_starts,
                   mla_stream_t stream);
int mla_attn_bwd_g(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, const int* seqlens,
                   void* dq, void* dk, void* dv, float* delta, int B, int S, int H, int head_dim, long long ld_qkv, long long ld_o,
                   float scale, const float* rope_cos, const float* rope_sin, void* dqT, void* dkT, void* dvT, void* oT,
                   long long ldt, int* head_sync, long long head_sync_ints, int grp_start, int grp_len, const int* grp_starts,
                   int rope_per_sample, mla_stream_t stream);
/* rope_cos / rope_sin ([S, 64] fp32, both or neither): when given, dq and dk are written with the backward of apply_rotary_pos_emb
 * (modeling_llama.py:184-208) already applied -- the same values mla_rope_inplace(backward = 1) would produce on them afterwards.
 * Launch form (mla_attn_bwd and mla_attn_bwd_t; results are bit-identical either way): with head_sync == NULL the dQ kernel and the
 * dK / dV kernel are two launches. With head_sync given, ONE launch runs both block types and the dQ blocks hand delta to the dK / dV
 * blocks of their head through two integer counters per head IN THE CALLER'S BUFFER: head_sync = mla_attn_bwd_sync_ints(B, H) ints
 * (4-B aligned), zero before the first call; every launch leaves it zero again (the last consumer of a head resets its pair), so one
 * buffer serves any sequence of shapes on a stream and a captured launch replays correctly. One buffer per stream in flight. The
 * library allocates nothing and keeps nothing. The one-launch form assumes workgroup id L runs on XCD L & 7 and that workgroups
 * start in id order per XCD (mla_dispatch_probe measures both; mla_amd/hip.py passes head_sync only on a device where they hold); a
 * wait that lasts 30 s of wall clock traps. MLA_ATTN_BWD_MERGED=0 forces two launches whatever is passed.
 * `delta` is written by the call and only meaningful after it has completed. */
long long mla_attn_bwd_sync_ints(int B, int H);
int mla_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, const int* seqlens,
                 void* dq, void* dk, void* dv, float* delta, int B, int S, int H, int head_dim, long long ld_qkv, long long ld_o,
                 float scale, const float* rope_cos, const float* rope_sin, int* head_sync, long long head_sync_ints,
                 mla_stream_t stream);
/* mla_attn_bwd + token-contiguous copies dqT / dkT / dvT / oT [H * head_dim, ldt] (column = b * S + s; columns >= B * S untouched)
 * of dq / dk / dv / o: the k-contiguous operands of the q|k|v and o projection wgrad GEMMs (autograd of modeling_llama.py:371-380),
 * written from the registers that hold the rows instead of by four transpose passes. All four or none; S % 4 == 0, ldt % 4 == 0. */
int mla_attn_bwd_t(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, const int* seqlens,
                   void* dq, void* dk, void* dv, float* delta, int B, int S, int H, int head_dim, long long ld_qkv, long long ld_o,
                   float scale, const float* rope_cos, const float* rope_sin, void* dqT, void* dkT, void* dvT, void* oT,
                   long long ldt, int* head_sync, long long head_sync_ints, mla_stream_t stream);
/* Five-product form of the backward -- an EXPERIMENT kernel (measured no faster than the seven-product pair on MI355X):
 * compiled only into the experiment build (build.sh MLA_EXPERIMENTAL=1, mla_query(3) == 1); the product library exports the symbol
 * and rejects the call with a negative code.
 * the dK / dV kernel hands dS^T to a one-product dQ kernel through the
 * caller-owned workspace `ws` (mla_attn_bwd_ws_bytes(B, S, H) bytes, 16-B aligned) instead of both kernels recomputing Q K^T and
 * dO V^T; delta = rowsum(O o dO) is its own pass. Same outputs and argument meaning as mla_attn_bwd_t (dqT / dkT / dvT / oT: all or
 * none); deterministic (no atomics). Replaces the flash-attn backward behind modeling_llama.py:531-553. */
long long mla_attn_bwd_ws_bytes(int B, int S, int H);
int mla_attn_bwd_ws(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, const int* seqlens,
                    void* dq, void* dk, void* dv, float* delta, int B, int S, int H, int head_dim, long long ld_qkv, long long ld_o,
                    float scale, const float* rope_cos, const float* rope_sin, void* dqT, void* dkT, void* dvT, void* oT, long long ldt,
                    void* ws, long long ws_bytes, mla_stream_t stream);

/* ---- inference with a cached prefix (mla_amd/infer.py; replaces 7 of the 8 whole forwards of MLA.predict_action_diff,
 * models/mla/model_mla.py:742-775 + models/diffusion/gaussian_diffusion.py:608-688). HBM-bound: algorithmic bytes = the weight matrix /
 * the head's cached K and V rows.
 * mla_gemv_bf16: out row m = x[m] . W^T (+ residual[m]) for M <= 8 rows; W [N, K] k-contiguous is read exactly once (16 B per lane,
 *   non-temporal), x is held in LDS (M x K x 2 bytes <= 160 KiB), fp32 accumulation. Row m of `out` is written at
 *   out + (m / rows_per_batch) * out_batch_stride + (m % rows_per_batch) * ldo, so the q|k|v rows of the new tokens can land directly in
 *   the per-sample cache slots. Replaces the nn.Linear calls of modeling_llama.py:240, 351-353, 390 for the suffix rows.
 *   pre: what is applied to the input rows on their way into LDS -- 0 nothing; 1 LlamaRMSNorm with weight pre_w and eps
 *   (modeling_llama.py:76-90, the arithmetic of mla_rmsnorm_fwd); 2 SwiGLU: x rows are packed gate|up [2 K], the input is
 *   silu(gate) * up (modeling_llama.py:240, the arithmetic of mla_swiglu_fwd).
 *   rope_cos / rope_sin ([rows_per_batch, 64] fp32, both or neither; no residual then): columns [0, rope_cols) are rotated per head of
 *   128 in the epilogue (apply_rotary_pos_emb modeling_llama.py:184-208, the arithmetic of mla_rope_inplace on the bf16-rounded
 *   projection; row m uses table row m % rows_per_batch) -- with pre = 1 this is north_star's "fused RMSNorm + RoPE + QKV" as ONE kernel,
 *   on the inference path. */
int mla_gemv_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                  int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre, const void* pre_w, float eps,
                  const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
/* mla_attn_decode: R <= 8 new query rows per (sample, head) -- rows [S_kv - R, S_kv) of the packed q|k|v cache (row stride ld, sample stride
 *   batch_stride, q / k / v = the three slices' first elements) -- against keys / values [0, S_kv - R + r] (causal, scale applied to the
 *   scores, fp32 softmax, P rounded to bf16 before P V like the flash kernel). o: [B * R, H * 128] bf16. head_dim 128.
 *   Replaces the attention of modeling_llama.py:371-380 for the suffix rows. */
int mla_attn_decode(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, int S_kv, int R, long long ld,
                    long long batch_stride, long long ld_o, float scale, mla_stream_t stream);
/* mla_gemm_skinny_bf16: mla_gemv_bf16's contract (same arguments, output addressing, pre modes and RoPE epilogue) for 1 <= M <= 64 rows
 *   and any K % 8 == 0: W is read exactly once (16 B per lane, non-temporal, straight into the A operands of v_mfma_f32_16x16x32_bf16),
 *   the x rows are the B operands (read per 16-row W tile, nothing staged: LDS does not grow with K), fp32 accumulation. Deterministic:
 *   every output is one fixed-order sum of the K-range partials of 8 waves, no atomics, no workspace. With pre = 1 / 2 the operand values
 *   are bit for bit what mla_rmsnorm_fwd / mla_swiglu_fwd write. The suffix pass of an action chunk of 8 .. 63 rows. */
int mla_gemm_skinny_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                         int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre, const void* pre_w, float eps,
                         const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
/* ---- weight-only FP8 for the suffix projections (opt-in: MLA.predict_action_diff(suffix_weights="fp8")). Format: per row n of W [N, K],
 *   amax[n] = max_k |W[n, k]|, scale[n] = amax[n] / 448.0f (1.0f when amax[n] == 0), q[n, k] = e4m3fn_rne(clamp(float(W[n, k]) / scale[n],
 *   -448, 448)): OCP e4m3fn bytes (gfx950's format; NOT MI300's e4m3fnuz) and fp32 scales [N]. Both divisions are correctly rounded fp32
 *   divisions, so (W.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn) on the CPU reproduces the bytes.
 * mla_quant_fp8_rows: W [N, K] bf16 (row stride ldw elements) -> q [N, K] bytes (row stride ldq bytes) + scale [N]. K % 16 == 0, 16-B aligned
 *   rows. One workgroup per row (row absmax, then encode), deterministic, no workspace, no atomics, no allocation. Non-finite input is NOT
 *   supported (finite input never produces a NaN code: the clamp is in front of the conversion). Runs once per weight version.
 * mla_gemv_w8 / mla_gemm_skinny_w8: mla_gemv_bf16 / mla_gemm_skinny_bf16 -- the same argument meaning, rows_per_batch / out_batch_stride
 *   addressing, pre modes 0 / 1 / 2 (bit for bit the operand values of mla_rmsnorm_fwd / mla_swiglu_fwd), residual and q|k rotary epilogue
 *   -- with W [N, K] e4m3fn bytes (ldw in elements = bytes, 16-B aligned rows) and w_scale [N] fp32. K % 16 == 0; M <= 8 with the bf16 x
 *   rows in LDS (gemv) resp. 1 <= M <= 64 (skinny). Arithmetic: fp32 sum of x[m, k] * float(q[n, k]) over the UNSCALED codes (every e4m3
 *   value is a bf16 value: decoding is exact), the finished sum times w_scale[n], then the residual add or the rotation, one bf16 rounding;
 *   no scale touches a partial sum. Half the weight bytes of the bf16 forms per call: 16 weights per 16-B load, decoded in registers
 *   (v_cvt_pk_f32_fp8 in the gemv, v_cvt_scalef32_pk_bf16_fp8 into the MFMA A fragments in the skinny form, whose k order inside a
 *   64-wide step differs from the bf16 kernel's). Fixed-order sums, no atomics, graph-capturable. */
int mla_quant_fp8_rows(const void* W, long long ldw, void* q, long long ldq, float* scale, int N, int K, mla_stream_t stream);
int mla_gemv_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre,
                const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
int mla_gemm_skinny_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                       long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre,
                       const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
/* mla_gemm_skinny_gateup_swiglu_bf16 / _w8: the gate|up projection of 1 <= M <= 64 rows with SwiGLU in the epilogue (opt-in:
 *   MLA.predict_action_diff(suffix_operand="once")). x [M, K] bf16 (ldx); W [2 I, K] the packed gate|up matrix, gate rows [0, I), up rows
 *   [I, 2 I), bf16 or e4m3fn bytes with w_scale [2 I]; out [M, I] bf16 (ldo >= I):
 *     out[m, n] = bf16(silu(g) * u),  g = bf16(x[m] . W[n]),  u = bf16(x[m] . W[I + n])   (W8: each fp32 sum times its own row's scale first)
 *   Workgroup t holds gate rows 8 t .. 8 t + 7 and up rows I + 8 t .. I + 8 t + 7 as one 16-row tile; K split, MFMA order and the
 *   fixed-order sum of the 8 wave partials are mla_gemm_skinny_*'s, so the result is bit for bit mla_swiglu_fwd of the plain form's
 *   [M, 2 I] output, which never reaches memory. No residual, no rotary epilogue, no pre-transform; no atomics, no workspace,
 *   graph-capturable. I % 8 == 0, K % 8 == 0 (bf16) / K % 16 == 0 (w8), 16-B aligned rows; otherwise -1 and nothing is launched. */
int mla_gemm_skinny_gateup_swiglu_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, int M, int I,
                                       int K, mla_stream_t stream);
int mla_gemm_skinny_gateup_swiglu_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out,
                                     long long ldo, int M, int I, int K, mla_stream_t stream);
/* ---- weight-only MXFP4 for the suffix projections (opt-in: MLA.predict_action_diff(suffix_mx="fp4")). Format (OCP MXFP4), for W [N, K]
 *   bf16 with K % 32 == 0: codes q [N, K / 2] bytes, element 2 j in the low nibble of byte j and element 2 j + 1 in the high one, nibble =
 *   sign (8) | index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}; scales s [N, K / 32] bytes, one e8m0 byte per block of 32 consecutive k of a row,
 *   byte = e + 127 with e = clamp(floor(log2(block amax)) - 2, -125, 125) taken from the exponent bits (127 and all codes +0 for an
 *   all-zero block; 255 is never written). |w| / 2^e is rounded to the nearest grid value, ties to the even mantissa bit (0.25 -> 0,
 *   0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating at 6; the sign is kept. Blocks never cross rows, so packed
 *   q|k|v and gate|up matrices quantise as one.
 * mla_quant_mxfp4_rows: W [N, K] bf16 (row stride ldw elements) -> q (row stride ldq bytes, 16-B aligned rows, ldq >= K / 2) + s (row
 *   stride lds bytes >= K / 32). One workgroup per row, one thread per block, integer work on the bf16 bits: deterministic, no workspace,
 *   no atomics. Non-finite input is NOT supported. Runs once per weight version.
 * mla_gemv_w4 / mla_gemm_skinny_w4 / mla_gemm_skinny_gateup_swiglu_w4 / mla_gemm_suffix_w4 / mla_gemm_suffix_w4_pos: the `_w8` entry
 *   points' contracts, argument checks and epilogues with W = the code bytes (ldw in BYTES, ldw % 16 == 0, ldw >= K / 2), w_scale = the
 *   scale bytes and ld_scale their row stride (>= K / 32). K % 32 == 0. The codes are decoded WITH their block scale in registers
 *   (v_cvt_scalef32_pk_f32_fp4 in the gemv, v_cvt_scalef32_pk_bf16_fp4 into the MFMA A fragments): every e2m1 value has two significant
 *   bits and the scale is a power of two, so the decode is exact in bf16 and out = the bf16 kernels on the dequantised matrix up to
 *   summation order -- no scale multiply behind the sum, no new rounding point; residual, rotary and SwiGLU epilogues are the bf16 forms'.
 *   The MFMA forms keep the `_w8` kernels' 64-wide K steps, wave split and summation order (a lane's 16 codes are 8 B inside one scale
 *   block), so every 64-row slice of mla_gemm_suffix_w4 is bit for bit mla_gemm_skinny_w4's output and the gate|up form is
 *   mla_swiglu_fwd of the plain form's output. A quarter of the bf16 forms' weight bytes per call (+ 1 / 16 of that in scales). */
int mla_quant_mxfp4_rows(const void* W, long long ldw, void* q, long long ldq, void* s, long long lds, int N, int K, mla_stream_t stream);
int mla_gemv_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out, long long ldo,
                long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, int pre,
                const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
int mla_gemm_skinny_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                       long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N,
                       int K, int pre, const void* pre_w, float eps, const float* rope_cos, const float* rope_sin, int rope_cols,
                       mla_stream_t stream);
int mla_gemm_skinny_gateup_swiglu_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale,
                                     void* out, long long ldo, int M, int I, int K, mla_stream_t stream);
int mla_gemm_suffix_w4(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                       long long ldo, long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                       long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                       mla_stream_t stream);
int mla_gemm_suffix_w4_pos(const void* x, long long ldx, const void* W, long long ldw, const void* w_scale, long long ld_scale, void* out,
                           long long ldo, long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                           long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                           const int* rope_pos, int rope_rows, mla_stream_t stream);
/* mla_attn_chunk: mla_attn_decode's contract for 1 <= R <= 64 query rows and any S_kv >= R: online softmax over key tiles of 64 (LDS does
 *   not grow with S_kv), QK^T and PV on the MFMA pipe, P rounded to bf16 before P V like the flash kernel; the key tiles are shared out
 *   over 4 waves per (sample, head, 16 queries) and their softmax states merged in a fixed order (deterministic, graph-capturable). */
int mla_attn_chunk(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, int S_kv, int R, long long ld,
                   long long batch_stride, long long ld_o, float scale, mla_stream_t stream);
/* ---- batched action sampling (mla_amd/infer.py BatchedPrefixCachedEps): B observations with prompts of different lengths on ONE
 * cached-prefix pass. The per-sample lengths are DEVICE arrays, so a captured graph serves any mix of lengths.
 * mla_attn_chunk_ragged: mla_attn_chunk with the key count of sample b read from kv_len[b] (int32 [B] on the device, clamped to
 *   [R, S_cap]; S_cap = rows per sample the caller owns): the R queries of sample b are cache rows [kv_len[b] - R, kv_len[b]), query r
 *   sees keys [0, kv_len[b] - R + r]. Same grid, same LDS (independent of the lengths), same fixed-order merge: the output rows of
 *   sample b are bit for bit those of mla_attn_chunk with B = 1 and S_kv = kv_len[b] on that sample's rows. */
int mla_attn_chunk_ragged(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, const int* kv_len, int S_cap,
                          int R, long long ld, long long batch_stride, long long ld_o, float scale, mla_stream_t stream);
/* mla_gemm_suffix_bf16: the weight-streaming projection out row m = x[m] . W^T (+ residual[m]) for 1 <= M <= 256 rows and any
 *   K % 8 == 0, plain input only (RMSNorm / SwiGLU are formed once per projection by mla_rmsnorm_fwd / mla_swiglu_fwd). Row m is row
 *   p = m % rows_per_batch of sample b = m / rows_per_batch and is written at out + b * out_batch_stride + (slot[b] + p) * ldo; with
 *   the RoPE epilogue (columns [0, rope_cols), no residual) it is rotated with table row slot[b] + p of rope_cos / rope_sin
 *   ([cap_rows, 64] fp32). slot: int32 [B] on the device (the sample's prefix length), or NULL = all zero (mla_gemm_skinny_bf16's
 *   addressing, cap_rows ignored). Rows with slot[b] + p outside [0, cap_rows) are not written. Deterministic (fixed-order sums, no
 *   atomics, no workspace). M <= 64: mla_gemm_skinny_bf16's K split and summation order -- bit-identical to it when every slot[b] is
 *   the same (out and the tables offset by that slot). M > 64: 32 W rows per workgroup and up to 16 x blocks per wave, so that x is
 *   re-read from L2 once per 32 weight rows. Every W fragment is loaded by exactly one wave of one workgroup. */
int mla_gemm_suffix_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                         int rows_per_batch, const int* slot, int cap_rows, const void* residual, long long ld_res, int M, int N, int K,
                         const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
/* mla_gemm_suffix_w8: mla_gemm_suffix_bf16 -- the same rows, slot / cap_rows addressing (the overlapping "groups" form included), residual
 *   and q|k rotary epilogue, launch forms and unwritten rows outside [0, cap_rows) -- over weight-only FP8: W [N, K] e4m3fn bytes (ldw in
 *   elements = bytes, ldw % 16 == 0: a row starts on 16 B) and w_scale [N] fp32 as mla_quant_fp8_rows writes them. K >= 16, K % 16 == 0.
 *   Arithmetic: mla_gemm_skinny_w8's -- 64-wide K steps split over the 8 waves as there, a lane's 16 codes decoded at scale 1 into the A
 *   fragments of two MFMAs, the 8 partial sums added in the same order, the finished sum times w_scale[n] (the rotation partner's times
 *   w_scale[n ^ 64]), then the residual add or the rotation and one bf16 rounding. Every output element depends on its own x row, its own
 *   W row and that K split only: for any M <= 256 rows [64 i, 64 i + 64) are bit for bit what mla_gemm_skinny_w8 (pre 0) writes for
 *   that slice. Half the weight bytes of the bf16 form per call; no scratch, no workspace, no atomics, graph-capturable. */
int mla_gemm_suffix_w8(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                       long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual, long long ld_res,
                       int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols, mla_stream_t stream);
/* ---- N action chunks for ONE observation (mla_amd/infer.py SampleGroupsEps): G groups of R suffix rows behind one shared prefix.
 * mla_attn_chunk_groups: q / k / v point at the packed post-RoPE q|k|v cache of one sample, [S_p + G * R, 3 H] with row stride ld:
 *   rows [0, S_p) are the prefix, row S_p + g * R + p is suffix row p of group g. Query (g, p) sees the logical keys j = 0 .. S_p + p,
 *   where logical key j is memory row j (j < S_p) or j + g * R (j >= S_p): the prefix and, causally, the group's own rows. Output row
 *   g * R + p of o (row stride ld_o), bf16. 1 <= R <= 64, G >= 1, S_p >= 0, head_dim 128, 16-B aligned rows. mla_attn_chunk's arithmetic
 *   over the logical key sequence (64-key tiles from key 0 shared out over 4 waves, fixed-order merge): group g's rows are bit for bit
 *   mla_attn_chunk with B = 1 and S_kv = S_p + R on cat(rows [0, S_p), rows [S_p + g R, S_p + (g + 1) R)). Masked and padding loads stay
 *   inside the group's own key set: no output depends on another group's rows. No allocation, no atomics, no workspace;
 *   graph-capturable.
 * mla_attn_chunk_groups_gw: the same with the launch form given -- gw: groups one workgroup serves (1, 2, 4; 0 = the library's choice,
 *   which is what mla_attn_chunk_groups launches): prefix-only key tiles are loaded, and their V tile transposed, once per workgroup;
 *   order: 0 = head-major work items in dispatch order, 1 = one contiguous chunk of the head-major order per XCD (block b takes item
 *   (b % 8) * (grid / 8) + b / 8; only when grid % 8 == 0), -1 = the library's choice. Same bits for every form; kept for measurement
 *   (tools/bench_infer.py --samples). */
int mla_attn_chunk_groups(const void* q, const void* k, const void* v, void* o, int G, int H, int head_dim, int S_p, int R, long long ld,
                          long long ld_o, float scale, mla_stream_t stream);
int mla_attn_chunk_groups_gw(const void* q, const void* k, const void* v, void* o, int G, int H, int head_dim, int S_p, int R, long long ld,
                             long long ld_o, float scale, int gw, int order, mla_stream_t stream);
/* ---- N action chunks for each of B observations (mla_amd/infer.py BatchedSampleGroupsEps): the two forms above composed. The cache is
 * [B, S_cap, 3 H] (row stride ld, sample stride batch_stride); in sample b rows [0, S_p[b]) are its prefix and row S_p[b] + g * R + p is
 * suffix row p of group g; rows behind S_p[b] + G * R are never read. All per-sample lengths are DEVICE arrays.
 * mla_attn_chunk_ragged_groups: mla_attn_chunk_groups per sample with S_p[b] = clamp(prefix_len[b], 0, S_cap - G * R), prefix_len int32 [B]
 *   on the device (S_cap >= G * R: the clamp keeps every read inside the sample's S_cap rows). Query (b, g, p) sees the logical keys
 *   0 .. S_p[b] + p of its sample, logical key j being memory row j (j < S_p[b]) or j + g * R; output row (b * G + g) * R + p of o.
 *   1 <= R <= 64, G >= 1, B >= 1, head_dim 128. One workgroup serves one sample and derives the clamped S_p[b] once, wave-uniformly; the
 *   grid (B * H * ceil(G / gw) * ceil(R / 16)) and the LDS do not depend on the lengths: graph-capturable for any mix of them. The rows
 *   of (b, g) are bit for bit mla_attn_chunk with B = 1 and S_kv = S_p[b] + R on cat(prefix rows of b, rows of group g) -- equivalently
 *   mla_attn_chunk_groups on sample b's slice with S_p = S_p[b]. No output depends on another group's rows, another sample's rows or the
 *   tail rows [S_p[b] + G * R, S_cap) of its own sample. No allocation, no atomics, no workspace.
 * mla_attn_chunk_ragged_groups_gw: the same with mla_attn_chunk_groups_gw's launch form arguments (same bits for every form).
 * mla_gemm_suffix_bf16_pos / mla_gemm_suffix_w8_pos: mla_gemm_suffix_bf16 / _w8 with the rotary position separated from the cache row:
 *   row m = (s, p) (s = m / rows_per_batch) is written at row slot[s] + p as there (rows outside [0, cap_rows) are not written) and, with
 *   the RoPE epilogue, rotated with table row rope_pos[s] + p of rope_cos / rope_sin ([rope_rows, 64] fp32); rope_pos: int32
 *   [ceil(M / rows_per_batch)] on the device. A row whose position falls outside [0, rope_rows) is not written (no column of it).
 *   rope_pos == NULL is mla_gemm_suffix_bf16 / _w8 itself (same kernel, same bits; rope_rows ignored). The engine's addressing: out the
 *   flat [B * S_cap, 3 H] cache with out_batch_stride 0, s = b * G + g, slot[s] = b * S_cap + S_p[b] + g * R, cap_rows = B * S_cap,
 *   rope_pos[s] = S_p[b], rope_rows = S_cap. */
int mla_attn_chunk_ragged_groups(const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim,
                                 const int* prefix_len, int S_cap, int R, long long ld, long long batch_stride, long long ld_o, float scale,
                                 mla_stream_t stream);
int mla_attn_chunk_ragged_groups_gw(const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim,
                                    const int* prefix_len, int S_cap, int R, long long ld, long long batch_stride, long long ld_o, float scale,
                                    int gw, int order, mla_stream_t stream);
int mla_gemm_suffix_bf16_pos(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                             int rows_per_batch, const int* slot, int cap_rows, const void* residual, long long ld_res, int M, int N, int K,
                             const float* rope_cos, const float* rope_sin, int rope_cols, const int* rope_pos, int rope_rows,
                             mla_stream_t stream);
int mla_gemm_suffix_w8_pos(const void* x, long long ldx, const void* W, long long ldw, const float* w_scale, void* out, long long ldo,
                           long long out_batch_stride, int rows_per_batch, const int* slot, int cap_rows, const void* residual,
                           long long ld_res, int M, int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols,
                           const int* rope_pos, int rope_rows, mla_stream_t stream);
/* ---- compact prefill for ONE observation (mla_amd/infer.py, prefill="compact"; mla_amd/csrc/prefill.hip): row-sized MFMA GEMMs for the
 * ~545 prefix rows, for which the training GEMM's 256-row tiles leave most of the chip idle. out[M, N] = x[M, K] . W^T with W [N, K]
 * row-major (ldw), 1 <= M <= 1024, N % 128 == 0 (the column tile), K >= 32 and K % 32 == 0, x / W / out / residual rows 16-B aligned
 * (pointers, ldx, ldw, ldo, out_batch_stride, ld_res multiples of 8 elements). fp32 accumulation, ONE rounding to bf16. Tile 64 rows x
 * 128 columns x 64 k per workgroup; split-K until tiles x split >= 2 x 256 CUs (at least 8 K tiles per slice, split <= 16): slice s of a
 * tile writes its fp32 partial to workspace [split][ceil(M / 64) * 64][N], a second launch adds the slices in the order s = 0, 1, ... and
 * runs the epilogue. No atomics, no counters, no library-owned memory, no state: the same inputs give the same bits on every run; both
 * launches go on `stream` and are graph-capturable.
 *   mla_gemm_prefill_ws_bytes: the workspace bytes the launches need for a shape (0 when the plan does not split), -1 for a shape outside
 *     the contract. A launch with a smaller (or NULL, or misaligned) workspace returns -1 and launches nothing; split = 1 ignores it.
 *   mla_gemm_prefill_plan: out4 = {row tile, column tile, split, workgroups of the main launch} as the launcher chooses them for `cus`
 *     CUs (the launcher itself plans for 256); the pure-Python mirror is mla_amd/hip.py:plan_gemm_prefill.
 *   mla_gemm_prefill_bf16: out = x W^T (+ residual[m], addressed like x with ld_res). Row m is row m % rows_per_batch of sample
 *     m / rows_per_batch and is written at out + (m / rows_per_batch) * out_batch_stride + (m % rows_per_batch) * ldo, as in
 *     mla_gemm_skinny_bf16.
 *   mla_gemm_prefill_qkv_rope: the same addressing (the rows land straight in a cache's slots); columns [0, rope_cols) are rotated per head
 *     of 128 in the epilogue, ON THE FP32 SUMS (a' = a cos - b sin, b' = b cos + a sin with b = channel + 64; mla_gemm_qkv_rope rotates the
 *     bf16-rounded projection: the results differ by that rounding), with table row m % rows_per_batch of rope_cos / rope_sin
 *     ([rows_per_batch, 64] fp32). rope_cols % 128 == 0, rope_cols <= N, head_dim must be 128.
 *   mla_gemm_prefill_gateup_swiglu: wgu = the packed [2 I, K] gate|up matrix, I % 64 == 0; act[m, i] = silu(gate) * up with
 *     swiglu_fwd_elem's arithmetic on the fp32 sums, one rounding. Writes act [M, I] only: no gu, no transposed copy. */
int mla_gemm_prefill_plan(int M, int N, int K, int cus, int* out4);
long long mla_gemm_prefill_ws_bytes(int M, int N, int K);
int mla_gemm_prefill_bf16(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo, long long out_batch_stride,
                          int rows_per_batch, const void* residual, long long ld_res, int M, int N, int K, void* workspace,
                          size_t workspace_bytes, mla_stream_t stream);
int mla_gemm_prefill_qkv_rope(const void* x, long long ldx, const void* W, long long ldw, void* out, long long ldo,
                              long long out_batch_stride, int rows_per_batch, int M, int N, int K, const float* rope_cos,
                              const float* rope_sin, int rope_cols, int head_dim, void* workspace, size_t workspace_bytes,
                              mla_stream_t stream);
int mla_gemm_prefill_gateup_swiglu(const void* x, long long ldx, const void* wgu, long long ldw, void* act, long long ldo,
                                   long long out_batch_stride, int rows_per_batch, int M, int I, int K, void* workspace,
                                   size_t workspace_bytes, mla_stream_t stream);
/* ---- the same kernels over FP8 codes (opt-in prefill_precision="fp8"; OpF8 of mla_amd/csrc/prefill.hip): xq [M, K], Wq [N, K] are e4m3fn
 * codes with one fp32 scale per row (x_scale [M], w_scale [N]), exactly what mla_quant_fp8_rows writes. out[m, n] =
 * bf16((sum_k xq[m, k] Wq[n, k]) * x_scale[m] * w_scale[n] ...): the sums run over the unscaled codes in fp32 on
 * v_mfma_f32_16x16x128_f8f6f4, the two scales are applied to the finished sum, in that order, BEFORE the rotation (the partner channel
 * with its own w_scale), before silu(gate) * up (gate and up with the scales of their own rows of the packed matrix) and before the
 * residual; one rounding. 1 <= M <= 1024, N % 128 == 0, K >= 128 and K % 128 == 0 (one K tile is 128 codes); xq / Wq rows 16-B aligned
 * (ldx, ldw multiples of 16 codes), out / residual as in the bf16 family; output addressing, RoPE tables, split-K rule (on K tiles of
 * 128), workspace layout, determinism and the -1 refusals that launch nothing are the bf16 family's. mla_gemm_prefill_f8_plan /
 * _ws_bytes answer for this family; the pure-Python mirror is mla_amd/hip.py:plan_gemm_prefill_f8. */
int mla_gemm_prefill_f8_plan(int M, int N, int K, int cus, int* out4);
long long mla_gemm_prefill_f8_ws_bytes(int M, int N, int K);
int mla_gemm_prefill_f8(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw, const float* w_scale, void* out,
                        long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual, long long ld_res, int M, int N,
                        int K, void* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_gemm_prefill_f8_qkv_rope(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw, const float* w_scale,
                                 void* out, long long ldo, long long out_batch_stride, int rows_per_batch, int M, int N, int K,
                                 const float* rope_cos, const float* rope_sin, int rope_cols, int head_dim, void* workspace,
                                 size_t workspace_bytes, mla_stream_t stream);
int mla_gemm_prefill_f8_gateup_swiglu(const void* xq, long long ldx, const float* x_scale, const void* wgu_q, long long ldw,
                                      const float* w_scale, void* act, long long ldo, long long out_batch_stride, int rows_per_batch, int M,
                                      int I, int K, void* workspace, size_t workspace_bytes, mla_stream_t stream);
/* ---- the wide-row FP8 family (opt-in batch_prefill="fp8": the B x S_p prefix rows of a batched sampling call; the same templates of
 * mla_amd/csrc/prefill.hip): the contract of mla_gemm_prefill_f8* in every respect -- codes and per-row scales as mla_quant_fp8_rows
 * writes them, fp32 sums over the unscaled codes, (sum * x_scale[m]) * w_scale[n] before the rotation / SwiGLU / residual, one rounding,
 * rows_per_batch / out_batch_stride addressing with RoPE table row m % rows_per_batch, deterministic split-K through the caller's
 * workspace, no atomics, no state, graph-capturable, -1 refusals that launch nothing -- with 1 <= M <= 65536. The plan chooses the row
 * tile: 64 (the compact kernels and their split rule; always for M <= 1024, where every entry point writes bit for bit what its
 * mla_gemm_prefill_f8* twin writes) or, for M > 1024 once ceil(M / 128) * (N / 128) >= 3 x CUs, 128: a 2 x 2 grid of waves with 64 W
 * rows x 64 x rows each (16 accumulators, 32 MACs per LDS byte read against 21), two LDS stages of 32 KiB. Workspace layout
 * [split][ceil(M / row tile) * row tile][N] fp32. mla_gemm_prefill_f8_wide_plan: out4 = {row tile, column tile, split, workgroups};
 * the pure-Python mirror is mla_amd/hip.py:plan_gemm_prefill_f8_wide. mla_gemm_prefill_f8* keep refusing M > 1024. */
int mla_gemm_prefill_f8_wide_plan(int M, int N, int K, int cus, int* out4);
long long mla_gemm_prefill_f8_wide_ws_bytes(int M, int N, int K);
int mla_gemm_prefill_f8_wide(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw, const float* w_scale,
                             void* out, long long ldo, long long out_batch_stride, int rows_per_batch, const void* residual,
                             long long ld_res, int M, int N, int K, void* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_gemm_prefill_f8_wide_qkv_rope(const void* xq, long long ldx, const float* x_scale, const void* Wq, long long ldw,
                                      const float* w_scale, void* out, long long ldo, long long out_batch_stride, int rows_per_batch, int M,
                                      int N, int K, const float* rope_cos, const float* rope_sin, int rope_cols, int head_dim,
                                      void* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_gemm_prefill_f8_wide_gateup_swiglu(const void* xq, long long ldx, const float* x_scale, const void* wgu_q, long long ldw,
                                           const float* w_scale, void* act, long long ldo, long long out_batch_stride, int rows_per_batch,
                                           int M, int I, int K, void* workspace, size_t workspace_bytes, mla_stream_t stream);

/* ---- device-resident DDIM loop (mla_amd/infer.py _CachedEpsBase.sample_ddim, opt-in sampler="device"; mla_amd/csrc/sampler.hip): the
 * sampler's glue between two suffix passes with the step index in device memory, so that a captured sampler step can be replayed
 * num_ddim_steps times without a host round trip. Stateless, no allocation, no host access, on `stream`, graph-capturable.
 *   mla_ddim_step: s = *step; for 0 <= s < steps the eta = 0 DDIM update of GaussianDiffusion.ddim_sample (gaussian_diffusion.py:520-568,
 *     clip_denoised = False) with coef[s] = {a, b, c, d} ([steps, 4] fp32: sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
 *     sqrt(alphas_cumprod_prev), sqrt(1 - alphas_cumprod_prev), GaussianDiffusion.ddim_tables): ax = a x; px = ax - b eps;
 *     e2 = (ax - px) / b; x = px c + d e2, every operation rounded on its own (no FMA contraction): the host loop's bits. x [n] fp32 is
 *     updated in place, eps [n] bf16, x_bf16 [n] = bf16_rne(x) is written; with `advance` the counter then becomes s - 1 (thread 0, behind
 *     a workgroup barrier). Any other s: nothing is written, the counter stays. One workgroup; 1 <= n <= 65 536.
 *   mla_ddpm_step (sample_ddpm, opt-in ddpm_sampler="device"): mla_ddim_step's form and counter protocol for GaussianDiffusion.p_sample
 *     (gaussian_diffusion.py:395-440, clip_denoised = False, fixed-small posterior variance) with coef[s] = {a, b, c1, c2, sig} ([steps, 5]
 *     fp32: sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2,
 *     (s != 0) exp(0.5 posterior_log_variance_clipped), GaussianDiffusion.ddpm_tables) and the step's normal variates in row s of
 *     noise [steps, n] fp32, filled by the host before the first step: ax = a x; px = ax - b eps; mean = c1 px + c2 x;
 *     x = mean + sig noise[s n + i], every operation rounded on its own; at s = 0 the product 0 * noise is still formed and added (the
 *     sign of a zero result is the host loop's). A counter outside [0, steps) reads neither table.
 *   mla_ddim_step_pin / mla_ddpm_step_pin (sample_ddim / sample_ddpm with pin=, MLA.predict_action_diff*(known_actions=...)): the same two
 *     steps -- one kernel body each, the pinned form a template instance -- with the reference's denoised_fn hook
 *     (GaussianDiffusion.p_mean_variance, gaussian_diffusion.py:318-321, clip_denoised = False) as replacement inpainting: with known [n]
 *     fp32 and pin [n] uint8 (non-zero = pinned), px = pin[i] ? known[i] : px right behind px = ax - b eps; everything behind it reads the
 *     replaced px (DDIM: e2 = (ax - px) / b; x = px c + d e2. DDPM: mean = c1 px + c2 x; x = mean + sig noise), every operation rounded on
 *     its own: the bits of the host loops with denoised_fn = where(pin, known, px). The same counter protocol, one workgroup,
 *     1 <= n <= 65 536; a counter outside [0, steps) writes nothing and reads neither a table nor known / pin. pin all zero: the bits of
 *     mla_ddim_step / mla_ddpm_step. At the last step (s = 0: c = 1 and d = 0; c1 = 1, c2 = 0 and sig = 0) a pinned x == known
 *     for finite x, eps and noise.
 *   mla_sampler_rows: with R = 1 + T, for 0 <= *step < steps: h_in row g R = t_table[*step] ([steps, H] bf16), row g R + 1 + p =
 *     x_e[g T + p] (g < G, p < T); any other *step writes nothing. h_in [G R, H], x_e [G T, H] bf16, H % 8 == 0, 16-B aligned rows. */
int mla_ddim_step(float* x, const void* eps, void* x_bf16, const float* coef, int* step, int n, int steps, int advance,
                  mla_stream_t stream);
int mla_ddpm_step(float* x, const void* eps, void* x_bf16, const float* coef, const float* noise, int* step, int n, int steps,
                  int advance, mla_stream_t stream);
int mla_ddim_step_pin(float* x, const void* eps, void* x_bf16, const float* coef, const float* known, const unsigned char* pin, int* step,
                      int n, int steps, int advance, mla_stream_t stream);
int mla_ddpm_step_pin(float* x, const void* eps, void* x_bf16, const float* coef, const float* noise, const float* known,
                      const unsigned char* pin, int* step, int n, int steps, int advance, mla_stream_t stream);
int mla_sampler_rows(void* h_in, const void* t_table, const void* x_e, const int* step, int G, int T, int H, int steps,
                     mla_stream_t stream);

/* ---- split-key suffix attention (mla_amd/infer.py: PrefixCachedEps, opt-in suffix_attention="split"; the multi-row engines, opt-in
 * groups_attention="split": mla_attn_groups_split below; mla_amd/csrc/attn_split.hip):
 * mla_attn_chunk's contract -- packed post-RoPE q|k|v cache, the last R rows of S_kv are the queries, query r sees keys
 * [0, S_kv - R + r], 1 <= R <= 64, any S_kv >= R, head_dim 128, B >= 1, P rounded to bf16 before P V -- with every head's key range read
 * by several workgroups instead of one per 16 queries.
 *   mla_attn_chunk_split: the nT = ceil(S_kv / 64) key tiles are cut into `splits` contiguous ranges (sizes differ by at most one tile, the
 *     first nT % splits ranges take one more). Launch 1: workgroup (b, h, 16 queries, s) runs mla_attn_chunk's arithmetic over range s --
 *     wave w takes the range's tiles t0 + w, t0 + w + 4, ..., the four wave states are merged in the order 0..3 -- and writes the
 *     un-normalised state (m, l, 128 fp32 sums) of its valid query rows to `ws`; a range wholly behind a query's causal limit writes the
 *     empty state (m = -inf, l = 0). Launch 2: one wave per (b, h, query): M = max_s m_s, numerator and denominator summed over
 *     s = 0, 1, ... with the weight exp2(m_s - M) (an empty state adds exactly zero, no inf - inf is formed), one division, one bf16
 *     rounding, the row of o ([B * R, H * 128], row stride ld_o, 4-B aligned). splits = 0: the plan's. splits == 1: mla_attn_chunk's own
 *     launch -- no workspace access, no second launch, o bit for bit mla_attn_chunk's. ws: caller-owned, 16-B aligned, at least
 *     mla_attn_chunk_split_ws_bytes(...) bytes (may be null when splits resolves to 1); no word of it is read that this call did not
 *     write, nothing behind the needed bytes is touched. No allocation, no state between calls, no counters, no atomics, no workgroup
 *     waits on another; deterministic, graph-capturable. Masked and padding loads never touch rows at or behind S_kv. All argument checks
 *     (R, S_kv, head_dim, splits in [0, nT], ws / ws_bytes) run on the host before any launch.
 *   mla_attn_chunk_split_plan: out4 = {splits, tiles per split (the larger ranges'), workgroups of launch 1 = B H ceil(R / 16) splits,
 *     workgroups of launch 2 (0 when splits == 1)} for `cus` compute units (the launcher plans for 256): splits grows by one while
 *     launch 1 still fits one workgroup per CU, splits < nT and the largest range has more than 4 tiles (a workgroup takes 4 tiles per
 *     pass; below one pass a cut saves nothing), so every range keeps at least 2 tiles; 1 when twice the unsplit grid no longer fits the
 *     chip. Pure host function.
 *   mla_attn_chunk_split_ws_bytes: B H R splits 130 fp32 words for splits > 1 (0 = the plan's), 0 for splits == 1, -1 outside the
 *     contract. Pure host function.
 *   mla_attn_groups_split: the split for the multi-row engines (opt-in groups_attention="split"). Addressing and masking are exactly
 *     mla_attn_chunk_groups' (prefix_len == NULL: B must be 1, S_p_or_cap = S_p) or mla_attn_chunk_ragged_groups' (prefix_len int32 [B] on
 *     the device, S_p_or_cap = S_cap, S_p[b] = clamp(prefix_len[b], 0, S_cap - G R)): query (b, g, p) sees the logical keys
 *     0 .. S_p[b] + p, logical key j is memory row j (j < S_p[b]) or j + g R, output row (b G + g) R + p; G = 1 with prefix_len[b] =
 *     kv_len[b] - R is mla_attn_chunk_ragged. Per (b, g) the nT_b = ceil((S_p[b] + R) / 64) logical key tiles are cut as
 *     mla_attn_chunk_split cuts them (same ranges, wave order, state, combine launch with B G as its samples), so a (b, g) block with
 *     splits <= nT_b is bit for bit mla_attn_chunk_split (B = 1, the same splits) on cat(prefix rows of b, rows of group g). `splits` is
 *     fixed on the host and nT_b derived on the device: grid, LDS and workspace do not depend on the lengths; a sample with
 *     nT_b < splits gives its trailing ranges no tile and they write the empty state; range 0 always holds key 0. Plan and workspace are
 *     mla_attn_chunk_split_plan / _ws_bytes at (B G, H, R, S_max), S_max = S_p + R without prefix_len and S_cap - (G - 1) R with it;
 *     splits = 0 resolves to that plan, valid values are 0 .. ceil(S_max / 64). When splits resolves to 1 the call IS the head form
 *     (mla_attn_chunk_groups / mla_attn_chunk_ragged_groups in the library's default launch form): its bits, no workspace access, no
 *     second launch. One group per workgroup only. Everything else -- ws ownership and alignment, no allocation / state / counters /
 *     atomics / waiting, graph capture, all argument checks on the host before any launch, masked and padding loads clamped inside the
 *     query's own key set -- as for mla_attn_chunk_split. 1 <= R <= 64, head_dim 128, 16-B aligned rows. */
int mla_attn_chunk_split_plan(int B, int H, int R, int S_kv, int cus, int* out4);
long long mla_attn_chunk_split_ws_bytes(int B, int H, int R, int S_kv, int splits);
int mla_attn_chunk_split(const void* q, const void* k, const void* v, void* o, int B, int H, int head_dim, int S_kv, int R, long long ld,
                         long long batch_stride, long long ld_o, float scale, int splits, void* ws, size_t ws_bytes, mla_stream_t stream);
int mla_attn_groups_split(const void* q, const void* k, const void* v, void* o, int B, int G, int H, int head_dim, const int* prefix_len,
                          int S_p_or_cap, int R, long long ld, long long batch_stride, long long ld_o, float scale, int splits, void* ws,
                          size_t ws_bytes, mla_stream_t stream);

/* ---- losses: CrossEntropyLoss modeling_llama.py:1258-1269; InfoNCE models/mla/fuser/contrastive.py:208-215
 * mla_ce_fwd: lse[r] = logsumexp(logits[r, :ncols]), loss[r] = lse - logits[r, label] (0 for ignore_index or a label outside [0, ncols);
 * labels == null: label = r). A logit of -inf is a masked column and adds nothing, on bf16 and fp32 rows alike (as F.cross_entropy);
 * loss or lse may be null. */
int mla_ce_fwd(const void* logits, int logits_fp32, long long ld, const long long* labels, float* loss, float* lse, int rows,
               int ncols, long long ignore_index, mla_stream_t stream);
int mla_ce_bwd(const void* logits, int logits_fp32, long long ld, const long long* labels, const float* lse, const float* gscale,
               float inv_count, void* dlogits, long long ldd, int rows, int ncols, long long ignore_index, mla_stream_t stream);
int mla_infonce_bwd(const float* L, const float* rlse, const float* clse, const float* gscale, void* dL, int M, int Mp,
                    mla_stream_t stream);
int mla_l2norm_fwd(const void* x, void* y, float* norms, int rows, int ncols, float eps, mla_stream_t stream);
int mla_l2norm_bwd(const void* dy, const void* y, const float* norms, void* dx, int rows, int ncols, mla_stream_t stream);

/* ---- point-cloud tokenizer (forward): models/mla/pointcloud/backbone/Point_PN.py
 * furthest_point_sample :6-21 (start index = explicit input), knn_point :62-73, LGA :115-158 + PosE_Geo :231-249,
 * BatchNorm in train mode :179,209,215, Pooling :166-169; projection models/mla/fuser/contrastive.py:5-45 */
int mla_project_points(const float* xyz, const float* consts21, long long* idx, unsigned char* valid, int n, float W, float Hh,
                       float stride, int ph, int pw, mla_stream_t stream);
int mla_fps(const float* xyz, const long long* start, long long* out, int B, int N, int npoint, mla_stream_t stream);
int mla_knn(const float* xyz, const float* centers, int* out, int B, int N, int G, int k, mla_stream_t stream);
int mla_gather_rows_f32(const float* src, const long long* idx, float* out, int B, int N, int G, int W, mla_stream_t stream);
int mla_lga_prep(const float* xyz, const void* feats, const long long* fps_idx, const int* knn, void* rows, float* lc_xyz, int B,
                 int N, int G, int K, int C, float alpha, float beta, mla_stream_t stream);
int mla_colstats_blocks(long long rows);
int mla_colstats_bf16(const void* x, float* mean, float* var, long long rows, int C, int ld, float* workspace, size_t workspace_bytes,
                      mla_stream_t stream);
int mla_bn_apply(const void* x, const float* mean, const float* var, const void* w, const void* b, const void* res, void* y,
                 long long rows, int C, float eps, int relu, mla_stream_t stream);
int mla_maxpool_k(const void* x, void* out, long long groups, int K, int C, mla_stream_t stream);
/* backward of the two (trainable point tokenizer, stage "pretrain" with use_pointcloud): feature gradient of lga_prep -- a gather per
 * target point with every sum in a fixed order (deterministic, no atomics; every element of dfeats [B, N, C] fp32 is written) -- and
 * of the max over the K neighbours (first maximum). Reference: models/mla/pointcloud/backbone/Point_PN.py:115-158 (autograd of LGA). */
int mla_lga_prep_bwd(const void* drows, const long long* fps_idx, const int* knn, float* dfeats, int B, int N, int G, int K, int C,
                     mla_stream_t stream);
int mla_maxpool_k_bwd(const void* x, const void* dy, void* dx, long long groups, int K, int C, mla_stream_t stream);

/* ---- vision tokenizer (forward): models/mla/image/vision_tokenizer.py  Conv2d patchify :110,122 (im2col + GEMM),
 * LocalAttention :26-47 (avg-pool, 3x3 window attention) */
int mla_im2col_patch(const void* pix, int pix_fp32, void* rows, int B, int CT, int Himg, int Wimg, int P, int Kpad,
                     mla_stream_t stream);
int mla_avgpool_tokens(const void* x, void* y, int B, int gh, int gw, int C, int cs, mla_stream_t stream);
int mla_local_attn(const void* q, const void* kv, void* out, int B, int gh, int gw, int C, int cs, int heads, float scale,
                   mla_stream_t stream);
/* backward of the two (stage "pretrain": models/vlm/prismatic.py:415-447 trains vision_tower_2d): window-attention gradients
 * (dq [windows, C], dkv [tokens, 2C]; every k/v row belongs to one window) and avg-pool backward fused with a second addend */
int mla_local_attn_bwd(const void* q, const void* kv, const void* dout, void* dq, void* dkv, int B, int gh, int gw, int C, int cs,
                       int heads, float scale, mla_stream_t stream);
/* CLIP-style preprocessing of uint8 HWC frames on the GPU (the reference runs CLIPImageProcessor on the CPU per frame,
 * vla/datasets/datasets.py:52-69): PIL-exact 8-bit separable bicubic resize (host-built 2^22 fixed-point taps), 1/255 rescale,
 * mean/std normalisation, optional all-ones mask channel; mean3 / std3 are HOST pointers */
int mla_clip_preprocess(const unsigned char* img, int B, int Hin, int Win, const int* bounds_h, const int* coef_h, int ks_h,
                        const int* bounds_v, const int* coef_v, int ks_v, void* out, int out_fp32, int OH, int OW, const float* mean3,
                        const float* std3, int mask_channel, mla_stream_t stream);
int mla_avgpool_tokens_bwd(const void* dy, const void* other, void* dx, int B, int gh, int gw, int C, int cs, mla_stream_t stream);

/* ---- batched GEMM (two-level batch: outer = sample, inner = head) for the generation heads' nn.MultiheadAttention products
 * (models/mla/generation/models.py:44,103-122: QK^T, PV and their gradients). Same operand modes as mla_gemm_bf16; batch
 * (o, i) adds o*s?o + i*s?i ELEMENTS to each base pointer; n_inner >= 1. No bias / residual. */
int mla_gemm_batched_bf16(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int a_mode, int b_mode,
                          int out_fp32, float alpha, int n_outer, int n_inner, long long sAo, long long sAi, long long sBo,
                          long long sBi, long long sCo, long long sCi, mla_stream_t stream);

/* ---- post-training generation heads (BASELINE config[3]): models/mla/generation/models.py
 * nn.TransformerDecoderLayer :103-122 / TransformerBlock :39-65 pieces: softmax(+attention dropout) over the first nvalid of
 * ncols key columns, Dropout (+ residual add), DropPath (per-sample scale), LayerNorm with backward; PointCloudGenerationModule
 * :351-386: sequence mean :359, BatchNorm1d(train) backward :335; chamfer_distance_l2 gen_loss.py:12-18; image loss
 * models/vlm/prismatic.py:780-816 with ImageGenerationModule._generate_generated_patches models.py:226-286 evaluated for the
 * all-true ROI mask (use_roi = False, scripts/post_rlbench.sh:26) and images_to_patches utils.py:7-18 addressing.
 * Dropout decisions are a counter-based hash of (seed, element index): backward regenerates the forward mask. */
int mla_softmax_rows_fwd(const float* scores, void* P, void* Pd, long long rows, int ncols, int nvalid, float p,
                         unsigned long long seed, mla_stream_t stream);
/* dS = P' o (g - sum(g o P')), g = dPd o mask / (1 - p), P' = P / sum(P) (the bf16 probabilities renormalised in fp32).
 * dPd: fp32 (dpd_fp32 = 1, the product path: dP is never rounded, like torch's fused attention) or bf16. */
int mla_softmax_rows_bwd(const void* dPd, int dpd_fp32, const void* P, void* dS, long long rows, int ncols, int nvalid, float p,
                         unsigned long long seed, mla_stream_t stream);
int mla_dropout_fwd(const void* x, const void* residual, void* y, long long n, float p, unsigned long long seed, mla_stream_t stream);
int mla_dropout_bwd(const void* dy, void* dx, long long n, float p, unsigned long long seed, mla_stream_t stream);
int mla_scale_batch(const void* x, const float* scale, void* y, long long batch, long long per, mla_stream_t stream);
int mla_layernorm_stats_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, long long rows, int H,
                            float eps, mla_stream_t stream);
int mla_layernorm_bwd_blocks(long long rows);
int mla_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, void* dx, float* dw,
                      float* db, int accumulate, long long rows, int H, float* workspace, size_t workspace_bytes,
                      mla_stream_t stream);
int mla_seqmean_fwd(const void* x, void* y, int B, int S, int C, mla_stream_t stream);
int mla_seqmean_bwd(const void* dy, void* dx, int B, int S, int C, mla_stream_t stream);
int mla_bn_bwd_blocks(long long rows);
int mla_bn_bwd(const void* dy, const void* x, const float* mean, const float* var, const void* w, void* dx, float* dw, float* db,
               int accumulate, long long rows, int C, float eps, float* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_chamfer_fwd(const float* pred, const float* gt, float* d1, int* i1, float* d2, int* i2, float* loss, int B, int N, int M,
                    float* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_chamfer_bwd(const float* pred, const float* gt, const float* d1, const int* i1, const float* d2, const int* i2,
                    const float* gscale, float* dpred, int B, int N, int M, mla_stream_t stream);
int mla_imgloss_fwd(const void* delta_raw, int ld, const void* curr, const void* next, int img_fp32, float* sums, int B, int CT_curr,
                    int CT_next, int HW, int ps, float clip, float* workspace, size_t workspace_bytes, mla_stream_t stream);
/* partial ROI (use_roi = True): per patch either the ROI rule or warp (bilinear translation, border clamp) + alpha blend
 * (models.py:243-283), with the ROI / background / delta-reward sums of prismatic.py:786-816; backward also yields the alpha / offset
 * head gradients (one block per patch) */
int mla_imgroi_fwd(const void* delta_raw, int ld, const void* a_raw, int lda, const void* o_raw, int ldo, const unsigned char* roi,
                   const void* curr, const void* next, int img_fp32, float* sums, int B, int CT_curr, int CT_next, int HW, int ps,
                   float clip, float shift, float* workspace, size_t workspace_bytes, mla_stream_t stream);
int mla_imgroi_bwd(const void* delta_raw, int ld, const void* a_raw, int lda, const void* o_raw, int ldo, const unsigned char* roi,
                   const void* curr, const void* next, int img_fp32, const float* coef, void* ddelta_raw, float* dalpha_raw,
                   float* doff_raw, int B, int CT_curr, int CT_next, int HW, int ps, float clip, float shift, mla_stream_t stream);
int mla_imgloss_bwd(const void* delta_raw, int ld, const void* curr, const void* next, int img_fp32, const float* gscale,
                    void* ddelta_raw, int B, int CT_curr, int CT_next, int HW, int ps, float clip, mla_stream_t stream);

/* ---- multi-GPU rehearsal (no reference counterpart): stand-in for a collective's kernel on a side stream -- `blocks` resident
 * 1024-thread workgroups stream out = a + b over n fp32 (n % 4 == 0), sleeping `sleep_ticks` x 8128 clocks after every 64 KiB chunk; lds_bytes =
 * 163840 makes each workgroup the only resident of its CU (the CU is taken from a gemm256 workgroup), 0 lets it share the CU.
 * tools/contention_rehearsal.py measures the training step's sensitivity to it (profiles/r4_contention.txt). */
int mla_side_traffic(const float* a, const float* b, float* out, long long n, int blocks, int lds_bytes, int sleep_ticks, mla_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MLA_HIP_H */
