"""Prefix-cached epsilon model for the diffusion samplers (round 6).

Reference: `MLA.predict_action_diff` (models/mla/model_mla.py:592-775) hands `self.vlm.forward` to `ddim_sample_loop`
(models/diffusion/gaussian_diffusion.py:608-688), which calls it once per DDIM step -- 8 whole 548-token forwards through the encoders and
the 32 decoder layers, although with causal attention everything in front of the `[t, x]` tokens
(`[BOS | pc 256 | img 256 | tac 1 | text[1:k] | proprio]`, models/vlm/prismatic.py:981-1038) is identical in all 8 and the token behind
them (`text[k:]`) cannot influence the rows that are read out (`noise_pred = final_layer(h_last)[k'+2 : k'+2+T]`, :1115-1126).

`PrefixCachedEps(vlm, **model_kwargs)` runs the encoders and ONE prefill over the prefix rows with the training kernels
(`ops.DecoderLayerFn._fwd`: fused RMSNorm / QKV + RoPE GEMM / flash attention / SwiGLU GEMMs), keeps every layer's packed post-RoPE
q|k|v rows (`LayerActs.qkv`), and then serves each `model(x, t)` call with a pass over the `1 + T` suffix rows per sample: skinny weight-streaming GEMMs
(`mla_gemv_bf16` up to 8 rows, `mla_gemm_skinny_bf16` up to 64; every weight read once per pass), `mla_attn_decode` (up to 8 rows)
or `mla_attn_chunk` (up to 64) against the cached keys / values, the same RMSNorm / RoPE / SwiGLU
kernels' arithmetic as training (RMSNorm and SwiGLU are applied inside the projections' input staging). The 6 x 32 launches of a pass
(5 with the rotary embedding in the QKV kernel's epilogue) are captured once into a HIP graph and replayed per DDIM step.

Opt-in (`suffix_weights="fp8"`, see MODES): the sampler steps stream a per-row e4m3fn copy of the projections through
`mla_gemv_w8` / `mla_gemm_skinny_w8` (one chunk per call) or `mla_gemm_suffix_w8` (N chunks per observation, SampleGroupsEps) -- half the
weight bytes per step; prefill, activations, cache and attention are untouched.

Opt-in (`suffix_mx="fp4"`, see MODES): the same with an OCP MXFP4 copy (e2m1 codes, one e8m0 scale byte per 32 elements of a weight row)
through `mla_gemv_w4` / `mla_gemm_skinny_w4` / `mla_gemm_suffix_w4` -- a quarter of the weight bytes, decoded exactly in registers; a
4-bit weight error whose effect on a trained policy is not measured.

Opt-in (`sampler="device"`, see MODES): the DDIM loop around the suffix passes runs on the device -- `sample_ddim` replays one
captured sampler step (x_embedder, `mla_sampler_rows`, the suffix pass, final_layer, `mla_ddim_step`) per DDIM step with the step index in
device memory: no copy to the device and no host wait between the steps, bit for bit the host loop's result.

Opt-in (`ddpm_sampler="device"`, see MODES): the same for the DDPM loop of `use_ddim=False` -- `sample_ddpm` draws the steps'
normal variates up front into a device table (asynchronous launches, the host loop's order) and replays the captured step with
`mla_ddpm_step` as its update num_timesteps times: the host loop's bits and generator position.

Pinned chunk steps (`MLA.predict_action_diff*(known_actions=...)`): `sample_ddim` / `sample_ddpm` take `pin=(known, mask)` and run the same
loops with `mla_ddim_step_pin` / `mla_ddpm_step_pin` as the update -- the x0 prediction of every step is `known` where `mask` is set, the
reference's `denoised_fn` hook -- on a state and a captured step of their own; the un-pinned loops keep theirs.

DPM-Solver++(2M) (`MLA.predict_action_diff*(solver="dpmpp2m")`; no row of MODES: the solver belongs to the diffusion process, not to an
engine): with `sampler="device"`, `sample_dpmpp2m` runs the second-order multistep solver over the respaced process on the same loop --
`mla_dpmpp2m_step[_pin]` as the update, the previous step's x0 prediction in the state's `hist`, zeroed at every reset -- on states and
captured steps of its own: the bits of GaussianDiffusion.dpmpp2m_sample_loop, and the DDIM and DDPM loops keep theirs.

Opt-in (`suffix_attention="split"`, see MODES; PrefixCachedEps only): the attention launch of the suffix pass becomes
`mla_attn_chunk_split` -- every head's key tiles cut over several workgroups, the partial softmax states merged in a fixed order by a
second launch -- for every R; the same function up to summation order. The multi-row engines (BatchedPrefixCachedEps, SampleGroupsEps,
BatchedSampleGroupsEps) take the same argument from the public `groups_attention="split"` (MODES) and launch
`mla_attn_groups_split`: that split per (sample, group), the prefix lengths still read on the device.

Opt-in (`suffix_operand="once"`, see MODES; PrefixCachedEps only): a pass over more than 8 suffix rows forms each RMSNorm
operand once with the stand-alone kernel, runs every projection on the plain `mla_gemm_skinny_*` form and takes SwiGLU into the gate|up
projection's epilogue (`mla_gemm_skinny_gateup_swiglu_*`) -- seven launches per layer instead of five, the same bits.

Opt-in (`prefill="compact"`, `prefill_precision="fp8"`, see MODES; PrefixCachedEps and SampleGroupsEps):
the prefix rows of one observation run on the row-sized GEMMs of csrc/prefill.hip, and with "fp8" their four projections per layer on
e4m3fn codes of weights AND activations (csrc/prefill.hip, the K = 128 FP8 MFMA) -- the same FP8 weight copy the suffix pass streams.

Opt-in (`batch_prefill="fp8"`, see MODES; BatchedPrefixCachedEps and BatchedSampleGroupsEps): the NB x S_pmax right-padded
prefix rows of a batched call run through the same compact layer in ONE pass per layer, their projections on the wide-row FP8 GEMMs
(mla_gemm_prefill_f8_wide*: up to 65 536 rows, 64- or 128-row tiles).

Semantics vs the reference: identical arithmetic up to summation order (fp32 accumulation everywhere), with ONE stated difference -- the
reference's point tokenizer draws fresh random FPS start indices inside every one of the 8 forwards (Point_PN.py:10); here they are
drawn once per action chunk (the prefix is computed once). With given start indices (`fps_starts_override`, as in
tests/test_inference_gpu.py) the two are the same function."""
from __future__ import annotations

import collections
import functools
import logging
import math
import os
import warnings
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import hip, ops

_USE_GRAPH = os.environ.get("MLA_INFER_GRAPH", "1") != "0"
_LOG = logging.getLogger(__name__)

SPLICE_TAG = 29871                                  # prismatic.py:882-887 (eval): the [t, x] tokens go in front of its last occurrence
PROMPT_TAIL = (29871, 32001, 32002, 29871)          # model_mla.py:640-645: appended unless the row already ends with the tag, then [:-3]


class Mode(NamedTuple):
    """One opt-in keyword of MLA.predict_action_diff*: a row of MODES."""
    name: str
    values: tuple                    # the default first
    needs: Optional[str] = None      # what a value other than the default requires of the call (check_mode): None, "reuse_prefix",
                                     # "compact" (prefill="compact"), "ddim" / "ddpm" (reuse_prefix and that sampler loop)
    tag: Optional[str] = None        # an engine's mode: tag + value joins the engine key (_engine); None: a mode of the call
    lacks: str = ""                  # check_mode's clause: what the whole-forward sampler (reuse_prefix=False) has instead


# Every row: name, values, needs, tag, lacks. The order is the order of the engine key's suffix.
MODES = (
    # What the suffix pass streams (MLA.predict_action_diff(suffix_weights=...)); the prefill does not depend on it (bf16 weights unless
    # prefill_precision says otherwise), so the prefix keys / values keep bf16-weight precision:
    #   "bf16"         the decoder weights as they are (default)
    #   "fp8"          a per-row e4m3fn copy (hip.quant_fp8_rows) through mla_gemv_w8 / mla_gemm_skinny_w8 (PrefixCachedEps) or
    #                  mla_gemm_suffix_w8 (SampleGroupsEps): half the bytes per sampler step
    #   "fp8_as_bf16"  the bf16 kernels on bf16(q * scale): the reference of the "fp8" path, and what the format costs on a checkpoint
    # Without the cached prefix, or on a shape no engine serves, the public methods refuse it themselves (route by route).
    Mode("suffix_weights", ("bf16", "fp8", "fp8_as_bf16"), None, ""),

    # How the prefix rows are prefilled (MLA.predict_action_diff(prefill=...)):
    #   "train"    the training forward kernels (ops.DecoderLayerFn._fwd: 256-row GEMM tiles built for 17 536 rows), default
    #   "compact"  the row-sized GEMMs of mla_amd/csrc/prefill.hip (64 x 128 tiles, deterministic split-K): q|k|v + RoPE written straight into
    #              the cache, gate|up + SwiGLU writing the product only; same function up to summation order and rounding points
    # The batched method refuses "compact" as not implemented, the other two without the cached prefix: each says so itself.
    Mode("prefill", ("train", "compact"), None, "prefill:"),

    # Which attention launch the sampler steps of PrefixCachedEps use (MLA.predict_action_diff(suffix_attention=...)):
    #   "head"   mla_attn_decode / mla_attn_chunk: one workgroup per (sample, head, 16 queries) reads the head's whole key range (default)
    #   "split"  mla_attn_chunk_split with the library's plan for every R: each head's key tiles cut over several workgroups, the partial
    #            softmax states merged in a fixed order by a second launch; same function up to summation order
    Mode("suffix_attention", ("head", "split"), "reuse_prefix", "attention:", "has no suffix pass"),

    # Which attention launch the sampler steps of the multi-row engines use (MLA.predict_action_diff_batch / predict_action_diff_samples
    # (groups_attention=...); BatchedPrefixCachedEps, SampleGroupsEps, BatchedSampleGroupsEps: it is THEIR suffix_attention attribute):
    #   "head"   mla_attn_chunk_ragged / mla_attn_chunk_groups / mla_attn_chunk_ragged_groups: one workgroup per (sample, group, head, 16
    #            queries) reads its whole key range (default)
    #   "split"  mla_attn_groups_split with the library's plan at the engine's capacity: the key tiles of every (sample, group, head) cut over
    #            several workgroups, the partial softmax states merged in a fixed order by a second launch; same function up to summation
    #            order. The plan splits for B * G <= 4 at R <= 16 and B * G <= 2 at 17 <= R <= 32 (32 heads, 256 CUs); beyond, it is the
    #            head launch by construction
    Mode("groups_attention", ("head", "split"), "reuse_prefix", "attention:", "has no suffix pass"),

    # What the compact prefill's four projections per layer compute on (MLA.predict_action_diff(prefill="compact", prefill_precision=...)):
    #   "bf16"         the bf16 weights and activations as they are (default)
    #   "fp8"          e4m3fn codes of BOTH operands on the K = 128 MFMA (mla_amd/csrc/prefill.hip): the model's FP8 weight copy (one scale
    #                  per output channel, shared with suffix_weights="fp8") and the projection inputs quantised per row (hip.quant_fp8_rows);
    #                  attention, cache, norms and residual stream stay bf16
    #   "fp8_as_bf16"  the bf16 compact kernels on bf16(code * scale) of the same weight codes, the projection inputs quantised and
    #                  dequantised by the same statement: the reference of the "fp8" path, and what the format costs on a checkpoint
    Mode("prefill_precision", ("bf16", "fp8", "fp8_as_bf16"), "compact", "precision:"),

    # How the batched engines prefill the NB x S_pmax right-padded prefix rows of a pass (MLA.predict_action_diff_batch(batch_prefill=...);
    # BatchedPrefixCachedEps, BatchedSampleGroupsEps):
    #   "train"        one varlen pass per layer on the training forward kernels, the bf16 weights (default)
    #   "fp8"          the compact prefill's layer (_compact_layer) over all NB x S_pmax rows at once, its four projections on e4m3fn codes of
    #                  BOTH operands: the wide-row GEMMs of mla_amd/csrc/prefill.hip (mla_gemm_prefill_f8_wide*, up to 65 536 rows, 64- or
    #                  128-row tiles) beyond 1024 rows, the compact ones up to there; the model's FP8 weight copy, shared with
    #                  suffix_weights="fp8"; attention, cache, norms and residual stream stay bf16
    #   "fp8_as_bf16"  per sample, the bf16 compact kernels on bf16(code * scale) of the same weight codes and on quantised-and-dequantised
    #                  inputs: the reference of the "fp8" path (slow: one pass over the layers per sample)
    Mode("batch_prefill", ("train", "fp8", "fp8_as_bf16"), "reuse_prefix", "batch_prefill:", "has no separate prefill"),

    # How a pass of PrefixCachedEps over MORE than 8 suffix rows forms the RMSNorm / SwiGLU operands of its projections
    # (MLA.predict_action_diff(suffix_operand=...)); up to 8 rows the GEMV stages its input once per workgroup and both values are one pass:
    #   "fused"  inside the projections' input staging (mla_gemm_skinny_* pre 1 / 2): five launches per layer, the operand re-formed by every
    #            workgroup (default)
    #   "once"   RMSNorm by the stand-alone kernel once per pass, every projection on the plain skinny form, SwiGLU in the gate|up
    #            projection's epilogue (mla_gemm_skinny_gateup_swiglu_*): seven launches per layer, the same bits
    Mode("suffix_operand", ("fused", "once"), "reuse_prefix", "operand:", "has no suffix pass"),

    # Who runs the DDIM loop around the suffix passes (MLA.predict_action_diff(sampler=...)):
    #   "host"    GaussianDiffusion.ddim_sample_loop: torch expressions per step, tables copied to the device per step (default)
    #   "device"  _CachedEpsBase.sample_ddim: one captured sampler step replayed num_ddim_steps times, the step index in device memory; no copy
    #             to the device and no host wait between the steps; the same bits
    Mode("sampler", ("host", "device"), "ddim", None, "has the host loop only"),

    # Who runs the DDPM loop (use_ddim=False: the training diffusion's p_sample_loop) around the suffix passes
    # (MLA.predict_action_diff(ddpm_sampler=...)); sampler= above keeps its meaning, the DDIM loop:
    #   "host"    GaussianDiffusion.p_sample_loop: torch expressions per step, a device wait in every step (default)
    #   "device"  _CachedEpsBase.sample_ddpm: the steps' normal variates drawn up front into a device table, then one captured sampler step
    #             replayed num_timesteps times; no copy to the device and no host wait between the steps; the same bits and generator position
    Mode("ddpm_sampler", ("host", "device"), "ddpm", None, "has the host loop only"),

    # A block-scaled 4-bit copy for the suffix pass (MLA.predict_action_diff(suffix_mx=...)). Like suffix_weights it chooses what the
    # suffix pass streams, so a value other than "off" together with suffix_weights other than "bf16" is an error (check_modes); it has
    # its own row because it has its own copy, kernels and cost. The prefill does not depend on it:
    #   "off"          whatever suffix_weights says (default)
    #   "fp4"          the model's OCP MXFP4 copy (hip.quant_mxfp4_rows: e2m1 codes, one e8m0 scale byte per 32 elements of a row) through
    #                  mla_gemv_w4 / mla_gemm_skinny_w4 (PrefixCachedEps) or mla_gemm_suffix_w4 (the row-GEMM engines): a quarter of the
    #                  bf16 bytes per sampler step. The weight error of the format is a 4-bit one (relative Frobenius error 0.11 on
    #                  Gaussian weights, against 0.012 for "fp8"); what it does to a trained policy is not measured
    #   "fp4_as_bf16"  the bf16 kernels on the dequantised copy (exactly the values the `_w4` kernels decode): the reference of the "fp4"
    #                  path, and what the format costs on a checkpoint, without the new kernels
    Mode("suffix_mx", ("off", "fp4", "fp4_as_bf16"), "reuse_prefix", "mx:", "has bf16 weights only"),
)
MODES = {mode.name: mode for mode in MODES}
# The order in which a public method validates them: the first wrong keyword is the one the error names.
CHECK_ORDER = ("suffix_operand", "suffix_weights", "suffix_mx", "prefill", "prefill_precision", "sampler", "ddpm_sampler", "suffix_attention",
               "groups_attention")


class Modes(collections.namedtuple("Modes", list(MODES), defaults=[mode.values[0] for mode in MODES.values()])):
    """The mode keywords of one call or one engine, every field at its default unless given: what the public methods, the factories,
    _engine and the constructors hand to each other."""
    __slots__ = ()

    def forwarded(self, *names) -> dict:
        """The keywords `names` as a call that ends in a single-observation method hands them on: without groups_attention among them,
        its "split" is that method's suffix_attention="split"; batch_prefill is that method's compact prefill at that precision."""
        keywords = {name: getattr(self, name) for name in names}
        if keywords.get("suffix_mx") == "off":                               # the default: the call is the one without the keyword
            del keywords["suffix_mx"]
        if "suffix_attention" in keywords and "groups_attention" not in keywords and self.groups_attention == "split":
            keywords["suffix_attention"] = "split"
        if self.batch_prefill != "train":
            keywords.update(prefill="compact", prefill_precision=self.batch_prefill)
        return keywords


def check_mode(name, value, reuse_prefix=True, use_ddim=True, num_ddim_steps=8, prefill="compact"):
    """The argument errors of one keyword: an unknown value; a value other than the default in a call that does not run what the value
    needs (Mode.needs) -- a keyword is never silently ignored, and there is never a silent bf16 prefill. A shape the engine does not
    serve is the caller's ValueError (needs_engine)."""
    mode = MODES[name]
    if value not in mode.values:
        raise ValueError(f"{name} must be one of {mode.values}, got {value!r}")
    if value == mode.values[0] or mode.needs is None:
        return
    if mode.needs == "compact":
        if prefill != "compact":
            raise ValueError(f"{name}=\"{value}\" runs on the compact prefill (prefill=\"compact\"); prefill={prefill!r} has the bf16 "
                             "kernels only")
        return
    if not reuse_prefix:
        raise ValueError(f"{name}=\"{value}\" runs on the cached prefix (reuse_prefix=True); the whole-forward sampler {mode.lacks}")
    ddim = use_ddim and num_ddim_steps is not None
    if mode.needs == "ddim" and not ddim:
        raise ValueError(f"{name}=\"{value}\" is the DDIM loop at eta = 0 (use_ddim=True and num_ddim_steps); the DDPM loop's device form "
                         f"is ddpm_sampler=\"{value}\"")
    if mode.needs == "ddpm" and ddim:
        raise ValueError(f"{name}=\"{value}\" is the DDPM loop (use_ddim=False or num_ddim_steps=None); this call runs the DDIM sampler, "
                         f"whose device loop is sampler=\"{value}\"")


def check_modes(modes: Modes, reuse_prefix=True, use_ddim=True, num_ddim_steps=8):
    """check_mode over a public method's keywords in CHECK_ORDER, before the model is touched (batch_prefill is the batched method's own
    check, behind these)."""
    for name in CHECK_ORDER:
        check_mode(name, getattr(modes, name), reuse_prefix, use_ddim, num_ddim_steps, modes.prefill)
        if name == "suffix_mx":
            check_one_suffix_copy(modes)


def check_one_suffix_copy(modes: Modes):
    """suffix_mx and suffix_weights both choose what the suffix pass streams: at most one of them away from its default."""
    if modes.suffix_mx != "off" and modes.suffix_weights != "bf16":
        raise ValueError(f"suffix_mx=\"{modes.suffix_mx}\" and suffix_weights=\"{modes.suffix_weights}\" both choose what the suffix pass "
                         "streams; use suffix_mx with suffix_weights=\"bf16\"")


def engine_modes(**keywords) -> Modes:
    """The bundle of an engine's factory, its keywords validated in the order given (an engine IS the cached prefix)."""
    modes = Modes(**keywords)
    for name, value in keywords.items():
        check_mode(name, value, prefill=modes.prefill)
    check_one_suffix_copy(modes)
    return modes


def needs_engine(engine: str, n_action_rows: int, **keywords):
    """A keyword with a value other than its default on a shape the cached-prefix engine does not serve: an error that names the first
    such keyword, never the warned loop of whole-forward calls."""
    for name, value in keywords.items():
        if value != MODES[name].values[0]:
            raise ValueError(f"{name}=\"{value}\": the cached-prefix engine ({engine}) does not serve {1 + n_action_rows} suffix rows per "
                             f"sample at this head_dim; use {name}=\"{MODES[name].values[0]}\"")


def suffix_attention_single_only(mode, route: str):
    """suffix_attention="split" on a route that does not end in predict_action_diff: the ragged and groups engines keep their own
    attention launches."""
    if mode == "split":
        raise NotImplementedError(f"suffix_attention=\"split\": {route} runs the ragged / groups engines, whose attention launches "
                                  "(mla_attn_chunk_ragged, mla_attn_chunk_groups and their batched forms) take their split-key form from "
                                  "groups_attention=\"split\"; suffix_attention serves predict_action_diff (one observation, one chunk) only")


_GRAPH_OFF = "MLA_INFER_GRAPH=0: the device sampler launches its steps one by one"      # graph_error of an eager sample_ddim / sample_ddpm


class _DdimState:
    """What sample_ddim / sample_ddpm / sample_dpmpp2m keep per (engine, batch, action_dim, diffusion): the chunk x fp32 and its bf16 cast,
    the step counter, the coefficient and timestep-embedding tables, and the captured step; a DDPM state also has `noise`
    [steps, B T D] fp32, the steps' normal variates, and a DPM-Solver++(2M) state `hist` [B, T, D] fp32, the previous step's x0
    prediction, zeroed at every reset (both None in a DDIM state: they select the update kernel). A pinned state (pin=) also has `known`
    [B, T, D] fp32 and `pin` [B, T, D] uint8, refilled per call (None in an un-pinned state: the update is the plain kernel). All
    device tensors are allocated outside inference mode."""
    __slots__ = ("diffusion", "steps", "x", "x_bf16", "step", "coef", "timesteps", "t_table", "t_key", "graph", "graph_key", "failed",
                 "noise", "known", "pin", "hist")


class _Coded:
    """What the coded projection weights share. A class is a tuple (q, scale) as its quantiser writes them and says: fmt, its row of
    hip.WEIGHT_FORMATS; name, the mode value that streams the codes (name + "_as_bf16": the bf16 kernels on their dequantisation);
    slot and label, where vlm.__dict__ keeps the model's copy and what the log calls it; of(W), the quantiser; dequantised(), the
    exact bf16 matrix. A new format is a row of hip.WEIGHT_FORMATS, a class here and its entry in CODED."""
    __slots__ = ()

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self)


class W8(_Coded, collections.namedtuple("W8", "q scale")):
    """A quantised projection weight: q [N, K] float8_e4m3fn codes, scale [N] fp32 (one per output channel)."""
    __slots__ = ()
    fmt, name, slot, label = hip.WEIGHT_FORMATS["w8"], "fp8", "_prefix_fp8", "suffix_weights: FP8"

    @classmethod
    def of(cls, W):
        return cls(*hip.quant_fp8_rows(W))

    def dequantised(self) -> torch.Tensor:
        return (self.q.float() * self.scale[:, None]).to(torch.bfloat16)


class W4(_Coded, collections.namedtuple("W4", "q scale")):
    """An MXFP4 projection weight: q [N, K / 2] uint8 (two e2m1 codes per byte), scale [N, K / 32] uint8 (one e8m0 byte per block of 32)."""
    __slots__ = ()
    fmt, name, slot, label = hip.WEIGHT_FORMATS["w4"], "fp4", "_prefix_mxfp4", "suffix_mx: MXFP4"

    @classmethod
    def of(cls, W):
        return cls(*hip.quant_mxfp4_rows(W))

    def dequantised(self) -> torch.Tensor:
        """bf16 [N, K], exact: sign * {0, 0.5, 1, 1.5, 2, 3, 4, 6}[index] * 2^(scale - 127) is a bf16 value."""
        grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], device=self.q.device)
        N, K = self.q.shape[0], self.q.shape[1] * 2
        q = self.q.to(torch.int64)
        val = grid[torch.stack([q & 15, q >> 4], dim=-1).view(N, K)]
        scale = torch.pow(2.0, self.scale.to(torch.float32) - 127.0)         # exact: integer exponents within [-125, 125]
        return (val.view(N, K // 32, 32) * scale[..., None]).view(N, K).to(torch.bfloat16)


CODED = {cls.name: cls for cls in (W8, W4)}          # by the mode value (suffix_weights / suffix_mx / prefill_precision / batch_prefill)


def _fake_quant_rows(x):
    """bf16(code * scale) of hip.quant_fp8_rows(x): what a projection of prefill_precision="fp8" sees of its input rows, as bf16."""
    return W8.of(x).dequantised()


def _operands(weights):
    """(format row, the W [and scale] arguments) of a projection's weights as ONE launch reads them: a coded weight as it is, bf16 views
    as their common view -- None when they are not adjacent in memory."""
    if isinstance(weights, _Coded):
        return weights.fmt, tuple(weights)
    wcat = ops.cat_view(weights) if len(weights) > 1 else weights[0]
    return hip.WEIGHT_FORMATS["bf16"], (None if wcat is None else (wcat,))


class _CachedEpsBase:
    """What the cached-prefix engines share: the packed weights, the captured suffix pass and the `model(x, t)` call of the samplers.
    A subclass provides prefill() and _suffix_pass() and sets B, R, T, H, h_in, h_out, cache."""

    suffix_operand = "fused"         # MODES: read by PrefixCachedEps._suffix_pass; the row-GEMM engines form the operand once anyway
    suffix_mx = "off"                # MODES: read by _stream; "off" leaves the choice to suffix_weights

    def __init__(self, vlm, n_action_rows: int = 1, modes: Modes = Modes()):
        """modes: as the factory validated them (engine_modes). The multi-row engines' attention mode is groups_attention."""
        self.suffix_weights, self.prefill_mode, self.prefill_precision = modes.suffix_weights, modes.prefill, modes.prefill_precision
        self.suffix_attention = "split" if "split" in (modes.suffix_attention, modes.groups_attention) else "head"
        self.suffix_operand, self.batch_prefill, self.suffix_mx = modes.suffix_operand, modes.batch_prefill, modes.suffix_mx
        self._attn_ws = None         # "split": the partial softmax states of mla_attn_chunk_split, allocated once beside h_in / h_out
        self._prefill_ws = None      # "compact": the split-K workspace of the prefill GEMMs, allocated once beside h_in / h_out
        self._prefill_xq = None      # prefill_precision "fp8": the projection inputs' codes (one buffer, viewed [rows, K]) ...
        self._prefill_xs = None      # ... and their scales [rows], allocated once beside _prefill_ws
        self.vlm = vlm
        llm = vlm.llm_backbone.llm
        self.model, self.cfg = llm.model, llm.config
        self.T = n_action_rows
        self.R = 1 + self.T
        self.nheads, self.eps = self.cfg.num_attention_heads, self.cfg.rms_norm_eps
        self.cache = None
        self.graph = None
        self._graph_failed = False
        self.graph_error = None      # why the suffix pass could not be captured (eager launches then), for diagnostics
        self._packed = None          # per layer: the 9 weights with q|k|v and gate|up as views of ONE buffer each (see _weights)
        self._packed_key = None
        self._suffix = None          # per layer: what the suffix pass streams -- _packed itself ("bf16") or a form of a coded copy (_weight_copy)
        self._ddim = {}              # sample_ddim's state per (B, action_dim): see _DdimState
        self._ddpm = {}              # sample_ddpm's, kept apart: a DDIM and a DDPM call on one engine keep their captured steps
        self._ddim_pin = {}          # the states of the pinned calls (pin=), kept apart in the same way: the un-pinned call replays ...
        self._ddpm_pin = {}          # ... the step it replays without them, whatever pinned calls ran in between
        self._dpmpp2m = {}           # sample_dpmpp2m's states, kept apart like the DDPM ones: a DDIM call replays the step it always ...
        self._dpmpp2m_pin = {}       # ... replayed, whatever solver ran in between

    @classmethod
    def _serves(cls, vlm, rows: int, limit: int, tag: tuple, message: str, warn: bool = True) -> bool:
        """The shape predicate of every engine (supports*): `rows` suffix rows within `limit` and head_dim 128. Otherwise False, with
        `message` as a RuntimeWarning once per (tag, rows, head_dim) and model unless warn=False."""
        cfg = vlm.llm_backbone.llm.config
        D = cfg.hidden_size // cfg.num_attention_heads
        if rows <= limit and D == 128:
            return True
        seen = vlm.__dict__.setdefault("_prefix_unsupported", set())
        if warn and tag + (rows, D) not in seen:
            seen.add(tag + (rows, D))
            warnings.warn(message.format(rows=rows, limit=limit, D=D), RuntimeWarning, stacklevel=4)
        return False

    @classmethod
    def _engine(cls, vlm, store: str, key: tuple, ctor: tuple, **modes):
        """The vlm's engine for `key` in vlm.__dict__[store], constructed as cls(vlm, *ctor) on first use; at most 4 per store, the oldest
        leaves first. An engine's mode (Modes' fields as keywords) other than the default is part of the key, as its row of MODES tags it
        -- the engines coexist: a captured graph holds the addresses of ITS weights and ITS attention launches. The caller prefills."""
        engines = vlm.__dict__.setdefault(store, {})
        key += tuple(mode.tag + value for mode, value in zip(MODES.values(), Modes(**modes)) if mode.tag is not None and value != mode.values[0])
        eng = engines.get(key)
        if eng is None:
            if len(engines) >= 4:
                engines.pop(next(iter(engines)))
            eng = engines[key] = cls(vlm, *ctor)
        return eng

    def _weights(self):
        """Every layer's (ln1, wq, wk, wv, wo, ln2, wg, wu, wd) with q|k|v and gate|up adjacent in memory, so that the prefill runs the
        fused QKV + RoPE and gate|up + SwiGLU GEMMs and a suffix pass needs one GEMV each instead of three / two (33 MB projections are
        ~40 % launch + ramp). Under FSDPStrategy the parameters already live like that in the unit's flat buffer (views are used as they
        are); otherwise the engine keeps packed COPIES (9.4 GB at 7B), rebuilt when a parameter's storage or version changes."""
        key = tuple((p.data_ptr(), p._version) for layer in self.model.layers for p in layer._weights())
        shared = self.vlm.__dict__.setdefault("_prefix_packed", {})          # one packed copy per model, shared by its engines
        if shared.get("key") != key:
            packed = []
            with torch.no_grad(), torch.inference_mode(False):
                for layer in self.model.layers:
                    ln1, wq, wk, wv, wo, ln2, wg, wu, wd = layer._weights()
                    if ops.cat_view((wq, wk, wv)) is None:
                        buf = torch.cat([wq.detach(), wk.detach(), wv.detach()], 0)
                        H = wq.shape[0]
                        wq, wk, wv = buf[:H], buf[H:H + wk.shape[0]], buf[H + wk.shape[0]:]
                    if ops.cat_view((wg, wu)) is None:
                        buf = torch.cat([wg.detach(), wu.detach()], 0)
                        wg, wu = buf[:wg.shape[0]], buf[wg.shape[0]:]
                    packed.append((ln1, wq, wk, wv, wo, ln2, wg, wu, wd))
            shared["key"], shared["packed"] = key, packed
        if self._packed is not shared["packed"]:
            self.graph = None            # a captured pass holds the previous buffers' addresses
            self._packed, self._packed_key = shared["packed"], key
        coded = CODED.get(self._stream.removesuffix("_as_bf16"))
        suffix = self._packed if coded is None else self._weight_copy(coded, self._stream)
        if self._suffix is not suffix:
            self.graph = None
            self._suffix = suffix
        return self._packed

    @property
    def _stream(self) -> str:
        """What the suffix pass streams, as the value of the one keyword that says so: suffix_mx unless it is "off", else suffix_weights
        (check_one_suffix_copy: at most one of the two is away from its default). A key of CODED: the pass streams codes."""
        return self.suffix_weights if self.suffix_mx == "off" else self.suffix_mx

    def _weight_copy(self, coded, form):
        """The model's copy of the decoder projections in the format `coded` (W8 / W4), as `form` (call behind _weights()):
        coded.name -- per layer (ln1, coded q|k|v, coded o, ln2, coded gate|up, coded down), quantised from the packed copy (a scale
        belongs to one row or to a block inside one, so the packed matrices quantise as one);
        coded.name + "_as_bf16" -- the packed tuple's layout with the dequantised matrices, built from the same codes on first use.
        One per model and format in its own slot of vlm.__dict__, independent of the other format's and shared by the model's engines --
        the suffix pass, and for W8 the prefill of prefill_precision / batch_prefill whatever the suffix pass streams --, keyed like the
        packed copy on (data_ptr, _version) of the layer weights and rebuilt when that changes."""
        shared = self.vlm.__dict__.setdefault(coded.slot, {})
        if shared.get("key") != self._packed_key:
            layers, nbytes = [], 0
            with torch.no_grad(), torch.inference_mode(False):
                for ln1, wq, wk, wv, wo, ln2, wg, wu, wd in self._packed:
                    mats = [coded.of(m) for m in (ops.cat_view((wq, wk, wv)), wo, ops.cat_view((wg, wu)), wd)]
                    nbytes += sum(m.nbytes for m in mats)
                    layers.append((ln1, mats[0], mats[1], ln2, mats[2], mats[3]))
            shared.clear()
            shared["key"], shared[coded.name] = self._packed_key, layers
            _LOG.info("%s copy of the decoder projections, %.2f GB beside the bf16 weights", coded.label, nbytes / 1e9)
        if form not in shared:
            deq = []
            with torch.no_grad(), torch.inference_mode(False):
                for (ln1, qkv, o, ln2, gu, d), packed in zip(shared[coded.name], self._packed):
                    qkv, o, gu, d = (m.dequantised() for m in (qkv, o, gu, d))
                    nq, nk, ng = packed[1].shape[0], packed[2].shape[0], packed[6].shape[0]
                    deq.append((ln1, qkv[:nq], qkv[nq:nq + nk], qkv[nq + nk:], o, ln2, gu[:ng], gu[ng:], d))
            shared[form] = deq
        return shared[form]

    def _suffix_layers(self):
        """Per layer ((ln1, qkv, o, ln2, gate_up, down), cache) of a suffix pass: every projection one coded weight (_stream "fp8" / "fp4")
        or a tuple of bf16 matrices -- views of the packed 9-tuple ("bf16") or of a dequantised twin ("fp8_as_bf16", "fp4_as_bf16")."""
        for w, c in zip(self._suffix, self.cache):
            yield (w if self._stream in CODED else (w[0], w[1:4], w[4:5], w[5], w[6:8], w[8:9])), c

    def _finish(self, h):
        """The end of every suffix pass: the model's final norm over the rows, into the static output rows."""
        hn, _ = hip.rmsnorm_fwd(h, self.model.norm.weight, self.eps)
        self.h_out.copy_(hn)

    def _prefill_rows(self, h, B, S_p, out_bs, weights=None):
        """The decoder layers over the prefix rows h [B * S_p, H] of B samples with S_p rows each, every layer's packed post-RoPE q|k|v
        rows (`LayerActs.qkv`) into rows [0, S_p) of its cache ([B, S_cap, 3H], or [rows, 3H] for one sample): on the training forward
        kernels, one layer at a time, or ("compact") on the row-sized GEMMs, which write the cache rows themselves (sample b at element
        offset b * out_bs). weights: what _weights() returned, when the caller has called it already."""
        if self.prefill_mode == "compact":
            self._compact_prefill(h, B, S_p, self.cache, out_bs)
            return
        for w, c in zip(self._weights() if weights is None else weights, self.cache):
            h, acts = ops.DecoderLayerFn._fwd(h, None, self.cos_p, self.sin_p, B, S_p, self.nheads, self.eps, w)
            rows = c[:, :S_p] if c.dim() == 3 else c[:S_p]
            rows.copy_(acts.qkv[:B * S_p].view(rows.shape))
            del acts

    def _prefix_rows(self, input_ids, k, images, point_cloud, camera_name, proprio, tactile=None, gripper_xyz=None):
        """The decoder's input rows in front of the [t, x] tokens, [B, S_p, H]: [BOS | fused tokens | text[1:k] | proprio] (call under no_grad)."""
        vlm = self.vlm
        parts, _, _, _, _, _ = vlm.get_fused_tokens(images, point_cloud, tactile, gripper_xyz, camera_name)
        vlm.vision_tower_2d.assert_masks_ok()
        text_emb = vlm.llm_backbone.embed_input_ids(input_ids)
        proprio_e = vlm.proprio_embedder(proprio.to(torch.bfloat16))
        return torch.cat([text_emb[:, :1]] + parts + [text_emb[:, 1:k], proprio_e], dim=1).contiguous()

    # ------------------------------------------------------------------------------------------ the compact prefill
    def _check_compact(self, rows: int):
        """prefill="compact" serves at most 1024 prefix rows at head_dim 128; anything else is an error, never a silent "train" prefill."""
        if self.prefill_mode != "compact":
            return
        D = self.cfg.hidden_size // self.nheads
        if rows > hip.PREFILL_MMAX or D != 128:
            raise ValueError(f"prefill=\"compact\" serves at most {hip.PREFILL_MMAX} prefix rows at head_dim 128 (got {rows} rows, head_dim "
                             f"{D}); use prefill=\"train\"")

    def _compact_buffers(self, rows, dev, precision=None):
        """What the compact prefill keeps per engine, allocated once (call outside inference mode): ONE split-K workspace for the four
        projections of a layer at `rows` rows (the launches of a prefill run one after the other) and, for precision "fp8" (default:
        prefill_precision), the projection inputs' codes and scales. rows: the row count, or every row count the engine may launch (the
        batched engines: a plan splits less as the rows grow, so the largest row count need not need the largest workspace)."""
        H, I = self.cfg.hidden_size, self.cfg.intermediate_size
        fp8 = (self.prefill_precision if precision is None else precision) == "fp8"
        counts = (rows,) if isinstance(rows, int) else tuple(rows)
        rows = max(counts)
        kind = hip.PREFILL_KINDS["fp8" if fp8 else "bf16"]
        if fp8 and rows > hip.PREFILL_MMAX:
            kind = hip.PREFILL_KIND_F8_WIDE
        need = [kind.ws_bytes(M, N, K) for M in counts for N, K in ((3 * H, H), (H, H), (2 * I, H), (H, I))]
        if min(need) < 0:
            raise ValueError(f"prefill=\"compact\": the projections of this model (hidden {H}, intermediate {I}) are outside the compact "
                             f"GEMMs' contract (N % 128 == 0, K % {kind.k_gran} == 0); use prefill=\"train\"")
        self._prefill_ws = torch.empty(max(max(need), 16), dtype=torch.uint8, device=dev)
        if fp8:
            self._prefill_xq = torch.empty(rows * max(H, I), dtype=torch.float8_e4m3fn, device=dev)
            self._prefill_xs = torch.empty(rows, dtype=torch.float32, device=dev)

    def _prefill_layers(self):
        """Per layer what _compact_layer runs on: the packed 9-tuple ("bf16"), its dequantised twin ("fp8_as_bf16") or the W8 6-tuple
        ("fp8") of the model's FP8 copy (_weight_copy)."""
        packed = self._weights()
        return packed if self.prefill_precision == "bf16" else self._weight_copy(W8, self.prefill_precision)

    def _compact_prefill(self, h, B, S_p, cache_out, out_bs):
        """The decoder layers over the B * S_p prefix rows h [B * S_p, H] on the compact GEMMs; cache_out[l] is layer l's cache tensor whose
        sample b holds its rows at element offset b * out_bs + p * row stride."""
        for w, c in zip(self._prefill_layers(), cache_out):
            h = self._compact_layer(w, h, B, S_p, c, out_bs)
        return h

    def _compact_layer(self, w, h, B, S_p, c, out_bs, precision=None, rope=None):
        """One decoder layer of the compact prefill on its weights w (an entry of _prefill_layers()) -> the layer's output rows: rmsnorm_fwd,
        q|k|v + RoPE into the cache c, the training flash attention on the cache's q / k / v views, o + residual, rmsnorm_fwd, gate|up +
        SwiGLU (the product only), down + residual. The precision only decides how a projection's input and weight are presented:
        "bf16" as they are; "fp8_as_bf16" the dequantised weights, every input quantised and dequantised per row; "fp8" the W8 codes and
        scales, every input quantised per row into the engine's code / scale buffers (mla_quant_fp8_rows) for the GEMMs over codes.
        Norms, attention, cache and residual stream are bf16 throughout. precision / rope: the batched engines' batch_prefill mode and
        their tables for S_p rows (default: prefill_precision, cos_p / sin_p); more than 1024 rows of codes run on the wide-row GEMMs."""
        H, D, ws, M = self.H, self.D, self._prefill_ws, B * S_p
        precision = self.prefill_precision if precision is None else precision
        cos_p, sin_p = (self.cos_p, self.sin_p) if rope is None else rope
        if precision == "fp8" and M > hip.PREFILL_MMAX:
            ln1, wqkv, wo, ln2, wgu, wd = w
            plain, qkv_rope, gateup_swiglu = hip.gemm_prefill_f8_wide, hip.gemm_prefill_f8_wide_qkv_rope, hip.gemm_prefill_f8_wide_gateup_swiglu
        elif precision == "fp8":
            ln1, wqkv, wo, ln2, wgu, wd = w
            plain, qkv_rope, gateup_swiglu = hip.gemm_prefill_f8, hip.gemm_prefill_f8_qkv_rope, hip.gemm_prefill_f8_gateup_swiglu
        else:
            ln1, wq, wk, wv, wo, ln2, wg, wu, wd = w
            wqkv, wgu = ops.cat_view((wq, wk, wv)), ops.cat_view((wg, wu))
            assert wqkv is not None and wgu is not None, "the packed weights are adjacent in memory (_weights)"
            plain, qkv_rope, gateup_swiglu = hip.gemm_prefill, hip.gemm_prefill_qkv_rope, hip.gemm_prefill_gateup_swiglu

        def operands(x, W):
            if precision == "fp8":
                K = x.shape[1]
                return (*hip.quant_fp8_rows(x, self._prefill_xq[:M * K].view(M, K), self._prefill_xs[:M]), W.q, W.scale)
            return (_fake_quant_rows(x) if precision == "fp8_as_bf16" else x), W
        ld = c.stride(-2)
        xn, _ = hip.rmsnorm_fwd(h, ln1, self.eps)
        qkv_rope(*operands(xn, wqkv), c, ld, out_bs, S_p, (cos_p, sin_p, 2 * H), D, ws=ws)
        o = self._prefill_attention(c, B, S_p, ld, out_bs)
        h1 = torch.empty_like(h)
        plain(*operands(o, wo), h1, H, 0, M, residual=h, ws=ws)
        xn2, _ = hip.rmsnorm_fwd(h1, ln2, self.eps)
        act = torch.empty((M, self.cfg.intermediate_size), dtype=torch.bfloat16, device=h.device)
        gateup_swiglu(*operands(xn2, wgu), act, ws=ws)
        h = torch.empty_like(h1)
        plain(*operands(act, wd), h, H, 0, M, residual=h1, ws=ws)
        return h

    def _prefill_attention(self, c, B, S_p, ld, out_bs):
        """The training flash attention over the prefix rows of the cache c, per sample -> o [B * S_p, H]."""
        H, flat = self.H, c.reshape(-1)
        o = [hip.attn_fwd(*(flat[b * out_bs + j * H:] for j in range(3)), 1, S_p, self.nheads, self.D, ld, None, 1.0 / math.sqrt(self.D))[0]
             for b in range(B)]
        return o[0] if B == 1 else torch.cat(o, 0)

    def _run(self):
        if _USE_GRAPH and not self._graph_failed:
            if self.graph is None:
                try:
                    self._suffix_pass()                                      # warm-up outside the capture (function attributes, allocator)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    # captured outside inference mode: the generator's graph-state tensors are created by the first capture of a
                    # process and live as long as any graph does -- as inference tensors they would make every later capture that
                    # runs outside inference mode fail; the pass itself only touches the engine's (normal) buffers
                    with torch.inference_mode(False), torch.no_grad(), torch.cuda.graph(g):
                        self._suffix_pass()
                    self.graph = g
                except Exception as e:   # noqa: BLE001 -- a failed capture is not fatal: the eager launches compute the same thing
                    self._graph_failed, self.graph_error = True, repr(e)
                    self.graph = None
                    torch.cuda.synchronize()
            if self.graph is not None:
                self.graph.replay()
                return
        self._suffix_pass()

    # ------------------------------------------------------------------------------------------ the model(x, t, **kw) the samplers call
    def __call__(self, x, t, **ignored):
        """Same contract as PrismaticVLM.forward in eval mode: returns (None, noise_pred [B, T, action_dim])."""
        vlm, bf16 = self.vlm, torch.bfloat16
        with torch.no_grad():
            x_e = vlm.x_embedder(x.to(bf16))                                  # [B, T, H]   (prismatic.py:873-880 casts)
            t_e = vlm.t_embedder(t.to(bf16)).unsqueeze(1)                     # [B, 1, H]
            assert x_e.shape[1] == self.T, (x_e.shape, self.T)
            self.h_in.copy_(torch.cat([t_e, x_e], dim=1).reshape(self.B * self.R, self.H))
            self._run()
            picked = self.h_out.view(self.B, self.R, self.H)[:, 1:].reshape(self.B * self.T, self.H).contiguous()
            noise_pred = vlm.final_layer(picked).view(self.B, self.T, -1)
        return None, noise_pred

    # ----------------------------------------------------- the sampler loops on the device (sampler="device", ddpm_sampler="device")
    def _sampler_state(self, x0, diffusion, loop: str, pinned: bool = False):
        """The persistent state of the "ddim", "ddpm" or "dpmpp2m" loop (kept in _ddim / _ddpm / _dpmpp2m, a pinned call's in _ddim_pin /
        _ddpm_pin / _dpmpp2m_pin: the six do not evict each other's captured steps) for chunks shaped like x0 [B, T, D] under
        `diffusion` (per B: the group engines keep one per set_groups G)."""
        B, T, D = x0.shape
        assert B == self.B and T == self.T, (tuple(x0.shape), self.B, self.T)
        ddpm = loop == "ddpm"
        store = getattr(self, "_" + loop + ("_pin" if pinned else ""))
        st = store.get((B, D))
        if st is None or st.diffusion is not diffusion:
            dev = self.h_in.device
            coef, timesteps = {"ddim": lambda: diffusion.ddim_tables(dev, eta=0.0), "ddpm": lambda: diffusion.ddpm_tables(dev),
                               "dpmpp2m": lambda: diffusion.dpmpp2m_tables(dev)}[loop]()
            st = _DdimState()
            st.diffusion, st.steps, st.timesteps = diffusion, int(coef.shape[0]), timesteps
            with torch.inference_mode(False), torch.no_grad():                # the state outlives the (inference-mode) call that creates it
                st.x = torch.zeros((B, T, D), dtype=torch.float32, device=dev)
                st.x_bf16 = torch.zeros((B, T, D), dtype=torch.bfloat16, device=dev)
                st.step = torch.full((1,), st.steps - 1, dtype=torch.int32, device=dev)
                st.coef = coef.clone()
                st.t_table = torch.zeros((st.steps, self.H), dtype=torch.bfloat16, device=dev)
                st.noise = torch.zeros((st.steps, B * T * D), dtype=torch.float32, device=dev) if ddpm else None
                st.hist = torch.zeros((B, T, D), dtype=torch.float32, device=dev) if loop == "dpmpp2m" else None
                st.known = torch.zeros((B, T, D), dtype=torch.float32, device=dev) if pinned else None
                st.pin = torch.zeros((B, T, D), dtype=torch.uint8, device=dev) if pinned else None
            st.t_key = st.graph = st.graph_key = None
            st.failed = False
            store[(B, D)] = st
        return st

    def _sampler_t_table(self, st):
        """Row i of t_table = the timestep token of step i: vlm.t_embedder on the [B] batch of the mapped timestep cast to bf16, exactly
        as __call__ forms it per step (row 0 of B equal rows, checked once per build: the bits do not depend on how the GEMM treats the
        row count). Rebuilt in place -- a captured step keeps its address -- when a t_embedder parameter changes."""
        key = tuple((p.data_ptr(), p._version) for p in self.vlm.t_embedder.parameters())
        if st.t_key == key:
            return
        with torch.no_grad():
            rows = torch.stack([self.vlm.t_embedder(st.timesteps[i].expand(self.B).to(torch.bfloat16)) for i in range(st.steps)])
            if not bool((rows == rows[:, :1]).all()):
                raise RuntimeError("device sampler: t_embedder gives different rows for the same timestep; the device loop keeps one row "
                                   "per step (use the host loop)")
            st.t_table.copy_(rows[:, 0])
        st.t_key = key

    def _sampler_one_step(self, st):
        """One sampler step, every launch on the current stream and none of them waiting for the host: the launches of __call__ with the
        timestep token looked up (mla_sampler_rows), then the state's update (DDIM, DDPM with the step's row of st.noise, or
        DPM-Solver++(2M) with st.hist; the pinned kernels on a pinned state), which counts the device-side step index down."""
        vlm = self.vlm
        x_e = vlm.x_embedder(st.x_bf16)                                       # [B, T, H]
        hip.sampler_rows(self.h_in, st.t_table, x_e.contiguous(), st.step, self.B, self.T)
        self._suffix_pass()                                                   # launched directly: a graph cannot replay inside a capture
        picked = self.h_out.view(self.B, self.R, self.H)[:, 1:].reshape(self.B * self.T, self.H).contiguous()
        noise_pred = vlm.final_layer(picked)                                  # [B * T, D] bf16
        if st.hist is not None:
            if st.pin is None:
                hip.dpmpp2m_step(st.x, noise_pred.contiguous(), st.x_bf16, st.hist, st.coef, st.step, advance=True)
            else:
                hip.dpmpp2m_step_pin(st.x, noise_pred.contiguous(), st.x_bf16, st.hist, st.coef, st.known, st.pin, st.step, advance=True)
        elif st.pin is None:
            if st.noise is None:
                hip.ddim_step(st.x, noise_pred.contiguous(), st.x_bf16, st.coef, st.step, advance=True)
            else:
                hip.ddpm_step(st.x, noise_pred.contiguous(), st.x_bf16, st.coef, st.noise, st.step, advance=True)
        elif st.noise is None:
            hip.ddim_step_pin(st.x, noise_pred.contiguous(), st.x_bf16, st.coef, st.known, st.pin, st.step, advance=True)
        else:
            hip.ddpm_step_pin(st.x, noise_pred.contiguous(), st.x_bf16, st.coef, st.noise, st.known, st.pin, st.step, advance=True)

    def _sampler_graph(self, st):
        """The captured step for the current weights, or None (MLA_INFER_GRAPH=0 or a failed capture: eager launches of the same sequence,
        the reason in graph_error). Captured under _run's conditions; the warm-up launch runs a real step on the state, so this is called
        in front of the reset of a call."""
        if not _USE_GRAPH:
            if self.graph_error is None:
                self.graph_error = _GRAPH_OFF
            return None
        if st.failed:
            return None
        if self.graph_error == _GRAPH_OFF:
            self.graph_error = None
        key = (self._packed_key, self.suffix_weights, self.suffix_mx,
               tuple(p.data_ptr() for m in (self.vlm.x_embedder, self.vlm.final_layer) for p in m.parameters()))
        if st.graph is None or st.graph_key != key:
            st.graph = None
            try:
                with torch.no_grad():
                    self._sampler_one_step(st)                                # warm-up outside the capture (function attributes, allocator)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.inference_mode(False), torch.no_grad(), torch.cuda.graph(g):
                    self._sampler_one_step(st)
                st.graph, st.graph_key = g, key
            except Exception as e:   # noqa: BLE001 -- a failed capture is not fatal: the eager launches compute the same thing
                st.failed, self.graph_error = True, repr(e)
                st.graph = None
                torch.cuda.synchronize()
        return st.graph

    def _sampler_loop(self, st, x0, pin=None):
        """What the device loops share behind the state lookup: the timestep-token table and the captured step for the current
        weights, the reset of the state to x0 and step steps - 1, and st.steps replays (or eager steps). A DDPM state: in front of the
        replays, one randn_like(x) per step in the host loop's order (step steps - 1 first) into row s of st.noise -- asynchronous
        launches. A DPM-Solver++(2M) state: st.hist is zeroed in the reset (behind the capture, whose warm-up step wrote a prediction
        there: the first step forms 0 * hist). A pinned state: pin = (known, mask) is copied into st.known / st.pin in front of the
        replays (behind the capture: its warm-up step runs on whatever the last call left there)."""
        self._sampler_t_table(st)
        graph = self._sampler_graph(st)
        with torch.no_grad():
            st.x.copy_(x0)
            st.x_bf16.copy_(x0.to(torch.bfloat16))
            st.step.fill_(st.steps - 1)
            if st.hist is not None:
                st.hist.zero_()
            if pin is not None:
                st.known.copy_(pin[0])
                st.pin.copy_(pin[1])
            if st.noise is not None:
                for s in reversed(range(st.steps)):
                    st.noise[s].copy_(torch.randn_like(st.x).view(-1))
            for _ in range(st.steps):
                if graph is not None:
                    graph.replay()
                else:
                    self._sampler_one_step(st)

    @staticmethod
    def _check_pin(x0, pin):
        """pin = (known, mask) of a pinned device loop: both shaped like x0, known floating point, mask bool."""
        if pin is None:
            return
        known, mask = pin
        if tuple(known.shape) != tuple(x0.shape) or tuple(mask.shape) != tuple(x0.shape) or mask.dtype != torch.bool \
                or not known.is_floating_point():
            raise ValueError(f"pin: known {tuple(known.shape)} {known.dtype} and mask {tuple(mask.shape)} {mask.dtype} must be a "
                             f"floating-point and a bool tensor shaped like the chunk {tuple(x0.shape)}")

    def sample_ddim(self, x0, diffusion, pin=None):
        """ddim_sample_loop(self, x0.shape, x0, clip_denoised=False, eta=0.0) of `diffusion` with the loop on the device -> samples
        [B, T, D] fp32, the same bits. pin = (known [B, T, D] fp32, mask [B, T, D] bool): the loop with denoised_fn =
        where(mask, known, .) -- every step's x0 prediction is `known` where `mask` is set (mla_ddim_step_pin; the result there == known)
        -- on a state and a captured step of its own: the un-pinned call replays the step it replays without pinned calls. After the (already done) prefill the host enqueues diffusion.num_timesteps replays of one captured
        sampler step (x_embedder, mla_sampler_rows, the suffix pass, final_layer, mla_ddim_step) and returns; nothing is copied to the
        device and the host never waits for the device between the steps. The generator ends where the host loop leaves it (one unused
        randn_like per step)."""
        x0 = x0.float()
        self._check_pin(x0, pin)
        st = self._sampler_state(x0, diffusion, "ddim", pinned=pin is not None)
        self._sampler_loop(st, x0, pin)
        with torch.no_grad():
            for _ in range(st.steps):
                torch.randn_like(st.x)                                        # ddim_sample draws its noise even at eta = 0
            return st.x.clone()

    def sample_ddpm(self, x0, diffusion, pin=None):
        """p_sample_loop(self, x0.shape, x0, clip_denoised=False) of `diffusion` with the loop on the device -> samples [B, T, D] fp32,
        the same bits. pin: sample_ddim's (mla_ddpm_step_pin), the draws and the generator position are the un-pinned call's. The host first enqueues the loop's num_timesteps randn_like draws, in the loop's order, into the state's noise
        table -- the suffix pass draws nothing, so every step sees the values the host loop's own draw would have given it, and the
        generator ends where the host loop leaves it -- then num_timesteps replays of one captured sampler step (x_embedder,
        mla_sampler_rows, the suffix pass, final_layer, mla_ddpm_step reading row *step of the table). Nothing is copied to the device and
        the host never waits for the device between the steps."""
        x0 = x0.float()
        self._check_pin(x0, pin)
        st = self._sampler_state(x0, diffusion, "ddpm", pinned=pin is not None)
        self._sampler_loop(st, x0, pin)
        with torch.no_grad():
            return st.x.clone()

    def sample_dpmpp2m(self, x0, diffusion, pin=None):
        """dpmpp2m_sample_loop(self, x0.shape, x0, clip_denoised=False) of `diffusion` (DPM-Solver++(2M) on the respaced process) with the
        loop on the device -> samples [B, T, D] fp32, the same bits. pin: sample_ddim's (mla_dpmpp2m_step_pin: the pinned entries of
        every step's x0 prediction, of the history and of the result == known). A state and a captured step of its own (x_embedder,
        mla_sampler_rows, the suffix pass, final_layer, mla_dpmpp2m_step[_pin]), which also holds the previous step's x0 prediction,
        zeroed at the reset: the DDIM and DDPM states and their captured steps are not touched. Nothing is copied to the device, the host
        never waits for the device between the steps, and nothing is drawn: the generator stays where the host loop leaves it."""
        x0 = x0.float()
        self._check_pin(x0, pin)
        st = self._sampler_state(x0, diffusion, "dpmpp2m", pinned=pin is not None)
        self._sampler_loop(st, x0, pin)
        with torch.no_grad():
            return st.x.clone()



class PrefixCachedEps(_CachedEpsBase):
    """One engine per (batch, prefix length, action rows): the per-layer q|k|v cache, the suffix pass's static input / output rows and its
    captured graph live as long as the engine, `prefill()` refreshes the cache for a new observation (the graph stays valid: same
    addresses). `PrefixCachedEps.for_inputs(vlm, ...)` returns the vlm's engine for the given inputs, prefilled."""

    @staticmethod
    def _splice_position(input_ids):
        L = input_ids.shape[1]
        is_tag = input_ids == SPLICE_TAG
        if not bool(is_tag.any(dim=1).all()):
            raise IndexError(f"input_ids row without the splice tag {SPLICE_TAG} (models/vlm/prismatic.py:983)")
        k = (L - 1 - torch.flip(is_tag, dims=[1]).int().argmax(dim=1))       # last occurrence per row
        if not bool((k == k[0]).all()):
            raise ValueError("PrefixCachedEps needs the same splice position in every row (predict_action_diff is batch 1)")
        return int(k[0])

    MAX_ROWS = 64                    # B * (1 + T) suffix rows: mla_gemm_skinny_bf16 / mla_attn_chunk serve up to 64

    @classmethod
    def supports(cls, vlm, batch: int, n_action_rows: int) -> bool:
        """Whether the suffix pass's kernels serve this shape: B * (1 + T) <= 64 rows and head_dim 128. Otherwise the caller runs the
        reference's control flow (a whole forward per sampler step); warns once per shape."""
        return cls._serves(vlm, batch * (1 + n_action_rows), cls.MAX_ROWS, (), "PrefixCachedEps: {rows} suffix rows (max {limit}) / head_dim "
                           "{D} (needs 128) are beyond the cached-prefix kernels; sampling with a whole forward per step")

    @classmethod
    def for_inputs(cls, vlm, input_ids, n_action_rows: int = 1, suffix_weights: str = "bf16", prefill: str = "train",
                   suffix_attention: str = "head", prefill_precision: str = "bf16", suffix_operand: str = "fused", suffix_mx: str = "off",
                   **model_kwargs):
        modes = engine_modes(suffix_weights=suffix_weights, suffix_mx=suffix_mx, prefill=prefill, suffix_attention=suffix_attention,
                             prefill_precision=prefill_precision, suffix_operand=suffix_operand)
        k = cls._splice_position(input_ids)
        # a handful of prompt lengths per process; each engine holds 0.4 GB at 7B
        eng = cls._engine(vlm, "_prefix_engines", (int(input_ids.shape[0]), k, int(n_action_rows), str(input_ids.device)),
                          (n_action_rows, modes), **modes._asdict())
        eng.prefill(input_ids, k, **model_kwargs)
        return eng

    def prefill(self, input_ids, k, images=None, point_cloud=None, camera_name=None, proprio=None, tactile=None, gripper_xyz=None, **unused):
        bf16, dev = torch.bfloat16, input_ids.device
        with torch.no_grad():
            prefix = self._prefix_rows(input_ids, k, images, point_cloud, camera_name, proprio, tactile, gripper_xyz)       # [B, S_p, H]
            B, S_p, H = prefix.shape
            self._check_compact(B * S_p)
            if self.cache is None:
                self.B, self.S_p, self.H = B, S_p, H
                self.S_cap = S_p + self.R
                self.D = H // self.nheads
                rot = self.model.layers[0].self_attn.rotary_emb
                self.cos_p, self.sin_p = rot.tables(S_p, dev)
                cos_c, sin_c = rot.tables(self.S_cap, dev)
                self.cos_s, self.sin_s = cos_c[S_p:].contiguous(), sin_c[S_p:].contiguous()
                with torch.inference_mode(False):                            # the engine outlives the (inference-mode) call that creates it
                    self.cache = [torch.empty((B, self.S_cap, 3 * H), dtype=bf16, device=dev) for _ in self.model.layers]
                    self.h_in = torch.zeros((B * self.R, H), dtype=bf16, device=dev)
                    self.h_out = torch.zeros((B * self.R, H), dtype=bf16, device=dev)
                    if self.prefill_mode == "compact":
                        self._compact_buffers(B * S_p, dev)
                    if self.suffix_attention == "split":
                        need = hip.attn_split_ws_bytes(B, self.nheads, self.R, self.S_cap)
                        if need < 0:
                            raise RuntimeError(f"mla_attn_chunk_split_ws_bytes: {hip.lib().mla_last_error().decode()}")
                        self._attn_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            assert (B, S_p, H) == (self.B, self.S_p, self.H)
            self._prefill_rows(prefix.reshape(B * S_p, H), B, S_p, self.cache[0].stride(0))

    def _suffix_attn(self):
        """The attention launch of the suffix pass: "head" -- mla_attn_decode where the R x S_kv scores fit LDS, mla_attn_chunk's online
        softmax beyond; "split" -- mla_attn_chunk_split with the library's plan for every R, on the engine's workspace. No fallback: with
        head_dim other than 128 the launcher refuses (PrefixCachedEps.supports keeps such models off the engine)."""
        if self.suffix_attention == "split":
            ws = self._attn_ws
            return lambda c, B, nheads, D, S_kv, R, scale: hip.attn_chunk_split(c, B, nheads, D, S_kv, R, scale, ws=ws)
        return hip.attn_decode if hip.attn_decode_fits(self.R, self.S_cap) else hip.attn_chunk

    # ------------------------------------------------------------------------------------------ one pass over the suffix rows
    def _gemv(self, x, weights, out=None, residual=None, rpb=1, out_bs=0, **pre):
        """f(x) [M, K] @ W^T (+ residual) -> [M, N]; `weights` is one coded weight or a tuple of bf16 matrices: one launch (_operands),
        or one per matrix when the bf16 matrices are not adjacent in memory.
        pre: norm_weight= / eps= (RMSNorm of the rows) or swiglu=True (x = packed gate|up rows), applied inside the kernel's input staging."""
        fmt, W = _operands(weights)
        M = x.shape[0]
        N, K = (sum(w.shape[0] for w in weights), weights[0].shape[1]) if W is None else (W[0].shape[0], W[0].shape[1] * fmt.k_per_col)
        if out is None:
            out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
            rpb, out_bs = M, 0
        ldo = out.stride(-2)
        # mla_gemv_* wherever it accepts the rows (the results of every configuration it served stay bit for bit the same), the MFMA
        # skinny GEMM beyond (M > 8, or the M x K input rows do not fit the LDS: 7B down projection at M = 8). Measured for w8 at 7B
        # (profiles/fp8_infer_latency.txt): right at M = 2; at M = 5 .. 8 the MFMA form would be 2-7 % faster per layer,
        # M = 3, 4 not measured -- the switch point is left here, for every format, until they are.
        gemv = getattr(hip, ("gemv" if hip.gemv_fits(M, K) else "gemm_skinny") + fmt.suffix)
        if W is not None:
            gemv(x, *W, out, ldo, out_bs, rpb, residual, **pre)
        else:                                                                # parameters not laid out back to back (no FlatUnit): one launch each
            off = 0
            for w in weights:
                gemv(x, w, out, ldo, out_bs, rpb, None if residual is None else residual[:, off:], out_col=off, **pre)
                off += w.shape[0]
        return out

    def _gate_up_act(self, xn2, gu_w):
        """silu(xn2 @ Wg^T) * (xn2 @ Wu^T) -> act [M, I] of the "once" pass: the gate|up projection with the SwiGLU epilogue where gate|up
        is one matrix (a coded weight, or bf16 views adjacent in memory) -- the packed rows never reach memory --, otherwise one plain
        launch per matrix into a gate|up buffer and the stand-alone swiglu_fwd. The same bits either way."""
        fmt, W = _operands(gu_w)
        if W is not None:
            return getattr(hip, "gemm_skinny_gateup_swiglu" + fmt.suffix)(xn2, *W)
        return hip.swiglu_fwd(self._gemv(xn2, gu_w))

    def _suffix_pass_once(self):
        """suffix_operand "once" over more than 8 rows: seven launches per layer. Each RMSNorm operand is formed once per pass by the
        stand-alone kernel (the values the fused form re-forms per workgroup), every projection runs on the plain skinny form, and SwiGLU
        sits in the gate|up projection's epilogue: bit for bit the "fused" pass."""
        B, R, H, S_p, S_cap = self.B, self.R, self.H, self.S_p, self.S_cap
        h = self.h_in
        scale = 1.0 / math.sqrt(self.D)
        attn = self._suffix_attn()
        for (ln1, qkv, wo, ln2, gu_w, wd), c in self._suffix_layers():
            fused = self.D == 128 and _operands(qkv)[1] is not None          # the rotary epilogue, as in _suffix_pass
            xn, _ = hip.rmsnorm_fwd(h, ln1, self.eps)
            self._gemv(xn, qkv, out=c[:, S_p:], rpb=R, out_bs=c.stride(0), **({"rope": (self.cos_s, self.sin_s, 2 * H)} if fused else {}))
            if not fused:
                for b in range(B):
                    hip.rope_inplace(c[b, S_p:], self.cos_s, self.sin_s, R, self.nheads, self.D, 0, H)
            o = attn(c, B, self.nheads, self.D, S_cap, R, scale)
            h1 = self._gemv(o, wo, residual=h)
            xn2, _ = hip.rmsnorm_fwd(h1, ln2, self.eps)
            h = self._gemv(self._gate_up_act(xn2, gu_w), wd, residual=h1)
        self._finish(h)

    def _suffix_pass(self):
        """Five launches per layer, whatever the suffix pass streams (bf16 views or the FP8 copy: activations / cache / attention are the
        same). suffix_operand "once" with more than 8 rows: _suffix_pass_once's seven; up to 8 rows the GEMV stages its input once per
        workgroup already, and the pass is this one in both modes."""
        B, R, H, S_p, S_cap = self.B, self.R, self.H, self.S_p, self.S_cap
        if self.suffix_operand == "once" and B * R > hip.GEMV_MMAX:
            return self._suffix_pass_once()
        h = self.h_in
        scale = 1.0 / math.sqrt(self.D)
        attn = self._suffix_attn()                                             # "head": R x S_kv scores in LDS vs online softmax
        for (ln1, qkv, wo, ln2, gu_w, wd), c in self._suffix_layers():
            # north_star's "fused RMSNorm + RoPE + QKV" as ONE kernel: RMSNorm inside the projection's input staging, the rotary embedding of
            # the q and k columns in its epilogue; the rows go straight into the cache slots [S_p, S_p + R) of every sample
            fused = self.D == 128 and _operands(qkv)[1] is not None
            self._gemv(h, qkv, out=c[:, S_p:], rpb=R, out_bs=c.stride(0), norm_weight=ln1, eps=self.eps,
                       **({"rope": (self.cos_s, self.sin_s, 2 * H)} if fused else {}))
            if not fused:
                for b in range(B):
                    hip.rope_inplace(c[b, S_p:], self.cos_s, self.sin_s, R, self.nheads, self.D, 0, H)
            o = attn(c, B, self.nheads, self.D, S_cap, R, scale)
            h1 = self._gemv(o, wo, residual=h)
            gu = self._gemv(h1, gu_w, norm_weight=ln2, eps=self.eps)
            h = self._gemv(gu, wd, residual=h1, swiglu=True)                   # SwiGLU inside the down projection's input staging
        self._finish(h)


# ================================================================================================ the row-GEMM engines
# More than one chunk per pass: B observations with prompts of different lengths (MLA.predict_action_diff_batch; the reference's
# `predict_action_batch`, models/mla/model_mla.py:994, names the use case -- "batch inference in the simulators" -- but reads an attribute
# MLA never defines), N draws for one observation (predict_action_diff_samples), or both. A pass streams the decoder weights once whatever
# the row count, so the chunks of a pass cost one prefill plus 8 weight passes instead of one prefill and 8 passes each.
class SubBatchPlan(NamedTuple):
    """One cached-prefix pass of `plan_batch`: samples [start, stop) of the call. Per sample b: ids[b] the final prompt ids, k[b] the splice
    position (the last tag), S_p[b] prefix rows ([BOS | front tokens | text[1:k] | proprio]), slot[b] = S_p[b] the first cache row of its
    suffix rows, kv_len[b] = S_p[b] + R the keys its last suffix row sees. S_pmax: rows every prefix is right-padded to for the prefill;
    S_cap: rows per sample of the cache (S_pmax + R rounded up to the bucket), part of the engine's key."""
    start: int
    stop: int
    ids: Tuple[Tuple[int, ...], ...]
    k: Tuple[int, ...]
    S_p: Tuple[int, ...]
    slot: Tuple[int, ...]
    kv_len: Tuple[int, ...]
    S_pmax: int
    S_cap: int
    R: int


def plan_batch(ids_rows: Sequence[Sequence[int]], n_action_rows: int, n_front: int, max_rows: int = 256, bucket: int = 64,
               add_tail: bool = True):
    """Pure host planning of a batched sampling call -> list of SubBatchPlan, in order.
    ids_rows: one id sequence per sample (different lengths). add_tail: predict_action_diff's prompt handling per row -- a row that does
    not end with the tag gets PROMPT_TAIL appended and the last three ids dropped again. A row without the tag raises IndexError (as the
    splice of prismatic.py:983 would). n_front: fused tokens between BOS and the text (513 at 7B). R = 1 + n_action_rows suffix rows per
    sample; consecutive samples are grouped into passes of at most max_rows suffix rows."""
    R = 1 + int(n_action_rows)
    if R > max_rows:
        raise ValueError(f"{R} suffix rows per sample exceed the {max_rows} rows of a pass")
    if len(ids_rows) == 0:
        raise ValueError("plan_batch: no samples")
    rows, ks = [], []
    for b, row in enumerate(ids_rows):
        row = [int(t) for t in row]
        if add_tail and (len(row) == 0 or row[-1] != SPLICE_TAG):
            row = (row + list(PROMPT_TAIL))[:-3]
        if SPLICE_TAG not in row:
            raise IndexError(f"input_ids row {b} without the splice tag {SPLICE_TAG} (models/vlm/prismatic.py:983)")
        k = len(row) - 1 - row[::-1].index(SPLICE_TAG)                    # last occurrence
        if k < 1:
            raise IndexError(f"input_ids row {b}: the splice tag {SPLICE_TAG} must not be the first id")
        rows.append(tuple(row))
        ks.append(k)
    per = max_rows // R
    plans = []
    for start in range(0, len(rows), per):
        stop = min(start + per, len(rows))
        k = tuple(ks[start:stop])
        S_p = tuple(1 + n_front + (kk - 1) + 1 for kk in k)
        S_pmax = max(S_p)
        S_cap = -(-(S_pmax + R) // bucket) * bucket
        plans.append(SubBatchPlan(start, stop, tuple(rows[start:stop]), k, S_p, S_p, tuple(v + R for v in S_p), S_pmax, S_cap, R))
    return plans


class _RowGemmEps(_CachedEpsBase):
    """What BatchedPrefixCachedEps, SampleGroupsEps and BatchedSampleGroupsEps share: the suffix pass over up to 256 rows. RMSNorm / SwiGLU
    are formed once per projection by the stand-alone kernels (the values the fused forms produce), then the plain weight-streaming GEMM
    (mla_gemm_suffix_bf16, or mla_gemm_suffix_w8 over the model's FP8 copy) runs over all M suffix rows of the pass. Per layer, c = the
    layer's cache:
        rmsnorm_fwd -> q|k|v into the cache, q and k rotated in the epilogue -> attention -> o + residual -> rmsnorm_fwd -> gate|up ->
        swiglu_fwd -> down + residual
    An engine says where the q|k|v rows land (_cache_write) and which attention reads them (_attention); everything else is the same.
    The two engines with ragged prompts also share the prefill: right-padded prefixes, one varlen pass per layer (_varlen_prefill)."""

    MAX_ROWS = 256                   # suffix rows per pass (mla_gemm_suffix_bf16 / _w8 and their `_pos` forms); more are served as consecutive passes
    MAX_R = 64                       # rows per sample / group (mla_attn_chunk_ragged, mla_attn_chunk_groups, mla_attn_chunk_ragged_groups)
    BUCKET = 64                      # cache capacity granularity in rows (the engines with ragged prompts)
    batch_prefill = "train"          # MODES: how _varlen_prefill runs the prefix rows (the two engines with ragged prompts)

    def _batch_prefill_buffers(self, NB: int, G: int, dev):
        """batch_prefill "fp8" / "fp8_as_bf16": the compact prefill's buffers at the engine's capacity, allocated once (call outside
        inference mode). An engine serves every S_pmax of its capacity bucket: S_cap - G R - BUCKET < S_pmax <= S_cap - G R."""
        if self.batch_prefill == "train":
            return
        hi = self.S_cap - G * self.R
        lengths = range(max(1, hi - self.BUCKET + 1), hi + 1)
        if self.batch_prefill == "fp8":
            self._compact_buffers([NB * S for S in lengths], dev, "fp8")
        else:                                                                # the yardstick runs one sample at a time
            self._compact_buffers(list(lengths), dev, "fp8_as_bf16")

    def _check_batch_prefill(self, NB: int, S_pmax: int):
        """What the batch prefill serves: "fp8" up to 65 536 rows per sub-batch (the wide-row GEMMs), "fp8_as_bf16" up to 1024 prefix rows
        per sample (the compact bf16 GEMMs); anything else is an error, never a silent "train" prefill."""
        if self.batch_prefill == "fp8" and NB * S_pmax > hip.PREFILL_WIDE_MMAX:
            raise ValueError(f"batch_prefill=\"fp8\" serves at most {hip.PREFILL_WIDE_MMAX} prefill rows per sub-batch (got {NB} x {S_pmax} = "
                             f"{NB * S_pmax}); use batch_prefill=\"train\" or fewer observations per call")
        if self.batch_prefill == "fp8_as_bf16" and S_pmax > hip.PREFILL_MMAX:
            raise ValueError(f"batch_prefill=\"fp8_as_bf16\" serves at most {hip.PREFILL_MMAX} prefix rows per sample (got {S_pmax}); use "
                             "batch_prefill=\"train\"")

    def _batch_compact_prefill(self, prefix, NB: int, S_pmax: int, rope):
        """batch_prefill "fp8": every layer ONCE over the NB * S_pmax right-padded prefix rows (_compact_layer with B = NB: the q|k|v
        epilogue writes sample b's rows at cache offset b * cache.stride(0)), on the wide-row GEMMs beyond 1024 rows. No ragged
        addressing is needed: attention is causal and the padding is on the right, so a valid row never sees a pad row. A pad row
        starts as zeros -- the quantiser gives it scale 1 and codes 0 -- and stays finite through every layer; pad rows land in cache
        rows [S_p[b], S_pmax) that no suffix row reads before the suffix pass has overwritten them, exactly as the "train" prefill's
        c[:, :S_pmax].copy_. "fp8_as_bf16": the same layers per sample (B = 1, at most 1024 rows) on the dequantised weight codes and
        the quantised-and-dequantised inputs."""
        self._weights()
        layers = self._weight_copy(W8, self.batch_prefill)
        if self.batch_prefill == "fp8":
            h = prefix.reshape(NB * S_pmax, self.H)
            for w, c in zip(layers, self.cache):
                h = self._compact_layer(w, h, NB, S_pmax, c, c.stride(0), "fp8", rope)
            return
        for b in range(NB):
            h = prefix[b]
            for w, c in zip(layers, self.cache):
                h = self._compact_layer(w, h, 1, S_pmax, c[b], 0, "fp8_as_bf16", rope)

    def _cache_write(self, c):
        """-> (ldo, out_batch_stride, keywords) of the q|k|v projection into the layer's cache c (rows_per_batch is R)."""
        raise NotImplementedError

    def _attention(self, c, scale):
        raise NotImplementedError

    def _split_workspace(self, B: int, G: int, S_p_or_cap: int, ragged: bool, dev):
        """suffix_attention "split": the workspace of mla_attn_groups_split at the engine's capacity (B samples of G groups; S_p of the
        one prefix, or S_cap with the lengths in device memory), allocated once beside h_in / h_out (call outside inference mode), and
        attn_plan = (S_max, the library's plan there). Shorter prefixes need no more (the split count is fixed on the host), so one captured
        graph serves every length mix of a bucket. Fewer groups on one prefix (set_groups) may: the plan cuts a smaller launch into more
        ranges, so that form takes the largest need over 1 .. G groups."""
        if self.suffix_attention != "split":
            return
        self.attn_plan = hip.attn_groups_split_plan(B, G, self.nheads, self.R, S_p_or_cap, ragged)
        S_max = self.attn_plan[0]
        need = max(hip.attn_split_ws_bytes(B * g, self.nheads, self.R, S_max) for g in (range(1, G + 1) if not ragged else (G,)))
        if need < 0:
            raise RuntimeError(f"mla_attn_chunk_split_ws_bytes: {hip.lib().mla_last_error().decode()}")
        self._attn_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def _proj(self, x, weights, out=None, residual=None):
        """x [M, K] @ W^T (+ residual): `weights` is a tuple of adjacent bf16 views or one coded weight (mla_gemm_suffix_<format>); out =
        a layer's cache: the q|k|v rows go to their samples' / groups' slots."""
        fmt, W = _operands(weights)
        assert W is not None, "the packed weights are adjacent in memory (_weights)"
        M, N, gemm = x.shape[0], W[0].shape[0], functools.partial(getattr(hip, "gemm_suffix" + fmt.suffix), x, *W)
        if out is None:
            out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
            gemm(out, out.stride(0), 0, M, residual)
        else:
            ldo, out_bs, kw = self._cache_write(out)
            gemm(out, ldo, out_bs, self.R, residual, **kw)
        return out

    def _suffix_pass(self):
        h = self.h_in
        scale = 1.0 / math.sqrt(self.D)
        for (ln1, qkv, wo, ln2, gu_w, wd), c in self._suffix_layers():
            xn, _ = hip.rmsnorm_fwd(h, ln1, self.eps)
            self._proj(xn, qkv, out=c)
            o = self._attention(c, scale)
            h1 = self._proj(o, wo, residual=h)
            xn2, _ = hip.rmsnorm_fwd(h1, ln2, self.eps)
            gu = self._proj(xn2, gu_w)
            h = self._proj(hip.swiglu_fwd(gu), wd, residual=h1)
        self._finish(h)

    @staticmethod
    def _front_tokens(vlm, images, point_cloud, camera_name):
        """The encoders once over all observations of a call -> [B, n_front, H], the fused tokens between BOS and the text."""
        with torch.no_grad():
            parts, _, _, _, _, _ = vlm.get_fused_tokens(images, point_cloud, None, None, camera_name)
            vlm.vision_tower_2d.assert_masks_ok()
            return torch.cat(parts, dim=1)

    def _varlen_prefill(self, sub, front, proprio, G, index):
        """The prefill of observations [sub.start, sub.stop) with G groups of suffix rows each: the prefixes right-padded to S_pmax, one
        varlen pass per layer on the training kernels (ops.DecoderLayerFn._fwd with seqlens; the bf16 weights, whatever the suffix pass
        streams), the rows copied into the [NB, S_cap, 3H] cache -- or, batch_prefill "fp8" / "fp8_as_bf16", _batch_compact_prefill. index: {attribute: values} of the int32 device tensors the suffix
        pass's kernels read, allocated on the first call and refreshed by copy_ (a captured graph keeps their addresses)."""
        vlm, bf16, dev = self.vlm, torch.bfloat16, front.device
        NB, S_pmax = sub.stop - sub.start, sub.S_pmax
        self._check_batch_prefill(NB, S_pmax)
        with torch.no_grad():
            proprio_e = vlm.proprio_embedder(proprio.to(bf16))                # [NB, 1, H]
            H = front.shape[2]
            prefix = torch.zeros((NB, S_pmax, H), dtype=bf16, device=dev)
            for b in range(NB):
                e = vlm.llm_backbone.embed_input_ids(torch.tensor([sub.ids[b]], dtype=torch.long, device=dev))[0]
                prefix[b, :sub.S_p[b]] = torch.cat([e[:1], front[b], e[1:sub.k[b]], proprio_e[b]], dim=0)
            if self.cache is None:
                self.NB, self.G, self.B, self.H, self.S_cap = NB, G, NB * G, H, sub.S_cap        # B = NB * G is the sampler's batch
                self.D = H // self.nheads
                self.rot = self.model.layers[0].self_attn.rotary_emb
                self.cos_c, self.sin_c = self.rot.tables(self.S_cap, dev)    # the epilogue rotates a suffix row with the table row of its position
                rows = NB * G * self.R
                with torch.inference_mode(False):                            # the engine outlives the (inference-mode) call that creates it
                    self.cache = [torch.zeros((NB, self.S_cap, 3 * H), dtype=bf16, device=dev) for _ in self.model.layers]
                    self.h_in = torch.zeros((rows, H), dtype=bf16, device=dev)
                    self.h_out = torch.zeros((rows, H), dtype=bf16, device=dev)
                    for name, values in index.items():
                        setattr(self, name, torch.zeros(len(values), dtype=torch.int32, device=dev))
                    self._split_workspace(NB, G, self.S_cap, True, dev)
                    self._batch_prefill_buffers(NB, G, dev)
            assert (NB, G, H, sub.S_cap, sub.R) == (self.NB, self.G, self.H, self.S_cap, self.R) and S_pmax + G * self.R <= self.S_cap
            for name, values in index.items():
                getattr(self, name).copy_(torch.tensor(values, dtype=torch.int32))
            seqlens = torch.tensor(sub.S_p, dtype=torch.int32, device=dev)
            cos_p, sin_p = self.rot.tables(S_pmax, dev)
            if self.batch_prefill != "train":
                self._batch_compact_prefill(prefix, NB, S_pmax, (cos_p, sin_p))
                return
            h = prefix.reshape(NB * S_pmax, H)
            for w, c in zip(self._weights(), self.cache):
                h, acts = ops.DecoderLayerFn._fwd(h, seqlens, cos_p, sin_p, NB, S_pmax, self.nheads, self.eps, w)
                c[:, :S_pmax].copy_(acts.qkv[:NB * S_pmax].view(NB, S_pmax, 3 * H))
                del acts


class BatchedPrefixCachedEps(_RowGemmEps):
    """PrefixCachedEps for B samples whose splice tags sit at different positions (bf16 suffix weights only; the prefill per batch_prefill). The cache is [B, S_cap, 3H] and the
    suffix rows of sample b live at rows S_p[b] .. S_p[b] + R (rows behind them are never read). `slot` and `kv_len` are device tensors
    the kernels read (mla_gemm_suffix_bf16, mla_attn_chunk_ragged), refreshed by copy_ in prefill(): one engine -- and one captured graph
    -- per (B, S_cap, R, device) serves every mix of prompt lengths in that capacity bucket."""

    @classmethod
    def supports_batch(cls, vlm, n_action_rows: int, warn: bool = True) -> bool:
        """head_dim 128 and at most 64 suffix rows per sample; otherwise the caller loops over whole-forward batch-1 calls (warns once;
        warn=False: the plain predicate, for the callers that raise instead)."""
        return cls._serves(vlm, 1 + n_action_rows, cls.MAX_R, ("batch",), "BatchedPrefixCachedEps: {rows} suffix rows per sample (max {limit}) "
                           "/ head_dim {D} (needs 128) are beyond the batched cached-prefix kernels; sampling every observation with a whole "
                           "forward per step", warn)

    @classmethod
    def for_batch(cls, vlm, ids_rows, n_action_rows: int, images=None, point_cloud=None, camera_name=None, proprio=None, add_tail=True,
                  suffix_attention: str = "head", batch_prefill: str = "train", **unused):
        """Generator over the passes of one call: runs the encoders once over all samples, plans (plan_batch: ids_rows are the prompts as
        the caller has them, the prompt tail is handled there) and yields
        (SubBatchPlan, prefilled engine) per sub-batch. Two sub-batches may share an engine: finish sampling one before taking the next.
        suffix_attention: "head" (mla_attn_chunk_ragged) or "split" (mla_attn_groups_split, one group per sample); batch_prefill:
        MODES' batch_prefill; one engine per mode."""
        modes = engine_modes(groups_attention=suffix_attention, batch_prefill=batch_prefill)
        front = cls._front_tokens(vlm, images, point_cloud, camera_name)
        for sub in plan_batch(ids_rows, n_action_rows, int(front.shape[1]), cls.MAX_ROWS, cls.BUCKET, add_tail=add_tail):
            eng = cls._engine(vlm, "_prefix_engines_batched", (sub.stop - sub.start, sub.S_cap, sub.R, str(front.device)),
                              (n_action_rows, modes), **modes._asdict())
            eng.prefill(sub, front[sub.start:sub.stop], proprio[sub.start:sub.stop])
            yield sub, eng

    def prefill(self, sub: SubBatchPlan, front, proprio):
        index = {"slot": sub.slot, "kv_len": sub.kv_len}
        if self.suffix_attention == "split":                                  # the groups form counts a sample's prefix rows
            index["prefix_len"] = tuple(n - sub.R for n in sub.kv_len)
        self._varlen_prefill(sub, front, proprio, 1, index)

    def _cache_write(self, c):
        # q|k|v rows of sample b -> cache rows slot[b] .. slot[b] + R, q and k rotated at those positions
        return c.stride(-2), c.stride(0), {"slot": self.slot, "cap_rows": self.S_cap, "rope": (self.cos_c, self.sin_c, 2 * self.H)}

    def _attention(self, c, scale):
        if self.suffix_attention == "split":
            return hip.attn_groups_split(c, self.B, 1, self.nheads, self.D, self.prefix_len, self.R, scale, ws=self._attn_ws)
        return hip.attn_chunk_ragged(c, self.B, self.nheads, self.D, self.kv_len, self.R, scale)


# ================================================================================================ N action chunks for one observation
# MLA.predict_action_diff_samples: N independent draws for ONE observation. Everything in front of the [t, x] tokens is the same in all
# of them, so the encoders and the prefill run once (batch 1, S_p rows) and the cache holds ONE prefix followed by G groups of R suffix
# rows: [S_p + G R, 3H] per layer. The projection writes group g's rows at S_p + g R + p (the kernel's "samples" overlapping: batch
# stride R rows, every slot S_p) and mla_attn_chunk_groups is the attention. The prefill stays on the bf16 weights in every mode.
def plan_sample_groups(num_samples: int, R: int, max_rows: int = 256):
    """Pure host planning: the passes [(start, stop), ...] that serve samples [0, num_samples) in order, at most max_rows // R groups
    (R suffix rows each) per pass."""
    num_samples, R, max_rows = int(num_samples), int(R), int(max_rows)
    if num_samples < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    if R < 1 or R > max_rows:
        raise ValueError(f"{R} suffix rows per sample do not fit the {max_rows} rows of a pass")
    per = max_rows // R
    return [(start, min(start + per, num_samples)) for start in range(0, num_samples, per)]


class SampleGroupsEps(_RowGemmEps):
    """One engine per (splice position, action rows, group capacity, device): ONE cache per layer with the prefix rows and room for
    `capacity` groups, prefilled once per call; `set_groups(G)` selects how many groups the next `model(x [G, T, D], t [G])` calls serve
    (G <= capacity: the sub-batches of a call whose N exceeds a pass share the cache and the prefill) and one captured graph is kept per
    distinct G. Rows of groups >= G are neither written nor read by a pass of G groups."""

    @classmethod
    def supports_samples(cls, vlm, n_action_rows: int, warn: bool = True) -> bool:
        """head_dim 128 and at most 64 suffix rows per sample; otherwise the bf16 caller loops over batch-1 calls (warns once per shape;
        warn=False: the plain predicate, for the callers that raise instead)."""
        return cls._serves(vlm, 1 + n_action_rows, cls.MAX_R, ("samples",), "SampleGroupsEps: {rows} suffix rows per sample (max {limit}) / "
                           "head_dim {D} (needs 128) are beyond the shared-prefix kernels; drawing every sample with its own "
                           "predict_action_diff call", warn)

    @classmethod
    def for_inputs(cls, vlm, input_ids, n_action_rows: int, num_samples: int, suffix_weights: str = "bf16", prefill: str = "train",
                   prefill_precision: str = "bf16", suffix_attention: str = "head", suffix_mx: str = "off", **model_kwargs):
        """-> (engine, prefilled for this observation; passes [(start, stop), ...] of plan_sample_groups). One engine -- and its graphs --
        per suffix_weights, prefill and attention mode, as in PrefixCachedEps.for_inputs. suffix_attention: "head"
        (mla_attn_chunk_groups) or "split" (mla_attn_groups_split)."""
        modes = engine_modes(suffix_weights=suffix_weights, suffix_mx=suffix_mx, prefill=prefill, prefill_precision=prefill_precision,
                             groups_attention=suffix_attention)
        k = PrefixCachedEps._splice_position(input_ids)
        passes = plan_sample_groups(num_samples, 1 + n_action_rows, cls.MAX_ROWS)
        capacity = max(stop - start for start, stop in passes)
        eng = cls._engine(vlm, "_prefix_engines_samples", (k, int(n_action_rows), capacity, str(input_ids.device)),
                          (n_action_rows, capacity, modes), **modes._asdict())
        eng.prefill(input_ids, k, **model_kwargs)
        return eng, passes

    def __init__(self, vlm, n_action_rows: int, capacity: int, modes: Modes = Modes()):
        super().__init__(vlm, n_action_rows, modes)
        self.capacity = int(capacity)
        self._graphs = {}            # G -> captured pass over G groups
        self._graphs_packed = None   # the weights those graphs hold the addresses of

    def set_groups(self, G: int):
        assert 1 <= G <= self.capacity and self.cache is not None
        self.B = G
        self.h_in, self.h_out = self._h_in[:G * self.R], self._h_out[:G * self.R]
        self.graph = self._graphs.get(G)

    def prefill(self, input_ids, k, images=None, point_cloud=None, camera_name=None, proprio=None, tactile=None, gripper_xyz=None, **unused):
        bf16, dev = torch.bfloat16, input_ids.device
        assert input_ids.shape[0] == 1, "one observation"
        with torch.no_grad():
            prefix = self._prefix_rows(input_ids, k, images, point_cloud, camera_name, proprio, tactile, gripper_xyz)
            _, S_p, H = prefix.shape
            self._check_compact(S_p)
            if self.cache is None:
                self.S_p, self.H = S_p, H
                self.D = H // self.nheads
                rot = self.model.layers[0].self_attn.rotary_emb
                self.cos_p, self.sin_p = rot.tables(S_p, dev)
                self.cos_c, self.sin_c = rot.tables(S_p + self.R, dev)        # the epilogue rotates row S_p + p of a group with table row S_p + p
                rows = self.capacity * self.R
                with torch.inference_mode(False):                            # the engine outlives the (inference-mode) call that creates it
                    self.cache = [torch.zeros((S_p + rows, 3 * H), dtype=bf16, device=dev) for _ in self.model.layers]
                    self._h_in = torch.zeros((rows, H), dtype=bf16, device=dev)
                    self._h_out = torch.zeros((rows, H), dtype=bf16, device=dev)
                    self.slot = torch.full((self.capacity,), S_p, dtype=torch.int32, device=dev)
                    if self.prefill_mode == "compact":
                        self._compact_buffers(S_p, dev)
                    self._split_workspace(1, self.capacity, S_p, False, dev)
                self.set_groups(self.capacity)
            assert (S_p, H) == (self.S_p, self.H)
            weights = self._weights()
            if self._graphs_packed is not self._suffix:                      # new weights: every captured pass holds stale addresses
                self._graphs.clear()
                self._graphs_packed = self._suffix
                self.graph = None
            self._prefill_rows(prefix.reshape(S_p, H), 1, S_p, 0, weights)

    def _run(self):
        super()._run()
        if self.graph is not None:
            self._graphs[self.B] = self.graph

    def _cache_write(self, c):
        # group g = "sample" g of the kernel: base row g R, slot S_p; q|k|v row p of group g -> cache row S_p + g R + p, rotated at S_p + p
        return c.stride(0), self.R * c.stride(0), {"slot": self.slot, "cap_rows": self.S_p + self.R, "rope": (self.cos_c, self.sin_c, 2 * self.H)}

    def _attention(self, c, scale):
        if self.suffix_attention == "split":
            return hip.attn_groups_split(c, 1, self.B, self.nheads, self.D, self.S_p, self.R, scale, ws=self._attn_ws)
        return hip.attn_chunk_groups(c, self.B, self.nheads, self.D, self.S_p, self.R, scale)


# ================================================================================================ N action chunks for each of B observations
# MLA.predict_action_diff_batch(num_samples=N): the two engines above composed. The encoders and ONE varlen prefill serve the B prefixes of
# a pass (BatchedPrefixCachedEps), every sample's cache holds its prefix followed by G = N groups of R suffix rows (SampleGroupsEps): the
# cache is [B, S_cap, 3H], row S_p[b] + g R + p of sample b is suffix row p of group g. With several groups behind a per-sample prefix the
# cache row and the rotary position of a suffix row differ (row S_p[b] + g R + p rotates at S_p[b] + p), hence mla_gemm_suffix_bf16_pos /
# _w8_pos with two device arrays, and mla_attn_chunk_ragged_groups as the attention. A pass streams the decoder weights once over the
# B G R <= 256 rows: B N chunks cost one prefill pass per sub-batch and 8 weight passes, not B prefills and 8 B passes.
class SampleSubBatchPlan(NamedTuple):
    """One pass of `plan_batch_samples`: observations [start, stop) of the call with G groups each. ids / k / S_p / S_pmax / R as in
    SubBatchPlan; prefix_len[b] = S_p[b]; per group s = b * G + g (b counted inside the pass): slot[s] = b * S_cap + S_p[b] + g * R its
    first row in the flat [B * S_cap, 3H] cache, rope_pos[s] = S_p[b] its first rotary position; S_cap = S_pmax + G * R rounded up to the
    bucket, part of the engine's key."""
    start: int
    stop: int
    ids: Tuple[Tuple[int, ...], ...]
    k: Tuple[int, ...]
    S_p: Tuple[int, ...]
    prefix_len: Tuple[int, ...]
    slot: Tuple[int, ...]
    rope_pos: Tuple[int, ...]
    S_pmax: int
    S_cap: int
    R: int
    G: int


def plan_batch_samples(ids_rows: Sequence[Sequence[int]], n_action_rows: int, n_front: int, num_samples: int, max_rows: int = 256,
                       bucket: int = 64, add_tail: bool = True):
    """Pure host planning of predict_action_diff_batch(num_samples=N) -> list of SampleSubBatchPlan, in order, or None when one
    observation's N groups exceed a pass (N > max_rows // R: the caller then loops predict_action_diff_samples per observation, which
    splits its passes on one prefill). Prompt handling, splice position and errors per row are plan_batch's; a pass holds
    (max_rows // R) // N consecutive observations with all N groups each."""
    N, R = int(num_samples), 1 + int(n_action_rows)
    if N < 1:
        raise ValueError(f"num_samples must be >= 1, got {num_samples}")
    if R > max_rows:
        raise ValueError(f"{R} suffix rows per sample exceed the {max_rows} rows of a pass")
    per = max_rows // R
    if N > per:
        plan_batch(ids_rows, n_action_rows, n_front, max_rows, bucket, add_tail)      # the rows' errors do not depend on N
        return None
    plans = []
    for sub in plan_batch(ids_rows, n_action_rows, n_front, (per // N) * R, bucket, add_tail):
        S_cap = -(-(sub.S_pmax + N * R) // bucket) * bucket
        slot = tuple(b * S_cap + s + g * R for b, s in enumerate(sub.S_p) for g in range(N))
        rope_pos = tuple(s for s in sub.S_p for _ in range(N))
        plans.append(SampleSubBatchPlan(sub.start, sub.stop, sub.ids, sub.k, sub.S_p, sub.S_p, slot, rope_pos, sub.S_pmax, S_cap, R, N))
    return plans


class BatchedSampleGroupsEps(_RowGemmEps):
    """One engine -- and one captured graph -- per (observations NB, groups G, S_cap, R, device[, suffix_weights]) serves every mix of
    prompt lengths of a capacity bucket: `prefix_len` [NB], `slot` and `rope_pos` [NB * G] are device tensors the kernels read
    (mla_attn_chunk_ragged_groups, mla_gemm_suffix_bf16_pos / mla_gemm_suffix_w8_pos), refreshed by copy_ in prefill(). The suffix pass
    runs over the NB * G * R rows in the order (b, g, p). `model(x [NB * G, T, D], t [NB * G])`: self.B = NB * G is the sampler's batch."""

    @classmethod
    def supports_batch_samples(cls, vlm, n_action_rows: int, warn: bool = True) -> bool:
        """head_dim 128 and at most 64 suffix rows per group; otherwise the bf16 caller loops predict_action_diff_samples per observation
        (warns once per shape; warn=False: the plain predicate, for the callers that raise instead)."""
        return cls._serves(vlm, 1 + n_action_rows, cls.MAX_R, ("batch_samples",), "BatchedSampleGroupsEps: {rows} suffix rows per sample (max "
                           "{limit}) / head_dim {D} (needs 128) are beyond the batched shared-prefix kernels; drawing every observation's "
                           "samples with its own call", warn)

    @classmethod
    def fits_pass(cls, n_action_rows: int, num_samples: int) -> bool:
        """Whether one observation's N groups fit a pass (plan_batch_samples would not return None)."""
        return int(num_samples) <= cls.MAX_ROWS // (1 + int(n_action_rows))

    @classmethod
    def for_batch(cls, vlm, ids_rows, n_action_rows: int, num_samples: int, suffix_weights: str = "bf16", images=None, point_cloud=None,
                  camera_name=None, proprio=None, add_tail=True, suffix_attention: str = "head", batch_prefill: str = "train",
                  suffix_mx: str = "off", **unused):
        """Generator over the passes of one call: runs the encoders once over all observations, plans (plan_batch_samples) and yields
        (SampleSubBatchPlan, prefilled engine) per sub-batch. Two sub-batches may share an engine: finish sampling one before taking the
        next. suffix_attention: "head" (mla_attn_chunk_ragged_groups) or "split" (mla_attn_groups_split); batch_prefill:
        MODES' batch_prefill; one engine per mode."""
        modes = engine_modes(suffix_weights=suffix_weights, suffix_mx=suffix_mx, groups_attention=suffix_attention, batch_prefill=batch_prefill)
        front = cls._front_tokens(vlm, images, point_cloud, camera_name)
        plans = plan_batch_samples(ids_rows, n_action_rows, int(front.shape[1]), num_samples, cls.MAX_ROWS, cls.BUCKET, add_tail=add_tail)
        if plans is None:
            raise ValueError(f"{num_samples} groups of {1 + n_action_rows} rows exceed the {cls.MAX_ROWS} rows of a pass (fits_pass)")
        for sub in plans:
            eng = cls._engine(vlm, "_prefix_engines_batch_samples", (sub.stop - sub.start, sub.G, sub.S_cap, sub.R, str(front.device)),
                              (n_action_rows, modes), **modes._asdict())
            eng.prefill(sub, front[sub.start:sub.stop], proprio[sub.start:sub.stop])
            yield sub, eng

    def prefill(self, sub: SampleSubBatchPlan, front, proprio):
        self._varlen_prefill(sub, front, proprio, sub.G, {"prefix_len": sub.prefix_len, "slot": sub.slot, "rope_pos": sub.rope_pos})

    def _cache_write(self, c):
        # flat [NB * S_cap, 3H] cache: q|k|v row p of group (b, g) -> row slot = b S_cap + S_p[b] + g R + p, rotated at position S_p[b] + p
        return c.stride(-2), 0, {"slot": self.slot, "cap_rows": self.NB * self.S_cap, "rope": (self.cos_c, self.sin_c, 2 * self.H),
                                 "rope_pos": self.rope_pos, "rope_rows": self.S_cap}

    def _attention(self, c, scale):
        if self.suffix_attention == "split":
            return hip.attn_groups_split(c, self.NB, self.G, self.nheads, self.D, self.prefix_len, self.R, scale, ws=self._attn_ws)
        return hip.attn_chunk_ragged_groups(c, self.NB, self.G, self.nheads, self.D, self.prefix_len, self.R, scale)
