"""suffix_operand="once" of the batch-1 cached-prefix engine, as recorded launch lists (CPU, no library), in the recorder style of
test_infer_suffix_plan_host.py: a fake PrefixCachedEps, the mla_amd.hip wrappers replaced by recorders. The expected lists are written
from the mode's contract, not from the code:

  per layer, "once" over more than 8 suffix rows (M = B R, c = the layer's cache) -- seven launches
    xn  = rmsnorm_fwd(h, ln1)
    q|k|v: plain skinny(xn, qkv) into cache rows [S_p, S_p + R), RoPE epilogue
    attention
    h1  = plain skinny(o, wo, residual=h)
    xn2 = rmsnorm_fwd(h1, ln2)
    act = gemm_skinny_gateup_swiglu(xn2, gate|up)              [M, I]; the packed gate|up rows do not exist
    h   = plain skinny(act, wd, residual=h1)
  up to 8 rows: the "fused" pass, launch for launch
  gate|up not adjacent in memory (bf16): one plain launch per matrix into a [M, 2 I] buffer, swiglu_fwd, plain down (and q|k|v one launch
  per matrix + rope_inplace, as in the "fused" pass)"""
import math
import types

import pytest
import torch

from mla_amd import hip, infer
from test_infer_suffix_plan_host import (BF16, D, EPS, H, I, LAYERS, NHEADS, SCALE, SUFFIX, Recorder, _check, _layer_weights, _prefix_engine,
                                         _w, expected_prefix)

R17 = 17


class OperandRecorder(Recorder):
    """The plan test's recorder plus the three wrappers of the gate|up + SwiGLU projection."""

    def __init__(self, monkeypatch, **kw):
        super().__init__(monkeypatch, **kw)
        for name in ("gemm_skinny_gateup_swiglu", "gemm_skinny_gateup_swiglu_w8", "gemm_skinny_gateup_swiglu_w4"):
            monkeypatch.setattr(hip, name, self._wrap(name, getattr(hip, name), self._act))

    @staticmethod
    def _act(i, a):
        return torch.zeros((a["x"].shape[0], a["W"].shape[0] // 2), dtype=BF16)


def _engine17(rec, mode, packed=True, operand="once", attention="head"):
    """A PrefixCachedEps of one sample with 17 suffix rows behind 12 prefix rows. ---- follows the engine's attributes ----"""
    B, S_p = 1, 12
    S_cap = S_p + R17
    e = infer.PrefixCachedEps.__new__(infer.PrefixCachedEps)
    e.suffix_weights, e.suffix_mx = ("bf16", "fp4") if mode == "fp4" else (mode, "off")
    e.suffix_attention, e._attn_ws, e.suffix_operand = attention, None, operand
    e.R, e.T, e.H, e.D, e.nheads, e.eps = R17, R17 - 1, H, D, NHEADS, EPS
    e.model = types.SimpleNamespace(norm=types.SimpleNamespace(weight=rec.know("norm", torch.ones(H, dtype=BF16))))
    e._suffix = e._packed = _layer_weights(rec, mode, packed)
    e.cache = [rec.know(f"cache{l}", torch.zeros((B, S_cap, 3 * H), dtype=BF16)) for l in range(LAYERS)]
    e.h_in, e.h_out = rec.know("h_in", torch.zeros((B * R17, H), dtype=BF16)), torch.zeros((B * R17, H), dtype=BF16)
    e.B, e.S_p, e.S_cap = B, S_p, S_cap
    e.cos_s, e.sin_s = rec.know("cos_s", torch.zeros((R17, D))), rec.know("sin_s", torch.zeros((R17, D)))
    if attention == "split":
        e._attn_ws = rec.know("attn_ws", torch.zeros(64, dtype=torch.uint8))
    return e


def expected_once(mode, packed=True, attention="attn_chunk"):
    """The contract's launch list at B = 1, R = 17, S_p = 12 + the final norm."""
    B, S_p, M = 1, 12, R17
    S_cap = S_p + R17
    kernel = "gemm_skinny" + SUFFIX[mode]
    fresh = lambda out, N: {"out": out, "ldo": N, "out_batch_stride": 0, "rows_per_batch": M}            # noqa: E731
    calls, h = [], "h_in"
    for l in range(LAYERS):
        c, into = f"cache{l}", {"out": f"cache{l}+{S_p * 3 * H}", "ldo": 3 * H, "out_batch_stride": S_cap * 3 * H, "rows_per_batch": R17}
        xn = f"@{len(calls)}.ret[{M}, {H}]"
        calls.append(("rmsnorm_fwd", {"x2d": h, "w": f"L{l}.ln1", "eps": EPS}))
        if packed:
            calls.append((kernel, {"x": xn, **_w(l, "qkv", mode), **into, "rope": ("cos_s", "sin_s", 2 * H)}))
        else:
            calls += [(kernel, {"x": xn, "W": f"L{l}.{n}", **into, **({"out_col": j * H} if j else {})}) for j, n in enumerate("qkv")]
            calls.append(("rope_inplace", {"buf2d": f"{c}+{S_p * 3 * H}", "cos": "cos_s", "sin": "sin_s", "S": R17, "nheads": NHEADS, "D": D,
                                           "q_off": 0, "k_off": H}))
        i = len(calls)
        calls.append((attention, {"cache": c, "B": B, "nheads": NHEADS, "D": D, "S_kv": S_cap, "R": R17, "scale": SCALE,
                                  **({"ws": "attn_ws"} if attention == "attn_chunk_split" else {})}))
        o, h1, xn2 = f"@{i}.ret[{M}, {H}]", f"@{i + 1}.out[{M}, {H}]", f"@{i + 2}.ret[{M}, {H}]"
        calls.append((kernel, {"x": o, **_w(l, "o", mode), **fresh(h1, H), "residual": h}))
        calls.append(("rmsnorm_fwd", {"x2d": h1, "w": f"L{l}.ln2", "eps": EPS}))
        if packed:
            act = f"@{i + 3}.ret[{M}, {I}]"
            calls.append(("gemm_skinny_gateup_swiglu" + SUFFIX[mode], {"x": xn2, **_w(l, "gu", mode)}))
        else:
            gu, act = f"@{i + 3}.out[{M}, {2 * I}]", f"@{i + 5}.ret[{M}, {I}]"
            calls += [(kernel, {"x": xn2, "W": f"L{l}.{n}", **fresh(gu, 2 * I), **({"out_col": j * I} if j else {})}) for j, n in enumerate("gu")]
            calls.append(("swiglu_fwd", {"gu2d": gu}))
        h2 = f"@{len(calls)}.out[{M}, {H}]"
        calls.append((kernel, {"x": act, **_w(l, "d", mode), **fresh(h2, H), "residual": h1}))
        h = h2
    calls.append(("rmsnorm_fwd", {"x2d": h, "w": "norm", "eps": EPS}))
    return calls


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp4"])
def test_once_pass_is_seven_launches_per_layer(monkeypatch, mode):
    rec = OperandRecorder(monkeypatch, gemv_fits=False, decode_fits=False)
    want = expected_once(mode)
    assert len(want) == 7 * LAYERS + 1
    _check(rec, _engine17(rec, mode), want)


def test_once_pass_with_split_attention(monkeypatch):
    rec = OperandRecorder(monkeypatch, gemv_fits=False, decode_fits=False)
    _check(rec, _engine17(rec, "bf16", attention="split"), expected_once("bf16", attention="attn_chunk_split"))


def test_once_pass_weights_apart_runs_plain_launches_and_swiglu_fwd(monkeypatch):
    rec = OperandRecorder(monkeypatch, gemv_fits=False, decode_fits=False)
    _check(rec, _engine17(rec, "bf16", packed=False), expected_once("bf16", packed=False))


def test_default_mode_at_17_rows_keeps_the_fused_pass(monkeypatch):
    """ "fused" at 17 rows: five launches per layer, none of them a stand-alone norm or the new wrapper."""
    rec = OperandRecorder(monkeypatch, gemv_fits=False, decode_fits=False)
    eng = _engine17(rec, "bf16", operand="fused")
    eng._suffix_pass()
    names = [c[0] for c in rec.calls]
    assert names == (["gemm_skinny", "attn_chunk", "gemm_skinny", "gemm_skinny", "gemm_skinny"] * LAYERS + ["rmsnorm_fwd"])
    assert rec.calls[0][1]["norm_weight"] == "L0.ln1" and rec.calls[4][1]["swiglu"] is True


@pytest.mark.parametrize("mode,kernel", [("bf16", "gemv"), ("fp8", "gemv_w8"), ("fp4", "gemv_w4")])
def test_once_up_to_8_rows_is_the_fused_pass(monkeypatch, mode, kernel):
    """R = 4 (gemv_fits true): the list of "once" is the list of "fused", launch for launch."""
    rec = OperandRecorder(monkeypatch, gemv_fits=True)
    B, S_p = 1, 12
    eng = _prefix_engine(rec, mode, B, S_p)
    eng.suffix_operand = "once"
    _check(rec, eng, expected_prefix(mode, B, S_p, kernel, "attn_decode"))


def test_once_at_8_rows_of_two_samples_is_the_fused_pass(monkeypatch):
    """The switch is on B * R, not on R: 2 samples x 4 rows = 8 rows keep the five launches."""
    rec = OperandRecorder(monkeypatch, gemv_fits=True)
    eng = _prefix_engine(rec, "bf16", 2, 12)
    eng.suffix_operand = "once"
    _check(rec, eng, expected_prefix("bf16", 2, 12, "gemv", "attn_decode"))


def test_mode_validation():
    assert infer.MODES["suffix_operand"].values == ("fused", "once")
    infer.check_mode("suffix_operand", "fused")
    infer.check_mode("suffix_operand", "once")
    infer.check_mode("suffix_operand", "fused", reuse_prefix=False)
    for bad in ("Once", "", None, "plain"):
        with pytest.raises(ValueError, match="suffix_operand"):
            infer.check_mode("suffix_operand", bad)
    with pytest.raises(ValueError, match="reuse_prefix"):
        infer.check_mode("suffix_operand", "once", reuse_prefix=False)
    with pytest.raises(ValueError, match="suffix_operand"):
        infer.needs_engine("PrefixCachedEps", 70, suffix_operand="once")
    infer.needs_engine("PrefixCachedEps", 70, suffix_operand="fused")


def test_public_methods_validate_the_mode_in_front_of_everything_else():
    from mla_amd.mla import MLA
    # every other mode is wrong too: the error names suffix_operand
    with pytest.raises(ValueError, match="suffix_operand"):
        infer.check_modes(infer.Modes(suffix_weights="nope", prefill="nope", sampler="nope", suffix_attention="nope", prefill_precision="nope",
                                      groups_attention="nope", ddpm_sampler="nope", suffix_operand="nope"), True, True, 8)
    base = dict(suffix_weights="bf16", prefill="train", sampler="host", suffix_attention="head")
    with pytest.raises(ValueError, match="suffix_operand"):
        infer.check_modes(infer.Modes(**base, suffix_operand="once"), False, True, 8)
    infer.check_modes(infer.Modes(**base, suffix_operand="once"), True, True, 8)
    stand_in = types.SimpleNamespace()                                        # the mode errors come before `self` is touched
    for method, args in ((MLA.predict_action_diff, ()), (MLA.predict_action_diff_samples, ()), (MLA.predict_action_diff_batch, ([None], [None]))):
        with pytest.raises(ValueError, match="suffix_operand"):
            method(stand_in, *args, suffix_operand="twice", suffix_weights="nope")
        with pytest.raises(ValueError, match="suffix_operand"):
            method(stand_in, *args, suffix_operand="once", reuse_prefix=False)


def test_engine_key_carries_the_mode():
    made = []

    class Eng(infer._CachedEpsBase):
        def __init__(self, vlm, *ctor):
            made.append(ctor)

    vlm = types.SimpleNamespace()
    a = Eng._engine(vlm, "store", ("k", 1), ("fused",))
    b = Eng._engine(vlm, "store", ("k", 1), ("once",), suffix_operand="once")
    c = Eng._engine(vlm, "store", ("k", 1), ("once+split",), suffix_attention="split", suffix_operand="once")
    assert a is not b and b is not c and made == [("fused",), ("once",), ("once+split",)]
    assert list(vlm.__dict__["store"]) == [("k", 1), ("k", 1, "operand:once"), ("k", 1, "attention:split", "operand:once")]
    assert Eng._engine(vlm, "store", ("k", 1), ("again",), suffix_operand="once") is b and len(made) == 3
    assert infer._CachedEpsBase.suffix_operand == "fused" and math.isfinite(SCALE)
