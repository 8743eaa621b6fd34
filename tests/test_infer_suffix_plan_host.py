"""The launches of a cached-prefix suffix pass, per engine, as a recorded list (CPU, no library): which mla_amd.hip wrapper, with which
scalars and WHICH tensors (the cache, the slot / length tensors, the rope tables, the residual), in which order. The engines are built
without a model (`Class.__new__` plus the attributes a pass reads), the wrappers are replaced by recorders that return CPU tensors of the
right shape. The expected lists are written from the engines' contract, not from the code:

  per layer, row-GEMM engines (M = all suffix rows of the pass, c = the layer's cache)
    rmsnorm_fwd -> q|k|v projection into the cache -> attention -> o + residual -> rmsnorm_fwd -> gate|up -> swiglu_fwd -> down + residual
    engine                    q|k|v (ldo, out_batch_stride, rows_per_batch) + keywords                                    attention
    BatchedPrefixCachedEps    (c.stride(-2), c.stride(0), R), slot, cap_rows=S_cap, rope                                  attn_chunk_ragged(c, B, nheads, D, kv_len, R, scale)
    SampleGroupsEps           (c.stride(0), R * c.stride(0), R), slot, cap_rows=S_p + R, rope                             attn_chunk_groups(c, G, nheads, D, S_p, R, scale)
    BatchedSampleGroupsEps    (c.stride(-2), 0, R), slot, cap_rows=NB * S_cap, rope, rope_pos, rope_rows=S_cap            attn_chunk_ragged_groups(c, NB, G, nheads, D, prefix_len, R, scale)
  every other projection: (out.stride(0), 0, M) into a fresh [M, N] tensor, residual=h for o and residual=h1 for down

  per layer, PrefixCachedEps: q|k|v (RMSNorm in the input staging, RoPE in the epilogue) into cache rows [S_p, S_p + R) of every sample ->
    attention -> o + residual -> gate|up (RMSNorm in the input staging) -> down (SwiGLU in the input staging) + residual

Only the lines that build the fake engines may follow the engines' attributes; the expected lists are the contract."""
import inspect
import math
import types

import pytest
import torch

from mla_amd import hip, infer

H, NHEADS, D, I, R, LAYERS = 256, 2, 128, 512, 4, 2
EPS, SCALE = 1e-5, 1.0 / math.sqrt(128)
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------- recording
class Recorder:
    """Replaces the wrappers a pass may call. A tensor argument is recorded as the label of the known tensor whose storage holds its first
    element (+ the element offset when it is a view further in); a tensor seen for the first time is a fresh one and gets the label
    "@<call>.<argument><shape>"; a returned tensor is "@<call>.ret<shape>". Arguments at their default value are left out, so positional
    and keyword calls record the same."""

    def __init__(self, monkeypatch, gemv_fits=True, decode_fits=None):
        self.calls, self.roots, self.keep = [], [], []
        for name, ret in (("rmsnorm_fwd", self._rms), ("swiglu_fwd", self._swiglu), ("rope_inplace", None),
                          ("gemv", None), ("gemm_skinny", None), ("gemv_w8", None), ("gemm_skinny_w8", None),
                          ("gemv_w4", None), ("gemm_skinny_w4", None),
                          ("gemm_suffix", None), ("gemm_suffix_w8", None), ("gemm_suffix_w4", None),
                          ("attn_decode", self._attn), ("attn_chunk", self._attn), ("attn_chunk_split", self._attn),
                          ("attn_chunk_ragged", self._attn), ("attn_chunk_groups", self._attn_groups),
                          ("attn_chunk_ragged_groups", self._attn_ragged_groups)):
            monkeypatch.setattr(hip, name, self._wrap(name, getattr(hip, name), ret))
        monkeypatch.setattr(hip, "gemv_fits", lambda M, K: gemv_fits)
        if decode_fits is not None:
            monkeypatch.setattr(hip, "attn_decode_fits", lambda R_, S_kv: decode_fits)

    def know(self, label, t):
        self.keep.append(t)                                                   # alive to the end: no address is handed out twice
        self.roots.append((t.data_ptr(), t.data_ptr() + max(t.numel(), 1) * t.element_size(), t.element_size(), label))
        return t

    def label(self, t, where):
        p = t.data_ptr()
        for lo, hi, es, label in self.roots:
            if lo <= p < hi:
                return label if p == lo else f"{label}+{(p - lo) // es}"
        self.know(f"{where}{list(t.shape)}", t)
        return f"{where}{list(t.shape)}"

    def _norm(self, v, where):
        if torch.is_tensor(v):
            return self.label(v, where)
        if isinstance(v, tuple):
            return tuple(self._norm(x, where) for x in v)
        return v

    def _wrap(self, name, real, ret):
        sig = inspect.signature(real)

        def rec(*a, **kw):
            i = len(self.calls)
            bound = sig.bind(*a, **kw)
            args = {k: self._norm(v, f"@{i}.{k}") for k, v in bound.arguments.items()
                    if not (sig.parameters[k].default is not inspect.Parameter.empty and _same(v, sig.parameters[k].default))}
            self.calls.append((name, args))
            if ret is None:
                return None
            out = ret(i, bound.arguments)
            self.know(f"@{i}.ret{list((out[0] if isinstance(out, tuple) else out).shape)}", out[0] if isinstance(out, tuple) else out)
            return out
        return rec

    @staticmethod
    def _rms(i, a):
        return torch.full(a["x2d"].shape, float(i), dtype=BF16), None

    @staticmethod
    def _swiglu(i, a):
        return torch.zeros((a["gu2d"].shape[0], a["gu2d"].shape[1] // 2), dtype=BF16)

    @staticmethod
    def _attn(i, a):
        return torch.zeros((a["B"] * a["R"], a["nheads"] * a["D"]), dtype=BF16)

    @staticmethod
    def _attn_groups(i, a):
        return torch.zeros((a["G"] * a["R"], a["nheads"] * a["D"]), dtype=BF16)

    @staticmethod
    def _attn_ragged_groups(i, a):
        return torch.zeros((a["B"] * a["G"] * a["R"], a["nheads"] * a["D"]), dtype=BF16)


def _same(v, default):
    if torch.is_tensor(v) or torch.is_tensor(default):
        return v is default
    return v == default


# ---------------------------------------------------------------------------------------------------- fake weights and engines
def _layer_weights(rec, mode, packed=True):
    """Per layer: what _weights() / _quantised() hand a pass in `mode`, every tensor known to the recorder.
    bf16: (ln1, wq, wk, wv, wo, ln2, wg, wu, wd) with q|k|v and gate|up adjacent (packed) or apart; fp8: (ln1, W8, W8, ln2, W8, W8);
    fp4: (ln1, W4, W4, ln2, W4, W4) -- code pairs [N, K / 2] and block scales [N, K / 32], both uint8."""
    out = []
    for l in range(LAYERS):
        ln1, ln2 = rec.know(f"L{l}.ln1", torch.ones(H, dtype=BF16)), rec.know(f"L{l}.ln2", torch.ones(H, dtype=BF16))
        if mode == "fp8":
            mats = []
            for name, (N, K) in (("qkv", (3 * H, H)), ("o", (H, H)), ("gu", (2 * I, H)), ("d", (H, I))):
                mats.append(infer.W8(rec.know(f"L{l}.{name}.q", torch.zeros((N, K), dtype=torch.float8_e4m3fn)),
                                     rec.know(f"L{l}.{name}.scale", torch.ones(N, dtype=torch.float32))))
            out.append((ln1, mats[0], mats[1], ln2, mats[2], mats[3]))
            continue
        if mode == "fp4":
            mats = []
            for name, (N, K) in (("qkv", (3 * H, H)), ("o", (H, H)), ("gu", (2 * I, H)), ("d", (H, I))):
                mats.append(infer.W4(rec.know(f"L{l}.{name}.q", torch.zeros((N, K // 2), dtype=torch.uint8)),
                                     rec.know(f"L{l}.{name}.s", torch.zeros((N, K // 32), dtype=torch.uint8))))
            out.append((ln1, mats[0], mats[1], ln2, mats[2], mats[3]))
            continue
        wo, wd = rec.know(f"L{l}.o", torch.zeros((H, H), dtype=BF16)), rec.know(f"L{l}.d", torch.zeros((H, I), dtype=BF16))
        if packed:
            qkv, gu = rec.know(f"L{l}.qkv", torch.zeros((3 * H, H), dtype=BF16)), rec.know(f"L{l}.gu", torch.zeros((2 * I, H), dtype=BF16))
            wq, wk, wv, wg, wu = qkv[:H], qkv[H:2 * H], qkv[2 * H:], gu[:I], gu[I:]
        else:
            wq, wk, wv = (rec.know(f"L{l}.{n}", torch.zeros((H, H), dtype=BF16)) for n in "qkv")
            wg, wu = (rec.know(f"L{l}.{n}", torch.zeros((I, H), dtype=BF16)) for n in "gu")
        out.append((ln1, wq, wk, wv, wo, ln2, wg, wu, wd))
    return out


def _fake(cls, rec, mode, rows, caches, weights=None, **attrs):
    """cls.__new__ plus what a suffix pass reads. ---- the only lines that follow the engines' attributes ----"""
    e = cls.__new__(cls)
    e.suffix_weights, e.suffix_mx = ("bf16", "fp4") if mode == "fp4" else (mode, "off")
    e.suffix_attention, e._attn_ws = "head", None
    e.R, e.T, e.H, e.D, e.nheads, e.eps = R, R - 1, H, D, NHEADS, EPS
    e.model = types.SimpleNamespace(norm=types.SimpleNamespace(weight=rec.know("norm", torch.ones(H, dtype=BF16))))
    e._suffix = e._packed = weights if weights is not None else _layer_weights(rec, mode)
    e.cache = [rec.know(f"cache{l}", c) for l, c in enumerate(caches)]
    e.h_in, e.h_out = rec.know("h_in", torch.zeros((rows, H), dtype=BF16)), torch.zeros((rows, H), dtype=BF16)
    for k, v in attrs.items():
        setattr(e, k, rec.know(k, v) if torch.is_tensor(v) else v)
    return e


def _i32(n):
    return torch.zeros(n, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------- expected lists
SUFFIX = {"bf16": "", "fp8": "_w8", "fp4": "_w4"}                             # of the wrapper a pass over `mode` weights calls


def _w(l, name, mode):
    if mode == "bf16":
        return {"W": f"L{l}.{name}"}
    return {"W": f"L{l}.{name}.q", "w_scale": f"L{l}.{name}." + {"fp8": "scale", "fp4": "s"}[mode]}


def expected_row_gemm(mode, M, qkv_out, attention):
    """The eight launches per layer of the row-GEMM engines + the final norm. qkv_out(l): (ldo, out_batch_stride, rows_per_batch, keywords)
    of the cache write; attention(l): (wrapper, arguments)."""
    gemm = "gemm_suffix" + SUFFIX[mode]
    calls, h = [], "h_in"
    for l in range(LAYERS):
        i = len(calls)
        ldo, obs, rpb, kw = qkv_out(l)
        name, args = attention(l)
        xn, o, h1, xn2, gu, act, h2 = (f"@{i}.ret[{M}, {H}]", f"@{i + 2}.ret[{M}, {H}]", f"@{i + 3}.out[{M}, {H}]", f"@{i + 4}.ret[{M}, {H}]",
                                       f"@{i + 5}.out[{M}, {2 * I}]", f"@{i + 6}.ret[{M}, {I}]", f"@{i + 7}.out[{M}, {H}]")
        calls += [
            ("rmsnorm_fwd", {"x2d": h, "w": f"L{l}.ln1", "eps": EPS}),
            (gemm, {"x": xn, **_w(l, "qkv", mode), "out": f"cache{l}", "ldo": ldo, "out_batch_stride": obs, "rows_per_batch": rpb, **kw}),
            (name, args),
            (gemm, {"x": o, **_w(l, "o", mode), "out": h1, "ldo": H, "out_batch_stride": 0, "rows_per_batch": M, "residual": h}),
            ("rmsnorm_fwd", {"x2d": h1, "w": f"L{l}.ln2", "eps": EPS}),
            (gemm, {"x": xn2, **_w(l, "gu", mode), "out": gu, "ldo": 2 * I, "out_batch_stride": 0, "rows_per_batch": M}),
            ("swiglu_fwd", {"gu2d": gu}),
            (gemm, {"x": act, **_w(l, "d", mode), "out": h2, "ldo": H, "out_batch_stride": 0, "rows_per_batch": M, "residual": h1}),
        ]
        h = h2
    calls.append(("rmsnorm_fwd", {"x2d": h, "w": "norm", "eps": EPS}))
    return calls


def _check(rec, eng, expected):
    eng._suffix_pass()
    assert len(rec.calls) == len(expected), [c[0] for c in rec.calls]
    for i, (got, want) in enumerate(zip(rec.calls, expected)):
        assert got == want, f"launch {i}: {got} != {want}"
    assert bool((eng.h_out == float(len(expected) - 1)).all()), "h_out holds the final norm's rows"


# ---------------------------------------------------------------------------------------------------- the row-GEMM engines
def test_batched_prefix_engine_launches(monkeypatch):
    rec = Recorder(monkeypatch)
    B, S_cap = 3, 64
    eng = _fake(infer.BatchedPrefixCachedEps, rec, "bf16", B * R, [torch.zeros((B, S_cap, 3 * H), dtype=BF16) for _ in range(LAYERS)],
                B=B, S_cap=S_cap, slot=_i32(B), kv_len=_i32(B), cos_c=torch.zeros((S_cap, D)), sin_c=torch.zeros((S_cap, D)))
    _check(rec, eng, expected_row_gemm(
        "bf16", B * R,
        lambda l: (3 * H, S_cap * 3 * H, R, {"slot": "slot", "cap_rows": S_cap, "rope": ("cos_c", "sin_c", 2 * H)}),
        lambda l: ("attn_chunk_ragged", {"cache": f"cache{l}", "B": B, "nheads": NHEADS, "D": D, "kv_len": "kv_len", "R": R, "scale": SCALE})))


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp4"])
def test_sample_groups_engine_launches(monkeypatch, mode):
    rec = Recorder(monkeypatch)
    G, capacity, S_p = 2, 3, 10
    eng = _fake(infer.SampleGroupsEps, rec, mode, capacity * R, [torch.zeros((S_p + capacity * R, 3 * H), dtype=BF16) for _ in range(LAYERS)],
                capacity=capacity, S_p=S_p, slot=_i32(capacity), cos_c=torch.zeros((S_p + R, D)), sin_c=torch.zeros((S_p + R, D)), _graphs={})
    eng._h_in, eng._h_out = eng.h_in, eng.h_out
    eng.set_groups(G)
    assert eng.B == G and eng.h_in.shape[0] == G * R and eng.h_in.data_ptr() == eng._h_in.data_ptr()
    _check(rec, eng, expected_row_gemm(
        mode, G * R,
        lambda l: (3 * H, R * 3 * H, R, {"slot": "slot", "cap_rows": S_p + R, "rope": ("cos_c", "sin_c", 2 * H)}),
        lambda l: ("attn_chunk_groups", {"cache": f"cache{l}", "G": G, "nheads": NHEADS, "D": D, "S_p": S_p, "R": R, "scale": SCALE})))


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp4"])
def test_batched_sample_groups_engine_launches(monkeypatch, mode):
    rec = Recorder(monkeypatch)
    NB, G, S_cap = 2, 2, 64
    eng = _fake(infer.BatchedSampleGroupsEps, rec, mode, NB * G * R, [torch.zeros((NB, S_cap, 3 * H), dtype=BF16) for _ in range(LAYERS)],
                NB=NB, G=G, B=NB * G, S_cap=S_cap, prefix_len=_i32(NB), slot=_i32(NB * G), rope_pos=_i32(NB * G),
                cos_c=torch.zeros((S_cap, D)), sin_c=torch.zeros((S_cap, D)))
    _check(rec, eng, expected_row_gemm(
        mode, NB * G * R,
        lambda l: (3 * H, 0, R, {"slot": "slot", "cap_rows": NB * S_cap, "rope": ("cos_c", "sin_c", 2 * H), "rope_pos": "rope_pos",
                                 "rope_rows": S_cap}),
        lambda l: ("attn_chunk_ragged_groups", {"cache": f"cache{l}", "B": NB, "G": G, "nheads": NHEADS, "D": D, "prefix_len": "prefix_len",
                                                "R": R, "scale": SCALE})))


# ---------------------------------------------------------------------------------------------------- PrefixCachedEps
def _prefix_engine(rec, mode, B, S_p, packed=True, attention="head"):
    S_cap = S_p + R
    eng = _fake(infer.PrefixCachedEps, rec, mode, B * R, [torch.zeros((B, S_cap, 3 * H), dtype=BF16) for _ in range(LAYERS)],
                weights=_layer_weights(rec, mode, packed), B=B, S_p=S_p, S_cap=S_cap, cos_s=torch.zeros((R, D)), sin_s=torch.zeros((R, D)))
    if attention == "split":
        eng.suffix_attention, eng._attn_ws = "split", rec.know("attn_ws", torch.zeros(64, dtype=torch.uint8))
    return eng


def expected_prefix(mode, B, S_p, kernel, attention, packed=True):
    """PrefixCachedEps: five launches per layer with packed weights; apart (bf16 only): one launch per weight at its output column, the
    rotary embedding as its own launch per sample."""
    M, S_cap = B * R, S_p + R
    pre1 = lambda l: {"norm_weight": f"L{l}.ln1", "eps": EPS}                 # noqa: E731
    pre2 = lambda l: {"norm_weight": f"L{l}.ln2", "eps": EPS}                 # noqa: E731
    calls, h = [], "h_in"
    for l in range(LAYERS):
        c, into = f"cache{l}", {"out": f"cache{l}+{S_p * 3 * H}", "ldo": 3 * H, "out_batch_stride": S_cap * 3 * H, "rows_per_batch": R}
        if packed:
            calls.append((kernel, {"x": h, **_w(l, "qkv", mode), **into, **pre1(l), "rope": ("cos_s", "sin_s", 2 * H)}))
        else:
            calls += [(kernel, {"x": h, "W": f"L{l}.{n}", **into, **({"out_col": j * H} if j else {}), **pre1(l)}) for j, n in enumerate("qkv")]
            calls += [("rope_inplace", {"buf2d": f"{c}+{(b * S_cap + S_p) * 3 * H}", "cos": "cos_s", "sin": "sin_s", "S": R, "nheads": NHEADS,
                                        "D": D, "q_off": 0, "k_off": H}) for b in range(B)]
        i = len(calls)
        calls.append((attention, {"cache": c, "B": B, "nheads": NHEADS, "D": D, "S_kv": S_cap, "R": R, "scale": SCALE,
                                  **({"ws": "attn_ws"} if attention == "attn_chunk_split" else {})}))
        o, h1 = f"@{i}.ret[{M}, {H}]", f"@{i + 1}.out[{M}, {H}]"
        fresh = lambda out, N: {"out": out, "ldo": N, "out_batch_stride": 0, "rows_per_batch": M}        # noqa: E731
        calls.append((kernel, {"x": o, **_w(l, "o", mode), **fresh(h1, H), "residual": h}))
        gu = f"@{i + 2}.out[{M}, {2 * I}]"
        if packed:
            calls.append((kernel, {"x": h1, **_w(l, "gu", mode), **fresh(gu, 2 * I), **pre2(l)}))
        else:
            calls += [(kernel, {"x": h1, "W": f"L{l}.{n}", **fresh(gu, 2 * I), **({"out_col": j * I} if j else {}), **pre2(l)})
                      for j, n in enumerate("gu")]
        h2 = f"@{len(calls)}.out[{M}, {H}]"
        calls.append((kernel, {"x": gu, **_w(l, "d", mode), **fresh(h2, H), "residual": h1, "swiglu": True}))
        h = h2
    calls.append(("rmsnorm_fwd", {"x2d": h, "w": "norm", "eps": EPS}))
    return calls


@pytest.mark.parametrize("mode,fits,kernel", [("bf16", True, "gemv"), ("bf16", False, "gemm_skinny"),
                                               ("fp8", True, "gemv_w8"), ("fp8", False, "gemm_skinny_w8"),
                                               ("fp4", True, "gemv_w4"), ("fp4", False, "gemm_skinny_w4")])
def test_prefix_engine_launches_packed(monkeypatch, mode, fits, kernel):
    rec = Recorder(monkeypatch, gemv_fits=fits)
    B, S_p = 1, 12
    assert hip.attn_decode_fits(R, S_p + R)
    _check(rec, _prefix_engine(rec, mode, B, S_p), expected_prefix(mode, B, S_p, kernel, "attn_decode"))


@pytest.mark.parametrize("fits,kernel", [(True, "gemv"), (False, "gemm_skinny")])
def test_prefix_engine_launches_weights_apart(monkeypatch, fits, kernel):
    rec = Recorder(monkeypatch, gemv_fits=fits)
    B, S_p = 2, 12
    _check(rec, _prefix_engine(rec, "bf16", B, S_p, packed=False), expected_prefix("bf16", B, S_p, kernel, "attn_decode", packed=False))


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp4"])
@pytest.mark.parametrize("attention,decode_fits,wrapper", [("head", False, "attn_chunk"), ("split", True, "attn_chunk_split"),
                                                            ("split", False, "attn_chunk_split")])
def test_prefix_engine_attention_launch(monkeypatch, mode, attention, decode_fits, wrapper):
    rec = Recorder(monkeypatch, gemv_fits=True, decode_fits=decode_fits)
    B, S_p = 1, 12
    _check(rec, _prefix_engine(rec, mode, B, S_p, attention=attention),
           expected_prefix(mode, B, S_p, "gemv" + SUFFIX[mode], wrapper))
