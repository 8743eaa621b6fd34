"""ctypes binding of libmla_hip.so (C-ABI declared in include/mla_hip.h).

The header is the one statement of every signature: the build shows it to the compiler next to each definition, and the argtypes and
restypes set in lib() are parsed from it at import (abi.py), so a new entry point needs its definition, its declaration and its
wrapper here -- no ctypes row. Entry points added after the first header's symbol set was pinned (tests/test_abi.py) are declared
in its sibling include/mla_hip_optim.h, which is treated the same way.

Every wrapper launches on torch's current HIP stream, never synchronises, and raises RuntimeError on a
non-zero return code. There is deliberately NO fallback: if the shared library is missing or a kernel rejects its
arguments the product path fails loudly (oracle/ is test infrastructure only).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_void_p
from typing import NamedTuple, Optional

import torch

from . import abi

_LIB_PATH = os.environ.get("MLA_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmla_hip.so")   # override: A/B experiments
_lib = None

ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, ACT_SILU = 0, 1, 2, 3

# split-K tail of the 256x256 GEMM (mla_gemm_bf16_ws): on by default; MLA_GEMM_SPLITK=0 turns it off for A/B measurements
SPLITK = os.environ.get("MLA_GEMM_SPLITK", "1") != "0"
SPLITK_WS_BYTES = int(os.environ.get("MLA_GEMM_SPLITK_WS_MB", "64")) << 20     # fp32 partial tiles of the K-slices (256 KiB each); 256 MiB would also split the 688-tile down-projection wgrad (176 tail tiles x 4): measured 1.2 % SLOWER per launch

# bench.py sets this to a list to time every GEMM launch with HIP events on the launch stream (roofline.achieved)
GEMM_PROFILE = None

# name -> argtypes / restype of every entry point, derived from the header's declarations (abi.py): there is no hand-written ctypes row
_HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mla_hip.h")
_RESTYPES, _SIGNATURES = abi.load(_HEADER_PATH)
# the sibling header (entry points added after mla_hip.h's symbol set was pinned, see its opening comment): a second derived table.
# _SIGNATURES, _RESTYPES and exported_symbols() keep describing mla_hip.h alone; lib() binds both.
_OPTIM_HEADER_PATH = os.path.join(os.path.dirname(_HEADER_PATH), "mla_hip_optim.h")
_OPTIM_RESTYPES, _OPTIM_SIGNATURES = abi.load(_OPTIM_HEADER_PATH)


def exported_symbols():
    """Names every build of libmla_hip.so must export: the header's declarations (checked by the CPU test-suite)."""
    return sorted(_SIGNATURES)


def lib():
    """Load the shared library (once). Raises if it is absent -- there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(mla_amd has no CPU fallback)")
        L = ctypes.CDLL(_LIB_PATH)
        for sigs, rets in ((_SIGNATURES, _RESTYPES), (_OPTIM_SIGNATURES, _OPTIM_RESTYPES)):
            for name, argt in sigs.items():
                fn = getattr(L, name)
                fn.argtypes = argt
                fn.restype = rets[name]
        _lib = L
    return _lib


def gemm_cus(n: int = -1) -> int:
    """CUs the GEMM launches plan their split-K tails for (mla_gemm_cus): n >= 8 (multiple of 8) sets, 0 = device count, < 0 queries."""
    return lib().mla_gemm_cus(n)


def side_traffic(a32, b32, out32, blocks: int, lds_bytes: int = 0, sleep_ticks: int = 0):
    """Stand-in for a collective's kernel on the CURRENT stream (mla_side_traffic): out = a + b streamed by `blocks` workgroups."""
    call("mla_side_traffic", _p(a32), _p(b32), _p(out32), a32.numel(), blocks, lds_bytes, sleep_ticks)


def gemm_source_id() -> str:
    """sha256[:16] over the gemm256 kernel family's sources the loaded library was built from (build.sh stamps it)."""
    return lib().mla_gemm_source_id().decode()


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def _check(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {lib().mla_last_error().decode()}")


def _req(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor must live on the GPU (mla_amd has no CPU path)")


def call(name: str, *args):
    """Raw call helper: appends the current stream and checks the return code."""
    rc = getattr(lib(), name)(*args, _stream())
    _check(rc, name)


_ws_cache = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Per-(device, stream) scratch buffer owned by torch (kernels never allocate)."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 24), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# --------------------------------------------------------------------------------------------- GEMM
def gemm(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, *, a_mode: int = 0, b_mode: int = 0,
         M: Optional[int] = None, N: Optional[int] = None, K: Optional[int] = None, lda: Optional[int] = None,
         ldb: Optional[int] = None, ldc: Optional[int] = None, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, ldr: Optional[int] = None, out_dtype=torch.bfloat16,
         accumulate: bool = False, alpha: float = 1.0, force_generic: int = 0) -> torch.Tensor:
    """C[M,N] = alpha * sum_k Aop(m,k) Bop(n,k) (+bias[n]) (+residual[m,n]) (+C if accumulate).

    a_mode/b_mode 0: operand stored [rows, K] (k contiguous); 1: stored [K, rows] (reduction-major).
    force_generic: 0 = auto (256x256 kernel for large k-contiguous shapes, else 128x128, else SIMT fallback),
    1 = SIMT fallback, 2 = never use the 256x256 kernel, 3 = force the 256x256 kernel for any mode (tests / A-B).
    2-D tensors with unit inner stride; leading dimension taken from stride(0).
    """
    _req(a, torch.bfloat16, "gemm a")
    _req(b, torch.bfloat16, "gemm b")
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    if M is None:
        M = a.shape[0] if a_mode == 0 else a.shape[1]
    if K is None:
        K = a.shape[1] if a_mode == 0 else a.shape[0]
    if N is None:
        N = b.shape[0] if b_mode == 0 else b.shape[1]
    kb = b.shape[1] if b_mode == 0 else b.shape[0]
    if kb != K:
        raise ValueError(f"gemm: reduction mismatch {K} vs {kb}")
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    assert out.stride(-1) == 1
    out_fp32 = 1 if out.dtype == torch.float32 else 0
    if not out_fp32:
        _req(out, torch.bfloat16, "gemm out")
    ldc = out.stride(0) if ldc is None else ldc
    if residual is not None:
        _req(residual, torch.bfloat16, "gemm residual")
        ldr = residual.stride(0) if ldr is None else ldr
    if bias is not None:
        _req(bias, torch.bfloat16, "gemm bias")
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()   # torch's current stream == the stream the kernel is launched on (see _stream())
    if SPLITK and (force_generic & 15) == 0 and M >= 256 and N >= 256:
        ws = workspace(SPLITK_WS_BYTES, a.device)      # per (device, stream) scratch owned by torch
        call("mla_gemm_bf16_ws", _p(a), _p(b), _p(out), _p(residual), _p(bias), M, N, K, lda, ldb, ldc, ldr or 0, a_mode, b_mode,
             out_fp32, 1 if accumulate else 0, float(alpha), int(force_generic), _p(ws), SPLITK_WS_BYTES)
    else:
        call("mla_gemm_bf16", _p(a), _p(b), _p(out), _p(residual), _p(bias), M, N, K, lda, ldb, ldc, ldr or 0, a_mode, b_mode,
             out_fp32, 1 if accumulate else 0, float(alpha), int(force_generic))
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * M * N * K, (a_mode, b_mode, M, N, K)))
    return out


def gemm_kloop(mode: int = -1) -> int:
    """Selects (0 / 1) or queries (-1) the main loop of the 256x256 GEMM's k-contiguous instantiations: 1 = hand-scheduled assembly
    (default), 0 = compiler-scheduled. Same bits either way; for A/B measurements and tests."""
    return int(lib().mla_gemm_kloop(int(mode)))


def gemm_sq_slots(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, a_mode: int = 0, b_mode: int = 0) -> int:
    """Number of sum-of-squares partials gemm_sq() writes for these operands, or -1 when the shape is outside its contract."""
    M, K = a.shape if a_mode == 0 else (a.shape[1], a.shape[0])
    N, kb = b.shape if b_mode == 0 else (b.shape[1], b.shape[0])
    ok = (a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and out.dtype == torch.float32 and kb == K and
          (a_mode == 0 or M % 8 == 0) and
          a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1 and M >= 256 and N >= 256 and K % 64 == 0 and N % 8 == 0 and
          a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0 and out.stride(0) % 8 == 0 and
          all(t.data_ptr() % 16 == 0 for t in (a, b, out)) and tuple(out.shape) == (M, N))
    if not ok:
        return -1
    return int(lib().mla_gemm_sq_slots(M, N, K, SPLITK_WS_BYTES if SPLITK else 0))


def gemm_sq(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, accumulate: bool, part: Optional[torch.Tensor] = None,
            a_mode: int = 0, b_mode: int = 0):
    """out[M, N] (fp32) (+)= a[M, K] b[N, K]^T like gemm(), and sum(out^2) of the FINAL values as partial sums written to `part`
    (fp32, >= gemm_sq_slots() elements; allocated here when None): returns (part, number of valid partials) -- or None when the shape
    is outside the 256x256 kernel (the caller then runs gemm() and the gradient norm reads the buffer as before).
    mla_sum_partials adds the partials up in a fixed order. a_mode / b_mode as in gemm(): 1 = that operand is stored [K, rows]."""
    need = gemm_sq_slots(a, b, out, a_mode, b_mode)
    if need < 0:
        return None
    M, K = a.shape if a_mode == 0 else (a.shape[1], a.shape[0])
    N = b.shape[0] if b_mode == 0 else b.shape[1]
    if part is None:
        part = torch.empty(need, dtype=torch.float32, device=out.device)
    assert part.dtype == torch.float32 and part.is_contiguous() and part.numel() >= need
    slots = ctypes.c_int(0)
    ws = workspace(SPLITK_WS_BYTES, a.device) if SPLITK else None
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    if a_mode or b_mode:
        call("mla_gemm_bf16_ws_sq_rm", _p(a), _p(b), _p(out), M, N, K, a.stride(0), b.stride(0), out.stride(0), int(a_mode), int(b_mode),
             1 if accumulate else 0, 1.0, _p(ws), SPLITK_WS_BYTES if ws is not None else 0, _p(part), part.numel(), ctypes.byref(slots))
    else:
        call("mla_gemm_bf16_ws_sq", _p(a), _p(b), _p(out), M, N, K, a.stride(0), b.stride(0), out.stride(0), 1 if accumulate else 0, 1.0,
             _p(ws), SPLITK_WS_BYTES if ws is not None else 0, _p(part), part.numel(), ctypes.byref(slots))
    assert int(slots.value) == need
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * M * N * K, (a_mode, b_mode, M, N, K)))
    return part, need


def sum_partials(partials: torch.Tensor, n: int, out1: torch.Tensor, accumulate: bool):
    call("mla_sum_partials", _p(partials), int(n), _p(out1), 1 if accumulate else 0)


def _rs_args(norm, rows, device):
    """(ss, parts, eps, rstd) of a folded RMSNorm for the _rs entry points. norm = (ss [rows, parts] fp32 or None, rstd [rows] fp32 or
    None, eps): partials given -> rstd is computed by the launch and returned; else the given rstd is read."""
    ss, rstd, eps = norm
    if ss is not None:
        assert ss.dtype == torch.float32 and ss.is_contiguous() and ss.shape[0] == rows
        rstd = torch.empty(rows, dtype=torch.float32, device=device)
        return ss, int(ss.shape[1]), float(eps), rstd
    assert rstd is not None and rstd.dtype == torch.float32 and rstd.is_contiguous() and rstd.numel() == rows
    return None, 0, float(eps), rstd


def qkv_rope_ok(x2d, wqkv, out, cos, sin, S, rope_cols) -> bool:
    T, K = x2d.shape
    N = wqkv.shape[0]
    return (T >= 256 and N >= 256 and K % 64 == 0 and N % 8 == 0 and rope_cols % 256 == 0 and x2d.stride(0) % 8 == 0 and
            wqkv.stride(0) % 8 == 0 and out.stride(0) % 8 == 0 and cos.dtype == torch.float32 and cos.is_contiguous() and
            sin.is_contiguous() and cos.shape == (S, 64) and all(t.data_ptr() % 16 == 0 for t in (x2d, wqkv, out, cos, sin)))


def gemm_qkv_rope(x2d, wqkv, out, cos, sin, S, rope_cols, norm=None):
    """out[T, N] = x2d @ wqkv^T with RoPE applied to columns [0, rope_cols) in the GEMM epilogue (bit-identical to gemm + rope_inplace).
    Returns False when the shape is outside the fused kernel's contract (the caller then runs the two separate launches).
    norm = (ss, rstd, eps): x2d is x * g of a folded RMSNorm (mla_gemm_qkv_rope_rs: fused RMSNorm + QKV + RoPE); returns rstd [T]."""
    T, K = x2d.shape
    N = wqkv.shape[0]
    ok = qkv_rope_ok(x2d, wqkv, out, cos, sin, S, rope_cols)
    if not ok:
        return False
    if norm is not None:
        _req(x2d, torch.bfloat16, "gemm_qkv_rope x")
        _req(wqkv, torch.bfloat16, "gemm_qkv_rope w")
        ss, parts, eps, rstd = _rs_args(norm, T, x2d.device)
        prof = GEMM_PROFILE
        if prof is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        call("mla_gemm_qkv_rope_rs", _p(x2d), _p(wqkv), _p(out), T, N, K, x2d.stride(0), wqkv.stride(0), out.stride(0), _p(cos), _p(sin),
             int(S), int(rope_cols), _p(ss), parts, eps, _p(rstd))
        if prof is not None:
            ev1.record()
            prof.append((ev0, ev1, 2.0 * T * N * K, (0, 0, T, N, K, "rope_epilogue")))
        return rstd
    _req(x2d, torch.bfloat16, "gemm_qkv_rope x")
    _req(wqkv, torch.bfloat16, "gemm_qkv_rope w")
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    call("mla_gemm_qkv_rope", _p(x2d), _p(wqkv), _p(out), T, N, K, x2d.stride(0), wqkv.stride(0), out.stride(0), _p(cos), _p(sin),
         int(S), int(rope_cols))
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * T * N * K, (0, 0, T, N, K, "rope_epilogue")))
    return True


def gateup_swiglu_ok(x2d, wgu, want_t) -> bool:
    T, K = x2d.shape
    I = wgu.shape[0] // 2
    return (T >= 256 and I % 128 == 0 and K % 64 == 0 and wgu.shape[0] == 2 * I and x2d.stride(0) % 8 == 0 and wgu.stride(0) % 8 == 0 and
            (not want_t or T % 8 == 0) and all(t.data_ptr() % 16 == 0 for t in (x2d, wgu)))


def gemm_gateup_swiglu(x2d, wgu, want_t, norm=None, want_act=True, want_gu=True):
    """(gu [T, 2I], act [T, I], actT [I, T] or None) from ONE launch: the SwiGLU product is formed in the gate|up GEMM's epilogue.
    None when the shape is outside the fused kernel's contract (the caller then runs gemm + swiglu_fwd[_dual]).
    norm = (ss, rstd, eps): x2d is x * g of a folded RMSNorm (mla_gemm_gateup_swiglu_rs); rstd [T] is appended to the result."""
    T, K = x2d.shape
    I = wgu.shape[0] // 2
    ok = gateup_swiglu_ok(x2d, wgu, want_t)
    if not ok:
        return None
    _req(x2d, torch.bfloat16, "gemm_gateup_swiglu x")
    _req(wgu, torch.bfloat16, "gemm_gateup_swiglu w")
    act = torch.empty((T, I), dtype=torch.bfloat16, device=x2d.device) if (want_act or not want_t) else None   # want_act=False: act^T only
    gu = torch.empty((T, 2 * I), dtype=torch.bfloat16, device=x2d.device) if (want_gu or act is None) else None  # want_gu=False: the product only
    actT = torch.empty((I, T), dtype=torch.bfloat16, device=x2d.device) if want_t else None
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    rstd = None
    if norm is not None:
        ss, parts, eps, rstd = _rs_args(norm, T, x2d.device)
        call("mla_gemm_gateup_swiglu_rs", _p(x2d), _p(wgu), _p(gu), _p(act), _p(actT), T, I, K, x2d.stride(0), wgu.stride(0), T,
             _p(ss), parts, eps, _p(rstd))
    else:
        call("mla_gemm_gateup_swiglu", _p(x2d), _p(wgu), _p(gu), _p(act), _p(actT), T, I, K, x2d.stride(0), wgu.stride(0), T)
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * T * 2 * I * K, (0, 0, T, 2 * I, K, "swiglu_fwd_epilogue")))
    return (gu, act, actT) if norm is None else (gu, act, actT, rstd)


def gemm_dact_swiglu_bwd(dy2d, wT, gu2d, want_t=True):
    """(dgu [T, 2I], dguT [2I, T]) = SwiGLU backward of d(act) = dy2d @ wT^T without ever writing d(act); None when the shape is outside
    the fused kernel's contract (the caller then runs gemm + swiglu_bwd_t). want_t=False: dguT is None and never produced."""
    T, K = dy2d.shape
    I = wT.shape[0]
    ok = (T >= 256 and I >= 256 and K % 64 == 0 and I % 8 == 0 and T % 8 == 0 and gu2d.shape == (T, 2 * I) and gu2d.is_contiguous() and
          dy2d.stride(0) % 8 == 0 and wT.stride(0) % 8 == 0 and all(t.data_ptr() % 16 == 0 for t in (dy2d, wT, gu2d)))
    if not ok:
        return None
    _req(dy2d, torch.bfloat16, "gemm_dact_swiglu_bwd dy")
    _req(wT, torch.bfloat16, "gemm_dact_swiglu_bwd wT")
    dgu = torch.empty_like(gu2d)
    dguT = torch.empty((2 * I, T), dtype=torch.bfloat16, device=gu2d.device) if want_t else None
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    call("mla_gemm_dact_swiglu_bwd", _p(dy2d), _p(wT), _p(gu2d), _p(dgu), _p(dguT), T, I, K, dy2d.stride(0), wT.stride(0), T)
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * T * I * K, (0, 0, T, I, K, "swiglu_bwd_epilogue")))
    return dgu, dguT


def dact_swiglu_bwd_rm_ok(dy2d, w, gu2d) -> bool:
    """Whether gemm_dact_swiglu_bwd_rm serves these operands (the caller's dispatch; the library checks the same contract itself)."""
    T, K = dy2d.shape
    I = w.shape[1]
    return (T >= 256 and I >= 256 and K % 64 == 0 and I % 8 == 0 and T % 8 == 0 and w.shape[0] == K and w.stride(1) == 1 and
            gu2d.shape == (T, 2 * I) and gu2d.is_contiguous() and dy2d.stride(1) == 1 and dy2d.stride(0) % 8 == 0 and
            w.stride(0) % 8 == 0 and all(t.data_ptr() % 16 == 0 for t in (dy2d, w, gu2d)))


def gemm_dact_swiglu_bwd_rm(dy2d, w, gu2d, want_t=True, dgu=None, dguT=None):
    """gemm_dact_swiglu_bwd on the down-projection weight AS STORED, w [K, I] (a row-strided view is fine): d(act) = dy2d @ w without a
    W^T copy; the bits of gemm_dact_swiglu_bwd(dy2d, transpose(w), ...). No shape filter here: what the kernel does not serve is an
    error from the library. dgu / dguT: optional output buffers ([T, 2I] / [2I, T] contiguous)."""
    T, K = dy2d.shape
    I = w.shape[1]
    for t, nm in ((dy2d, "dy"), (w, "w"), (gu2d, "gu")):
        _req(t, torch.bfloat16, "gemm_dact_swiglu_bwd_rm " + nm)
    if w.shape[0] != K or w.stride(1) != 1 or dy2d.stride(1) != 1 or gu2d.shape != (T, 2 * I) or not gu2d.is_contiguous():
        raise ValueError("gemm_dact_swiglu_bwd_rm: needs dy [T, K], w [K, I] (unit column stride), gu [T, 2I] contiguous")
    if dgu is None:
        dgu = torch.empty_like(gu2d)
    if dguT is None and want_t:
        dguT = torch.empty((2 * I, T), dtype=torch.bfloat16, device=gu2d.device)
    if not want_t:
        dguT = None
    for t, shp, nm in ((dgu, (T, 2 * I), "dgu"), (dguT, (2 * I, T), "dguT")):
        if t is not None and (t.shape != shp or not t.is_contiguous() or t.dtype != torch.bfloat16):
            raise ValueError(f"gemm_dact_swiglu_bwd_rm: {nm} must be a contiguous bf16 {shp}")
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    call("mla_gemm_dact_swiglu_bwd_rm", _p(dy2d), _p(w), _p(gu2d), _p(dgu), _p(dguT), T, I, K, dy2d.stride(0), w.stride(0), T)
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * T * I * K, (0, 1, T, I, K, "swiglu_bwd_epilogue")))
    return dgu, dguT


# --------------------------------------------------------------------------------------------- norms
def rmsnorm_fwd(x2d, w, eps):
    _req(x2d, torch.bfloat16, "rmsnorm x")
    _req(w, torch.bfloat16, "rmsnorm w")
    rows, H = x2d.shape
    y = torch.empty_like(x2d)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    call("mla_rmsnorm_fwd", _p(x2d), _p(w), _p(y), _p(rstd), rows, H, float(eps))
    return y, rstd


def rmsnorm_prep(x2d, w, eps, want_rstd=True):
    """(xg = bf16(x * w), rstd [rows] or None): the two halves of a folded RMSNorm for rows that do not come out of a GEMM epilogue."""
    _req(x2d, torch.bfloat16, "rmsnorm_prep x")
    _req(w, torch.bfloat16, "rmsnorm_prep w")
    rows, H = x2d.shape
    xg = torch.empty_like(x2d)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device) if want_rstd else None
    call("mla_rmsnorm_prep", _p(x2d), _p(w), _p(xg), _p(rstd), rows, H, float(eps))
    return xg, rstd


def res_norm_ok(a, b, residual) -> bool:
    M, K = a.shape
    N = b.shape[0]
    return (M >= 256 and N >= 256 and N % 256 == 0 and K % 64 == 0 and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0 and
            residual.stride(0) % 8 == 0 and a.stride(1) == 1 and b.stride(1) == 1 and residual.stride(1) == 1 and
            all(t.data_ptr() % 16 == 0 for t in (a, b, residual)))


def gemm_res_norm(a, b, residual, g):
    """(h, xg, ss): h = a @ b^T + residual (the new residual-stream rows), xg = bf16(h * g) and ss [M, N / 256] = per-tile partials of
    sum(h^2) per row -- the producer half of a folded RMSNorm (mla_gemm_res_norm), one GEMM launch."""
    _req(a, torch.bfloat16, "gemm_res_norm a")
    _req(b, torch.bfloat16, "gemm_res_norm b")
    _req(residual, torch.bfloat16, "gemm_res_norm residual")
    _req(g, torch.bfloat16, "gemm_res_norm g")
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and residual.shape == (M, N) and g.numel() == N and g.data_ptr() % 16 == 0
    h = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    xg = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    ss = torch.empty((M, N // 256), dtype=torch.float32, device=a.device)
    ws = workspace(SPLITK_WS_BYTES, a.device) if SPLITK else None
    prof = GEMM_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    call("mla_gemm_res_norm", _p(a), _p(b), _p(h), _p(residual), _p(g), _p(xg), _p(ss), M, N, K, a.stride(0), b.stride(0), N,
         residual.stride(0), _p(ws), SPLITK_WS_BYTES if ws is not None else 0)
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * M * N * K, (0, 0, M, N, K)))
    return h, xg, ss


def rmsnorm_bwd(dy, x2d, w, rstd, dres=None, dw_out=None, dw_accumulate=False):
    rows, H = x2d.shape
    dx = torch.empty_like(x2d)
    nb = lib().mla_rmsnorm_bwd_blocks(rows)
    ws = workspace(nb * H * 4, x2d.device) if dw_out is not None else None
    call("mla_rmsnorm_bwd", _p(dy), _p(x2d), _p(w), _p(rstd), _p(dres), _p(dx), _p(dw_out), 1 if dw_accumulate else 0, rows, H,
         _p(ws), ws.numel() if ws is not None else 0)
    return dx


def timm_rmsnorm_fwd(x2d, w, eps):
    """timm==0.9.10 RmsNorm (torch.var based, see include/mla_hip.h). Returns (y, mean, rstd)."""
    _req(x2d, torch.bfloat16, "timm_rmsnorm x")
    _req(w, torch.bfloat16, "timm_rmsnorm w")
    rows, H = x2d.shape
    y = torch.empty_like(x2d)
    stats = torch.empty(2, rows, dtype=torch.float32, device=x2d.device)
    call("mla_timm_rmsnorm_fwd", _p(x2d), _p(w), _p(y), _p(stats[0]), _p(stats[1]), rows, H, float(eps))
    return y, stats[0], stats[1]


def timm_rmsnorm_bwd(dy, x2d, w, mean, rstd, dw_out=None, dw_accumulate=False):
    rows, H = x2d.shape
    dx = torch.empty_like(x2d)
    nb = lib().mla_rmsnorm_bwd_blocks(rows)
    ws = workspace(nb * H * 4, x2d.device) if dw_out is not None else None
    call("mla_timm_rmsnorm_bwd", _p(dy), _p(x2d), _p(w), _p(mean), _p(rstd), _p(dx), _p(dw_out), 1 if dw_accumulate else 0, rows, H,
         _p(ws), ws.numel() if ws is not None else 0)
    return dx


def colsum(dy2d, out_f32, accumulate):
    rows, N = dy2d.shape
    rs = lib().mla_colsum_blocks(rows)
    ws = workspace(rs * N * 4, dy2d.device)
    call("mla_colsum_bf16", _p(dy2d), _p(out_f32), 1 if accumulate else 0, rows, N, dy2d.stride(0), _p(ws), ws.numel())


def layernorm_fwd(x2d, w, b, eps):
    rows, H = x2d.shape
    y = torch.empty_like(x2d)
    call("mla_layernorm_fwd", _p(x2d), _p(w), _p(b), _p(y), rows, H, float(eps))
    return y


def rope_inplace(buf2d, cos, sin, S, nheads, D, q_off, k_off, backward=False):
    tokens = buf2d.shape[0]
    call("mla_rope_inplace", _p(buf2d), _p(cos), _p(sin), tokens, S, nheads, D, buf2d.stride(0), q_off, k_off,
         1 if backward else 0)


def swiglu_fwd(gu2d):
    rows, two_i = gu2d.shape
    act = torch.empty((rows, two_i // 2), dtype=torch.bfloat16, device=gu2d.device)
    call("mla_swiglu_fwd", _p(gu2d), _p(act), rows, two_i // 2)
    return act


def swiglu_bwd(dact, gu2d, want_act=False):
    rows, two_i = gu2d.shape
    dgu = torch.empty_like(gu2d)
    act = torch.empty_like(dact) if want_act else None
    call("mla_swiglu_bwd", _p(dact), _p(gu2d), _p(dgu), _p(act), rows, two_i // 2)
    return dgu, act


def swiglu_bwd_t(dact, gu2d):
    """dgu [rows, 2I] and its transpose [2I, rows] from one pass over dact and gu."""
    rows, two_i = gu2d.shape
    dgu = torch.empty_like(gu2d)
    dguT = torch.empty((two_i, rows), dtype=gu2d.dtype, device=gu2d.device)
    call("mla_swiglu_bwd_t", _p(dact), _p(gu2d), _p(dgu), _p(dguT), rows, two_i // 2, rows)
    return dgu, dguT


def act_fwd(x, kind):
    y = torch.empty_like(x)
    call("mla_act_fwd", _p(x), _p(y), x.numel(), kind)
    return y


def act_bwd(dy, x, kind):
    dx = torch.empty_like(x)
    call("mla_act_bwd", _p(dy), _p(x), _p(dx), x.numel(), kind)
    return dx


def cast_f32_to_bf16(x, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call("mla_cast_f32_to_bf16", _p(x), _p(out), x.numel())
    return out


def cast_bf16_to_f32(x, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("mla_cast_bf16_to_f32", _p(x), _p(out), x.numel())
    return out


def add_bf16(a, b):
    y = torch.empty_like(a)
    call("mla_add_bf16", _p(a), _p(b), _p(y), a.numel())
    return y


def embedding_fwd(ids, table):
    tokens = ids.numel()
    vocab, H = table.shape
    out = torch.empty((tokens, H), dtype=torch.bfloat16, device=table.device)
    call("mla_embedding_fwd", _p(ids), _p(table), _p(out), tokens, H, vocab)
    return out


def embedding_bwd(ids, dy2d, grad_f32):
    """grad_f32[ids[t]] += dy2d[t], deterministic (ascending token order; an aligned batch of 64 equal ids -- padding -- is summed
    first into the workspace row the library asks for)."""
    vocab, H = grad_f32.shape
    tokens = ids.numel()
    ws = torch.empty((tokens // 64, H), dtype=torch.float32, device=grad_f32.device) if tokens >= 64 else None
    call("mla_embedding_bwd", _p(ids), _p(dy2d), _p(grad_f32), _p(ws), tokens, H, vocab)


def adamw_step(p32, g32, m, v, p16, lr, beta1, beta2, eps, wd, step, grad_scale=None):
    call("mla_adamw_step", _p(p32), _p(g32), _p(m), _p(v), _p(p16), p32.numel(), float(lr), float(beta1), float(beta2),
         float(eps), float(wd), int(step), _p(grad_scale))


def adamw_step_groups(p32, g32, m, v, p16, n_decay, lr, beta1, beta2, eps, wd, step, grad_scale=None):
    """adamw_step over a flat range laid out [decayed | not decayed]: weight decay on the first n_decay elements only."""
    call("mla_adamw_step_groups", _p(p32), _p(g32), _p(m), _p(v), _p(p16), p32.numel(), int(n_decay), float(lr), float(beta1), float(beta2),
         float(eps), float(wd), int(step), _p(grad_scale))


def ema_factors(decay):
    """(decay, 1 - decay) as the library takes them: decay cast to fp32, 1 - decay formed in double and cast once (the convention of
    the bias corrections, include/mla_hip.h). ctypes rounds a Python float to fp32 the same way."""
    d = float(decay)
    if not 0.0 <= d <= 1.0:
        raise ValueError(f"ema decay must lie in [0, 1], got {decay}")
    return d, 1.0 - d


def adamw_ema_step(p32, g32, m, v, ema, p16, lr, beta1, beta2, eps, wd, step, grad_scale, ema_decay):
    """adamw_step that also advances the weight average: ema = (1 - ema_decay) * p_new + ema_decay * ema on the fp32 master."""
    _req(ema, torch.float32, "adamw_ema_step ema")
    assert ema.numel() == p32.numel() and ema.is_contiguous()
    d, omd = ema_factors(ema_decay)
    call("mla_adamw_ema_step", _p(p32), _p(g32), _p(m), _p(v), _p(ema), _p(p16), p32.numel(), float(lr), float(beta1), float(beta2),
         float(eps), float(wd), int(step), _p(grad_scale), d, omd)


def adamw_ema_step_groups(p32, g32, m, v, ema, p16, n_decay, lr, beta1, beta2, eps, wd, step, grad_scale, ema_decay):
    """adamw_step_groups that also advances the weight average (see adamw_ema_step)."""
    _req(ema, torch.float32, "adamw_ema_step_groups ema")
    assert ema.numel() == p32.numel() and ema.is_contiguous()
    d, omd = ema_factors(ema_decay)
    call("mla_adamw_ema_step_groups", _p(p32), _p(g32), _p(m), _p(v), _p(ema), _p(p16), p32.numel(), int(n_decay), float(lr), float(beta1),
         float(beta2), float(eps), float(wd), int(step), _p(grad_scale), d, omd)


def adamw_m16_step(p32, g32, m16, v16, ema, p16, n_decay, lr, beta1, beta2, eps, wd, step, grad_scale, ema_decay, seed, index_base):
    """adamw_step_groups with both moments stored as bf16 and rounded stochastically (mla_adamw_m16_step, include/mla_hip_optim.h);
    ema: the fp32 weight average advanced in the same launch, or None (ema_decay is then ignored). The random bits are a function
    of (seed, step, index_base + i): index_base is the global index of element 0, so consecutive launches continue one stream."""
    _req(p32, torch.float32, "adamw_m16_step p32")
    _req(g32, torch.float32, "adamw_m16_step g32")
    _req(m16, torch.bfloat16, "adamw_m16_step m16")
    _req(v16, torch.bfloat16, "adamw_m16_step v16")
    n = p32.numel()
    assert g32.numel() == n and m16.numel() == n and v16.numel() == n and all(t.is_contiguous() for t in (p32, g32, m16, v16))
    d, omd = 0.0, 0.0
    if ema is not None:
        _req(ema, torch.float32, "adamw_m16_step ema")
        assert ema.numel() == n and ema.is_contiguous()
        d, omd = ema_factors(ema_decay)
    if p16 is not None:
        _req(p16, torch.bfloat16, "adamw_m16_step p16")
        assert p16.numel() == n and p16.is_contiguous()
    call("mla_adamw_m16_step", _p(p32), _p(g32), _p(m16), _p(v16), _p(ema), _p(p16), n, int(n_decay), float(lr), float(beta1),
         float(beta2), float(eps), float(wd), int(step), _p(grad_scale), d, omd, int(seed) & 0xFFFFFFFFFFFFFFFF, int(index_base))


def adamw_guard_step(p32, g32, m, v, ema, p16, n_decay, lr, beta1, beta2, eps, wd, step, grad_scale, ema_decay, seed, index_base, skip1):
    """Every form of the AdamW pass behind the device flag skip1 of clip_coef_guard (mla_adamw_guard_step, include/mla_hip_optim.h):
    skip1[0] != 0 and the launch touches nothing; skip1[0] == 0 and it writes the bits of adamw_step_groups / adamw_ema_step_groups (m, v
    fp32; seed and index_base unused) or of adamw_m16_step (m, v bf16). ema: the fp32 weight average, or None."""
    _req(p32, torch.float32, "adamw_guard_step p32")
    _req(g32, torch.float32, "adamw_guard_step g32")
    _req(skip1, torch.int32, "adamw_guard_step skip1")
    if m.dtype not in (torch.float32, torch.bfloat16) or v.dtype != m.dtype:
        raise TypeError(f"adamw_guard_step: moments must both be fp32 or both bf16, got {m.dtype} and {v.dtype}")
    n = p32.numel()
    assert g32.numel() == n and m.numel() == n and v.numel() == n and all(t.is_contiguous() for t in (p32, g32, m, v))
    d, omd = 0.0, 0.0
    if ema is not None:
        _req(ema, torch.float32, "adamw_guard_step ema")
        assert ema.numel() == n and ema.is_contiguous()
        d, omd = ema_factors(ema_decay)
    if p16 is not None:
        _req(p16, torch.bfloat16, "adamw_guard_step p16")
        assert p16.numel() == n and p16.is_contiguous()
    call("mla_adamw_guard_step", _p(p32), _p(g32), _p(m), _p(v), _p(ema), _p(p16), n, int(n_decay), float(lr), float(beta1), float(beta2),
         float(eps), float(wd), int(step), _p(grad_scale), d, omd, int(m.dtype == torch.bfloat16), int(seed) & 0xFFFFFFFFFFFFFFFF,
         int(index_base), _p(skip1))


def ema_update(ema, p32, decay):
    """ema = (1 - decay) * p32 + decay * ema, fp32, in place: the weight average as a pass of its own."""
    _req(ema, torch.float32, "ema_update ema")
    _req(p32, torch.float32, "ema_update p32")
    assert ema.numel() == p32.numel() and ema.is_contiguous() and p32.is_contiguous()
    d, omd = ema_factors(decay)
    call("mla_ema_update", _p(ema), _p(p32), p32.numel(), d, omd)


def sumsq(x32, out1, accumulate):
    ws = workspace(8192, x32.device)
    call("mla_sumsq_f32", _p(x32), x32.numel(), _p(out1), 1 if accumulate else 0, _p(ws), ws.numel())


def clip_coef(sumsq1, max_norm, coef1, norm1=None):
    call("mla_clip_coef", _p(sumsq1), float(max_norm), _p(coef1), _p(norm1))


def clip_coef_guard(sumsq1, max_norm, coef1, norm1, skip1):
    """clip_coef plus the verdict of the skip_nonfinite guard (mla_clip_coef_guard, include/mla_hip_optim.h): skip1, one int32 on the
    device, becomes 1 when sumsq1 is +inf or NaN (coef1 = 0, norm1 = the non-finite norm) and 0 otherwise (coef1, norm1 as clip_coef)."""
    _req(skip1, torch.int32, "clip_coef_guard skip1")
    call("mla_clip_coef_guard", _p(sumsq1), float(max_norm), _p(coef1), _p(norm1), _p(skip1))


def q_sample(x0, noise, t, sqrt_ac, sqrt_1mac):
    out = torch.empty_like(x0)
    batch = x0.shape[0]
    call("mla_q_sample", _p(x0), _p(noise), _p(t), _p(sqrt_ac), _p(sqrt_1mac), _p(out), batch, x0.numel() // batch,
         sqrt_ac.numel())
    return out


# --------------------------------------------------------------------------------------------- attention
def _group_args(groups, B):
    """groups = (start, len): start an int (every sample) or an int32 device tensor [B] (per sample) -> (scalar start, tensor or None)"""
    start = groups[0]
    if torch.is_tensor(start):
        _req(start, torch.int32, "attention group starts")
        assert start.numel() == B and start.is_contiguous()
        return 0, start
    return int(start), None


def attn_fwd(q, k, v, B, S, H, D, ld_qkv, seqlens, scale, rows=None, groups=None):
    """q/k/v: views into the packed [B*S, 3*H*D] buffer (first element of each slice). rows > B*S: the output gets that many rows,
    the extra ones zero (row padding of the caller, ops.DecoderLayerFn). groups = (start, len): shared-prefix sequences -- rows >= start
    are suffix groups of `len` rows, a query sees the prefix and (causally) its own group only (mla_attn_fwd_g)."""
    rows = B * S if rows is None else rows
    o = torch.empty((rows, H * D), dtype=torch.bfloat16, device=q.device)
    if rows > B * S:
        o[B * S:].zero_()
    lse = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    if groups is not None:
        gs, gst = _group_args(groups, B)
        call("mla_attn_fwd_g", _p(q), _p(k), _p(v), _p(o), _p(lse), _p(seqlens), B, S, H, D, ld_qkv, H * D, float(scale), gs, int(groups[1]), _p(gst))
    else:
        call("mla_attn_fwd", _p(q), _p(k), _p(v), _p(o), _p(lse), _p(seqlens), B, S, H, D, ld_qkv, H * D, float(scale))
    return o, lse


# The five-product backward is OPT-IN (MLA_ATTN_BWD5=1): measured on MI355X it is not faster than the two-kernel, seven-product form
# (S = 548: delta 81 + dK/dV 438 + dQ 262 us vs 419 + 352; S = 2048: 189 + 3420 + 1681 vs 3039 + 2218) -- MFMA work is cheap here
# and the one-product dQ kernel is bound by streaming dS^T and re-streaming K through LDS.
ATTN_BWD5 = os.environ.get("MLA_ATTN_BWD5", "0") == "1"


# ---- one-launch backward: the head counters are OURS (the library keeps nothing), one zero-initialised int32 buffer per (device, stream),
# handed over only on a device where the dispatch probe holds (mla_hip.h: mla_attn_bwd, mla_dispatch_probe).
_HEAD_SYNC = {}          # (device index, stream handle) -> int32 tensor; the kernel leaves it zero after every launch
_DISPATCH_OK = {}        # device index -> (bool, dict): result of dispatch_probe()
ATTN_BWD_MERGED = os.environ.get("MLA_ATTN_BWD_MERGED", "105") != "0"


def dispatch_probe(device="cuda", blocks=4096, hold_us=20):
    """Measures what attn_bwd_merged_kernel assumes (include/mla_hip.h: mla_dispatch_probe). Returns (ok, info): ok iff there are 8
    XCDs, workgroup L ran on XCD L & 7 for every L, and per XCD no workgroup took its start ticket more than two residency rounds (2 x 64
    slots: 32 CUs x 2 workgroups) away from its place in id order -- the workgroups of one round start together and take their tickets
    in any order (measured on MI355X: worst displacement 52-56), an out-of-order dispatcher would show displacements of the grid's
    size. Synchronises -- called once per device, outside any capture."""
    dev = torch.device(device)
    out = torch.zeros(1 + 2 * blocks, dtype=torch.int32, device=dev)
    call("mla_dispatch_probe", _p(out), blocks, hold_us)
    rec = out.cpu()[1:].view(blocks, 2)
    ticket, xcc = rec[:, 0].long(), rec[:, 1].long()
    ids = torch.arange(blocks)
    n_xcd = int(xcc.unique().numel())
    xcd_ok = bool((xcc == (ids & 7)).all())
    worst = 0
    for x in range(8):
        t = ticket[ids % 8 == x]                       # start tickets of the workgroups with id = x mod 8, in id order
        rank = torch.argsort(torch.argsort(t))          # place of each in start order
        worst = max(worst, int((rank - torch.arange(t.numel())).abs().max()))
    info = {"xcds": n_xcd, "xcc_is_id_mod_8": xcd_ok, "worst_start_displacement": worst, "blocks": blocks,
            "tickets_complete": bool(torch.equal(torch.sort(ticket).values, ids))}
    return (n_xcd == 8 and xcd_ok and worst <= 128 and info["tickets_complete"]), info


def _head_sync(device, B, H):
    """The caller-owned counter pair per head for the one-launch backward, or None (= two launches)."""
    if not ATTN_BWD_MERGED:
        return None
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _DISPATCH_OK:
        if torch.cuda.is_current_stream_capturing():
            return None                                  # first use inside a capture: the probe synchronises -- stay on two launches
        with torch.cuda.device(idx):
            _DISPATCH_OK[idx] = dispatch_probe(torch.device("cuda", idx))
    if not _DISPATCH_OK[idx][0]:
        return None
    need = int(lib().mla_attn_bwd_sync_ints(B, H))
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    buf = _HEAD_SYNC.get(key)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            return None
        # (an outgrown buffer may still be read by queued launches: torch's stream-ordered allocator does not hand its memory to
        # anything that could run before them)
        buf = torch.zeros(max(need, 4096), dtype=torch.int32, device=torch.device("cuda", idx))
        _HEAD_SYNC[key] = buf
    return buf


def attn_bwd(q, k, v, o, dout, lse, seqlens, dq, dk, dv, B, S, H, D, ld_qkv, scale, rope_cos=None, rope_sin=None, transposed=None,
             five: Optional[bool] = None, merged: Optional[bool] = None, groups=None):
    """five (experiment build only, see ATTN_BWD5): the five-product form -- the dK / dV kernel hands dS^T (bf16 tiles in a torch-owned
    scratch buffer) to a one-product dQ kernel instead of both kernels recomputing Q K^T and dO V^T (mla_attn_bwd_ws).
    merged (default: on where the dispatch probe holds; MLA_ATTN_BWD_MERGED=0 turns it off): one launch for the dQ and dK / dV blocks
    with this module's per-stream head counters; False = two launches. Bit-identical either way.
    rope_cos / rope_sin ([S, D/2] fp32): dq / dk come out with the RoPE backward already applied (no separate pass).
    transposed = (dqkvT [3*H*D, ldt], oT [H*D, ldt]) bf16: also filled with the token-contiguous copies of dq|dk|dv and o (columns
    b*S + s; columns >= B*S are left alone) -- the wgrad operands, without transpose passes. Needs S % 4 == 0, ldt % 4 == 0."""
    delta = torch.empty((B, H, S), dtype=torch.float32, device=q.device)
    five = ATTN_BWD5 if five is None else five
    if rope_cos is not None:
        _req(rope_cos, torch.float32, "rope cos")
        _req(rope_sin, torch.float32, "rope sin")
        assert rope_cos.shape in ((S, D // 2), (B * S, D // 2)) and rope_sin.shape == rope_cos.shape and rope_cos.is_contiguous() and rope_sin.is_contiguous()
        assert rope_cos.shape[0] == S or groups is not None, "per-sample RoPE tables [B * S, 64] go with mla_attn_bwd_g (groups=...)"
    if transposed is not None:
        dqkvT, oT = transposed
        _req(dqkvT, torch.bfloat16, "dqkvT")
        _req(oT, torch.bfloat16, "oT")
        ldt = dqkvT.stride(0)
        assert dqkvT.shape[0] == 3 * H * D and oT.shape[0] == H * D and oT.stride(0) == ldt and dqkvT.stride(1) == 1 and oT.stride(1) == 1
    if five:
        nbytes = int(lib().mla_attn_bwd_ws_bytes(B, S, H))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)           # transient: freed (to torch's pool) after the launches are queued
        if transposed is not None:
            tq, tk, tv, to_ = dqkvT[:H * D], dqkvT[H * D:2 * H * D], dqkvT[2 * H * D:], oT
        else:
            tq = tk = tv = to_ = None
            ldt = 0
        call("mla_attn_bwd_ws", _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(seqlens), _p(dq), _p(dk), _p(dv), _p(delta), B, S,
             H, D, ld_qkv, H * D, float(scale), _p(rope_cos), _p(rope_sin), _p(tq), _p(tk), _p(tv), _p(to_), ldt, _p(ws), nbytes)
        return
    sync = _head_sync(q.device, B, H) if merged is None or merged else None
    if merged and sync is None:
        raise RuntimeError("attn_bwd(merged=True): the one-launch backward is not available here "
                           f"(MLA_ATTN_BWD_MERGED=0, a stream capture before the first use, or the dispatch probe failed: {_DISPATCH_OK})")
    n_sync = sync.numel() if sync is not None else 0
    if groups is not None:                               # shared-prefix sequences (mla_attn_bwd_g; see attn_fwd)
        tq = tk = tv = to_ = None
        if transposed is not None:
            tq, tk, tv, to_ = dqkvT[:H * D], dqkvT[H * D:2 * H * D], dqkvT[2 * H * D:], oT
        gs, gst = _group_args(groups, B)
        call("mla_attn_bwd_g", _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(seqlens), _p(dq), _p(dk), _p(dv), _p(delta), B, S,
             H, D, ld_qkv, H * D, float(scale), _p(rope_cos), _p(rope_sin), _p(tq), _p(tk), _p(tv), _p(to_), ldt if transposed is not None else 0,
             _p(sync), n_sync, gs, int(groups[1]), _p(gst), 1 if (rope_cos is not None and rope_cos.shape[0] == B * S and B > 1) else 0)
        return
    if transposed is not None:
        call("mla_attn_bwd_t", _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(seqlens), _p(dq), _p(dk), _p(dv), _p(delta), B, S,
             H, D, ld_qkv, H * D, float(scale), _p(rope_cos), _p(rope_sin), _p(dqkvT[:H * D]), _p(dqkvT[H * D:2 * H * D]),
             _p(dqkvT[2 * H * D:]), _p(oT), ldt, _p(sync), n_sync)
        return
    call("mla_attn_bwd", _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(seqlens), _p(dq), _p(dk), _p(dv), _p(delta), B, S,
         H, D, ld_qkv, H * D, float(scale), _p(rope_cos), _p(rope_sin), _p(sync), n_sync)


# --------------------------------------------------------------------------------------------- inference (mla_amd/infer.py)
class WeightFormat(NamedTuple):
    """How the suffix projections (PROJ_FAMILIES) read a weight W [N, K] and its scale: a row of WEIGHT_FORMATS."""
    name: str                            # mla_<family>_<name>[_pos] in the library, hip.<family>_<name> here (bf16: hip.<family>)
    dtype: torch.dtype                   # of W
    k_per_col: int                       # elements of K per stored column of W (2: MXFP4 code pairs, W [N, K / 2])
    scale_dtype: Optional[torch.dtype]   # of w_scale; None: no scale argument
    scale_block: int                     # K per scale: w_scale [N, K / scale_block], its row stride passed on; 0: one per row, [N] contiguous
    k_gran: int                          # K granularity of the launchers

    @property
    def suffix(self) -> str:
        return "" if self.scale_dtype is None else "_" + self.name


# bf16 as stored; w8: e4m3fn codes and one fp32 scale per row (quant_fp8_rows); w4: MXFP4 code pairs and e8m0 block scales (quant_mxfp4_rows)
WEIGHT_FORMATS = {f.name: f for f in (WeightFormat("bf16", torch.bfloat16, 1, None, 0, 8),
                                      WeightFormat("w8", torch.float8_e4m3fn, 1, torch.float32, 0, 16),
                                      WeightFormat("w4", torch.uint8, 2, torch.uint8, 32, 32))}
_WF_BF16, _WF_W8, _WF_W4 = WEIGHT_FORMATS.values()
PROJ_FAMILIES = ("gemv", "gemm_skinny", "gemm_skinny_gateup_swiglu", "gemm_suffix")   # hip.<family><suffix> calls mla_<family>_<name>


def _scale_args(fmt, N: int, K: int, scale):
    """The scale of an [N, K] matrix against the row's shape rule (a K off a bf16 / w8 granularity is the launchers' refusal) -> its call arguments."""
    if fmt.scale_block:
        assert K % fmt.k_gran == 0 and scale.shape == (N, K // fmt.scale_block) and scale.stride(1) == 1, f"K % {fmt.k_gran} == 0 required"
        return _p(scale), scale.stride(0)
    assert scale.numel() == N and scale.is_contiguous()
    return (_p(scale),)


def _quant_rows(fmt, name, W, q, scale, scale_name):
    """The quantisers' shared body (mla_<name>): W [N, K] bf16, rows may be strided -> (q, scale) of the row's dtypes and shapes, allocated where not given."""
    _req(W, torch.bfloat16, f"{name} W")
    N, K = W.shape
    if q is None:
        q = torch.empty((N, K // fmt.k_per_col), dtype=fmt.dtype, device=W.device)
    if scale is None:
        scale = torch.empty((N, K // fmt.scale_block) if fmt.scale_block else N, dtype=fmt.scale_dtype, device=W.device)
    _req(q, fmt.dtype, f"{name} q")
    _req(scale, fmt.scale_dtype, f"{name} {scale_name}")
    assert W.stride(1) == 1 and q.shape == (N, K // fmt.k_per_col) and q.stride(1) == 1
    call("mla_" + name, _p(W), W.stride(0), _p(q), q.stride(0), *_scale_args(fmt, N, K, scale), N, K)
    return q, scale


def _proj_operands(fmt, name, x, W, w_scale, out=None):
    """The operand checks every suffix projection call opens with, against the format's row: x and out (where given) bf16, W and w_scale
    of the row's dtypes, the scale of the row's shape, unit inner strides -> (K, the scale arguments of the call: () for bf16 weights)."""
    _req(x, torch.bfloat16, f"{name} x")
    _req(W, fmt.dtype, f"{name} W")
    K, scale_arg = W.shape[1] * fmt.k_per_col, ()
    if fmt.scale_dtype is not None:
        _req(w_scale, fmt.scale_dtype, f"{name} w_scale")
        scale_arg = _scale_args(fmt, W.shape[0], K, w_scale)
    if out is not None:
        _req(out, torch.bfloat16, f"{name} out")
    assert x.stride(1) == 1 and W.stride(1) == 1
    return K, scale_arg


def _proj_epilogue(name, M, residual, out_col, rope, rope_rows):
    """The residual and rotary-epilogue checks of the suffix projections -> (residual arguments, rope arguments) of the call. rope =
    (cos [rope_rows, 64], sin, rope_cols) goes with neither a residual nor a column offset."""
    res_arg, rope_arg = (None, 0), (None, None, 0)
    if rope is not None:
        _req(rope[0], torch.float32, f"{name} rope cos")
        _req(rope[1], torch.float32, f"{name} rope sin")
        assert rope[0].shape == (rope_rows, 64) and rope[1].shape == rope[0].shape and rope[0].is_contiguous() and rope[1].is_contiguous()
        assert out_col == 0 and residual is None
        rope_arg = (_p(rope[0]), _p(rope[1]), int(rope[2]))
    if residual is not None:
        _req(residual, torch.bfloat16, f"{name} residual")
        assert residual.shape[0] == M and residual.stride(1) == 1
        res_arg = (_p(residual), residual.stride(0))
    return res_arg, rope_arg


def _skinny_call(family, fmt, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope, w_scale=None):
    """gemv and gemm_skinny in every weight format: mla_<family>_<fmt.name>, the format's scale arguments behind W's."""
    name = f"mla_{family}_{fmt.name}"
    K, scale_arg = _proj_operands(fmt, name, x, W, w_scale, out)
    M, N = x.shape[0], W.shape[0]
    assert K == (x.shape[1] // 2 if swiglu else x.shape[1]) and not (swiglu and norm_weight is not None)
    pre = 2 if swiglu else (1 if norm_weight is not None else 0)
    if norm_weight is not None:
        _req(norm_weight, torch.bfloat16, f"{name} norm weight")
        assert norm_weight.numel() == K and norm_weight.is_contiguous()
    res_arg, rope_arg = _proj_epilogue(name, M, residual, out_col, rope, rows_per_batch)
    call(name, _p(x), x.stride(0), _p(W), W.stride(0), *scale_arg, c_void_p(out.data_ptr() + 2 * out_col), ldo, out_batch_stride, rows_per_batch,
         *res_arg, M, N, K, pre, _p(norm_weight), float(eps), *rope_arg)


GEMV_MMAX, GEMV_LDS = 8, 160 * 1024


def gemv_fits(M: int, K: int) -> bool:
    """True when mla_gemv_bf16 accepts M rows of K inputs (M <= 8, the M x K bf16 rows + 64 B in LDS)."""
    return 1 <= M <= GEMV_MMAX and M * K * 2 + 64 <= GEMV_LDS


def gemv(x, W, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, norm_weight=None, eps=0.0, swiglu=False, rope=None):
    """out row m (at out + (m // rows_per_batch) * out_batch_stride + (m % rows_per_batch) * ldo + out_col) = f(x[m]) @ W^T (+ residual[m]);
    M <= 8 rows, every weight row read once (mla_gemv_bf16). `out` is a base tensor: only its data pointer is used.
    f = identity; or LlamaRMSNorm(x; norm_weight, eps); or (swiglu=True, x = packed gate|up rows [M, 2 K]) silu(gate) * up.
    rope = (cos [rows_per_batch, 64], sin, rope_cols): output columns [0, rope_cols) are rotated per head of 128 in the epilogue."""
    _skinny_call("gemv", _WF_BF16, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope)


def gemm_skinny(x, W, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, norm_weight=None, eps=0.0, swiglu=False, rope=None):
    """gemv's contract for 1 <= M <= 64 rows and any K (mla_gemm_skinny_bf16): every weight row read once, on the MFMA pipe, x never
    staged in LDS. Same arguments, output addressing, fused RMSNorm / SwiGLU inputs and RoPE epilogue as gemv."""
    _skinny_call("gemm_skinny", _WF_BF16, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope)


def quant_fp8_rows(W, q=None, scale=None):
    """Per-row FP8 quantisation of W [N, K] bf16 (rows may be strided; K % 16 == 0) for the `_w8` projections (mla_quant_fp8_rows):
    scale[n] = amax[n] / 448 (1 for an all-zero row), q = e4m3fn_rne(clamp(W / scale, -448, 448)); the CPU statement
    (W.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn) gives the same bytes. Returns (q [N, K] float8_e4m3fn,
    scale [N] fp32); q / scale may be given (views of a packed buffer). Non-finite input is not supported."""
    return _quant_rows(_WF_W8, "quant_fp8_rows", W, q, scale, "scale")


def gemv_w8(x, W, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, norm_weight=None, eps=0.0, swiglu=False,
            rope=None):
    """gemv over FP8 weights (mla_gemv_w8): W [N, K] float8_e4m3fn, w_scale [N] fp32 as quant_fp8_rows writes them; out row m =
    w_scale * (f(x[m]) @ float(W)^T) (+ residual[m]), the scale applied to the finished fp32 sum. K % 16 == 0; everything else is gemv's."""
    _skinny_call("gemv", _WF_W8, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope, w_scale)


def gemm_skinny_w8(x, W, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, norm_weight=None, eps=0.0,
                   swiglu=False, rope=None):
    """gemv_w8's contract for 1 <= M <= 64 rows and any K % 16 == 0 (mla_gemm_skinny_w8): the codes are decoded to bf16 into the MFMA
    operands."""
    _skinny_call("gemm_skinny", _WF_W8, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope, w_scale)


def quant_mxfp4_rows(W, q=None, s=None):
    """OCP MXFP4 quantisation of W [N, K] bf16 (rows may be strided; K % 32 == 0) for the `_w4` projections (mla_quant_mxfp4_rows):
    q [N, K / 2] uint8 -- element 2 j in the low nibble of byte j, nibble = sign (8) | index into {0, 0.5, 1, 1.5, 2, 3, 4, 6} -- and
    s [N, K / 32] uint8, one e8m0 byte (e + 127) per block of 32 consecutive k of a row, e = clamp(floor(log2 amax) - 2, -125, 125) from
    the exponent bits; round to nearest, ties to the even mantissa bit, saturating at 6 (include/mla_hip.h has the whole statement).
    Returns (q, s); both may be given (views of a packed buffer: q rows 16-B aligned, unit inner strides; the scale row stride is passed
    on). Non-finite input is not supported."""
    return _quant_rows(_WF_W4, "quant_mxfp4_rows", W, q, s, "s")


def gemv_w4(x, W, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, norm_weight=None, eps=0.0, swiglu=False,
            rope=None):
    """gemv over MXFP4 weights (mla_gemv_w4): W [N, K / 2] uint8 codes, w_scale [N, K / 32] uint8 as quant_mxfp4_rows writes them; the codes
    are decoded with their block scale (exact in bf16), so out row m = f(x[m]) @ dequantised(W)^T (+ residual[m]) with gemv's single bf16
    rounding. K % 32 == 0; everything else is gemv's."""
    _skinny_call("gemv", _WF_W4, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope, w_scale)


def gemm_skinny_w4(x, W, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, norm_weight=None, eps=0.0,
                   swiglu=False, rope=None):
    """gemv_w4's contract for 1 <= M <= 64 rows and any K % 32 == 0 (mla_gemm_skinny_w4): the codes are decoded to bf16 into the MFMA
    operands, on gemm_skinny_w8's K steps."""
    _skinny_call("gemm_skinny", _WF_W4, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, norm_weight, eps, swiglu, rope, w_scale)


def _skinny_gateup_call(fmt, x, W, out, ldo, w_scale=None):
    """The shared call of the gate|up + SwiGLU projection in every weight format: _skinny_call's argument checks without a residual, a
    rotary epilogue or a pre-transform; out [M, I] is allocated when not given (ldo: its row stride in elements, default out.stride(0))."""
    name = f"mla_gemm_skinny_gateup_swiglu_{fmt.name}"
    K, scale_arg = _proj_operands(fmt, name, x, W, w_scale)
    assert W.shape[0] % 2 == 0 and x.shape[1] == K
    M, I = x.shape[0], W.shape[0] // 2
    if out is None:
        out = torch.empty((M, I), dtype=torch.bfloat16, device=x.device)
    _req(out, torch.bfloat16, f"{name} out")
    call(name, _p(x), x.stride(0), _p(W), W.stride(0), *scale_arg, _p(out), out.stride(0) if ldo is None else ldo, M, I, K)
    return out


def gemm_skinny_gateup_swiglu(x, W, out=None, ldo=None):
    """silu(x @ Wg^T) * (x @ Wu^T) for 1 <= M <= 64 rows, W = the packed gate|up matrix [2 I, K] (mla_gemm_skinny_gateup_swiglu_bf16):
    gemm_skinny's plain form with SwiGLU in the epilogue -- bit for bit swiglu_fwd(gemm_skinny(x, W)), the [M, 2 I] rows never reach
    memory. Returns out [M, I] bf16 (`out` may be given: a base tensor with row stride ldo >= I)."""
    return _skinny_gateup_call(_WF_BF16, x, W, out, ldo)


def gemm_skinny_gateup_swiglu_w8(x, W, w_scale, out=None, ldo=None):
    """gemm_skinny_gateup_swiglu over FP8 weights (mla_gemm_skinny_gateup_swiglu_w8): W [2 I, K] float8_e4m3fn, w_scale [2 I] fp32; each
    finished fp32 sum times its own row's scale in front of the bf16 rounding, as gemm_skinny_w8 does. K % 16 == 0."""
    return _skinny_gateup_call(_WF_W8, x, W, out, ldo, w_scale)


def gemm_skinny_gateup_swiglu_w4(x, W, w_scale, out=None, ldo=None):
    """gemm_skinny_gateup_swiglu over MXFP4 weights (mla_gemm_skinny_gateup_swiglu_w4): W [2 I, K / 2] uint8 codes, w_scale [2 I, K / 32]
    uint8; bit for bit swiglu_fwd of gemm_skinny_w4's output. K % 32 == 0."""
    return _skinny_gateup_call(_WF_W4, x, W, out, ldo, w_scale)


def attn_decode(cache, B, nheads, D, S_kv, R, scale):
    """cache [B, S_cap >= S_kv, 3 * nheads * D] packed post-RoPE q|k|v rows; the R query rows are rows [S_kv - R, S_kv) of every sample,
    query r attends to keys [0, S_kv - R + r] (mla_attn_decode). Returns o [B * R, nheads * D] bf16."""
    _req(cache, torch.bfloat16, "attn_decode cache")
    H = nheads * D
    assert cache.shape[0] == B and cache.shape[2] == 3 * H and cache.stride(2) == 1 and cache.shape[1] >= S_kv
    o = torch.empty((B * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    call("mla_attn_decode", c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), B, nheads, D, S_kv, R, cache.stride(1),
         cache.stride(0), H, float(scale))
    return o


DEC_RMAX = 8


def attn_decode_fits(R: int, S_kv: int) -> bool:
    """True when mla_attn_decode accepts R query rows against S_kv keys (R <= 8, the R x S_kv fp32 scores + 8 R x 128 partials in LDS)."""
    return 1 <= R <= DEC_RMAX and R <= S_kv and (R * S_kv + 8 * R * 128) * 4 <= 160 * 1024


def attn_chunk(cache, B, nheads, D, S_kv, R, scale):
    """attn_decode's contract for 1 <= R <= 64 query rows and any S_kv (mla_attn_chunk: online softmax over key tiles, MFMA QK^T / PV).
    Returns o [B * R, nheads * D] bf16."""
    _req(cache, torch.bfloat16, "attn_chunk cache")
    H = nheads * D
    assert cache.shape[0] == B and cache.shape[2] == 3 * H and cache.stride(2) == 1 and cache.shape[1] >= S_kv
    o = torch.empty((B * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    call("mla_attn_chunk", c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), B, nheads, D, S_kv, R, cache.stride(1),
         cache.stride(0), H, float(scale))
    return o


# ---- split-key suffix attention (mla_amd/csrc/attn_split.hip): attn_chunk with every head's key tiles cut over several workgroups
ATTN_SPLIT_WAVES, ATTN_SPLIT_STATE_WORDS, ATTN_SPLIT_COMBINE_WAVES = 4, 130, 4


class AttnSplitPlan(NamedTuple):
    """What mla_attn_chunk_split does with a shape: ranges the 64-key tiles are cut into, tiles of the larger ranges, workgroups of the
    first launch (B * H * ceil(R / 16) * splits), workgroups of the combine launch and workspace bytes (both 0 when splits == 1)."""
    splits: int
    tiles_per_split: int
    workgroups: int
    combine_workgroups: int
    ws_bytes: int


def plan_attn_split(B: int, H: int, R: int, S_kv: int, cus: int = 256) -> AttnSplitPlan:
    """Pure-Python mirror of the launcher's choice (attn_split.hip:sp_plan; mla_attn_chunk_split_plan returns the library's): splits grows
    by one while the first launch still fits one workgroup per CU, splits < nT and the largest range has more than 4 tiles of 64 keys (one
    tile per wave and pass: cutting below one pass saves nothing)."""
    if not (B >= 1 and H >= 1 and 1 <= R <= 64 and S_kv >= R and cus >= 1):
        raise ValueError(f"plan_attn_split: B, H, cus >= 1 and 1 <= R <= 64, R <= S_kv required (B {B}, H {H}, R {R}, S_kv {S_kv}, cus {cus})")
    base, nT = B * H * -(-R // 16), -(-S_kv // 64)
    splits = 1
    while base * (splits + 1) <= cus and splits < nT and -(-nT // splits) > ATTN_SPLIT_WAVES:
        splits += 1
    return AttnSplitPlan(splits, -(-nT // splits), base * splits, -(-B * H * R // ATTN_SPLIT_COMBINE_WAVES) if splits > 1 else 0,
                         B * H * R * splits * ATTN_SPLIT_STATE_WORDS * 4 if splits > 1 else 0)


def attn_split_plan(B: int, H: int, R: int, S_kv: int, cus: int = 256) -> tuple:
    """The library's plan (mla_attn_chunk_split_plan): (splits, tiles per split, workgroups, combine workgroups)."""
    out = (c_int * 4)()
    _check(lib().mla_attn_chunk_split_plan(int(B), int(H), int(R), int(S_kv), int(cus), out), "mla_attn_chunk_split_plan")
    return tuple(out)


def attn_split_ws_bytes(B: int, H: int, R: int, S_kv: int, splits: int = 0) -> int:
    """Workspace bytes mla_attn_chunk_split needs (mla_attn_chunk_split_ws_bytes; splits 0 = the plan's); -1 outside the contract."""
    return int(lib().mla_attn_chunk_split_ws_bytes(int(B), int(H), int(R), int(S_kv), int(splits)))


def attn_chunk_split(cache, B, nheads, D, S_kv, R, scale, splits=None, ws=None):
    """attn_chunk's contract with every head's key tiles cut into `splits` ranges read by their own workgroups, and a second launch that
    merges the partial softmax states in a fixed order (mla_attn_chunk_split). splits None = the library's plan; an explicit value
    (1 .. ceil(S_kv / 64)) is for tests and the kernel table; 1 gives attn_chunk's bits. ws: caller-owned scratch of at least
    attn_split_ws_bytes(...) bytes (any dtype); None allocates one for this call. Returns o [B * R, nheads * D] bf16."""
    _req(cache, torch.bfloat16, "attn_chunk_split cache")
    H = nheads * D
    assert cache.shape[0] == B and cache.shape[2] == 3 * H and cache.stride(2) == 1 and cache.shape[1] >= S_kv
    sp = 0 if splits is None else int(splits)
    if ws is None:
        need = attn_split_ws_bytes(B, nheads, R, S_kv, sp)
        if need > 0:
            ws = torch.empty(need, dtype=torch.uint8, device=cache.device)
    else:
        assert ws.is_cuda and ws.is_contiguous()
    o = torch.empty((B * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    call("mla_attn_chunk_split", c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), B, nheads, D, S_kv, R, cache.stride(1),
         cache.stride(0), H, float(scale), sp, _p(ws), ws.numel() * ws.element_size() if ws is not None else 0)
    return o


SUFFIX_MMAX = 256


def _suffix_call(fmt, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, rope, slot, cap_rows, w_scale=None,
                 rope_pos=None, rope_rows=None):
    """The shared call of the batched suffix projection in every weight format: mla_gemm_suffix_<fmt.name>, the format's scale arguments
    behind W's; rope_pos (int32, one rotary position per sample) selects the `_pos` entry point."""
    sym, name = f"mla_gemm_suffix_{fmt.name}", "gemm_suffix" + fmt.suffix
    K, scale_arg = _proj_operands(fmt, name, x, W, w_scale, out)
    M, N = x.shape[0], W.shape[0]
    assert x.shape[1] == K
    if slot is not None:
        _req(slot, torch.int32, f"{name} slot")
        assert cap_rows is not None and slot.is_contiguous() and slot.numel() * rows_per_batch >= M
    cap = int(cap_rows) if slot is not None else int(rows_per_batch)
    pos_arg = ()
    if rope_pos is not None:
        _req(rope_pos, torch.int32, f"{name} rope_pos")
        assert rope is not None and rope_rows is not None and rope_pos.is_contiguous() and rope_pos.numel() * rows_per_batch >= M
        pos_arg = (_p(rope_pos), int(rope_rows))
        sym += "_pos"
    res_arg, rope_arg = _proj_epilogue(name, M, residual, out_col, rope, cap if rope_pos is None else int(rope_rows))
    call(sym, _p(x), x.stride(0), _p(W), W.stride(0), *scale_arg, c_void_p(out.data_ptr() + 2 * out_col), ldo, out_batch_stride,
         rows_per_batch, _p(slot), cap, *res_arg, M, N, K, *rope_arg, *pos_arg)


def gemm_suffix(x, W, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, rope=None, slot=None, cap_rows=None,
                rope_pos=None, rope_rows=None):
    """out row m = x[m] @ W^T (+ residual[m]) for 1 <= M <= 256 rows of a batch of samples (mla_gemm_suffix_bf16; plain input only).
    Row m is row p = m % rows_per_batch of sample b = m // rows_per_batch and lands at out + b * out_batch_stride + (slot[b] + p) * ldo
    + out_col. slot: int32 [B] device tensor (the sample's prefix length) with cap_rows = rows per sample that `out` (and the tables) hold;
    None = every slot 0. rope = (cos [cap_rows or rows_per_batch, 64], sin, rope_cols): row slot[b] + p of the tables rotates the row.
    rope_pos (mla_gemm_suffix_bf16_pos): int32 [B] device tensor with rope_rows = rows of the tables ([rope_rows, 64]); the row is then
    rotated with table row rope_pos[b] + p instead, and not written when that lies outside [0, rope_rows). None = the call above."""
    _suffix_call(_WF_BF16, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, rope, slot, cap_rows, rope_pos=rope_pos, rope_rows=rope_rows)


def gemm_suffix_w8(x, W, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, rope=None, slot=None, cap_rows=None,
                   rope_pos=None, rope_rows=None):
    """gemm_suffix over FP8 weights (mla_gemm_suffix_w8): W [N, K] float8_e4m3fn, w_scale [N] fp32 as quant_fp8_rows writes them; out row m =
    w_scale * (x[m] @ float(W)^T) (+ residual[m]), the scale applied to the finished fp32 sum (gemm_skinny_w8's arithmetic: every 64-row
    slice is bit for bit its output). K % 16 == 0; rows, slots, rope, rope_pos (mla_gemm_suffix_w8_pos) and addressing are gemm_suffix's."""
    _suffix_call(_WF_W8, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, rope, slot, cap_rows, w_scale, rope_pos, rope_rows)


def gemm_suffix_w4(x, W, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, rope=None, slot=None, cap_rows=None,
                   rope_pos=None, rope_rows=None):
    """gemm_suffix over MXFP4 weights (mla_gemm_suffix_w4): W [N, K / 2] uint8 codes, w_scale [N, K / 32] uint8 as quant_mxfp4_rows writes
    them; gemm_skinny_w4's arithmetic (every 64-row slice is bit for bit its output). K % 32 == 0; rows, slots, rope, rope_pos
    (mla_gemm_suffix_w4_pos) and addressing are gemm_suffix's."""
    _suffix_call(_WF_W4, x, W, out, ldo, out_batch_stride, rows_per_batch, residual, out_col, rope, slot, cap_rows, w_scale, rope_pos, rope_rows)


# ---- compact prefill GEMMs (mla_amd/csrc/prefill.hip): 1 <= M <= 1024 rows, 64 x 128 tiles, deterministic split-K through a workspace. Two
# operand kinds: bf16 x and W, or ("_f8" names) e4m3fn codes of BOTH operands with one fp32 scale per row (quant_fp8_rows) on
# v_mfma_f32_16x16x128_f8f6f4; a K tile is 64 bf16 or 128 codes
PREFILL_MMAX, PREFILL_BM, PREFILL_BN, PREFILL_BK = 1024, 64, 128, 64
PREFILL_F8_BK = 128
PREFILL_MAX_SPLIT, PREFILL_MIN_KTILES = 16, 8


class PrefillKind(NamedTuple):
    """An operand kind: what follows "gemm_prefill" in its Python and library names, K granularity, K tile, operand dtype."""
    infix: str
    k_gran: int
    k_tile: int
    dtype: torch.dtype

    def ws_bytes(self, M: int, N: int, K: int) -> int:
        """Workspace bytes the library's launcher needs for the shape (mla_gemm_prefill[_f8]_ws_bytes); -1 outside the contract."""
        return int(getattr(lib(), f"mla_gemm_prefill{self.infix}_ws_bytes")(int(M), int(N), int(K)))


PREFILL_KINDS = {"bf16": PrefillKind("", 32, PREFILL_BK, torch.bfloat16),
                 "fp8": PrefillKind("_f8", PREFILL_F8_BK, PREFILL_F8_BK, torch.float8_e4m3fn)}
_PF_BF16, _PF_F8 = PREFILL_KINDS["bf16"], PREFILL_KINDS["fp8"]
# the wide-row FP8 family ("_f8_wide" names): _PF_F8's contract for 1 <= M <= 65536, the row tile (64 | 128) chosen by the plan
PREFILL_WIDE_MMAX, PREFILL_WIDE_BM, PREFILL_WIDE_WGS_PER_CU = 65536, 128, 3
_PF_F8_WIDE = PREFILL_KIND_F8_WIDE = PrefillKind("_f8_wide", PREFILL_F8_BK, PREFILL_F8_BK, torch.float8_e4m3fn)


class PrefillGemmPlan(NamedTuple):
    """What the prefill launcher does with a shape: tile (rows, columns), split-K factor, workgroups of the main launch, rows covered
    (M rounded up to the row tile), workspace bytes = split * rows_covered * N * 4 (0 when split == 1), and a note when the plan stays
    under two workgroups per CU."""
    tile_m: int
    tile_n: int
    split: int
    workgroups: int
    rows_covered: int
    ws_bytes: int
    note: str


def _prefill_fits(kind, M, N, K):
    return 1 <= M <= (PREFILL_WIDE_MMAX if kind is _PF_F8_WIDE else PREFILL_MMAX) and N >= PREFILL_BN and N % PREFILL_BN == 0 and K >= kind.k_gran and K % kind.k_gran == 0


def _prefill_plan(kind, M, N, K, cus):
    """The launcher's choice (prefill.hip:plan / plan_wide) for an operand kind: 64 x 128 tiles -- the wide family: 128 x 128 for M > 1024
    once those alone give 3 x cus workgroups (measured: profiles/batch_prefill_fp8_infer_latency.txt) --, split-K doubled while tiles x split < 2 x cus, split < 16 and every slice keeps at least
    8 K tiles."""
    wide = kind is _PF_F8_WIDE
    if not _prefill_fits(kind, M, N, K):
        raise ValueError(f"plan_gemm_prefill{kind.infix}: 1 <= M <= {PREFILL_WIDE_MMAX if wide else PREFILL_MMAX}, N % {PREFILL_BN} == 0, "
                         f"K % {kind.k_gran} == 0 required (M {M}, N {N}, K {K})")
    bm = PREFILL_BM
    if wide and M > PREFILL_MMAX and -(-M // PREFILL_WIDE_BM) * (N // PREFILL_BN) >= PREFILL_WIDE_WGS_PER_CU * cus:
        bm = PREFILL_WIDE_BM
    mt, nt, ktiles = -(-M // bm), N // PREFILL_BN, -(-K // kind.k_tile)
    tiles = mt * nt
    split = 1
    while tiles * split < 2 * cus and split < PREFILL_MAX_SPLIT and ktiles // (split * 2) >= PREFILL_MIN_KTILES:
        split *= 2
    wgs = tiles * split
    note = ""
    if wgs < cus:
        note = (f"{wgs} workgroups < {cus} CUs: " +
                (f"split-K is capped at {PREFILL_MAX_SPLIT}" if split == PREFILL_MAX_SPLIT else
                 f"K = {K} has {ktiles} K tiles, a slice keeps at least {PREFILL_MIN_KTILES}"))
    return PrefillGemmPlan(bm, PREFILL_BN, split, wgs, mt * bm, split * mt * bm * N * 4 if split > 1 else 0, note)


def gemm_prefill_fits(M: int, N: int, K: int) -> bool:
    """True when the compact prefill GEMMs accept the shape: 1 <= M <= 1024, N % 128 == 0 (2 I for the SwiGLU form), K % 32 == 0."""
    return _prefill_fits(_PF_BF16, M, N, K)


def gemm_prefill_f8_fits(M: int, N: int, K: int) -> bool:
    """As gemm_prefill_fits, over codes: K % 128 == 0."""
    return _prefill_fits(_PF_F8, M, N, K)


def plan_gemm_prefill(M: int, N: int, K: int, cus: int = 256) -> PrefillGemmPlan:
    """Pure-Python mirror of the launcher's choice on K tiles of 64 bf16 (mla_gemm_prefill_plan returns the library's)."""
    return _prefill_plan(_PF_BF16, M, N, K, cus)


def plan_gemm_prefill_f8(M: int, N: int, K: int, cus: int = 256) -> PrefillGemmPlan:
    """As plan_gemm_prefill, on K tiles of 128 codes (mla_gemm_prefill_f8_plan returns the library's)."""
    return _prefill_plan(_PF_F8, M, N, K, cus)


def gemm_prefill_f8_wide_fits(M: int, N: int, K: int) -> bool:
    """As gemm_prefill_f8_fits, for the wide-row family: 1 <= M <= 65536."""
    return _prefill_fits(_PF_F8_WIDE, M, N, K)


def plan_gemm_prefill_f8_wide(M: int, N: int, K: int, cus: int = 256) -> PrefillGemmPlan:
    """As plan_gemm_prefill_f8, for the wide-row family (mla_gemm_prefill_f8_wide_plan returns the library's): tile_m is 64 or 128; for
    M <= 1024 it is plan_gemm_prefill_f8's plan."""
    return _prefill_plan(_PF_F8_WIDE, M, N, K, cus)


def gemm_prefill_f8_wide_ws_bytes(M: int, N: int, K: int) -> int:
    """As gemm_prefill_f8_ws_bytes, for the wide-row family (mla_gemm_prefill_f8_wide_ws_bytes)."""
    return _PF_F8_WIDE.ws_bytes(M, N, K)


def gemm_prefill_ws_bytes(M: int, N: int, K: int) -> int:
    """Workspace bytes the library's launcher needs for the shape (mla_gemm_prefill_ws_bytes); -1 outside the contract."""
    return _PF_BF16.ws_bytes(M, N, K)


def gemm_prefill_f8_ws_bytes(M: int, N: int, K: int) -> int:
    """As gemm_prefill_ws_bytes, over codes (mla_gemm_prefill_f8_ws_bytes)."""
    return _PF_F8.ws_bytes(M, N, K)


def _prefill(form, scales, x, W, out, ldo, out_batch_stride, rows_per_batch, ws, residual=None, out_col=0, rope=None, head_dim=128,
             wide=False):
    """One launch of the family in the form "" (plain + residual), "_qkv_rope" or "_gateup_swiglu", over bf16 operands x [M, K] / W [N, K]
    (scales None) or over their FP8 codes with scales = (x_scale [M], w_scale [N]); wide: the wide-row entry points (codes only)."""
    assert not wide or scales is not None
    kind, q = (_PF_BF16, "") if scales is None else (_PF_F8_WIDE if wide else _PF_F8, "q")
    name = f"gemm_prefill{kind.infix}{form}"
    _req(x, kind.dtype, f"{name} x{q}")
    _req(W, kind.dtype, f"{name} W{q}")
    for t, what in zip(scales or (), ("x_scale", "w_scale")):
        _req(t, torch.float32, f"{name} {what}")
    _req(out, torch.bfloat16, f"{name} out")
    assert x.dim() == 2 and W.dim() == 2 and W.shape[1] == x.shape[1] and x.stride(1) == 1 and W.stride(1) == 1
    operands = [_p(x), x.stride(0), _p(W), W.stride(0)]
    if scales is not None:
        x_scale, w_scale = scales
        assert x_scale.numel() == x.shape[0] and x_scale.is_contiguous() and w_scale.numel() == W.shape[0] and w_scale.is_contiguous()
        operands = [*operands[:2], _p(x_scale), *operands[2:], _p(w_scale)]
    if ws is not None:
        assert ws.is_cuda and ws.is_contiguous()
    (M, K), N = x.shape, W.shape[0]
    if form == "_qkv_rope":
        cos, sin, rope_cols = rope
        _req(cos, torch.float32, f"{name} cos")
        _req(sin, torch.float32, f"{name} sin")
        assert cos.shape == (rows_per_batch, 64) and sin.shape == cos.shape and cos.is_contiguous() and sin.is_contiguous()
        shape = [M, N, K, _p(cos), _p(sin), int(rope_cols), int(head_dim)]
    elif form == "_gateup_swiglu":
        assert N % 2 == 0
        ldo, rows_per_batch = out.stride(0) if ldo is None else ldo, M if rows_per_batch is None else rows_per_batch
        shape = [M, N // 2, K]
    else:
        if residual is not None:
            _req(residual, torch.bfloat16, f"{name} residual")
            assert residual.shape[0] == M and residual.stride(1) == 1
        shape = [_p(residual), residual.stride(0) if residual is not None else 0, M, N, K]
    call(f"mla_{name}" + ("_bf16" if name == "gemm_prefill" else ""), *operands, c_void_p(out.data_ptr() + 2 * out_col), ldo, out_batch_stride,
         rows_per_batch, *shape, _p(ws), ws.numel() * ws.element_size() if ws is not None else 0)


def gemm_prefill(x, W, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, ws=None):
    """out row m (at out + (m // rows_per_batch) * out_batch_stride + (m % rows_per_batch) * ldo + out_col) = x[m] @ W^T (+ residual[m])
    for 1 <= M <= 1024 rows (mla_gemm_prefill_bf16). `out` is a base tensor: only its data pointer is used. ws: caller-owned scratch of
    at least gemm_prefill_ws_bytes(M, N, K) bytes (any dtype; may be None when the plan does not split)."""
    _prefill("", None, x, W, out, ldo, out_batch_stride, rows_per_batch, ws, residual=residual, out_col=out_col)


def gemm_prefill_qkv_rope(x, W, out, ldo, out_batch_stride, rows_per_batch, rope, head_dim=128, ws=None):
    """gemm_prefill's rows and addressing with the rotary embedding of columns [0, rope_cols) in the epilogue (mla_gemm_prefill_qkv_rope):
    rope = (cos [rows_per_batch, 64] fp32, sin, rope_cols); row m is rotated with table row m % rows_per_batch, per head of 128."""
    _prefill("_qkv_rope", None, x, W, out, ldo, out_batch_stride, rows_per_batch, ws, rope=rope, head_dim=head_dim)


def gemm_prefill_gateup_swiglu(x, wgu, act, ldo=None, out_batch_stride=0, rows_per_batch=None, ws=None):
    """act[m] = silu(x[m] @ Wg^T) * (x[m] @ Wu^T) for the packed wgu = [Wg; Wu] [2 I, K] (mla_gemm_prefill_gateup_swiglu): the product is
    formed in the epilogue on the fp32 sums; nothing but act [M, I] is written. Addressing as gemm_prefill (default: act's own rows)."""
    _prefill("_gateup_swiglu", None, x, wgu, act, ldo, out_batch_stride, rows_per_batch, ws)


def gemm_prefill_f8(xq, x_scale, Wq, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, ws=None):
    """gemm_prefill over FP8 codes of both operands (mla_gemm_prefill_f8): out row m = bf16((xq[m] @ Wq^T) * x_scale[m] * w_scale
    (+ residual[m])), xq [M, K] / Wq [N, K] float8_e4m3fn and x_scale [M] / w_scale [N] fp32 as quant_fp8_rows writes them; the sums run
    over the codes in fp32. Addressing and ws as gemm_prefill, with gemm_prefill_f8_ws_bytes(M, N, K)."""
    _prefill("", (x_scale, w_scale), xq, Wq, out, ldo, out_batch_stride, rows_per_batch, ws, residual=residual, out_col=out_col)


def gemm_prefill_f8_qkv_rope(xq, x_scale, Wq, w_scale, out, ldo, out_batch_stride, rows_per_batch, rope, head_dim=128, ws=None):
    """gemm_prefill_qkv_rope over codes (mla_gemm_prefill_f8_qkv_rope): both scales are applied before the rotation, the partner channel
    with its own w_scale."""
    _prefill("_qkv_rope", (x_scale, w_scale), xq, Wq, out, ldo, out_batch_stride, rows_per_batch, ws, rope=rope, head_dim=head_dim)


def gemm_prefill_f8_gateup_swiglu(xq, x_scale, wgu_q, w_scale, act, ldo=None, out_batch_stride=0, rows_per_batch=None, ws=None):
    """gemm_prefill_gateup_swiglu over codes (mla_gemm_prefill_f8_gateup_swiglu): wgu_q = the packed [2 I, K] gate|up codes, w_scale [2 I];
    gate and up are scaled with the scales of their own rows before silu(gate) * up."""
    _prefill("_gateup_swiglu", (x_scale, w_scale), xq, wgu_q, act, ldo, out_batch_stride, rows_per_batch, ws)


def gemm_prefill_f8_wide(xq, x_scale, Wq, w_scale, out, ldo, out_batch_stride, rows_per_batch, residual=None, out_col=0, ws=None):
    """gemm_prefill_f8 for 1 <= M <= 65536 rows (mla_gemm_prefill_f8_wide): the same contract; the plan (plan_gemm_prefill_f8_wide) chooses
    64- or 128-row tiles, for M <= 1024 the bits are gemm_prefill_f8's. ws: at least gemm_prefill_f8_wide_ws_bytes(M, N, K) bytes."""
    _prefill("", (x_scale, w_scale), xq, Wq, out, ldo, out_batch_stride, rows_per_batch, ws, residual=residual, out_col=out_col, wide=True)


def gemm_prefill_f8_wide_qkv_rope(xq, x_scale, Wq, w_scale, out, ldo, out_batch_stride, rows_per_batch, rope, head_dim=128, ws=None):
    """gemm_prefill_f8_qkv_rope for 1 <= M <= 65536 rows (mla_gemm_prefill_f8_wide_qkv_rope)."""
    _prefill("_qkv_rope", (x_scale, w_scale), xq, Wq, out, ldo, out_batch_stride, rows_per_batch, ws, rope=rope, head_dim=head_dim, wide=True)


def gemm_prefill_f8_wide_gateup_swiglu(xq, x_scale, wgu_q, w_scale, act, ldo=None, out_batch_stride=0, rows_per_batch=None, ws=None):
    """gemm_prefill_f8_gateup_swiglu for 1 <= M <= 65536 rows (mla_gemm_prefill_f8_wide_gateup_swiglu)."""
    _prefill("_gateup_swiglu", (x_scale, w_scale), xq, wgu_q, act, ldo, out_batch_stride, rows_per_batch, ws, wide=True)


# --------------------------------------------------------------------------------------------- device-resident DDIM loop (sampler.hip)
DDIM_NMAX = 65536


def _ddim_step_checks(who, x, eps, x_bf16, coef, step):
    """The argument checks of ddim_step / ddim_step_pin -> x.numel()."""
    _req(x, torch.float32, who + " x")
    _req(eps, torch.bfloat16, who + " eps")
    _req(x_bf16, torch.bfloat16, who + " x_bf16")
    _req(coef, torch.float32, who + " coef")
    _req(step, torch.int32, who + " step")
    n = x.numel()
    if not (x.is_contiguous() and eps.is_contiguous() and x_bf16.is_contiguous() and coef.is_contiguous()):
        raise ValueError(f"{who}: x, eps, x_bf16 and coef must be contiguous")
    if eps.numel() != n or x_bf16.numel() != n or coef.dim() != 2 or coef.shape[1] != 4 or step.numel() != 1:
        raise ValueError(f"{who}: x {tuple(x.shape)}, eps {tuple(eps.shape)}, x_bf16 {tuple(x_bf16.shape)}, coef {tuple(coef.shape)}, "
                         f"step {tuple(step.shape)}")
    if not 1 <= n <= DDIM_NMAX:
        raise ValueError(f"{who}: {n} elements outside [1, {DDIM_NMAX}]")
    return n


def _ddpm_step_checks(who, x, eps, x_bf16, coef, noise, step):
    """The argument checks of ddpm_step / ddpm_step_pin -> x.numel()."""
    _req(x, torch.float32, who + " x")
    _req(eps, torch.bfloat16, who + " eps")
    _req(x_bf16, torch.bfloat16, who + " x_bf16")
    _req(coef, torch.float32, who + " coef")
    _req(noise, torch.float32, who + " noise")
    _req(step, torch.int32, who + " step")
    n = x.numel()
    if not (x.is_contiguous() and eps.is_contiguous() and x_bf16.is_contiguous() and coef.is_contiguous() and noise.is_contiguous()):
        raise ValueError(f"{who}: x, eps, x_bf16, coef and noise must be contiguous")
    if eps.numel() != n or x_bf16.numel() != n or coef.dim() != 2 or coef.shape[1] != 5 or step.numel() != 1 \
            or tuple(noise.shape) != (coef.shape[0], n):
        raise ValueError(f"{who}: x {tuple(x.shape)}, eps {tuple(eps.shape)}, x_bf16 {tuple(x_bf16.shape)}, coef {tuple(coef.shape)}, "
                         f"noise {tuple(noise.shape)} (wanted [steps, x.numel()]), step {tuple(step.shape)}")
    if not 1 <= n <= DDIM_NMAX:
        raise ValueError(f"{who}: {n} elements outside [1, {DDIM_NMAX}]")
    return n


def _pin_checks(who, n, known, pin):
    """known fp32 and pin uint8, contiguous, x.numel() elements each."""
    _req(known, torch.float32, who + " known")
    _req(pin, torch.uint8, who + " pin")
    if not (known.is_contiguous() and pin.is_contiguous()):
        raise ValueError(f"{who}: known and pin must be contiguous")
    if known.numel() != n or pin.numel() != n:
        raise ValueError(f"{who}: known {tuple(known.shape)} and pin {tuple(pin.shape)} need x.numel() = {n} elements each")


def ddim_step(x, eps, x_bf16, coef, step, advance=True):
    """mla_ddim_step: the eta = 0 DDIM update of the chunk x (fp32, in place; any shape, contiguous) with row step[0] of coef [steps, 4] and
    the bf16 epsilons eps (same number of elements); x_bf16 <- bf16(x); advance: step[0] -= 1. A step[0] outside [0, steps) writes nothing."""
    n = _ddim_step_checks("ddim_step", x, eps, x_bf16, coef, step)
    call("mla_ddim_step", _p(x), _p(eps), _p(x_bf16), _p(coef), _p(step), n, coef.shape[0], 1 if advance else 0)


def ddim_step_pin(x, eps, x_bf16, coef, known, pin, step, advance=True):
    """mla_ddim_step_pin: ddim_step with the x0 prediction replaced by known (fp32) where pin (uint8) is non-zero, x.numel() elements
    each: ddim_sample with denoised_fn = where(pin, known, .), the same bits. pin all zero: ddim_step's bits."""
    n = _ddim_step_checks("ddim_step_pin", x, eps, x_bf16, coef, step)
    _pin_checks("ddim_step_pin", n, known, pin)
    call("mla_ddim_step_pin", _p(x), _p(eps), _p(x_bf16), _p(coef), _p(known), _p(pin), _p(step), n, coef.shape[0], 1 if advance else 0)


def ddpm_step(x, eps, x_bf16, coef, noise, step, advance=True):
    """mla_ddpm_step: the DDPM posterior step (GaussianDiffusion.p_sample, clip_denoised=False) of the chunk x (fp32, in place; any shape,
    contiguous) with row step[0] of coef [steps, 5], the bf16 epsilons eps and row step[0] of noise [steps, x.numel()] fp32; x_bf16 <-
    bf16(x); advance: step[0] -= 1. A step[0] outside [0, steps) writes nothing."""
    n = _ddpm_step_checks("ddpm_step", x, eps, x_bf16, coef, noise, step)
    call("mla_ddpm_step", _p(x), _p(eps), _p(x_bf16), _p(coef), _p(noise), _p(step), n, coef.shape[0], 1 if advance else 0)


def ddpm_step_pin(x, eps, x_bf16, coef, noise, known, pin, step, advance=True):
    """mla_ddpm_step_pin: ddpm_step with the x0 prediction replaced by known (fp32) where pin (uint8) is non-zero, x.numel() elements
    each: p_sample with denoised_fn = where(pin, known, .), the same bits. pin all zero: ddpm_step's bits."""
    n = _ddpm_step_checks("ddpm_step_pin", x, eps, x_bf16, coef, noise, step)
    _pin_checks("ddpm_step_pin", n, known, pin)
    call("mla_ddpm_step_pin", _p(x), _p(eps), _p(x_bf16), _p(coef), _p(noise), _p(known), _p(pin), _p(step), n, coef.shape[0],
         1 if advance else 0)


def _dpmpp2m_step_checks(who, x, eps, x_bf16, hist, coef, step):
    """The argument checks of dpmpp2m_step / dpmpp2m_step_pin -> x.numel()."""
    _req(x, torch.float32, who + " x")
    _req(eps, torch.bfloat16, who + " eps")
    _req(x_bf16, torch.bfloat16, who + " x_bf16")
    _req(hist, torch.float32, who + " hist")
    _req(coef, torch.float32, who + " coef")
    _req(step, torch.int32, who + " step")
    n = x.numel()
    if not (x.is_contiguous() and eps.is_contiguous() and x_bf16.is_contiguous() and hist.is_contiguous() and coef.is_contiguous()):
        raise ValueError(f"{who}: x, eps, x_bf16, hist and coef must be contiguous")
    if eps.numel() != n or x_bf16.numel() != n or hist.numel() != n or coef.dim() != 2 or coef.shape[1] != 5 or step.numel() != 1:
        raise ValueError(f"{who}: x {tuple(x.shape)}, eps {tuple(eps.shape)}, x_bf16 {tuple(x_bf16.shape)}, hist {tuple(hist.shape)}, "
                         f"coef {tuple(coef.shape)}, step {tuple(step.shape)}")
    if not 1 <= n <= DDIM_NMAX:
        raise ValueError(f"{who}: {n} elements outside [1, {DDIM_NMAX}]")
    return n


def dpmpp2m_step(x, eps, x_bf16, hist, coef, step, advance=True):
    """mla_dpmpp2m_step (include/mla_hip_optim.h): the DPM-Solver++(2M) update of the chunk x (fp32, in place; any shape, contiguous) with
    row step[0] of coef [steps, 5] (GaussianDiffusion.dpmpp2m_tables), the bf16 epsilons eps and hist (fp32, x.numel() elements, in place:
    the previous step's x0 prediction in, this step's out; zeros in front of the first step); x_bf16 <- bf16(x); advance: step[0] -= 1.
    A step[0] outside [0, steps) writes nothing."""
    n = _dpmpp2m_step_checks("dpmpp2m_step", x, eps, x_bf16, hist, coef, step)
    call("mla_dpmpp2m_step", _p(x), _p(eps), _p(x_bf16), _p(hist), _p(coef), _p(step), n, coef.shape[0], 1 if advance else 0)


def dpmpp2m_step_pin(x, eps, x_bf16, hist, coef, known, pin, step, advance=True):
    """mla_dpmpp2m_step_pin: dpmpp2m_step with the x0 prediction replaced by known (fp32) where pin (uint8) is non-zero, x.numel()
    elements each, in front of every use and of the store into hist: dpmpp2m_sample_loop with denoised_fn = where(pin, known, .), the
    same bits. pin all zero: dpmpp2m_step's bits."""
    n = _dpmpp2m_step_checks("dpmpp2m_step_pin", x, eps, x_bf16, hist, coef, step)
    _pin_checks("dpmpp2m_step_pin", n, known, pin)
    call("mla_dpmpp2m_step_pin", _p(x), _p(eps), _p(x_bf16), _p(hist), _p(coef), _p(known), _p(pin), _p(step), n, coef.shape[0],
         1 if advance else 0)


def sampler_rows(h_in, t_table, x_e, step, G, T):
    """mla_sampler_rows: rows [0, G (1 + T)) of h_in <- per group [t_table[step[0]] | x_e rows g T .. g T + T); rows behind them are not
    touched. h_in [>= G (1 + T), H], t_table [steps, H], x_e [>= G T, H] (or [G, T, H]) bf16, contiguous."""
    for t, name in ((h_in, "h_in"), (t_table, "t_table"), (x_e, "x_e")):
        _req(t, torch.bfloat16, "sampler_rows " + name)
        if not t.is_contiguous():
            raise ValueError(f"sampler_rows: {name} must be contiguous")
    _req(step, torch.int32, "sampler_rows step")
    H = t_table.shape[-1]
    if G < 1 or T < 1 or h_in.dim() != 2 or t_table.dim() != 2 or h_in.shape[1] != H or x_e.shape[-1] != H or step.numel() != 1 \
            or h_in.shape[0] < G * (1 + T) or x_e.numel() < G * T * H:
        raise ValueError(f"sampler_rows: G {G}, T {T}, h_in {tuple(h_in.shape)}, t_table {tuple(t_table.shape)}, x_e {tuple(x_e.shape)}")
    call("mla_sampler_rows", _p(h_in), _p(t_table), _p(x_e), _p(step), G, T, H, t_table.shape[0])


def attn_chunk_ragged(cache, B, nheads, D, kv_len, R, scale):
    """attn_chunk with one key count per sample: kv_len int32 [B] on the device, the R queries of sample b are cache rows
    [kv_len[b] - R, kv_len[b]) (mla_attn_chunk_ragged; lengths are clamped to [R, cache.shape[1]]). Returns o [B * R, nheads * D] bf16."""
    _req(cache, torch.bfloat16, "attn_chunk_ragged cache")
    _req(kv_len, torch.int32, "attn_chunk_ragged kv_len")
    H = nheads * D
    assert cache.shape[0] == B and cache.shape[2] == 3 * H and cache.stride(2) == 1 and kv_len.numel() == B and kv_len.is_contiguous()
    o = torch.empty((B * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    call("mla_attn_chunk_ragged", c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), B, nheads, D, _p(kv_len),
         cache.shape[1], R, cache.stride(1), cache.stride(0), H, float(scale))
    return o


def attn_chunk_groups(cache, G, nheads, D, S_p, R, scale, gw=None, order=None):
    """Attention of G groups of R suffix rows behind ONE sample's prefix (mla_attn_chunk_groups): cache [S_p + G * R, 3H] (or with a
    leading 1) packed post-RoPE q|k|v, rows [0, S_p) the prefix, row S_p + g * R + p suffix row p of group g, which sees the prefix and
    rows S_p + g * R .. S_p + g * R + p. Group g's rows are bit for bit attn_chunk(B = 1, S_kv = S_p + R) on cat(prefix, group g's rows).
    gw: groups per workgroup (1, 2, 4), order: 0 head-major work items as dispatched / 1 one chunk of them per XCD (measurement only --
    the bits depend on neither), None = the library's choice.
    Returns o [G * R, nheads * D] bf16."""
    _req(cache, torch.bfloat16, "attn_chunk_groups cache")
    if cache.dim() == 3:
        assert cache.shape[0] == 1
        cache = cache[0]
    H = nheads * D
    assert cache.dim() == 2 and cache.shape[1] == 3 * H and cache.stride(1) == 1 and G >= 1 and R >= 1 and S_p >= 0
    assert cache.shape[0] >= S_p + G * R, (tuple(cache.shape), S_p, G, R)
    o = torch.empty((G * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    args = (c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), G, nheads, D, S_p, R, cache.stride(0), H, float(scale))
    if gw is None and order is None:
        call("mla_attn_chunk_groups", *args)
    else:
        call("mla_attn_chunk_groups_gw", *args, int(gw or 0), -1 if order is None else int(order))
    return o


def attn_chunk_ragged_groups(cache, B, G, nheads, D, prefix_len, R, scale, gw=None, order=None):
    """attn_chunk_groups for B samples with their own prefix lengths (mla_attn_chunk_ragged_groups): cache [B, S_cap, 3H] packed post-RoPE
    q|k|v, prefix_len int32 [B] on the device (clamped to [0, S_cap - G * R]); in sample b rows [0, S_p[b]) are the prefix and row
    S_p[b] + g * R + p is suffix row p of group g. The rows of (b, g) are bit for bit attn_chunk_groups on cache[b] with S_p = S_p[b].
    gw / order: attn_chunk_groups' launch form arguments (same bits). Returns o [B * G * R, nheads * D] bf16, row (b * G + g) * R + p."""
    _req(cache, torch.bfloat16, "attn_chunk_ragged_groups cache")
    _req(prefix_len, torch.int32, "attn_chunk_ragged_groups prefix_len")
    H = nheads * D
    assert cache.dim() == 3 and cache.shape[0] == B and cache.shape[2] == 3 * H and cache.stride(2) == 1 and G >= 1 and R >= 1
    assert cache.shape[1] >= G * R and prefix_len.numel() == B and prefix_len.is_contiguous()
    o = torch.empty((B * G * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    args = (c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), B, G, nheads, D, _p(prefix_len), cache.shape[1], R,
            cache.stride(1), cache.stride(0), H, float(scale))
    if gw is None and order is None:
        call("mla_attn_chunk_ragged_groups", *args)
    else:
        call("mla_attn_chunk_ragged_groups_gw", *args, int(gw or 0), -1 if order is None else int(order))
    return o


def attn_groups_split_plan(B: int, G: int, H: int, R: int, S_p_or_cap: int, ragged: bool, cus: int = 256) -> tuple:
    """(S_max, the library's plan) of mla_attn_groups_split for a groups shape: the plan is mla_attn_chunk_split_plan at (B * G, H, R,
    S_max) -- (splits, tiles per split, workgroups, combine workgroups) -- and S_max the most logical keys a group can have: S_p + R for
    one sample with S_p prefix rows (ragged=False, B must be 1), S_cap - (G - 1) * R for B samples of S_cap cache rows with their prefix
    lengths in device memory (ragged=True)."""
    B, G, R, S = int(B), int(G), int(R), int(S_p_or_cap)
    if B < 1 or G < 1 or (not ragged and (B != 1 or S < 0)) or (ragged and S < G * R):
        raise ValueError(f"attn_groups_split_plan: B, G >= 1, B == 1 and S_p >= 0 (plain) or S_cap >= G * R (ragged) required (B {B}, G {G}, "
                         f"R {R}, S_p / S_cap {S}, ragged {bool(ragged)})")
    S_max = S - (G - 1) * R if ragged else S + R
    return S_max, attn_split_plan(B * G, H, R, S_max, cus)


def attn_groups_split(cache, B, G, nheads, D, prefix, R, scale, splits=None, ws=None):
    """attn_chunk_groups / attn_chunk_ragged_groups with every (sample, group)'s key tiles cut into `splits` ranges read by their own
    workgroups and merged in a fixed order by a second launch (mla_attn_groups_split). prefix: an int S_p with cache [S_p + G * R, 3H] (or
    with a leading 1; B must be 1), or an int32 device tensor [B] with cache [B, S_cap, 3H] (clamped to [0, S_cap - G * R]); G = 1 with
    prefix = kv_len - R is attn_chunk_ragged. splits None = the library's plan (attn_groups_split_plan), fixed on the host whatever the
    lengths; an explicit value (1 .. ceil(S_max / 64)) is for tests and the kernel table; 1 is the head form itself. A (b, g) block with
    splits <= its own tile count is bit for bit attn_chunk_split (B = 1, the same splits) on cat(prefix rows of b, rows of group g).
    ws: caller-owned scratch of at least attn_split_ws_bytes(B * G, nheads, R, S_max, splits) bytes; None allocates one for this call.
    Returns o [B * G * R, nheads * D] bf16, row (b * G + g) * R + p."""
    _req(cache, torch.bfloat16, "attn_groups_split cache")
    H = nheads * D
    ragged = isinstance(prefix, torch.Tensor)
    if ragged:
        _req(prefix, torch.int32, "attn_groups_split prefix")
        assert cache.dim() == 3 and cache.shape[0] == B and cache.shape[2] == 3 * H and cache.stride(2) == 1 and G >= 1 and R >= 1
        assert cache.shape[1] >= G * R and prefix.numel() == B and prefix.is_contiguous()
        S, ld, bs = cache.shape[1], cache.stride(1), cache.stride(0)
    else:
        if cache.dim() == 3:
            assert cache.shape[0] == 1
            cache = cache[0]
        S = int(prefix)
        assert B == 1 and cache.dim() == 2 and cache.shape[1] == 3 * H and cache.stride(1) == 1 and G >= 1 and R >= 1 and S >= 0
        assert cache.shape[0] >= S + G * R, (tuple(cache.shape), S, G, R)
        ld, bs = cache.stride(0), 0
    sp = 0 if splits is None else int(splits)
    if ws is None:
        need = attn_split_ws_bytes(B * G, nheads, R, S - (G - 1) * R if ragged else S + R, sp)
        if need > 0:
            ws = torch.empty(need, dtype=torch.uint8, device=cache.device)
    else:
        assert ws.is_cuda and ws.is_contiguous()
    o = torch.empty((B * G * R, H), dtype=torch.bfloat16, device=cache.device)
    base = cache.data_ptr()
    call("mla_attn_groups_split", c_void_p(base), c_void_p(base + 2 * H), c_void_p(base + 4 * H), _p(o), B, G, nheads, D,
         _p(prefix) if ragged else None, S, R, ld, bs, H, float(scale), sp, _p(ws), ws.numel() * ws.element_size() if ws is not None else 0)
    return o


# --------------------------------------------------------------------------------------------- losses
def ce_fwd(logits2d, labels, ncols=None, ignore_index=-100, want_loss=True):
    rows = logits2d.shape[0]
    ncols = logits2d.shape[1] if ncols is None else ncols
    loss = torch.empty(rows, dtype=torch.float32, device=logits2d.device) if want_loss else None
    lse = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    call("mla_ce_fwd", _p(logits2d), 1 if logits2d.dtype == torch.float32 else 0, logits2d.stride(0), _p(labels), _p(loss),
         _p(lse), rows, ncols, ignore_index)
    return loss, lse


def ce_bwd(logits2d, labels, lse, gscale1, inv_count, ncols=None, ignore_index=-100):
    rows = logits2d.shape[0]
    ncols = logits2d.shape[1] if ncols is None else ncols
    d = torch.zeros(logits2d.shape, dtype=torch.bfloat16, device=logits2d.device)
    call("mla_ce_bwd", _p(logits2d), 1 if logits2d.dtype == torch.float32 else 0, logits2d.stride(0), _p(labels), _p(lse),
         _p(gscale1), float(inv_count), _p(d), d.stride(0), rows, ncols, ignore_index)
    return d


def infonce_bwd(L, rlse, clse, gscale1, M):
    Mp = L.shape[0]
    dL = torch.empty((Mp, Mp), dtype=torch.bfloat16, device=L.device)
    call("mla_infonce_bwd", _p(L), _p(rlse), _p(clse), _p(gscale1), _p(dL), M, Mp)
    return dL


def l2norm_fwd(x2d, eps=1e-12):
    rows, n = x2d.shape
    y = torch.empty_like(x2d)
    norms = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    call("mla_l2norm_fwd", _p(x2d), _p(y), _p(norms), rows, n, float(eps))
    return y, norms


def l2norm_bwd(dy, y, norms):
    rows, n = y.shape
    dx = torch.empty_like(y)
    call("mla_l2norm_bwd", _p(dy), _p(y), _p(norms), _p(dx), rows, n)
    return dx


def calib_mfma(device="cuda", total_ms=300.0, measure_ms=200.0, blocks=None):
    """The random-operand MFMA stream of this box (include/mla_hip.h: mla_calib_mfma): launches of ~20 ms back to back for ~total_ms,
    the rate over the last ~measure_ms (HIP events on the launch stream) in PFLOP/s -- the first launches ramp the power controller.
    Synchronises. Returns dict(pflops, launches, ms_per_launch)."""
    dev = torch.device(device)
    if blocks is None:
        blocks = torch.cuda.get_device_properties(dev).multi_processor_count
    ops_ = torch.randn(512 * 24 * 8, device=dev).to(torch.bfloat16)
    out = torch.empty(blocks * 512, dtype=torch.float32, device=dev)
    fl = ctypes.c_double(0.0)
    iters = 16384                                          # ~19 ms per launch at 1.9 PFLOP/s on 256 CUs
    call("mla_calib_mfma", _p(ops_), _p(out), blocks, 256, ctypes.byref(fl))          # code-object load + clocks up
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call("mla_calib_mfma", _p(ops_), _p(out), blocks, iters, ctypes.byref(fl))
    e1.record()
    torch.cuda.synchronize(dev)
    one = max(e0.elapsed_time(e1), 1e-3)
    n_total = max(2, int(round(total_ms / one)))
    n_meas = max(1, min(n_total - 1, int(round(measure_ms / one))))
    evs = []
    for i in range(n_total):
        if i == n_total - n_meas:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            evs.append(ev)
        call("mla_calib_mfma", _p(ops_), _p(out), blocks, iters, ctypes.byref(fl))
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    evs.append(ev)
    torch.cuda.synchronize(dev)
    ms = evs[0].elapsed_time(evs[1])
    return {"pflops": fl.value * n_meas / (ms * 1e-3) / 1e15, "launches": n_meas, "ms_per_launch": ms / n_meas, "blocks": blocks}


def selftest(device="cuda"):
    src = torch.arange(256, dtype=torch.int32, device=device) * 7 + 3
    out_tr = torch.zeros(256, dtype=torch.int32, device=device)
    out_g = torch.zeros(256, dtype=torch.int32, device=device)
    call("mla_selftest", _p(src), _p(out_tr), _p(out_g))
    return src, out_tr, out_g


# --------------------------------------------------------------------------------------------- point cloud / vision
def transpose(x2d, out=None):
    """out[c][r] = x2d[r][c] (bf16, unit inner stride, any row stride)."""
    R, C = x2d.shape
    if out is None:
        out = torch.empty((C, R), dtype=torch.bfloat16, device=x2d.device)
    call("mla_transpose_bf16", _p(x2d), _p(out), R, C, x2d.stride(0), out.stride(0))
    return out


def rmsnorm_apply(x2d, w, rstd):
    """[T, H] = rmsnorm(x) with the saved rstd, row-major: bit for bit the y of the rmsnorm_fwd that made rstd."""
    rows, H = x2d.shape
    out = torch.empty_like(x2d)
    call("mla_rmsnorm_apply", _p(x2d), _p(w), _p(rstd), _p(out), rows, H)
    return out


def rmsnorm_apply_t(x2d, w, rstd):
    """[H, T] = transpose(rmsnorm(x) with the saved rstd) -- recompute + transpose in one pass."""
    rows, H = x2d.shape
    out = torch.empty((H, rows), dtype=torch.bfloat16, device=x2d.device)
    call("mla_rmsnorm_apply_t", _p(x2d), _p(w), _p(rstd), _p(out), rows, H, rows)
    return out


def swiglu_fwd_dual(gu2d):
    """(act [rows, I], actT [I, rows]) in one pass over gu."""
    rows, two_i = gu2d.shape
    act = torch.empty((rows, two_i // 2), dtype=torch.bfloat16, device=gu2d.device)
    actT = torch.empty((two_i // 2, rows), dtype=torch.bfloat16, device=gu2d.device)
    call("mla_swiglu_fwd_dual", _p(gu2d), _p(act), _p(actT), rows, two_i // 2, rows)
    return act, actT


def swiglu_fwd_t(gu2d):
    rows, two_i = gu2d.shape
    out = torch.empty((two_i // 2, rows), dtype=torch.bfloat16, device=gu2d.device)
    call("mla_swiglu_fwd_t", _p(gu2d), _p(out), rows, two_i // 2, rows)
    return out


def gather_rows(src2d, idx, out_rows=None, scatter=False):
    """gather: out[r] = src[idx[r]] (out has len(idx) rows, or out_rows >= len(idx) rows with a zero tail);
    scatter: out[idx[r]] = src[r] (out has out_rows rows, zero-filled)."""
    H = src2d.shape[1]
    n = idx.numel()
    if scatter:
        out = torch.zeros((out_rows, H), dtype=torch.bfloat16, device=src2d.device)
    elif out_rows is not None and out_rows != n:
        assert out_rows >= n, f"gather_rows: out_rows={out_rows} < len(idx)={n} (the kernel writes len(idx) rows)"
        out = torch.zeros((out_rows, H), dtype=torch.bfloat16, device=src2d.device)
    else:
        out = torch.empty((n, H), dtype=torch.bfloat16, device=src2d.device)
    call("mla_gather_rows_bf16", _p(src2d), _p(idx), _p(out), n, H, 1 if scatter else 0)
    return out


def project_points(xyz_n3, consts21, idx_out, valid_out, W, Hh, stride, ph, pw):
    call("mla_project_points", _p(xyz_n3), _p(consts21), _p(idx_out), _p(valid_out), xyz_n3.shape[0], W, Hh, stride, ph, pw)


def fps(xyz, start, npoint):
    B, N, _ = xyz.shape
    out = torch.empty((B, npoint), dtype=torch.int64, device=xyz.device)
    call("mla_fps", _p(xyz), _p(start), _p(out), B, N, npoint)
    return out


def knn(xyz, centers, k):
    B, N, _ = xyz.shape
    G = centers.shape[1]
    out = torch.empty((B, G, k), dtype=torch.int32, device=xyz.device)
    call("mla_knn", _p(xyz), _p(centers), _p(out), B, N, G, k)
    return out


def gather_rows_f32(src_bnw, idx_bg):
    B, N, W = src_bnw.shape
    G = idx_bg.shape[1]
    out = torch.empty((B, G, W), dtype=torch.float32, device=src_bnw.device)
    call("mla_gather_rows_f32", _p(src_bnw), _p(idx_bg), _p(out), B, N, G, W)
    return out


def lga_prep(xyz, feats_bnc, fps_idx, knn_idx, alpha, beta):
    B, N, _ = xyz.shape
    C = feats_bnc.shape[2]
    G, K = knn_idx.shape[1], knn_idx.shape[2]
    rows = torch.empty((B * G * K, 2 * C), dtype=torch.bfloat16, device=xyz.device)
    lc = torch.empty((B, G, 3), dtype=torch.float32, device=xyz.device)
    call("mla_lga_prep", _p(xyz), _p(feats_bnc), _p(fps_idx), _p(knn_idx), _p(rows), _p(lc), B, N, G, K, C, float(alpha),
         float(beta))
    return rows, lc


def colstats(x2d):
    rows, C = x2d.shape
    mean = torch.empty(C, dtype=torch.float32, device=x2d.device)
    var = torch.empty(C, dtype=torch.float32, device=x2d.device)
    P = lib().mla_colstats_blocks(rows)
    ws = workspace(P * 2 * C * 4, x2d.device)
    call("mla_colstats_bf16", _p(x2d), _p(mean), _p(var), rows, C, x2d.stride(0), _p(ws), ws.numel())
    return mean, var


def bn_apply(x2d, mean, var, w, b, eps, residual=None, relu=False):
    rows, C = x2d.shape
    y = torch.empty_like(x2d)
    call("mla_bn_apply", _p(x2d), _p(mean), _p(var), _p(w), _p(b), _p(residual), _p(y), rows, C, float(eps), 1 if relu else 0)
    return y


def maxpool_k(x2d, groups, K):
    C = x2d.shape[1]
    out = torch.empty((groups, C), dtype=torch.bfloat16, device=x2d.device)
    call("mla_maxpool_k", _p(x2d), _p(out), groups, K, C)
    return out


def im2col_patch(pix, P, Kpad):
    B, CT, Himg, Wimg = pix.shape
    rows = torch.empty((B * (Himg // P) * (Wimg // P), Kpad), dtype=torch.bfloat16, device=pix.device)
    call("mla_im2col_patch", _p(pix), 1 if pix.dtype == torch.float32 else 0, _p(rows), B, CT, Himg, Wimg, P, Kpad)
    return rows


def avgpool_tokens(x, B, gh, gw, cs):
    C = x.shape[-1]
    y = torch.empty((B * (gh // cs) * (gw // cs), C), dtype=torch.bfloat16, device=x.device)
    call("mla_avgpool_tokens", _p(x), _p(y), B, gh, gw, C, cs)
    return y


def local_attn(q, kv, B, gh, gw, cs, heads, scale):
    C = q.shape[-1]
    out = torch.empty_like(q)
    call("mla_local_attn", _p(q), _p(kv), _p(out), B, gh, gw, C, cs, heads, float(scale))
    return out


# --------------------------------------------------------------------------------------------- generation heads
def gemm_batched(a, b, out, *, M, N, K, lda, ldb, ldc, a_mode=0, b_mode=0, alpha=1.0, n_outer, n_inner, sA, sB, sC):
    """out[o,i] = alpha * Aop[o,i] . Bop[o,i]^T over a two-level batch; a/b/out are base tensors (offset = data_ptr), strides in
    elements as (outer, inner) pairs. out may be bf16 or fp32."""
    _req(a, torch.bfloat16, "gemm_batched A")
    _req(b, torch.bfloat16, "gemm_batched B")
    out_fp32 = 1 if out.dtype == torch.float32 else 0
    if not out_fp32:
        _req(out, torch.bfloat16, "gemm_batched C")
    call("mla_gemm_batched_bf16", _p(a), _p(b), _p(out), M, N, K, lda, ldb, ldc, a_mode, b_mode, out_fp32, float(alpha), n_outer,
         n_inner, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1])
    return out


def softmax_rows_fwd(scores, nvalid, p, seed):
    ncols = scores.shape[-1]
    rows = scores.numel() // ncols
    P = torch.empty(scores.shape, dtype=torch.bfloat16, device=scores.device)
    Pd = torch.empty_like(P) if p > 0 else P
    call("mla_softmax_rows_fwd", _p(scores), _p(P), _p(Pd), rows, ncols, nvalid, float(p), seed)
    return P, Pd


def softmax_rows_bwd(dPd, P, nvalid, p, seed):
    ncols = P.shape[-1]
    dS = torch.empty_like(P)
    call("mla_softmax_rows_bwd", _p(dPd), 1 if dPd.dtype == torch.float32 else 0, _p(P), _p(dS), P.numel() // ncols, ncols, nvalid, float(p), seed)
    return dS


def dropout_fwd(x, residual, p, seed):
    y = torch.empty_like(x)
    call("mla_dropout_fwd", _p(x), _p(residual), _p(y), x.numel(), float(p), seed)
    return y


def dropout_bwd(dy, p, seed):
    dx = torch.empty_like(dy)
    call("mla_dropout_bwd", _p(dy), _p(dx), dy.numel(), float(p), seed)
    return dx


def scale_batch(x, scale):
    y = torch.empty_like(x)
    call("mla_scale_batch", _p(x), _p(scale), _p(y), x.shape[0], x.numel() // x.shape[0])
    return y


def layernorm_stats_fwd(x2d, w, b, eps):
    rows, H = x2d.shape
    y = torch.empty_like(x2d)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty_like(mean)
    call("mla_layernorm_stats_fwd", _p(x2d), _p(w), _p(b), _p(y), _p(mean), _p(rstd), rows, H, float(eps))
    return y, mean, rstd


def layernorm_bwd(dy2d, x2d, w, mean, rstd, dw=None, db=None, accumulate=False):
    rows, H = x2d.shape
    dx = torch.empty_like(x2d)
    nb = lib().mla_layernorm_bwd_blocks(rows)
    ws = workspace(nb * 2 * H * 4, x2d.device)
    call("mla_layernorm_bwd", _p(dy2d), _p(x2d), _p(w), _p(mean), _p(rstd), _p(dx), _p(dw), _p(db), 1 if accumulate else 0, rows, H,
         _p(ws), ws.numel())
    return dx


def seqmean_fwd(x3d):
    B, S, C = x3d.shape
    y = torch.empty((B, C), dtype=torch.bfloat16, device=x3d.device)
    call("mla_seqmean_fwd", _p(x3d), _p(y), B, S, C)
    return y


def seqmean_bwd(dy2d, S):
    B, C = dy2d.shape
    dx = torch.empty((B, S, C), dtype=torch.bfloat16, device=dy2d.device)
    call("mla_seqmean_bwd", _p(dy2d), _p(dx), B, S, C)
    return dx


def bn_bwd(dy2d, x2d, mean, var, w, eps, dw=None, db=None, accumulate=False):
    rows, C = x2d.shape
    dx = torch.empty_like(x2d)
    nb = lib().mla_bn_bwd_blocks(rows)
    ws = workspace((nb * 2 * C + 2 * C) * 4, x2d.device)
    call("mla_bn_bwd", _p(dy2d), _p(x2d), _p(mean), _p(var), _p(w), _p(dx), _p(dw), _p(db), 1 if accumulate else 0, rows, C, float(eps),
         _p(ws), ws.numel())
    return dx


def chamfer_fwd(pred, gt):
    B, N, _ = pred.shape
    M = gt.shape[1]
    dev = pred.device
    d1 = torch.empty((B, N), dtype=torch.float32, device=dev)
    i1 = torch.empty((B, N), dtype=torch.int32, device=dev)
    d2 = torch.empty((B, M), dtype=torch.float32, device=dev)
    i2 = torch.empty((B, M), dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ws = workspace(64, dev)
    call("mla_chamfer_fwd", _p(pred), _p(gt), _p(d1), _p(i1), _p(d2), _p(i2), _p(loss), B, N, M, _p(ws), ws.numel())
    return loss, d1, i1, d2, i2


def chamfer_bwd(pred, gt, d1, i1, d2, i2, gscale):
    B, N, _ = pred.shape
    dpred = torch.empty_like(pred)
    call("mla_chamfer_bwd", _p(pred), _p(gt), _p(d1), _p(i1), _p(d2), _p(i2), _p(gscale), _p(dpred), B, N, gt.shape[1])
    return dpred


def imgloss_fwd(delta_raw, curr, nxt, ps, clip):
    """delta_raw [B, npatch, ld] bf16 with ld >= 3*ps*ps (columns beyond are padding)."""
    B, ld = delta_raw.shape[0], delta_raw.shape[-1]
    fp32 = curr.dtype == torch.float32
    if curr.dtype != nxt.dtype or curr.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("imgloss: curr/next images must both be fp32 or both bf16")
    sums = torch.empty(3, dtype=torch.float32, device=delta_raw.device)
    ws = workspace(2048 * 3 * 4, delta_raw.device)
    call("mla_imgloss_fwd", _p(delta_raw), ld, _p(curr), _p(nxt), 1 if fp32 else 0, _p(sums), B, curr.shape[1], nxt.shape[1], curr.shape[2],
         ps, float(clip), _p(ws), ws.numel())
    return sums


def imgloss_bwd(delta_raw, curr, nxt, ps, clip, gscale):
    ld = delta_raw.shape[-1]
    out = torch.zeros_like(delta_raw) if ld != 3 * ps * ps else torch.empty_like(delta_raw)
    call("mla_imgloss_bwd", _p(delta_raw), ld, _p(curr), _p(nxt), 1 if curr.dtype == torch.float32 else 0, _p(gscale), _p(out),
         delta_raw.shape[0], curr.shape[1], nxt.shape[1], curr.shape[2], ps, float(clip))
    return out


def local_attn_bwd(q, kv, dout, B, gh, gw, cs, heads, scale):
    C = q.shape[1]
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    call("mla_local_attn_bwd", _p(q), _p(kv), _p(dout), _p(dq), _p(dkv), B, gh, gw, C, cs, heads, float(scale))
    return dq, dkv


def avgpool_tokens_bwd(dy, other, B, gh, gw, cs):
    C = dy.shape[1]
    dx = torch.empty((B * gh * gw, C), dtype=torch.bfloat16, device=dy.device)
    call("mla_avgpool_tokens_bwd", _p(dy), _p(other), _p(dx), B, gh, gw, C, cs)
    return dx


def imgroi_fwd(delta_raw, a_raw, o_raw, roi_u8, curr, nxt, ps, clip, shift):
    """sums[4] = ROI sum diff^2, ROI sum |diff|, background sum |diff|, sum |delta| (see mla_imgroi_fwd).
    delta_raw is [B, npatch, ld]; a_raw and o_raw are 2-D, [B * npatch, lda] and [B * npatch, ldo >= 2], one row per patch (as
    ops.ImageGenRoiLossFn passes them): stride(0) is taken as the row pitch, column 0 of a_raw and columns 0..1 of o_raw are read."""
    B, npatch, ld = delta_raw.shape
    if curr.dtype != nxt.dtype or curr.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("imgroi: curr/next images must both be fp32 or both bf16")
    sums = torch.empty(4, dtype=torch.float32, device=delta_raw.device)
    ws = workspace(B * npatch * 16, delta_raw.device)
    call("mla_imgroi_fwd", _p(delta_raw), ld, _p(a_raw), a_raw.stride(0), _p(o_raw), o_raw.stride(0), _p(roi_u8), _p(curr), _p(nxt),
         1 if curr.dtype == torch.float32 else 0, _p(sums), B, curr.shape[1], nxt.shape[1], curr.shape[2], ps, float(clip), float(shift), _p(ws),
         ws.numel())
    return sums


def imgroi_bwd(delta_raw, a_raw, o_raw, roi_u8, curr, nxt, ps, clip, shift, coef):
    """(ddelta_raw [B, npatch, ld] bf16 with the padding columns zeroed, dalpha_raw [B * npatch] fp32, doff_raw [B * npatch, 2] fp32).
    a_raw and o_raw are 2-D with one row per patch, exactly as in imgroi_fwd: stride(0) is the row pitch."""
    B, npatch, ld = delta_raw.shape
    dev = delta_raw.device
    dd = torch.empty_like(delta_raw)
    da = torch.empty(B * npatch, dtype=torch.float32, device=dev)
    do = torch.empty((B * npatch, 2), dtype=torch.float32, device=dev)
    call("mla_imgroi_bwd", _p(delta_raw), ld, _p(a_raw), a_raw.stride(0), _p(o_raw), o_raw.stride(0), _p(roi_u8), _p(curr), _p(nxt),
         1 if curr.dtype == torch.float32 else 0, _p(coef), _p(dd), _p(da), _p(do), B, curr.shape[1], nxt.shape[1], curr.shape[2], ps,
         float(clip), float(shift))
    return dd, da, do


def clip_preprocess(img_u8, bounds_h, coef_h, bounds_v, coef_v, OH, OW, mean, std, out_dtype=torch.float32, mask_channel=True):
    """img_u8 [B, H, W, 3] uint8 on the GPU -> [B, 3 (+1), OH, OW]; tables from mla_amd.vision_tokenizer.pil_resample_tables."""
    if img_u8.dtype != torch.uint8 or not img_u8.is_cuda:
        raise TypeError("clip_preprocess: uint8 CUDA tensor [B, H, W, 3] expected")
    B, H, W, _ = img_u8.shape
    out = torch.empty((B, 4 if mask_channel else 3, OH, OW), dtype=out_dtype, device=img_u8.device)
    m = (c_float * 3)(*[float(v) for v in mean])
    sd = (c_float * 3)(*[float(v) for v in std])
    call("mla_clip_preprocess", _p(img_u8.contiguous()), B, H, W, _p(bounds_h), _p(coef_h), coef_h.shape[1], _p(bounds_v), _p(coef_v),
         coef_v.shape[1], _p(out), 1 if out_dtype == torch.float32 else 0, OH, OW, m, sd, 1 if mask_channel else 0)
    return out


def lga_prep_bwd(drows, fps_idx, knn_idx, B, N, C):
    G, K = knn_idx.shape[1], knn_idx.shape[2]
    dfeats = torch.empty((B, N, C), dtype=torch.float32, device=drows.device)    # every element is written (gather form)
    call("mla_lga_prep_bwd", _p(drows), _p(fps_idx), _p(knn_idx), _p(dfeats), B, N, G, K, C)
    return dfeats


def maxpool_k_bwd(x2d, dy, groups, K):
    dx = torch.empty_like(x2d)
    call("mla_maxpool_k_bwd", _p(x2d), _p(dy), _p(dx), groups, K, x2d.shape[1])
    return dx
