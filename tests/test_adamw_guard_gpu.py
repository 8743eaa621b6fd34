"""MI355X: the two entry points of the skip_nonfinite guard (include/mla_hip_optim.h) against the entry points they wrap, bit for bit.

mla_clip_coef_guard over guard_cases.CLIP_CASES: a finite sumsq gives mla_clip_coef's coef and norm and flag 0; +inf and NaN give
flag 1, coef 0 and the non-finite norm (all also equal to the numpy model).

mla_adamw_guard_step over trunk_cases.ADAMW_N (n < 4 and n % 4 != 0 included: the scalar kernel and the tail run) x placements
{aligned, every stream offset by one element} x moments {fp32, bf16} x every combination of p16 / grad_scale / ema x n_decay in
{n, n - n % 4, 5}, NaN guard zones on both sides of every stream:
  flag 0: every stream equals what mla_adamw_step_groups / mla_adamw_ema_step_groups (fp32 moments) or mla_adamw_m16_step (bf16) leaves
          from the same state, and the guard zones are intact;
  flag 1: every stream and every guard zone is unchanged -- also with inf in g at element 0, at element n - 1 and inside the n % 4 tail."""
import ctypes

import numpy as np
import pytest
import torch

import adamw_m16_cases as M
import guard_cases as GC
import trunk_cases as T
from conftest import poison_free_memory
from ema_cases import ema_start

pytestmark = pytest.mark.gpu
BF, F32 = T.BF, T.F32
STEP, WD, DECAY, BASE = 3, 0.01, 0.9999, 8
FLAGS = [(p16, gs, ema) for p16 in (True, False) for gs in (True, False) for ema in (True, False)]
_STATE = {}


def _hip():
    from mla_amd import hip
    return hip


def _state(moments, dev):
    """(p, g, m, v, ema) of the largest size, on the device; built once and never written."""
    if moments not in _STATE:
        n = max(T.ADAMW_N)
        p, g, m, v = M.m16_state("unit", n) if moments == "bf16" else T.adamw_state("unit", n)
        _STATE[moments] = tuple(t.to(dev) for t in (p, g, m, v, ema_start("unit", n)))
    return _STATE[moments]


def place(t, off, n=None, dtype=None):
    """t[:n] (or, for t = None, n NaNs) as a view at element offset `off` of a NaN-filled buffer."""
    buf = torch.full((n + 8,), float("nan"), dtype=dtype or t.dtype, device="cuda")
    view = buf[off:off + n]
    if t is not None:
        view.copy_(t[:n])
    return view


def same_buffer(a, b):
    """the whole underlying buffers, guard zones included, bit for bit"""
    if a is None or b is None:
        return a is None and b is None
    return T.bits_equal(a._base, b._base)


def streams(st, n, off, with_p16, with_ema):
    p, g, m, v, e = st
    return [place(p, off, n), place(g, off, n), place(m, off, n), place(v, off, n), place(e, off, n) if with_ema else None,
            place(None, off, n, BF) if with_p16 else None]


def unguarded(hip, s, n_decay, gs_t):
    p, g, m, v, ema, p16 = s
    h = T.ADAMW_HYPER
    hy = (h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, gs_t)
    if m.dtype == BF:
        hip.adamw_m16_step(p, g, m, v, ema, p16, n_decay, *hy, DECAY, M.SEED, BASE)
    elif ema is not None:
        hip.adamw_ema_step_groups(p, g, m, v, ema, p16, n_decay, *hy, DECAY)
    else:
        hip.adamw_step_groups(p, g, m, v, p16, n_decay, *hy)


def guarded(hip, s, n_decay, gs_t, flag):
    p, g, m, v, ema, p16 = s
    h = T.ADAMW_HYPER
    hip.adamw_guard_step(p, g, m, v, ema, p16, n_decay, h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, gs_t, DECAY, M.SEED, BASE, flag)


def test_clip_coef_guard(dev):
    hip = _hip()
    for sumsq, max_norm in GC.CLIP_CASES:
        ss = torch.tensor([sumsq], dtype=F32, device=dev)
        out = torch.full((3,), float("nan"), dtype=F32, device=dev)                     # [coef, norm, sentinel]
        ref = torch.full((3,), float("nan"), dtype=F32, device=dev)
        flag = torch.full((3,), -7, dtype=torch.int32, device=dev)
        hip.clip_coef_guard(ss, max_norm, out[0:1], out[1:2], flag[1:2])
        hip.clip_coef(ss, max_norm, ref[0:1], ref[1:2])
        coef, nrm, skip = GC.clip_coef_guard_model(sumsq, max_norm)
        got, want, fl = out.cpu(), ref.cpu(), flag.cpu().tolist()
        print(f"sumsq={sumsq} max_norm={max_norm}: coef={float(got[0])} norm={float(got[1])} skip={fl[1]} (clip_coef: {float(want[0])}, {float(want[1])})")
        assert fl[0] == fl[2] == -7 and torch.isnan(got[2]), "wrote outside its three outputs"
        assert fl[1] == skip == int(not np.isfinite(sumsq))
        assert T.bits_equal(got[1:2], want[1:2]) and T.bits_equal(got[1:2], torch.from_numpy(np.asarray([nrm])))
        if skip:
            assert float(got[0]) == 0.0 and not np.signbit(float(got[0])) and not torch.isfinite(got[1])
        else:
            assert T.bits_equal(got[0:1], want[0:1]) and T.bits_equal(got[0:1], torch.from_numpy(np.asarray([coef])))
    hip.clip_coef_guard(ss, 1.0, out[0:1], None, flag[1:2])                             # norm_out may be NULL, as in mla_clip_coef
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        hip.clip_coef_guard(ss, 1.0, out[0:1], out[1:2], flag[1:2].float())


@pytest.mark.parametrize("moments", ["fp32", "bf16"])
def test_adamw_guard(dev, moments):
    hip = _hip()
    st = _state(moments, dev)
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    flags = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    go, skip = flags[0:1], flags[1:2]
    poison_free_memory()
    cases = 0
    for n in T.ADAMW_N:
        for n_decay in sorted({n, n - n % 4} | ({5} if n >= 5 else set())):
            for off in (0, 1):
                for with_p16, with_gs, with_ema in FLAGS:
                    ctx = (moments, n, n_decay, off, with_p16, with_gs, with_ema)
                    g_t = gs_t if with_gs else None
                    start = streams(st, n, off, with_p16, with_ema)
                    want = streams(st, n, off, with_p16, with_ema)
                    unguarded(hip, want, n_decay, g_t)
                    got = streams(st, n, off, with_p16, with_ema)
                    guarded(hip, got, n_decay, g_t, go)
                    for name, a, b in zip("p g m v ema p16".split(), got, want):
                        assert same_buffer(a, b), (ctx, name, "flag 0 differs from the unguarded entry point")
                    assert not T.bits_equal(got[0], start[0]) or n < 4, (ctx, "flag 0 did not step")
                    for pos in GC.bad_positions(n):
                        held = streams(st, n, off, with_p16, with_ema)
                        held[1][pos] = float("inf")
                        keep = [None if t is None else t._base.clone() for t in held]
                        guarded(hip, held, n_decay, g_t, skip)
                        for name, a, b in zip("p g m v ema p16".split(), held, keep):
                            assert a is None or T.bits_equal(a._base, b), (ctx, name, pos, "flag 1 wrote something")
                    cases += 1
    assert cases == 2 * 8 * sum(len({n, n - n % 4} | ({5} if n >= 5 else set())) for n in T.ADAMW_N)
    assert flags.tolist() == [0, 1]


def test_guard_wrapper_refusals(dev):
    hip = _hip()
    n = 64
    p, g, m, v, _ = (t[:n].clone() for t in _state("fp32", dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (p, g, m, v)]
    args = (None, None, n, 2e-5, 0.9, 0.999, 1e-8, WD, STEP, None, DECAY, 0, 0)
    with pytest.raises(TypeError):
        hip.adamw_guard_step(p, g, m, v.to(BF), *args, flag)                            # moments of two formats
    with pytest.raises(TypeError):
        hip.adamw_guard_step(p, g, m.double(), v.double(), *args, flag)
    with pytest.raises(TypeError):
        hip.adamw_guard_step(p, g, m, v, *args, flag.long())
    L = hip.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.mla_adamw_guard_step(ptr(p), ptr(g), ptr(m), ptr(v), None, None, n, n, 2e-5, 0.9, 0.999, 1e-8, WD, STEP, None, 0.0, 0.0, 0, 0, 0,
                                  None, None) == -1
    torch.cuda.synchronize()
    assert all(T.bits_equal(a, b) for a, b in zip((p, g, m, v), before)), "a refused call wrote something"
