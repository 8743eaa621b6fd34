"""Inputs, the fp32 emulation and the fp64 reference of the weight average (EMA) -- ema_elem of mla_amd/csrc/elementwise.hip,
e = fma(one_minus_decay, p, decay * e) -- shared by tests/test_adamw_ema_gpu.py and tests/test_ema_cases_host.py.

Bound of the emulation (and so of the kernel, which equals it bit for bit) against the update evaluated in fp64 with the two factors
as the ABI carries them: the product decay * e is rounded once (<= U32 |decay e|), the fma once (<= U32 |result| <= U32 (|decay e| +
|one_minus p|)): 2 U32 (|decay e| + |one_minus p|), i.e. 2 ulp, plus one subnormal spacing per rounding where the terms are that small."""
import numpy as np
import torch

import trunk_cases as T

DECAYS = (0.9999, 0.0, 1.0)


def ema_start(family, n):
    """fp32 [n] from its own seed: of every four elements one exactly 0 and one of magnitude 1e-6 (like adamw_state's p, at other
    positions: p has them at k == 1 and k == 2)."""
    e = torch.randn(n, generator=T._gen("adamw_ema", family))
    k = torch.arange(n) % 4
    return torch.where(k == 0, torch.zeros(n), torch.where(k == 3, e * 1e-6, e))


def ema_factors32(decay):
    """(decay, 1 - decay) as the wrappers hand them to the library: decay cast to fp32; 1 - decay formed in double, cast once."""
    return np.float32(decay), np.float32(1.0 - float(decay))


def ema_emul32(e, p_new, decay, factors=None):
    """The kernel's arithmetic in numpy fp32. `factors` overrides (decay32, one_minus32) -- for deliberately wrong emulations."""
    f = np.float32
    d32, omd = ema_factors32(decay) if factors is None else factors
    e, p_new = e.cpu().numpy().astype(f), p_new.cpu().numpy().astype(f)
    return torch.from_numpy(T._fma32(np.full_like(e, omd), p_new, f(d32) * e))


def ema_ref64(e, p_new, decay):
    """The update in fp64 from the fp32 state, the factors rounded to fp32 first. Returns (value, bound)."""
    d32, omd = (float(x) for x in ema_factors32(decay))
    e, p_new = e.to(T.F64), p_new.to(T.F64)
    a, b = d32 * e, omd * p_new
    return a + b, 2 * T.U32 * (a.abs() + b.abs()) + 2 * 2.0 ** -149


def ema_ratio(got, ref, bound):
    g = got.to(T.F64)
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, T.INF))
    return float(T._ratio(err, bound).max()) if err.numel() else 0.0
