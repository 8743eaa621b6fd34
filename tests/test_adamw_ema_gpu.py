"""MI355X: the weight average (EMA) folded into the AdamW launch -- mla_adamw_ema_step / mla_adamw_ema_step_groups -- and the
stand-alone pass mla_ema_update, bit for bit.

What is asserted per case (states of trunk_cases.adamw_state, an EMA start vector of its own seed with one quarter exact zeros and one
quarter of magnitude 1e-6):
  (a) p, m, v, p16 after the fused step == the plain step's from the same state;
  (b) ema == the numpy emulation fma32(one_minus, p_new, decay32 * ema) on the kernel's own new p (the product rounded, one fma; the
      fp32 master, never the bf16 copy; decay cast to fp32, 1 - decay formed in double and cast once);
  (c) ema == plain step followed by ema_update;
  (d) nothing outside [0, n) of the EMA buffer is written (NaN guard on both sides, as adamw_place keeps around the other arrays);
  (e) decay 1.0 leaves the EMA as it was, decay 0.0 makes it the new p.
Sizes are trunk_cases.ADAMW_N (4 / 4096 / 4100 reach the 16-byte kernel through mla_adamw_ema_step, the others through _step_groups with
n_decay = n - n % 4 and a scalar tail; n_decay = 5 cuts a group: scalar kernel), layouts those of adamw_place with the EMA array aligned
and at offset 1 (offset 1 alone must send an otherwise aligned case to the scalar kernel)."""
import ctypes

import pytest
import torch

import trunk_cases as T
from conftest import poison_free_memory
from ema_cases import DECAYS, ema_emul32, ema_start

pytestmark = pytest.mark.gpu
BF, F32 = T.BF, T.F32
STEP, WD = 3, 0.01


def _hip():
    from mla_amd import hip
    return hip


def place_ema(e0, off, dev):
    buf = torch.full((e0.numel() + 8,), float("nan"), dtype=F32, device=dev)
    view = buf[off:off + e0.numel()]
    view.copy_(e0)
    return view


def guard_intact(t):
    base, off, n = t._base, t.storage_offset(), t.numel()
    return bool(torch.isnan(base[:off]).all()) and bool(torch.isnan(base[off + n:]).all())


def run_case(hip, st, e0, n, layout, ema_off, n_decay, gs_t, decay):
    """One fused step, one plain step and one plain step + ema_update from the same state; asserts (a) - (e)."""
    dev = st[0].device
    h = T.ADAMW_HYPER
    hyper = (h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, gs_t)
    src = tuple(t[:n] for t in st)
    ctx = (n, layout, ema_off, n_decay, gs_t is not None, decay)
    (p, g, m, v), p16 = T.adamw_place(*src, layout, dev)          # fused
    (q, gq, mq, vq), q16 = T.adamw_place(*src, layout, dev)       # plain (+ the stand-alone pass)
    ema, ema2 = place_ema(e0[:n], ema_off, dev), place_ema(e0[:n], ema_off, dev)
    if n_decay is None:
        hip.adamw_ema_step(p, g, m, v, ema, p16, *hyper, decay)
        hip.adamw_step(q, gq, mq, vq, q16, *hyper)
    else:
        hip.adamw_ema_step_groups(p, g, m, v, ema, p16, n_decay, *hyper, decay)
        hip.adamw_step_groups(q, gq, mq, vq, q16, n_decay, *hyper)
    hip.ema_update(ema2, q, decay)
    # (a)
    assert T.bits_equal(p, q) and T.bits_equal(m, mq) and T.bits_equal(v, vq), (ctx, "p / m / v differ from the plain step")
    assert (p16 is None) == (q16 is None) and (p16 is None or T.bits_equal(p16, q16)), (ctx, "p16 differs from the plain step")
    assert p16 is None or T.bits_equal(p16, p.to(BF)), (ctx, "p16 is bf16 of the new master")
    assert T.bits_equal(g, src[1]), (ctx, "the gradient is read only")
    # (b)
    want = ema_emul32(e0[:n], p, decay).to(dev)
    assert T.bits_equal(ema, want), (ctx, "ema differs from the emulation", int((ema != want).sum()))
    # (c)
    assert T.bits_equal(ema2, ema), (ctx, "fused ema differs from step + ema_update")
    # (d)
    for t in (p, g, m, v, ema, ema2) + ((p16,) if p16 is not None else ()):
        assert guard_intact(t), (ctx, "wrote outside its range")
    # (e)
    if decay == 1.0:
        assert T.bits_equal(ema, e0[:n].to(dev)), (ctx, "decay 1: the average must not move")
    if decay == 0.0:
        assert T.bits_equal(ema, p), (ctx, "decay 0: the average is the new master")


_STATE = {}


def _state(family, dev):
    if family not in _STATE:
        n = max(T.ADAMW_N)
        _STATE[family] = (tuple(t.to(dev) for t in T.adamw_state(family, n)), ema_start(family, n))
    return _STATE[family]


@pytest.mark.parametrize("family", T.ADAMW_FAMILIES)
def test_adamw_ema(dev, family):
    hip = _hip()
    st, e0 = _state(family, dev)
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    poison_free_memory()
    cases = vec = 0
    for n in T.ADAMW_N:
        boundaries = [None, n - n % 4] + ([5] if n >= 5 else [])
        for layout in T.ADAMW_LAYOUTS:                      # with and without p16, aligned and not
            for ema_off in (0, 1):
                for n_decay in boundaries:
                    for decay in DECAYS:
                        for gs in (None, gs_t):
                            run_case(hip, st, e0, n, layout, ema_off, n_decay, gs, decay)
                            cases += 1
                            vec += int(ema_off == 0 and T.adamw_all_vector(layout, n, n_decay))
    assert vec >= 40 and cases - vec >= 40, (cases, vec)     # both kernels were exercised


def test_ema_update_layouts(dev):
    """The stand-alone pass on its own: 16-byte groups + scalar tail where both pointers are aligned, the scalar kernel otherwise."""
    hip = _hip()
    st, e0 = _state("unit", dev)
    poison_free_memory()
    for n in T.ADAMW_N:
        for p_off in (0, 1):
            for e_off in (0, 1):
                for decay in DECAYS:
                    p = place_ema(st[0][:n], p_off, dev)
                    ema = place_ema(e0[:n], e_off, dev)
                    hip.ema_update(ema, p, decay)
                    assert T.bits_equal(p, st[0][:n]) and guard_intact(p) and guard_intact(ema), (n, p_off, e_off, decay)
                    assert T.bits_equal(ema, ema_emul32(e0[:n], st[0][:n], decay).to(dev)), (n, p_off, e_off, decay)


def test_adamw_ema_past_the_grid_cap(dev):
    """The capped-grid chunked walk with the EMA stream: n = ADAMW_N_CAPPED + 3 through mla_adamw_ema_step_groups with n_decay = n - 7
    (8192 blocks, a chunk of 1024 groups each, a three-element scalar tail), and the same size through mla_ema_update."""
    hip = _hip()
    n = T.ADAMW_N_CAPPED + 3
    n_decay = n - 7
    assert T.adamw_all_vector("aligned", n, n_decay) and n // 4 > 8192 * 256 and n % 4 == 3
    st = tuple(t.to(dev) for t in T.adamw_state("unit", n, tag="big"))
    e0 = ema_start("big", n)
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    poison_free_memory()
    run_case(hip, st, e0, n, "aligned", 0, n_decay, gs_t, 0.9999)


def test_invalid_arguments(dev):
    """ema == NULL, n < 0 and a decay outside [0, 1] return the library's invalid-argument code (-1) and launch nothing: there is no
    silent plain step. The Python wrappers refuse an out-of-range decay before the call."""
    hip = _hip()
    L = hip.lib()
    n = 64
    st = tuple(t.to(dev) for t in T.adamw_state("unit", n))
    p, g, m, v = (t.clone() for t in st)
    ema = ema_start("unit", n).to(dev)
    before = [t.clone() for t in (p, g, m, v, ema)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    h = T.ADAMW_HYPER
    hy = (h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, None)

    def step(e, nn, d, omd):
        return L.mla_adamw_ema_step(ptr(p), ptr(g), ptr(m), ptr(v), e, None, nn, *hy, d, omd, None)

    def groups(e, nn, d, omd):
        return L.mla_adamw_ema_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), e, None, nn, 8, *hy, d, omd, None)

    for fn in (step, groups):
        assert fn(None, n, 0.5, 0.5) == -1
        assert fn(None, 0, 0.5, 0.5) == -1
        assert fn(ptr(ema), -1, 0.5, 0.5) == -1
        for d, omd in ((1.5, 0.0), (-0.25, 1.0), (0.5, 1.5), (0.5, -0.5), (float("nan"), 0.5)):
            assert fn(ptr(ema), n, d, omd) == -1, (d, omd)
    assert L.mla_ema_update(None, ptr(p), n, 0.5, 0.5, None) == -1
    assert L.mla_ema_update(ptr(ema), None, n, 0.5, 0.5, None) == -1
    assert L.mla_ema_update(ptr(ema), ptr(p), -1, 0.5, 0.5, None) == -1
    for d, omd in ((1.5, 0.0), (-0.25, 1.0), (0.5, 1.5), (float("nan"), 0.5)):
        assert L.mla_ema_update(ptr(ema), ptr(p), n, d, omd, None) == -1, (d, omd)
    assert b"decay" in L.mla_last_error()
    for bad in (1.5, -0.1):
        with pytest.raises(ValueError):
            hip.ema_update(ema, p, bad)
        with pytest.raises(ValueError):
            hip.adamw_ema_step(p, g, m, v, ema, None, *hy, bad)
        with pytest.raises(ValueError):
            hip.adamw_ema_step_groups(p, g, m, v, ema, None, 8, *hy, bad)
    torch.cuda.synchronize()
    assert all(T.bits_equal(a, b) for a, b in zip((p, g, m, v, ema), before)), "a refused call wrote something"
    assert L.mla_ema_update(ptr(ema), ptr(p), 0, 0.5, 0.5, None) == 0          # n == 0 is valid and a no-op
