"""MI355X: the AdamW step with bf16 moments and stochastic rounding -- mla_adamw_m16_step (include/mla_hip_optim.h) -- against the
numpy model of tests/adamw_m16_cases.py, bit for bit.

What is asserted per case of the main matrix (states of trunk_cases.adamw_state with the moments rounded to bf16):
  (1) m16, v16 == the emulation's (Philox word of the element's GLOBAL index, stochastic rounding of the unrounded fp32 moment);
  (2) p == the emulation's (adamw_emul32's arithmetic on the decoded moments; p comes from the unrounded moments);
  (3) p16 == bf16(p);  (4) ema == ema_emul32 on the kernel's own new p;  (5) g is unchanged;
  (6) nothing outside [0, n) of any buffer is written (NaN guards on both sides of every stream, the bf16 ones included).
Sizes are trunk_cases.ADAMW_N; n_decay in {n, n - n % 4, 5}; index_base in {0, 8, 3, 2^34 + 4} (3 sends everything to the scalar kernel);
placements: all streams aligned, all offset by one element, and each stream alone offset by one element (which alone must send the
case to the scalar kernel). The aligned and the all-offset placements run every combination of p16 / grad_scale / ema, the
single-stream placements rotate through them."""
import ctypes

import numpy as np
import pytest
import torch

import adamw_m16_cases as M
import trunk_cases as T
from conftest import poison_free_memory
from ema_cases import ema_emul32, ema_start

pytestmark = pytest.mark.gpu
BF, F32 = T.BF, T.F32
STEP, WD, DECAY = 3, 0.01, 0.9999
STREAMS = ("p", "g", "m16", "v16", "p16", "ema")
LAYOUTS = ("aligned", "offset1") + tuple(s + "_off" for s in STREAMS)
FLAGS = [(p16, gs, ema) for p16 in (True, False) for gs in (True, False) for ema in (True, False)]


def _hip():
    from mla_amd import hip
    return hip


def place(t, off, dev, dtype=None):
    """`t` (or, for t = an int, that many NaNs) as a view at element offset `off` of a NaN-filled buffer."""
    n = t if isinstance(t, int) else t.numel()
    buf = torch.full((n + 8,), float("nan"), dtype=dtype or t.dtype, device=dev)
    view = buf[off:off + n]
    if not isinstance(t, int):
        view.copy_(t)
    return view


def guard_intact(t):
    base, off, n = t._base, t.storage_offset(), t.numel()
    return bool(torch.isnan(base[:off]).all()) and bool(torch.isnan(base[off + n:]).all())


def offsets(layout):
    return {s: int(layout == "offset1" or layout == s + "_off") for s in STREAMS}


def is_vector(layout, n, n_decay, index_base, with_p16, with_ema):
    """True when the 16-byte kernel is launched: every PRESENT stream aligned, n >= 4, neither the decay boundary nor the Philox
    counter cuts a group of four."""
    off = offsets(layout)
    used = [s for s in STREAMS if (s != "p16" or with_p16) and (s != "ema" or with_ema)]
    return n >= 4 and n_decay % 4 == 0 and index_base % 4 == 0 and not any(off[s] for s in used)


_STATE, _EMUL = {}, {}


def _state(family, dev, n=None, tag=0):
    key = (family, tag)
    if key not in _STATE:
        n = n or max(T.ADAMW_N)
        _STATE[key] = (M.m16_state(family, n, tag), ema_start(family if tag == 0 else tag, n))
    return _STATE[key]


def _emul(family, tag, st, n, n_decay, index_base, gs, dev, seed=M.SEED, step=STEP):
    """The emulated step of a case (shared by every placement and flag combination of it), kept on the device."""
    key = (family, tag, n, n_decay, index_base, gs, seed, step)
    if key not in _EMUL:
        out = M.adamw_m16_emul32(*(t[:n] for t in st), step, WD, gs, n_decay=n_decay, seed=seed, index_base=index_base, **T.ADAMW_HYPER)
        _EMUL[key] = tuple(t.to(dev) for t in out)
    return _EMUL[key]


def run_case(hip, family, tag, st, e0, n, layout, n_decay, index_base, with_p16, gs_t, with_ema, dev):
    off = offsets(layout)
    ctx = (family, n, layout, n_decay, index_base, with_p16, gs_t is not None, with_ema)
    h = T.ADAMW_HYPER
    p, g, m16, v16 = (place(t[:n], off[s], dev) for t, s in zip(st, STREAMS))
    p16 = place(n, off["p16"], dev, BF) if with_p16 else None
    ema = place(e0[:n], off["ema"], dev) if with_ema else None
    hip.adamw_m16_step(p, g, m16, v16, ema, p16, n_decay, h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, gs_t, DECAY, M.SEED, index_base)
    want_p, want_m, want_v, _, _ = _emul(family, tag, st, n, n_decay, index_base, T.ADAMW_GS if gs_t is not None else None, dev)
    assert T.bits_equal(m16, want_m), (ctx, "m16 differs from the emulation", int((m16.view(torch.int16) != want_m.view(torch.int16)).sum()))
    assert T.bits_equal(v16, want_v), (ctx, "v16 differs from the emulation", int((v16.view(torch.int16) != want_v.view(torch.int16)).sum()))
    assert T.bits_equal(p, want_p), (ctx, "p differs from the emulation", int((p != want_p).sum()))
    assert p16 is None or T.bits_equal(p16, p.to(BF)), (ctx, "p16 is bf16 of the new master")
    if with_ema:
        want_e = ema_emul32(e0[:n], p, DECAY).to(dev)
        assert T.bits_equal(ema, want_e), (ctx, "ema differs from the emulation", int((ema != want_e).sum()))
    assert T.bits_equal(g, st[1][:n].to(dev)), (ctx, "the gradient is read only")
    for t in (p, g, m16, v16) + ((p16,) if with_p16 else ()) + ((ema,) if with_ema else ()):
        assert guard_intact(t), (ctx, "wrote outside its range")


@pytest.mark.parametrize("family", T.ADAMW_FAMILIES)
def test_adamw_m16(dev, family):
    hip = _hip()
    st, e0 = _state(family, dev)
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    poison_free_memory()
    cases = vec = rot = 0
    for n in T.ADAMW_N:
        for n_decay in sorted({n, n - n % 4} | ({5} if n >= 5 else set())):
            for index_base in M.INDEX_BASES:
                for layout in LAYOUTS:
                    if layout in ("aligned", "offset1"):
                        flags = FLAGS
                    else:       # a single stream off: it has to be present; the other switches rotate
                        rot += 1
                        f = FLAGS[rot % 8]
                        flags = [(f[0] or layout == "p16_off", f[1], f[2] or layout == "ema_off")]
                    for with_p16, with_gs, with_ema in flags:
                        run_case(hip, family, 0, st, e0, n, layout, n_decay, index_base, with_p16, gs_t if with_gs else None, with_ema, dev)
                        cases += 1
                        vec += int(is_vector(layout, n, n_decay, index_base, with_p16, with_ema))
    assert vec >= 40 and cases - vec >= 40, (cases, vec)     # both kernels were exercised


def _step(hip, st, n, dev, n_decay=None, index_base=0, seed=M.SEED, step=STEP, lo=0, gs_t=None):
    """One m16 launch over elements [lo, lo + n) of the state, fresh aligned copies; returns (p, m16, v16)."""
    h = T.ADAMW_HYPER
    p, g, m16, v16 = (t[lo:lo + n].to(dev).clone() for t in st)
    hip.adamw_m16_step(p, g, m16, v16, None, None, n if n_decay is None else n_decay, h["lr"], h["beta1"], h["beta2"], h["eps"], WD, step,
                       gs_t, 0.0, seed, index_base)
    return p, m16, v16


def _within_one_ulp16(stored, full):
    d = np.abs(stored.float().cpu().numpy().astype(np.float64) - full.cpu().numpy().astype(np.float64))
    return bool((d <= M.ulp16_of(full.cpu().numpy())).all())


def test_consistent_with_the_fp32_step(dev):
    """From the same state (moments exactly representable in bf16) the new p is bit-identical to mla_adamw_step_groups' wherever the
    fp32 moments need no rounding -- and in fact everywhere, since p comes from the unrounded moments; the stored moments lie within
    one bf16 spacing of the fp32 step's."""
    hip = _hip()
    n, n_decay = 4100, 3000
    st, _ = _state("unit", dev)
    st = [t[:n].clone() for t in st]
    for t in st[1:]:
        t[::3] = 0.0                 # g = m = v = 0: the new moments are exactly 0 and need no rounding
    h = T.ADAMW_HYPER
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    p, m16n, v16n = _step(hip, st, n, dev, n_decay=n_decay, gs_t=gs_t)
    q, g, m, v = st[0][:n].to(dev).clone(), st[1][:n].to(dev).clone(), st[2][:n].to(dev).float(), st[3][:n].to(dev).float()
    hip.adamw_step_groups(q, g, m, v, None, n_decay, h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, gs_t)
    exact = (m.to(BF).float() == m) & (v.to(BF).float() == v)
    assert n // 3 <= int(exact.sum()) < n
    assert T.bits_equal(p[exact], q[exact]), "p differs from the fp32 step where the moments need no rounding"
    assert T.bits_equal(m16n[exact], m.to(BF)[exact]) and T.bits_equal(v16n[exact], v.to(BF)[exact]), "an exact moment was moved"
    assert T.bits_equal(p, q), "p comes from the unrounded moments: equal to the fp32 step everywhere"
    assert _within_one_ulp16(m16n, m) and _within_one_ulp16(v16n, v)


def test_split_invariance_and_reruns(dev):
    hip = _hip()
    n, n_decay, base = 4100, 3000, 2 ** 34 + 4
    st, _ = _state("unit", dev)
    whole = _step(hip, st, n, dev, n_decay=n_decay, index_base=base)
    for cut in (2048, 1001):
        a = _step(hip, st, cut, dev, n_decay=min(n_decay, cut), index_base=base)
        b = _step(hip, st, n - cut, dev, n_decay=max(n_decay - cut, 0), index_base=base + cut, lo=cut)
        for w, x, y in zip(whole, a, b):
            assert T.bits_equal(w, torch.cat([x, y])), cut
    again = _step(hip, st, n, dev, n_decay=n_decay, index_base=base)
    assert all(T.bits_equal(a, b) for a, b in zip(whole, again)), "two runs with the same seed differ"
    # another seed or another step: other moments, p within the envelope of moments one bf16 spacing apart
    full_m, full_v = _emul("unit", "split", st, n, n_decay, base, None, dev)[3:]
    for kw in (dict(seed=M.SEED + 1), dict(step=STEP + 1)):
        other = _step(hip, st, n, dev, n_decay=n_decay, index_base=base, **kw)
        assert not T.bits_equal(other[1], whole[1]) and not T.bits_equal(other[2], whole[2]), kw
        if "seed" in kw:
            assert T.bits_equal(other[0], whole[0]), "p does not depend on the random bits of the same step"
            assert _within_one_ulp16(other[1], full_m) and _within_one_ulp16(other[2], full_v)
        else:
            fm, fv = _emul("unit", "split", st, n, n_decay, base, None, dev, step=STEP + 1)[3:]
            assert _within_one_ulp16(other[1], fm) and _within_one_ulp16(other[2], fv)


def test_adamw_m16_past_the_grid_cap(dev):
    """The capped-grid chunked walk: n = ADAMW_N_CAPPED + 3 with n_decay = n - 7 (8192 blocks, a chunk of 1024 groups each, a
    three-element scalar tail whose Philox counters continue the vector part's)."""
    hip = _hip()
    n = T.ADAMW_N_CAPPED + 3
    n_decay = n - 7
    assert n // 4 > 8192 * 256 and n % 4 == 3
    st, e0 = _state("unit", dev, n=n, tag="big")
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    poison_free_memory()
    assert is_vector("aligned", n, n_decay, 2 ** 34 + 4, True, True)
    run_case(hip, "unit", "big", st, e0, n, "aligned", n_decay, 2 ** 34 + 4, True, gs_t, True, dev)


def test_invalid_arguments(dev):
    """Every listed violation returns the library's invalid-argument code (-1) and launches nothing; n == 0 is a valid no-op; the
    wrapper refuses fp32 moment tensors and an out-of-range decay."""
    hip = _hip()
    L = hip.lib()
    n = 64
    st, e0 = _state("unit", dev)
    p, g, m16, v16 = (t[:n].to(dev).clone() for t in st)
    ema = e0[:n].to(dev)
    before = [t.clone() for t in (p, g, m16, v16, ema)]
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    h = T.ADAMW_HYPER
    hy = (h["lr"], h["beta1"], h["beta2"], h["eps"], WD)

    def call(p_=p, g_=g, m_=m16, v_=v16, e_=None, n_=n, nd=n, step=STEP, d=0.5, omd=0.5, base=0):
        return L.mla_adamw_m16_step(ptr(p_), ptr(g_), ptr(m_), ptr(v_), ptr(e_), None, n_, nd, *hy, step, None, d, omd, M.SEED, base, None)

    for kw in (dict(p_=None), dict(g_=None), dict(m_=None), dict(v_=None), dict(n_=-1, nd=0), dict(step=0), dict(nd=-1), dict(nd=n + 1),
               dict(base=-1)):
        assert call(**kw) == -1, kw
    for d, omd in ((1.5, 0.0), (-0.25, 1.0), (0.5, 1.5), (0.5, -0.5), (float("nan"), 0.5), (0.5, float("nan"))):
        assert call(e_=ema, d=d, omd=omd) == -1, (d, omd)
    assert b"decay" in L.mla_last_error()
    assert call(n_=0, nd=0) == 0
    args = (n, h["lr"], h["beta1"], h["beta2"], h["eps"], WD, STEP, None)
    with pytest.raises(TypeError):
        hip.adamw_m16_step(p, g, m16.float(), v16, None, None, *args, 0.5, M.SEED, 0)
    with pytest.raises(TypeError):
        hip.adamw_m16_step(p, g, m16, v16.float(), None, None, *args, 0.5, M.SEED, 0)
    for bad in (1.5, -0.1):
        with pytest.raises(ValueError):
            hip.adamw_m16_step(p, g, m16, v16, ema, None, *args, bad, M.SEED, 0)
    torch.cuda.synchronize()
    assert all(T.bits_equal(a, b) for a, b in zip((p, g, m16, v16, ema), before)), "a refused call wrote something"
