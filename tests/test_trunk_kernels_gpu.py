"""Per-element parity of the HBM-bound kernels every training step runs -- mla_rmsnorm_fwd / _prep / _bwd / _apply_t,
mla_timm_rmsnorm_fwd / _bwd, mla_layernorm_fwd, mla_swiglu_fwd / _bwd and their _t / _dual forms, mla_act_fwd / _bwd, mla_rope_inplace,
mla_cast_*, mla_add_bf16, mla_colsum_bf16, mla_sumsq_f32, mla_sum_partials, mla_clip_coef, mla_adamw_step / _step_groups, mla_ce_fwd,
mla_infonce_bwd, mla_l2norm_fwd / _bwd -- each called through its mla_amd.hip wrapper against the fp64 references of
tests/trunk_cases.py. Every tolerance is a bound function of that module (its docstring states the rules); every test prints its worst
|err| / bound. The free pool is NaN-filled before every launch group: the wrappers return torch.empty buffers, and an element a
kernel skips must not inherit a correct value an earlier launch left behind.

Which case takes which path (dispatch conditions in elementwise.hip / loss.hip):
  rmsnorm_bwd_kernel<2> / <4>      H <= 4096 / H in {4104, 8192}; rows > 512 walk several rows per workgroup with the prefetch running
                                   past the end (513: one workgroup has two rows; 1061: a ragged second and third pass; 1536: three each)
  reduce_partials_kernel           unrolled loop only: P = 512, 64 (every lane); unrolled + tail: P = 511 (the (511, 136) backward) and P = 63
                                   (colsum, 16383 rows), in row lane 15; tail only: P <= 48 (P = 37, 1; colsum rs = 1, 2)
  NORM_MAXC chunks                 H = 2056 / 4104: the last 256-lane chunk holds one 16-byte piece; H = 8: one lane works
  colsum_partial_vec_kernel        contig and aligned_slice at N % 8 == 0; colsum_partial_kernel: N in {1, 7}, odd_slice, ld_odd
                                   rows < 512: one row slice; 16383: 63 slices; 16384 / 16640: the 64-slice cap (per = 256 / 260)
  sumsq_partial_kernel             n < 4: tail only; 4195333: 2048 blocks x 256 lanes x 4 = 2097152 < n, the grid-stride loop runs twice
  sum_final_kernel                 aligned: 16-byte loads (+ unrolled loop at n = 4099) and tail; buf[1:]: the scalar walk
  adamw_vec4_kernel / adamw_kernel the 16-byte kernel needs aligned arrays and n_decay % 4 == 0, and mla_adamw_step passes n_decay = n:
                                   n in {4, 4096, 4100} (aligned, no_p16); n % 4 != 0 reaches it through mla_adamw_step_groups with
                                   n_decay = n - n % 4 (+ scalar tail). Everything else is all scalar. 8392708: the grid capped at
                                   8192 blocks, one trip each; 33558535: a second trip per block and a scalar tail
  ce_fwd_kernel                    bf16: scalar walk; fp32: 16-byte loads on the rows whose start is aligned (every row at ld % 4 == 0,
                                   rows 0 and 4 at ld = ncols + 1 with ncols % 4 == 0, ...), scalar walk on the others and on the tail
  infonce_bwd_kernel               Mp % 4 == 0: 4 columns per lane; (7, 9) and (130, 130): scalar
"""
import pytest
import torch

import trunk_cases as T
from conftest import poison_free_memory

pytestmark = pytest.mark.gpu
BF, F32, F64 = T.BF, T.F32, T.F64
NAN = float("nan")


def _hip():
    from mla_amd import hip
    return hip


def _say(capsys, text):
    with capsys.disabled():
        print("\nTRUNK " + text, end="")


def _eslack(ref32, ref64):
    return (ref32.to(F64) - ref64).abs()


class Worst(dict):
    def add(self, name, ratio):
        self[name] = max(self.get(name, 0.0), ratio)

    def line(self):
        return "  ".join(f"{k} {v:.3f}" for k, v in self.items())

    def check(self, *ctx):
        bad = {k: v for k, v in self.items() if not v <= 1}
        assert not bad, (ctx, bad)


# ------------------------------------------------------------------------------------------------ norms, forward
@pytest.mark.parametrize("H", T.NORM_H)
@pytest.mark.parametrize("family", T.NORM_FAMILIES)
def test_norm_forward(dev, family, H, capsys):
    hip = _hip()
    wst = Worst()
    w, b = T.norm_weight(H).to(dev), T.norm_bias(H).to(dev)
    for rows in T.NORM_ROWS:
        x = T.norm_rows(family, rows, H).to(dev)
        y64, xg64, r64 = T.rmsnorm_ref(x, w, T.NORM_EPS, F64)
        y32, xg32, _ = T.rmsnorm_ref(x, w, T.NORM_EPS, F32)
        l64, l32 = T.layernorm_ref(x, w, b, T.NORM_EPS, F64), T.layernorm_ref(x, w, b, T.NORM_EPS, F32)
        poison_free_memory()
        y, rstd = hip.rmsnorm_fwd(x, w, T.NORM_EPS)
        xg, rstd_p = hip.rmsnorm_prep(x, w, T.NORM_EPS)
        xg_only, none = hip.rmsnorm_prep(x, w, T.NORM_EPS, want_rstd=False)
        ln = hip.layernorm_fwd(x, w, b, T.NORM_EPS)
        wst.add("rmsnorm_fwd", T.bf16_ratio(y, y64, T.row_slack(y32, y64), k=2)[0])
        wst.add("rmsnorm_fwd.rstd", T.scalar_ratio(rstd, r64))
        wst.add("rmsnorm_prep", T.bf16_ratio(xg, xg64, T.row_slack(xg32, xg64))[0])
        wst.add("rmsnorm_prep.rstd", T.scalar_ratio(rstd_p, r64))
        wst.add("layernorm_fwd", T.bf16_ratio(ln, l64, T.row_slack(l32, l64))[0])
        assert none is None and T.bits_equal(xg_only, xg)
        y2, rstd2 = hip.rmsnorm_fwd(x, w, T.NORM_EPS)
        assert T.bits_equal(y2, y) and T.bits_equal(rstd2, rstd), (family, H, rows, "second launch differs")
        assert T.bits_equal(hip.layernorm_fwd(x, w, b, T.NORM_EPS), ln) and T.bits_equal(hip.rmsnorm_prep(x, w, T.NORM_EPS)[1], rstd_p)
    _say(capsys, f"norm_fwd {family:<8} H {H:>4}: {wst.line()}")
    wst.check(family, H)


@pytest.mark.parametrize("H", T.TIMM_H)
@pytest.mark.parametrize("family", T.NORM_FAMILIES)
def test_timm_forward(dev, family, H, capsys):
    hip = _hip()
    wst = Worst()
    w = T.norm_weight(H).to(dev)
    for rows in T.NORM_ROWS:
        x = T.norm_rows(family, rows, H).to(dev)
        y64, m64, r64, _, _ = T.timm_ref(x, w, T.NORM_EPS, F64)
        y32 = T.timm_ref(x, w, T.NORM_EPS, F32)[0]
        poison_free_memory()
        y, mean, rstd = hip.timm_rmsnorm_fwd(x, w, T.NORM_EPS)
        wst.add("timm_fwd", T.bf16_ratio(y, y64, T.row_slack(y32, y64))[0])
        wst.add("timm_fwd.mean", T.mean_ratio(mean, x))
        wst.add("timm_fwd.rstd", T.scalar_ratio(rstd, r64))
        y2, mean2, rstd2 = hip.timm_rmsnorm_fwd(x, w, T.NORM_EPS)
        assert T.bits_equal(y2, y) and T.bits_equal(mean2, mean) and T.bits_equal(rstd2, rstd)
    _say(capsys, f"timm_fwd {family:<8} H {H:>4}: {wst.line()}")
    wst.check(family, H)


@pytest.mark.parametrize("rows,H", T.APPLY_T_SHAPES)
def test_rmsnorm_apply_t_is_the_transposed_forward(dev, rows, H):
    hip = _hip()
    w = T.norm_weight(H).to(dev)
    for family in T.NORM_FAMILIES:
        x = T.norm_rows(family, rows, H, "apply_t").to(dev)
        poison_free_memory()
        y, rstd = hip.rmsnorm_fwd(x, w, T.NORM_EPS)
        yt = hip.rmsnorm_apply_t(x, w, rstd)
        assert yt.shape == (H, rows) and T.bits_equal(yt, y.t().contiguous()), (family, rows, H)


# ------------------------------------------------------------------------------------------------ norms, backward
def _dw_modes(H, dev):
    base = T.flat_input(H, "dwbase").to(dev)
    return (("none", None, False, None), ("fresh", lambda: torch.full((H,), NAN, dtype=F32, device=dev), False, None),
            ("accumulate", lambda: base.clone(), True, base.to(F64)))


@pytest.mark.parametrize("family", T.NORM_FAMILIES)
@pytest.mark.parametrize("rows,H", T.BWD_SHAPES)
def test_rmsnorm_backward(dev, rows, H, family, capsys):
    hip = _hip()
    wst = Worst()
    w, dy = T.norm_weight(H).to(dev), T.norm_dy(rows, H).to(dev)
    x, dres_t = T.norm_rows(family, rows, H, "bwd").to(dev), T.norm_rows("gauss", rows, H, "dres").to(dev)
    rstd = T.rmsnorm_ref(x, w, T.NORM_EPS, F64)[2].float()
    for dres in (None, dres_t):
        dx64, t64 = T.rmsnorm_bwd_ref(dy, x, w, rstd, dres, F64)
        slack = T.row_slack(T.rmsnorm_bwd_ref(dy, x, w, rstd, dres, F32)[0], dx64)
        for mode, make, acc, base64 in _dw_modes(H, dev):
            poison_free_memory()
            dw = make() if make else None
            dx = hip.rmsnorm_bwd(dy, x, w, rstd, dres=dres, dw_out=dw, dw_accumulate=acc)
            wst.add("dx" if dres is None else "dx+dres", T.bf16_ratio(dx, dx64, slack)[0])
            if dw is not None:
                wst.add("dw." + mode, T.dw_check(dw, t64, base64))
                dw2 = make()
                dx2 = hip.rmsnorm_bwd(dy, x, w, rstd, dres=dres, dw_out=dw2, dw_accumulate=acc)
                assert T.bits_equal(dw2, dw) and T.bits_equal(dx2, dx), (family, rows, H, mode, "second launch differs")
    _say(capsys, f"rmsnorm_bwd {family:<8} {rows:>4} x {H:>4}: {wst.line()}")
    wst.check(family, rows, H)


@pytest.mark.parametrize("family", T.NORM_FAMILIES)
@pytest.mark.parametrize("rows,H", T.BWD_SHAPES)
def test_timm_rmsnorm_backward(dev, rows, H, family, capsys):
    hip = _hip()
    wst = Worst()
    w, dy = T.norm_weight(H).to(dev), T.norm_dy(rows, H).to(dev)
    x = T.norm_rows(family, rows, H, "bwd").to(dev)
    _, m64, r64, _, _ = T.timm_ref(x, w, T.NORM_EPS, F64)
    mean, rstd = m64.float(), r64.float()
    dx64, t64 = T.timm_bwd_ref(dy, x, w, mean, rstd, F64)
    slack = T.row_slack(T.timm_bwd_ref(dy, x, w, mean, rstd, F32)[0], dx64)
    for mode, make, acc, base64 in _dw_modes(H, dev):
        poison_free_memory()
        dw = make() if make else None
        dx = hip.timm_rmsnorm_bwd(dy, x, w, mean, rstd, dw_out=dw, dw_accumulate=acc)
        wst.add("dx", T.bf16_ratio(dx, dx64, slack)[0])
        if dw is not None:
            wst.add("dw." + mode, T.dw_check(dw, t64, base64))
            dw2 = make()
            dx2 = hip.timm_rmsnorm_bwd(dy, x, w, mean, rstd, dw_out=dw2, dw_accumulate=acc)
            assert T.bits_equal(dw2, dw) and T.bits_equal(dx2, dx), (family, rows, H, mode, "second launch differs")
    _say(capsys, f"timm_bwd {family:<8} {rows:>4} x {H:>4}: {wst.line()}")
    wst.check(family, rows, H)


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("rows", T.COLSUM_ROWS)
def test_colsum(dev, rows, capsys):
    hip = _hip()
    wst = Worst()
    for N in (T.COLSUM_N if rows <= 513 else T.COLSUM_N_LARGE):
        x = T.colsum_input(rows, N)
        t64 = x.to(dev).to(F64)
        ref, sumabs = t64.sum(0), t64.abs().sum(0)
        base = T.flat_input(N, "colsum_base").to(dev)
        for layout in T.COLSUM_LAYOUTS:
            view = T.place_2d(x, layout, dev)
            vec = T.colsum_is_vec(view)
            assert vec == (N % 8 == 0 and layout in ("contig", "aligned_slice")), (rows, N, layout)
            for acc in (False, True):
                poison_free_memory()
                out = base.clone() if acc else torch.full((N,), NAN, dtype=F32, device=dev)
                hip.colsum(view, out, acc)
                name = ("vec" if vec else "scalar") + (".acc" if acc else "")
                if acc:
                    wst.add(name, T.reduction_ratio(out, ref + base.to(F64), rows + 1, sumabs + base.to(F64).abs()))
                else:
                    wst.add(name, T.reduction_ratio(out, ref, rows, sumabs))
                out2 = base.clone() if acc else torch.full((N,), NAN, dtype=F32, device=dev)
                hip.colsum(view, out2, acc)
                assert T.bits_equal(out2, out), (rows, N, layout, acc, "second launch differs")
    _say(capsys, f"colsum rows {rows:>5}: {wst.line()}")
    wst.check(rows)


@pytest.mark.parametrize("n", T.SUMSQ_N)
def test_sumsq(dev, n, capsys):
    hip = _hip()
    wst = Worst()
    x = T.flat_input(n, "sumsq").to(dev)
    t64 = x.to(F64) ** 2
    for acc, base in ((False, NAN), (True, 1234.5)):
        poison_free_memory()
        out = torch.full((1,), base, dtype=F32, device=dev)
        hip.sumsq(x, out, acc)
        if acc:
            wst.add("sumsq.acc", T.reduction_ratio(out[0], t64.sum() + base, n + 1, t64.sum() + base))
        else:
            wst.add("sumsq", T.reduction_ratio(out[0], t64.sum(), n, t64.sum()))
        out2 = torch.full((1,), base, dtype=F32, device=dev)
        hip.sumsq(x, out2, acc)
        assert T.bits_equal(out2, out), (n, acc, "second launch differs")
    _say(capsys, f"sumsq n {n:>8}: {wst.line()}")
    wst.check(n)


@pytest.mark.parametrize("n", T.PARTIALS_N)
def test_sum_partials(dev, n, capsys):
    hip = _hip()
    wst = Worst()
    x = T.flat_input(n, "sumsq")
    for layout in ("aligned", "offset1"):
        buf = torch.full((n + 9,), NAN, dtype=F32, device=dev)
        part = buf[1:1 + n] if layout == "offset1" else buf[:n]
        part.copy_(x)
        if n == 0:
            part = buf[1:2] if layout == "offset1" else buf[:1]        # a pointer is required; nothing behind it may be read
        assert part.data_ptr() % 16 == (4 if layout == "offset1" else 0)
        p64 = x.to(dev).to(F64)
        for acc, base in ((False, NAN), (True, -77.25)):
            poison_free_memory()
            out = torch.full((1,), base, dtype=F32, device=dev)
            hip.sum_partials(part, n, out, acc)
            ref, sumabs, terms = (p64.sum() + base, p64.abs().sum() + abs(base), n + 1) if acc else (p64.sum(), p64.abs().sum(), n)
            wst.add(layout + (".acc" if acc else ""), T.reduction_ratio(out[0], ref, terms, sumabs))
            out2 = torch.full((1,), base, dtype=F32, device=dev)
            hip.sum_partials(part, n, out2, acc)
            assert T.bits_equal(out2, out), (n, layout, acc, "second launch differs")
    _say(capsys, f"sum_partials n {n:>4}: {wst.line()}")
    wst.check(n)


def test_clip_coef(dev, capsys):
    hip = _hip()
    wst = Worst()
    for s in T.CLIP_SUMSQ:
        coef64, norm64 = T.clip_ref(s, 1.0)
        ss = torch.tensor([s], dtype=F32, device=dev)
        for want_norm in (False, True):
            coef = torch.full((1,), NAN, dtype=F32, device=dev)
            norm = torch.full((1,), NAN, dtype=F32, device=dev) if want_norm else None
            hip.clip_coef(ss, 1.0, coef, norm)
            wst.add("coef", T.rel_ratio(coef, torch.tensor([coef64], dtype=F64, device=dev), 4))
            if want_norm:
                wst.add("norm", T.rel_ratio(norm, torch.tensor([norm64], dtype=F64, device=dev), 4))
        assert (float(coef) == 1.0) == (s < 1.0), s
    _say(capsys, f"clip_coef: {wst.line()}")
    wst.check()


# ------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("kind", range(4))
def test_activations_every_bf16_value(dev, kind, capsys):
    """Forward and backward over every finite bf16 bit pattern with |x| <= 65536 (36610 values: the 16-byte loop and a tail of 2)."""
    hip = _hip()
    wst = Worst()
    x = T.unary_inputs().to(dev)
    poison_free_memory()
    y = hip.act_fwd(x, kind)
    y64, y32 = T.act_ref(kind, x, F64), T.act_ref(kind, x, F32)
    r, n = T.bf16_ratio(y, y64, _eslack(y32, y64))
    wst.add("fwd", r)
    d64, d32 = T.act_dref(kind, x, F64), T.act_dref(kind, x, F32)
    for dyv in T.SWIGLU_DACT:
        dy = torch.full_like(x, dyv)
        dx = hip.act_bwd(dy, x, kind)
        s = dy.to(F64)
        wst.add(f"bwd(dy={dyv})", T.bf16_ratio(dx, s * d64, _eslack(dy.float() * d32, s * d64))[0])
    if kind == 2:
        assert T.bits_equal(y, torch.where(x > 0, x, torch.zeros_like(x)))
    _say(capsys, f"act {T.ACT_NAMES[kind]:<9} all bf16 values: {wst.line()}  (forward elements outside: {n})")
    wst.check(kind)


@pytest.mark.parametrize("n", T.TAIL_N)
def test_elementwise_tails(dev, n, capsys):
    """n in {1, 7}: tail only; 8: no tail; 9, 1003: both -- the activations, both casts and add."""
    hip = _hip()
    wst = Worst()
    g = T._gen("tails", n)
    x = (3.0 * torch.randn(n, generator=g)).to(BF).to(dev)
    dy = torch.randn(n, generator=g).to(BF).to(dev)
    x32 = (torch.randn(n, generator=g) * 100.0).to(dev)
    poison_free_memory()
    for kind in range(4):
        y64, y32 = T.act_ref(kind, x, F64), T.act_ref(kind, x, F32)
        wst.add("act_fwd", T.bf16_ratio(hip.act_fwd(x, kind), y64, _eslack(y32, y64))[0])
        d64, d32 = dy.to(F64) * T.act_dref(kind, x, F64), dy.float() * T.act_dref(kind, x, F32)
        wst.add("act_bwd", T.bf16_ratio(hip.act_bwd(dy, x, kind), d64, _eslack(d32, d64))[0])
    assert T.bits_equal(hip.cast_bf16_to_f32(x), x.float()), n
    assert T.bits_equal(hip.cast_f32_to_bf16(x32), x32.to(BF)), n
    assert T.bits_equal(hip.add_bf16(x, dy), (x.float() + dy.float()).to(BF)), n
    _say(capsys, f"tails n {n:>4}: {wst.line()}")
    wst.check(n)


def test_cast_bf16_to_f32_every_bit_pattern(dev):
    x = T.all_bf16()
    poison_free_memory()
    y = _hip().cast_bf16_to_f32(x.to(dev)).cpu()
    assert T.bits_equal(y, x.float()) and int(torch.isnan(y).sum()) == 2 * 127


def test_cast_f32_to_bf16_ties(dev):
    """Every finite bf16 value, the tie above it and the tie -+ one fp32 ulp: round to nearest even, as torch's .to(bfloat16)."""
    x = T.cast_inputs()
    poison_free_memory()
    y = _hip().cast_f32_to_bf16(x.to(dev)).cpu()
    want = x.to(BF)
    assert T.bits_equal(y, want), int((y.view(torch.int16) != want.view(torch.int16)).sum())


def test_add_bf16_ties(dev):
    a, b = T.add_tie_inputs()
    poison_free_memory()
    y = _hip().add_bf16(a.to(dev), b.to(dev)).cpu()
    want = (a.float() + b.float()).to(BF)
    assert T.bits_equal(y, want), int((y.view(torch.int16) != want.view(torch.int16)).sum())


def test_swiglu_every_bf16_gate(dev, capsys):
    hip = _hip()
    wst = Worst()
    gu_h, I = T.swiglu_inputs()
    gu = gu_h.to(dev)
    fl = T.sigmoid_flushed(gu[:, :I])                   # gates below -87.3: the documented 0 of the reciprocal's flush
    a64, a32 = T.swiglu_ref(gu, F64), T.swiglu_ref(gu, F32)
    a_slack, a64 = T.flush_expected(_eslack(a32, a64), fl), T.flush_expected(a64, fl)
    assert 0 < int(fl[0].sum()) and float(gu[0, :I][fl[0]].float().max()) == -87.5
    poison_free_memory()
    act = hip.swiglu_fwd(gu)
    wst.add("fwd", T.bf16_ratio(act, a64, a_slack)[0])
    for d in T.SWIGLU_DACT:
        dact = torch.full((gu.shape[0], I), d, dtype=BF, device=dev)
        g64, _ = T.swiglu_bwd_ref(dact, gu, F64)
        g32, _ = T.swiglu_bwd_ref(dact, gu, F32)
        fl2 = torch.cat([fl, fl], 1)
        g_slack, g64 = T.flush_expected(_eslack(g32, g64), fl2), T.flush_expected(g64, fl2)
        for want_act in (False, True):
            poison_free_memory()
            dgu, act_out = hip.swiglu_bwd(dact, gu, want_act=want_act)
            wst.add(f"bwd(d={d})", T.bf16_ratio(dgu, g64, g_slack)[0])
            if want_act:
                wst.add("bwd.act", T.bf16_ratio(act_out, a64, a_slack)[0])
            else:
                assert act_out is None
    _say(capsys, f"swiglu every bf16 gate x up {T.SWIGLU_UP}: {wst.line()}")
    wst.check()


@pytest.mark.parametrize("rows,I", T.SWIGLU_T_SHAPES)
def test_swiglu_transposed_forms_are_bit_equal(dev, rows, I):
    hip = _hip()
    g = T._gen("swiglu_t", rows, I)
    gu = (3.0 * torch.randn(rows, 2 * I, generator=g)).to(BF).to(dev)
    dact = torch.randn(rows, I, generator=g).to(BF).to(dev)
    poison_free_memory()
    act = hip.swiglu_fwd(gu)
    assert T.bits_equal(hip.swiglu_fwd_t(gu), act.t().contiguous())
    act_d, act_dt = hip.swiglu_fwd_dual(gu)
    assert T.bits_equal(act_d, act) and T.bits_equal(act_dt, act.t().contiguous())
    dgu, _ = hip.swiglu_bwd(dact, gu)
    dgu_t, dgu_tt = hip.swiglu_bwd_t(dact, gu)
    assert T.bits_equal(dgu_t, dgu) and T.bits_equal(dgu_tt, dgu.t().contiguous())


@pytest.mark.parametrize("S", T.ROPE_S)
@pytest.mark.parametrize("D", T.ROPE_D)
def test_rope(dev, D, S, capsys):
    hip = _hip()
    wst = Worst()
    q_off, k_off, ld, nh = T.rope_layout(D)
    x = T.rope_input(S, D).to(dev)
    cos, sin = (t.to(dev) for t in T.rope_tables(S, D))
    keep = ~T.rope_mask(D).to(dev)
    y64, y32 = T.rope_ref(x, cos, sin, S, D, F64), T.rope_ref(x, cos, sin, S, D, F32)
    buf = x.clone()
    hip.rope_inplace(buf, cos, sin, S, nh, D, q_off, k_off)
    wst.add("fwd", T.bf16_ratio(buf, y64, _eslack(y32, y64))[0])
    assert T.bits_equal(buf[:, keep], x[:, keep]), (D, S, "a column outside q and k changed")
    b64, b32 = T.rope_ref(x, cos, sin, S, D, F64, backward=True), T.rope_ref(x, cos, sin, S, D, F32, backward=True)
    bwd = x.clone()
    hip.rope_inplace(bwd, cos, sin, S, nh, D, q_off, k_off, backward=True)
    wst.add("bwd", T.bf16_ratio(bwd, b64, _eslack(b32, b64))[0])
    # backward after forward returns the input: two bf16 roundings; slack = what the fp32 round trip through the bf16 forward
    # output leaves (the rounding of y weighs on its partner column). With 4 x that slack this check is LOOSER than a plain k = 2:
    # about k = 2 plus several U16 of the partner column. The forward and backward checks above, at k = 1 each, carry the weight.
    trip = T.rope_ref(y32.to(BF), cos, sin, S, D, F32, backward=True)
    hip.rope_inplace(buf, cos, sin, S, nh, D, q_off, k_off, backward=True)
    wst.add("round trip", T.bf16_ratio(buf, x.to(F64), _eslack(trip, x.to(F64)), k=2)[0])
    assert T.bits_equal(buf[:, keep], x[:, keep])
    _say(capsys, f"rope D {D:>3} S {S:>2}: {wst.line()}")
    wst.check(D, S)


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("dtype", (BF, F32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("family", T.CE_FAMILIES)
def test_ce_fwd(dev, family, dtype, capsys):
    hip = _hip()
    wst = Worst()
    for ncols in T.CE_NCOLS:
        x = T.ce_logits(family, ncols).to(dtype).to(dev)
        labels = T.ce_labels(family, ncols).to(dev)
        ref = {id(lab): T.ce_ref(x, lab, F64) for lab in (labels, None)}
        for ld in T.ce_lds(ncols):
            buf = torch.full((T.CE_ROWS, ld), NAN, dtype=dtype, device=dev)
            view = buf[:, :ncols]
            view.copy_(x)
            for lab in (labels, None):
                lse64, loss64, scale = ref[id(lab)]
                poison_free_memory()
                loss, lse = hip.ce_fwd(view, lab)
                wst.add("lse", T.scalar_ratio(lse, lse64, T.lse_scale(lse64)))
                wst.add("loss" if lab is not None else "loss(labels=None)", T.scalar_ratio(loss, loss64, scale))
                loss2, lse2 = hip.ce_fwd(view, lab)
                assert T.bits_equal(lse2, lse) and T.bits_equal(loss2, loss), (family, ncols, ld, "second launch differs")
            none, lse_only = hip.ce_fwd(view, labels, want_loss=False)
            assert none is None and T.bits_equal(lse_only, lse), (family, ncols, ld, "want_loss=False")
    _say(capsys, f"ce_fwd {family:<8} {'bf16' if dtype == BF else 'fp32'}: {wst.line()}")
    wst.check(family, dtype)


@pytest.mark.parametrize("M,Mp", T.INFONCE_SHAPES)
def test_infonce_bwd(dev, M, Mp, capsys):
    hip = _hip()
    wst = Worst()
    for scale in T.INFONCE_SCALES:
        L, rl, cl, gs = (t.to(dev) for t in T.infonce_case(M, Mp, scale))
        r64, r32 = T.infonce_ref(L, rl, cl, gs, M, F64), T.infonce_ref(L, rl, cl, gs, M, F32)
        poison_free_memory()
        dL = hip.infonce_bwd(L, rl, cl, gs, M)
        wst.add(f"x{scale:g}", T.bf16_ratio(dL, r64, _eslack(r32, r64))[0])
        z = dL.float()
        assert bool((z[M:] == 0).all()) and bool((z[:, M:] == 0).all()), (M, Mp, "padding is exactly zero")
        if M > 1:
            assert bool((z.diagonal()[:M] < 0).all()), (M, Mp, "the diagonal is negative")
    _say(capsys, f"infonce_bwd M {M:>3} Mp {Mp:>3}: {wst.line()}")
    wst.check(M, Mp)


@pytest.mark.parametrize("ncols", T.L2_NCOLS)
def test_l2norm(dev, ncols, capsys):
    hip = _hip()
    wst = Worst()
    for rows in T.L2_ROWS:
        x = T.l2_rows(rows, ncols).to(dev)
        dy = T.norm_rows("gauss", rows, ncols, "l2dy").to(dev)
        y64, n64 = T.l2_ref(x, T.L2_EPS, F64)
        y32, _ = T.l2_ref(x, T.L2_EPS, F32)
        poison_free_memory()
        y, norms = hip.l2norm_fwd(x, T.L2_EPS)
        wst.add("fwd", T.bf16_ratio(y, y64, T.row_slack(y32, y64))[0])
        wst.add("norms", T.scalar_ratio(norms, n64))
        if rows >= 3:
            assert float(norms[1]) == T.f32v(T.L2_EPS) and bool((y[1].float() == 0).all()), (rows, ncols, "zero row: y = 0, norm = eps")
        y_in, n_in = y32.to(BF), n64.float()                # the backward's inputs come from the reference, not from the kernel above
        d64, d32 = T.l2_bwd_ref(dy, y_in, n_in, F64), T.l2_bwd_ref(dy, y_in, n_in, F32)
        dx = hip.l2norm_bwd(dy, y_in, n_in)
        wst.add("bwd", T.bf16_ratio(dx, d64, T.row_slack(d32, d64))[0])
        y2, norms2 = hip.l2norm_fwd(x, T.L2_EPS)
        assert T.bits_equal(y2, y) and T.bits_equal(norms2, norms) and T.bits_equal(hip.l2norm_bwd(dy, y_in, n_in), dx)
    _say(capsys, f"l2norm ncols {ncols:>4}: {wst.line()}")
    wst.check(ncols)


# ------------------------------------------------------------------------------------------------ AdamW
_STATE = {}


def _state(family, dev):
    if family not in _STATE:
        _STATE[family] = tuple(t.to(dev) for t in T.adamw_state(family, max(T.ADAMW_N)))
    return _STATE[family]


def _adamw_case(hip, st, n, layout, step, wd, gs_t, n_decay=None):
    """One step in `layout`; returns the (m, v, p) ratios after checking the bf16 copy and the buffers' surroundings."""
    dev = st[0].device
    p0, g0, m0, v0 = (t[:n] for t in st)
    (p, g, m, v), p16 = T.adamw_place(p0, g0, m0, v0, layout, dev)
    h = T.ADAMW_HYPER
    if n_decay is None:
        hip.adamw_step(p, g, m, v, p16, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, step, gs_t)
    else:
        hip.adamw_step_groups(p, g, m, v, p16, n_decay, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, step, gs_t)
    ref = T.adamw_ref64(p0, g0, m0, v0, step, wd, None if gs_t is None else T.ADAMW_GS, n_decay=n_decay)
    assert T.bits_equal(g, g0), "the gradient is read only"
    for t in (p, g, m, v) + ((p16,) if p16 is not None else ()):
        base, off = t._base, t.storage_offset()
        assert bool(torch.isnan(base[:off]).all()) and bool(torch.isnan(base[off + n:]).all()), (layout, n, "wrote outside its range")
    if p16 is not None:
        assert T.bits_equal(p16, p.to(BF)), (layout, n, "p16 is bf16(p) of the kernel's own p")
    return T.adamw_ratios(p, m, v, ref, p0)


@pytest.mark.parametrize("step", T.ADAMW_STEPS)
@pytest.mark.parametrize("family", T.ADAMW_FAMILIES)
def test_adamw(dev, family, step, capsys):
    hip = _hip()
    st = _state(family, dev)
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    wst = Worst()
    poison_free_memory()
    for wd in T.ADAMW_WD:
        for gs in (None, gs_t):
            for n in T.ADAMW_N:
                for layout in T.ADAMW_LAYOUTS:
                    runs = [(None, "vec" if T.adamw_all_vector(layout, n) else "scalar")]
                    if n % 4 and T.adamw_all_vector(layout, n, n - n % 4):       # whole groups in the 16-byte kernel + a scalar tail
                        runs.append((n - n % 4, "vec+tail"))
                    for n_decay, tag in runs:
                        rm, rv, rp = _adamw_case(hip, st, n, layout, step, wd, gs, n_decay=n_decay)
                        wst.add(tag + ".m", rm)
                        wst.add(tag + ".v", rv)
                        wst.add(tag + ".p", rp)
    _say(capsys, f"adamw {family:<5} step {step:>6}: {wst.line()}")
    wst.check(family, step)


@pytest.mark.parametrize("n", (T.ADAMW_N_CAPPED, T.ADAMW_N_BIG))
def test_adamw_past_the_grid_cap(dev, n, capsys):
    """The capped-grid chunked walk of adamw_vec4_kernel, the path every real shard takes: n = 8392708 through mla_adamw_step (8192
    blocks, one trip each, no tail), n = 33558535 through mla_adamw_step_groups with n_decay = n - 7 (a second trip, a scalar tail)."""
    hip = _hip()
    st = tuple(t.to(dev) for t in T.adamw_state("unit", n, tag="big"))
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    n_decay = None if n % 4 == 0 else n - 7
    assert T.adamw_all_vector("aligned", n, n_decay) and (n // 4 > 8192 * 256) and (n == T.ADAMW_N_CAPPED or n // 4 > 8192 * 1024)
    poison_free_memory()
    r = _adamw_case(hip, st, n, "aligned", 3, 0.01, gs_t, n_decay=n_decay)
    _say(capsys, f"adamw unit step 3 n {n}: m {r[0]:.3f} v {r[1]:.3f} p {r[2]:.3f}")
    assert max(r) <= 1, r


@pytest.mark.parametrize("n", (4100, 262147))
def test_adamw_step_groups(dev, n, capsys):
    """Against the fp64 reference with per-element decay (not against a second launch: test_kernels_gpu.py does that)."""
    hip = _hip()
    st = _state("unit", dev)
    gs_t = torch.tensor([T.ADAMW_GS], dtype=F32, device=dev)
    wst = Worst()
    poison_free_memory()
    for n_decay in (0, 5, 4096, 4098, n):
        for layout in ("aligned", "offset1"):
            rm, rv, rp = _adamw_case(hip, st, n, layout, 3, 0.01, gs_t, n_decay=n_decay)
            tag = "vec" if T.adamw_all_vector(layout, n, n_decay) else "scalar"
            wst.add(tag + ".m", rm)
            wst.add(tag + ".v", rv)
            wst.add(tag + ".p", rp)
    _say(capsys, f"adamw_step_groups n {n}: {wst.line()}")
    wst.check(n)
