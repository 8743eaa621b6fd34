"""CPU checks of tests/trunk_cases.py, the helper module of tests/test_trunk_kernels_gpu.py: every fp32 emulation stays inside the
bound it will be used with (so the inputs keep an honest fp32 kernel inside the rule), the sentinels weigh >= 100 x the bound, the
timm variance of the chosen seeds is away from a bf16 rounding boundary, and a set of deliberately wrong emulations -- the (H - 1)
divisor, a dropped 8-column chunk, a dropped row, fp32 bias corrections, an ignored clip coefficient -- is caught."""
import math

import pytest
import torch

import trunk_cases as T

BF, F32, F64 = T.BF, T.F32, T.F64


def _emul(ref32):
    """An honest kernel: the fp32 evaluation rounded once to bf16."""
    return ref32.to(BF)


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("family", T.NORM_FAMILIES)
def test_norm_forward_emulations(family):
    worst = {}
    for H in sorted(set(T.NORM_H) | set(T.TIMM_H)):
        for rows in T.NORM_ROWS:
            x, w, b = T.norm_rows(family, rows, H), T.norm_weight(H), T.norm_bias(H)
            if H in T.NORM_H:
                y64, xg64, r64 = T.rmsnorm_ref(x, w, T.NORM_EPS, F64)
                y32, xg32, r32 = T.rmsnorm_ref(x, w, T.NORM_EPS, F32)
                y_emul = (w.float() * (x.float() * r32[:, None]).to(BF).float()).to(BF)     # the documented double rounding
                cases = [("rmsnorm", T.bf16_ratio(y_emul, y64, T.row_slack(y32, y64), k=2)[0]),
                         ("prep", T.bf16_ratio(_emul(xg32), xg64, T.row_slack(xg32, xg64))[0]),
                         ("rstd", T.scalar_ratio(r32, r64))]
                l64, l32 = T.layernorm_ref(x, w, b, T.NORM_EPS, F64), T.layernorm_ref(x, w, b, T.NORM_EPS, F32)
                cases.append(("layernorm", T.bf16_ratio(_emul(l32), l64, T.row_slack(l32, l64))[0]))
                # wrong emulations: the rstd rule sees an (H - 1) divisor and a dropped chunk at every H
                for kw in (dict(divisor=H - 1), dict(skip_last_chunk=True)):
                    if H == 8 and "skip_last_chunk" in kw:
                        continue
                    bad = T.rmsnorm_ref(x, w, T.NORM_EPS, F32, **kw)[2]
                    if family == "tiny":            # eps dominates: the statistic itself barely shows in rstd
                        continue
                    assert T.scalar_ratio(bad, r64) > 1, (family, H, rows, kw)
            if H in T.TIMM_H:
                t64, t32 = T.timm_ref(x, w, T.NORM_EPS, F64), T.timm_ref(x, w, T.NORM_EPS, F32)
                cases = cases if H in T.NORM_H else []
                cases += [("timm", T.bf16_ratio(_emul(t32[0]), t64[0], T.row_slack(t32[0], t64[0]))[0]),
                          ("timm_mean", T.mean_ratio(t32[1], x)), ("timm_rstd", T.scalar_ratio(t32[2], t64[2]))]
                for v in (t64[3], t64[4]):
                    assert float(T.bf16_boundary_distance(v).min()) > 2.0 ** -20, (family, H, rows, "variance on a bf16 rounding boundary")
            for name, r in cases:
                worst[name] = max(worst.get(name, 0.0), r)
                assert r <= 1, (family, H, rows, name, r)
    print(family, {k: round(v, 3) for k, v in worst.items()})


def test_rstd_rule_sees_what_the_bf16_rule_cannot():
    """At H = 2056 an (H - 1) divisor moves y by 2.4e-4 relative, far inside one bf16 rounding; rstd is held to 8 x 2^-24."""
    H = 2056
    x, w = T.norm_rows("gauss", 5, H), T.norm_weight(H)
    y64, _, r64 = T.rmsnorm_ref(x, w, T.NORM_EPS, F64)
    y32, _, _ = T.rmsnorm_ref(x, w, T.NORM_EPS, F32)
    ybad, _, rbad = T.rmsnorm_ref(x, w, T.NORM_EPS, F32, divisor=H - 1)
    assert T.bf16_ratio(_emul(ybad), y64, T.row_slack(y32, y64), k=2)[1] == 0
    assert T.scalar_ratio(rbad, r64) > 100


@pytest.mark.parametrize("rows,H", T.BWD_SHAPES)
def test_norm_backward_emulations(rows, H):
    w = T.norm_weight(H)
    dy = T.norm_dy(rows, H)
    for family in T.NORM_FAMILIES:
        x = T.norm_rows(family, rows, H, "bwd")
        dres = T.norm_rows("gauss", rows, H, "dres")
        rstd = T.rmsnorm_ref(x, w, T.NORM_EPS, F64)[2].float()
        dx64, t64 = T.rmsnorm_bwd_ref(dy, x, w, rstd, dres, F64)
        dx32, t32 = T.rmsnorm_bwd_ref(dy, x, w, rstd, dres, F32)
        assert T.bf16_ratio(_emul(dx32), dx64, T.row_slack(dx32, dx64))[0] <= 1, (family, "dx")
        r = T.dw_check(t32.sum(0), t64)
        assert r <= 1, (family, "dw", r)
        base = T.flat_input(H, "dwbase")
        assert T.dw_check(base + t32.sum(0), t64, base.double()) <= 1
        bound = T.reduction_bound(rows, t64.abs().sum(0))
        assert T.sentinel_ratio(t64, bound, T.bwd_sentinel_rows(rows)) >= 100, (family, rows, H)
        if rows > 1:
            assert T.dw_check(t32[:-1].sum(0), t64) > 100, (family, "a dw that skips the last row")
        _, tm, tr, _, _ = T.timm_ref(x, w, T.NORM_EPS, F64)
        if H > 8:
            tx64, tt64 = T.timm_bwd_ref(dy, x, w, tm.float(), tr.float(), F64)
            tx32, tt32 = T.timm_bwd_ref(dy, x, w, tm.float(), tr.float(), F32)
            assert T.bf16_ratio(_emul(tx32), tx64, T.row_slack(tx32, tx64))[0] <= 1, (family, "timm dx")
            assert T.dw_check(tt32.sum(0), tt64) <= 1, (family, "timm dw")


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("rows", T.COLSUM_ROWS)
def test_colsum_emulation_and_sentinels(rows):
    for N in (T.COLSUM_N if rows <= 513 else T.COLSUM_N_LARGE):
        x = T.colsum_input(rows, N)
        t64 = x.double()
        ref, sumabs = t64.sum(0), t64.abs().sum(0)
        assert T.reduction_ratio(x.float().sum(0), ref, rows, sumabs) <= 1
        sent = T.colsum_sentinel_rows(rows)
        assert T.sentinel_ratio(t64, T.reduction_bound(rows, sumabs), sent) >= 100, (rows, N)
        rs = T.colsum_blocks(rows)
        if rs > 1:                                    # a colsum that skips the first row of a block slice
            per = (rows + rs - 1) // rs
            keep = torch.ones(rows, dtype=torch.bool)
            keep[per] = False
            assert T.reduction_ratio(x.float()[keep].sum(0), ref, rows, sumabs) > 100


@pytest.mark.parametrize("n", T.SUMSQ_N)
def test_flat_reductions(n):
    x = T.flat_input(n, "sumsq")
    t64 = x.double() ** 2
    assert T.reduction_ratio((x * x).sum(), t64.sum(), n, t64.sum()) <= 1
    assert T.sentinel_ratio(t64, T.reduction_bound(n, t64.sum()), range(max(n - 3, 0), n)) >= 100
    if n > 3:
        assert T.reduction_ratio((x[:-1] * x[:-1]).sum(), t64.sum(), n, t64.sum()) > 100
    if n in T.PARTIALS_N:
        p64 = x.double()
        assert T.reduction_ratio(x.sum(), p64.sum(), n, p64.abs().sum()) <= 1
        assert T.sentinel_ratio(p64, T.reduction_bound(n, p64.abs().sum()), range(max(n - 3, 0), n)) >= 100


def test_clip_reference():
    for s in T.CLIP_SUMSQ:
        coef, nrm = T.clip_ref(s, 1.0)
        assert coef == pytest.approx(min(1.0, 1.0 / (math.sqrt(s) + 1e-6)), rel=1e-6) and (coef == 1.0) == (s < 1.0)
        assert nrm == pytest.approx(math.sqrt(s), rel=1e-7)


# ------------------------------------------------------------------------------------------------ element-wise
def test_unary_inputs_cover_the_range():
    x = T.unary_inputs()
    assert x.numel() == 2 * (128 * 143 + 1)          # zero, sub-normals and the 142 binades below 2^16, 65536 itself, both signs
    f = x.float()
    assert bool(torch.isfinite(f).all()) and float(f.abs().max()) == 65536.0
    assert int((f == 0).sum()) == 2 and float(f[f > 0].min()) < 1e-40
    assert len(set(x.view(torch.int16).tolist())) == x.numel()


@pytest.mark.parametrize("kind", range(4))
def test_activation_emulations(kind):
    x = T.unary_inputs()
    for ref in (T.act_ref, T.act_dref):
        r64, r32 = ref(kind, x, F64), ref(kind, x, F32)
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), (kind, ref.__name__)
        worst, n = T.bf16_ratio(_emul(r32), r64, (r32.double() - r64).abs())
        assert n == 0, (kind, ref.__name__, worst)


def test_activation_derivatives_match_autograd():
    x = torch.linspace(-6, 6, 241, dtype=F64, requires_grad=True)
    for kind in range(4):
        (g,) = torch.autograd.grad(T.act_ref(kind, x, F64).sum(), x)
        assert float((g - T.act_dref(kind, x.detach(), F64)).abs().max()) < 1e-12, kind


def test_swiglu_and_rope_emulations():
    gu, I = T.swiglu_inputs()
    a64, a32 = T.swiglu_ref(gu, F64), T.swiglu_ref(gu, F32)
    assert T.bf16_ratio(_emul(a32), a64, (a32.double() - a64).abs())[1] == 0
    for d in T.SWIGLU_DACT:
        dact = torch.full((gu.shape[0], I), d).to(BF)
        g64, g32 = T.swiglu_bwd_ref(dact, gu, F64)[0], T.swiglu_bwd_ref(dact, gu, F32)[0]
        assert T.bf16_ratio(_emul(g32), g64, (g32.double() - g64).abs())[1] == 0
    for D in T.ROPE_D:
        for S in T.ROPE_S:
            buf = T.rope_input(S, D)
            cos, sin = T.rope_tables(S, D)
            assert buf.shape[0] == 2 * S + 3
            y64, y32 = T.rope_ref(buf, cos, sin, S, D, F64), T.rope_ref(buf, cos, sin, S, D, F32)
            assert T.bf16_ratio(_emul(y32), y64, (y32.double() - y64).abs())[1] == 0
            keep = ~T.rope_mask(D)
            assert torch.equal(y64[:, keep], buf.double()[:, keep])
            back32 = T.rope_ref(_emul(y32), cos, sin, S, D, F32, backward=True)          # round trip, bf16 storage in between
            slack = (back32.double() - buf.double()).abs()
            assert T.bf16_ratio(_emul(back32), buf.double(), slack, k=2)[1] == 0


def test_swiglu_flush_region():
    """The documented limit of the SwiGLU sigmoid: gates from -87.5 down are expected as 0, -87.0 is held to the rule; what is given
    up there is far above the 2^-120 floor the rule has (so the floor cannot stand in for the limit)."""
    gu, I = T.swiglu_inputs()
    g = gu[0, :I]
    fl = T.sigmoid_flushed(g)
    assert float(g[fl].float().max()) == -87.5 and float(g[~fl].float().min()) == -87.0
    a64 = T.swiglu_ref(gu, F64)
    lost = a64[:, fl].abs().amax(1)                      # per `up` value
    assert float(lost[0]) > T.FLOOR and float(lost[3]) > 300 * T.FLOOR
    assert bool((T.flush_expected(a64, fl)[:, fl] == 0).all()) and torch.equal(T.flush_expected(a64, fl)[:, ~fl], a64[:, ~fl])


def test_cast_and_add_inputs():
    x = T.cast_inputs()
    assert bool(torch.isfinite(x).all()) and x.numel() == 4 * 65280
    y = x.to(BF)
    assert int((y.float() != x).sum()) >= 3 * 65000          # three of four inputs really round
    a, b = T.add_tie_inputs()
    s = a.float() + b.float()
    assert bool(torch.isfinite(s).all())
    n = a.numel() // 6
    same = (torch.sign(a.float()) == torch.sign(b.float()))[:2 * n]          # away from zero; towards zero a power of two lands on a finer grid instead
    assert bool(((s[:2 * n].view(torch.int32) & 0xFFFF) == 0x8000)[same].all()), "a + half an ulp is an exact tie in fp32"
    assert int(same.sum()) == n


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("family", T.CE_FAMILIES)
def test_ce_emulation(family):
    for ncols in T.CE_NCOLS:
        for dtype in (BF, F32):
            x = T.ce_logits(family, ncols).to(dtype)
            for labels in (T.ce_labels(family, ncols), None):
                lse64, loss64, scale = T.ce_ref(x, labels, F64)
                lse32, loss32, _ = T.ce_ref(x, labels, F32)
                assert bool(torch.isfinite(lse64).all()), (family, ncols)
                assert T.scalar_ratio(lse32, lse64, T.lse_scale(lse64)) <= 1, (family, ncols, dtype)
                assert T.scalar_ratio(loss32, loss64, scale) <= 1, (family, ncols, dtype)
                if labels is not None:
                    assert bool((loss64[1:4] == 0).all()) and bool(torch.isfinite(loss64).all())
        if family == "flat":
            assert float((lse64 - (x[:, 0].double() + math.log(ncols))).abs().max()) < 1e-12


def test_infonce_and_l2_emulations():
    for M, Mp in T.INFONCE_SHAPES:
        for scale in T.INFONCE_SCALES:
            L, rl, cl, gs = T.infonce_case(M, Mp, scale)
            r64, r32 = T.infonce_ref(L, rl, cl, gs, M, F64), T.infonce_ref(L, rl, cl, gs, M, F32)
            assert T.bf16_ratio(_emul(r32), r64, (r32.double() - r64).abs())[1] == 0
            assert bool((r64.diagonal()[:M] < 0).all() if M > 1 else (r64[0, 0] == 0)) and bool((r64[M:] == 0).all()) and bool((r64[:, M:] == 0).all())
    for ncols in T.L2_NCOLS:
        for rows in T.L2_ROWS:
            x = T.l2_rows(rows, ncols)
            y64, n64 = T.l2_ref(x, T.L2_EPS, F64)
            y32, n32 = T.l2_ref(x, T.L2_EPS, F32)
            assert T.bf16_ratio(_emul(y32), y64, T.row_slack(y32, y64))[1] == 0
            assert T.scalar_ratio(n32, n64) <= 1
            if rows >= 3:
                assert float(n64[1]) == T.f32v(T.L2_EPS) and bool((y64[1] == 0).all())
            dy = T.norm_rows("gauss", rows, ncols, "l2dy")
            d64, d32 = T.l2_bwd_ref(dy, _emul(y32), n32, F64), T.l2_bwd_ref(dy, _emul(y32), n32, F32)
            assert T.bf16_ratio(_emul(d32), d64, T.row_slack(d32, d64))[1] == 0


# ------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("family", T.ADAMW_FAMILIES)
def test_adamw_emulation(family, capsys):
    n = 4100
    st = T.adamw_state(family, n)
    worst = [0.0, 0.0, 0.0]
    worst_float = {}
    for step in T.ADAMW_STEPS:
        for wd in T.ADAMW_WD:
            for gs in (None, T.ADAMW_GS):
                ref = T.adamw_ref64(*st, step, wd, gs)
                p, m, v = T.adamw_emul32(*st, step, wd, gs, bias="double")
                r = T.adamw_ratios(p, m, v, ref, st[0])
                worst = [max(a, b) for a, b in zip(worst, r)]
                assert max(r) <= 1, (family, step, wd, gs, r)
                pf, mf, vf = T.adamw_emul32(*st, step, wd, gs, bias="float")
                worst_float[step] = max(worst_float.get(step, 0.0), T.adamw_ratios(pf, mf, vf, ref, st[0])[2])
                if gs is not None and family != "zero":
                    bad = T.adamw_emul32(*st, step, wd, gs, use_gs=False)
                    assert max(T.adamw_ratios(*bad, ref, st[0])) > 100, (family, step, "AdamW that ignores grad_scale")
    with capsys.disabled():
        print(f"\nadamw {family:<5} emulation, double corrections: worst m {worst[0]:.3f} v {worst[1]:.3f} p {worst[2]:.3f} of the bound; "
              "fp32 corrections, p by step: " + " ".join(f"{s}:{r:.2f}" for s, r in worst_float.items()))
    if family == "unit":
        assert worst_float[2] > 1, "fp32 bias corrections at step 2 must be outside the bound"


def test_adamw_groups_reference():
    st = T.adamw_state("unit", 64)
    a = T.adamw_ref64(*st, 3, 0.01, None, n_decay=5)
    full, none = T.adamw_ref64(*st, 3, 0.01, None), T.adamw_ref64(*st, 3, 0.0, None)
    assert torch.equal(a["p"][:5], full["p"][:5]) and torch.equal(a["p"][5:], none["p"][5:])
