"""Per-element parity of the kernels of the post-training generation heads -- mla_softmax_rows_fwd / _bwd, mla_dropout_fwd / _bwd,
mla_scale_batch, mla_layernorm_stats_fwd, mla_layernorm_bwd, mla_seqmean_fwd / _bwd, mla_bn_bwd, mla_chamfer_fwd / _bwd,
mla_imgloss_fwd / _bwd, mla_imgroi_fwd / _bwd (gen.hip) -- and of the backward halves of the tokenizer kernels, mla_lga_prep_bwd,
mla_maxpool_k_bwd (pointcloud.hip) and mla_avgpool_tokens_bwd (vision.hip), each called through its mla_amd.hip wrapper against the
fp64 references of tests/gen_cases.py. Every tolerance is a bound function of tests/trunk_cases.py; every test prints its worst
|err| / bound on a `GEN` line. The free pool is NaN-filled before every launch group, and a second identical launch must be bit-equal.

Which case takes which path:
  layernorm_stats_fwd / _bwd   H = 8: one lane works; 2056: the last 256-lane chunk holds one 16-byte piece; 8192: all LN_MAXC chunks.
                               rows <= 512: one row per block (511 / 512: the reduction of 511 / 512 partials); 513: block 0 walks two
                               rows; 1061: the block count capped at 512, a ragged second and third pass
  bn_bwd_partial_kernel        rows < 2048: one row slice; 2048 / 3000: two slices (3000: per = 1500, even; 132101: the 128-slice cap,
                               per = 1033, a ragged last slice of 910 rows); C in {1, 63, 65, 200}: a partly filled 64-column block
  softmax_rows_*               nvalid 1: one lane, one term; 255 | 257, 1025: below, across and four trips over the 256-lane stride;
                               ncols > nvalid: padding columns (NaN in scores and dPd: never read, outputs exactly 0);
                               dPd fp32 and bf16, each at p = 0 and p = 0.1
  dropout_* / scale_batch      n <= 256: one block; 257, 1003: a ragged last block; 2097157: the grid capped at 8192 blocks, lanes 0..4 of
                               block 0 take a second trip
  lga_prep_bwd_kernel          G = 1; G = 65, 130: a second / third ballot pass; K = 33, 128: the hit mask crosses a word / fills four;
                               C = 264: a second trip over the channels; `hostile` lists: a point in every group, a repeated index, a
                               point that is a centre and a neighbour, points in no list
  chamfer_*                    N or M = 4096: the 48 KB of LDS; N = 1, 128, 255 < 256: a partly filled block; lattice16: ties
  imgloss_* / imgroi_kernel    HW = 84, 24: fewer elements than the 2048-block grid has lanes; HW = 336: 677376 elements, the second
                               trip; ps = 6: 3 ps^2 = 108 < 256 lanes; ld padded: the padding columns of ddraw; fp32 and bf16 images
"""
import pytest
import torch

import gen_cases as G
from conftest import poison_free_memory

pytestmark = pytest.mark.gpu
BF, F32, F64 = G.BF, G.F32, G.F64
NAN = float("nan")


def _hip():
    from mla_amd import hip
    return hip


def _say(capsys, text):
    with capsys.disabled():
        print("\nGEN " + text, end="")


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


def _grad_modes(H, dev):
    """(name, make dw, make db, accumulate, base64): both null; both fresh (NaN-filled); both accumulated onto a non-zero base."""
    base = G.flat_bf16(H, "dwbase").float().to(dev)
    fresh = lambda: torch.full((H,), NAN, dtype=F32, device=dev)      # noqa: E731
    return (("none", None, False, None), ("fresh", fresh, False, None), ("accumulate", lambda: base.clone(), True, base.to(F64)))


# ------------------------------------------------------------------------------------------------ LayerNorm with statistics
@pytest.mark.parametrize("H", G.LN_H)
@pytest.mark.parametrize("family", G.LN_FAMILIES)
def test_layernorm_stats_forward(dev, family, H, capsys):
    hip = _hip()
    wst = Worst()
    w, b = G.norm_weight(H).to(dev), G.norm_bias(H).to(dev)
    for rows in G.LN_ROWS:
        x = G.norm_rows(family, rows, H).to(dev)
        y64, m64, r64 = G.ln_stats_ref(x, w, b, G.LN_EPS, F64)
        y32 = G.ln_stats_ref(x, w, b, G.LN_EPS, F32)[0]
        poison_free_memory()
        y, mean, rstd = hip.layernorm_stats_fwd(x, w, b, G.LN_EPS)
        wst.add("y", G.bf16_ratio(y, y64, G.row_slack(y32, y64))[0])
        wst.add("mean", G.mean_ratio(mean, x))
        wst.add("rstd", G.scalar_ratio(rstd, r64))
        y2, mean2, rstd2 = hip.layernorm_stats_fwd(x, w, b, G.LN_EPS)
        assert G.bits_equal(y2, y) and G.bits_equal(mean2, mean) and G.bits_equal(rstd2, rstd), (family, H, rows, "second launch differs")
    _say(capsys, f"ln_fwd {family:<8} H {H:>4}: {wst.line()}")
    wst.check(family, H)


@pytest.mark.parametrize("family", G.LN_FAMILIES)
@pytest.mark.parametrize("rows,H", G.LN_BWD_SHAPES)
def test_layernorm_backward(dev, rows, H, family, capsys):
    hip = _hip()
    wst = Worst()
    w, dy = G.norm_weight(H).to(dev), G.norm_dy(rows, H).to(dev)
    x = G.norm_rows(family, rows, H, "bwd").to(dev)
    _, m64, r64 = G.ln_stats_ref(x, w, G.norm_bias(H).to(dev), G.LN_EPS, F64)
    mean, rstd = m64.float(), r64.float()
    dx64, tw64, tb64 = G.ln_bwd_ref(dy, x, w, mean, rstd, F64)
    slack = G.row_slack(G.ln_bwd_ref(dy, x, w, mean, rstd, F32)[0], dx64)
    for mode, make, acc, base64 in _grad_modes(H, dev):
        poison_free_memory()
        dw, db = (make(), make()) if make else (None, None)
        dx = hip.layernorm_bwd(dy, x, w, mean, rstd, dw=dw, db=db, accumulate=acc)
        wst.add("dx", G.bf16_ratio(dx, dx64, slack)[0])
        if make:
            wst.add("dw." + mode, G.dw_check(dw, tw64, base64))
            wst.add("db." + mode, G.dw_check(db, tb64, base64))
            dw2, db2 = make(), make()
            dx2 = hip.layernorm_bwd(dy, x, w, mean, rstd, dw=dw2, db=db2, accumulate=acc)
            assert G.bits_equal(dw2, dw) and G.bits_equal(db2, db) and G.bits_equal(dx2, dx), (family, rows, H, mode, "second launch differs")
    _say(capsys, f"ln_bwd {family:<8} {rows:>4} x {H:>4}: {wst.line()}")
    wst.check(family, rows, H)


# ------------------------------------------------------------------------------------------------ BatchNorm(train) backward
@pytest.mark.parametrize("rows", G.BN_ROWS)
def test_bn_backward(dev, rows, capsys):
    hip = _hip()
    wst = Worst()
    assert hip.lib().mla_bn_bwd_blocks(rows) == G.bn_blocks(rows)
    for C in (G.BN_C if rows <= 3000 else G.BN_C_LARGE):
        for family in G.BN_FAMILIES:
            dy, x, w, mean, var = (t.to(dev) for t in G.bn_case(family, rows, C))
            dx64, tw64, tb64 = G.bn_bwd_ref(dy, x, w, mean, var, G.BN_EPS, F64)
            slack = _eslack(G.bn_bwd_ref(dy, x, w, mean, var, G.BN_EPS, F32)[0], dx64).amax(0, keepdim=True)
            for mode, make, acc, base64 in _grad_modes(C, dev):
                poison_free_memory()
                dw, db = (make(), make()) if make else (None, None)
                dx = hip.bn_bwd(dy, x, mean, var, w, G.BN_EPS, dw=dw, db=db, accumulate=acc)
                wst.add("dx", G.bf16_ratio(dx, dx64, slack)[0])
                if make:
                    wst.add("dw." + mode, G.dw_check(dw, tw64, base64))
                    wst.add("db." + mode, G.dw_check(db, tb64, base64))
                    dw2, db2 = make(), make()
                    dx2 = hip.bn_bwd(dy, x, mean, var, w, G.BN_EPS, dw=dw2, db=db2, accumulate=acc)
                    assert G.bits_equal(dw2, dw) and G.bits_equal(db2, db) and G.bits_equal(dx2, dx), (family, rows, C, mode, "second launch differs")
            wst.check(family, rows, C)
    _say(capsys, f"bn_bwd rows {rows:>6}: {wst.line()}")


# ------------------------------------------------------------------------------------------------ masked row softmax
@pytest.mark.parametrize("family", G.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("ncols,nvalid", G.SOFTMAX_SHAPES)
def test_softmax_rows(dev, ncols, nvalid, family, capsys):
    hip = _hip()
    wst = Worst()
    rows = G.SOFTMAX_ROWS
    s_h = G.softmax_scores(family, ncols, nvalid)
    s, Pb = s_h.to(dev), G.softmax_saved_p(s_h, nvalid).to(dev)
    for p in G.SOFTMAX_P:
        keep = G.softmax_keep(rows, ncols, p).to(dev)
        P64, Pd64 = G.softmax_fwd_ref(s, nvalid, keep, p, F64)
        P32, Pd32 = G.softmax_fwd_ref(s, nvalid, keep, p, F32)
        poison_free_memory()
        P, Pd = hip.softmax_rows_fwd(s, nvalid, p, G.SEED)
        tag = "" if p == 0 else ".drop"
        wst.add("P" + tag, G.bf16_ratio(P, P64, G.row_slack(P32, P64))[0])
        wst.add("Pd" + tag, G.bf16_ratio(Pd, Pd64, G.row_slack(Pd32, Pd64))[0])
        assert bool((P[:, nvalid:] == 0).all()) and bool((Pd[:, nvalid:] == 0).all()), (family, ncols, nvalid, p, "padding columns")
        assert bool((Pd[~keep] == 0).all()), (family, ncols, nvalid, p, "a dropped element is not 0")
        alive = keep & (P64 > 1e-30)
        assert bool((Pd[alive] != 0).all()), (family, ncols, nvalid, p, "a kept element is 0: the mask is not r * ncols + c")
        P2, Pd2 = hip.softmax_rows_fwd(s, nvalid, p, G.SEED)
        assert G.bits_equal(P2, P) and G.bits_equal(Pd2, Pd), (family, ncols, nvalid, p, "second launch differs")
        for dtype in (F32, BF):
            d = G.softmax_dpd(family, ncols, nvalid, dtype).to(dev)
            dS64 = G.softmax_bwd_ref(d, Pb, nvalid, keep, p, F64)
            dS32 = G.softmax_bwd_ref(d, Pb, nvalid, keep, p, F32)
            poison_free_memory()
            dS = hip.softmax_rows_bwd(d, Pb, nvalid, p, G.SEED)
            name = "dS." + ("f32" if dtype == F32 else "bf16") + tag
            wst.add(name, G.bf16_ratio(dS, dS64, G.row_slack(dS32, dS64))[0])
            assert bool((dS[:, nvalid:] == 0).all()), (family, ncols, nvalid, p, dtype, "padding columns")
            if family == "near_uniform":
                wst.add("rowsum" + tag, G.rowsum_ratio(dS, dS64, nvalid))
            assert G.bits_equal(hip.softmax_rows_bwd(d, Pb, nvalid, p, G.SEED), dS), (family, ncols, nvalid, p, dtype, "second launch differs")
    _say(capsys, f"softmax {family:<12} {ncols:>4} / {nvalid:>4}: {wst.line()}")
    wst.check(family, ncols, nvalid)


# ------------------------------------------------------------------------------------------------ dropout, DropPath
@pytest.mark.parametrize("n", G.DROPOUT_N)
def test_dropout(dev, n, capsys):
    hip = _hip()
    wst = Worst()
    x, res = G.flat_bf16(n, "x").to(dev), G.flat_bf16(n, "res").to(dev)
    for p in G.DROPOUT_P:
        keep = G.keep_mask(G.SEED, n, p).to(dev)
        for r in (None, res):
            y64, y32 = G.dropout_ref(x, r, keep, p, F64), G.dropout_ref(x, r, keep, p, F32)
            poison_free_memory()
            y = hip.dropout_fwd(x, r, p, G.SEED)
            wst.add("fwd" if r is None else "fwd+res", G.bf16_ratio(y, y64, _eslack(y32, y64))[0])
            if r is None:
                assert torch.equal(y != 0, keep), (n, p, "the zeroed set is not the documented mask")
            else:
                assert G.bits_equal(y[~keep], r[~keep]), (n, p, "a dropped element is not the residual")
            assert G.bits_equal(hip.dropout_fwd(x, r, p, G.SEED), y), (n, p, "second launch differs")
        d64, d32 = G.dropout_ref(x, None, keep, p, F64), G.dropout_ref(x, None, keep, p, F32)
        poison_free_memory()
        dx = hip.dropout_bwd(x, p, G.SEED)
        wst.add("bwd", G.bf16_ratio(dx, d64, _eslack(d32, d64))[0])
        assert torch.equal(dx != 0, keep), (n, p, "backward zeroes another set than forward")
        assert G.bits_equal(hip.dropout_bwd(x, p, G.SEED), dx)
    _say(capsys, f"dropout n {n:>7}: {wst.line()}")
    wst.check(n)


def test_scale_batch(dev, capsys):
    hip = _hip()
    wst = Worst()
    for batch in G.SCALE_BATCH:
        for per in G.SCALE_PER:
            x, scale = (t.to(dev) for t in G.scale_batch_case(batch, per))
            r64, r32 = x.to(F64) * scale.to(F64)[:, None], x.float() * scale[:, None]
            poison_free_memory()
            y = hip.scale_batch(x, scale)
            wst.add("y", G.bf16_ratio(y, r64, _eslack(r32, r64))[0])
            if batch > 1:
                assert bool((y[0] == 0).all()), "a dropped sample is not 0"
            assert G.bits_equal(hip.scale_batch(x, scale), y)
    _say(capsys, f"scale_batch: {wst.line()}")
    wst.check()


# ------------------------------------------------------------------------------------------------ seqmean, avgpool
def test_seqmean(dev, capsys):
    hip = _hip()
    wst = Worst()
    for B, S, C in G.SEQMEAN_SHAPES:
        x = G.seqmean_input(B, S, C).to(dev)
        m64, slack = G.seqmean_fwd_ref(x)
        dy = G.flat_bf16(B * C, "seqdy").view(B, C).to(dev)
        b64, b32 = G.seqmean_bwd_ref(dy, S, F64), G.seqmean_bwd_ref(dy, S, F32)
        poison_free_memory()
        y, dx = hip.seqmean_fwd(x), hip.seqmean_bwd(dy, S)
        wst.add("fwd", G.bf16_ratio(y, m64, slack)[0])
        wst.add("bwd", G.bf16_ratio(dx, b64, _eslack(b32, b64))[0])
        assert G.bits_equal(hip.seqmean_fwd(x), y) and G.bits_equal(hip.seqmean_bwd(dy, S), dx), (B, S, C, "second launch differs")
    _say(capsys, f"seqmean: {wst.line()}")
    wst.check()


def test_avgpool_tokens_backward(dev, capsys):
    hip = _hip()
    wst = Worst()
    for B, gh, gw, C, cs in G.AVGPOOL_SHAPES:
        dy, other = (t.to(dev) for t in G.avgpool_bwd_case(B, gh, gw, C, cs))
        for o in (None, other):
            r64, r32 = G.avgpool_bwd_ref(dy, o, B, gh, gw, cs, F64), G.avgpool_bwd_ref(dy, o, B, gh, gw, cs, F32)
            poison_free_memory()
            dx = hip.avgpool_tokens_bwd(dy, o, B, gh, gw, cs)
            wst.add("dx" if o is None else "dx+other", G.bf16_ratio(dx, r64, _eslack(r32, r64))[0])
            assert G.bits_equal(hip.avgpool_tokens_bwd(dy, o, B, gh, gw, cs), dx), (B, gh, gw, C, cs, "second launch differs")
    _say(capsys, f"avgpool_bwd: {wst.line()}")
    wst.check()


# ------------------------------------------------------------------------------------------------ lga_prep_bwd, maxpool_k_bwd
@pytest.mark.parametrize("B,N,G_,K,C", G.LGA_SHAPES)
def test_lga_prep_backward(dev, B, N, G_, K, C, capsys):
    hip = _hip()
    wst = Worst()
    for lists in G.LGA_LISTS:
        drows, fps, knn, unused = G.lga_bwd_case(B, N, G_, K, C, lists)
        e64, sab, cnt = G.lga_bwd_emul(drows, fps, knn, B, N, C, F64)
        e32 = G.lga_bwd_emul(drows, fps, knn, B, N, C, F32)[0]
        poison_free_memory()
        got = hip.lga_prep_bwd(drows.to(dev), fps.to(dev), knn.to(dev), B, N, C)
        wst.add(lists, G.reduction_ratio(got.cpu(), e64, int(cnt.max()), sab))
        assert G.bits_equal(got.cpu(), e32), (lists, "not the documented order: ascending g, ascending k, then the centre's k-sum")
        for n in unused:
            assert bool((got[:, n] == 0).all()), (lists, n, "a point in no list does not read 0")
        assert G.bits_equal(hip.lga_prep_bwd(drows.to(dev), fps.to(dev), knn.to(dev), B, N, C), got), "second launch differs"
    _say(capsys, f"lga_prep_bwd B {B} N {N} G {G_} K {K} C {C}: {wst.line()}")
    wst.check(B, N, G_, K, C)


def test_maxpool_k_backward(dev):
    hip = _hip()
    for groups in G.POOL_GROUPS:
        for K in G.POOL_K:
            for C in G.POOL_C:
                x, dy = G.pool_bwd_case(groups, K, C)
                ref = G.pool_bwd_ref(x, dy, groups, K)
                poison_free_memory()
                dx = hip.maxpool_k_bwd(x.to(dev), dy.to(dev), groups, K)
                assert G.bits_equal(dx.cpu(), ref), (groups, K, C)
                assert G.bits_equal(hip.maxpool_k_bwd(x.to(dev), dy.to(dev), groups, K), dx)


# ------------------------------------------------------------------------------------------------ chamfer
@pytest.mark.parametrize("B,N,M", G.CHAMFER_SHAPES)
def test_chamfer(dev, B, N, M, capsys):
    hip = _hip()
    wst = Worst()
    gs = torch.tensor([G.IMG_GSCALE], device=dev)
    for cloud in G.CHAMFER_CLOUDS:
        pred, gt = (t.to(dev) for t in G.chamfer_case(cloud, B, N, M))
        r = G.chamfer_fwd_ref(pred, gt)
        poison_free_memory()
        loss, d1, i1, d2, i2 = hip.chamfer_fwd(pred, gt)
        exact = cloud == "lattice16"
        r1, bad1 = G.chamfer_dist_check(d1, i1, r["sq"], r["delta"], exact)
        r2, bad2 = G.chamfer_dist_check(d2, i2, r["sq"].transpose(1, 2), r["delta"].transpose(1, 2), exact)
        assert bad1 == 0 and bad2 == 0, (cloud, B, N, M, bad1, bad2, "indices outside the band (lattice16: not the first minimum)")
        wst.add("d1", r1)
        wst.add("d2", r2)
        wst.add("loss", G.chamfer_loss_ratio(loss, d1, d2))
        again = hip.chamfer_fwd(pred, gt)
        assert all(G.bits_equal(a, b) for a, b in zip(again, (loss, d1, i1, d2, i2))), (cloud, "second launch differs")
        # backward from the host-built fp64 minima, so that ties cannot split the comparison
        hd1, hd2, hi1, hi2 = r["d1"].float(), r["d2"].float(), r["i1"].int(), r["i2"].int()
        dp64, sab, cnt = G.chamfer_bwd_ref(pred, gt, hd1, hi1, hd2, hi2, gs, F64)
        poison_free_memory()
        dp = hip.chamfer_bwd(pred, gt, hd1, hi1, hd2, hi2, gs)
        wst.add("dpred", G.reduction_ratio(dp, dp64, int(cnt.max()), sab))
        if cloud == "coincident":
            k = min(3, N, M)
            assert bool(torch.isfinite(dp).all()) and bool((d1[:, :k] == 0).all()), "coincident points: distance 0, a finite gradient"
        assert G.bits_equal(hip.chamfer_bwd(pred, gt, hd1, hi1, hd2, hi2, gs), dp), (cloud, "second launch differs")
    _say(capsys, f"chamfer B {B} N {N:>4} M {M:>4}: {wst.line()}")
    wst.check(B, N, M)


# ------------------------------------------------------------------------------------------------ image losses
def _imgloss_cases():
    for ps, HW in G.IMG_GEOM:
        for ld in G.img_lds(ps):
            for dtype in (F32, BF):
                yield ps, HW, ld, dtype


@pytest.mark.parametrize("ps,HW,ld,dtype", list(_imgloss_cases()))
def test_imgloss(dev, ps, HW, ld, dtype, capsys):
    hip = _hip()
    wst = Worst()
    pd = 3 * ps * ps
    draw, curr, nxt = (t.to(dev) for t in G.imgloss_case(ps, HW, ld, dtype))
    gs = torch.tensor([G.IMG_GSCALE], device=dev)
    r64 = G.imgloss_ref(draw, curr, nxt, ps, G.IMG_CLIP, gs, F64)
    r32 = G.imgloss_ref(draw, curr, nxt, ps, G.IMG_CLIP, gs, F32)
    assert int(G.kink_sets(r64, None, ps)[0].sum()) == 0
    poison_free_memory()
    sums = hip.imgloss_fwd(draw, curr, nxt, ps, G.IMG_CLIP)
    dd = hip.imgloss_bwd(draw, curr, nxt, ps, G.IMG_CLIP, gs)
    for k, name in enumerate(("sum_sq", "sum_l1", "sum_delta")):
        wst.add(name, G.fp32_ratio(sums[k:k + 1], r64["sums"][k:k + 1], r32["sums"][k:k + 1], r64["n"], r64["sumabs"][k:k + 1]))
    wst.add("ddraw", G.bf16_ratio(dd[..., :pd], r64["ddraw"], _eslack(r32["ddraw"], r64["ddraw"]))[0])
    assert bool((dd[..., pd:] == 0).all()), "padding columns of ddraw"
    assert G.bits_equal(hip.imgloss_fwd(draw, curr, nxt, ps, G.IMG_CLIP), sums) and G.bits_equal(hip.imgloss_bwd(draw, curr, nxt, ps, G.IMG_CLIP, gs), dd)
    _say(capsys, f"imgloss ps {ps:>2} HW {HW:>3} ld {ld:>4} {str(dtype)[6:]:<8}: {wst.line()}")
    wst.check(ps, HW, ld, dtype)


def _imgroi_cases():
    for ps, HW in G.IMG_GEOM:
        for i, (mask, shifts) in enumerate(G.ROI_CASES):
            for j, dtype in enumerate((F32, BF)):
                yield ps, HW, G.img_lds(ps)[(i + j) % 2], dtype, mask, shifts


@pytest.mark.parametrize("ps,HW,ld,dtype,mask,shifts", list(_imgroi_cases()))
def test_imgroi(dev, ps, HW, ld, dtype, mask, shifts, capsys):
    hip = _hip()
    wst = Worst()
    pd = 3 * ps * ps
    draw, a, o, roi, curr, nxt = (t.to(dev) for t in G.imgroi_case(ps, HW, ld, dtype, mask, shifts))
    n = roi.numel()
    coef = G.roi_coef(roi, n, ps).to(dev)
    r64 = G.imgroi_ref(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef, F64)
    r32 = G.imgroi_ref(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef, F32)
    el, pt = G.kink_sets(r64, shifts, ps)
    assert int(el.sum()) == 0 and int(pt.sum()) == 0
    poison_free_memory()
    sums = hip.imgroi_fwd(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT)
    dd, da, do = hip.imgroi_bwd(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef)
    for k, name in enumerate(("roi_sq", "roi_l1", "bg_l1", "delta")):
        wst.add(name, G.fp32_ratio(sums[k:k + 1], r64["sums"][k:k + 1], r32["sums"][k:k + 1], n * pd, r64["sumabs"][k:k + 1]))
    wst.add("ddraw", G.bf16_ratio(dd[..., :pd], r64["ddraw"], _eslack(r32["ddraw"], r64["ddraw"]))[0])
    wst.add("dalpha", G.fp32_ratio(da, r64["dalpha"], r32["dalpha"], pd, r64["dalpha_abs"]))
    wst.add("doff", G.fp32_ratio(do, r64["doff"], r32["doff"], pd, r64["doff_abs"]))
    assert bool((dd[..., pd:] == 0).all()), "padding columns of ddraw"
    inroi = roi.bool()
    assert bool((da[inroi] == 0).all()) and bool((do[inroi] == 0).all()), "an ROI patch has no alpha / offset gradient"
    dd2, da2, do2 = hip.imgroi_bwd(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef)
    assert G.bits_equal(hip.imgroi_fwd(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT), sums)
    assert G.bits_equal(dd2, dd) and G.bits_equal(da2, da) and G.bits_equal(do2, do), "second launch differs"
    _say(capsys, f"imgroi ps {ps:>2} HW {HW:>3} ld {ld:>4} {str(dtype)[6:]:<8} {mask:<6} {shifts:<6}: {wst.line()}")
    wst.check(ps, HW, ld, dtype, mask, shifts)
