"""CPU checks of tests/gen_cases.py, the helper module of tests/test_gen_kernels_gpu.py: every fp64 reference against an independent
torch formulation (F.layer_norm / F.batch_norm / torch.softmax / F.avg_pool2d autograd, index_add_, oracle.gen_oracle for chamfer and
both image losses), every fp32 evaluation inside the bound it will be used with, the sentinel property of every reduction family, the
empty kink sets of every image case, the keep fraction of the documented dropout hash, a set of plausible mutations -- a dropped last
row, a dropped last valid column, a mask index shifted by one, a missing renormalisation, the last maximum instead of the first,
CT_curr swapped for CT_next, a second-nearest neighbour -- each of which must land far outside its bound, and the argument checks of the
C ABI of these kernels (on the host, before any launch)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import gen_cases as G
from oracle import gen_oracle

BF, F32, F64 = G.BF, G.F32, G.F64
P = ctypes.c_void_p(16)


def _emul(ref32):
    """An honest kernel: the fp32 evaluation rounded once to bf16."""
    return ref32.to(BF)


def _close(a, b, tol):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * (float(b.abs().max()) + 1e-300)


# ------------------------------------------------------------------------------------------------ dropout hash
def test_hash_known_structure_and_keep_fraction():
    n = 1 << 20
    for seed in (0, G.SEED, 2 ** 64 - 1):
        for p in (0.1, 0.5, 0.999):
            k = G.keep_mask(seed, n, p)
            sd = math.sqrt(p * (1 - p) / n)
            assert abs(float(k.double().mean()) - (1 - G.f32v(p))) <= 5 * sd, (seed, p)
        assert bool(G.keep_mask(seed, 1000, 0.0).all())
    # a function of the flat index alone: any window of a longer mask is the mask of that window
    a = G.keep_mask(G.SEED, 5000, 0.5)
    assert torch.equal(a[1234:1234 + 777], G.keep_mask(G.SEED, 777, 0.5, offset=1234))
    assert not torch.equal(a[1:4001], a[:4000]) and not torch.equal(a, G.keep_mask(G.SEED + 1, 5000, 0.5))
    # the hash of (0, 0) is 0 by construction (every step maps 0 to 0): p > 0 drops index 0 of seed 0
    assert int(G.hash_u32(0, [0])[0]) == 0 and not bool(G.keep_mask(0, 1, 0.1)[0])


@pytest.mark.parametrize("p", G.DROPOUT_P)
def test_dropout_reference_and_shifted_mask(p):
    n = 1003
    x, res = G.flat_bf16(n, "x"), G.flat_bf16(n, "res")
    keep = G.keep_mask(G.SEED, n, p)
    for r in (None, res):
        r64, r32 = G.dropout_ref(x, r, keep, p, F64), G.dropout_ref(x, r, keep, p, F32)
        assert G.bf16_ratio(_emul(r32), r64, (r32.double() - r64).abs())[0] <= 1
        if 0 < p <= 0.5:                     # at 0.999 both masks drop nearly everything
            shifted = G.dropout_ref(x, r, G.keep_mask(G.SEED, n, p, offset=1), p, F32)
            assert G.bf16_ratio(_emul(shifted), r64, (r32.double() - r64).abs())[0] > 100, "a mask indexed by i + 1"
    if p > 0 and bool(keep.any()):
        assert _close(G.dropout_ref(x, None, keep, p, F64)[keep], x.double()[keep] / (1 - G.f32v(p)), 1e-15)


def test_scale_batch_case():
    for batch in G.SCALE_BATCH:
        x, s = G.scale_batch_case(batch, 7)
        assert s.shape == (batch,) and (batch == 1 or (float(s[0]) == 0 and float(s[2]) < 0))


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("family", G.LN_FAMILIES)
def test_layernorm_forward_reference(family):
    for H in G.LN_H:
        for rows in G.LN_ROWS:
            x, w, b = G.norm_rows(family, rows, H), G.norm_weight(H), G.norm_bias(H)
            y64, m64, r64 = G.ln_stats_ref(x, w, b, G.LN_EPS, F64)
            y32, m32, r32 = G.ln_stats_ref(x, w, b, G.LN_EPS, F32)
            t = F.layer_norm(x.double(), (H,), w.double(), b.double(), G.f32v(G.LN_EPS))
            assert _close(y64, t, 1e-12), (family, H, rows)
            assert _close(m64, x.double().mean(-1), 1e-12) and _close(r64, 1 / torch.sqrt(x.double().var(-1, unbiased=False) + G.f32v(G.LN_EPS)), 1e-12)
            assert G.bf16_ratio(_emul(y32), y64, G.row_slack(y32, y64))[0] <= 1
            assert G.mean_ratio(m32, x) <= 1 and G.scalar_ratio(r32, r64) <= 1, (family, H, rows)
            if family != "tiny" and H > 8:
                bad = 1 / torch.sqrt(x.double()[:, :-8].var(-1, unbiased=False) * (H - 8) / H + G.f32v(G.LN_EPS))
                assert G.scalar_ratio(bad.float(), r64) > 1, (family, H, "a variance that skips the last chunk")


@pytest.mark.parametrize("rows,H", G.LN_BWD_SHAPES)
def test_layernorm_backward_reference(rows, H):
    w, dy = G.norm_weight(H), G.norm_dy(rows, H)
    for family in G.LN_FAMILIES:
        x = G.norm_rows(family, rows, H, "bwd")
        _, m64, r64 = G.ln_stats_ref(x, w, G.norm_bias(H), G.LN_EPS, F64)
        mean, rstd = m64.float(), r64.float()
        dx64, tw64, tb64 = G.ln_bwd_ref(dy, x, w, mean, rstd, F64)
        dx32, tw32, tb32 = G.ln_bwd_ref(dy, x, w, mean, rstd, F32)
        assert G.bf16_ratio(_emul(dx32), dx64, G.row_slack(dx32, dx64))[0] <= 1, (family, "dx")
        base = G.flat_bf16(H, "dwbase").float()
        for t32, t64 in ((tw32, tw64), (tb32, tb64)):
            assert G.dw_check(t32.sum(0), t64) <= 1 and G.dw_check(base + t32.sum(0), t64, base.double()) <= 1
            bound = G.reduction_bound(rows, t64.abs().sum(0))
            assert G.sentinel_ratio(t64, bound, G.bwd_sentinel_rows(rows)) >= 100, (family, rows, H)
            if rows > 1:
                assert G.dw_check(t32[:-1].sum(0), t64) > 100, (family, "a sum that skips the last row")
        if family == "gauss" and rows <= 37:
            xa, wa = x.double().requires_grad_(), w.double().requires_grad_()
            ba = torch.zeros(H, dtype=F64, requires_grad=True)
            F.layer_norm(xa, (H,), wa, ba, G.f32v(G.LN_EPS)).backward(dy.double())
            # the statistics are the fp32 roundings of the exact ones: agreement to their 2^-24
            assert _close(dx64, xa.grad, 1e-5) and _close(tw64.sum(0), wa.grad, 1e-5) and _close(tb64.sum(0), ba.grad, 1e-12)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
@pytest.mark.parametrize("rows", G.BN_ROWS)
def test_bn_backward_reference(rows):
    for C in (G.BN_C if rows <= 3000 else G.BN_C_LARGE):
        for family in G.BN_FAMILIES:
            dy, x, w, mean, var = G.bn_case(family, rows, C)
            dx64, tw64, tb64 = G.bn_bwd_ref(dy, x, w, mean, var, G.BN_EPS, F64)
            dx32, tw32, tb32 = G.bn_bwd_ref(dy, x, w, mean, var, G.BN_EPS, F32)
            slack = (dx32.double() - dx64).abs().amax(0, keepdim=True)
            assert G.bf16_ratio(_emul(dx32), dx64, slack)[0] <= 1, (family, rows, C)
            for name, t32, t64 in (("dw", tw32, tw64), ("db", tb32, tb64)):
                assert G.dw_check(t32.sum(0), t64) <= 1, (family, rows, C, name)
                assert G.dw_check(G.bn_sums_emul32(t32), t64) <= 1, (family, rows, C, name, "the honest fp32 sum in the kernel's order")
                if name == "db" or (C >= 63 and rows >= 3):
                    bound = G.reduction_bound(rows, t64.abs().sum(0))
                    assert G.sentinel_ratio(t64, bound, G.bn_sentinel_rows(rows)) >= 100, (family, rows, C, name)
            if rows > 1:
                assert G.dw_check(tb32[:-1].sum(0), tb64) > 100, "a db that skips the last row"
            if family in ("gauss", "constcol") and 3 <= rows <= 3000:
                xa, wa = x.double().requires_grad_(), w.double().requires_grad_()
                ba = torch.zeros(C, dtype=F64, requires_grad=True)
                F.batch_norm(xa, None, None, wa, ba, True, 0.0, G.f32v(G.BN_EPS)).backward(dy.double())
                assert _close(dx64, xa.grad, 1e-4) and _close(tw64.sum(0), wa.grad, 1e-4) and _close(tb64.sum(0), ba.grad, 1e-12), (family, rows, C)
    assert G.bn_blocks(2047) == 1 and G.bn_blocks(2048) == 2 and G.bn_blocks(3000) == 2 and G.bn_blocks(132101) == 128
    assert len(G.bn_sentinel_rows(3000)) == 4 and G.bn_sentinel_rows(3000)[1:3] == [1499, 1500]


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("ncols,nvalid", G.SOFTMAX_SHAPES)
def test_softmax_references(ncols, nvalid):
    rows = G.SOFTMAX_ROWS
    for family in G.SOFTMAX_FAMILIES:
        s = G.softmax_scores(family, ncols, nvalid)
        assert bool(torch.isnan(s[:, nvalid:]).all())
        for p in G.SOFTMAX_P:
            keep = G.softmax_keep(rows, ncols, p)
            P64, Pd64 = G.softmax_fwd_ref(s, nvalid, keep, p, F64)
            P32, Pd32 = G.softmax_fwd_ref(s, nvalid, keep, p, F32)
            assert _close(P64[:, :nvalid], torch.softmax(s[:, :nvalid].double(), -1), 1e-13)
            assert not bool(torch.isnan(P64).any()) and bool((P64[:, nvalid:] == 0).all()) and bool((Pd64[~keep] == 0).all())
            assert G.bf16_ratio(_emul(P32), P64, G.row_slack(P32, P64))[0] <= 1
            assert G.bf16_ratio(_emul(Pd32), Pd64, G.row_slack(Pd32, Pd64))[0] <= 1
            if nvalid > 1 and family != "near_uniform":
                lost = G.softmax_fwd_ref(s, nvalid - 1, keep, p, F32)[0]
                if family == "spike" or nvalid <= 64:
                    assert G.bf16_ratio(_emul(lost), P64, G.row_slack(P32, P64))[0] > 100, (family, "the last valid column dropped")
            if p > 0 and nvalid >= 45:
                wrong = G.keep_mask(G.SEED, rows * nvalid, p).view(rows, nvalid)        # indexed by r * nvalid + c
                if nvalid != ncols:
                    assert not torch.equal(wrong, keep[:, :nvalid])
            Pb = G.softmax_saved_p(s, nvalid)
            for dtype in (F32, BF):
                d = G.softmax_dpd(family, ncols, nvalid, dtype)
                dS64 = G.softmax_bwd_ref(d, Pb, nvalid, keep, p, F64)
                dS32 = G.softmax_bwd_ref(d, Pb, nvalid, keep, p, F32)
                assert not bool(torch.isnan(dS64).any()) and bool((dS64[:, nvalid:] == 0).all())
                assert G.bf16_ratio(_emul(dS32), dS64, G.row_slack(dS32, dS64))[0] <= 1, (family, p, dtype)
                if family == "near_uniform":
                    assert float(dS64.sum(-1).abs().max()) <= 1e-12 * nvalid * float(dS64.abs().max())
                    assert G.rowsum_ratio(_emul(dS32), dS64, nvalid) <= 1, (family, p, dtype)
        # the reference on exact probabilities is autograd through softmax
        xa = s[:, :nvalid].double().clone().requires_grad_()
        d = G.softmax_dpd(family, ncols, nvalid, F32)
        pa = torch.softmax(xa, -1)
        pa.backward(d[:, :nvalid].double())
        keep1 = torch.ones(rows, ncols, dtype=torch.bool)
        exact = G.softmax_bwd_ref(d, G.softmax_fwd_ref(s, nvalid, keep1, 0.0, F64)[0], nvalid, keep1, 0.0, F64)
        assert _close(exact[:, :nvalid], xa.grad, 1e-11), family


def test_softmax_invariant_sees_a_missing_renormalisation():
    """The round-6 case: ~550 near-uniform keys, dPd a large common value plus a small variation. Without P' = P / sum(P) the row sum
    of dS is (1 - sum P) dot, far outside the rounding of dS."""
    ncols, nvalid = 552, 548
    s = G.softmax_scores("near_uniform", ncols, nvalid)
    keep = torch.ones(G.SOFTMAX_ROWS, ncols, dtype=torch.bool)
    Pb, d = G.softmax_saved_p(s, nvalid), G.softmax_dpd("near_uniform", ncols, nvalid, F32)
    dS64 = G.softmax_bwd_ref(d, Pb, nvalid, keep, 0.0, F64)
    pr, g = Pb[:, :nvalid].float(), d[:, :nvalid]
    plain = torch.zeros(G.SOFTMAX_ROWS, ncols)
    plain[:, :nvalid] = pr * (g - (g * pr).sum(-1, keepdim=True))
    assert G.rowsum_ratio(_emul(plain), dS64, nvalid) > 10
    assert G.bf16_ratio(_emul(plain), dS64, G.row_slack(G.softmax_bwd_ref(d, Pb, nvalid, keep, 0.0, F32), dS64))[0] > 5


# ------------------------------------------------------------------------------------------------ seqmean, avgpool, lga, maxpool
def test_seqmean_and_avgpool_references():
    for B, S, C in G.SEQMEAN_SHAPES:
        x = G.seqmean_input(B, S, C)
        m64, slack = G.seqmean_fwd_ref(x)
        assert _close(m64, x.double().mean(1), 1e-13)
        seq = torch.zeros(B, C)
        for t in range(S):
            seq = seq + x[:, t].float()
        assert G.bf16_ratio(_emul(seq / S), m64, slack)[0] <= 1
        if S > 1:
            assert G.bf16_ratio(_emul(x[:, :-1].float().sum(1) / S), m64, slack)[0] > 100, "the last position dropped"
        xa = x.double().requires_grad_()
        dy = G.flat_bf16(B * C, "seqdy").view(B, C)
        xa.mean(1).backward(dy.double())
        assert _close(G.seqmean_bwd_ref(dy, S, F64), xa.grad, 1e-14)
    for B, gh, gw, C, cs in G.AVGPOOL_SHAPES:
        dy, other = G.avgpool_bwd_case(B, gh, gw, C, cs)
        xa = torch.zeros(B, gh, gw, C, dtype=F64, requires_grad=True)
        pooled = F.avg_pool2d(xa.permute(0, 3, 1, 2), cs).permute(0, 2, 3, 1).reshape(-1, C)
        (pooled * dy.double()).sum().backward()
        for o in (None, other):
            want = xa.grad.reshape(-1, C) + (0 if o is None else o.double())
            r64, r32 = G.avgpool_bwd_ref(dy, o, B, gh, gw, cs, F64), G.avgpool_bwd_ref(dy, o, B, gh, gw, cs, F32)
            assert _close(r64, want, 1e-14)
            assert G.bf16_ratio(_emul(r32), r64, (r32.double() - r64).abs())[0] <= 1
        if cs > 1 and dy.shape[0] > 1:
            swapped = G.avgpool_bwd_ref(dy, None, B, gw, gh, cs, F32) if gh != gw else G.avgpool_bwd_ref(dy.flip(0), None, B, gh, gw, cs, F32)
            assert G.bf16_ratio(_emul(swapped), G.avgpool_bwd_ref(dy, None, B, gh, gw, cs, F64), torch.zeros(()))[0] > 100


@pytest.mark.parametrize("B,N,G_,K,C", G.LGA_SHAPES)
def test_lga_backward_emulation(B, N, G_, K, C):
    for lists in G.LGA_LISTS:
        drows, fps, knn, unused = G.lga_bwd_case(B, N, G_, K, C, lists)
        assert all(len(set(fps[b].tolist())) == G_ for b in range(B)), "FPS indices are distinct"
        e64, sab, cnt = G.lga_bwd_emul(drows, fps, knn, B, N, C, F64)
        e32 = G.lga_bwd_emul(drows, fps, knn, B, N, C, F32)[0]
        want = G.lga_bwd_index_add(drows, fps, knn, B, N, C)
        assert _close(e64, want, 1e-13), lists
        assert G.reduction_ratio(e32, e64, int(cnt.max()), sab) <= 1
        for n in unused:
            assert bool((e64[:, n] == 0).all()) and bool((cnt[:, n] == 0).all())
        if lists == "hostile":
            assert bool((knn[:, ::2, 0].long() == fps[:, ::2]).all()) and bool((knn[:, :, K - 1] == knn[0, 0, K - 1]).all())
            assert int(cnt.max()) >= G_
        if K > 1 and unused:
            # a kernel that loses position K - 1 of every hit mask (K > 32: a bit of another word): those rows go to a spare point
            moved = knn.clone()
            moved[:, :, K - 1] = unused[0]
            lost = G.lga_bwd_emul(drows, fps, moved, B, N, C, F32)[0]
            lost[:, unused[0]] = 0
            assert G.reduction_ratio(lost, e64, int(cnt.max()), sab) > 100


def test_maxpool_backward_reference():
    for groups in G.POOL_GROUPS:
        for K in G.POOL_K:
            for C in G.POOL_C:
                x, dy = G.pool_bwd_case(groups, K, C)
                ref = G.pool_bwd_ref(x, dy, groups, K)
                xa = x.double().view(groups, K, C)
                assert bool(((ref.view(groups, K, C) != 0).sum(1) == 1).all()), "one neighbour per (group, channel) takes the gradient"
                took = (ref.view(groups, K, C) != 0)
                top = xa.amax(1, keepdim=True).expand_as(xa)
                assert bool((xa[took] == top[took]).all())
                assert bool((ref.view(groups, K, C)[:, 0, 0] == dy[:, 0]).all()), "all-equal column: the first neighbour"
                if C > 1:
                    assert bool((ref.view(groups, K, C)[:, 0, C - 1] == dy[:, C - 1]).all()), "-inf column: the first neighbour"
                if K > 1:
                    assert not G.bits_equal(G.pool_bwd_ref(x, dy, groups, K, last=True), ref), "the last maximum is told from the first"


# ------------------------------------------------------------------------------------------------ chamfer
@pytest.mark.parametrize("B,N,M", G.CHAMFER_SHAPES)
def test_chamfer_references(B, N, M):
    gs = torch.tensor([G.IMG_GSCALE])
    for cloud in G.CHAMFER_CLOUDS:
        pred, gt = G.chamfer_case(cloud, B, N, M)
        r = G.chamfer_fwd_ref(pred, gt)
        # an honest fp32 kernel: squared distances in fp32, first minimum, square root
        sq32 = ((pred[:, :, None, :] - gt[:, None, :, :]) ** 2).sum(-1)
        for d64, sqv, dl, axis in ((r["d1"], r["sq"], r["delta"], 2), (r["d2"], r["sq"].transpose(1, 2), r["delta"].transpose(1, 2), 1)):
            mn32, i32 = (sq32 if axis == 2 else sq32.transpose(1, 2)).min(-1)
            ratio, bad = G.chamfer_dist_check(mn32.sqrt(), i32.int(), sqv, dl, exact=False)
            assert ratio <= 1 and bad == 0, (cloud, axis, ratio, bad)
            if sqv.shape[-1] > 1 and cloud == "uniform":
                second = sqv.topk(2, -1, largest=False)
                ratio, bad = G.chamfer_dist_check(second.values[..., 1].sqrt().float(), second.indices[..., 1].int(), sqv, dl, exact=False)
                assert ratio > 100 and bad > 0, "the second-nearest neighbour"
        if cloud == "lattice16":
            assert G.bits_equal(sq32.double(), r["sq"]), "fp32 arithmetic is exact on the lattice"
        if cloud == "coincident":
            k = min(3, N, M)
            assert bool((r["d1"][:, :k] == 0).all())
        d1, d2 = r["d1"].float(), r["d2"].float()
        want = gen_oracle.chamfer_distance_l2(pred.double(), gt.double())
        t = torch.cat([d1.double().reshape(-1) / (B * N), d2.double().reshape(-1) / (B * M)])
        assert abs(float(t.sum()) - float(want)) <= 1e-6 * float(want) + 1e-12
        assert G.chamfer_loss_ratio(t.float().sum(), d1, d2) <= 1
        dp64, sab, cnt = G.chamfer_bwd_ref(pred, gt, d1, r["i1"], d2, r["i2"], gs, F64)
        dp32 = G.chamfer_bwd_ref(pred, gt, d1, r["i1"], d2, r["i2"], gs, F32)[0]
        assert bool(torch.isfinite(dp64).all())
        assert G.reduction_ratio(dp32, dp64, int(cnt.max()), sab) <= 1, cloud
        if cloud in ("uniform", "offset") and N * M <= 128 * 300:
            pa = pred.double().requires_grad_()
            (gen_oracle.chamfer_distance_l2(pa, gt.double()) * gs.double()[0]).backward()
            assert _close(dp64, pa.grad, 1e-5), cloud
        if N > 1 and cloud == "uniform":
            i2b = (r["i2"] + 1) % N
            assert G.reduction_ratio(G.chamfer_bwd_ref(pred, gt, d1, r["i1"], d2, i2b, gs, F32)[0], dp64, int(cnt.max()), sab) > 100


# ------------------------------------------------------------------------------------------------ image losses
def _imgloss_cases():
    for ps, HW in G.IMG_GEOM:
        for ld in G.img_lds(ps):
            for dtype in (F32, BF):
                yield ps, HW, ld, dtype


@pytest.mark.parametrize("ps,HW,ld,dtype", list(_imgloss_cases()))
def test_imgloss_reference(ps, HW, ld, dtype):
    draw, curr, nxt = G.imgloss_case(ps, HW, ld, dtype)
    gs = torch.tensor([G.IMG_GSCALE])
    r64 = G.imgloss_ref(draw, curr, nxt, ps, G.IMG_CLIP, gs, F64)
    r32 = G.imgloss_ref(draw, curr, nxt, ps, G.IMG_CLIP, gs, F32)
    el, _ = G.kink_sets(r64, None, ps)
    assert int(el.sum()) == 0, "no element under a kink guard: nothing is left out (cap: 0.1 %)"
    assert G.fp32_ratio(r32["sums"], r64["sums"], r32["sums"], r64["n"], r64["sumabs"]) <= 1
    assert G.bf16_ratio(_emul(r32["ddraw"]), r64["ddraw"], (r32["ddraw"].double() - r64["ddraw"]).abs())[0] <= 1
    swapped = G.imgloss_ref(draw, curr, nxt, ps, G.IMG_CLIP, gs, F32, ct_curr=G.IMG_CTN)
    assert G.fp32_ratio(swapped["sums"][:2], r64["sums"][:2], r32["sums"][:2], r64["n"], r64["sumabs"][:2]) > 100, "CT_curr swapped for CT_next"
    if HW <= 84:
        pd = 3 * ps * ps
        da = draw[..., :pd].double().requires_grad_()
        loss, parts = gen_oracle.image_generation_loss(G.IMG_CLIP * torch.tanh(da), curr.double(), nxt.double(), ps)
        (loss * gs.double()[0]).backward()
        n = r64["n"]
        # the reference carries 0.05 and 0.1 as the kernels' fp32 constants: agreement with the oracle's doubles to 2^-24
        assert _close(r64["sums"] / n, torch.stack([parts["mse"], parts["l1"], parts["delta_abs"]]).detach(), 1e-7)
        assert _close(r64["ddraw"], da.grad, 1e-7)


def _imgroi_cases():
    for ps, HW in G.IMG_GEOM:
        for i, (mask, shifts) in enumerate(G.ROI_CASES):
            for j, dtype in enumerate((F32, BF)):
                yield ps, HW, G.img_lds(ps)[(i + j) % 2], dtype, mask, shifts


@pytest.mark.parametrize("ps,HW,ld,dtype,mask,shifts", list(_imgroi_cases()))
def test_imgroi_reference(ps, HW, ld, dtype, mask, shifts):
    draw, a, o, roi, curr, nxt = G.imgroi_case(ps, HW, ld, dtype, mask, shifts)
    n, pd = roi.numel(), 3 * ps * ps
    coef = G.roi_coef(roi, n, ps)
    r64 = G.imgroi_ref(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef, F64)
    r32 = G.imgroi_ref(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef, F32)
    el, pt = G.kink_sets(r64, shifts, ps)
    assert int(el.sum()) == 0 and int(pt.sum()) == 0, "no element and no patch under a kink guard (caps: 0.1 % / 2 %)"
    assert G.fp32_ratio(r32["sums"], r64["sums"], r32["sums"], n * pd, r64["sumabs"]) <= 1
    assert G.bf16_ratio(_emul(r32["ddraw"]), r64["ddraw"], (r32["ddraw"].double() - r64["ddraw"]).abs())[0] <= 1
    assert G.fp32_ratio(r32["dalpha"], r64["dalpha"], r32["dalpha"], pd, r64["dalpha_abs"]) <= 1
    assert G.fp32_ratio(r32["doff"], r64["doff"], r32["doff"], pd, r64["doff_abs"]) <= 1
    if shifts == "border":
        sx, sy = r64["coord"]
        assert float(sx.min()) < 0 and float(sx.max()) > ps - 1 and float(sy.min()) < 0 and float(sy.max()) > ps - 1
    if mask in ("random", "none"):
        swapped = G.imgroi_ref(draw, a, o, roi, curr, nxt, ps, G.IMG_CLIP, G.IMG_SHIFT, coef, F32, ct_curr=G.IMG_CTN)
        assert G.fp32_ratio(swapped["sums"][2:3], r64["sums"][2:3], r32["sums"][2:3], n * pd, r64["sumabs"][2:3]) > 100
    if HW == G.IMG_GEOM[2][1]:
        # autograd through the oracle (it samples in fp32: agreement to fp32 accuracy)
        B = G.IMG_B
        da = draw[..., :pd].float().requires_grad_()
        aa, oa = a[:, 0].float().requires_grad_(), o[:, :2].float().requires_grad_()
        loss, _ = gen_oracle.image_generation_roi_loss(G.IMG_CLIP * torch.tanh(da), torch.sigmoid(aa).view(B, -1), (G.IMG_SHIFT * torch.tanh(oa)).view(B, -1, 2),
                                                       roi.bool().view(B, -1), curr.float(), nxt.float(), ps)
        (loss * G.IMG_GSCALE).backward()
        s, nr = r64["sums"], int(roi.sum()) * pd
        want = (s[0] / nr + 0.5 * s[1] / nr if nr else 0.0) + (0.01 * s[2] / (n * pd - nr) if n * pd > nr else 0.0) - 0.1 * s[3] / (n * pd)
        assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
        assert _close(r64["ddraw"], da.grad, 1e-4) and _close(r64["dalpha"], aa.grad, 1e-3 if mask != "all" else 1.0)
        if shifts != "zero" and mask != "all":
            assert _close(r64["doff"], oa.grad, 1e-3)
        if mask == "all":
            assert float(r64["dalpha"].abs().max()) == 0 and float(r64["doff"].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ C ABI
def test_backward_entry_points_reject_what_their_forward_twins_reject():
    from mla_amd import hip
    lib = hip.lib()

    def bad(name, *args, msg=None):
        rc = getattr(lib, name)(*args, None)
        err = lib.mla_last_error()
        assert rc < 0 and name.encode() in err and (msg is None or msg in err), (name, args, rc, err)
    pd = 3 * 6 * 6
    for name, pre in (("mla_imgloss_fwd", (P, P, 1, P)), ("mla_imgloss_bwd", (P, P, 1, P, P))):
        tail = (P, 1 << 20) if name.endswith("fwd") else ()
        bad(name, P, pd - 1, *pre, 2, 4, 3, 24, 6, 5.0, *tail)
        bad(name, P, pd, *pre, 2, 4, 3, 25, 6, 5.0, *tail)
        bad(name, P, pd, *pre, 2, 4, 3, 24, 0, 5.0, *tail)
    for name, mid, tail in (("mla_imgroi_fwd", (P,), (P, 1 << 20)), ("mla_imgroi_bwd", (P, P, P, P), ())):
        for ld, ldo, HW, ps in ((pd - 1, 8, 24, 6), (pd, 8, 25, 6), (pd, 1, 24, 6), (pd, 8, 24, 0)):
            bad(name, P, ld, P, 8, P, ldo, P, P, P, 1, *mid, 2, 4, 3, HW, ps, 5.0, 8.0, *tail)
    bad("mla_bn_bwd", P, P, P, P, P, P, None, None, 0, 4, 0, 1e-5, P, 1 << 20)
    bad("mla_bn_bwd", P, P, P, P, P, P, None, None, 0, 0, 8, 1e-5, P, 1 << 20)
    for nvalid, p in ((0, 0.0), (9, 0.0), (4, 1.0), (4, -0.5)):
        bad("mla_softmax_rows_bwd", P, 1, P, P, 2, 8, nvalid, p, 1)
        bad("mla_softmax_rows_fwd", P, P, P, 2, 8, nvalid, p, 1)
    bad("mla_dropout_bwd", P, P, 8, 1.0, 1)
    for dims in ((0, 3, 8), (2, 0, 8), (2, 3, 0)):
        bad("mla_seqmean_bwd", P, P, *dims)
        bad("mla_seqmean_fwd", P, P, *dims)
    for dims in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        bad("mla_chamfer_bwd", P, P, P, P, P, P, P, P, *dims)
    bad("mla_chamfer_bwd", P, P, P, None, P, P, P, P, 1, 4, 4)
    for N, M in ((G.CHAMFER_MAX + 1, 4), (4, G.CHAMFER_MAX + 1)):
        bad("mla_chamfer_fwd", P, P, P, P, P, P, P, 1, N, M, P, 64, msg=b"4096")
    for dims in ((0, 4, 8), (3, 0, 8), (3, 4, 0)):
        bad("mla_maxpool_k_bwd", P, P, P, *dims)
    for dims in ((0, 4, 4, 8, 2), (1, 0, 4, 8, 2), (1, 4, 4, 0, 2), (1, 4, 4, 8, 0), (1, 4, 4, 8, 3)):
        bad("mla_avgpool_tokens_bwd", P, None, P, *dims)
    bad("mla_layernorm_bwd", P, P, P, P, P, P, None, None, 0, 4, 12, P, 1 << 20)
    bad("mla_layernorm_bwd", P, P, P, P, P, P, None, None, 0, 4, 136, P, 16, msg=b"workspace")
    bad("mla_lga_prep_bwd", P, P, P, P, 1, 8, 4, 129, 8, msg=b"K <= 128")
