"""Kernel-level parity of the point and vision tokenizer forward kernels -- mla_fps, mla_knn, mla_gather_rows_f32, mla_lga_prep,
mla_colstats_bf16, mla_bn_apply, mla_maxpool_k, mla_im2col_patch, mla_avgpool_tokens, mla_local_attn (+ _bwd) -- and of mla_ce_bwd,
mla_gather_rows_bf16 and mla_add_bf16, each called through its mla_amd.hip wrapper against the high-precision references of
tests/tokenizer_cases.py, at the shapes the model never uses: both kernels of every two-way dispatch, ragged sizes, ties, duplicate
points, capped grids. The free pool is NaN-filled before every group (the wrappers return torch.empty buffers: an element a kernel
skips must not inherit a correct value an earlier launch left behind).

Which case takes which kernel (dispatch conditions in pointcloud.hip / vision.hip):
  lga_prep_kernel (scalar)        test_lga_prep[*-12-5], [*-27-7] (fd = 2C / 6 in {4, 9}: not a multiple of 8) and the second launch of
                                  [*-96-81] (feats 8 bytes into a larger buffer: not 16-byte aligned)
  lga_prep_vec_kernel             test_lga_prep[*-96-81], [*-192-81], [*-24-9], [*-384-128]
  colstats_partial_kernel         test_bn_zero_mean[*-2056] (C / 8 = 257 > 256), test_colstats_strided[*-20] (C % 8 != 0) and the
                                  `ld % 8 != 0` slice of every test_colstats_strided case
  colstats_partial_vec_kernel     test_bn_zero_mean[*-8 / 96 / 192 / 2048], the `ld % 8 == 0` slice of test_colstats_strided
  bn_apply_flat_kernel            test_bn_zero_mean[*-2056] and the misaligned-residual launch of every test_bn_zero_mean case
  bn_apply_kernel                 every other bn_apply launch; [172037-96] caps the grid at 4096 (two strides in flight + 5 tail rows),
                                  C = 96 / 192 have a block of 252 / 240 lanes (RL * C / 8 != 256)
  maxpool_k_kernel (scalar)       test_maxpool_k[*-27];  maxpool_k_vec_kernel: C = 8, 192
  im2col_kernel<bf16_t> / <float> test_im2col[bf16-*] / [fp32-*]

Bounds (none is taken from a kernel):
  exact                 integer outputs, copies, max-pool, im2col, the cs = 1 pool, lc_xyz.
  one bf16 rounding     |err| <= 2^-8 |ref| + 4 x slack, slack = max |fp32 reference - fp64 reference| over all inputs of the family
                        (tokenizer_cases.measured_slack, recomputed here). Measured on the host:
                            lga_prep   9.670e-06     batch norm   1.010e-06
                        The scalar and the 8-wide lga_prep kernels agree bit for bit on all three clouds at C = 96 (max |diff| 0).
                        With fp32 running sums in colstats, test_bn_zero_mean[2047-2048] (one block, one row lane: 2047 adds in a
                        row) left 3 elements 1.0e-06 outside this bound (|err| 5.0e-06 where b + res cancels the output); the
                        running sums are fp64 since, and nothing is outside.
                        avg-pool: the absolute term is 2^-20 max |x| (at most 16 fp32 roundings of partial sums <= 16 max |x|, / cs^2).
  project bounds        fro_rel < 4e-3 for bf16 outputs, 5e-3 / 1e-2 for local_attn forward / backward, 2e-2 max_rel per window,
                        1e-5 for the fp32 statistics (per column: |mean - m64| <= 1e-5 sqrt(E x^2), |var - v64| <= 1e-5 E x^2 -- the
                        bound on each accumulated moment, which on zero-mean data is the relative bound on the variance).
  offset columns        mean / std 8 and 64: the kernel pair colstats + bn_apply may be at most 2 x as far from fp64 as torch's own
                        fp32 batch norm on the CPU rounded to bf16 (max |err| and Frobenius, constant column left out).
                        Measured on an MI355X (every case is printed by test_bn_offset_columns): the kernel pair is 1.00 .. 1.04 x
                        the yardstick in max |err| and 1.00 x in Frobenius error; e.g. rows = 6145, C = 96: max |err| 1.560e-02
                        | 1.560e-02, fro 1.671e-03 | 1.671e-03 (yardstick | kernels); worst ratio rows = 2047, C = 2056:
                        1.562e-02 | 1.624e-02. Both are the one bf16 rounding of the output; the one-pass variance does not show.
  kNN                   the band of tokenizer_cases.knn_violations (factor 8 in delta); lattice16: the exact sequence.
  ce_bwd                fp32 autograd; |err| <= 2^-8 |ref| + 2e-5 g (g = gscale * inv_count: the softmax probability is <= 1 and the
                        fp32 subtraction logit - lse at |values| <= 40 plus the fast exponential resolve it to ~1e-5), fro_rel < 4e-3.
"""
import pytest
import torch

import tokenizer_cases as TC
from conftest import poison_free_memory

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _hip():
    from mla_amd import hip
    return hip


def _ulp_close(a, b):
    """bf16 tensors within one bf16 ulp of each other, elementwise (an ulp is at most 2^-7 of the value)."""
    a, b = a.float(), b.float()
    return bool(((a - b).abs() <= 2.0 ** -7 * torch.maximum(a.abs(), b.abs())).all())


# ------------------------------------------------------------------------------------------------ FPS
@pytest.mark.parametrize("N", TC.FPS_N)
@pytest.mark.parametrize("cloud", TC.CLOUDS)
def test_fps(dev, cloud, N):
    hip = _hip()
    for kind in TC.FPS_STARTS:
        xyz, start, ref = TC.fps_case(cloud, N, kind)
        poison_free_memory()
        xd, sd = xyz.to(dev), start.to(dev)
        for B in TC.FPS_B:
            for npoint in TC.fps_npoints(N):
                out = hip.fps(xd[:B].contiguous(), sd[:B].contiguous(), npoint).cpu()
                assert torch.equal(out, ref[:B, :npoint]), (cloud, N, kind, B, npoint, int((out != ref[:B, :npoint]).sum()))
    if cloud == "lattice16" and N >= 1000:          # duplicates: the tail is the lowest index repeated, as in the reference
        distinct = len({tuple(p.tolist()) for p in xyz[0]})
        assert distinct < N and bool((out[0, distinct:] == 0).all())


def test_fps_rejects_2049_points(dev):
    hip = _hip()
    xyz = TC.make_cloud("uniform", 1, 2049).to(dev)
    with pytest.raises(RuntimeError, match="mla_fps"):
        hip.fps(xyz, torch.zeros(1, dtype=torch.long, device=dev), 16)


# ------------------------------------------------------------------------------------------------ kNN, fp32 gather
@pytest.mark.parametrize("N", TC.KNN_N)
@pytest.mark.parametrize("cloud", TC.CLOUDS)
def test_knn_and_gather(dev, cloud, N):
    hip = _hip()
    xyz = TC.make_cloud(cloud, TC.KNN_B, N)
    xd = xyz.to(dev)
    for G in TC.KNN_G:
        centres, cidx = TC.knn_centres(xyz, G)
        poison_free_memory()
        cd = hip.gather_rows_f32(xd, cidx.to(dev))
        assert torch.equal(cd.cpu(), centres), (cloud, N, G, "gather_rows_f32 is xyz[b, idx]")
        for k in TC.knn_ks(N):
            runs = [hip.knn(xd, cd, k).cpu() for _ in range(3)]
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), (cloud, N, G, k, "repeated launches differ")
            idx = runs[0]
            assert idx.dtype == torch.int32 and idx.shape == (TC.KNN_B, G, k)
            v = TC.knn_violations(idx, xyz, centres)
            assert not any(v.values()), (cloud, N, G, k, v)
            if cloud == "lattice16":
                ref = TC.knn_exact(xyz, centres, k)
                assert torch.equal(idx.long(), ref), (cloud, N, G, k, int((idx.long() != ref).sum()), "(distance, index) ascending")
            if k == N:
                assert torch.equal(idx.long().sort(-1).values, torch.arange(N).expand(TC.KNN_B, G, N)), "k == N: a permutation"


# ------------------------------------------------------------------------------------------------ lga_prep
@pytest.mark.parametrize("C,K", TC.LGA_CK)
@pytest.mark.parametrize("cloud", TC.LGA_CLOUDS)
def test_lga_prep(dev, cloud, C, K, capsys):
    hip = _hip()
    xyz, feats, fps_idx, knn_idx = TC.lga_case(cloud, C, K)
    ref, lc_ref = TC.lga_prep_ref(xyz, feats, fps_idx, knn_idx)
    slack = TC.measured_slack("lga")
    xd, fd_, kd = xyz.to(dev), fps_idx.to(dev), knn_idx.to(dev)
    fb = feats.to(BF).to(dev)
    assert fb.data_ptr() % 16 == 0
    launches = [("aligned", fb)]
    if C == 96:                                      # the same features 8 bytes into a larger buffer: the scalar kernel
        big = torch.empty(fb.numel() + 16, dtype=BF, device=dev)
        view = big[4:4 + fb.numel()].view(fb.shape)
        view.copy_(fb)
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        launches.append(("misaligned", view))
    outs = {}
    for name, f in launches:
        poison_free_memory()
        rows, lc = hip.lga_prep(xd, f, fd_, kd, TC.ALPHA, TC.BETA)
        rows, lc = rows.cpu(), lc.cpu()
        outs[name] = rows
        assert torch.equal(lc, lc_ref.float()), (cloud, C, K, name, "lc_xyz is a copy")
        n, over, err = TC.one_rounding_violations(rows, ref, slack)
        with capsys.disabled():
            print(f"\nLGA {cloud:<9} C {C:>3} K {K:>3} {name:<10} max |err| {err:.3e}  fro {TC.fro(rows, ref):.3e}  outside 2^-8|ref| + 4 x {slack:.2e}: {n}")
        assert n == 0, (cloud, C, K, name, n, over)
        assert TC.fro(rows, ref) < 4e-3
        if cloud == "planar":
            sl, exp = TC.planar_expected(xyz, feats, fps_idx, knn_idx)
            assert torch.equal(rows[:, sl], exp), (C, K, name, "clamped coordinate: sin = 0, cos = 1, one rounding")
    if "misaligned" in outs:
        a, b = outs["aligned"], outs["misaligned"]
        with capsys.disabled():
            print(f"LGA {cloud:<9} C {C} scalar vs vector kernel: max |diff| {float((a.float() - b.float()).abs().max()):.3e}  bit-equal: {torch.equal(a, b)}")
        assert _ulp_close(a, b), "scalar and vector kernels more than one bf16 ulp apart"


# ------------------------------------------------------------------------------------------------ batch norm
def _check_stats(mean, var, x, tag):
    m64, v64 = TC.bn_stats64(x)
    ex2 = v64 + m64 * m64
    mean, var = mean.cpu().double(), var.cpu().double()
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all()), tag
    assert bool((var >= 0).all()), (tag, "var >= 0")
    dm, dv = (mean - m64).abs() - 1e-5 * ex2.sqrt(), (var - v64).abs() - 1e-5 * ex2
    assert bool((dm <= 0).all()), (tag, "mean", int(dm.argmax()), float(dm.max()))
    assert bool((dv <= 0).all()), (tag, "var", int(dv.argmax()), float(dv.max()))
    return m64, v64


@pytest.mark.parametrize("rows,C", TC.bn_shapes())
def test_bn_zero_mean(dev, rows, C, capsys):
    hip = _hip()
    x, w, b, res = TC.bn_inputs(rows, C)
    slack = TC.measured_slack("bn")
    xd, wd, bd = x.to(BF).to(dev), w.to(BF).to(dev), b.to(BF).to(dev)
    rd = res.to(BF).to(dev)
    big = torch.empty(rd.numel() + 16, dtype=BF, device=dev)
    rmis = big[4:4 + rd.numel()].view(rd.shape)
    rmis.copy_(rd)
    assert rmis.data_ptr() % 16 == 8
    poison_free_memory()
    mean, var = hip.colstats(xd)
    m64, v64 = _check_stats(mean, var, x, (rows, C))
    if rows >= 20:
        assert TC.fro(mean.cpu(), m64) < 1e-5 and TC.fro(var.cpu(), v64) < 1e-5
    for rname, r, rref in (("none", None, None), ("res", rd, res), ("res-misaligned", rmis, res)):
        for relu in (False, True):
            poison_free_memory()
            y = hip.bn_apply(xd, mean, var, wd, bd, TC.BN_EPS, residual=r, relu=relu).cpu()
            ref = TC.bn_ref(x, w, b, res=rref, relu=relu)
            assert bool(torch.isfinite(y.float()).all()), (rows, C, rname, relu, "finite, the constant column included")
            n, over, err = TC.one_rounding_violations(y[:, :C - 1], ref[:, :C - 1], slack)
            f = TC.fro(y[:, :C - 1], ref[:, :C - 1])
            with capsys.disabled():
                print(f"\nBN rows {rows:>6} C {C:>4} res {rname:<14} relu {int(relu)}: max |err| {err:.3e} fro {f:.3e} outside: {n}")
            assert n == 0, (rows, C, rname, relu, n, over)
            assert f < 4e-3
            if relu:
                assert bool((y.float() >= 0).all())


@pytest.mark.parametrize("C", TC.BN_C + TC.BN_STATS_ONLY_C)
@pytest.mark.parametrize("rows", (20, 2047, 6145))
def test_colstats_strided(dev, rows, C):
    """Column slices of a wider buffer (ld > C): ld % 8 == 0 with a 16-byte aligned start keeps the 8-wide kernel (C % 8 == 0,
    C <= 2048), ld % 8 != 0 takes the scalar one. The columns outside the slice hold 1e4."""
    hip = _hip()
    x = TC.bn_inputs(rows, C)[0] if C % 8 == 0 else TC._bf(torch.randn(rows, C, generator=TC._gen("cs", rows, C)) * 1.5 + 0.3)
    xb = x.to(BF).to(dev)
    poison_free_memory()
    mean, var = hip.colstats(xb)
    _check_stats(mean, var, x, (rows, C, "contiguous"))
    for W, off in ((C + 16, 8), (C + 5, 3)):
        wide = torch.full((rows, W), 1e4, dtype=BF, device=dev)
        wide[:, off:off + C] = xb
        sl = wide[:, off:off + C]
        assert sl.stride(0) == W and not sl.is_contiguous()
        poison_free_memory()
        mean, var = hip.colstats(sl)
        _check_stats(mean, var, x, (rows, C, "ld", W))


@pytest.mark.parametrize("rows,C", [(r, c) for c in TC.BN_C for r in (2047, 6145)] + [(TC.BN_BIG_ROWS, 96)])
def test_bn_offset_columns(dev, rows, C, capsys):
    hip = _hip()
    x, w, b, res = TC.bn_inputs(rows, C, "offset")
    xd, wd, bd, rd = (t.to(BF).to(dev) for t in (x, w, b, res))
    poison_free_memory()
    mean, var = hip.colstats(xd)
    _check_stats(mean, var, x, (rows, C, "offset"))
    for r, rref, relu in ((None, None, False), (rd, res, True)):
        poison_free_memory()
        y = hip.bn_apply(xd, mean, var, wd, bd, TC.BN_EPS, residual=r, relu=relu).cpu().double()
        ref = TC.bn_ref(x, w, b, res=rref, relu=relu)
        yard = TC.bn_torch32(x, w, b, res=rref, relu=relu).double()
        assert bool(torch.isfinite(y).all())
        s = slice(0, C - 1)
        ek, ey = float((y - ref)[:, s].abs().max()), float((yard - ref)[:, s].abs().max())
        fk, fy = TC.fro(y[:, s], ref[:, s]), TC.fro(yard[:, s], ref[:, s])
        with capsys.disabled():
            print(f"\nBN-OFFSET rows {rows:>6} C {C:>4} res/relu {int(relu)}: max |err| kernel {ek:.3e} yardstick {ey:.3e} ({ek / ey:.2f} x)   "
                  f"fro kernel {fk:.3e} yardstick {fy:.3e} ({fk / fy:.2f} x)")
        assert ek <= 2 * ey and fk <= 2 * fy, (rows, C, relu, ek, ey, fk, fy)


# ------------------------------------------------------------------------------------------------ max-pool over neighbours
@pytest.mark.parametrize("C", TC.POOL_C)
@pytest.mark.parametrize("K", TC.POOL_K)
def test_maxpool_k(dev, K, C):
    hip = _hip()
    x = TC.pool_inputs(K, C)
    out = hip.maxpool_k(x.to(dev), TC.POOL_GROUPS, K).cpu()
    ref = x.float().view(TC.POOL_GROUPS, K, C).amax(1)
    assert torch.equal(out.float(), ref), (K, C, int((out.float() != ref).sum()))
    assert bool((out[:, ::3].float() < 0).all())


# ------------------------------------------------------------------------------------------------ vision
@pytest.mark.parametrize("dt,B,CT,H,W,P", TC.IM2COL_CASES + TC.IM2COL_BIG)
def test_im2col(dev, dt, B, CT, H, W, P):
    hip = _hip()
    pix = torch.randn(B, CT, H, W, generator=TC._gen("pix", dt, B, CT, H, W))
    pix[:, 3:] = 7.0                                                           # the mask channel must never be read
    if dt == "bf16":
        pix = pix.to(BF)
    pd = pix.to(dev)
    for Kpad in TC.im2col_kpads(P):
        poison_free_memory()
        rows = hip.im2col_patch(pd, P, Kpad).cpu()
        ref = TC.im2col_ref(pix, P, Kpad)
        assert rows.shape == ref.shape and torch.equal(rows, ref), (dt, B, CT, H, W, P, Kpad, int((rows != ref).sum()))
        assert bool((rows[:, 3 * P * P:] == 0).all())


@pytest.mark.parametrize("C", (256, 1024))
@pytest.mark.parametrize("grid", ((6, 12), (12, 24), (48, 48), (4, 8)))
@pytest.mark.parametrize("cs", (1, 2, 3, 4))
def test_avgpool_tokens(dev, cs, grid, C):
    hip = _hip()
    B = 2
    gh, gw = TC.grid_for(grid, cs)
    x = torch.randn(B * gh * gw, C, generator=TC._gen("avg", cs, grid, C)).to(BF)
    y = hip.avgpool_tokens(x.to(dev), B, gh, gw, cs).cpu()
    if cs == 1:
        assert torch.equal(y, x), "cs = 1 is the identity, bit for bit"
        return
    ref = TC.avgpool_ref(x, B, gh, gw, cs)
    assert y.shape == ref.shape
    n, over, err = TC.one_rounding_violations(y, ref, 2.0 ** -22 * float(x.float().abs().max()))     # 4 x slack = 2^-20 max |x|
    assert n == 0, (cs, grid, C, n, over, err)
    assert TC.fro(y, ref) < 4e-3


def _attn_cases():
    out = []
    for C in TC.ATTN_C:
        for cs in TC.ATTN_CS:
            for grid in TC.ATTN_GRIDS:
                for B in TC.ATTN_B:
                    if grid == (48, 48) and B == 3 and C != 1024:       # 56 MB of k/v at C = 2048; B = 3 at the model's width only
                        continue
                    out.append((C, cs, grid, B))
    return out


@pytest.mark.parametrize("C,cs,grid,B", _attn_cases())
def test_local_attn_forward_backward(dev, C, cs, grid, B, capsys):
    hip = _hip()
    gh, gw = TC.grid_for(grid, cs)
    q, kv, do = TC.attn_inputs(B, gh, gw, C, cs)
    qd, kvd, dod = q.to(dev), kv.to(dev), do.to(dev)
    for scale in TC.attn_scales(C):
        ro, rdq, rdkv = TC.local_attn_ref(q, kv, do, B, gh, gw, cs, scale)
        poison_free_memory()
        out = hip.local_attn(qd, kvd, B, gh, gw, cs, TC.HEADS, scale).cpu()
        dq, dkv = hip.local_attn_bwd(qd, kvd, dod, B, gh, gw, cs, TC.HEADS, scale)
        dq, dkv = dq.cpu(), dkv.cpu()
        for t in (out, dq, dkv):
            assert bool(torch.isfinite(t.float()).all())
        wr = lambda t, lo: TC.window_rows(t.double()[:, lo:lo + C].contiguous(), B, gh, gw, cs)
        table = [("out", out, ro, 5e-3), ("dq", dq, rdq, 1e-2), ("dk", wr(dkv, 0), wr(rdkv, 0), 1e-2), ("dv", wr(dkv, C), wr(rdkv, C), 1e-2)]
        for name, a, r, bound in table:
            f = TC.fro(a, r) if float(r.double().norm()) > 0 else float(a.double().norm())
            pw, at = TC.per_window_max_rel(a, r)
            with capsys.disabled():
                print(f"\nATTN C {C:>4} cs {cs} grid {gh}x{gw} B {B} scale x{scale * C ** 0.5:.0f} {name:<3}: fro {f:.3e} (< {bound})  worst window {pw:.3e} at {at} (< 2e-2)")
            assert f < bound, (C, cs, grid, B, scale, name, f)
            assert pw < 2e-2, (C, cs, grid, B, scale, name, pw, at)


# ------------------------------------------------------------------------------------------------ ce_bwd, gather_rows, add_bf16
@pytest.mark.parametrize("dt,ncols,ld", TC.CE_CASES)
def test_ce_bwd(dev, dt, ncols, ld):
    hip = _hip()
    logits, labels = TC.ce_inputs(dt, ncols, ld)
    inv_count, gscale = 1.0 / 6.0, 1.5
    ref = TC.ce_bwd_ref(logits, labels, ncols, inv_count, gscale)
    lse = torch.logsumexp(logits[:, :ncols].float(), -1)
    ld_ = (logits.to(BF) if dt == "bf16" else logits).to(dev)
    poison_free_memory()
    d = hip.ce_bwd(ld_, labels.to(dev), lse.to(dev), torch.tensor([gscale], device=dev), inv_count, ncols=ncols).cpu().float()
    assert d.shape == (TC.CE_ROWS, ld)
    assert bool((d[:, ncols:] == 0).all()), "padded columns stay zero"
    assert bool((d[labels == -100] == 0).all()), "ignored rows are exactly zero"
    got = d[:, :ncols].double()
    err = (got - ref.double()).abs()
    assert bool((err <= 2.0 ** -8 * ref.double().abs() + 2e-5 * gscale * inv_count).all()), float(err.max())
    assert TC.fro(got, ref) < 4e-3
    keep = labels != -100
    assert bool((got[keep, labels[keep]] < 0).all())


@pytest.mark.parametrize("H", (136, 4096))
def test_gather_rows_bf16(dev, H):
    hip = _hip()
    g = TC._gen("gather", H)
    src = torch.randn(50, H, generator=g).to(BF)
    idx = torch.randint(0, 50, (77,), generator=g)
    sd = src.to(dev)
    poison_free_memory()
    assert torch.equal(hip.gather_rows(sd, idx.to(dev)).cpu(), src[idx])
    out = hip.gather_rows(sd, idx.to(dev), out_rows=100).cpu()
    assert torch.equal(out[:77], src[idx]) and bool((out[77:] == 0).all())
    to = torch.randperm(131, generator=g)[:50]                                  # scatter: out[to[r]] = src[r], 131 rows > the source's 50
    poison_free_memory()
    out = hip.gather_rows(sd, to.to(dev), out_rows=131, scatter=True).cpu()
    ref = torch.zeros(131, H, dtype=BF)
    ref[to] = src
    assert torch.equal(out, ref), "unaddressed rows are zero"


def test_add_bf16_ragged(dev):
    hip = _hip()
    g = TC._gen("add")
    a, b = (torch.randn(1003, generator=g) * 3).to(BF), torch.randn(1003, generator=g).to(BF)
    poison_free_memory()
    y = hip.add_bf16(a.to(dev), b.to(dev)).cpu()
    assert torch.equal(y, (a.float() + b.float()).to(BF))
