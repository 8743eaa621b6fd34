"""Host-only helpers of tests/test_tokenizer_kernels_gpu.py: input builders, case lists and high-precision references of the point and
vision tokenizer forward kernels (FPS, kNN, lga_prep, train-mode batch norm, max-pool over neighbours, im2col, token average pool,
window attention) and of three small kernels nothing else calls directly (ce_bwd, gather_rows, add_bf16). Nothing here touches the
GPU; tests/test_tokenizer_cases_host.py checks it.

Clouds ([B, N, 3] fp32):
  uniform     [-1, 1]^3                                  baseline
  lattice16   coordinates k / 16, k in 0..15             many exact ties and duplicate points; every product and sum of the FPS and
                                                         kNN formulas is exact in fp32, so the expected indices are unique
  offset      N(0, 0.05^2) around (3, -2, 5)             the -2 <c, p> + |c|^2 + |p|^2 expansion of the kNN distance cancels
  planar      uniform x, y; z constant                   the max-abs offset of z is 0 and takes the 1e-6 clamp in lga_prep

References:
  fps_ref       fp32 numpy loop in the kernel's stated order (dx*dx + dy*dy) + dz*dz, np.minimum, np.argmax (first maximum = the lower
                index on ties). Equals oracle.torch_oracle.furthest_point_sample index for index.
  kNN           no index list is THE answer in fp32: a result is valid when the indices are in range and distinct within a group, every
                chosen point has d64 <= dk + 2 delta and every unchosen point d64 >= dk - 2 delta, with d64 the fp64 distance, dk the
                k-th smallest and delta = 8 * 2^-24 * (|c| + |p|)^2 per pair (knn_violations). On lattice16 the arithmetic is exact and
                the kernel documents a (distance, index) ascending sort: the expected output is the exact sequence
                np.argsort(d64, kind="stable")[:k] (knn_exact).
  lga_prep_ref  cat(feats[knn], feats[centre]) + oracle.torch_oracle.pos_embed_geo of the centre-subtracted, per-(group, coordinate)
                max-abs normalised offsets (clamp 1e-6), in fp64 (or fp32: the slack measurement).
  bn_ref        train statistics (biased variance) and y = (x - m) / sqrt(v + eps) * w + b (+ res) (relu), fp64 or fp32.
  im2col_ref (unfold), avgpool_ref (F.avg_pool2d, fp64), local_attn_ref (fp64 window attention and its autograd).

Slack: a bf16 output is held to |err| <= 2^-8 |ref| + 4 x slack, where slack = max |fp32 reference - fp64 reference| over ALL the
inputs of the family the GPU test uses (measured_slack). It covers what an fp32 evaluation cannot resolve -- the sin / cos argument
error at beta = 100, the batch-norm arithmetic -- and is measured, never taken from a kernel."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_oracle as TO

BF = torch.bfloat16
CLOUDS = ("uniform", "lattice16", "offset", "planar")
PLANAR_Z = 0.375
ALPHA, BETA = 1000.0, 100.0
BN_EPS = 1e-5


def _bf(x):
    return x.to(BF).float()


def _gen(*key):
    h = 0
    for k in key:
        for ch in str(k):
            h = (h * 131 + ord(ch)) % 2147483647
    return torch.Generator().manual_seed(h)


# ------------------------------------------------------------------------------------------------ clouds
def make_cloud(name, B, N, seed=0):
    g = _gen("cloud", name, N, seed)
    if name == "uniform":
        x = torch.rand(B, N, 3, generator=g) * 2 - 1
    elif name == "lattice16":
        x = torch.randint(0, 16, (B, N, 3), generator=g).float() / 16
    elif name == "offset":
        x = torch.randn(B, N, 3, generator=g) * 0.05 + torch.tensor([3.0, -2.0, 5.0])
    elif name == "planar":
        x = torch.rand(B, N, 3, generator=g) * 2 - 1
        x[..., 2] = PLANAR_Z
    else:
        raise ValueError(name)
    return x.float().contiguous()


# ------------------------------------------------------------------------------------------------ FPS
FPS_N = (1, 2, 255, 256, 257, 1000, 1024, 2047, 2048)
FPS_B = (1, 3, 33)
FPS_STARTS = ("zero", "last", "random")


def fps_npoints(N):
    return sorted({1, max(1, N // 2), N})


def fps_start(kind, B, N, seed=0):
    if kind == "zero":
        return torch.zeros(B, dtype=torch.long)
    if kind == "last":
        return torch.full((B,), N - 1, dtype=torch.long)
    return torch.randint(0, N, (B,), generator=_gen("start", N, seed))


def fps_ref(xyz, npoint, start):
    """[B, npoint] int64. A selection of npoint points is a prefix of the selection of any larger number."""
    x = xyz.numpy().astype(np.float32)
    B, N, _ = x.shape
    X, Y, Z = (np.ascontiguousarray(x[..., c]) for c in range(3))
    ar = np.arange(B)
    far = start.numpy().astype(np.int64).copy()
    dist = np.full((B, N), 1e10, dtype=np.float32)
    out = np.zeros((B, npoint), dtype=np.int64)
    for i in range(npoint):
        out[:, i] = far
        dx, dy, dz = X - X[ar, far][:, None], Y - Y[ar, far][:, None], Z - Z[ar, far][:, None]
        dd = (dx * dx + dy * dy) + dz * dz
        assert dd.dtype == np.float32
        np.minimum(dist, dd, out=dist)
        far = np.argmax(dist, axis=-1)
    return torch.from_numpy(out)


@functools.lru_cache(maxsize=None)
def fps_case(cloud, N, start_kind):
    """The cloud at the largest batch, its start indices and the full selection (npoint = N); smaller B / npoint are slices."""
    B = max(FPS_B)
    xyz = make_cloud(cloud, B, N)
    start = fps_start(start_kind, B, N)
    return xyz, start, fps_ref(xyz, N, start)


# ------------------------------------------------------------------------------------------------ kNN
KNN_N = (1, 77, 512, 1000, 1024)
KNN_G = (1, 100, 512)
KNN_B = 2


def knn_ks(N):
    return sorted({k for k in (1, 33, 81, N) if k <= N})


def knn_centres(xyz, G, seed=0):
    """Centres are points of the cloud (as in the model, and so that lattice16 stays exact); with replacement when G > N."""
    B, N, _ = xyz.shape
    g = _gen("centres", N, G, seed)
    idx = torch.stack([torch.randperm(N, generator=g)[:G] if G <= N else torch.randint(0, N, (G,), generator=g) for _ in range(B)])
    return TO.index_points(xyz, idx).contiguous(), idx


def knn_d64(xyz, centres):
    d = centres.double()[:, :, None, :] - xyz.double()[:, None, :, :]
    return (d * d).sum(-1)                                                    # [B, G, N]


def knn_delta(xyz, centres):
    return 8 * 2.0 ** -24 * (centres.double().norm(dim=-1)[:, :, None] + xyz.double().norm(dim=-1)[:, None, :]) ** 2


def knn_violations(idx, xyz, centres):
    """idx [B, G, k] (any integer dtype). Returns dict(range, distinct, chosen_far, unchosen_near): the number of violations of each
    condition of the band."""
    B, N, _ = xyz.shape
    idx = idx.long()
    k = idx.shape[-1]
    bad_range = int(((idx < 0) | (idx >= N)).sum())
    safe = idx.clamp(0, N - 1)
    chosen = torch.zeros(B, idx.shape[1], N, dtype=torch.long).scatter_add_(-1, safe, torch.ones_like(safe))
    d64, delta = knn_d64(xyz, centres), knn_delta(xyz, centres)
    dk = d64.sort(-1).values[..., k - 1:k]
    on = chosen > 0
    return {"range": bad_range, "distinct": int((chosen > 1).sum()) + int((on.sum(-1) != k).sum()),
            "chosen_far": int((on & (d64 > dk + 2 * delta)).sum()), "unchosen_near": int((~on & (d64 < dk - 2 * delta)).sum())}


def knn_exact(xyz, centres, k):
    """The exact (distance, index) ascending sequence; meaningful where fp32 distances are exact (lattice16)."""
    return torch.from_numpy(np.argsort(knn_d64(xyz, centres).numpy(), axis=-1, kind="stable")[..., :k].copy())


def knn_match_share(idx, xyz, centres):
    """Share of the groups whose index SET equals the fp64 top-k set (stable order)."""
    k = idx.shape[-1]
    ref = knn_exact(xyz, centres, k).sort(-1).values
    return float((idx.long().sort(-1).values == ref).all(-1).float().mean())


# ------------------------------------------------------------------------------------------------ lga_prep
LGA_CK = ((96, 81), (192, 81), (24, 9), (12, 5), (27, 7), (384, 128))
LGA_SCALAR_CK = ((12, 5), (27, 7))                   # fd = 2C / 6 not a multiple of 8: the scalar kernel
LGA_CLOUDS = ("uniform", "planar", "lattice16")
LGA_B, LGA_N, LGA_G = 2, 256, 24


@functools.lru_cache(maxsize=None)
def lga_case(cloud, C, K):
    """xyz [B, N, 3], feats [B, N, C] (bf16-exact fp32), fps_idx [B, G] int64 (distinct), knn_idx [B, G, K] int32 (the exact fp64
    neighbours of the centres)."""
    xyz = make_cloud(cloud, LGA_B, LGA_N, seed=7)
    g = _gen("lga", cloud, C, K)
    feats = _bf(torch.randn(LGA_B, LGA_N, C, generator=g))
    fps_idx = torch.stack([torch.randperm(LGA_N, generator=g)[:LGA_G] for _ in range(LGA_B)])
    centres = TO.index_points(xyz, fps_idx)
    return xyz, feats, fps_idx, knn_exact(xyz, centres, K).int()


def lga_prep_ref(xyz, feats, fps_idx, knn_idx, dtype=torch.float64, alpha=ALPHA, beta=BETA):
    """rows [B * G * K, 2C], lc_xyz [B, G, 3] in `dtype` (Point_PN.py:125-134 LGA 'scan' normalisation + PosE_Geo)."""
    x, f = xyz.to(dtype), feats.to(dtype)
    knn_idx = knn_idx.long()
    B, G, K = knn_idx.shape
    lc_xyz, lc_x = TO.index_points(x, fps_idx), TO.index_points(f, fps_idx)
    knn_xyz, knn_x = TO.index_points(x, knn_idx), TO.index_points(f, knn_idx)
    kx = knn_xyz.permute(0, 3, 1, 2) - lc_xyz.permute(0, 2, 1).unsqueeze(-1)              # [B, 3, G, K]
    mx = kx.abs().max(dim=-1, keepdim=True)[0].clamp(min=1e-6)
    kx = kx / mx
    kf = torch.cat([knn_x, lc_x[:, :, None, :].expand(-1, -1, K, -1)], dim=-1)          # [B, G, K, 2C]
    pe = TO.pos_embed_geo(kx, 2 * f.shape[-1], alpha, beta).permute(0, 2, 3, 1)
    return (kf + pe).reshape(B * G * K, -1), lc_xyz


def planar_expected(xyz, feats, fps_idx, knn_idx):
    """The channels of the clamped coordinate (z: channels [4 fd, 6 fd)) of a planar cloud: feature + sin 0 = feature in the sin half,
    feature + cos 0 = feature + 1 in the cos half, rounded once to bf16. Returns (channel slice, expected bf16 [B * G * K, 2 fd])."""
    B, G, K = knn_idx.shape
    C = feats.shape[-1]
    fd = 2 * C // 6
    kf = torch.cat([TO.index_points(feats, knn_idx.long()), TO.index_points(feats, fps_idx)[:, :, None, :].expand(-1, -1, K, -1)], -1)
    z = kf[..., 4 * fd:].clone()
    z[..., fd:] += 1.0
    return slice(4 * fd, 6 * fd), z.reshape(B * G * K, 2 * fd).to(BF)


# ------------------------------------------------------------------------------------------------ batch norm
BN_C = (8, 96, 192, 2048, 2056)                      # C = 20: colstats only (BN_STATS_ONLY_C), bn_apply needs C % 8 == 0
BN_STATS_ONLY_C = (20,)
BN_ROWS = (1, 20, 2047, 6145)
BN_BIG_ROWS = 4096 * 21 * 2 + 5                      # C = 96: 21 row lanes, grid capped at 4096 -> two full strides + 5 tail rows
BN_BIG_C = (8, 96)                                   # 33 MB at C = 96; the wider channel counts would be 66 MB and more
BN_OFFSETS = (8.0, 64.0)


def bn_shapes():
    return [(r, c) for c in BN_C for r in BN_ROWS] + [(BN_BIG_ROWS, c) for c in BN_BIG_C]


@functools.lru_cache(maxsize=4)
def bn_inputs(rows, C, family="zero_mean"):
    """x [rows, C], w, b [C], res [rows, C]: fp32 tensors with bf16-exact values. family zero_mean: column std in [0.5, 2], column mean
    0.25 N(0, 1) std; family offset: column mean / std alternates 8 and 64. Column C - 1 is constant in both."""
    g = _gen("bn", rows, C, family)
    std = torch.rand(C, generator=g) * 1.5 + 0.5
    if family == "zero_mean":
        mean = torch.randn(C, generator=g) * 0.25 * std
    else:
        mean = torch.tensor([BN_OFFSETS[c % 2] for c in range(C)]) * std * torch.where(torch.arange(C) % 4 < 2, 1.0, -1.0)
    x = torch.randn(rows, C, generator=g) * std + mean
    x[:, C - 1] = 3.0 if family == "zero_mean" else 64.0
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g) * 0.5
    res = torch.randn(rows, C, generator=g)
    return _bf(x), _bf(w), _bf(b), _bf(res)


def bn_stats64(x):
    x = x.double()
    return x.mean(0), x.var(0, unbiased=False)


def bn_ref(x, w, b, eps=BN_EPS, res=None, relu=False, dtype=torch.float64):
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    m, v = x.mean(0), x.var(0, unbiased=False)
    y = (x - m) / torch.sqrt(v + eps) * w + b
    if res is not None:
        y = y + res.to(dtype)
    return F.relu(y) if relu else y


def bn_torch32(x, w, b, eps=BN_EPS, res=None, relu=False):
    """The yardstick of the offset columns: torch's own fp32 train-mode batch norm on the CPU, output rounded to bf16."""
    y = F.batch_norm(x.float(), None, None, w.float(), b.float(), True, 0.0, eps)
    if res is not None:
        y = y + res.float()
    return (F.relu(y) if relu else y).to(BF)


# ------------------------------------------------------------------------------------------------ max-pool over neighbours
POOL_K = (1, 3, 4, 81, 128)
POOL_C = (8, 192, 27)
POOL_GROUPS = 37


def pool_inputs(K, C):
    """[groups * K, C] bf16; every third column all negative, column 1 all equal."""
    g = _gen("pool", K, C)
    x = torch.randn(POOL_GROUPS * K, C, generator=g)
    x[:, ::3] = -x[:, ::3].abs() - 0.5
    x[:, 1] = -2.0
    return x.to(BF)


# ------------------------------------------------------------------------------------------------ vision
def im2col_ref(pix, P, Kpad):
    """pix [B, CT, H, W] (fp32 or bf16) -> bf16 [B * gh * gw, Kpad], zero padded."""
    cols = F.unfold(pix[:, :3].float(), P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)
    out = torch.zeros(cols.shape[0], Kpad)
    out[:, :3 * P * P] = cols
    return out.to(BF)


# (dtype, B, CT, Himg, Wimg, P): Himg != Wimg. IM2COL_BIG crosses the 16384-block grid cap at Kpad = 640 (3 * 48 * 48 * 640 / 256 =
# 17 280 blocks of work; 15 876 at Kpad = 588, just under it)
IM2COL_CASES = tuple((dt, 2, ct, h, w, p) for dt in ("fp32", "bf16") for ct in (3, 4) for (h, w, p) in ((28, 42, 14), (6, 10, 2), (70, 28, 14)))
IM2COL_BIG = tuple((dt, 3, 4, 672, 672, 14) for dt in ("fp32", "bf16"))


def im2col_kpads(P):
    k = 3 * P * P
    return sorted({k, (k + 63) // 64 * 64})


def avgpool_ref(x, B, gh, gw, cs):
    """x [B * gh * gw, C] -> fp64 [B * oh * ow, C]"""
    C = x.shape[-1]
    y = F.avg_pool2d(x.double().view(B, gh, gw, C).permute(0, 3, 1, 2), cs, cs)
    return y.permute(0, 2, 3, 1).reshape(-1, C)


ATTN_C = (256, 512, 1024, 2048)
ATTN_CS = (1, 2, 3, 4)
ATTN_GRIDS = ((6, 12), (48, 48), (4, 8))
ATTN_B = (1, 3)
HEADS = 8


def grid_for(grid, cs):
    """The grid cropped to a multiple of cs (the model crops the patch grid the same way before it pools)."""
    return grid[0] // cs * cs, grid[1] // cs * cs


def attn_scales(C):
    return (C ** -0.5, 8 * C ** -0.5)


def attn_inputs(B, gh, gw, C, cs, seed=0):
    g = _gen("attn", B, gh, gw, C, cs, seed)
    nw = B * (gh // cs) * (gw // cs)
    return (torch.randn(nw, C, generator=g).to(BF), torch.randn(B * gh * gw, 2 * C, generator=g).to(BF),
            torch.randn(nw, C, generator=g).to(BF))


def local_attn_ref(q, kv, dout, B, gh, gw, cs, scale, heads=HEADS):
    """fp64 window attention (vision_tokenizer.py LocalAttention: one query per cs x cs window, 8 heads) and its autograd.
    Returns out [nw, C], dq [nw, C], dkv [B * gh * gw, 2C]."""
    C = q.shape[-1]
    oh, ow, hd = gh // cs, gw // cs, C // heads
    ql, kvl = q.double().requires_grad_(), kv.double().requires_grad_()
    qh = ql.view(B, oh, ow, heads, hd)
    kvh = kvl.view(B, oh, cs, ow, cs, 2, heads, hd).permute(0, 1, 3, 2, 4, 5, 6, 7).reshape(B, oh, ow, cs * cs, 2, heads, hd)
    s = torch.einsum("bijhd,bijnhd->bijhn", qh * scale, kvh[:, :, :, :, 0])
    out = torch.einsum("bijhn,bijnhd->bijhd", torch.softmax(s, -1), kvh[:, :, :, :, 1]).reshape(-1, C)
    out.backward(dout.double())
    return out.detach(), ql.grad, kvl.grad


def window_rows(t, B, gh, gw, cs):
    """[B * gh * gw, W] -> [windows, cs * cs * W]: the rows of every window side by side (per-window metrics of dkv)."""
    W = t.shape[-1]
    oh, ow = gh // cs, gw // cs
    return t.view(B, oh, cs, ow, cs, W).permute(0, 1, 3, 2, 4, 5).reshape(B * oh * ow, cs * cs * W)


def per_window_max_rel(a, ref):
    """max over the windows (rows) of max |a - ref| / max |ref| within the window; a window whose reference is identically zero must be
    identically zero (its ratio is then 0, else inf)."""
    a, ref = a.double(), ref.double()
    err, mag = (a - ref).abs().amax(-1), ref.abs().amax(-1)
    ratio = torch.where(mag > 0, err / mag.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()), int(ratio.argmax())


def fro(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


# ------------------------------------------------------------------------------------------------ slack
def one_rounding_violations(got, ref64, slack):
    """Elements with |got - ref| > 2^-8 |ref| + 4 slack (or not finite). Returns (count, worst excess, worst |err|)."""
    got, ref64 = got.double(), ref64.double()
    err = (got - ref64).abs()
    over = err - (2.0 ** -8 * ref64.abs() + 4 * slack)
    bad = (over > 0) | ~torch.isfinite(got)
    return int(bad.sum()), float(over.max()), float(err.max())


@functools.lru_cache(maxsize=None)
def measured_slack(family):
    """max |fp32 reference - fp64 reference| over every input of the family the GPU test uses (lga: all LGA_CK x LGA_CLOUDS; bn: all
    bn_shapes() of the zero_mean family with residual and without, before the relu, the constant column left out -- its 1 / sqrt(eps) =
    316 amplifies the rounding of the mean and the test holds it to its own condition)."""
    worst = 0.0
    if family == "lga":
        for C, K in LGA_CK:
            for cloud in LGA_CLOUDS:
                c = lga_case(cloud, C, K)
                worst = max(worst, float((lga_prep_ref(*c, dtype=torch.float32)[0].double() - lga_prep_ref(*c)[0]).abs().max()))
    elif family == "bn":
        for rows, C in bn_shapes():
            x, w, b, res = bn_inputs(rows, C)
            for r in (None, res):
                d = (bn_ref(x, w, b, res=r, dtype=torch.float32).double() - bn_ref(x, w, b, res=r)).abs()
                worst = max(worst, float(d[:, :C - 1].max()) if C > 1 else 0.0)
    else:
        raise ValueError(family)
    return worst


# ------------------------------------------------------------------------------------------------ small kernels
CE_CASES = tuple((dt, v, ld) for dt in ("bf16", "fp32") for (v, ld) in ((32064, 32064), (1000, 1000), (1000, 1024), (32001, 32064)))
CE_ROWS = 9


def ce_inputs(dt, ncols, ld):
    """logits [rows, ld] (columns >= ncols hold large values a kernel must not read into the softmax), labels (three rows ignored)."""
    g = _gen("ce", dt, ncols, ld)
    logits = torch.randn(CE_ROWS, ld, generator=g) * 2.0
    logits[:, ncols:] = 30.0
    if dt == "bf16":
        logits = _bf(logits)
    labels = torch.randint(0, ncols, (CE_ROWS,), generator=g)
    labels[0], labels[CE_ROWS - 1] = 0, ncols - 1
    labels[[1, 4, 6]] = -100
    return logits, labels


def ce_bwd_ref(logits, labels, ncols, inv_count, gscale, ignore_index=-100):
    """fp32 autograd of F.cross_entropy(..., ignore_index, reduction="sum") * inv_count * gscale; [rows, ncols] fp32."""
    l = logits[:, :ncols].float().clone().requires_grad_()
    (F.cross_entropy(l, labels, ignore_index=ignore_index, reduction="sum") * inv_count * gscale).backward()
    return l.grad
