"""Host-only helpers of tests/test_gen_kernels_gpu.py: input builders, case lists and references for the kernels of the post-training
generation heads (mla_amd/csrc/gen.hip) and the backward halves of the tokenizer kernels (mla_lga_prep_bwd, mla_maxpool_k_bwd in
pointcloud.hip, mla_avgpool_tokens_bwd in vision.hip). Nothing here needs a GPU: every reference works on the device of its arguments
and tests/test_gen_cases_host.py checks the module on the CPU.

Every bound comes from tests/trunk_cases.py (its docstring states the rules): bf16_ratio, scalar_ratio / mean_ratio, reduction_ratio,
bits_equal. Every reference is the formula in the kernel's comment, evaluated in fp64 (the expectation) and in fp32 without the output
rounding (slack = |ref32 - ref64|: per element for element-wise kernels, the row maximum for row kernels, the column maximum for the
column kernels of BatchNorm). The fp32 row sums run in the kernels' order (trunk_cases.block_sum32 for the 16-byte row kernels,
lane_sum32 here for the lane-strided softmax rows).

Dropout: keep_mask is a numpy uint64 statement of the counter hash documented at the top of gen.hip --
    x = idx * 0x9E3779B97F4A7C15 + seed;  x ^= x >> 32;  x *= 0xD6E8FEB86659FD93;  x ^= x >> 32;  x *= 0xD6E8FEB86659FD93;  x ^= x >> 32
    keep  <=>  (uint32(x) >> 8) * 2^-24 >= p          (exact in fp32; p as the ABI carries it; p <= 0 keeps everything)
-- so every dropout assertion is per element: dropped elements are exactly 0, kept ones bf16(x / (1 - p) [+ res]).

Sentinels: the rows of every reduction input carry weight where an indexing slip would lose them (the last row x 64, the first and
last row of every block's walk or slice x 8), so that losing one moves the result by >= 100 x its bound (asserted on the host).

Kinks of the image losses: sign(diff), sign(delta) jump at 0 and the warp derivative jumps where a sample coordinate is an integer or
meets the clamp. The builders push the inputs away from them (`next` is moved where |diff64| < 1e-4, `draw` where |delta64| < 1e-4, an
offset where a coordinate comes within 1e-4 of an integer), so that the guard sets of the issue are EMPTY and nothing is left out of
any comparison -- 0 elements and 0 patches, inside the cap of 0.1 % / 2 %; the host test asserts it from the reference alone. Shifts
of exactly 0 are kept: there the documented derivative is the right-sided one (floor), and the reference states it.

Chamfer: d1 / d2 are held to 8 U32 d + slack_d, slack_d the fp32 rounding term `tokenizer_cases.knn_delta` of the pair (a bound on the
squared distance) carried through the square root; an index is valid when its fp64 squared distance is within 2 delta of the minimum
(on lattice16 fp32 arithmetic is exact and the first minimum is the only valid index). The loss is a mean of the kernel's own d1 / d2
and is held to the reduction rule against the fp64 mean of those."""
import numpy as np
import torch

import tokenizer_cases as K
from trunk_cases import (BF, F32, F64, U16, U32, _gen, bf16_ratio, bits_equal, block_sum32, bwd_sentinel_rows, dw_check, f32v,  # noqa: F401
                         mean_ratio, norm_bias, norm_dy, norm_rows, norm_weight, reduction_bound, reduction_ratio, row_slack,
                         scalar_ratio, sentinel_ratio)

INF = float("inf")
NAN = float("nan")
LN_EPS = 1e-5
LN_FAMILIES = ("gauss", "outlier", "tiny", "offset", "rowscale")
LN_H = (8, 136, 2048, 2056, 8192)
LN_ROWS = (1, 5)
LN_BWD_SHAPES = ((1, 136), (37, 2056), (37, 8192), (511, 136), (512, 136), (513, 136), (1061, 2056))

BN_EPS = 1e-5
BN_ROWS = (1, 3, 1023, 2048, 3000, 131072 + 1029)
BN_C = (1, 63, 64, 65, 200)
BN_C_LARGE = (1, 65)
BN_FAMILIES = ("gauss", "offset", "constcol", "outlier_row")

SOFTMAX_SHAPES = ((8, 1), (8, 8), (64, 45), (256, 255), (264, 257), (552, 548), (1032, 1025))
SOFTMAX_ROWS = 5
SOFTMAX_FAMILIES = ("gauss", "near_uniform", "spike", "shifted", "masked")
SOFTMAX_P = (0.0, 0.1)
SEED = 0x1234567887654321

DROPOUT_N = (1, 255, 256, 257, 1003, 2097152 + 5)
DROPOUT_P = (0.0, 0.1, 0.5, 0.999)
SCALE_BATCH = (1, 4)
SCALE_PER = (1, 7, 4104)

SEQMEAN_SHAPES = ((1, 1, 1), (3, 45, 255), (2, 548, 257), (2, 7, 520))
AVGPOOL_SHAPES = ((1, 2, 2, 8, 2), (2, 6, 4, 24, 2), (2, 6, 6, 136, 3), (1, 4, 4, 8, 1))
LGA_SHAPES = ((1, 5, 1, 1, 8), (2, 70, 65, 9, 24), (1, 200, 130, 33, 264), (1, 300, 64, 128, 8))
LGA_LISTS = ("distinct", "hostile")
POOL_K = (1, 9, 128)
POOL_C = (1, 48, 264)
POOL_GROUPS = (1, 65)

CHAMFER_SHAPES = ((1, 1, 1), (2, 128, 300), (1, 255, 4096), (1, 4096, 257), (3, 256, 256))
CHAMFER_CLOUDS = ("uniform", "lattice16", "offset", "coincident")
CHAMFER_MAX = 4096

IMG_B, IMG_CTC, IMG_CTN = 2, 4, 3
IMG_GEOM = ((42, 84), (42, 336), (6, 24))
IMG_CLIP, IMG_SHIFT, IMG_GSCALE = 5.0, 8.0, 0.7
ROI_MASKS = ("random", "all", "none", "single")
ROI_SHIFTS = ("small", "border", "zero")
KINK = 1e-4


def img_lds(ps):
    """Row pitches of delta_raw: exactly 3 ps^2, and padded to the next multiple of 64."""
    pd = 3 * ps * ps
    return (pd, pd // 64 * 64 + 64)


# (mask, shifts) of the partial-ROI cases, run at every geometry, both image types; the row pitch alternates between the two of img_lds
ROI_CASES = (("random", "small"), ("random", "border"), ("random", "zero"), ("all", "border"), ("none", "border"), ("single", "small"))


# ------------------------------------------------------------------------------------------------ dropout hash
_M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)


def hash_u32(seed, idx):
    """The documented counter hash of (seed, flat index) -> uint32, in numpy uint64 (wrapping) arithmetic."""
    with np.errstate(over="ignore"):
        x = np.asarray(idx, dtype=np.uint64) * _M1 + np.uint64(seed)
        s = np.uint64(32)
        x ^= x >> s
        x *= _M2
        x ^= x >> s
        x *= _M2
        x ^= x >> s
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def keep_mask(seed, n, p, offset=0):
    """bool [n]: element offset + i is kept. (h >> 8) < 2^24 is exact in fp32, and so is its product with 2^-24."""
    if f32v(p) <= 0:
        return torch.ones(n, dtype=torch.bool)
    u = (hash_u32(seed, np.arange(offset, offset + n, dtype=np.uint64)) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy(u >= np.float32(p))


def inv_keep(p, dt):
    """1 / (1 - p) from p as the ABI carries it."""
    return torch.tensor(1.0, dtype=dt) / (torch.tensor(1.0, dtype=dt) - torch.tensor(f32v(p), dtype=dt)) if f32v(p) > 0 else torch.tensor(1.0, dtype=dt)


def dropout_ref(x, res, keep, p, dt):
    v = x.to(dt) * keep.to(x.device).to(dt) * inv_keep(p, dt).to(x.device)
    return v if res is None else v + res.to(dt)


def flat_bf16(n, tag):
    """N(0,1) pushed away from zero (a dropped element is told from a kept one by being exactly 0), the last elements 64, -96, 80."""
    x = torch.randn(n, generator=_gen("genflat", tag, n))
    x = x + 0.25 * torch.sign(x)
    x = torch.where(x == 0, torch.full_like(x, 0.25), x)          # randn does return an exact 0 now and then (n = 2097157 has one)
    k = min(3, n)
    x[n - k:] = torch.tensor([64.0, -96.0, 80.0])[3 - k:]
    return x.to(BF)


def scale_batch_case(batch, per):
    x = flat_bf16(batch * per, "scale").view(batch, per)
    scale = torch.tensor([0.0, 1.0 / 0.9, -1.75, 1.0 / 0.9][:batch] if batch > 1 else [1.0 / 0.9], dtype=F32)
    return x, scale


# ------------------------------------------------------------------------------------------------ LayerNorm with statistics
def ln_stats_ref(x, w, b, eps, dt):
    """(y, mean, rstd): the two-pass form of layernorm_stats_fwd_kernel."""
    H = x.shape[1]
    xs = x.to(dt)
    rs = (lambda v: v.sum(-1)) if dt == F64 else block_sum32
    mean = rs(xs) / H
    d = xs - mean[:, None]
    rstd = 1.0 / torch.sqrt(rs(d * d) / H + torch.tensor(f32v(eps), dtype=dt, device=x.device))
    return d * rstd[:, None] * w.to(dt) + b.to(dt), mean, rstd


def ln_bwd_ref(dy, x, w, mean32, rstd32, dt):
    """(dx, dw terms, db terms): dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum_rows dy xhat, db = sum_rows dy."""
    H = x.shape[1]
    rs = (lambda v: v.sum(-1)) if dt == F64 else block_sum32
    r, mu = rstd32.to(dt)[:, None], mean32.to(dt)[:, None]
    xh = (x.to(dt) - mu) * r
    g = dy.to(dt) * w.to(dt)
    s1, s2 = (rs(g) / H)[:, None], (rs(g * xh) / H)[:, None]
    return r * (g - s1 - xh * s2), dy.to(dt) * xh, dy.to(dt)


# ------------------------------------------------------------------------------------------------ BatchNorm(train) backward
def bn_blocks(rows):
    return min(max(rows // 1024, 1), 128)


def bn_sentinel_rows(rows):
    P = bn_blocks(rows)
    per = (rows + P - 1) // P
    out = set()
    for b in range(P):
        r0, r1 = b * per, min(b * per + per, rows)
        if r0 < r1:
            out |= {r0, r1 - 1}
    return sorted(out | {rows - 1})


def bn_case(family, rows, C):
    """(dy, x, w, mean32, var32): mean / var are the fp64 batch statistics of the bf16 input rounded to fp32."""
    g = _gen("bnbwd", family, rows, C)
    x = torch.randn(rows, C, generator=g)
    if family == "offset":
        x = x * 0.05 + 8.0
    elif family == "constcol":
        x[:, C // 2] = 1.375
    elif family == "outlier_row":
        # not on a sentinel row: 300 sigma x the sentinel weight would put > 90 % of sum |terms| into one term, after which every
        # addition of a lane's walk rounds at that term's ulp -- the honest fp32 sum in the kernel's order (bn_sums_emul32) is then
        # itself outside the reduction rule, and the input could not tell a right kernel from a wrong one
        x[rows // 3] = 300.0
    elif family != "gauss":
        raise ValueError(family)
    x = x.to(BF)
    dy = torch.randn(rows, C, generator=g)
    dy = dy + 0.25 * torch.sign(dy)
    for r in bn_sentinel_rows(rows):                  # x 256: at 132101 rows the bound of a column sum is ~0.3 of one average term
        dy[r] *= 256.0
    dy[rows - 1] *= 8.0
    w = (1.0 + 0.1 * torch.randn(C, generator=g)).to(BF)
    xs = x.to(F64)
    mean = xs.mean(0)
    var = ((xs - mean) ** 2).mean(0)
    return dy.to(BF), x, w, mean.to(F32), var.to(F32)


def bn_bwd_ref(dy, x, w, mean32, var32, eps, dt):
    """(dx, dw terms, db terms): dx = w rstd (dy - sum dy / N - xhat sum(dy xhat) / N)."""
    N = x.shape[0]
    rs = 1.0 / torch.sqrt(var32.to(dt) + torch.tensor(f32v(eps), dtype=dt, device=x.device))
    xh = (x.to(dt) - mean32.to(dt)) * rs
    d = dy.to(dt)
    return w.to(dt) * rs * (d - d.sum(0) / N - xh * (d * xh).sum(0) / N), d * xh, d


def bn_sums_emul32(terms32):
    """fp32 column sums of terms [rows, C] in the order of bn_bwd_partial_kernel + reduce_strided_kernel: the rows are cut into
    bn_blocks(rows) slices; in a slice, row lane l adds rows l, l + 4, ... in turn and the four lanes are added in turn; the slice
    partials p, p + 4, ... are added in turn by lane p % 4 and joined as (0 + 1) + (2 + 3)."""
    rows, C = terms32.shape
    P = bn_blocks(rows)
    per = (rows + P - 1) // P
    steps = (per + 3) // 4
    pad = torch.zeros(P, steps * 4, C, dtype=F32, device=terms32.device)
    for b in range(P):
        r0, r1 = b * per, min(b * per + per, rows)
        pad[b, :r1 - r0] = terms32[r0:r1]
    pad = pad.view(P, steps, 4, C)
    acc = torch.zeros(P, 4, C, dtype=F32, device=terms32.device)
    for s in range(steps):
        acc = acc + pad[:, s]
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    lane = torch.zeros(4, C, dtype=F32, device=terms32.device)
    for b in range(P):
        lane[b % 4] = lane[b % 4] + part[b]
    return (lane[0] + lane[1]) + (lane[2] + lane[3])


# ------------------------------------------------------------------------------------------------ masked row softmax
def lane_sum32(v):
    """fp32 row sums in the order of the lane-strided 256-lane kernels: lane t adds columns t, t + 256, ... in turn, a pairwise tree
    joins the 64 lanes of a wave, the four waves are added in turn from 0."""
    rows, n = v.shape
    trips = (n + 255) // 256
    pad = torch.zeros(rows, trips * 256, dtype=F32, device=v.device)
    pad[:, :n] = v.to(F32)
    pad = pad.view(rows, trips, 256)
    acc = torch.zeros(rows, 256, dtype=F32, device=v.device)
    for t in range(trips):
        acc = acc + pad[:, t]
    a = acc.view(rows, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a[..., :o] + a[..., o:2 * o]
    a = a[..., 0]
    return (((torch.zeros_like(a[:, 0]) + a[:, 0]) + a[:, 1]) + a[:, 2]) + a[:, 3]


def softmax_scores(family, ncols, nvalid, rows=SOFTMAX_ROWS):
    """fp32 [rows, ncols]; the padding columns hold NaN (they are never read)."""
    g = _gen("softmax", family, ncols, nvalid)
    x = torch.randn(rows, nvalid, generator=g)
    if family == "gauss":
        x = x * 3.0
    elif family == "near_uniform":
        x = x * 1e-3
    elif family == "spike":
        x[:, nvalid - 1] += 60.0
    elif family == "shifted":
        x = x + 1e4
    elif family == "masked":
        x = x * 3.0
        hole = torch.rand(rows, nvalid, generator=g) < 0.3
        hole[:, nvalid - 1] = False
        x[hole] = -INF
    else:
        raise ValueError(family)
    s = torch.full((rows, ncols), NAN)
    s[:, :nvalid] = x
    return s


def softmax_keep(rows, ncols, p, seed=SEED):
    """The mask of the Pd output: indexed by r * ncols + c, padding columns included."""
    return keep_mask(seed, rows * ncols, p).view(rows, ncols)


def softmax_fwd_ref(scores, nvalid, keep, p, dt):
    """(P, Pd) [rows, ncols]: softmax over the first nvalid columns, 0 beyond; Pd = P keep / (1 - p)."""
    rows, ncols = scores.shape
    x = scores[:, :nvalid].to(dt)
    e = torch.exp(x - x.amax(-1, keepdim=True))
    den = e.sum(-1) if dt == F64 else lane_sum32(e)
    P = torch.zeros(rows, ncols, dtype=dt, device=scores.device)
    P[:, :nvalid] = e / den[:, None]
    return P, P * keep.to(scores.device).to(dt) * inv_keep(p, dt).to(scores.device)


def softmax_dpd(family, ncols, nvalid, dtype, rows=SOFTMAX_ROWS):
    """Upstream gradient; NaN in the padding columns. near_uniform carries the large common value of the round-6 comment."""
    g = torch.randn(rows, nvalid, generator=_gen("dpd", family, ncols, nvalid))
    if family == "near_uniform":
        g = g * 0.05 + 32.0
    d = torch.full((rows, ncols), NAN)
    d[:, :nvalid] = g
    return d.to(dtype)


def softmax_saved_p(scores, nvalid):
    """The bf16 rounding of the fp64 softmax: what backward is fed, independent of the forward kernel."""
    keep = torch.ones(scores.shape, dtype=torch.bool)
    return softmax_fwd_ref(scores, nvalid, keep, 0.0, F64)[0].to(F32).to(BF)


def softmax_bwd_ref(dPd, P, nvalid, keep, p, dt):
    """dS = P' (g - sum_c g P'), g = dPd keep / (1 - p), P' = P / sum_c P; 0 in the padding columns (which are never read)."""
    rows, ncols = P.shape
    rs = (lambda v: v.sum(-1)) if dt == F64 else lane_sum32
    g = dPd[:, :nvalid].to(dt) * keep[:, :nvalid].to(P.device).to(dt) * inv_keep(p, dt).to(P.device)
    pr = P[:, :nvalid].to(dt)
    psum = rs(pr)
    inv = torch.where(psum > 0, 1.0 / psum, torch.zeros_like(psum))[:, None]
    dot = rs(g * pr)[:, None] * inv
    dS = torch.zeros(rows, ncols, dtype=dt, device=P.device)
    dS[:, :nvalid] = pr * inv * (g - dot)
    return dS


def rowsum_ratio(got, ref64, nvalid):
    """The near-uniform invariant: the documented renormalised form sums to 0 per row before rounding, so |sum_c dS| is held to the
    rounding of dS alone, nvalid U16 max|dS|."""
    s = got.to(F64).sum(-1).abs()
    return float((s / (nvalid * U16 * ref64.abs().amax(-1) + 2.0 ** -120)).max())


# ------------------------------------------------------------------------------------------------ seqmean, avgpool
def seqmean_input(B, S, C):
    x = torch.randn(B, S, C, generator=_gen("seqmean", B, S, C))
    x[:, S - 1] *= 8.0
    return x.to(BF)


def seqmean_fwd_ref(x):
    """(mean64 [B, C], slack): slack = the reduction rule over the S terms, divided by S."""
    S = x.shape[1]
    xs = x.to(F64)
    return xs.sum(1) / S, reduction_bound(S, xs.abs().sum(1)) / S


def seqmean_bwd_ref(dy, S, dt):
    return (dy.to(dt) / S)[:, None, :].expand(dy.shape[0], S, dy.shape[1])


def avgpool_bwd_case(B, gh, gw, C, cs):
    g = _gen("avgpoolbwd", B, gh, gw, C, cs)
    dy = torch.randn(B * (gh // cs) * (gw // cs), C, generator=g)
    dy[-1] *= 8.0
    return dy.to(BF), torch.randn(B * gh * gw, C, generator=g).to(BF)


def avgpool_bwd_ref(dy, other, B, gh, gw, cs, dt):
    """dx[b, y, x, c] = dy[b, y / cs, x / cs, c] / cs^2 (+ other[b, y, x, c])."""
    C = dy.shape[1]
    d = dy.to(dt).view(B, gh // cs, gw // cs, C) * torch.tensor(f32v(1.0 / (cs * cs)) if dt == F32 else 1.0 / (cs * cs), dtype=dt)
    d = d.repeat_interleave(cs, 1).repeat_interleave(cs, 2).reshape(B * gh * gw, C)
    return d if other is None else d + other.to(dt)


# ------------------------------------------------------------------------------------------------ lga_prep_bwd, maxpool_k_bwd
def lga_bwd_case(B, N, G, K, C, lists):
    """(drows [B G K, 2C] bf16, fps_idx [B, G] int64, knn [B, G, K] int32, unused points). `distinct`: every group lists K distinct
    points. `hostile`: on top of that one point sits in every group at position K - 1, group 0 repeats an index, and every even
    group lists its own centre. The last two points (N >= K + 3) are in no list and centre no group: they must read exactly 0."""
    g = _gen("lgabwd", B, N, G, K, C, lists)
    spare = 2 if N >= K + 3 else 0
    pool = N - spare
    knn = torch.stack([torch.stack([torch.randperm(pool, generator=g)[:K] for _ in range(G)]) for _ in range(B)])
    fps = torch.stack([torch.randperm(pool, generator=g)[:G] for _ in range(B)])
    if lists == "hostile":
        knn[:, :, K - 1] = pool // 2
        if K >= 3:
            knn[:, 0, 1] = knn[:, 0, 0]
        knn[:, ::2, 0] = fps[:, ::2]
    elif lists != "distinct":
        raise ValueError(lists)
    drows = torch.randn(B * G * K, 2 * C, generator=g)
    drows[-1] *= 8.0
    return drows.to(BF), fps.long(), knn.int(), list(range(pool, N))


def lga_bwd_emul(drows, fps_idx, knn, B, N, C, dt):
    """(dfeats [B, N, C], sum of |terms|, number of terms [B, N]) in the documented order: ascending g, then ascending k, every hit
    added in turn; then the k-sum of the group centred on the point (summed in ascending k) as one term."""
    G, K = knn.shape[1], knn.shape[2]
    npdt = np.float64 if dt == F64 else np.float32
    d = drows.to(F32).cpu().numpy().astype(npdt).reshape(B, G, K, 2 * C)
    kn, fp = knn.cpu().numpy(), fps_idx.cpu().numpy()
    acc, sab, cnt = np.zeros((B, N, C), npdt), np.zeros((B, N, C), np.float64), np.zeros((B, N), np.int64)
    bs = np.arange(B)
    for g in range(G):
        for k in range(K):
            n = kn[:, g, k]
            acc[bs, n] = acc[bs, n] + d[:, g, k, :C]
            sab[bs, n] += np.abs(d[:, g, k, :C])
            cnt[bs, n] += 1
    s = np.zeros((B, G, C), npdt)
    for k in range(K):
        s = s + d[:, :, k, C:]
    for g in range(G):
        n = fp[:, g]
        acc[bs, n] = acc[bs, n] + s[:, g]
        sab[bs, n] += np.abs(d[:, g, :, C:]).sum(1)
        cnt[bs, n] += K
    return torch.from_numpy(acc), torch.from_numpy(sab), torch.from_numpy(cnt)


def lga_bwd_index_add(drows, fps_idx, knn, B, N, C):
    """The same gradient as a scatter, fp64 (the independent formulation of the host test)."""
    G, K = knn.shape[1], knn.shape[2]
    d = drows.to(F64).view(B, G * K, 2 * C)
    out = torch.zeros(B, N, C, dtype=F64)
    for b in range(B):
        out[b].index_add_(0, knn[b].reshape(-1).long(), d[b, :, :C])
        out[b].index_add_(0, fps_idx[b], d[b, :, C:].view(G, K, C).sum(1))
    return out


def pool_bwd_case(groups, K, C):
    """(x [groups K, C] bf16, dy [groups, C]): column 0 all equal, column C - 1 all -inf, ties of the maximum elsewhere (the value of
    neighbour K // 2 copied to the last), so that only `first maximum` is right."""
    g = _gen("poolbwd", groups, K, C)
    x = torch.randn(groups, K, C, generator=g).to(BF)
    top = x.float().amax(1)
    x[:, K - 1, :] = torch.where(torch.rand(groups, C, generator=g) < 0.5, top.to(BF), x[:, K - 1, :])
    x[:, :, 0] = 0.75
    if C > 1:
        x[:, :, C - 1] = -INF
    dy = torch.randn(groups, C, generator=g)
    dy = (dy + 0.25 * torch.sign(dy)).to(BF)
    return x.view(groups * K, C), dy


def pool_bwd_ref(x, dy, groups, K, last=False):
    """dx: dy at the first neighbour that attains the maximum, 0 elsewhere (last = True: the wrong `last maximum`)."""
    C = x.shape[1]
    v = x.to(F32).cpu().numpy().reshape(groups, K, C)
    arg = (K - 1 - np.argmax(v[:, ::-1], axis=1)) if last else np.argmax(v, axis=1)       # numpy returns the first occurrence
    onehot = torch.from_numpy(arg)[:, None, :] == torch.arange(K)[None, :, None]
    return torch.where(onehot.to(dy.device), dy[:, None, :].expand(groups, K, C), torch.zeros((), dtype=BF, device=dy.device)).reshape(groups * K, C)


# ------------------------------------------------------------------------------------------------ chamfer
def chamfer_case(cloud, B, N, M):
    """(pred [B, N, 3], gt [B, M, 3]) fp32. `coincident`: uniform clouds, the first min(3, N, M) points of pred copied from gt."""
    base = "uniform" if cloud == "coincident" else cloud
    pred, gt = K.make_cloud(base, B, N, seed=1), K.make_cloud(base, B, M, seed=2)
    if cloud == "coincident":
        k = min(3, N, M)
        pred[:, :k] = gt[:, M - k:]
    return pred, gt


def chamfer_fwd_ref(pred, gt):
    """dict(sq [B, N, M] fp64 squared distances, delta [B, N, M], d1, i1, d2, i2): distances fp64, indices the first minimum."""
    sq = K.knn_d64(gt, pred)                       # centres = pred: [B, N, M]
    delta = K.knn_delta(gt, pred)
    i1 = torch.from_numpy(np.argmin(sq.cpu().numpy(), axis=2))
    i2 = torch.from_numpy(np.argmin(sq.cpu().numpy(), axis=1))
    return dict(sq=sq, delta=delta, d1=sq.amin(2).sqrt(), i1=i1.to(pred.device), d2=sq.amin(1).sqrt(), i2=i2.to(pred.device))


def chamfer_dist_check(d, i, sq, delta, exact):
    """(ratio of the distances, number of invalid indices) of one direction: sq / delta [B, A, Bn], d / i [B, A] minima over the last
    axis. Distances: 8 U32 d + slack_d, slack_d = min(delta / (2 d), sqrt(delta)) at the chosen pair (0 on exact clouds)."""
    mn, first = sq.min(-1)
    ii = i.long().clamp(0, sq.shape[-1] - 1)
    chosen_sq, chosen_delta = sq.gather(-1, ii[..., None])[..., 0], delta.gather(-1, ii[..., None])[..., 0]
    in_range = (i >= 0) & (i < sq.shape[-1])
    if exact:
        bad = int((~in_range | (ii != torch.from_numpy(np.argmin(sq.cpu().numpy(), axis=-1)).to(i.device))).sum())
        slack = torch.zeros_like(mn)
    else:
        bad = int((~in_range | (chosen_sq > mn + 2 * chosen_delta)).sum())
        dd = mn.sqrt()
        slack = torch.minimum(chosen_delta / (2 * dd).clamp(min=1e-300), chosen_delta.sqrt())
    ref = mn.sqrt()
    return scalar_ratio(d, ref, ref + slack / (8 * U32)), bad


def chamfer_loss_ratio(loss, d1, d2):
    """The loss against the fp64 mean of the kernel's own d1 / d2: mean_b(mean_n d1 + mean_m d2)."""
    B, N = d1.shape
    M = d2.shape[1]
    t = torch.cat([d1.to(F64).reshape(-1) / (B * N), d2.to(F64).reshape(-1) / (B * M)])
    return reduction_ratio(loss.reshape(1), t.sum().reshape(1), t.numel(), t.abs().sum().reshape(1))


def chamfer_bwd_ref(pred, gt, d1, i1, d2, i2, gscale, dt):
    """(dpred [B, N, 3], sum |terms|, terms per output [B, N]); d1 / d2 fp32 as saved, clamped at 1e-12."""
    B, N, _ = pred.shape
    M = gt.shape[1]
    g = gscale.to(dt)[0] / B
    p, q = pred.to(dt), gt.to(dt)
    lo = torch.tensor(f32v(1e-12), dtype=dt, device=pred.device)
    q1 = torch.gather(q, 1, i1.long()[..., None].expand(B, N, 3))
    t1 = (p - q1) * (g / (N * torch.maximum(d1.to(dt), lo)))[..., None]
    p2 = torch.gather(p, 1, i2.long()[..., None].expand(B, M, 3))
    t2 = (p2 - q) * (g / (M * torch.maximum(d2.to(dt), lo)))[..., None]
    out, sab = t1.clone(), t1.abs().to(F64)
    cnt = torch.ones(B, N, dtype=torch.long, device=pred.device)
    for b in range(B):
        out[b].index_add_(0, i2[b].long(), t2[b])
        sab[b].index_add_(0, i2[b].long(), t2[b].abs().to(F64))
        cnt[b].index_add_(0, i2[b].long(), torch.ones(M, dtype=torch.long, device=pred.device))
    return out, sab, cnt


# ------------------------------------------------------------------------------------------------ image losses
def patches(img, ps, CT=None):
    """[B, CT, HW, HW] -> [B npatch, 3, ps, ps] of channels 0..2 (images_to_patches order). CT overrides the channel count the flat
    buffer is read with (the mutation `CT_curr swapped for CT_next`)."""
    B, C, HW, _ = img.shape
    if CT is not None and CT != C:
        img = img.reshape(-1)[:B * CT * HW * HW].view(B, CT, HW, HW)
    g = HW // ps
    x = img[:, :3].reshape(B, 3, g, ps, g, ps).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B * g * g, 3, ps, ps)


def _images(ps, HW, dtype, tag):
    g = _gen("img", ps, HW, tag)
    curr = torch.randn(IMG_B, IMG_CTC, HW, HW, generator=g)
    # every (sample, channel) plane has its own level, -28 .. 28: a slip in the channel count or the plane index moves 0.05 curr by >= 0.4
    curr = (curr + (8.0 * torch.arange(IMG_B * IMG_CTC) - 28.0).view(IMG_B, IMG_CTC, 1, 1)).to(dtype)
    nxt = torch.randn(IMG_B, IMG_CTN, HW, HW, generator=g).to(dtype)
    return curr, nxt, g


def _draw(npatch_all, ps, ld, g):
    """bf16 [B, npatch, ld]: N(0,1) with |draw| >= 2^-6 (away from the kink of sign(delta)); the padding columns hold NaN."""
    pd = 3 * ps * ps
    d = torch.randn(npatch_all, pd, generator=g)
    d = torch.where(d.abs() < 2.0 ** -6, torch.full_like(d, 0.5), d)
    out = torch.full((npatch_all, ld), NAN)
    out[:, :pd] = d
    return out.to(BF).view(IMG_B, npatch_all // IMG_B, ld)


def _unpatch_add(nxt, corr, ps):
    """nxt [B, 3, HW, HW] + corr [B npatch, 3, ps, ps] put back at the patches' places."""
    B, C, HW, _ = nxt.shape
    g = HW // ps
    c = corr.view(B, g, g, 3, ps, ps).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, HW, HW)
    return (nxt.to(F64) + c).to(nxt.dtype)


def imgloss_case(ps, HW, ld, dtype):
    """(draw, curr, next): `next` is moved by 0.5 wherever |diff64| < 1e-4, so that no element sits on the kink of sign(diff)."""
    curr, nxt, g = _images(ps, HW, dtype, "full")
    npatch = (HW // ps) ** 2
    draw = _draw(IMG_B * npatch, ps, ld, g)
    for _ in range(3):
        r = imgloss_ref(draw, curr, nxt, ps, IMG_CLIP, None, F64)
        near = r["diff"].abs() < 8 * KINK
        if not bool(near.any()):
            break
        nxt = _unpatch_add(nxt, near.to(F64) * 0.5, ps)
    return draw, curr, nxt


def imgloss_ref(draw, curr, nxt, ps, clip, gscale, dt, ct_curr=None):
    """dict(sums [3], sumabs [3], n, ddraw [B, npatch, pd] (gscale given), diff, delta): generated = 0.05 curr + clip tanh(draw);
    sums = { sum diff^2, sum |diff|, sum |delta| }; d(draw) = gscale / n (2 diff + 0.5 sign(diff) - 0.1 sign(delta)) clip (1 - tanh^2)."""
    B, npatch, ld = draw.shape
    pd = 3 * ps * ps
    th = torch.tanh(draw[..., :pd].to(dt)).reshape(B * npatch, 3, ps, ps)
    delta = clip * th
    diff = torch.tensor(0.05, dtype=F32).to(dt) * patches(curr, ps, ct_curr).to(dt) + delta - patches(nxt, ps).to(dt)
    terms = [diff * diff, diff.abs(), delta.abs()]
    out = dict(sums=torch.stack([t.sum() for t in terms]), sumabs=torch.stack([t.to(F64).sum() for t in terms]), n=diff.numel(),
               diff=diff, delta=delta)
    if gscale is not None:
        g = gscale.to(dt)[0] / diff.numel()
        dd = g * (2 * diff + 0.5 * torch.sign(diff) - torch.tensor(0.1, dtype=F32).to(dt) * torch.sign(delta)) * clip * (1 - th * th)
        out["ddraw"] = dd.reshape(B, npatch, pd)
    return out


def roi_mask(kind, n):
    g = _gen("roi", kind, n)
    if kind == "random":
        m = torch.rand(n, generator=g) < 0.35
        m[0], m[n - 1] = True, False
    elif kind == "all":
        m = torch.ones(n, dtype=torch.bool)
    elif kind == "none":
        m = torch.zeros(n, dtype=torch.bool)
    elif kind == "single":
        m = torch.zeros(n, dtype=torch.bool)
        m[n - 1] = True
    else:
        raise ValueError(kind)
    return m.to(torch.uint8)


def roi_coef(roi, npatch_all, ps, gscale=IMG_GSCALE):
    """coef[3] = { g / n_roi, 0.01 g / n_bg, -0.1 g / n_all } in elements, zero where a term is absent (fp32, as ops builds it)."""
    pd = 3 * ps * ps
    n_roi = int(roi.sum()) * pd
    n_bg = npatch_all * pd - n_roi
    return torch.tensor([gscale / n_roi if n_roi else 0.0, 0.01 * gscale / n_bg if n_bg else 0.0, -0.1 * gscale / (npatch_all * pd)], dtype=F32)


def imgroi_case(ps, HW, ld, dtype, mask, shifts):
    """(draw, a_raw [B npatch, 8], o_raw [B npatch, 8], roi u8 [B npatch], curr, next). a_raw / o_raw are 2-D with a row pitch of 8,
    the unused columns NaN. a_raw holds +-20 on the first background rows; o_raw: `small` |t| < 1 px, `border` |t| up to shift (rows
    and columns cross both borders), `zero` exactly 0. Offsets whose sample coordinates come within 1e-4 of an integer are replaced,
    and `next` is moved wherever |diff64| < 1e-4."""
    curr, nxt, g = _images(ps, HW, dtype, "roi" + mask + shifts)
    n = IMG_B * (HW // ps) ** 2
    draw = _draw(n, ps, ld, g)
    roi = roi_mask(mask, n)
    a = torch.full((n, 8), NAN)
    a[:, 0] = torch.randn(n, generator=g) * 1.5
    a[1::7, 0], a[2::7, 0] = 20.0, -20.0
    o = torch.full((n, 8), NAN)
    if shifts == "small":
        o[:, :2] = (torch.rand(n, 2, generator=g) * 2 - 1) * 0.1
    elif shifts == "border":
        o[:, :2] = torch.randn(n, 2, generator=g) * 1.5
    elif shifts == "zero":
        o[:, :2] = 0.0
    else:
        raise ValueError(shifts)
    o = o.to(BF)
    if shifts != "zero":
        for _ in range(4):
            t = IMG_SHIFT * torch.tanh(o[:, :2].to(F64))
            near = (t - t.round()).abs() < 8 * KINK
            if not bool(near.any()):
                break
            o[:, :2] = torch.where(near, (o[:, :2].float() * 0.75 + 0.05).to(BF), o[:, :2])
    a = a.to(BF)
    for _ in range(3):
        r = imgroi_ref(draw, a, o, roi, curr, nxt, ps, IMG_CLIP, IMG_SHIFT, None, F64)
        near = r["diff"].abs() < 8 * KINK
        if not bool(near.any()):
            break
        nxt = _unpatch_add(nxt, near.to(F64) * 0.5, ps)
    return draw, a, o, roi, curr, nxt


def imgroi_ref(draw, a_raw, o_raw, roi, curr, nxt, ps, clip, shift, coef, dt, ct_curr=None):
    """The documented formula of imgroi_kernel. ROI patch: diff = 0.05 curr + delta - next (MSE + 0.5 L1). Other patches:
    diff = alpha (warp(curr; tx, ty) + delta) + (1 - alpha) curr - next (0.01 L1), warp = bilinear sample of the patch at
    (x + tx, y + ty) with the border clamp, its derivative 0 where the clamp acts. All: -0.1 mean |delta|.
    dict(sums [4], sumabs [4], diff, delta, coord (sx, sy before the clamp); with coef: ddraw, dalpha, doff and the sums of |terms|
    of dalpha / doff per patch)."""
    B, npatch, ld = draw.shape
    n, pd, dev = B * npatch, 3 * ps * ps, draw.device
    one = torch.ones((), dtype=dt, device=dev)
    th = torch.tanh(draw[..., :pd].to(dt)).reshape(n, 3, ps, ps)
    delta = clip * th
    cp, npx = patches(curr, ps, ct_curr).to(dt), patches(nxt, ps).to(dt)
    inroi = (roi != 0).view(n, 1, 1, 1)
    alpha = (one / (one + torch.exp(-a_raw[:, 0].to(dt)))).view(n, 1, 1, 1)
    tt = torch.tanh(o_raw[:, :2].to(dt))
    tx, ty = (shift * tt[:, 0]).view(n, 1, 1), (shift * tt[:, 1]).view(n, 1, 1)
    ar = torch.arange(ps, dtype=dt, device=dev)
    mx = float(ps - 1)
    sx0, sy0 = (ar.view(1, 1, ps) + tx).expand(n, ps, ps), (ar.view(1, ps, 1) + ty).expand(n, ps, ps)
    cx, cy = (sx0 < 0) | (sx0 > mx), (sy0 < 0) | (sy0 > mx)
    sx, sy = sx0.clamp(0, mx), sy0.clamp(0, mx)
    xi, yi = torch.floor(sx), torch.floor(sy)
    wx, wy = (sx - xi).unsqueeze(1), (sy - yi).unsqueeze(1)
    xi, yi = xi.long(), yi.long()
    xj, yj = (xi + 1).clamp(max=ps - 1), (yi + 1).clamp(max=ps - 1)
    flat = cp.reshape(n, 3, ps * ps)

    def px(y, x):
        return torch.gather(flat, 2, (y * ps + x).view(n, 1, ps * ps).expand(n, 3, ps * ps)).view(n, 3, ps, ps)
    p00, p01, p10, p11 = px(yi, xi), px(yi, xj), px(yj, xi), px(yj, xj)
    zero = torch.zeros((), dtype=dt, device=dev)
    ddx = torch.where(cx.unsqueeze(1), zero, (1 - wy) * (p01 - p00) + wy * (p11 - p10))
    ddy = torch.where(cy.unsqueeze(1), zero, (1 - wx) * (p10 - p00) + wx * (p11 - p01))
    wv = (1 - wy) * ((1 - wx) * p00 + wx * p01) + wy * ((1 - wx) * p10 + wx * p11)
    d_roi = torch.tensor(0.05, dtype=F32).to(dt) * cp + delta - npx
    d_bg = alpha * (wv + delta) + (1 - alpha) * cp - npx
    diff = torch.where(inroi, d_roi, d_bg)
    terms = [torch.where(inroi, diff * diff, zero), torch.where(inroi, diff.abs(), zero), torch.where(inroi, zero, diff.abs()), delta.abs()]
    out = dict(sums=torch.stack([t.sum() for t in terms]), sumabs=torch.stack([t.to(F64).sum() for t in terms]), diff=diff, delta=delta,
               coord=(sx0, sy0), inroi=inroi)
    if coef is not None:
        k = coef.to(dt).to(dev)
        gp = k[1] * torch.sign(diff)
        gdelta = torch.where(inroi, k[0] * (2 * diff + 0.5 * torch.sign(diff)), gp * alpha) + k[2] * torch.sign(delta)
        out["ddraw"] = (gdelta * clip * (1 - th * th)).reshape(B, npatch, pd)
        ta = torch.where(inroi, zero, gp * (wv + delta - cp))
        tgx, tgy = torch.where(inroi, zero, gp * alpha * ddx), torch.where(inroi, zero, gp * alpha * ddy)
        fa = (alpha * (1 - alpha)).view(n)
        fo = shift * (1 - tt * tt)
        out["dalpha"] = ta.sum((1, 2, 3)) * fa
        out["doff"] = torch.stack([tgx.sum((1, 2, 3)), tgy.sum((1, 2, 3))], 1) * fo
        out["dalpha_abs"] = ta.to(F64).abs().sum((1, 2, 3)) * fa.to(F64)
        out["doff_abs"] = torch.stack([tgx.to(F64).abs().sum((1, 2, 3)), tgy.to(F64).abs().sum((1, 2, 3))], 1) * fo.to(F64).abs()
    return out


def kink_sets(ref, shifts, ps):
    """(elements under a guard, background patches with a coordinate under a guard) of an image-loss reference (fp64): |diff| < 1e-4,
    |delta| < 1e-4; a sample coordinate within 1e-4 of an integer or of the clamp edge (exactly-zero shifts exempt)."""
    el = (ref["diff"].abs() < KINK) | (ref["delta"].abs() < KINK)
    pt = torch.zeros(ref["diff"].shape[0], dtype=torch.bool, device=el.device)
    if "coord" in ref and shifts != "zero":
        for s in ref["coord"]:
            near = ((s - s.round()).abs() < KINK).flatten(1).any(1)
            pt |= near & ~ref["inroi"].view(-1)
    return el, pt


def fp32_ratio(got, ref64, ref32, n, sumabs):
    """fp32 sums of n terms: the reduction rule + 4 slack, slack = |ref32 - ref64|."""
    g = got.to(F64)
    err = (g - ref64).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, INF))
    bound = reduction_bound(n, sumabs) + 4 * (ref32.to(F64) - ref64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.where(torch.isnan(r), torch.full_like(r, INF), r).max())
