"""Host-only helpers of tests/test_trunk_kernels_gpu.py: input families, case lists, fp64 references, fp32 emulations and the bound
functions for the HBM-bound kernels every training step runs -- RMSNorm forward / prep / backward, the timm RmsNorm, LayerNorm
forward, SwiGLU and the four activations, RoPE, casts and add, column sums, the gradient-norm reduction, the clip coefficient,
AdamW, CE forward, InfoNCE backward and L2 normalisation (mla_amd/csrc/elementwise.hip, loss.hip, the *_t / *_dual forms of
transpose.hip). Nothing here needs a GPU: every function works on the device of its arguments, and tests/test_trunk_cases_host.py
checks the module on the CPU.

Unit round-offs: U16 = 2^-8 (bf16), U32 = 2^-24 (fp32).

Bound rules (the GPU file never invents a tolerance; every ratio printed there is |err| / bound from one of these):
  bf16 output, per element   |got - ref64| <= k U16 (1 + 2^-6) |ref64| + 4 slack + 2^-120                          (bf16_ratio)
                             k = number of bf16 roundings on the documented path: 2 for rmsnorm_fwd (the cast before the weight
                             multiply, then the output), 1 otherwise. slack = |ref32 - ref64|, ref32 = the same formula in fp32
                             without the output rounding; per element for element-wise kernels, the row maximum for row kernels.
                             The row sums of ref32 are taken in the order the kernels document (block_sum32: every lane of a
                             256-lane block walks its 16-byte chunks, then a pairwise tree over a wave, then the four waves in
                             turn). 2^-120 allows the flush of sub-normals. No element is excluded; a NaN is outside.
  fp32 per-row scalar        |got - ref64| <= 8 U32 scale; scale = |ref64|, max(1, |lse|) for lse, |lse| + |logit[label]| for the
                             loss (0 for an ignored row: exactly 0 is expected)                                    (scalar_ratio)
                             The row mean of the timm RmsNorm keeps this rule on rows that do not cancel (`offset`); on the
                             others it is a signed sum and is held to the reduction rule, a change to the issue's rule (mean_ratio)
  fp32 reduction, n terms    |got - ref64| <= (ceil(log2 n) + 8) U32 sum |terms|                                 (reduction_ratio)
  AdamW, one step            adamw_ratios: m 8 U32 (|b1 m| + |(1 - b1) g gs|), v 8 U32 v64, p 2 U32 |p| + 8 U32 U with
                             U = lr / bc1 (|b1 m| + |(1 - b1) g gs|) / den64. The fp64 reference takes the hyper-parameters as the
                             ABI carries them (fp32, promoted) and forms the bias corrections in double.
  exact                      integer, copy and cast outputs bit for bit, a NaN matching any NaN                      (bits_equal)

Sentinels: every reduction input carries weight where an indexing slip would lose it -- the last row x 64, the first and last row of
every block's row slice x 8, the last three elements of a flat array 64 / -96 / 80 -- so that losing one of them moves the result by
>= 100 x the bound (sentinel_ratio; asserted per family by the host test).

Row families (bf16 rows): gauss N(0,1); outlier 2500 at column H - 1, -900 at column 0, +-300 on the 2047 | 2048 seam; tiny x 1e-4
(eps dominates the mean square); offset 0.05 N(0,1) + 7 (the cancellation of the timm variance); rowscale rows x logspace(-3, 3).

The unary kernels run over every finite bf16 bit pattern with |x| <= 65536 (unary_inputs). The range stops there because beyond
about 1e19 the derivative of the tanh GELU is 0 x inf in fp32 in any implementation (x^2 overflows next to 1 - tanh^2 = 0).

Documented limit: SwiGLU takes its sigmoid from the hardware reciprocal, which flushes a result below 2^-126 to 0 (gates below
-87.3). The 2^-120 floor does not cover that (the lost sigmoid is multiplied by |gate| ~ 87 and by `up`), so for those gates the
expected output is the documented 0 (sigmoid_flushed / flush_expected). The SiLU activation kernels divide instead and follow the rule."""
import functools
import math

import numpy as np
import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U16 = 2.0 ** -8
U32 = 2.0 ** -24
FLOOR = 2.0 ** -120
INF = float("inf")

NORM_FAMILIES = ("gauss", "outlier", "tiny", "offset", "rowscale")
NORM_H = (8, 136, 2048, 2056, 4096, 4104, 8192)
TIMM_H = (16, 136, 2048, 2056, 4096, 4104, 8192)
NORM_ROWS = (1, 5)
NORM_EPS = 1e-5
APPLY_T_SHAPES = ((136, 2056), (8, 4104))
BWD_SHAPES = ((1, 136), (37, 4096), (37, 4104), (37, 8192), (511, 136), (512, 136), (513, 136), (1061, 2056), (1536, 136))
BWD_BLOCK_CAP = 512

COLSUM_ROWS = (1, 255, 256, 513, 16383, 16384, 16640)
COLSUM_N = (1, 7, 40, 64, 72, 200)
COLSUM_N_LARGE = (7, 40)
COLSUM_LAYOUTS = ("contig", "aligned_slice", "odd_slice", "ld_odd")
SUMSQ_N = (1, 2, 3, 4, 5, 1023, 1024, 1027, 100003, 2097152, 2097155, 4195333)
PARTIALS_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)
CLIP_SUMSQ = (0.0, 1e-12, 0.25, 1.0, 4.0, 1e12)

ACT_NAMES = ("gelu_erf", "gelu_tanh", "relu", "silu")
TAIL_N = (1, 7, 8, 9, 1003)
SWIGLU_UP = (1.0, -3.0, 2.0 ** -10, 300.0)
SWIGLU_DACT = (1.0, -0.37)
SWIGLU_T_SHAPES = ((8, 8), (40, 136), (200, 2056))
ROPE_D = (16, 64, 128)
ROPE_S = (1, 37)

CE_ROWS = 6
CE_NCOLS = (1, 3, 4, 5, 255, 256, 257, 1000, 32064)
CE_FAMILIES = ("gauss", "wide", "peaked", "flat", "shifted", "masked")
INFONCE_SHAPES = ((1, 4), (3, 4), (100, 128), (7, 9), (130, 130))
INFONCE_SCALES = (4.0, 30.0)
L2_NCOLS = (8, 136, 520, 4096)
L2_ROWS = (1, 3, 4, 5, 101)
L2_EPS = 1e-12

ADAMW_FAMILIES = ("unit", "tiny", "huge", "zero")
ADAMW_STEPS = (1, 2, 3, 7, 1000, 100000)
ADAMW_N = (1, 3, 4, 5, 4095, 4096, 4100, 262147)
# The 16-byte kernel runs only when n_decay % 4 == 0 (mla_adamw_step passes n_decay = n): of ADAMW_N, n in {4, 4096, 4100}; the other
# sizes reach it through mla_adamw_step_groups with n_decay = n - n % 4, which leaves a scalar tail.
ADAMW_N_CAPPED = 8388608 + 4100           # n / 4 > 2097152: the grid is capped at 8192 blocks, each walks a chunk of 1024 groups once
ADAMW_N_BIG = 33554432 + 4100 + 3         # n / 4 > 8192 x 1024: a block takes a second trip of its loop; + 3 = a scalar tail
ADAMW_WD = (0.0, 0.01)
ADAMW_LAYOUTS = ("aligned", "offset1", "p16_offset2", "no_p16")
ADAMW_HYPER = dict(lr=2e-5, beta1=0.9, beta2=0.999, eps=1e-8)
ADAMW_GS = 0.37


def _gen(*key):
    h = 0
    for k in key:
        for ch in str(k):
            h = (h * 131 + ord(ch)) % 2147483647
    return torch.Generator().manual_seed(h)


def f32v(x):
    """The value a float argument has once the C ABI carried it as `float`."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ bounds
def _ratio(err, bound):
    """err / bound element-wise; 0 where err is exactly 0 (a zero bound then demands exactness), inf for a NaN."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isnan(r), torch.full_like(r, INF), r)


def bf16_bound(ref64, slack, k=1):
    return k * U16 * (1 + 2.0 ** -6) * ref64.abs() + 4 * slack + FLOOR


def bf16_ratio(got, ref64, slack, k=1):
    """(worst |err| / bound, elements outside) of a bf16 output against the per-element rule."""
    g = got.to(F64)
    err = (g - ref64).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, INF))
    r = _ratio(err, bf16_bound(ref64, slack, k))
    return float(r.max()), int((r > 1).sum())


def scalar_ratio(got, ref64, scale=None):
    """Worst ratio of fp32 per-row scalars to 8 U32 scale. Equal infinities agree."""
    g = got.to(F64)
    scale = ref64.abs() if scale is None else scale
    same_inf = torch.isinf(ref64) & (g == ref64)
    err = torch.where(same_inf, torch.zeros_like(g), (g - ref64).abs())
    err = torch.where(torch.isnan(err), torch.full_like(err, INF), err)
    bound = torch.where(same_inf, torch.ones_like(g), 8 * U32 * scale)
    return float(_ratio(err, bound).max())


def reduction_bound(n, sumabs):
    return (math.ceil(math.log2(max(n, 1))) + 8) * U32 * sumabs


def reduction_ratio(got, ref64, n, sumabs):
    g = got.to(F64)
    err = (g - ref64).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, INF))
    return float(_ratio(err, reduction_bound(n, sumabs)).max())


def mean_ratio(got, x):
    """A row mean (fp32 [rows]) of x [rows, H]. Rows whose sum does not cancel (|sum x| >= sum |x| / 2: the `offset` family) are
    held to the scalar rule 8 U32 |mean|. On the others |mean| is no scale -- on zero-mean rows no fp32 sum is within 8 U32 of what
    is left -- and the mean is held to the reduction rule over its H terms, divided by H."""
    H = x.shape[1]
    xs = x.to(F64)
    tot, sumabs = xs.sum(-1), xs.abs().sum(-1)
    g = got.to(F64) * H
    err = (g - tot).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, INF))
    bound = torch.where(tot.abs() >= 0.5 * sumabs, 8 * U32 * tot.abs(), reduction_bound(H, sumabs))
    return float(_ratio(err, bound).max())


def rel_ratio(got, ref64, units):
    """|got - ref64| / (units U32 |ref64|)."""
    g = got.to(F64)
    err = (g - ref64).abs()
    return float(_ratio(torch.where(torch.isfinite(g), err, torch.full_like(err, INF)), units * U32 * ref64.abs()).max())


def bits_equal(a, b):
    """Bit for bit, a NaN matching any NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        both_nan = torch.isnan(a) & torch.isnan(b)
        return bool(((a.contiguous().view(it) == b.contiguous().view(it)) | both_nan).all())
    return bool(torch.equal(a, b))


def sentinel_ratio(terms, bound, idx):
    """Smallest weight of a sentinel element over the bound: terms [n] or [n, cols] (columns are taken together: the move of the
    result vector in the 1-norm over the 1-norm of its bound), bound scalar or [cols], idx the sentinel rows."""
    t = terms.to(F64).abs()
    b = torch.as_tensor(bound, dtype=F64)
    if t.dim() == 2:
        t, b = t.sum(1), b.sum()
    return float((t[list(idx)] / b).min())


# ------------------------------------------------------------------------------------------------ row sums in the kernels' order
def block_sum32(v):
    """fp32 sum of every row of v [rows, H] (H % 8 == 0, H <= 8192) in the order of the 256-lane row kernels: lane t adds the elements
    of its 16-byte chunks t, t + 256, ... in turn, a pairwise tree joins the 64 lanes of a wave, the four waves are added in turn."""
    rows, H = v.shape
    nch = H // 8
    pad = torch.zeros(rows, 1024, 8, dtype=F32, device=v.device)
    pad[:, :nch] = v.to(F32).view(rows, nch, 8)
    pad = pad.view(rows, 4, 256, 8)
    acc = torch.zeros(rows, 256, dtype=F32, device=v.device)
    for c in range(4):
        for j in range(8):
            acc = acc + pad[:, c, :, j]
    a = acc.view(rows, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a[..., :o] + a[..., o:2 * o]
    a = a[..., 0]
    return ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]


def wave_sum32(v):
    """Same for the one-wave-per-row kernels (L2 normalisation): lane t walks chunks t, t + 64, ..., then the pairwise tree."""
    rows, H = v.shape
    nch = H // 8
    per = (nch + 63) // 64
    pad = torch.zeros(rows, per * 64, 8, dtype=F32, device=v.device)
    pad[:, :nch] = v.to(F32).view(rows, nch, 8)
    pad = pad.view(rows, per, 64, 8)
    a = torch.zeros(rows, 64, dtype=F32, device=v.device)
    for c in range(per):
        for j in range(8):
            a = a + pad[:, c, :, j]
    for o in (32, 16, 8, 4, 2, 1):
        a = a[..., :o] + a[..., o:2 * o]
    return a[..., 0]


def _rowsum(v, dt, order=block_sum32):
    return v.sum(-1) if dt == F64 else order(v)


def _bf_round(v):
    """v rounded to bf16, in v's dtype (the two roundings the timm RmsNorm puts on its variance)."""
    return v.to(F32).to(BF).to(v.dtype)


def row_slack(a32, b64):
    return (a32.to(F64) - b64).abs().amax(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------ norms
def norm_rows(family, rows, H, tag=""):
    g = _gen("norm", family, rows, H, tag)
    x = torch.randn(rows, H, generator=g)
    if family == "outlier":
        x[:, H - 1] = 2500.0
        x[:, 0] = -900.0
        if H > 2048:
            x[:, 2047] = 300.0
            x[:, 2048] = -300.0
    elif family == "tiny":
        x = x * 1e-4
    elif family == "offset":
        x = x * 0.05 + 7.0
    elif family == "rowscale":
        x = x * torch.logspace(-3, 3, rows)[:, None]
    elif family != "gauss":
        raise ValueError(family)
    return x.to(BF)


def norm_weight(H, tag="w"):
    return (1.0 + 0.1 * torch.randn(H, generator=_gen("normw", H, tag))).to(BF)


def norm_bias(H):
    return (0.1 * torch.randn(H, generator=_gen("normb", H))).to(BF)


def bwd_sentinel_rows(rows):
    return sorted({0, rows - 1} | {r for r in (BWD_BLOCK_CAP - 1, BWD_BLOCK_CAP) if r < rows})


def norm_dy(rows, H, tag="dy"):
    """Upstream gradient of the backward cases: N(0,1), the rows where the 512-block walk starts, wraps and ends x 8, the last x 64."""
    dy = torch.randn(rows, H, generator=_gen("normdy", rows, H, tag))
    for r in bwd_sentinel_rows(rows):
        dy[r] *= 8.0
    dy[rows - 1] *= 8.0
    return dy.to(BF)


def rmsnorm_ref(x, w, eps, dt, divisor=None, skip_last_chunk=False):
    """(y, xg, rstd): y = w * (x * rstd), xg = x * w, rstd = (mean(x^2) + eps)^-1/2. divisor / skip_last_chunk build the wrong
    emulations of the host test."""
    H = x.shape[1]
    xs, ws = x.to(dt), w.to(dt)
    sq = xs * xs
    if skip_last_chunk:
        sq = sq.clone()
        sq[:, H - 8:] = 0
    ms = _rowsum(sq, dt) / (divisor or H)
    rstd = 1.0 / torch.sqrt(ms + torch.tensor(f32v(eps), dtype=dt, device=x.device))
    return ws * (xs * rstd[:, None]), xs * ws, rstd


def layernorm_ref(x, w, b, eps, dt):
    H = x.shape[1]
    xs = x.to(dt)
    mean = _rowsum(xs, dt) / H
    d = xs - mean[:, None]
    var = _rowsum(d * d, dt) / H
    rstd = 1.0 / torch.sqrt(var + torch.tensor(f32v(eps), dtype=dt, device=x.device))
    return d * rstd[:, None] * w.to(dt) + b.to(dt)


def timm_ref(x, w, eps, dt):
    """(y, mean, rstd, var, var_eps): torch.var based timm 0.9 RmsNorm; var and var + eps are rounded to bf16 by design, the
    unrounded values come back for the boundary check."""
    H = x.shape[1]
    xs = x.to(dt)
    mean = _rowsum(xs, dt) / H
    d = xs - mean[:, None]
    var = _rowsum(d * d, dt) / (H - 1)
    var_eps = _bf_round(var) + torch.tensor(f32v(eps), dtype=dt, device=x.device)
    rstd = 1.0 / torch.sqrt(_bf_round(var_eps))
    return xs * rstd[:, None] * w.to(dt), mean, rstd, var, var_eps


def bf16_boundary_distance(v):
    """Relative distance of every v (fp64, > 0) to the nearest point where the rounding to bf16 changes its result."""
    b = v.to(F32).to(BF).to(F64)
    ulp = torch.exp2(torch.floor(torch.log2(v.abs())) - 7)
    return torch.minimum((v - (b + ulp / 2)).abs(), (v - (b - ulp / 2)).abs()) / v.abs()


def rmsnorm_bwd_ref(dy, x, w, rstd32, dres, dt):
    """(dx, dw terms [rows, H]): dx = dres + rstd (dy w - n mean(dy w n)), n = x rstd; dw = sum over rows of dy n."""
    H = x.shape[1]
    rs = rstd32.to(dt)[:, None]
    n = x.to(dt) * rs
    dn = dy.to(dt) * w.to(dt)
    dot = (_rowsum(dn * n, dt) / H)[:, None]
    dx = rs * (dn - n * dot)
    if dres is not None:
        dx = dres.to(dt) + dx
    return dx, dy.to(dt) * n


def timm_bwd_ref(dy, x, w, mean32, rstd32, dt):
    H = x.shape[1]
    rs, mu = rstd32.to(dt)[:, None], mean32.to(dt)[:, None]
    xs = x.to(dt)
    dn = dy.to(dt) * w.to(dt)
    dot = _rowsum(dn * xs, dt)[:, None] * rs * rs * rs / (H - 1)
    return rs * dn - (xs - mu) * dot, dy.to(dt) * xs * rs


def dw_check(got, terms64, base64=None):
    """Ratio of a weight gradient (fp32 [H]) to the reduction rule over the rows (+ the buffer it was accumulated onto)."""
    ref, sumabs, n = terms64.sum(0), terms64.abs().sum(0), terms64.shape[0]
    if base64 is not None:
        ref, sumabs, n = ref + base64, sumabs + base64.abs(), n + 1
    return reduction_ratio(got, ref, n, sumabs)


# ------------------------------------------------------------------------------------------------ reductions
def colsum_blocks(rows):
    return min(max(rows // 256, 1), 64)


def colsum_sentinel_rows(rows):
    rs = colsum_blocks(rows)
    per = (rows + rs - 1) // rs
    out = set()
    for b in range(rs):
        r0, r1 = b * per, min(b * per + per, rows)
        if r0 < r1:
            out |= {r0, r1 - 1}
    return sorted(out | {rows - 1})


def colsum_input(rows, N):
    x = torch.randn(rows, N, generator=_gen("colsum", rows, N))
    x = x + 0.25 * torch.sign(x)                      # no element near zero: every sentinel row carries weight in every column
    for r in colsum_sentinel_rows(rows):
        x[r] *= 8.0
    x[rows - 1] *= 8.0
    return x.to(BF)


def place_2d(x, layout, device):
    """x in one of the column layouts, the rest of the buffer NaN: contig; aligned_slice = columns 8.. of a buffer 24 wider;
    odd_slice = columns 3.. of the same; ld_odd = the leading columns of a buffer 5 wider."""
    rows, N = x.shape
    if layout == "contig":
        return x.to(device).contiguous()
    wide, off = {"aligned_slice": (N + 24, 8), "odd_slice": (N + 24, 3), "ld_odd": (N + 5, 0)}[layout]
    buf = torch.full((rows, wide), float("nan"), dtype=x.dtype, device=device)
    view = buf[:, off:off + N]
    view.copy_(x)
    return view


def colsum_is_vec(view):
    return view.shape[1] % 8 == 0 and view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0


def flat_input(n, tag):
    """fp32 [n]: N(0,1) pushed away from zero, the last three elements 64, -96, 80."""
    x = torch.randn(n, generator=_gen("flat", tag, n))
    x = x + 0.25 * torch.sign(x)
    s = torch.tensor([64.0, -96.0, 80.0])
    k = min(3, n)
    if k:
        x[n - k:] = s[3 - k:]
    return x


def clip_ref(sumsq, max_norm):
    """(coef, norm) of torch's clip_grad_norm_ in fp64 from the fp32 input and the fp32 constant 1e-6."""
    nrm = math.sqrt(f32v(sumsq))
    return min(1.0, f32v(max_norm) / (nrm + f32v(1e-6))), nrm


# ------------------------------------------------------------------------------------------------ element-wise
def all_bf16():
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)


@functools.lru_cache(maxsize=None)
def unary_inputs():
    """Every finite bf16 bit pattern with |x| <= 65536 (both zeros and the sub-normals included)."""
    a = all_bf16()
    keep = torch.isfinite(a) & (a.float().abs() <= 65536.0)
    return a[keep].clone()


_K0 = math.sqrt(2.0 / math.pi)
_K1 = 0.044715
_RS2 = math.sqrt(0.5)
_RS2PI = 1.0 / math.sqrt(2.0 * math.pi)


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def act_ref(kind, x, dt):
    x = x.to(dt)
    if kind == 0:
        return 0.5 * x * (1.0 + torch.erf(x * _RS2))
    if kind == 1:
        return 0.5 * x * (1.0 + torch.tanh(_K0 * (x + _K1 * x * x * x)))
    if kind == 2:
        return torch.where(x > 0, x, torch.zeros_like(x))
    return x * _sigmoid(x)


def act_dref(kind, x, dt):
    x = x.to(dt)
    if kind == 0:
        return 0.5 * (1.0 + torch.erf(x * _RS2)) + x * _RS2PI * torch.exp(-0.5 * x * x)
    if kind == 1:
        t = torch.tanh(_K0 * (x + _K1 * x * x * x))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * x * x)
    if kind == 2:
        return (x > 0).to(dt)
    s = _sigmoid(x)
    return s + x * s * (1.0 - s)


def cast_inputs():
    """fp32: for every finite bf16 value b -- b, the tie b + ulp / 2, and the tie -+ one fp32 ulp."""
    a = all_bf16()
    bits = a[torch.isfinite(a)].view(torch.int16).to(torch.int32) << 16
    return torch.cat([bits, bits | 0x8000, (bits | 0x8000) - 1, (bits | 0x8000) + 1]).view(F32)


def add_tie_inputs():
    """(a, b) bf16: a over every normal value with a biased exponent in [16, 240], b = -+ half an ulp of a (the sum is an exact tie),
    the next bf16 value above it and the one below."""
    a = all_bf16()
    e = (a.view(torch.int16).to(torch.int32) >> 7) & 0xFF
    a = a[(e >= 16) & (e <= 240)]
    e = (a.view(torch.int16).to(torch.int32) >> 7) & 0xFF
    half = (e - 8) << 7
    outs_a, outs_b = [], []
    for bits in (half, half + 1, half - 1):
        for sign in (0, 0x8000):
            outs_a.append(a)
            b = bits | sign
            outs_b.append(torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(BF))
    return torch.cat(outs_a), torch.cat(outs_b)


def swiglu_inputs():
    """(gu [4, 2I], I): the gate runs over unary_inputs() (zero-padded to a multiple of 8), one row per `up` value."""
    g = unary_inputs()
    I = (g.numel() + 7) // 8 * 8
    gu = torch.zeros(len(SWIGLU_UP), 2 * I, dtype=BF)
    gu[:, :g.numel()] = g
    for r, u in enumerate(SWIGLU_UP):
        gu[r, I:] = u
    return gu, I


def sigmoid_flushed(g):
    """Gates whose sigmoid is below 2^-126 (g < -87.3): the SwiGLU kernels take it from v_rcp_f32, which returns 0 there -- the
    documented limit of mla_swiglu_* (include/mla_hip.h). The expected outputs are then 0, not silu(g) * up ~ 87 x 2^-126 x up."""
    return _sigmoid(g.to(F64)) < 2.0 ** -126


def flush_expected(ref, flushed):
    """ref with the flushed elements replaced by the documented 0 (use on the fp64 reference and on the slack alike)."""
    return torch.where(flushed, torch.zeros_like(ref), ref)


def swiglu_ref(gu, dt):
    I = gu.shape[1] // 2
    g, u = gu[:, :I].to(dt), gu[:, I:].to(dt)
    return g * _sigmoid(g) * u


def swiglu_bwd_ref(dact, gu, dt):
    """(dgu [rows, 2I], act)."""
    I = gu.shape[1] // 2
    g, u, d = gu[:, :I].to(dt), gu[:, I:].to(dt), dact.to(dt)
    s = _sigmoid(g)
    sl = g * s
    return torch.cat([d * u * (s + sl * (1.0 - s)), d * sl], 1), sl * u


def rope_tables(S, D):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = torch.arange(S, dtype=F64)[:, None] * inv[None, :]
    return torch.cos(ang).to(F32), torch.sin(ang).to(F32)


def rope_layout(D):
    """(q_off, k_off, ld, nheads) of the RoPE cases: two heads inside a wider buffer."""
    q_off, k_off = 8, 8 + 2 * D + 16
    return q_off, k_off, k_off + 2 * D + 8, 2


def rope_input(S, D):
    tokens = 2 * S + 3
    return (torch.randn(tokens, rope_layout(D)[2], generator=_gen("rope", S, D)) * 2.0).to(BF)


def rope_ref(buf, cos, sin, S, D, dt, backward=False):
    """The rotated buffer without the output rounding (columns outside q and k unchanged); position = token % S."""
    q_off, k_off, ld, nh = rope_layout(D)
    out = buf.to(dt).clone()
    pos = torch.arange(buf.shape[0], device=buf.device) % S
    c, s = cos.to(dt)[pos], sin.to(dt)[pos] * (-1.0 if backward else 1.0)
    half = D // 2
    for off in (q_off, k_off):
        for h in range(nh):
            a = buf[:, off + h * D: off + h * D + half].to(dt)
            b = buf[:, off + h * D + half: off + (h + 1) * D].to(dt)
            out[:, off + h * D: off + h * D + half] = a * c - b * s
            out[:, off + h * D + half: off + (h + 1) * D] = b * c + a * s
    return out


def rope_mask(D):
    q_off, k_off, ld, nh = rope_layout(D)
    m = torch.zeros(ld, dtype=torch.bool)
    m[q_off:q_off + nh * D] = True
    m[k_off:k_off + nh * D] = True
    return m


# ------------------------------------------------------------------------------------------------ losses
def ce_lds(ncols):
    return (ncols,) if ncols == 32064 else (ncols, ncols + 1, ncols + 8)


def ce_logits(family, ncols, rows=CE_ROWS):
    g = _gen("ce", family, ncols)
    x = torch.randn(rows, ncols, generator=g)
    if family == "gauss":
        x = x * 3.0
    elif family == "wide":
        x = torch.rand(rows, ncols, generator=g) * 120.0 - 60.0
    elif family == "peaked":
        for r in range(rows):
            x[r, (7 * r + 3) % ncols] += 80.0
    elif family == "flat":
        x = (torch.arange(rows, dtype=F32) - 2.5)[:, None].expand(rows, ncols).clone()
    elif family == "shifted":
        x = x + 3000.0
    elif family == "masked":
        x = x * 3.0
        k = min(300, ncols - 1)
        scattered = torch.rand(rows, ncols, generator=g) < 0.1
        scattered[:, ncols - 1] = False
        x[scattered] = -INF
        x[:, :k] = -INF
    else:
        raise ValueError(family)
    return x


def ce_labels(family, ncols, rows=CE_ROWS):
    """valid, -100, >= ncols, -7, valid, valid. `masked` keeps its valid labels on the last column, which is finite."""
    lab = torch.tensor([(11 * r + 5) % ncols for r in range(rows)], dtype=torch.long)
    if family == "masked":
        lab[:] = ncols - 1
    lab[1], lab[2], lab[3] = -100, ncols + (0 if ncols % 2 else 5), -7
    return lab


def ce_ref(logits, labels, dt):
    """(lse, loss, loss scale) from logits [rows, ncols] as the kernel reads them (already in their storage type)."""
    x = logits.to(dt)
    rows, ncols = x.shape
    lse = torch.logsumexp(x, -1)
    lab = torch.arange(rows, device=x.device) if labels is None else labels.to(x.device)
    valid = (lab >= 0) & (lab < ncols) & (lab != -100)
    pick = x[torch.arange(rows, device=x.device), lab.clamp(0, ncols - 1)]
    zero = torch.zeros_like(lse)
    return lse, torch.where(valid, lse - pick, zero), torch.where(valid, lse.abs() + pick.abs(), zero)


def lse_scale(lse64):
    return lse64.abs().clamp(min=1.0)


def infonce_case(M, Mp, scale):
    """(L [Mp, Mp] fp32, rlse, clse [Mp] fp32, gscale [1]); everything outside the leading M is NaN."""
    g = _gen("infonce", M, Mp, scale)
    a = torch.nn.functional.normalize(torch.randn(M, 16, generator=g), dim=-1)
    b = torch.nn.functional.normalize(a + 0.5 * torch.randn(M, 16, generator=g), dim=-1)
    L = torch.full((Mp, Mp), float("nan"))
    L[:M, :M] = scale * (a @ b.T)
    rl, cl = torch.full((Mp,), float("nan")), torch.full((Mp,), float("nan"))
    rl[:M] = torch.logsumexp(L[:M, :M].double(), 1).float()
    cl[:M] = torch.logsumexp(L[:M, :M].double(), 0).float()
    return L, rl, cl, torch.tensor([0.7])


def infonce_ref(L, rl, cl, gscale, M, dt):
    Mp = L.shape[0]
    x = L[:M, :M].to(dt)
    gs = gscale.to(dt)[0] / (2.0 * M)
    v = gs * (torch.exp(x - rl[:M].to(dt)[:, None]) + torch.exp(x - cl[:M].to(dt)[None, :])
              - 2.0 * torch.eye(M, dtype=dt, device=L.device))
    out = torch.zeros(Mp, Mp, dtype=dt, device=L.device)
    out[:M, :M] = v
    return out


def l2_rows(rows, ncols):
    """N(0,1) rows; with three rows or more, row 1 is all zero (the eps clamp) and row 2 has magnitude 1e-3."""
    x = torch.randn(rows, ncols, generator=_gen("l2", rows, ncols))
    if rows >= 3:
        x[1] = 0.0
        x[2] *= 1e-3
    return x.to(BF)


def l2_ref(x, eps, dt):
    xs = x.to(dt)
    nrm = torch.sqrt(_rowsum(xs * xs, dt, wave_sum32)).clamp(min=f32v(eps))
    return xs / nrm[:, None], nrm


def l2_bwd_ref(dy, y, norms32, dt):
    ys, ds = y.to(dt), dy.to(dt)
    dot = _rowsum(ys * ds, dt, wave_sum32)[:, None]
    return (ds - ys * dot) / norms32.to(dt)[:, None]


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_state(family, n, tag=0):
    """(p, g, m, v) fp32 [n]: the state one step starts from. Of every four parameters one is exactly 0 and one of magnitude 1e-6
    (zero-initialised weights, biases): next to |p| ~ 1 the update of lr-sized steps is below one rounding of p and its error invisible."""
    gen = _gen("adamw", family, tag)
    p = torch.randn(n, generator=gen)
    k = torch.arange(n) % 4
    p = torch.where(k == 1, torch.zeros(n), torch.where(k == 2, p * 1e-6, p))
    g = torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.1 + 0.9 * torch.rand(n, generator=gen)) ** 2
    s = {"unit": 1.0, "tiny": 1e-9, "huge": 1e4, "zero": 1.0}[family]
    g, m, v = g * s, m * s, v * (s * s)
    if family == "zero":
        g = torch.zeros(n)
    return p, g, m, v


def adamw_ref64(p, g, m, v, step, wd, gs, n_decay=None, lr=2e-5, beta1=0.9, beta2=0.999, eps=1e-8):
    """One AdamW step in fp64 from the fp32 state. Hyper-parameters are rounded to fp32 first, as the ABI carries them; the bias
    corrections are exact. gs = the clip coefficient (None: 1). Returns dict(p, m, v, mabs, U)."""
    lr, b1, b2, eps, wd = (f32v(a) for a in (lr, beta1, beta2, eps, wd))
    gs = 1.0 if gs is None else f32v(gs)
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    gg = g * gs
    m64 = b1 * m + (1.0 - b1) * gg
    v64 = b2 * v + (1.0 - b2) * gg * gg
    den = torch.sqrt(v64) / math.sqrt(bc2) + eps
    decay = torch.full_like(p, 1.0 - lr * wd)
    if n_decay is not None:
        decay[n_decay:] = 1.0
    mabs = (b1 * m).abs() + ((1.0 - b1) * gg).abs()
    return dict(p=p * decay - lr / bc1 * m64 / den, m=m64, v=v64, mabs=mabs, U=lr / bc1 * mabs / den)


def adamw_ratios(p, m, v, ref, p_before):
    """Worst ratios (m, v, p) of one step's outputs to the AdamW rule."""
    def worst(got, want, bound):
        g = got.to(F64)
        err = (g - want).abs()
        err = torch.where(torch.isfinite(g), err, torch.full_like(err, INF))
        return float(_ratio(err, bound).max()) if err.numel() else 0.0
    return (worst(m, ref["m"], 8 * U32 * ref["mabs"]), worst(v, ref["v"], 8 * U32 * ref["v"]),
            worst(p, ref["p"], 2 * U32 * p_before.to(F64).abs() + 8 * U32 * ref["U"]))


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adamw_emul32(p, g, m, v, step, wd, gs, bias="double", use_gs=True, lr=2e-5, beta1=0.9, beta2=0.999, eps=1e-8):
    """The kernel's arithmetic in numpy fp32 (adamw_elem of elementwise.hip, every contraction as written there).
    bias = "double": corrections formed in double and cast once; "float": 1 - powf(beta, step) in fp32, as before this suite.
    use_gs = False ignores the clip coefficient (a wrong emulation)."""
    f = np.float32
    lr, b1, b2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    gs = f(1.0) if (gs is None or not use_gs) else f(gs)
    p, g, m, v = (t.numpy().astype(f) for t in (p, g, m, v))
    if bias == "double":
        bc1, bc2 = f(1.0 - float(b1) ** step), f(1.0 - float(b2) ** step)
    else:
        bc1, bc2 = f(1.0) - np.power(b1, f(step), dtype=f), f(1.0) - np.power(b2, f(step), dtype=f)
    stp, isq, decay = lr / bc1, f(1.0) / np.sqrt(bc2), f(1.0) - lr * wd
    gg = g * gs
    mm = _fma32(np.full_like(m, b1), m, (f(1.0) - b1) * gg)
    vv = _fma32(np.full_like(v, b2), v, ((f(1.0) - b2) * gg) * gg)
    den = _fma32(np.sqrt(vv), np.full_like(vv, isq), np.full_like(vv, eps))
    pp = _fma32(np.full_like(p, -stp), mm / den, p * decay)
    return torch.from_numpy(pp), torch.from_numpy(mm), torch.from_numpy(vv)


def adamw_place(p, g, m, v, layout, device):
    """The four fp32 arrays and the bf16 copy (or None) on `device` in one of ADAMW_LAYOUTS; the bf16 copy starts NaN."""
    n = p.numel()
    off = 1 if layout == "offset1" else 0

    def put(t):
        buf = torch.full((n + 8,), float("nan"), dtype=F32, device=device)
        view = buf[off:off + n]
        view.copy_(t)
        return view
    arrs = [put(t) for t in (p, g, m, v)]
    if layout == "no_p16":
        p16 = None
    else:
        o16 = 2 if layout == "p16_offset2" else (1 if layout == "offset1" else 0)
        p16 = torch.full((n + 8,), float("nan"), dtype=BF, device=device)[o16:o16 + n]
    return arrs, p16


def adamw_all_vector(layout, n, n_decay=None):
    """True when the 16-byte kernel is launched for the case: aligned arrays, n >= 4 and a decay boundary (n itself for
    mla_adamw_step) that does not cut a 16-byte group. It then takes the n // 4 whole groups and the scalar kernel the n % 4 tail;
    in every other case the scalar kernel takes everything."""
    return layout in ("aligned", "no_p16") and n >= 4 and (n if n_decay is None else n_decay) % 4 == 0
