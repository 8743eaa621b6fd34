"""Host-only helpers of tests/test_attention_numerics_gpu.py: input families that put one mechanism of a flash-attention kernel under
load each, two CPU references and per-row error metrics. Nothing here touches the GPU; tests/test_attention_cases_host.py checks it.

Families (head_dim 128, scale 1 / sqrt(128); q, k, v come back as fp32 tensors [B, H, S, 128] whose values are bf16-exact):
  gauss             randn * 0.7                                    the only input the older attention tests use (control)
  peaky             q, k randn * 3                                 near one-hot softmax, probabilities underflow in bf16
  rising            k_j = randn/2 + 0.25 j u, q = randn/2 + 8 u    running maximum rises in EVERY key tile: never a lazy rescale
  falling           the same with -0.25 j u                        maximum fixed in tile 0, alpha == 1 (lazy path) from tile 1 on
  late_spike        gauss + keys 10 u / 20 u in the middle / last tile  a large rescale after many lazy tiles (variant `diag`: the
                                                                   spike keys are causal-edge elements: tile offset 63 and row S - 1)
  one_lane          late_spike, q . u != 0 in ONE row of 32 only   the wave-wide ballot is true because of one lane
  sink              key 0 = 20 u, q += 6 u                         almost all mass on key 0 in every row
  outlier_channels  channels 3 and 77 of q, k, v times 20          massive-activation channels, |score| in the hundreds
  offset            q, k = randn/2 + 60 u                          every score ~ +320 with O(1) spread: max subtraction, lse precision
  const_keys        every key row identical                        softmax exactly uniform: closed forms, dq == 0
  neg_all           q = randn/2 + 48 u, k = randn/2 - 48 u         every score ~ -200: no hidden "max >= 0" assumption
u is a fixed unit vector per head.

References (`allowed` [B, Rq, S] bool says which keys a query row sees; a row that sees nothing is a pad row):
  r64   fp64 attention, gradients by autograd on fp64 leaves. o, lse (natural log, pad rows +inf), dq, dk, dv, and the magnitude sums
        A(.) the row metric divides by.
  rbf   the same mathematics in fp32 with the rounding points a bf16 flash kernel is entitled to: unnormalised p = exp(s - rowmax)
        rounded to bf16 before p V (three forward variants: row sum over the rounded p, over the unrounded p, and the deferred
        maximum of the assembly forward -- see rbf(); the yardstick is the worst of them row by row), o rounded to bf16, delta = rowsum(o_bf16 * dO), backward P recomputed from lse, dS = P (dP - delta) rounded to bf16 before the dQ / dK
        products, P rounded to bf16 before dV, gradients rounded to bf16. Scaled causal softmax attention as in transformers
        modeling_llama.py:371-380. It is the yardstick: a kernel may be k times as far from r64 as rbf is, never a literal bound.

Row metric of a bf16 output X (one token, one head): e_r(X) = ||X_r - R64_r|| / max(A_r, PHI * max_r A_r) with
  A(o)_i  = sum_j p_ij ||v_j||                               A(dv)_j = sum_i p_ij ||dO_i||
  A(dq)_i = c sum_j p_ij (|dP_ij| + |delta_i|) ||k_j||       A(dk)_j = c sum_i p_ij (|dP_ij| + |delta_i|) ||q_i||
(the row's own norm is no usable denominator: dq == 0 in const_keys, most dk / dv rows are ~0 where a few keys take all the mass)."""
import functools
import math

import torch

D = 128
SCALE = 1.0 / math.sqrt(D)
PHI = 1e-3
BF = torch.bfloat16
FAMILIES = ("gauss", "peaky", "rising", "falling", "late_spike", "one_lane", "sink", "outlier_channels", "offset", "const_keys", "neg_all")
TENSORS = ("o", "dq", "dk", "dv")


def _bf(x):
    return x.to(BF).float()


def unit_vectors(H):
    """The fixed unit vector of every head, [H, 128] (not bf16-rounded: only its products with gains are)."""
    g = torch.Generator().manual_seed(4242)
    u = torch.randn(H, D, generator=g, dtype=torch.float64)
    return (u / u.norm(dim=-1, keepdim=True)).float()


def spike_keys(S, variant="tile"):
    """Key positions of late_spike / one_lane: one in the middle key tile, one in the last (tile offset 5; variant `diag`: offset 63 of
    the middle tile and row S - 1, keys that the first query seeing them meets as its own diagonal element)."""
    last = (S - 1) // 64
    mid = last // 2
    if variant == "diag":
        pos = {min(mid * 64 + 63, S - 1), S - 1}
    else:
        pos = {min(mid * 64 + 5, S - 1), min(last * 64 + 5, S - 1)}
    return sorted(pos)


def make_qkv(family, S, H, seed, B=1, variant="tile", gain=None):
    """q, k, v [B, H, S, 128] fp32 holding bf16-exact values. `gain` overrides the family's main gain (offset: b; the spike families and
    sink: the key gain)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda s: torch.randn(B, H, S, D, generator=g) * s
    u = unit_vectors(H)[None, :, None, :]                                  # [1, H, 1, D]
    j = torch.arange(S, dtype=torch.float32)[None, None, :, None]
    if family == "gauss":
        q, k, v = rn(0.7), rn(0.7), rn(0.7)
    elif family == "peaky":
        q, k, v = rn(3.0), rn(3.0), rn(0.7)
    elif family in ("rising", "falling"):
        c = (0.25 if gain is None else gain) * (1 if family == "rising" else -1)
        q, k, v = rn(0.5) + 8.0 * u, rn(0.5) + c * j * u, rn(0.7)
    elif family in ("late_spike", "one_lane"):
        q, k, v = rn(0.7), rn(0.7), rn(0.7)
        if family == "one_lane":
            q = q - (q * u).sum(-1, keepdim=True) * u                      # q . u == 0 (up to bf16) ...
            rows = (torch.arange(S) % 32 == 7).float()[None, None, :, None]
            q = q + 6.0 * u * rows                                         # ... except in one row of every 32
        else:
            q = q + 6.0 * u
        pos = spike_keys(S, variant)
        for n, at in enumerate(pos):                                       # the earlier spike at half the gain: the last one still raises
            k[:, :, at] = (20.0 if gain is None else gain) * (1.0 if n == len(pos) - 1 else 0.5) * u[:, :, 0]
    elif family == "sink":
        q, k, v = rn(0.7) + 6.0 * u, rn(0.7), rn(0.7)
        k[:, :, 0] = (20.0 if gain is None else gain) * u[:, :, 0]
    elif family == "outlier_channels":
        q, k, v = rn(0.7), rn(0.7), rn(0.7)
        for t in (q, k, v):
            t[..., 3] *= 20.0
            t[..., 77] *= 20.0
    elif family == "offset":
        b = 60.0 if gain is None else gain
        q, k, v = rn(0.5) + b * u, rn(0.5) + b * u, rn(0.7)
    elif family == "const_keys":
        q, v = rn(0.7), rn(0.7)
        k = (torch.randn(B, H, 1, D, generator=g) * 0.7).expand(B, H, S, D).clone()
    elif family == "neg_all":
        b = 48.0 if gain is None else gain
        q, k, v = rn(0.5) + b * u, rn(0.5) - b * u, rn(0.7)
    else:
        raise ValueError(family)
    return _bf(q), _bf(k), _bf(v)


def make_spiked(S, H, seed, B=1, positions=(), gain=20.0, q_gain=6.0):
    """gauss with q += q_gain u and the keys at `positions` replaced by gain u: spikes at caller-chosen places (suffix-group cases)."""
    q, k, v = make_qkv("gauss", S, H, seed, B)
    u = unit_vectors(H)[None, :, None, :]
    q = q + q_gain * u
    for at in positions:
        k[:, :, at] = gain * u[:, :, 0]
    return _bf(q), _bf(k), v


def make_dout(B, H, Rq, seed):
    g = torch.Generator().manual_seed(seed + 977)
    return _bf(torch.randn(B, H, Rq, D, generator=g))


def pack_qkv(q, k, v):
    """[B, H, S, D] x 3 -> the packed bf16 buffer [B * S, 3 * H * D] the C-ABI takes."""
    B, H, S, _ = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B * S, H * D) for t in (q, k, v)], 1).to(BF).contiguous()


def rows2d(x):
    """[B, H, R, D] -> [B * R, H * D]"""
    B, H, R, _ = x.shape
    return x.transpose(1, 2).reshape(B * R, H * D)


def heads4d(x2d, B, H):
    """[B * R, H * D] -> [B, H, R, D] (fp64)"""
    return x2d.detach().cpu().double().view(B, -1, H, D).transpose(1, 2)


def allowed_mask(B, S, seqlens=None, groups=None, n_query=None):
    """[B, Rq, S] bool. Causal; seqlens (varlen / flash semantics): query rows at or beyond the length see nothing; groups = (start,
    len) with start an int or one int per sample: rows >= start are suffix groups of `len` rows, a query sees the prefix and its own
    group; n_query: only the LAST n_query rows are queries (the decode form)."""
    idx = torch.arange(S)
    base = idx[None, :] <= idx[:, None]
    out = base[None].repeat(B, 1, 1)
    if groups is not None:
        starts = groups[0] if isinstance(groups[0], (list, tuple)) else [groups[0]] * B
        for b, p in enumerate(starts):
            grp = torch.where(idx >= p, (idx - p) // groups[1], torch.full_like(idx, -1))
            out[b] &= (idx[None, :] < p) | (grp[None, :] == grp[:, None])
    if seqlens is not None:
        for b, n in enumerate(seqlens):
            out[b] &= (idx[:, None] < n) & (idx[None, :] < n)
    if n_query is not None:
        out = out[:, S - n_query:]
    return out


def _qrows(q, allowed):
    return q[:, :, q.shape[2] - allowed.shape[1]:]                          # the queries are the last Rq rows


def r64(q, k, v, dout, allowed):
    """fp64 reference. Returns a dict: o, lse, dq, dk, dv ([B, H, Rq or S, D]; lse [B, H, Rq]) and A_o, A_dq, A_dk, A_dv, valid_q
    [B, Rq], valid_k [B, S] (a key row is valid when some query sees it)."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    ql, kl, vl = _qrows(q, allowed).clone().requires_grad_(True), k.clone().requires_grad_(True), v.clone().requires_grad_(True)
    al = allowed[:, None]
    valid_q = allowed.any(-1)
    s = (ql @ kl.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~al, float("-inf"))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    lsum = e.sum(-1, keepdim=True)
    p = e / torch.where(lsum > 0, lsum, torch.ones_like(lsum))
    o = p @ vl
    lse = torch.where(valid_q[:, None], (m + torch.log(torch.where(lsum > 0, lsum, torch.ones_like(lsum))))[..., 0],
                      torch.full_like(m[..., 0], float("inf")))
    o.backward(dout)
    with torch.no_grad():
        pd, od = p.detach(), o.detach()
        dP = dout @ v.transpose(-1, -2)
        delta = (od * dout).sum(-1, keepdim=True)
        w = pd * (dP.abs() + delta.abs())
        nrm = lambda t: t.norm(dim=-1)
        A = {"o": pd @ nrm(v)[..., None], "dv": pd.transpose(-1, -2) @ nrm(dout)[..., None],
             "dq": SCALE * (w @ nrm(k)[..., None]), "dk": SCALE * (w.transpose(-1, -2) @ nrm(_qrows(q, allowed))[..., None])}
    return {"o": od, "lse": lse.detach(), "dq": ql.grad, "dk": kl.grad, "dv": vl.grad,
            "A_o": A["o"][..., 0], "A_dq": A["dq"][..., 0], "A_dk": A["dk"][..., 0], "A_dv": A["dv"][..., 0],
            "valid_q": valid_q, "valid_k": allowed.any(1)}


FWD_VARIANTS = ("", "_unrounded_sum", "_deferred_max")
DEFER = 8.0 * math.log(2.0)


def rbf(q, k, v, dout, allowed, backward=True):
    """Rounding-model reference (fp32 arithmetic, bf16 rounding points; see the module docstring). Three forward variants, each an
    arrangement a flash kernel of this library documents, keyed by suffix:
      ""                p = exp(s - rowmax) -> bf16, row sum over the ROUNDED p (attention.hip: the MFMA row sum of the 8-wave forward)
      "_unrounded_sum"  the same p, row sum over the unrounded p (infer.hip: attn_chunk_kernel adds the fp32 exponentials)
      "_deferred_max"   the maximum p is taken against moves only when a key tile exceeds it by more than 2^8 (tools/gen_attn_asm.py:41,
                        :210-212, the assembly forward's "deferred maximum, threshold 2^8"), so the unnormalised p reaches 256 and the
                        dominant term of a row is no longer exactly 1 before it is rounded; row sum over the unrounded p (:200-201)
    Returns o<suffix>, lse<suffix> and, when `backward`, dq<suffix>, dk<suffix>, dv<suffix> computed from that variant's o and lse."""
    q, k, v, dout = (t.float() for t in (q, k, v, dout))
    qr = _qrows(q, allowed)
    al = allowed[:, None]
    valid = allowed.any(-1)[:, None, :, None]
    s = ((qr @ k.transpose(-1, -2)) * SCALE).masked_fill(~al, float("-inf"))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    pb = _bf(p)
    # deferred maximum: per row, tile by tile, the subtracted value follows the tile maximum only past the threshold
    S = s.shape[-1]
    ref = torch.empty_like(s)
    run = torch.full_like(m, float("-inf"))
    for t0 in range(0, S, 64):
        mx = s[..., t0:t0 + 64].max(-1, keepdim=True).values
        run = torch.where((mx - run > DEFER) | (torch.isinf(run) & torch.isfinite(mx)), torch.maximum(run, mx), run)
        ref[..., t0:t0 + 64] = torch.where(torch.isfinite(run), run, torch.zeros_like(run))
    pd = _bf(torch.exp(s - ref)) * torch.exp(ref - m)
    out = {}
    for name, pr, lsum in (("", pb, pb.sum(-1, keepdim=True)), ("_unrounded_sum", pb, p.sum(-1, keepdim=True)),
                           ("_deferred_max", pd, p.sum(-1, keepdim=True))):
        safe = torch.where(lsum > 0, lsum, torch.ones_like(lsum))
        out["o" + name] = torch.where(valid, _bf((pr @ v) / safe), torch.zeros_like(qr))
        out["lse" + name] = torch.where(valid[..., 0], (m + torch.log(safe))[..., 0], torch.full_like(m[..., 0], float("inf")))
        if backward:
            delta = (out["o" + name] * dout).sum(-1, keepdim=True)
            P = torch.exp(s - out["lse" + name][..., None]).masked_fill(~al, 0.0)  # pad rows: exp(-inf - inf) = 0
            dS = _bf(P * (dout @ v.transpose(-1, -2) - delta))
            out["dq" + name] = _bf(SCALE * (dS @ k))
            out["dk" + name] = _bf(SCALE * (dS.transpose(-1, -2) @ qr))
            out["dv" + name] = _bf(_bf(P).transpose(-1, -2) @ dout)
    return out


# ------------------------------------------------------------------------------------------------ metrics
def row_err(x, ref, A, phi=PHI):
    """e_r [B, H, R] of x against ref (both [B, H, R, D]) with the magnitude sums A [B, H, R] as denominator, floored at phi * max A."""
    den = torch.clamp(A, min=phi * float(A.max()))
    return (x.double() - ref.double()).norm(dim=-1) / den


def floor_share(A, valid, phi=PHI):
    """Fraction of the valid rows whose A lies under the floor. valid [B, R] -> broadcast over heads."""
    vm = valid[:, None].expand_as(A)
    return float(((A < phi * float(A.max())) & vm).sum()) / max(1, int(vm.sum()))


def tile_ratio(e_x, e_y, valid, res=0.0):
    """Worst ratio over the 64-row tiles of max_r e_x / max(max_r e_y, median e_y over the valid rows of the tensor, res): the yardstick
    side e_y is the reference's own error, a tile where it happens to be exact is held to the tensor's median; res is the row error
    fp32 cannot resolve (resolution()). Returns (ratio, (b, h, tile))."""
    vm = valid[:, None].expand_as(e_x)
    B, H, R = e_x.shape
    med = float(e_y[vm].median()) if vm.any() else 0.0
    pad = (-R) % 64
    tiles = lambda e: torch.nn.functional.pad(torch.where(vm, e, torch.zeros_like(e)), (0, pad)).view(B, H, -1, 64).max(-1).values
    tx, ty = tiles(e_x), torch.clamp(tiles(e_y), min=max(med, res))
    ratio = torch.where(tx > 0, tx / torch.clamp(ty, min=1e-300), torch.zeros_like(tx))
    i = int(ratio.argmax())
    T = ratio.shape[2]
    return float(ratio.max()), (i // (H * T), (i // T) % H, i % T)


def resolution(A, phi=PHI):
    """The row error of 128 elements each off by the smallest normal fp32 number (2^-126), at the floor of the denominator. Below it
    two results are the same as far as fp32 can tell: the GPU's exp2 and its bf16 stores flush denormals to zero, the CPU's keep them
    (falling at S = 2048: gradients of 1e-39 in a tensor whose largest row is 3e3 -- 'errors' of 1.8e-39 against 1.0e-40)."""
    return math.sqrt(D) * 2.0 ** -126 / (phi * float(A.max()))


def fro(x, ref):
    return float((x.double() - ref.double()).norm() / ref.double().norm())


def lse_err(lse, ref):
    """max |lse - ref| per head over the finite (non-pad) rows, [H]; the pad pattern (+inf) must agree exactly."""
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == float("inf")).all()), "pad rows: lse = +inf exactly there"
    d = torch.where(fin, (lse.double() - ref.double()).abs(), torch.zeros_like(ref))
    return d.amax(dim=(0, 2))


def lse_floor(ref):
    """8 fp32 ulps of the largest |lse| per head: the kernels form lse = (s * scale * log2 e) * ln 2 + log(l) in fp32 -- the product
    constant, the scaled maximum, the multiplication back and the final sum each round a value of magnitude |lse| once (<= 4 half-ulp
    .. 1-ulp steps), doubled for the margin the project's yardstick rule uses."""
    fin = torch.isfinite(ref)
    a = torch.where(fin, ref.abs(), torch.zeros_like(ref)).amax(dim=(0, 2))
    return 8 * a * 2.0 ** -23


def qk_identity_gap(q, k, dq, dk, R):
    """(gap, sigma), each [B, H]: gap = |sum dq * q - sum dk * k| / (sum |dq64 * q| + sum |dk64 * k|) per (sample, head) -- scores depend
    on q and k through q k^T only, so the two sums are equal in exact arithmetic. The gap is a SIGNED sum of rounding errors, so one
    yardstick value may happen to lie near zero; sigma is the standard deviation the bf16 rounding of the two outputs alone gives it
    (relative error uniform within 2^-9 per element: 2^-9 / sqrt(3) x the root of the summed squares of the terms)."""
    qs = q[:, :, q.shape[2] - dq.shape[2]:].double()
    a, b = dq.double() * qs, dk.double() * k.double()
    a64, b64 = R["dq"] * qs, R["dk"] * k.double()
    den = a64.abs().sum(dim=(2, 3)) + b64.abs().sum(dim=(2, 3))
    den = torch.clamp(den, min=PHI * float(den.max()))                     # samples of length 0 or 1 (both sums zero): the floor of the
    sigma = 2.0 ** -9 / math.sqrt(3.0) * torch.sqrt((a64 ** 2).sum(dim=(2, 3)) + (b64 ** 2).sum(dim=(2, 3))) / den   # row metric
    sigma = torch.clamp(sigma, min=PHI * 2.0 ** -9)
    return (a.sum(dim=(2, 3)) - b.sum(dim=(2, 3))).abs() / den, sigma


@functools.lru_cache(maxsize=64)
def case(family, S, H, seed, B=1, seqlens=None, groups=None, n_query=None, variant="tile", gain=None, backward=True, spikes=None):
    """One cached case: inputs, mask and both references. seqlens / groups as tuples (hashable). family `spiked`: make_spiked with
    the key positions `spikes`."""
    q, k, v = make_spiked(S, H, seed, B, spikes) if family == "spiked" else make_qkv(family, S, H, seed, B, variant, gain)
    allowed = allowed_mask(B, S, seqlens, groups, n_query)
    Rq = allowed.shape[1]
    dout = make_dout(B, H, Rq, seed)
    return {"q": q, "k": k, "v": v, "dout": dout, "allowed": allowed, "r64": r64(q, k, v, dout, allowed),
            "rbf": rbf(q, k, v, dout, allowed, backward)}


def rbf_row_err(c, name):
    """The yardstick's row error for tensor `name`: the worst of the forward variants, row by row."""
    R, Y = c["r64"], c["rbf"]
    return torch.stack([row_err(Y[name + sfx], R[name], R["A_" + name]) for sfx in FWD_VARIANTS]).amax(0)


def rbf_fro(c, name):
    return max(fro(c["rbf"][name + sfx], c["r64"][name]) for sfx in FWD_VARIANTS)


def rbf_lse_err(c):
    return torch.stack([lse_err(c["rbf"]["lse" + sfx], c["r64"]["lse"]) for sfx in FWD_VARIANTS]).amax(0)


def valid_rows(c, name):
    return c["r64"]["valid_k" if name in ("dk", "dv") else "valid_q"]


def compare(c, got, k_bound, tensors=TENSORS, label=""):
    """Compares kernel outputs got[name] ([B, H, R, D], any float dtype on the CPU) and got['lse'] (optional) with the references of
    case c. Returns (lines, failures): the ratio table rows `label tensor tile-ratio fro-ratio` and the violated bounds."""
    R = c["r64"]
    lines, bad = [], []
    for name in tensors:
        x = got[name].double()
        valid = valid_rows(c, name)
        vm = valid[:, None, :, None].expand_as(x)
        if not bool(torch.isfinite(x).all()):
            bad.append(f"{label} {name}: not finite")
            continue
        if bool((x[~vm] != 0).any()):
            bad.append(f"{label} {name}: pad rows not exactly zero")
        ratio, where = tile_ratio(row_err(x, R[name], R["A_" + name]), rbf_row_err(c, name), valid, resolution(R["A_" + name]))
        # whole-tensor ratio only where the fp64 tensor is not zero (const_keys: dq == 0 up to fp64 rounding -> row bound alone)
        nonzero = float(R[name].norm()) > 1e-9 * float(R["A_" + name].norm())
        fy = rbf_fro(c, name) if nonzero else 0.0
        fr = fro(x, R[name]) / fy if nonzero and fy > 0 else 0.0
        share = floor_share(R["A_" + name], valid)
        lines.append(f"RATIO {label:<44} {name:<3} tile {ratio:6.2f} at b,h,tile={where}  fro {fr:5.2f}  floor-share {100 * share:5.1f}%")
        if ratio > k_bound:
            bad.append(f"{label} {name}: row error {ratio:.2f} x the yardstick's in tile {where} (bound {k_bound})")
        if fr > k_bound:
            bad.append(f"{label} {name}: Frobenius error {fr:.2f} x the yardstick's (bound {k_bound})")
    if "lse" in got:
        eh = lse_err(got["lse"], R["lse"])
        ey = rbf_lse_err(c)
        fl = lse_floor(R["lse"])
        ratio = float((eh / (ey + 1e-300)).max())
        lines.append(f"RATIO {label:<44} lse max|d| {float(eh.max()):.2e} yardstick {float(ey.max()):.2e} ratio {ratio:6.2f} floor {float(fl.max()):.1e}")
        if bool((eh > k_bound * ey + fl).any()):
            bad.append(f"{label} lse: |lse - r64| {eh.tolist()} > {k_bound} x {ey.tolist()} + {fl.tolist()}")
    return lines, bad
