"""GPU: the wide-row FP8 prefill GEMMs (mla_amd/csrc/prefill.hip: mla_gemm_prefill_f8_wide / _qkv_rope / _gateup_swiglu; the contract of
mla_gemm_prefill_f8* for 1 <= M <= 65536 rows, 64- or 128-row tiles chosen by the plan). Modelled on test_prefill_f8_gemm_gpu.py:

1. Exact: integer codes in [-8, 8] with unit scales give integer sums below 2^24 -- the output is bf16(integer product) bit for bit, on
   both row tiles, for one and several K tiles, partial row tiles, split-K with even and uneven slices.
2. Scales: powers of two keep everything exact, so the place of every scale shows in the bits (plain, rope, swiglu; both row tiles).
3. Random data: max-abs error against fp64 over the same codes and scales within twice that of the bf16 compact kernel on the
   dequantised operands, run in slices of at most 1024 rows (the project's margin of a new kernel over the existing one of the same
   contract).
4. Up to 1024 rows the wide entry points write what mla_gemm_prefill_f8* write, bit for bit.
5. Housekeeping: exact workspace size, determinism, strided output, refusals, graph capture.

Row tiles: the five shapes the feature was specified with all plan 64-row tiles (128-row tiles need ceil(M / 128) * (N / 128) >= 768), so
the smallest shapes that plan 128 rows are added: (1025, 11008, 128) -- 9 x 86 = 774 tiles, one K tile -- and (1153, 9856, 384) -- 10 x 77
tiles, the last row tile with ONE valid row, three K tiles (both LDS stages and the wrap). A split on the 128-row tile cannot be planned:
the tile is chosen where its tiles alone reach 3 x 256, beyond the 2 x 256 at which the split rule stops (test_prefill_f8_wide_host.py
proves it over a sweep; the launcher has no reduce launch for that tile); the split cases here run on the 64-row tile."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
GUARD = 4096                                             # bytes behind the workspace's stated size that must stay untouched
SENT = -777.0                                            # exactly representable in bf16

EXACT_SHAPES = [(1025, 128, 128), (1090, 256, 384), (1605, 768, 256), (2049, 256, 4096), (1100, 128, 11008),
                (1025, 11008, 128), (1153, 9856, 384)]
TILE128 = EXACT_SHAPES[5:]


class _Ws:
    """A workspace of exactly the stated size followed by a guard region; filled with a NaN pattern (a partial that is read before it is
    written poisons the output)."""

    def __init__(self, M, N, K, dev, fill=0xFF):
        from mla_amd import hip
        self.need = hip.gemm_prefill_f8_wide_ws_bytes(M, N, K)
        assert self.need == hip.plan_gemm_prefill_f8_wide(M, N, K).ws_bytes
        self.full = torch.full((self.need + GUARD,), fill, dtype=torch.uint8, device=dev)
        self.full[self.need:] = 0xA5
        self.ws = self.full[:self.need] if self.need else None

    def check(self):
        assert bool((self.full[self.need:] == 0xA5).all()), "the guard region behind the workspace was written"


@functools.lru_cache(maxsize=None)
def _int_case(M, N, K):
    """test_prefill_f8_gemm_gpu.py's asymmetric integer operands, computed once per shape; S = the exact integer product."""
    dev = torch.device("cuda:0")
    xi = torch.randint(-8, 9, (M, K), generator=torch.Generator().manual_seed(1000 + M + K))
    wi = torch.randint(-6, 7, (N, K), generator=torch.Generator().manual_seed(77 + N + K)) + (torch.arange(N)[:, None] % 5 - 2)
    ri = torch.randint(-64, 65, (M, N), generator=torch.Generator().manual_seed(5 + M + N))
    assert int(wi.abs().max()) <= 8 and 64 * K < 1 << 24
    xq, wq = xi.float().to(F8), wi.float().to(F8)
    assert torch.equal(xq.float(), xi.float()) and torch.equal(wq.float(), wi.float())
    S = xi.double().to(dev) @ wi.double().to(dev).t()
    return xq.to(dev), wq.to(dev), ri.to(BF).to(dev), S


def _ones(n, dev):
    return torch.ones(n, dtype=torch.float32, device=dev)


def _pow2_scales(M, N, dev):
    xs = torch.tensor([2.0 ** -(m % 5) for m in range(M)], dtype=torch.float32, device=dev)
    ws = torch.tensor([2.0 ** -(n % 7) for n in range(N)], dtype=torch.float32, device=dev)
    return xs, ws


# ------------------------------------------------------------------------------------------------ 1. exact
def test_both_row_tiles_and_split_shapes_occur():
    from mla_amd import hip
    plans = {s: hip.plan_gemm_prefill_f8_wide(*s) for s in EXACT_SHAPES}
    assert {p.tile_m for p in plans.values()} == {64, 128}
    assert all(plans[s].tile_m == 128 and plans[s].split == 1 for s in TILE128)
    assert plans[(2049, 256, 4096)].split == 4 and plans[(2049, 256, 4096)].ws_bytes > 0
    p = plans[(1100, 128, 11008)]
    assert p.split == 8 and 86 % p.split != 0                              # 86 K tiles: the last slice is shorter
    assert all(plans[s].split == 1 for s in EXACT_SHAPES[:3])
    assert all(s[0] % plans[s].tile_m != 0 and s[0] > plans[s].tile_m for s in EXACT_SHAPES)    # a partial row tile, more than one block


@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_integer_codes_give_the_integer_product_bit_for_bit(dev, M, N, K):
    from mla_amd import hip
    xq, wq, r, S = _int_case(M, N, K)
    p = hip.plan_gemm_prefill_f8_wide(M, N, K)
    for res, want in ((None, S), (r, S + r.double())):
        w = _Ws(M, N, K, dev)
        out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        hip.gemm_prefill_f8_wide(xq, _ones(M, dev), wq, _ones(N, dev), out, N, 0, M, residual=res, ws=w.ws)
        want = want.float().to(BF)                                         # integers below 2^24: exact in fp32, ONE rounding to bf16
        bad = int((out.float() != want.float()).sum())
        print(f"exact M {M} N {N} K {K} tile {p.tile_m} split {p.split} residual {res is not None}: {bad} of {M * N} differ")
        assert torch.equal(out, want), f"{bad} of {M * N} elements differ from the integer product"
        w.check()


# ------------------------------------------------------------------------------------------------ 2. scales
@pytest.mark.parametrize("M,N,K", [(2049, 256, 4096), (1153, 9856, 384)])
def test_plain_scales_are_per_row_and_per_column(dev, M, N, K):
    """x_scale[m] = 2^-(m % 5), w_scale[n] = 2^-(n % 7): the output is the unscaled integer product times both, bit for bit -- with and
    without the residual, which is added AFTER the scaling. One split case on 64-row tiles, one case on 128-row tiles."""
    from mla_amd import hip
    xq, wq, r, S = _int_case(M, N, K)
    xs, ws = _pow2_scales(M, N, dev)
    scaled = S * xs.double()[:, None] * ws.double()[None, :]
    for res, want in ((None, scaled), (r, scaled + r.double())):
        w = _Ws(M, N, K, dev)
        out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        hip.gemm_prefill_f8_wide(xq, xs, wq, ws, out, N, 0, M, residual=res, ws=w.ws)
        assert torch.equal(out, want.float().to(BF))
        w.check()


@pytest.mark.parametrize("H,K,tile", [(256, 256, 64), (256, 4096, 64), (2560, 128, 128)])
def test_rope_rotates_scaled_sums_with_the_partners_own_scale(dev, H, K, tile):
    """N = 3 H, rope_cols 2 H, THREE samples of 535 rows into cache slots of a larger sentinel-filled buffer whose batch stride is not
    rows x ld; K = 4096 splits (the rotation then runs in the reduction launch), H = 2560 plans 128-row tiles (13 x 60 = 780 tiles).
    Tables: (cos, sin) = (1, 0) on even positions -- the identity -- and (0, 1) on odd ones: a' = -b, b' = a exactly, where a / b are
    the SCALED sums of channel d / d + 64 -- each with the w_scale of its own column. Row m rotates with table row m % 535. The v columns
    are not rotated."""
    from mla_amd import hip
    S_rows, nb = 535, 3
    N, M = 3 * H, nb * S_rows
    p = hip.plan_gemm_prefill_f8_wide(M, N, K)
    assert p.tile_m == tile and (p.split > 1) == (K == 4096)
    xq, wq, _, S = _int_case(M, N, K)
    xs, ws = _pow2_scales(M, N, dev)
    v = S * xs.double()[:, None] * ws.double()[None, :]
    odd = (torch.arange(S_rows) % 2 == 1)
    cos = torch.where(odd, 0.0, 1.0)[:, None].repeat(1, 64).contiguous().to(dev)
    sin = torch.where(odd, 1.0, 0.0)[:, None].repeat(1, 64).contiguous().to(dev)
    want = v.clone()
    rows = ((torch.arange(M) % S_rows) % 2 == 1).to(dev)
    for h0 in range(0, 2 * H, 128):
        a, b = v[:, h0:h0 + 64], v[:, h0 + 64:h0 + 128]
        want[:, h0:h0 + 64] = torch.where(rows[:, None], -b, a)
        want[:, h0 + 64:h0 + 128] = torch.where(rows[:, None], a, b)
    assert not torch.equal(want[:, :2 * H], v[:, :2 * H])
    w = _Ws(M, N, K, dev)
    S_cap = S_rows + 17
    cache = torch.full((nb, S_cap, N + 8), SENT, dtype=BF, device=dev)
    assert cache.stride(0) != S_rows * cache.stride(1)
    hip.gemm_prefill_f8_wide_qkv_rope(xq, xs, wq, ws, cache, cache.stride(1), cache.stride(0), S_rows, (cos, sin, 2 * H), 128, ws=w.ws)
    got = cache[:, :S_rows, :N].reshape(M, N)
    assert torch.equal(got, want.float().to(BF))
    assert bool((cache[:, S_rows:] == SENT).all()) and bool((cache[:, :, N:] == SENT).all())
    w.check()
    # had the partner been rotated with the column's own scale instead of its own, some element would differ
    wrong = (S[:, 64:128] * xs.double()[:, None] * ws.double()[None, 0:64])
    assert not torch.equal(wrong, v[:, 64:128])


@pytest.mark.parametrize("M,I,K,tile", [(1090, 128, 4096, 64), (1605, 3840, 128, 128)])
def test_swiglu_scales_gate_and_up_with_their_own_rows(dev, M, I, K, tile):
    """The packed [2 I, K] matrix: tile column c < 64 is gate, >= 64 up, each with the w_scale of its own row. Reference: fp64
    silu(g) * u on the scaled integer sums. Bound: twice the max-abs error of hip.gemm_prefill_gateup_swiglu on bf16 copies of the same
    scaled operands (exact copies: powers of two times small integers are bf16 values), run in slices of at most 1024 rows.
    (1090, 128, 4096) takes the split-K path on 64-row tiles, (1605, 3840, 128) 128-row tiles (13 x 60 = 780)."""
    from mla_amd import hip
    p = hip.plan_gemm_prefill_f8_wide(M, 2 * I, K)
    assert p.tile_m == tile and (p.split > 1) == (tile == 64)
    xq, wq, _, S = _int_case(M, 2 * I, K)
    xs, ws = _pow2_scales(M, 2 * I, dev)
    y = S * xs.double()[:, None] * ws.double()[None, :]
    ref = torch.nn.functional.silu(y[:, :I]) * y[:, I:]
    xb, wb = (xq.float() * xs[:, None]).to(BF), (wq.float() * ws[:, None]).to(BF)
    assert torch.equal(xb.double() @ wb.double().t(), y)
    old = torch.empty((M, I), dtype=BF, device=dev)
    for m0 in range(0, M, 1024):
        rows = min(1024, M - m0)
        hip.gemm_prefill_gateup_swiglu(xb[m0:m0 + rows], wb, old[m0:m0 + rows],
                                       ws=torch.empty(max(hip.gemm_prefill_ws_bytes(rows, 2 * I, K), 16), dtype=torch.uint8, device=dev))
    e_old = float((old.double() - ref).abs().max())
    w = _Ws(M, 2 * I, K, dev)
    buf = torch.full((M + 2, I + 8), SENT, dtype=BF, device=dev)
    hip.gemm_prefill_f8_wide_gateup_swiglu(xq, xs, wq, ws, buf, ws=w.ws)
    act = buf[:M, :I]
    assert torch.isfinite(act.float()).all()
    e_new = float((act.double() - ref).abs().max())
    print(f"swiglu M {M} I {I} K {K} tile {p.tile_m} split {p.split}: e_new {e_new:.4e} e_old {e_old:.4e}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert bool((buf[M:] == SENT).all()) and bool((buf[:, I:] == SENT).all())
    w.check()
    buf2 = torch.full_like(buf, SENT)
    hip.gemm_prefill_f8_wide_gateup_swiglu(xq, xs, wq, ws, buf2, ws=_Ws(M, 2 * I, K, dev, 0x7F).ws)
    assert torch.equal(buf, buf2)


# ------------------------------------------------------------------------------------------------ 3. random data
@functools.lru_cache(maxsize=None)
def _rand_case(M, N, K):
    """Random operands quantised by the project's quantiser, the fp64 reference over the same codes and scales, and e_old = the error of
    the bf16 compact kernel on the dequantised operands, run in slices of at most 1024 rows."""
    from mla_amd import hip
    dev = torch.device("cuda:0")

    def rand(shape, seed, scale):
        g = torch.Generator(device=dev).manual_seed(seed)
        return (torch.randn(*shape, generator=g, device=dev) * scale).to(BF)
    x, W, r = rand((M, K), 3 * M + K, 0.5), rand((N, K), N + K, 0.05), rand((M, N), M + N, 1.0)
    (xq, xs), (wq, ws) = hip.quant_fp8_rows(x), hip.quant_fp8_rows(W)
    ref = (xq.float().double() @ wq.float().double().t()) * xs.double()[:, None] * ws.double()[None, :]
    xb, wb = (xq.float() * xs[:, None]).to(BF), (wq.float() * ws[:, None]).to(BF)
    old = torch.empty((M, N), dtype=BF, device=dev)
    for m0 in range(0, M, 1024):
        rows = min(1024, M - m0)
        hip.gemm_prefill(xb[m0:m0 + rows], wb, old[m0:m0 + rows], N, 0, rows,
                         ws=torch.empty(max(hip.gemm_prefill_ws_bytes(rows, N, K), 16), dtype=torch.uint8, device=dev))
    e_old = float((old.double() - xb.double() @ wb.double().t()).abs().max())
    return xq, xs, wq, ws, r, ref, e_old


RANDOM_SHAPES = [(2049, 256, 4096), (1153, 9856, 384)]                    # 64-row tiles with split 4; 128-row tiles


@pytest.mark.parametrize("M,N,K", RANDOM_SHAPES)
def test_random_data_within_twice_the_bf16_compact_kernels_error(dev, M, N, K):
    from mla_amd import hip
    xq, xs, wq, ws, _, ref, e_old = _rand_case(M, N, K)
    p = hip.plan_gemm_prefill_f8_wide(M, N, K)
    w = _Ws(M, N, K, dev)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    hip.gemm_prefill_f8_wide(xq, xs, wq, ws, out, N, 0, M, ws=w.ws)
    assert torch.isfinite(out.float()).all()
    e_new = float((out.double() - ref).abs().max())
    print(f"random M {M} N {N} K {K} tile {p.tile_m} split {p.split}: e_new {e_new:.4e} e_old {e_old:.4e}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    w.check()


# ------------------------------------------------------------------------------------------------ 4. the compact entry points' bits
@pytest.mark.parametrize("M", [545, 1024])
def test_up_to_1024_rows_the_bits_are_the_compact_entry_points(dev, M):
    """Plain (+ residual; N = 256, K = 4096 splits), rope and swiglu: torch.equal with gemm_prefill_f8 / _qkv_rope / _gateup_swiglu."""
    from mla_amd import hip
    N, K = 256, 4096
    xq, xs, wq, ws, r = _rand_case(M, N, K)[:5]
    big = torch.empty(1 << 25, dtype=torch.uint8, device=dev)
    assert hip.plan_gemm_prefill_f8_wide(M, N, K) == hip.plan_gemm_prefill_f8(M, N, K) and hip.plan_gemm_prefill_f8(M, N, K).split > 1
    a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
    hip.gemm_prefill_f8(xq, xs, wq, ws, a, N, 0, M, residual=r, ws=big)
    hip.gemm_prefill_f8_wide(xq, xs, wq, ws, b, N, 0, M, residual=r, ws=big)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    g = torch.Generator(device=dev).manual_seed(11)
    ang = torch.rand(M, 64, generator=g, device=dev) * 6.28
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
    hip.gemm_prefill_f8_qkv_rope(xq, xs, wq, ws, a, N, 0, M, (cos, sin, 128), 128, ws=big)
    hip.gemm_prefill_f8_wide_qkv_rope(xq, xs, wq, ws, b, N, 0, M, (cos, sin, 128), 128, ws=big)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    a, b = (torch.full((M, N // 2), float("nan"), dtype=BF, device=dev) for _ in range(2))
    hip.gemm_prefill_f8_gateup_swiglu(xq, xs, wq, ws, a, ws=big)
    hip.gemm_prefill_f8_wide_gateup_swiglu(xq, xs, wq, ws, b, ws=big)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. housekeeping
@pytest.mark.parametrize("M,N,K", RANDOM_SHAPES)
def test_second_launch_over_another_poison_gives_the_same_bits(dev, M, N, K):
    from mla_amd import hip
    xq, xs, wq, ws, r = _rand_case(M, N, K)[:5]
    outs = []
    for fill in (0xFF, 0x7F):
        w = _Ws(M, N, K, dev, fill=fill)
        out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        hip.gemm_prefill_f8_wide(xq, xs, wq, ws, out, N, 0, M, residual=r, ws=w.ws)
        w.check()
        outs.append(out)
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M,N,K,rpb", [(2049, 256, 4096, 683), (1153, 9856, 384, 1153)])
def test_strided_output_touches_nothing_else(dev, M, N, K, rpb):
    """ldo > N, a batch stride that is not rows x ldo, a column offset: the addressed elements are the dense output bit for bit, every
    other element of the (larger) buffer still holds the sentinel."""
    from mla_amd import hip
    xq, xs, wq, ws, r = _rand_case(M, N, K)[:5]
    w = _Ws(M, N, K, dev)
    dense = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    hip.gemm_prefill_f8_wide(xq, xs, wq, ws, dense, N, 0, M, residual=r, ws=w.ws)
    nb, lead, tail, ld, col = M // rpb, 3, 2, N + 72, 40
    assert nb * rpb == M
    buf = torch.full((nb, lead + rpb + tail, ld), SENT, dtype=BF, device=dev)
    assert buf.stride(0) != rpb * ld
    hip.gemm_prefill_f8_wide(xq, xs, wq, ws, buf[:, lead:], ld, buf.stride(0), rpb, residual=r, out_col=col, ws=w.ws)
    assert torch.equal(buf[:, lead:lead + rpb, col:col + N].reshape(M, N), dense)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, lead:lead + rpb, col:col + N] = False
    assert bool((buf[mask] == SENT).all())
    w.check()


def test_refusals_launch_nothing(dev):
    """M = 65537, K = 192, a workspace one byte short and no workspace where the plan splits return the documented code (-1 ->
    RuntimeError in the binding) in the host-side argument checks; the output keeps its sentinel. The compact entry point still refuses
    1025 rows."""
    from mla_amd import hip

    def codes(M, K):
        return torch.zeros((M, K), dtype=torch.uint8, device=dev).view(F8)
    out = torch.full((2049, 256), SENT, dtype=BF, device=dev)
    big = torch.empty(1 << 25, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="1 <= M <= 65536"):
        hip.gemm_prefill_f8_wide(codes(65537, 128), _ones(65537, dev), codes(256, 128), _ones(256, dev), out, 256, 0, 65537, ws=big)
    with pytest.raises(RuntimeError, match="1 <= M <= 1024"):
        hip.gemm_prefill_f8(codes(1025, 128), _ones(1025, dev), codes(256, 128), _ones(256, dev), out, 256, 0, 1025, ws=big)
    with pytest.raises(RuntimeError, match="K % 128 == 0"):
        hip.gemm_prefill_f8_wide(codes(2049, 192), _ones(2049, dev), codes(256, 192), _ones(256, dev), out, 256, 0, 2049, ws=big)
    need = hip.gemm_prefill_f8_wide_ws_bytes(2049, 256, 4096)
    assert need > 0
    x, W = codes(2049, 4096), codes(256, 4096)
    with pytest.raises(RuntimeError, match="workspace"):
        hip.gemm_prefill_f8_wide(x, _ones(2049, dev), W, _ones(256, dev), out, 256, 0, 2049,
                                 ws=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="workspace"):
        hip.gemm_prefill_f8_wide(x, _ones(2049, dev), W, _ones(256, dev), out, 256, 0, 2049, ws=None)
    with pytest.raises(TypeError, match="float8_e4m3fn"):
        hip.gemm_prefill_f8_wide(x.view(torch.uint8), _ones(2049, dev), W, _ones(256, dev), out, 256, 0, 2049, ws=big)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_graph_capture_replays_both_launches(dev):
    """The split-K pair of launches goes on the given stream only: a captured graph replays bit-identically to the eager call."""
    from mla_amd import hip
    M, N, K = 2049, 256, 4096
    xq, xs, wq, ws, r = _rand_case(M, N, K)[:5]
    w = _Ws(M, N, K, dev)
    assert w.need > 0
    eager = torch.empty((M, N), dtype=BF, device=dev)
    hip.gemm_prefill_f8_wide(xq, xs, wq, ws, eager, N, 0, M, residual=r, ws=w.ws)
    out = torch.empty((M, N), dtype=BF, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.gemm_prefill_f8_wide(xq, xs, wq, ws, out, N, 0, M, residual=r, ws=w.ws)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    w.check()
