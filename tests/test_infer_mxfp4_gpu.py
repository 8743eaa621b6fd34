"""GPU: weight-only MXFP4 for the suffix pass of cached-prefix action sampling -- the quantiser (mla_quant_mxfp4_rows), the five `_w4`
projection entry points and the `suffix_mx` modes of mla_amd/infer.py / MLA.predict_action_diff*.

The format is OCP MXFP4 (e2m1 codes, one e8m0 scale byte per 32 consecutive k of a weight row); its CPU statement is mxfp4_quant /
mxfp4_dequant of tests/test_infer_mxfp4_host.py. The kernels decode a code WITH its scale exactly, so they are the bf16 kernels on the
dequantised matrix up to summation order. Bounds: 4e-3 Frobenius-relative against an fp64 reference over the dequantised weights is the
project's bound for "one bf16 rounding of the fp32 sums" (tests/test_infer_fp8_gpu.py); 3e-2 per chunk / 2e-2 per epsilon are the bounds
of the cached-vs-whole-forward tests for "same function, other rounding". How far "fp4" is from the bf16 chunk on this RANDOM tiny model
is printed, not gated: it says nothing about a trained policy."""
import numpy as np
import pytest
import torch

from conftest import fro_rel
from oracle import recipe
from test_infer_mxfp4_host import GRID, mxfp4_dequant, mxfp4_quant, quant_case

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
SENT = 777.0                                                                 # bf16-exact
MS = [1, 17, 33, 49, 64, 65, 96, 97, 128, 129, 255, 256]                     # tests/test_infer_suffix_w8_gpu.py's: every launch form


def _rand(shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tables(S, dev, D=128, S0=0):
    fr = torch.outer(torch.arange(S0, S).float(), 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))
    return fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)


def _call(kernel, x, q, s, out=None, res=None, **kw):
    """One `_w4` projection of x [M, K] into a dense NaN-filled [M, N] (or `out`)."""
    from mla_amd import hip
    f = {"gemv": hip.gemv_w4, "skinny": hip.gemm_skinny_w4, "suffix": hip.gemm_suffix_w4}[kernel]
    M, N = x.shape[0], q.shape[0]
    if out is None:
        out = torch.full((M, N), float("nan"), dtype=BF, device=x.device)
    f(x, q, s, out, N, 0, M, res, **kw)
    return out


_WEIGHTS = {}


def _quantised(N, K, dev):
    """(codes, scale bytes, fp64 dequantised W on the device) of one deterministic [N, K] matrix: quantised on the device once per shape,
    compared with the CPU statement, shared by every test and left unchanged. The scale rows sit in a padded buffer (row stride K / 32 + 3)."""
    if (N, K) not in _WEIGHTS:
        from mla_amd import hip
        W = _rand((N, K), N + K, 0.05).to(BF)
        s = torch.zeros((N, K // 32 + 3), dtype=U8, device=dev)[:, :K // 32]
        q, s = hip.quant_mxfp4_rows(W.to(dev), s=s)
        q_ref, s_ref = mxfp4_quant(W)
        assert torch.equal(s.cpu(), s_ref) and torch.equal(mxfp4_dequant(q.cpu(), s.cpu()), mxfp4_dequant(q_ref, s_ref))
        _WEIGHTS[(N, K)] = (q, s, mxfp4_dequant(q_ref, s_ref).to(dev))
    return _WEIGHTS[(N, K)]


def _x(M, K, seed, dev, scale=0.5):
    """M rows inside a larger buffer whose rows >= M are NaN: a load beyond the rows of the call shows in the output."""
    buf = torch.full((M + 16, K), float("nan"), dtype=BF, device=dev)
    buf[:M] = _rand((M, K), seed, scale).to(BF).to(dev)
    return buf[:M]


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("case", ["300x512", "7x32", "strided"])
def test_quantiser_is_the_cpu_statement(dev, case):
    from mla_amd import hip
    W = quant_case(case)
    q_ref, s_ref = mxfp4_quant(W)
    Wd = W.to(dev)
    if case == "strided":
        Wd = torch.zeros((40, 768), dtype=BF, device=dev)[3:23, 128:384].copy_(W)
        assert Wd.stride(0) == 768 and not Wd.is_contiguous()
    q, s = hip.quant_mxfp4_rows(Wd)
    q2, s2 = hip.quant_mxfp4_rows(Wd)
    assert torch.equal(q, q2) and torch.equal(s, s2)
    assert torch.equal(s.cpu(), s_ref)                                        # scale bytes exactly
    assert torch.equal(mxfp4_dequant(q.cpu(), s.cpu()), mxfp4_dequant(q_ref, s_ref))        # decoded values: -0 and +0 both pass
    assert not bool((s == 255).any())
    if case == "300x512":
        assert bool((s.cpu()[7] == 127).all()) and not bool(q.cpu()[7].any())
        assert int(s.cpu()[11, 0]) == 130 and float(mxfp4_dequant(q.cpu(), s.cpu())[11, 17]) == 32.0     # 40 / 2^3 = 5: the tie goes to 4


# ------------------------------------------------------------------------------------------------ decode pins the format
@pytest.mark.parametrize("kernel,M", [("gemv", 2), ("skinny", 2), ("suffix", 2), ("suffix", 70)])
def test_decode_of_every_code_and_scale_byte(dev, kernel, M):
    """Row n of W holds code n & 15 in EVERY nibble; the scale bytes of a row's blocks cycle through {2, 100, 127, 140, 252}; one-hot x rows
    (value 1 or 0.5, at even and odd k) pick single products: out = coeff * value(code) * 2^(byte - 127) bit for bit. A swapped nibble
    order cannot show here (both nibbles are equal) -- test_nibble_order_is_low_first pins it; a wrong sign, grid value or scale does."""
    N, K = 32, 160
    code = torch.arange(N) & 15
    q = (code | (code << 4)).to(U8)[:, None].repeat(1, K // 2).contiguous()
    bytes_ = torch.tensor([2, 100, 127, 140, 252])
    s = bytes_[(torch.arange(N)[:, None] + torch.arange(K // 32)[None, :]) % 5].to(U8).contiguous()
    coeff = torch.tensor([1.0, 0.5])[torch.arange(M) % 2]
    cols = (torch.arange(M) * 37 + 3) % K
    x = torch.zeros(M, K)
    x[torch.arange(M), cols] = coeff
    val = torch.tensor(GRID, dtype=torch.float64)[code & 7] * torch.where(code >= 8, -1.0, 1.0).double()
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), s.double() - 127)[:, cols // 32]          # [N, M]
    want = (coeff.double()[:, None] * (val[:, None] * scale).t()).to(BF)
    assert torch.equal(want.double(), coeff.double()[:, None] * (val[:, None] * scale).t())             # every product is a bf16
    out = _call(kernel, x.to(BF).to(dev), q.to(dev), s.to(dev))
    # compared as values: the product of code 8 (-0) is summed with the +0 products of the other k, and (-0) + (+0) = +0
    assert torch.equal(out.cpu().float(), want.float()), (kernel, M)
    assert int((out.cpu().float() != 0).sum()) == M * (N - 4)                 # only codes 0 and 8 (4 of 32 rows) give zeros: no product was flushed


@pytest.mark.parametrize("kernel", ["gemv", "skinny", "suffix"])
def test_nibble_order_is_low_first(dev, kernel):
    """Byte j of a row = element 2 j in the low nibble, 2 j + 1 in the high one: rows whose elements count through the codes, every k
    picked by its own one-hot x row."""
    N, K = 16, 64
    elem = (torch.arange(K)[None, :] + torch.arange(N)[:, None]) % 16                                    # W[n, k] holds code (k + n) % 16
    q = (elem[:, 0::2] | (elem[:, 1::2] << 4)).to(U8).contiguous()
    s = torch.full((N, K // 32), 127, dtype=U8)
    want_full = mxfp4_dequant(q, s)                                           # [N, K]
    for k0 in range(0, K, 8):
        x = torch.zeros(8, K)
        x[torch.arange(8), k0 + torch.arange(8)] = 1.0
        out = _call(kernel, x.to(BF).to(dev), q.to(dev), s.to(dev))
        assert torch.equal(out.double().cpu(), want_full[:, k0:k0 + 8].t()), (kernel, k0)


# ------------------------------------------------------------------------------------------------ exact sums
@pytest.mark.parametrize("kernel,M", [("gemv", 3), ("skinny", 17), ("suffix", 65)])
def test_integer_operands_sum_exactly(dev, kernel, M):
    """x integers in [-4, 4], codes random over all 16 values, scale bytes in {126, 127, 128}, K = 512: every product is a multiple of
    0.25 and every partial sum stays far below 2^24 quarter-units, so the fp32 sum is exact in any order: out == bf16(exact sum)."""
    N, K = 200, 512
    g = torch.Generator().manual_seed(17)
    q = torch.randint(0, 256, (N, K // 2), generator=g).to(U8)
    s = torch.randint(126, 129, (N, K // 32), generator=g).to(U8)
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    want = (x @ mxfp4_dequant(q, s).t())
    assert float(want.abs().max()) * 4 < 2 ** 24 and float((want * 4 - (want * 4).round()).abs().max()) == 0
    out = _call(kernel, x.to(BF).to(dev), q.to(dev), s.to(dev))
    assert torch.equal(out.cpu().view(torch.int16), want.to(BF).view(torch.int16))


# ------------------------------------------------------------------------------------------------ projections vs fp64
def _parity_case(dev, kernel, M, N, K, res):
    q, s, Wd = _quantised(N, K, dev)
    x = _x(M, K, M * 1000 + N, dev)
    r = _rand((M, N), M + N, 1.0).to(BF).to(dev) if res else None
    want = x.double() @ Wd.t() + (r.double() if res else 0)
    a, b = _call(kernel, x, q, s, res=r), _call(kernel, x, q, s, res=r)
    assert torch.isfinite(a.float()).all()
    e = fro_rel(a, want)
    print(f"w4 {kernel} M {M} N {N} K {K} res {res}: fro_rel vs fp64 {e:.3e}")
    assert e < 4e-3                                                           # one bf16 rounding of the fp32 sums
    assert torch.equal(a, b)


@pytest.mark.parametrize("K", [32, 96, 512])
@pytest.mark.parametrize("N", [7, 256, 520])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemv_w4_matches_fp64_reference(dev, M, N, K):
    _parity_case(dev, "gemv", M, N, K, res=(M + N + K) % 2 == 1)
    _parity_case(dev, "gemv", M, N, K, res=(M + N + K) % 2 == 0)


@pytest.mark.parametrize("res", [False, True])
def test_gemv_w4_matches_fp64_reference_at_the_7b_down_projection(dev, res):
    _parity_case(dev, "gemv", 5, 1000, 11008, res)


@pytest.mark.parametrize("N,K", [(96, 32), (520, 4128), (1000, 11008)])
@pytest.mark.parametrize("M", [1, 9, 16, 17, 33, 64])
def test_gemm_skinny_w4_matches_fp64_reference(dev, M, N, K):
    """K = 32 is below the 64-wide K step, 4128 ends inside one, 11008 is the 7B down projection; N off the 16-row tile."""
    _parity_case(dev, "skinny", M, N, K, res=False)
    _parity_case(dev, "skinny", M, N, K, res=True)


@pytest.mark.parametrize("N,K", [(96, 32), (520, 4128)])
@pytest.mark.parametrize("M", MS)
def test_gemm_suffix_w4_matches_fp64_reference(dev, M, N, K):
    _parity_case(dev, "suffix", M, N, K, res=M % 2 == 1)
    _parity_case(dev, "suffix", M, N, K, res=M % 2 == 0)


@pytest.mark.parametrize("M", [85, 256])
def test_gemm_suffix_w4_matches_fp64_reference_at_the_7b_down_projection(dev, M):
    _parity_case(dev, "suffix", M, 1000, 11008, res=M % 2 == 1)


# ------------------------------------------------------------------------------------------------ exact relations
@pytest.mark.parametrize("kernel,M", [("gemv", 3), ("skinny", 17), ("suffix", 85)])
def test_one_more_in_every_scale_byte_doubles_every_output(dev, kernel, M):
    N, K = 80, 256
    q, s, _ = _quantised(N, K, dev)
    x = _x(M, K, 21, dev)
    a, b = _call(kernel, x, q, s), _call(kernel, x, q, (s + 1).contiguous())
    assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0
    assert torch.equal(b.float(), 2 * a.float())


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("M", MS)
def test_every_64_row_slice_is_the_skinny_w4_kernel_bit_for_bit(dev, M, res):
    N, K = 520, 4128
    q, s, _ = _quantised(N, K, dev)
    x = _x(M, K, M * 1000 + N, dev)
    r = _rand((M, N), M + N, 1.0).to(BF).to(dev) if res else None
    got = _call("suffix", x, q, s, res=r)
    for m0 in range(0, M, 64):
        m1 = min(m0 + 64, M)
        want = _call("skinny", x[m0:m1], q, s, res=None if r is None else r[m0:m1])
        assert torch.isfinite(want.float()).all() and torch.equal(got[m0:m1], want), (M, m0)


@pytest.mark.parametrize("M", [9, 17, 64])
def test_gateup_swiglu_w4_is_swiglu_of_the_plain_form(dev, M):
    from mla_amd import hip
    I, K = 264, 512
    q, s, _ = _quantised(2 * I, K, dev)
    x = _x(M, K, M + 5, dev, 1.0)
    plain = _call("skinny", x, q, s)
    want = hip.swiglu_fwd(plain)
    got = hip.gemm_skinny_gateup_swiglu_w4(x, q, s)
    assert got.shape == (M, I) and torch.isfinite(got.float()).all() and torch.equal(got, want)


@pytest.mark.parametrize("kernel,M,K,N", [("gemv", 2, 4096, 512), ("gemv", 5, 256, 96), ("gemv", 7, 8192, 64), ("skinny", 17, 4096, 96),
                                          ("skinny", 64, 512, 520), ("skinny", 9, 8192, 100)])
def test_w4_fused_rmsnorm_and_swiglu_inputs_match_the_separate_kernels(dev, kernel, M, K, N):
    from mla_amd import hip
    x = _rand((M, K), K + M, 1.3).to(BF).to(dev)
    w = (1 + _rand((K,), 5, 0.1)).to(BF).to(dev)
    q, s, _ = _quantised(N, K, dev)
    gu = _rand((M, 2 * K), K + 3 * M, 1.0).to(BF).to(dev)
    a = _call(kernel, hip.rmsnorm_fwd(x, w, 1e-5)[0], q, s)
    b = _call(kernel, x, q, s, norm_weight=w, eps=1e-5)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    a = _call(kernel, hip.swiglu_fwd(gu), q, s)
    b = _call(kernel, gu, q, s, swiglu=True)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("kernel,B,R,nh", [("gemv", 1, 2, 2), ("gemv", 2, 4, 2), ("gemv", 1, 8, 3), ("skinny", 1, 17, 2), ("skinny", 3, 17, 2)])
def test_w4_fused_rmsnorm_rope_qkv_is_the_three_kernels(dev, kernel, B, R, nh):
    """RMSNorm in the input path, the rotary embedding of the q | k columns in the epilogue, rows straight into per-sample cache slots ==
    rmsnorm_fwd + plain _w4 kernel + rope_inplace bit for bit; nothing outside the slots is written."""
    from mla_amd import hip
    f = {"gemv": hip.gemv_w4, "skinny": hip.gemm_skinny_w4}[kernel]
    D, K = 128, 512
    H = nh * D
    M, S_p, S_cap, ld = B * R, 11, 11 + R, 3 * nh * D + 64
    x = _rand((M, K), nh * 10 + R, 1.1).to(BF).to(dev)
    w = (1 + _rand((K,), 7, 0.1)).to(BF).to(dev)
    q, s, _ = _quantised(3 * H, K, dev)
    cos, sin = _tables(S_cap, dev, S0=S_p)
    ref = torch.zeros((B, S_cap, ld), dtype=BF, device=dev)
    f(hip.rmsnorm_fwd(x, w, 1e-5)[0], q, s, ref[:, S_p:], ld, ref.stride(0), R)
    plain = ref.clone()
    for b in range(B):
        hip.rope_inplace(ref[b, S_p:], cos, sin, R, nh, D, 0, H)
    got = torch.zeros_like(ref)
    f(x, q, s, got[:, S_p:], ld, got.stride(0), R, norm_weight=w, eps=1e-5, rope=(cos, sin, 2 * H))
    assert torch.isfinite(got.float()).all()
    assert float(got[:, :S_p].float().abs().max()) == 0 and float(got[:, :, 3 * H:].float().abs().max()) == 0
    assert torch.equal(got, ref)
    assert not torch.equal(got[:, S_p:, :2 * H], plain[:, S_p:, :2 * H]) and torch.equal(got[:, :, 2 * H:], plain[:, :, 2 * H:])


@pytest.mark.parametrize("kernel,M", [("gemv", 4), ("skinny", 4), ("skinny", 34), ("suffix", 34)])
def test_w4_cache_slot_addressing_is_the_plain_call(dev, kernel, M):
    """Rows of sample b land at out + b * batch_stride + r * ldo (+ column offset): the dense output bit for bit, nothing else touched."""
    from mla_amd import hip
    f = {"gemv": hip.gemv_w4, "skinny": hip.gemm_skinny_w4, "suffix": hip.gemm_suffix_w4}[kernel]
    N, K, rpb = 72, 256, 2
    q, s, _ = _quantised(N, K, dev)
    x = _rand((M, K), 32, 0.5).to(BF).to(dev)
    dense = _call(kernel, x, q, s)
    ld = N + 64
    buf = torch.zeros((M // rpb, 5, ld), dtype=BF, device=dev)
    f(x, q, s, buf[:, 3:], ld, buf.stride(0), rpb, None, out_col=32)
    assert torch.isfinite(dense.float()).all() and torch.equal(buf[:, 3:5, 32:32 + N].reshape(M, N), dense)
    assert float(buf[:, :3].float().abs().max()) == 0 and float(buf[:, 3:, :32].float().abs().max()) == 0
    assert float(buf[:, 3:, 32 + N:].float().abs().max()) == 0


def test_ragged_slots_and_pos_with_identity_positions(dev):
    """Unequal slot[b]: the fused output == the dense projection written at each sample's slot, then rope_inplace at positions slot[b] + p,
    bit for bit; everything else keeps the sentinel; `_pos` with rope_pos = slot is the plain call."""
    from mla_amd import hip
    B, R, nh, K, cap = 3, 17, 2, 512, 46
    H = nh * 128
    M, ld = B * R, 3 * H + 64
    slots = [11, 29, 20]
    q, s, _ = _quantised(3 * H, K, dev)
    x = _x(M, K, 7, dev, 1.1)
    cos, sin = _tables(cap, dev)
    dense = _call("suffix", x, q, s)
    slot = torch.tensor(slots, dtype=torch.int32, device=dev)
    got = torch.full((B, cap + 4, ld), SENT, dtype=BF, device=dev)
    hip.gemm_suffix_w4(x, q, s, got, ld, got.stride(0), R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=cap)
    ref = torch.full((B, cap + 4, ld), SENT, dtype=BF, device=dev)
    for b, s0 in enumerate(slots):
        ref[b, s0:s0 + R, :3 * H] = dense[b * R:(b + 1) * R]
        hip.rope_inplace(ref[b, s0:s0 + R], cos[s0:s0 + R].contiguous(), sin[s0:s0 + R].contiguous(), R, nh, 128, 0, H)
    assert torch.isfinite(dense.float()).all() and torch.equal(got, ref)
    assert not torch.equal(got[0, 11:11 + R, :2 * H], dense[:R, :2 * H])
    pos = torch.full((B, cap + 4, ld), SENT, dtype=BF, device=dev)
    hip.gemm_suffix_w4(x, q, s, pos, ld, pos.stride(0), R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=cap, rope_pos=slot.clone(), rope_rows=cap)
    assert torch.equal(pos, got)


def test_gemm_suffix_w4_graph_replay(dev):
    """Captured once, replayed after x was rewritten: the eager launch on the new x, bit for bit."""
    from mla_amd import hip
    M, N, K = 85, 520, 4128
    q, s, _ = _quantised(N, K, dev)
    x = _rand((M, K), 5, 0.5).to(BF).to(dev)
    first = _call("suffix", x, q, s)                                         # also the warm-up outside the capture
    out = torch.empty((M, N), dtype=BF, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.gemm_suffix_w4(x, q, s, out, N, 0, M)
    x.copy_(_rand((M, K), 6, 0.5).to(BF))
    eager = _call("suffix", x, q, s)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and not torch.equal(eager, first)


# ------------------------------------------------------------------------------------------------ end to end, tiny model
N = 3


def infer_inputs(T, tag):
    """The recipe of tests/test_infer_fp8_gpu.py; the N initial samples come from their own generator (row 0 is the single call's)."""
    g = recipe._gen(tag)
    ids = torch.randint(3, 29000, (1, 20), generator=g)
    ids[0, 0] = 1
    ids = torch.cat([ids, torch.tensor([[29871]])], dim=1)
    image = torch.cat([torch.randn(1, 3, 672, 672, generator=g), torch.ones(1, 1, 672, 672)], dim=1)
    lo, hi = torch.tensor([0.0, -0.4, 0.75]), torch.tensor([0.6, 0.4, 1.25])
    pc = lo + (hi - lo) * torch.rand(1, 1024, 3, generator=g)
    proprio = torch.rand(1, 1, 7, generator=g) * 2 - 1
    starts = [torch.randint(0, 1024, (1,), generator=g), torch.randint(0, 512, (1,), generator=g)]
    noise = torch.randn(N, T, 7, generator=recipe._gen(tag + "_mx"))
    return ids, image, pc, proprio, noise, starts


@pytest.fixture(scope="module", params=[3, 15], ids=["window3_gemv", "window15_skinny"])
def tiny(request, dev):
    """hidden 256, 9 layers, 2 heads of 128; window 3: R = 5 suffix rows (mla_gemv_w4), window 15: R = 17 (mla_gemm_skinny_w4). The
    default (bf16) chunk is computed before any suffix_mx call on the model."""
    from mla_amd.backbones import LLaMa2LLMBackbone
    from mla_amd.llama import LlamaConfig
    from mla_amd.mla import MLA
    from mla_amd.prismatic import PrismaticVLM
    window = request.param
    bb = LLaMa2LLMBackbone(config=LlamaConfig(**(recipe.TINY_LLAMA | {"vocab_size": 32000})))
    vlm = PrismaticVLM("tiny", bb, token_size=recipe.TOKEN_SIZE, use_diff=True, use_pointcloud=True, use_contrastive=True,
                       use_generation=False, future_action_window_size=window)
    m = MLA(vlm, None, token_size=recipe.TOKEN_SIZE, future_action_window_size=window, use_diff=True, use_pointcloud=True,
            use_contrastive=True)
    m.load_state_dict({k: recipe.det_weight(k, v.shape) for k, v in m.state_dict().items()}, strict=True)
    m.eval().to(dev)
    for p in m.parameters():
        p.data = p.data.to(BF)
    inputs = infer_inputs(window + 1, "infer" if window == 3 else f"infer_chunk{window + 1}")
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    ids, image, pc, proprio, noise, _ = inputs
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, num_ddim_steps=8)
    default = m.predict_action_diff(noise=noise[:1], **kw)                   # bf16, before any suffix_mx call on this model
    fp4 = m.predict_action_diff(noise=noise[:1], suffix_mx="fp4", **kw)
    default.setflags(write=False)
    fp4.setflags(write=False)
    return m, window, inputs, kw, default, fp4


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_fp4_chunk_matches_its_reference_and_off_leaves_bf16_alone(dev, tiny):
    """"fp4" vs "fp4_as_bf16" (the bf16 kernels on the dequantised copy): the same function up to summation order. suffix_mx="off" is
    the default call bit for bit and launch for launch, before AND after fp4 calls on the same model (engines and graphs are per mode);
    "fp4" is not the bf16 chunk (the path was taken) and launches `_w4` kernels only where bf16 launched projections."""
    from mla_amd import hip
    m, window, (_, _, _, _, noise, _), kw, default, fp4 = tiny
    kw = dict(kw, noise=noise[:1])
    ref = m.predict_action_diff(suffix_mx="fp4_as_bf16", **kw)
    assert fp4.shape == (window + 1, 7) and np.isfinite(fp4).all()
    launches, orig = {}, hip.call
    try:
        for name, extra in (("plain", {}), ("off", {"suffix_mx": "off"}), ("fp4", {"suffix_mx": "fp4"})):
            launches[name] = []
            hip.call = lambda sym, *a, into=launches[name]: (into.append(sym), orig(sym, *a))[1]
            out = m.predict_action_diff(**extra, **kw)
            assert np.array_equal(out, fp4 if name == "fp4" else default), name
    finally:
        hip.call = orig
    assert launches["off"] == launches["plain"] and len(launches["plain"]) > 0
    assert not [n for n in launches["off"] if "_w4" in n or "mxfp4" in n]
    assert not np.array_equal(fp4, default)
    d = _rel(fp4, ref)
    print(f"window {window}: fp4 vs fp4_as_bf16 chunk {d:.3e}; NOT gated: fp4 vs bf16 chunk {_rel(fp4, default):.3e}")
    assert d < 3e-2
    engines = m.vlm.__dict__["_prefix_engines"]
    assert {e.suffix_mx for e in engines.values()} == {"off", "fp4", "fp4_as_bf16"}
    assert len({id(e.graph) for e in engines.values() if e.graph is not None}) == len(engines) >= 3


def test_fp4_epsilon_graph_and_eager(dev, tiny):
    """One epsilon call at t = 91: "fp4" within 2e-2 of "fp4_as_bf16"; the fp4 suffix pass was captured; replay == eager launches."""
    from mla_amd import infer
    m, window, (ids, image, pc, proprio, noise, _), _, _, _ = tiny
    T = window + 1
    kw = dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    t = torch.tensor([91], device=dev)
    x = noise[:1].to(dev)
    with torch.inference_mode():
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, suffix_mx="fp4", **kw)
        _, eps = eng(x, t)
        ref_eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, suffix_mx="fp4_as_bf16", **kw)
        _, eps_ref = ref_eng(x, t)
        assert eng is not ref_eng and eng.suffix_mx == "fp4" and eng.suffix_weights == "bf16" and eng.R == T + 1
        assert eng.graph is not None, f"the fp4 suffix pass was not captured into a graph: {eng.graph_error}"
        e = fro_rel(eps, eps_ref)
        print(f"window {window}: fp4 vs fp4_as_bf16 epsilon {e:.3e}")
        assert e < 2e-2
        _, eps2 = eng(x, t)                                                  # replay
        old = infer._USE_GRAPH
        try:
            infer._USE_GRAPH = False
            _, eps_e = eng(x, t)                                             # eager launches on the same cache
        finally:
            infer._USE_GRAPH = old
    assert torch.equal(eps, eps2) and torch.equal(eps, eps_e)


def test_fp4_composes_with_the_device_sampler_operand_and_attention_modes(dev, tiny):
    """sampler="device" gives the host loop's bits; suffix_operand="once" the fused pass's; suffix_attention="split" and the DDPM device
    loop stay within the chunk bound of their host / head forms (other summation order / the same bits); known_actions pins."""
    m, window, (_, _, _, _, noise, _), kw, _, fp4 = tiny
    kw = dict(kw, noise=noise[:1])
    assert np.array_equal(m.predict_action_diff(suffix_mx="fp4", sampler="device", **kw), fp4)
    assert np.array_equal(m.predict_action_diff(suffix_mx="fp4", suffix_operand="once", **kw), fp4)
    split = m.predict_action_diff(suffix_mx="fp4", suffix_attention="split", **kw)
    assert np.isfinite(split).all() and _rel(split, fp4) < 3e-2
    kd = dict(kw, use_ddim=False, num_ddim_steps=None)
    torch.manual_seed(5)
    host = m.predict_action_diff(suffix_mx="fp4", **kd)
    torch.manual_seed(5)
    assert np.array_equal(m.predict_action_diff(suffix_mx="fp4", ddpm_sampler="device", **kd), host)
    known = fp4[:2] * 0.5
    pinned = m.predict_action_diff(suffix_mx="fp4", known_actions=known, **kw)
    assert np.allclose(pinned[:2], known, atol=1e-6) and np.array_equal(
        m.predict_action_diff(suffix_mx="fp4", known_actions=known, sampler="device", **kw), pinned)


def test_fp4_samples_are_the_fp4_batch_one_calls(dev, tiny):
    """N = 3 samples on one prefix (mla_gemm_suffix_w4): each within 3e-2 of its own predict_action_diff(suffix_mx="fp4") call; at
    window 15 both run the skinny kernel's summation order and the same attention arithmetic: bit-identical."""
    m, window, (_, _, _, _, noise, _), kw, _, fp4 = tiny
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_mx="fp4", **kw)
    singles = np.stack([fp4] + [m.predict_action_diff(suffix_mx="fp4", noise=noise[n:n + 1], **kw) for n in range(1, N)])
    d = [_rel(got[n], singles[n]) for n in range(N)]
    print(f"window {window}: fp4 samples vs batch-1 fp4 calls {['%.2e' % v for v in d]}; bit-identical: {np.array_equal(got, singles)}")
    assert got.shape == (N, window + 1, 7) and max(d) < 3e-2
    if window == 15:
        assert np.array_equal(got, singles)
    one = m.predict_action_diff_samples(num_samples=1, noise=noise[:1], suffix_mx="fp4", **kw)
    assert np.array_equal(one[0], fp4)
    ref = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_mx="fp4_as_bf16", **kw)
    assert max(_rel(got[n], ref[n]) for n in range(N)) < 3e-2
    assert np.array_equal(m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_mx="fp4", sampler="device", **kw), got)


def test_fp4_batch_of_two_observations_times_two_samples(dev, tiny):
    """B = 2 x N = 2 through predict_action_diff_batch(num_samples=2) (mla_gemm_suffix_w4_pos): every observation's samples within the
    chunk bound of predict_action_diff_samples on it."""
    m, window, (ids, image, pc, proprio, noise, _), kw, _, _ = tiny
    ids2 = torch.cat([ids[:, :5], ids[:, 9:]], dim=1)                         # a shorter prompt: ragged prefixes
    nz = torch.stack([noise[:2], noise[1:3]])
    starts = m.vlm.vision_tower_3d.fps_starts_override
    m.vlm.vision_tower_3d.fps_starts_override = [s.repeat(2) for s in starts]  # one start index per observation
    try:
        out = m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, cur_robot_states=[proprio[0, 0].numpy()] * 2,
                                          input_ids=[ids, ids2], noise=nz, num_ddim_steps=8, num_samples=2, suffix_mx="fp4")
    finally:
        m.vlm.vision_tower_3d.fps_starts_override = starts
    assert out.shape == (2, 2, window + 1, 7) and np.isfinite(out).all()
    for b, i in enumerate((ids, ids2)):
        want = m.predict_action_diff_samples(num_samples=2, noise=nz[b], suffix_mx="fp4", **dict(kw, input_ids=i))
        d = max(_rel(out[b, n], want[n]) for n in range(2))
        print(f"window {window}: fp4 batch observation {b} vs its samples call {d:.2e}")
        assert d < 3e-2


def test_fp4_copy_follows_the_weights_and_is_its_own(dev, tiny):
    """An in-place update of one decoder weight (mul_ bumps _version) changes the next "fp4" chunk; restoring it restores the chunk. The
    MXFP4 copy has its own slot: an FP8 call in between leaves it (and "fp4"'s bits) alone."""
    m, _, (_, _, _, _, noise, _), kw, _, fp4 = tiny
    kw = dict(kw, noise=noise[:1])
    w = m.vlm.llm_backbone.llm.model.layers[4].mlp.down_proj.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    changed = m.predict_action_diff(suffix_mx="fp4", **kw)
    with torch.no_grad():
        w.copy_(saved)
    copy = m.vlm.__dict__["_prefix_mxfp4"]
    restored = m.predict_action_diff(suffix_mx="fp4", **kw)
    assert not np.array_equal(changed, fp4) and np.array_equal(restored, fp4)
    layers = m.vlm.__dict__["_prefix_mxfp4"]["fp4"]
    m.predict_action_diff(suffix_weights="fp8", **kw)
    m.predict_action_diff(prefill="compact", prefill_precision="fp8", suffix_mx="fp4", **kw)
    assert m.vlm.__dict__["_prefix_mxfp4"] is copy and copy["fp4"] is layers and "_prefix_fp8" in m.vlm.__dict__
    assert np.array_equal(m.predict_action_diff(suffix_mx="fp4", **kw), fp4)


def test_fp4_refusals_raise(dev, tiny, monkeypatch, recwarn):
    """No silent fallback: without the cached prefix, with another suffix_weights, at a shape an engine does not serve, and for B >= 2
    without num_samples -- the exception classes of the FP8 refusals."""
    from mla_amd import infer
    m, _, (ids, image, pc, proprio, noise, _), kw, _, _ = tiny
    one = dict(kw, noise=noise[:1])
    with pytest.raises(ValueError, match="suffix_mx"):
        m.predict_action_diff(suffix_mx="fp4", reuse_prefix=False, **one)
    with pytest.raises(ValueError, match="suffix_mx"):
        m.predict_action_diff(suffix_mx="fp4", suffix_weights="fp8", **one)
    with pytest.raises(ValueError, match="suffix_mx"):
        m.predict_action_diff_samples(num_samples=2, noise=noise[:2], suffix_mx="fp4", reuse_prefix=False, **kw)
    bkw = dict(cur_robot_states=[proprio[0, 0].numpy()] * 2, input_ids=[ids, ids], noise=noise[:2], num_ddim_steps=8)
    with pytest.raises(NotImplementedError, match="BatchedPrefixCachedEps"):
        m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, suffix_mx="fp4", **bkw)
    with pytest.raises(ValueError, match="suffix_mx"):
        m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, suffix_mx="fp4", reuse_prefix=False, num_samples=1,
                                    **dict(bkw, noise=noise[:2, None]))
    monkeypatch.setattr(infer.PrefixCachedEps, "MAX_ROWS", 1)
    with pytest.raises(ValueError, match="suffix_mx"):
        m.predict_action_diff(suffix_mx="fp4", **one)
    monkeypatch.undo()
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_R", 2)
    with pytest.raises(ValueError, match="suffix_mx"):
        m.predict_action_diff_samples(num_samples=2, noise=noise[:2], suffix_mx="fp4", **kw)
    monkeypatch.undo()
    one_b = m.predict_action_diff_batch([image[0]], [pc[0].numpy()], cur_robot_states=[proprio[0, 0].numpy()], input_ids=[ids], noise=noise[:1],
                                        num_ddim_steps=8, suffix_mx="fp4")
    assert np.array_equal(one_b[0], m.predict_action_diff(suffix_mx="fp4", **one))
