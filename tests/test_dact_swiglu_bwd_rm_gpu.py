"""mla_gemm_dact_swiglu_bwd_rm (gemm256_kernel<0, 1, 2>: the fused down-projection dgrad + SwiGLU backward on W_down [H, I] AS STORED)
against mla_gemm_dact_swiglu_bwd on transpose(W). The reduction-major B image keeps the k-slot map, the K order and the accumulation order
per output of the k-contiguous one, so every comparison is torch.equal -- there is no tolerance. Shapes (T, H = K, I): the smallest at
which each mechanism can fail (see CASES)."""
import pytest
import torch

BF = torch.bfloat16
# (256, 64, 256): one tile, one K-tile (compiler-scheduled loop: an odd K-tile count).
# (264, 192, 512): 8-row partial row tile; three K-tiles (odd count, ring parity); two column tiles (gate / up pairing across pid_n).
# (520, 128, 264): 8-channel partial column tile; two K-tiles = the generated assembly main loop.
CASES = [(256, 64, 256), (264, 192, 512), (520, 128, 264)]


def bfr(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def operands(dev):
    """Per shape: dy [T, K], W [K, I] as stored, gate|up [T, 2I] and the reference outputs of the k-contiguous launch on transpose(W);
    made once, never written."""
    from mla_amd import hip
    out = {}
    for T, K, I in CASES:
        dy, w, gu = bfr(T, K, seed=T).to(dev), bfr(K, I, scale=0.05, seed=K + 1).to(dev), bfr(T, 2 * I, seed=I + 2).to(dev)
        ref = hip.gemm_dact_swiglu_bwd(dy, hip.transpose(w), gu, want_t=True)
        assert ref is not None
        out[(T, K, I)] = (dy, w, gu, ref[0], ref[1])
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_stored_weight_launch_is_the_transposed_weight_launch_bit_for_bit(dev, operands, shape):
    from mla_amd import hip
    T, K, I = shape
    dy, w, gu, ref_dgu, ref_dguT = operands[shape]
    dgu, dguT = hip.gemm_dact_swiglu_bwd_rm(dy, w, gu, want_t=True)
    assert dgu.shape == (T, 2 * I) and dguT.shape == (2 * I, T)
    assert same(dgu, ref_dgu), float((dgu.float() - ref_dgu.float()).abs().max())
    assert same(dguT, ref_dguT)
    # null transposed output: row-major result the same, a poisoned buffer that is NOT handed in keeps its poison
    poison = torch.full((2 * I, T), float("nan"), dtype=BF, device=dev)
    before = bits(poison).clone()
    dgu_n, none = hip.gemm_dact_swiglu_bwd_rm(dy, w, gu, want_t=False)
    assert none is None and same(dgu_n, ref_dgu)
    assert torch.equal(bits(poison), before)
    # a second launch on the same inputs repeats the first bit for bit
    dgu2, dguT2 = hip.gemm_dact_swiglu_bwd_rm(dy, w, gu, want_t=True)
    assert same(dgu2, dgu) and same(dguT2, dguT)
    # and the compiler-scheduled loop of the same instantiation gives the same bits as the generated one
    prev = hip.gemm_kloop(0)
    try:
        dgu3, dguT3 = hip.gemm_dact_swiglu_bwd_rm(dy, w, gu, want_t=True)
    finally:
        hip.gemm_kloop(1 if prev else 0)
    assert same(dgu3, ref_dgu) and same(dguT3, ref_dguT)


@pytest.mark.gpu
def test_row_strided_weight_inside_poisoned_buffers(dev, operands):
    """W as a row-strided view (row stride > I) of a larger NaN-filled buffer, NaN rows behind dy and gate|up, outputs carved out of
    NaN-filled buffers: the results are the reference's and nothing outside the outputs changes."""
    from mla_amd import hip
    T, K, I = 264, 192, 512
    dy, w, gu, ref_dgu, ref_dguT = operands[(T, K, I)]
    nan = float("nan")
    w_big = torch.full((K + 2, I + 64), nan, dtype=BF, device=dev)
    w_big[1:K + 1, 8:8 + I] = w
    w_v = w_big[1:K + 1, 8:8 + I]
    assert w_v.stride(0) == I + 64 and w_v.data_ptr() % 16 == 0
    dy_big = torch.full((T + 8, K), nan, dtype=BF, device=dev)
    dy_big[:T] = dy
    gu_big = torch.full((T + 8, 2 * I), nan, dtype=BF, device=dev)
    gu_big[:T] = gu
    dgu_big = torch.full((T + 16, 2 * I), nan, dtype=BF, device=dev)
    dguT_big = torch.full((2 * I + 16, T), nan, dtype=BF, device=dev)
    snap = [bits(t).clone() for t in (w_big, dy_big, gu_big)]
    dgu, dguT = hip.gemm_dact_swiglu_bwd_rm(dy_big[:T], w_v, gu_big[:T], want_t=True, dgu=dgu_big[8:8 + T], dguT=dguT_big[8:8 + 2 * I])
    torch.cuda.synchronize()
    assert same(dgu, ref_dgu) and same(dguT, ref_dguT)
    for t, s in zip((w_big, dy_big, gu_big), snap):
        assert torch.equal(bits(t), s)
    for guard in (dgu_big[:8], dgu_big[8 + T:], dguT_big[:8], dguT_big[8 + 2 * I:]):
        assert bool(torch.isnan(guard.float()).all())


@pytest.mark.gpu
def test_contract_violations_raise(dev):
    """What the kernel does not serve is an error from the library's argument check (no launch, no fallback)."""
    from mla_amd import hip
    T, K, I = 256, 128, 256
    dy, w, gu = bfr(T, K, seed=1).to(dev), bfr(K, I, seed=2).to(dev), bfr(T, 2 * I, seed=3).to(dev)
    with pytest.raises(RuntimeError, match="mla_gemm_dact_swiglu_bwd_rm"):          # T < 256
        hip.gemm_dact_swiglu_bwd_rm(dy[:248], w, gu[:248].contiguous())
    with pytest.raises(RuntimeError, match="mla_gemm_dact_swiglu_bwd_rm"):          # K % 64 != 0
        hip.gemm_dact_swiglu_bwd_rm(dy[:, :96].contiguous(), w[:96], gu)
    flat = torch.zeros(T * K + 8, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="16-B alignment"):                       # dy 8 bytes off a 16-B boundary
        hip.gemm_dact_swiglu_bwd_rm(flat[4:4 + T * K].view(T, K), w, gu)
    wflat = torch.zeros(K * I + 8, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="16-B alignment"):                       # W likewise
        hip.gemm_dact_swiglu_bwd_rm(dy, wflat[4:4 + K * I].view(K, I), gu)
    with pytest.raises(RuntimeError, match="mla_gemm_dact_swiglu_bwd_rm"):          # row stride of W not a multiple of 8
        hip.gemm_dact_swiglu_bwd_rm(dy, torch.zeros(K, I + 4, dtype=BF, device=dev)[:, :I], gu)
    torch.cuda.synchronize()
