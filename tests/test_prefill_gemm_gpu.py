"""GPU: the compact prefill GEMMs (mla_amd/csrc/prefill.hip: mla_gemm_prefill_bf16 / _qkv_rope / _gateup_swiglu) against an fp64
reference on the same bf16 operands. Yardstick: the error of the existing kernel of the same contract on identical operands
(hip.gemm, hip.gemm_qkv_rope, the `act` of hip.gemm_gateup_swiglu) -- e_new <= 2 e_old, max-abs. Shapes: partial row tiles, one and several
column tiles, the real row count with the split-K the plan picks for a narrow N, the full row range with K a multiple of 32 only, and the
down projection's long-K split."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 4096                                             # bytes behind the workspace's stated size that must stay untouched
SENT = -777.0                                            # exactly representable in bf16

PLAIN_SHAPES = [(M, N, 256) for M in (1, 65, 129) for N in (128, 384)] + [(545, 256, 4096), (1024, 128, 352), (545, 128, 11008)]


def _rand(shape, seed, scale, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(BF)


class _Ws:
    """A workspace of exactly the stated size followed by a guard region; filled with a NaN pattern (a partial that is read before it is
    written poisons the output)."""

    def __init__(self, M, N, K, dev, fill=0xFF):
        from mla_amd import hip
        self.need = hip.gemm_prefill_ws_bytes(M, N, K)
        assert self.need == hip.plan_gemm_prefill(M, N, K).ws_bytes
        self.full = torch.full((self.need + GUARD,), fill, dtype=torch.uint8, device=dev)
        self.full[self.need:] = 0xA5
        self.ws = self.full[:self.need] if self.need else None

    def check(self):
        assert bool((self.full[self.need:] == 0xA5).all()), "the guard region behind the workspace was written"


@functools.lru_cache(maxsize=None)
def _plain_case(M, N, K):
    """Operands, fp64 references and the existing GEMM's errors, computed once per shape."""
    from mla_amd import hip
    dev = torch.device("cuda:0")
    x, W, r = _rand((M, K), 3 * M + K, 0.5, dev), _rand((N, K), N + K, 0.05, dev), _rand((M, N), M + N, 1.0, dev)
    ref = x.double() @ W.double().t()
    ref_r = ref + r.double()
    e_old = float((hip.gemm(x, W).double() - ref).abs().max())
    e_old_r = float((hip.gemm(x, W, residual=r).double() - ref_r).abs().max())
    return x, W, r, ref, ref_r, e_old, e_old_r


@pytest.mark.parametrize("M,N,K", PLAIN_SHAPES)
def test_plain_and_residual_within_twice_the_existing_gemms_error(dev, M, N, K):
    from mla_amd import hip
    x, W, r, ref, ref_r, e_old, e_old_r = _plain_case(M, N, K)
    plan = hip.plan_gemm_prefill(M, N, K)
    for res, want, e0 in ((None, ref, e_old), (r, ref_r, e_old_r)):
        w = _Ws(M, N, K, dev)
        out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        hip.gemm_prefill(x, W, out, N, 0, M, residual=res, ws=w.ws)
        assert torch.isfinite(out.float()).all()
        e_new = float((out.double() - want).abs().max())
        print(f"plain M {M} N {N} K {K} split {plan.split} residual {res is not None}: e_new {e_new:.4e} e_old {e0:.4e}")
        assert e_new <= 2 * e0, (e_new, e0)
        w.check()
        # determinism: a second launch over a differently poisoned workspace gives the same bits
        w2 = _Ws(M, N, K, dev, fill=0x7F)
        out2 = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        hip.gemm_prefill(x, W, out2, N, 0, M, residual=res, ws=w2.ws)
        assert torch.equal(out, out2)
        w2.check()


def test_split_shapes_really_split():
    from mla_amd import hip
    assert hip.plan_gemm_prefill(545, 256, 4096).split > 1 and hip.plan_gemm_prefill(545, 128, 11008).split > 1
    assert hip.plan_gemm_prefill(130, 768, 4096).split > 1 and hip.plan_gemm_prefill(545, 256, 4096).ws_bytes > 0


@pytest.mark.parametrize("M,N,K,rpb", [(129, 384, 256, 43), (545, 256, 4096, 109), (64, 128, 256, 64)])
def test_strided_output_touches_nothing_else(dev, M, N, K, rpb):
    """ldo > N, a batch stride that is not rows x ldo, a column offset: the addressed elements are the dense output bit for bit, every
    other element of the (larger) buffer still holds the sentinel."""
    from mla_amd import hip
    x, W, r = _plain_case(M, N, K)[:3]
    w = _Ws(M, N, K, dev)
    dense = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    hip.gemm_prefill(x, W, dense, N, 0, M, residual=r, ws=w.ws)
    nb, lead, tail, ld, col = M // rpb, 3, 2, N + 72, 40
    assert nb * rpb == M
    buf = torch.full((nb, lead + rpb + tail, ld), SENT, dtype=BF, device=dev)
    assert buf.stride(0) != rpb * ld
    hip.gemm_prefill(x, W, buf[:, lead:], ld, buf.stride(0), rpb, residual=r, out_col=col, ws=w.ws)
    assert torch.equal(buf[:, lead:lead + rpb, col:col + N].reshape(M, N), dense)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, lead:lead + rpb, col:col + N] = False
    assert bool((buf[mask] == SENT).all())
    w.check()


def _rope_tables(S, dev, D=128):
    pos = torch.arange(S).float()
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(pos, inv)
    return fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)


def _rope_ref(y, cos, sin, S, rope_cols):
    """fp64 rotate-half of columns [0, rope_cols) per head of 128, row m at position m % S."""
    M = y.shape[0]
    pos = torch.arange(M, device=y.device) % S
    c, s = cos.double()[pos], sin.double()[pos]                        # [M, 64]
    out = y.clone()
    for h0 in range(0, rope_cols, 128):
        a, b = y[:, h0:h0 + 64], y[:, h0 + 64:h0 + 128]
        out[:, h0:h0 + 64] = a * c - b * s
        out[:, h0 + 64:h0 + 128] = b * c + a * s
    return out


@pytest.mark.parametrize("K", [256, 4096])
def test_qkv_rope_within_twice_the_fused_training_kernels_error(dev, K):
    """N = 3 x 256, rope_cols 512, head_dim 128, two samples of 65 rows (table row = m % 65) written into cache slots of a larger buffer;
    K = 4096 takes the split-K path (the rotation then runs in the reduction launch). Yardstick: mla_gemm_qkv_rope (needs >= 256 rows:
    the same two samples followed by two more)."""
    from mla_amd import hip
    S, nb, H = 65, 2, 256
    N, M = 3 * H, nb * S
    x4 = _rand((4 * S, K), 11 + K, 0.5, dev)
    x = x4[:M]
    W = _rand((N, K), 13 + K, 0.05, dev)
    cos, sin = _rope_tables(S, dev)
    ref = _rope_ref(x.double() @ W.double().t(), cos, sin, S, 2 * H)
    old = torch.empty((4 * S, N), dtype=BF, device=dev)
    assert hip.gemm_qkv_rope(x4, W, old, cos, sin, S, 2 * H) is True
    e_old = float((old[:M].double() - ref).abs().max())
    w = _Ws(M, N, K, dev)
    S_cap = S + 17
    cache = torch.full((nb, S_cap, N + 8), SENT, dtype=BF, device=dev)
    hip.gemm_prefill_qkv_rope(x, W, cache, cache.stride(1), cache.stride(0), S, (cos, sin, 2 * H), 128, ws=w.ws)
    got = cache[:, :S, :N].reshape(M, N)
    assert torch.isfinite(got.float()).all()
    e_new = float((got.double() - ref).abs().max())
    print(f"rope K {K} split {hip.plan_gemm_prefill(M, N, K).split}: e_new {e_new:.4e} e_old {e_old:.4e}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert bool((cache[:, S:] == SENT).all()) and bool((cache[:, :, N:] == SENT).all())
    w.check()
    # the rotation really happened, and only in the q | k columns
    plain = torch.empty((M, N), dtype=BF, device=dev)
    hip.gemm_prefill(x, W, plain, N, 0, M, ws=w.ws)
    assert not torch.equal(got[:, :2 * H], plain[:, :2 * H]) and torch.equal(got[:, 2 * H:], plain[:, 2 * H:])
    cache2 = torch.full_like(cache, SENT)
    hip.gemm_prefill_qkv_rope(x, W, cache2, cache.stride(1), cache.stride(0), S, (cos, sin, 2 * H), 128, ws=_Ws(M, N, K, dev, 0x7F).ws)
    assert torch.equal(cache, cache2)


@pytest.mark.parametrize("M,K", [(65, 256), (545, 4096)])
def test_gateup_swiglu_within_twice_the_fused_training_kernels_error(dev, M, K):
    """I = 128: silu(gate) * up from the packed [2 I, K] matrix, only act written. Yardstick: the `act` of mla_gemm_gateup_swiglu (needs
    >= 256 rows: x followed by zero rows). (545, 4096) takes the split-K path."""
    from mla_amd import hip
    I = 128
    Mp = max(M, 256)
    xp = torch.zeros((Mp, K), dtype=BF, device=dev)
    xp[:M] = _rand((M, K), 17 + M, 0.5, dev)
    x = xp[:M]
    Wgu = _rand((2 * I, K), 19 + K, 0.05, dev)
    y = x.double() @ Wgu.double().t()
    ref = torch.nn.functional.silu(y[:, :I]) * y[:, I:]
    old = hip.gemm_gateup_swiglu(xp, Wgu, False)
    assert old is not None
    e_old = float((old[1][:M].double() - ref).abs().max())
    w = _Ws(M, 2 * I, K, dev)
    buf = torch.full((M + 2, I + 8), SENT, dtype=BF, device=dev)
    hip.gemm_prefill_gateup_swiglu(x, Wgu, buf, ws=w.ws)
    act = buf[:M, :I]
    assert torch.isfinite(act.float()).all()
    e_new = float((act.double() - ref).abs().max())
    print(f"swiglu M {M} K {K} split {hip.plan_gemm_prefill(M, 2 * I, K).split}: e_new {e_new:.4e} e_old {e_old:.4e}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert bool((buf[M:] == SENT).all()) and bool((buf[:, I:] == SENT).all())
    w.check()
    buf2 = torch.full_like(buf, SENT)
    hip.gemm_prefill_gateup_swiglu(x, Wgu, buf2, ws=_Ws(M, 2 * I, K, dev, 0x7F).ws)
    assert torch.equal(buf, buf2)


def test_refusals_launch_nothing(dev):
    """M = 1025, K = 48 and a workspace one byte short return the documented code (-1 -> RuntimeError in the binding) in the host-side
    argument checks; the output keeps its sentinel."""
    from mla_amd import hip
    W = _rand((256, 4096), 5, 0.05, dev)
    out = torch.full((1025, 256), SENT, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="1 <= M <= 1024"):
        hip.gemm_prefill(_rand((1025, 4096), 6, 0.5, dev), W, out, 256, 0, 1025, ws=torch.empty(1 << 24, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="K % 32 == 0"):
        hip.gemm_prefill(_rand((64, 48), 7, 0.5, dev), _rand((256, 48), 8, 0.05, dev), out, 256, 0, 64)
    need = hip.gemm_prefill_ws_bytes(545, 256, 4096)
    x = _rand((545, 4096), 9, 0.5, dev)
    with pytest.raises(RuntimeError, match="workspace"):
        hip.gemm_prefill(x, W, out, 256, 0, 545, ws=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="workspace"):
        hip.gemm_prefill(x, W, out, 256, 0, 545, ws=None)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_graph_capture_replays_both_launches(dev):
    """The split-K pair of launches goes on the given stream only: a captured graph replays bit-identically to the eager call."""
    from mla_amd import hip
    M, N, K = 545, 256, 4096
    x, W, r = _plain_case(M, N, K)[:3]
    w = _Ws(M, N, K, dev)
    eager = torch.empty((M, N), dtype=BF, device=dev)
    hip.gemm_prefill(x, W, eager, N, 0, M, residual=r, ws=w.ws)
    out = torch.empty((M, N), dtype=BF, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.gemm_prefill(x, W, out, N, 0, M, residual=r, ws=w.ws)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    w.check()
