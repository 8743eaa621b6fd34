"""GPU: cached-prefix action sampling for action chunks of up to 64 suffix rows (mla_gemm_skinny_bf16, mla_attn_chunk, the engine
selection of mla_amd/infer.py). Projections the GEMV accepts (M <= 8, M x K rows in LDS) and attention it accepts (R <= 8) keep their
kernels; beyond, the skinny MFMA GEMM and the online-softmax chunk attention serve 9 .. 64 rows."""
import math

import numpy as np
import pytest
import torch

from conftest import fro_rel
from oracle import recipe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _rand(shape, seed, scale, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ skinny GEMM
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("N,K", [(12288, 4096), (22016, 4096), (4096, 11008), (1000, 11008), (7, 512)])
@pytest.mark.parametrize("M", [1, 8, 9, 16, 17, 33, 64])
def test_gemm_skinny_matches_fp32_reference(dev, M, N, K, res):
    """out[m] = x[m] @ W^T (+ residual) for 1 <= M <= 64, incl. N not a multiple of the 16-row tile and K not a multiple of the 32-wide
    step split over 8 waves; the batch-strided output with a column offset is the dense output bit for bit and touches nothing else."""
    from mla_amd import hip
    x = _rand((M, K), M * 7 + K, 0.5, dev)
    W = _rand((N, K), N + K, 0.05, dev)
    r = _rand((M, N), M + N, 1.0, dev) if res else None
    want = x.float() @ W.float().t() + (r.float() if res else 0)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    hip.gemm_skinny(x, W, out, N, 0, M, r)
    assert torch.isfinite(out.float()).all()
    assert fro_rel(out, want) < 4e-3
    rpb = M // 2 if M % 2 == 0 and M > 1 else M
    nb, S_cap, ld = M // rpb, rpb + 3, N + 64
    buf = torch.zeros((nb, S_cap, ld), dtype=BF, device=dev)
    hip.gemm_skinny(x, W, buf[:, 3:], ld, buf.stride(0), rpb, r, out_col=32)
    assert torch.equal(buf[:, 3:, 32:32 + N].reshape(M, N), out)
    assert float(buf[:, :3].float().abs().max()) == 0 and float(buf[:, 3:, :32].float().abs().max()) == 0
    assert float(buf[:, 3:, 32 + N:].float().abs().max()) == 0


@pytest.mark.parametrize("M,K,N", [(17, 4096, 1536), (64, 4096, 520), (17, 8192, 96)])
def test_gemm_skinny_fused_rmsnorm_is_the_separate_kernels(dev, M, K, N):
    """pre = 1: LlamaRMSNorm of the rows formed inside the kernel == rmsnorm_fwd followed by the plain skinny GEMM, bit for bit.
    (rmsnorm_fwd serves rows up to 8192; the product applies the fused norm at the hidden size, 4096 at 7B.)"""
    from mla_amd import hip
    x = _rand((M, K), K + M, 1.3, dev)
    w = (1 + 0.1 * torch.randn(K, generator=torch.Generator(device=dev).manual_seed(5), device=dev)).to(BF)
    W = _rand((N, K), N, 0.05, dev)
    a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
    hip.gemm_skinny(hip.rmsnorm_fwd(x, w, 1e-5)[0], W, a, N, 0, M)
    hip.gemm_skinny(x, W, b, N, 0, M, norm_weight=w, eps=1e-5)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("M,K,N", [(17, 11008, 4096), (64, 11008, 520), (9, 4096, 100)])
def test_gemm_skinny_fused_swiglu_is_the_separate_kernels(dev, M, K, N):
    """pre = 2: silu(gate) * up of the packed gate|up rows formed inside the kernel == swiglu_fwd + plain skinny GEMM, bit for bit, at the
    7B down-projection width the GEMV rejects."""
    from mla_amd import hip
    gu = _rand((M, 2 * K), K + 3 * M, 1.0, dev)
    W = _rand((N, K), N + 1, 0.05, dev)
    a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
    hip.gemm_skinny(hip.swiglu_fwd(gu), W, a, N, 0, M)
    hip.gemm_skinny(gu, W, b, N, 0, M, swiglu=True)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    with pytest.raises(RuntimeError):
        hip.gemv(gu, W, a, N, 0, M, swiglu=True)                       # the shape the GEMV cannot take


@pytest.mark.parametrize("B,R,nh,K", [(1, 17, 4, 4096), (4, 16, 2, 4096), (1, 64, 32, 512)])
def test_gemm_skinny_fused_rmsnorm_rope_qkv_is_the_three_kernels(dev, B, R, nh, K):
    """RMSNorm in the operand path + rotary embedding of the q | k columns in the epilogue, rows straight into per-sample cache slots ==
    rmsnorm_fwd + plain skinny GEMM + rope_inplace, bit for bit; the rotation really happened."""
    from mla_amd import hip
    D = 128
    H = nh * D
    M, S_p = B * R, 11
    S_cap = S_p + R
    x = _rand((M, K), nh * 10 + R, 1.1, dev)
    w = (1 + 0.1 * torch.randn(K, generator=torch.Generator(device=dev).manual_seed(7), device=dev)).to(BF)
    W = _rand((3 * H, K), nh + K, 0.06, dev)
    pos = torch.arange(S_p, S_cap).float()
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(pos, inv)
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    ref = torch.zeros((B, S_cap, 3 * H), dtype=BF, device=dev)
    hip.gemm_skinny(hip.rmsnorm_fwd(x, w, 1e-5)[0], W, ref[:, S_p:], 3 * H, ref.stride(0), R)
    plain = ref.clone()
    for b in range(B):
        hip.rope_inplace(ref[b, S_p:], cos, sin, R, nh, D, 0, H)
    got = torch.zeros_like(ref)
    hip.gemm_skinny(x, W, got[:, S_p:], 3 * H, got.stride(0), R, norm_weight=w, eps=1e-5, rope=(cos, sin, 2 * H))
    assert torch.isfinite(got.float()).all() and float(got[:, :S_p].float().abs().max()) == 0
    assert torch.equal(got, ref)
    assert not torch.equal(got[:, S_p:, :2 * H], plain[:, S_p:, :2 * H]) and torch.equal(got[:, :, 2 * H:], plain[:, :, 2 * H:])


# ------------------------------------------------------------------------------------------------ chunk attention
def _attn_ref(cache, B, H, S_kv, R):
    D = 128
    c = cache.float()[:, :S_kv]
    q = c[:, S_kv - R:, :H * D].view(B, R, H, D).transpose(1, 2)
    k = c[:, :, H * D:2 * H * D].view(B, S_kv, H, D).transpose(1, 2)
    v = c[:, :, 2 * H * D:].view(B, S_kv, H, D).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    mask = torch.arange(S_kv, device=cache.device)[None, :] > (S_kv - R + torch.arange(R, device=cache.device))[:, None]
    s = s.masked_fill(mask, float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * R, H * D)


@pytest.mark.parametrize("H", [2, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S_kv", [None, 77, 565, 2100])
@pytest.mark.parametrize("R", [1, 9, 16, 17, 64])
def test_attn_chunk_matches_fp32_reference(dev, R, S_kv, B, H):
    """mla_attn_chunk: the last R rows of the packed q|k|v cache are the queries, query r attends to keys [0, S_kv - R + r]; online
    softmax over key tiles; two calls are bit-identical."""
    from mla_amd import hip
    S_kv = R if S_kv is None else S_kv
    cache = _rand((B, S_kv + 3, 3 * H * 128), S_kv * 100 + R + B + H, 0.7, dev)
    o = hip.attn_chunk(cache, B, H, 128, S_kv, R, 1 / math.sqrt(128))
    assert torch.isfinite(o.float()).all()
    assert fro_rel(o, _attn_ref(cache, B, H, S_kv, R)) < 5e-3
    assert torch.equal(o, hip.attn_chunk(cache, B, H, 128, S_kv, R, 1 / math.sqrt(128)))


def test_attn_chunk_long_prefix_and_graph_replay(dev):
    """S_kv = 4096 (configs[4]-length prefixes: LDS does not grow with S_kv), and a captured graph replays bit-identically to eager."""
    from mla_amd import hip
    B, H, S_kv, R = 1, 4, 4096, 33
    cache = _rand((B, S_kv, 3 * H * 128), 11, 0.7, dev)
    eager = hip.attn_chunk(cache, B, H, 128, S_kv, R, 1 / math.sqrt(128))
    assert fro_rel(eager, _attn_ref(cache, B, H, S_kv, R)) < 5e-3
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = hip.attn_chunk(cache, B, H, 128, S_kv, R, 1 / math.sqrt(128))
    o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, eager)


# ------------------------------------------------------------------------------------------------ predict_action_diff at chunk length
def infer_inputs(T):
    g = recipe._gen(f"infer_chunk{T}")
    ids = torch.randint(3, 29000, (1, 20), generator=g)
    ids[0, 0] = 1
    ids = torch.cat([ids, torch.tensor([[29871]])], dim=1)
    image = torch.cat([torch.randn(1, 3, 672, 672, generator=g), torch.ones(1, 1, 672, 672)], dim=1)
    lo, hi = torch.tensor([0.0, -0.4, 0.75]), torch.tensor([0.6, 0.4, 1.25])
    pc = lo + (hi - lo) * torch.rand(1, 1024, 3, generator=g)
    proprio = torch.rand(1, 1, 7, generator=g) * 2 - 1
    noise = torch.randn(1, T, 7, generator=g)
    starts = [torch.randint(0, 1024, (1,), generator=g), torch.randint(0, 512, (1,), generator=g)]
    return ids, image, pc, proprio, noise, starts


def build_model(dev, window, token_size=recipe.TOKEN_SIZE, **llama):
    from mla_amd.backbones import LLaMa2LLMBackbone
    from mla_amd.llama import LlamaConfig
    from mla_amd.mla import MLA
    from mla_amd.prismatic import PrismaticVLM
    bb = LLaMa2LLMBackbone(config=LlamaConfig(**(recipe.TINY_LLAMA | {"vocab_size": 32000} | llama)))
    vlm = PrismaticVLM("tiny", bb, token_size=token_size, use_diff=True, use_pointcloud=True, use_contrastive=True,
                       use_generation=False, future_action_window_size=window)
    m = MLA(vlm, None, token_size=token_size, future_action_window_size=window, use_diff=True, use_pointcloud=True, use_contrastive=True)
    m.load_state_dict({k: recipe.det_weight(k, v.shape) for k, v in m.state_dict().items()}, strict=True)
    m.eval().to(dev)
    for p in m.parameters():
        p.data = p.data.to(BF)
    return m


def _eps_pair(dev, m, T, seed_inputs):
    """(cached-prefix epsilon, whole-forward epsilon, engine) of one sampler call at t = 91."""
    from mla_amd import infer
    ids, image, pc, proprio, noise, _ = seed_inputs
    kw = dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    with torch.inference_mode():                                              # as predict_action_diff calls the engine
        _, eps_full = m.vlm(noise.to(dev), torch.tensor([91], device=dev), **kw)
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **kw)
        _, eps_c = eng(noise.to(dev), torch.tensor([91], device=dev))
    return eps_c, eps_full, eng


@pytest.mark.parametrize("window", [15, 7])
def test_prefix_cached_sampler_at_action_chunk_length(dev, window):
    """The default action chunk (future_action_window_size = 15: 17 suffix rows) and window 7 (9 rows) sample through the cached prefix:
    same chunk as the whole-forward control flow within the bound of the T = 4 test, one epsilon within 2e-2 of the eval forward, the
    suffix pass captured into a graph that replays bit-identically to eager launches."""
    from mla_amd import infer
    T = window + 1
    m = build_model(dev, window)
    inputs = infer_inputs(T)
    ids, image, pc, proprio, noise, starts = inputs
    m.vlm.vision_tower_3d.fps_starts_override = starts
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, noise=noise, num_ddim_steps=8)
    full = m.predict_action_diff(reuse_prefix=False, **kw)
    cached = m.predict_action_diff(reuse_prefix=True, **kw)
    assert cached.shape == (T, 7) and np.isfinite(cached).all()
    d = np.linalg.norm(cached - full) / np.linalg.norm(full)
    print(f"window {window}: cached vs whole-forward chunk {d:.3e}")
    assert d < 3e-2
    eps_c, eps_full, eng = _eps_pair(dev, m, T, inputs)
    assert eng.R == T + 1 and eng.graph is not None, "the suffix pass was not captured into a graph"
    assert fro_rel(eps_c, eps_full.float().cpu()) < 2e-2
    _, eps_c2 = eng(noise.to(dev), torch.tensor([91], device=dev))
    old = infer._USE_GRAPH
    try:
        infer._USE_GRAPH = False
        _, eps_e = eng(noise.to(dev), torch.tensor([91], device=dev))
    finally:
        infer._USE_GRAPH = old
    assert torch.equal(eps_c, eps_c2) and torch.equal(eps_c, eps_e)


def test_prefix_cached_sampler_beyond_64_rows_falls_back(dev):
    """B * (1 + T) > 64 suffix rows: predict_action_diff warns and runs the reference's control flow -- the result IS reuse_prefix=False's."""
    window = 64                                                               # T = 65, 66 suffix rows
    T = window + 1
    m = build_model(dev, window)
    ids, image, pc, proprio, noise, starts = infer_inputs(T)
    m.vlm.vision_tower_3d.fps_starts_override = starts
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, noise=noise, num_ddim_steps=8)
    full = m.predict_action_diff(reuse_prefix=False, **kw)
    with pytest.warns(RuntimeWarning, match="suffix rows"):
        cached = m.predict_action_diff(reuse_prefix=True, **kw)
    assert cached.shape == (T, 7) and np.array_equal(cached, full)
    assert not m.vlm.__dict__.get("_prefix_engines")


@pytest.fixture(scope="module")
def model_7b_dims(dev):
    """Two decoder layers at 7B dimensions (hidden 4096, intermediate 11008, 32 heads of 128)."""
    m = build_model(dev, 15, token_size=4096, hidden_size=4096, intermediate_size=11008, num_attention_heads=32, num_hidden_layers=2)
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("R", [8, 17])
def test_prefix_cached_epsilon_at_7b_layer_dimensions(dev, model_7b_dims, R):
    """At 7B widths the down projection's 11008-wide rows reject the GEMV from 8 rows on (LDS); the cached epsilon at R = 8 and R = 17
    matches the whole forward."""
    m = model_7b_dims
    T = R - 1
    inputs = infer_inputs(T)
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    eps_c, eps_full, eng = _eps_pair(dev, m, T, inputs)
    assert eng.graph is not None, eng.graph_error
    assert torch.isfinite(eps_c.float()).all()
    assert fro_rel(eps_c, eps_full.float().cpu()) < 2e-2
