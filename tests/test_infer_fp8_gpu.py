"""GPU: weight-only FP8 for the suffix pass of cached-prefix action sampling -- the quantiser (mla_quant_fp8_rows), the two projection
kernels (mla_gemv_w8, mla_gemm_skinny_w8) and the `suffix_weights` modes of mla_amd/infer.py / MLA.predict_action_diff.

The format is OCP e4m3fn with one fp32 scale per output channel; the kernels sum x * code in fp32 over the unscaled codes and multiply the
finished sum by the scale. Bounds: 4e-3 Frobenius-relative against an fp64 reference over the dequantised weights is the project's bound for
"one bf16 rounding of the fp32 sums" (test_gemv_matches_fp32_reference); 3e-2 per chunk / 2e-2 per epsilon are the bounds of the
cached-vs-whole-forward tests for "same function, other rounding". How far "fp8" is from the bf16 chunk on this RANDOM tiny model is
printed, not gated: it says nothing about a trained policy."""
import os

import numpy as np
import pytest
import torch

from conftest import fro_rel
from oracle import recipe

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _rand(shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def quant_ref(W):
    """The CPU statement of the format: W bf16 [N, K] -> (codes float8_e4m3fn, scales fp32)."""
    f = W.float()
    amax = f.abs().amax(dim=1)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    return (f / s[:, None]).clamp(-448, 448).to(F8), s


def _kernels():
    from mla_amd import hip
    return {"gemv": hip.gemv_w8, "skinny": hip.gemm_skinny_w8}


def _quantised(N, K, seed, dev):
    from mla_amd import hip
    return hip.quant_fp8_rows(_rand((N, K), seed, 0.05).to(BF).to(dev))


# ------------------------------------------------------------------------------------------------ quantiser
def _quant_case(case):
    """bf16 source on the CPU; "strided" is a row block inside a wider buffer (row stride 768 > K = 256)."""
    if case == "300x512":
        W = _rand((300, 512), 1, 0.05)
        W[7] = 0.0                                       # all-zero row: scale 1, every code zero
        W[11] *= 0.01                                    # std 5e-4 next to a 40.0 outlier (scale 0.089): |w / s| sits around 2^-8 ... 2^-7 --
        W[11, 17] = 40.0                                 # the subnormals (< 2^-6) and, below 2^-10, zero
        return W.to(BF)
    if case == "7x16":
        return _rand((7, 16), 3, 0.05).to(BF)
    return _rand((40, 768), 2, 0.05).to(BF)[3:23, 128:384]


@pytest.mark.parametrize("case", ["300x512", "7x16", "strided"])
def test_quantiser_is_the_cpu_statement(dev, case):
    from mla_amd import hip
    W = _quant_case(case)
    q_ref, s_ref = quant_ref(W)
    Wd = W.to(dev)
    if case == "strided":
        Wd = torch.zeros((40, 768), dtype=BF, device=dev)[3:23, 128:384].copy_(W)
        assert Wd.stride(0) == 768 and not Wd.is_contiguous()
    q, s = hip.quant_fp8_rows(Wd)
    q2, s2 = hip.quant_fp8_rows(Wd)
    codes = q.view(torch.uint8).cpu()
    assert torch.equal(codes, q2.view(torch.uint8).cpu()) and torch.equal(s.cpu().view(torch.int32), s2.cpu().view(torch.int32))
    assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code"
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(q.cpu().float(), q_ref.float())                       # float compare: -0 and +0 both pass
    if case == "300x512":
        ref_codes = q_ref.view(torch.uint8)
        assert float(s_ref[7]) == 1.0 and not bool((ref_codes[7] & 0x7F).any()) and not bool((codes[7] & 0x7F).any())
        mag = ref_codes[11] & 0x7F                                           # the outlier row exercises what the test says it does
        assert int((mag == 0).sum()) > 0 and int(((mag > 0) & (mag < 8)).sum()) > 0 and int((mag == 0x7E).sum()) == 1


# ------------------------------------------------------------------------------------------------ decode pins the format
@pytest.mark.parametrize("kernel", ["gemv", "skinny"])
def test_decode_of_every_code_is_ocp_e4m3fn(dev, kernel):
    """Row n of W is filled with byte code n (the two NaN codes replaced by 0); one-hot x rows pick single products, all exactly
    representable: the output is scale * coeff * value(code). An FNUZ decode, a wrong subnormal or a sign slip fails."""
    codes = torch.arange(256, dtype=torch.uint8)
    codes[0x7F] = 0
    codes[0xFF] = 0
    W = codes[:, None].repeat(1, 64).contiguous()
    x = torch.zeros(2, 64)
    x[0, 3], x[1, 63] = 1.0, 0.5
    val = codes.view(F8).float()
    for sc in (1.0, 0.125):
        out = torch.full((2, 256), float("nan"), dtype=BF, device=dev)
        _kernels()[kernel](x.to(BF).to(dev), W.to(dev).view(F8), torch.full((256,), sc, device=dev), out, 256, 0, 2)
        want = sc * torch.stack([val, 0.5 * val])
        assert torch.equal(out.float().cpu(), want), (kernel, sc)


# ------------------------------------------------------------------------------------------------ projections vs fp64
def _projection_case(dev, kernel, M, N, K, res):
    q, s = _quantised(N, K, N + K, dev)
    x = _rand((M, K), M * 1000 + N, 0.5).to(BF).to(dev)
    r = _rand((M, N), M + N, 1.0).to(BF).to(dev) if res else None
    want = x.double() @ (q.float().double() * s.double()[:, None]).t() + (r.double() if res else 0)
    outs = []
    for _ in range(2):
        out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        _kernels()[kernel](x, q, s, out, N, 0, M, r)
        outs.append(out)
    assert torch.isfinite(outs[0].float()).all()
    e = fro_rel(outs[0], want)
    print(f"mla_{'gemv' if kernel == 'gemv' else 'gemm_skinny'}_w8 M {M} N {N} K {K} res {res}: fro_rel vs fp64 {e:.3e}")
    assert e < 4e-3                                                           # one bf16 rounding of the fp32 sums
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M,N,K,res", [(1, 256, 256, True), (2, 768, 256, False), (5, 1000, 11008, True), (8, 520, 4096, False),
                                       (3, 7, 512, False)])
def test_gemv_w8_matches_fp64_reference(dev, M, N, K, res):
    _projection_case(dev, "gemv", M, N, K, res)


@pytest.mark.parametrize("N,K", [(1000, 11008), (96, 48), (520, 4112)])
@pytest.mark.parametrize("M", [1, 9, 16, 17, 33, 64])
def test_gemm_skinny_w8_matches_fp64_reference(dev, M, N, K):
    """K = 48 is smaller than the 64-wide K step, 4112 ends inside one, 11008 is the 7B down projection; N off the 16-row tile."""
    _projection_case(dev, "skinny", M, N, K, res=M % 2 == 1)


@pytest.mark.parametrize("kernel,M", [("gemv", 3), ("skinny", 3), ("skinny", 17)])
def test_scale_multiplies_the_finished_sum(dev, kernel, M):
    """Doubling every scale doubles every output bit for bit (outputs of order 1: far from the ends of the bf16 range); a zero scale
    gives an exact zero column."""
    N, K = 80, 256
    q, _ = _quantised(N, K, 9, dev)
    s = (0.5 + torch.rand(N, generator=torch.Generator().manual_seed(4))).to(dev) / 448
    s[5] = 0.0
    x = _rand((M, K), 21, 0.5).to(BF).to(dev)
    a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
    _kernels()[kernel](x, q, s, a, N, 0, M)
    _kernels()[kernel](x, q, 2 * s, b, N, 0, M)
    assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0
    assert torch.equal(b.float(), 2 * a.float())
    assert float(a[:, 5].float().abs().max()) == 0 and float(b[:, 5].float().abs().max()) == 0


# ------------------------------------------------------------------------------------------------ fusions are the separate kernels
@pytest.mark.parametrize("kernel,M,K,N", [("gemv", 2, 4096, 512), ("gemv", 5, 256, 96), ("gemv", 7, 8192, 64), ("skinny", 17, 4096, 96),
                                          ("skinny", 64, 512, 520), ("skinny", 9, 8192, 100)])
def test_w8_fused_rmsnorm_and_swiglu_inputs_match_the_separate_kernels(dev, kernel, M, K, N):
    from mla_amd import hip
    f = _kernels()[kernel]
    x = _rand((M, K), K + M, 1.3).to(BF).to(dev)
    w = (1 + _rand((K,), 5, 0.1)).to(BF).to(dev)
    q, s = _quantised(N, K, N, dev)
    gu = _rand((M, 2 * K), K + 3 * M, 1.0).to(BF).to(dev)
    a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
    f(hip.rmsnorm_fwd(x, w, 1e-5)[0], q, s, a, N, 0, M)
    f(x, q, s, b, N, 0, M, norm_weight=w, eps=1e-5)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    a.fill_(float("nan"))
    b.fill_(float("nan"))
    f(hip.swiglu_fwd(gu), q, s, a, N, 0, M)
    f(gu, q, s, b, N, 0, M, swiglu=True)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("kernel,B,R,nh", [("gemv", 1, 2, 2), ("gemv", 2, 4, 2), ("gemv", 1, 8, 3), ("skinny", 1, 17, 2), ("skinny", 3, 17, 2)])
def test_w8_fused_rmsnorm_rope_qkv_is_the_three_kernels(dev, kernel, B, R, nh):
    """RMSNorm in the input path, the rotary embedding of the q | k columns in the epilogue (behind the scale), rows straight into
    per-sample cache slots == rmsnorm_fwd + plain _w8 kernel + rope_inplace bit for bit; nothing outside the slots is written."""
    from mla_amd import hip
    f = _kernels()[kernel]
    D, K = 128, 512
    H = nh * D
    M, S_p, S_cap, ld = B * R, 11, 11 + R, 3 * nh * D + 64
    x = _rand((M, K), nh * 10 + R, 1.1).to(BF).to(dev)
    w = (1 + _rand((K,), 7, 0.1)).to(BF).to(dev)
    q, s = _quantised(3 * H, K, nh + K, dev)
    fr = torch.outer(torch.arange(S_p, S_cap).float(), 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
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


@pytest.mark.parametrize("kernel,M", [("gemv", 4), ("skinny", 4), ("skinny", 34)])
def test_w8_cache_slot_addressing_is_the_plain_call(dev, kernel, M):
    """Rows of sample b land at out + b * batch_stride + r * ldo (+ column offset): the dense output bit for bit, nothing else touched."""
    f = _kernels()[kernel]
    N, K, rpb = 72, 256, 2
    q, s = _quantised(N, K, 31, dev)
    x = _rand((M, K), 32, 0.5).to(BF).to(dev)
    dense = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    f(x, q, s, dense, N, 0, M)
    ld = N + 64
    buf = torch.zeros((M // rpb, 5, ld), dtype=BF, device=dev)
    f(x, q, s, buf[:, 3:], ld, buf.stride(0), rpb, None, out_col=32)
    assert torch.equal(buf[:, 3:5, 32:32 + N].reshape(M, N), dense)
    assert float(buf[:, :3].float().abs().max()) == 0 and float(buf[:, 3:, :32].float().abs().max()) == 0
    assert float(buf[:, 3:, 32 + N:].float().abs().max()) == 0


# ------------------------------------------------------------------------------------------------ end to end, tiny model
def infer_inputs(T, tag):
    """The recipe of tests/test_inference_gpu.py (tag "infer": the inputs of the reference golden) / test_inference_chunk_gpu.py."""
    g = recipe._gen(tag)
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


@pytest.fixture(scope="module", params=[3, 15], ids=["window3_gemv", "window15_skinny"])
def tiny(request, dev):
    """hidden 256, 9 layers, 2 heads of 128; window 3: R = 5 suffix rows (mla_gemv_w8), window 15: R = 17 (mla_gemm_skinny_w8)."""
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
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, noise=noise, num_ddim_steps=8)
    return m, window, inputs, kw


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_fp8_chunk_matches_its_reference_and_leaves_bf16_alone(dev, tiny):
    """"fp8" vs "fp8_as_bf16" (the bf16 kernels on bf16(q * scale)): same function up to summation order and the 2^-9 rounding of q * scale.
    suffix_weights="bf16" is the default call bit for bit, before AND after an fp8 call on the same model (engines and graphs are per
    mode), and "fp8" is not "bf16" (the path was taken). Measured on MI355X: fp8 vs fp8_as_bf16 -- see DESIGN 3.5."""
    m, window, _, kw = tiny
    default = m.predict_action_diff(**kw)
    assert np.array_equal(m.predict_action_diff(suffix_weights="bf16", **kw), default)
    fp8 = m.predict_action_diff(suffix_weights="fp8", **kw)
    ref = m.predict_action_diff(suffix_weights="fp8_as_bf16", **kw)
    assert fp8.shape == (window + 1, 7) and np.isfinite(fp8).all()
    assert np.array_equal(m.predict_action_diff(suffix_weights="bf16", **kw), default)
    assert np.array_equal(m.predict_action_diff(**kw), default)
    assert not np.array_equal(fp8, default)
    d = _rel(fp8, ref)
    msg = f"window {window}: fp8 vs fp8_as_bf16 chunk {d:.3e}; NOT gated: fp8 vs bf16 chunk {_rel(fp8, default):.3e}"
    if window == 3:
        gold = np.load(os.path.join(G, "inference.npz"), allow_pickle=True)["mla_ddim8_actions"][0]
        msg += f", vs reference golden fp8 {_rel(fp8, gold):.3e} / bf16 {_rel(default, gold):.3e}"
    print(msg)
    assert d < 3e-2
    engines = m.vlm.__dict__["_prefix_engines"]
    assert len({id(e.graph) for e in engines.values() if e.graph is not None}) == len(engines) >= 3


def test_fp8_epsilon_graph_and_eager(dev, tiny):
    """One epsilon call at t = 91: "fp8" within 2e-2 of "fp8_as_bf16"; the fp8 suffix pass was captured; replay == eager launches."""
    from mla_amd import infer
    m, window, (ids, image, pc, proprio, noise, _), _ = tiny
    T = window + 1
    kw = dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    t = torch.tensor([91], device=dev)
    with torch.inference_mode():
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, suffix_weights="fp8", **kw)
        _, eps = eng(noise.to(dev), t)
        ref_eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, suffix_weights="fp8_as_bf16", **kw)
        _, eps_ref = ref_eng(noise.to(dev), t)
        assert eng is not ref_eng and eng.suffix_weights == "fp8" and eng.R == T + 1
        assert eng.graph is not None, f"the fp8 suffix pass was not captured into a graph: {eng.graph_error}"
        e = fro_rel(eps, eps_ref)
        print(f"window {window}: fp8 vs fp8_as_bf16 epsilon {e:.3e}")
        assert e < 2e-2
        _, eps2 = eng(noise.to(dev), t)                                        # replay
        old = infer._USE_GRAPH
        try:
            infer._USE_GRAPH = False
            _, eps_e = eng(noise.to(dev), t)                                   # eager launches on the same cache
        finally:
            infer._USE_GRAPH = old
    assert torch.equal(eps, eps2) and torch.equal(eps, eps_e)


def test_fp8_copy_follows_the_weights(dev, tiny):
    """An in-place update of one decoder weight (mul_ bumps _version) changes the next "fp8" chunk; restoring it restores the chunk."""
    m, _, _, kw = tiny
    before = m.predict_action_diff(suffix_weights="fp8", **kw)
    w = m.vlm.llm_backbone.llm.model.layers[4].mlp.down_proj.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    changed = m.predict_action_diff(suffix_weights="fp8", **kw)
    with torch.no_grad():
        w.copy_(saved)
    restored = m.predict_action_diff(suffix_weights="fp8", **kw)
    assert not np.array_equal(changed, before) and np.array_equal(restored, before)


def test_fp8_needs_the_cached_prefix_and_batch_one(dev, tiny):
    m, window, (ids, image, pc, proprio, noise, _), kw = tiny
    with pytest.raises(ValueError):
        m.predict_action_diff(suffix_weights="fp8", reuse_prefix=False, **kw)
    bkw = dict(cur_robot_states=[proprio[0, 0].numpy()] * 2, input_ids=[ids, ids], noise=torch.cat([noise, noise]), num_ddim_steps=8)
    with pytest.raises(NotImplementedError, match="BatchedPrefixCachedEps"):
        m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, suffix_weights="fp8", **bkw)
    one = m.predict_action_diff_batch([image[0]], [pc[0].numpy()], cur_robot_states=[proprio[0, 0].numpy()], input_ids=[ids], noise=noise,
                                      num_ddim_steps=8, suffix_weights="fp8")
    assert np.array_equal(one[0], m.predict_action_diff(suffix_weights="fp8", **kw))
