"""GPU: suffix_operand="once" of the batch-1 cached-prefix engine -- the gate|up projection with the SwiGLU epilogue
(mla_gemm_skinny_gateup_swiglu_bf16 / _w8) and the seven-launch pass built on it.

The acceptance criterion is bit identity, not a tolerance: a weight row's sum depends only on that row, the K split over the 8 waves and
the order of the partial sums, all of which the new kernel form shares with mla_gemm_skinny_*, so
    gemm_skinny_gateup_swiglu(x, W) == swiglu_fwd(gemm_skinny(x, W))            (torch.equal)
and the "once" pass (stand-alone RMSNorm, plain projections, SwiGLU epilogue) returns the arrays of the "fused" pass (np.array_equal)."""
import numpy as np
import pytest
import torch

from test_inference_chunk_gpu import build_model, infer_inputs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = -776.0                                                             # exact in bf16; no output of these tests comes near it


# ------------------------------------------------------------------------------------------------ kernel
def operands(M, I, K, seed, device):
    """x [M, K], W [2 I, K] bf16 from a CPU generator (the same bits everywhere), x scaled so that the largest |gate| is about 8: where
    SiLU is non-linear and the bf16 rounding in front of it matters."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(device)
    W = (torch.randn(2 * I, K, generator=g) * 0.05).to(BF).to(device)
    gate = x.to(BF).float() @ W[:I].float().t()
    x = (x * (8.0 / float(gate.abs().max()))).to(BF)
    return x, W


def check_span(gate, M, I):
    """The gate values of the reference span about +-8 (both signs; the far side too wherever there are enough values to expect it)."""
    lo, hi = float(gate.float().min()), float(gate.float().max())
    print(f"gate span [{lo:.3f}, {hi:.3f}] over {M * I} values")
    assert 6.0 <= max(-lo, hi) <= 10.0 and lo < 0.0 < hi
    if M * I >= 64:
        assert lo < -3.0 and hi > 3.0


def guarded(M, I, dev):
    """out with ldo = I + 16 and two guard rows, pre-filled with the sentinel."""
    return torch.full((M + 2, I + 16), SENTINEL, dtype=BF, device=dev)


def check_guards(buf, M, I):
    assert bool((buf[M:] == SENTINEL).all()) and bool((buf[:M, I:] == SENTINEL).all()), "a write outside out[:M, :I]"


MS = [1, 9, 16, 17, 33, 64]
# one tile; empty wave K ranges (3 steps over 8 waves); several tiles with a ragged last tile row count (520 = 65 x 8); K = 40 / 48: a K
# that is no multiple of the 32- / 64-wide step
SHAPES_BF16 = [(8, 32), (24, 96), (520, 512), (24, 40)]
SHAPES_W8 = [(8, 32), (24, 96), (520, 512), (24, 48)]


@pytest.mark.parametrize("I,K", SHAPES_BF16)
@pytest.mark.parametrize("M", MS)
def test_gateup_swiglu_bf16_is_swiglu_of_the_plain_form(dev, M, I, K):
    from mla_amd import hip
    x, W = operands(M, I, K, 1000 * M + I + K, dev)
    plain = torch.full((M, 2 * I), float("nan"), dtype=BF, device=dev)
    hip.gemm_skinny(x, W, plain, 2 * I, 0, M)
    check_span(plain[:, :I], M, I)
    want = hip.swiglu_fwd(plain)
    got = hip.gemm_skinny_gateup_swiglu(x, W)
    assert got.shape == (M, I) and torch.isfinite(got.float()).all() and torch.equal(got, want)
    buf = guarded(M, I, dev)
    assert hip.gemm_skinny_gateup_swiglu(x, W, out=buf, ldo=I + 16) is buf
    assert torch.equal(buf[:M, :I], want)
    check_guards(buf, M, I)


@pytest.mark.parametrize("I,K", SHAPES_W8)
@pytest.mark.parametrize("M", MS)
def test_gateup_swiglu_w8_is_swiglu_of_the_plain_form(dev, M, I, K):
    from mla_amd import hip
    x, W = operands(M, I, K, 2000 * M + I + K, dev)
    q, scale = hip.quant_fp8_rows(W)
    plain = torch.full((M, 2 * I), float("nan"), dtype=BF, device=dev)
    hip.gemm_skinny_w8(x, q, scale, plain, 2 * I, 0, M)
    check_span(plain[:, :I], M, I)
    want = hip.swiglu_fwd(plain)
    got = hip.gemm_skinny_gateup_swiglu_w8(x, q, scale)
    assert got.shape == (M, I) and torch.isfinite(got.float()).all() and torch.equal(got, want)
    buf = guarded(M, I, dev)
    hip.gemm_skinny_gateup_swiglu_w8(x, q, scale, out=buf, ldo=I + 16)
    assert torch.equal(buf[:M, :I], want)
    check_guards(buf, M, I)
    # the up rows' scales are their own: doubling them doubles up, hence (exactly, a power of two) the product
    scale2 = scale.clone()
    scale2[I:] *= 2.0
    assert torch.equal(hip.gemm_skinny_gateup_swiglu_w8(x, q, scale2).float(), want.float() * 2.0)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_gateup_swiglu_at_the_7b_projection(dev, w8):
    """(I, K) = (11 008, 4 096) at M = 17: the default action window's gate|up projection, 1 376 workgroups."""
    from mla_amd import hip
    M, I, K = 17, 11008, 4096
    x, W = operands(M, I, K, 7, dev)
    plain = torch.full((M, 2 * I), float("nan"), dtype=BF, device=dev)
    buf = guarded(M, I, dev)
    if w8:
        q, scale = hip.quant_fp8_rows(W)
        hip.gemm_skinny_w8(x, q, scale, plain, 2 * I, 0, M)
        hip.gemm_skinny_gateup_swiglu_w8(x, q, scale, out=buf, ldo=I + 16)
    else:
        hip.gemm_skinny(x, W, plain, 2 * I, 0, M)
        hip.gemm_skinny_gateup_swiglu(x, W, out=buf, ldo=I + 16)
    check_span(plain[:, :I], M, I)
    assert torch.equal(buf[:M, :I], hip.swiglu_fwd(plain))
    check_guards(buf, M, I)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("M,I,K", [(17, 12, 64), (17, 24, 36), (65, 24, 64)], ids=["I12", "K36", "M65"])
def test_gateup_swiglu_refusals(dev, w8, M, I, K):
    """I % 8, K % 8 (K % 16 for the FP8 form: K = 40 as well) and M > 64: a negative code with mla_last_error set, nothing launched."""
    from mla_amd import hip
    cases = [(M, I, K)] + ([(17, 24, 40)] if w8 and K == 36 else [])
    for M, I, K in cases:
        ldx = (K + 15) // 16 * 16                                             # aligned rows: the refusal is about M / I / K
        x = torch.ones((M, ldx), dtype=BF, device=dev)[:, :K]
        Wb = torch.ones((2 * I, ldx), dtype=BF, device=dev)
        W = (Wb.to(torch.float8_e4m3fn) if w8 else Wb)[:, :K]
        scale = torch.ones(2 * I, dtype=torch.float32, device=dev)
        buf = guarded(M, I, dev)
        name = "mla_gemm_skinny_gateup_swiglu_" + ("w8" if w8 else "bf16")
        args = [x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0)] + ([scale.data_ptr()] if w8 else []) + \
               [buf.data_ptr(), buf.stride(0), M, I, K, hip._stream()]
        rc = getattr(hip.lib(), name)(*args)
        assert rc < 0 and name in hip.lib().mla_last_error().decode()
        with pytest.raises(RuntimeError, match=name):
            if w8:
                hip.gemm_skinny_gateup_swiglu_w8(x, W, scale, out=buf, ldo=I + 16)
            else:
                hip.gemm_skinny_gateup_swiglu(x, W, out=buf, ldo=I + 16)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ engine, tiny model
@pytest.fixture(scope="module")
def tiny(dev):
    """window -> (model, predict_action_diff keywords, default(**modes)): one tiny model per window for the whole module, the "fused"
    chunk of every mode combination computed once."""
    built = {}

    def get(window):
        if window not in built:
            T = window + 1
            m = build_model(dev, window)
            ids, image, pc, proprio, noise, starts = infer_inputs(T)
            m.vlm.vision_tower_3d.fps_starts_override = starts
            kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, noise=noise)
            fused = {}

            def default(**modes):
                key = tuple(sorted(modes.items()))
                if key not in fused:
                    torch.manual_seed(11)
                    fused[key] = m.predict_action_diff(**kw, **modes)
                    assert fused[key].shape == (T, 7) and np.isfinite(fused[key]).all()
                return fused[key]
            built[window] = (m, kw, default)
        return built[window]
    yield get
    built.clear()
    torch.cuda.empty_cache()


def once(m, kw, **modes):
    torch.manual_seed(11)                                                     # the DDPM loop draws from the global generator
    return m.predict_action_diff(suffix_operand="once", **kw, **modes)


def engines(m, operand):
    return [e for e in m.vlm.__dict__["_prefix_engines"].values() if e.suffix_operand == operand]


@pytest.mark.parametrize("sampler", ["host", "device"])
@pytest.mark.parametrize("weights", ["bf16", "fp8", "fp8_as_bf16"])
@pytest.mark.parametrize("window", [15, 7])
def test_once_is_the_default_chunk(tiny, window, weights, sampler):
    """17 and 9 suffix rows: the seven-launch pass returns the array of the five-launch pass."""
    m, kw, default = tiny(window)
    modes = dict(suffix_weights=weights, sampler=sampler)
    want = default(**modes)
    got = once(m, kw, **modes)
    assert np.array_equal(got, want)
    eng = [e for e in engines(m, "once") if e.suffix_weights == weights and e.suffix_attention == "head"][-1]
    assert eng.R == window + 2 and eng.graph_error is None
    if sampler == "device":
        assert all(st.graph is not None for st in eng._ddim.values()) and eng._ddim


@pytest.mark.parametrize("window", [15, 7])
def test_once_with_split_attention_and_with_the_device_ddpm_loop(tiny, window):
    m, kw, default = tiny(window)
    for modes in (dict(suffix_attention="split"), dict(use_ddim=False, ddpm_sampler="device")):
        assert np.array_equal(once(m, kw, **modes), default(**modes)), modes
    assert all(e.graph_error is None for e in engines(m, "once"))


def test_once_at_5_rows_is_the_default_pass(tiny):
    """Window 3 (5 suffix rows): the GEMV pass in both modes."""
    m, kw, default = tiny(3)
    assert np.array_equal(once(m, kw), default())
    assert np.array_equal(once(m, kw, suffix_weights="fp8"), default(suffix_weights="fp8"))


def test_both_modes_capture_their_pass_and_coexist(tiny):
    m, kw, default = tiny(15)
    assert np.array_equal(m.predict_action_diff(**kw), default())              # run here: the store keeps the four latest engines
    once(m, kw)
    store = m.vlm.__dict__["_prefix_engines"]
    fused_keys = [k for k, e in store.items() if e.suffix_operand == "fused" and e.suffix_weights == "bf16" and e.suffix_attention == "head"]
    once_keys = [k for k, e in store.items() if e.suffix_operand == "once" and e.suffix_weights == "bf16" and e.suffix_attention == "head"]
    assert len(fused_keys) == 1 and len(once_keys) == 1 and once_keys[0] == fused_keys[0] + ("operand:once",)
    for k in fused_keys + once_keys:
        assert store[k].graph is not None and store[k].graph_error is None, (k, store[k].graph_error)
    assert store[fused_keys[0]] is not store[once_keys[0]]


def test_batch_and_samples_forward_the_mode(tiny):
    """B = 1 and num_samples = 1 end in predict_action_diff: the keyword arrives there."""
    m, kw, _ = tiny(15)
    want = once(m, kw)
    n_once = len(engines(m, "once"))
    b = m.predict_action_diff_batch([kw["image"]], [kw["pointcloud"]], cur_robot_states=[kw["cur_robot_state"]], input_ids=[kw["input_ids"]],
                                    noise=kw["noise"], suffix_operand="once")
    s = m.predict_action_diff_samples(num_samples=1, suffix_operand="once", **kw)
    assert b.shape == (1,) + want.shape and np.array_equal(b[0], want)
    assert s.shape == (1,) + want.shape and np.array_equal(s[0], want)
    assert len(engines(m, "once")) == n_once                                  # served by the engine of the direct call
    with pytest.raises(ValueError, match="suffix_operand"):
        m.predict_action_diff_samples(num_samples=1, suffix_operand="twice", **kw)
    with pytest.raises(ValueError, match="reuse_prefix"):
        m.predict_action_diff(suffix_operand="once", reuse_prefix=False, **kw)


# ------------------------------------------------------------------------------------------------ engine, 7B layer dimensions
@pytest.fixture(scope="module")
def model_7b_layers(dev):
    """Two decoder layers at 7B dimensions (hidden 4096, intermediate 11008, 32 heads of 128)."""
    m = build_model(dev, 15, token_size=4096, hidden_size=4096, intermediate_size=11008, num_attention_heads=32, num_hidden_layers=2)
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_once_epsilon_at_7b_layer_dimensions(dev, model_7b_layers, weights):
    """R = 17 at 7B widths: every row of one pass (and the epsilon read from it) is the same in both modes."""
    from mla_amd import infer
    m, T = model_7b_layers, 16
    ids, image, pc, proprio, noise, starts = infer_inputs(T)
    m.vlm.vision_tower_3d.fps_starts_override = starts
    kw = dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    rows, eps = {}, {}
    with torch.inference_mode():
        for operand in infer.MODES["suffix_operand"].values:
            eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, suffix_weights=weights, suffix_operand=operand, **kw)
            _, e = eng(noise.to(dev), torch.tensor([91], device=dev))
            assert eng.suffix_operand == operand and eng.R == 17 and eng.graph is not None, eng.graph_error
            rows[operand], eps[operand] = eng.h_out.clone(), e.clone()
    assert torch.isfinite(eps["once"].float()).all() and float(eps["once"].float().abs().max()) > 0
    assert torch.equal(rows["once"], rows["fused"]) and torch.equal(eps["once"], eps["fused"])
