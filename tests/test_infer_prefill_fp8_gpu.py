"""GPU: the opt-in FP8 prefill of the cached-prefix engines (MLA.predict_action_diff(prefill="compact", prefill_precision="fp8"),
mla_amd/infer.py _compact_layer on the GEMMs of mla_amd/csrc/prefill.hip) against its yardstick "fp8_as_bf16" (the bf16 compact
kernels on the dequantised codes), an fp32 statement of the fake-quantised decoder layer, and the bf16 compact prefill; the default paths
stay bit for bit what they were. Tiny model (hidden 256, intermediate 512, 9 layers, 2 heads of 128), windows 1 and 15."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe
from oracle import torch_oracle as TO

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
BOUND = 3e-2                                             # the cached-prefix engines' bound for "same function, other rounding" 
FP8 = dict(prefill="compact", prefill_precision="fp8")
YARD = dict(prefill="compact", prefill_precision="fp8_as_bf16")


def infer_inputs(T, tag):
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


def build_model(dev, window):
    from mla_amd.backbones import LLaMa2LLMBackbone
    from mla_amd.llama import LlamaConfig
    from mla_amd.mla import MLA
    from mla_amd.prismatic import PrismaticVLM
    bb = LLaMa2LLMBackbone(config=LlamaConfig(**(recipe.TINY_LLAMA | {"vocab_size": 32000})))
    vlm = PrismaticVLM("tiny", bb, token_size=recipe.TOKEN_SIZE, use_diff=True, use_pointcloud=True, use_contrastive=True,
                       use_generation=False, future_action_window_size=window)
    m = MLA(vlm, None, token_size=recipe.TOKEN_SIZE, future_action_window_size=window, use_diff=True, use_pointcloud=True,
            use_contrastive=True)
    m.load_state_dict({k: recipe.det_weight(k, v.shape) for k, v in m.state_dict().items()}, strict=True)
    m.eval().to(dev)
    for p in m.parameters():
        p.data = p.data.to(BF)
    return m


def _call_kwargs(inputs):
    ids, image, pc, proprio, noise, _ = inputs
    return dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, noise=noise, num_ddim_steps=8)


@pytest.fixture(scope="module", params=[1, 15], ids=["window1", "window15"])
def tiny(request, dev):
    """window 1: R = 3 suffix rows, window 15: R = 17; fixed noise and FPS start indices; a second observation under another tag."""
    window = request.param
    m = build_model(dev, window)
    inputs = infer_inputs(window + 1, f"prefill_fp8_chunk{window + 1}")
    other = infer_inputs(window + 1, f"prefill_fp8_other{window + 1}")
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    yield m, window, inputs, _call_kwargs(inputs), _call_kwargs(other)
    del m
    torch.cuda.empty_cache()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ 1. one layer, given input
def _fq(x):
    """hip.quant_fp8_rows's CPU statement followed by the dequantisation, per row of the last axis, in fp32."""
    amax = x.abs().amax(dim=-1, keepdim=True)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    return (x / s).clamp(-448, 448).to(F8).float() * s


def _oracle_layer(x, w8, nh, eps):
    """fp32 CPU statement of one fake-quantised decoder layer on the rows x [1, S, H]: the layer of oracle/torch_oracle.py with
    quantise -> dequantise at the four projection inputs and the dequantised weight codes (w8: the engine's (ln1, qkv, o, ln2, gate|up,
    down) with W8 projections) -> (post-RoPE q|k|v rows [S, 3H], layer output [S, H])."""
    ln1, qkv, wo, ln2, gu, wd = w8
    deq = lambda m: m.q.float().cpu() * m.scale.float().cpu()[:, None]          # noqa: E731
    _, S, H = x.shape
    D = H // nh
    cos, sin = TO.rope_tables(S, D)
    h = _fq(TO.rmsnorm(x, ln1.detach().float().cpu(), eps))
    q, k, v = (t.view(1, S, nh, D).transpose(1, 2) for t in F.linear(h, deq(qkv)).split(H, dim=-1))
    q, k = TO.apply_rope(q, k, cos, sin)
    rows = torch.cat([t.transpose(1, 2).reshape(S, H) for t in (q, k, v)], dim=1)
    a = TO.causal_attention(q, k, v).transpose(1, 2).reshape(1, S, H)
    x1 = x + F.linear(_fq(a), deq(wo))
    h2 = _fq(TO.rmsnorm(x1, ln2.detach().float().cpu(), eps))
    g, u = F.linear(h2, deq(gu)).chunk(2, dim=-1)
    out = x1 + F.linear(_fq(F.silu(g) * u), deq(wd))
    return rows, out[0]


def test_each_layer_against_the_fp32_fake_quantised_layer(dev, tiny):
    """Per layer, on the train engine's input rows of that layer: the FP8 layer is as close to the fp32 statement of the fake-quantised
    layer as the yardstick mode -- max|fp8 - oracle| <= 2 x max|fp8_as_bf16 - oracle|, for the post-RoPE q|k|v rows and for the layer
    output. One layer at a time on a given input: a code that flips on a rounding tie does not compound across layers."""
    from mla_amd import infer, ops
    m, window, inputs, _, _ = tiny
    T = window + 1
    ids, image, pc, proprio, _, _ = inputs
    kw = dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    with torch.inference_mode():
        eng_t = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **kw)
        eng_f = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **FP8, **kw)
        eng_y = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **YARD, **kw)
        assert len({id(eng_t), id(eng_f), id(eng_y)}) == 3 and (eng_f.prefill_precision, eng_y.prefill_precision) == ("fp8", "fp8_as_bf16")
        assert eng_f._prefill_xq is not None and eng_f._prefill_xs is not None and eng_y._prefill_xq is None and eng_t._prefill_ws is None
        k = infer.PrefixCachedEps._splice_position(kw["input_ids"])
        prefix = eng_t._prefix_rows(kw["input_ids"], k, kw["images"], kw["point_cloud"], kw["camera_name"], kw["proprio"])
        S_p, H = eng_t.S_p, eng_t.H
        h, layer_inputs = prefix.reshape(S_p, H), []
        for w in eng_t._weights():                                            # the train engine's input rows of every layer
            layer_inputs.append(h)
            h, _ = ops.DecoderLayerFn._fwd(h, None, eng_t.cos_p, eng_t.sin_p, 1, S_p, eng_t.nheads, eng_t.eps, w)
        w_f, w_y = eng_f._prefill_layers(), eng_y._prefill_layers()
        assert isinstance(w_f[0][1], infer.W8) and w_y[0][1].dtype == BF
        worst = 0.0
        for l, x in enumerate(layer_inputs):
            got = {}
            for name, eng, ws in (("fp8", eng_f, w_f), ("fp8_as_bf16", eng_y, w_y)):
                out = eng._compact_layer(ws[l], x, 1, S_p, eng.cache[l], eng.cache[l].stride(0))
                got[name] = (eng.cache[l][0, :S_p].float().cpu(), out.float().cpu())
            ref = _oracle_layer(x.float().cpu()[None], w_f[l], eng_f.nheads, eng_f.eps)
            for part, j in (("q|k|v", 0), ("output", 1)):
                assert torch.isfinite(got["fp8"][j]).all()
                e_f, e_y = (float((got[n][j] - ref[j]).abs().max()) for n in ("fp8", "fp8_as_bf16"))
                worst = max(worst, e_f / e_y)
                print(f"window {window} layer {l} {part}: max|fp8 - oracle| {e_f:.4e}, max|fp8_as_bf16 - oracle| {e_y:.4e}, "
                      f"max|fp8 - fp8_as_bf16| {float((got['fp8'][j] - got['fp8_as_bf16'][j]).abs().max()):.4e}")
                assert e_f <= 2 * e_y, (l, part, e_f, e_y)
    print(f"window {window}: worst fp8 / fp8_as_bf16 error ratio over the layers {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 2. chunk
def test_fp8_chunk_against_its_yardstick_and_the_defaults_stay(dev, tiny):
    """The "fp8" chunk is finite, deterministic and within 3e-2 of the "fp8_as_bf16" chunk (two implementations of one function); the
    default call and prefill="compact" alone return the same bits before and after. What the format costs -- d(fp8, compact bf16) -- is
    printed, not bounded by a chosen number; it has to be smaller than the distance between the compact bf16 chunks of two observations."""
    m, window, _, kw, other = tiny
    default, compact = m.predict_action_diff(**kw), m.predict_action_diff(prefill="compact", **kw)
    fp8 = m.predict_action_diff(**FP8, **kw)
    assert fp8.shape == (window + 1, 7) and np.isfinite(fp8).all()
    yard = m.predict_action_diff(**YARD, **kw)
    assert np.array_equal(m.predict_action_diff(**FP8, **kw), fp8)            # deterministic
    assert np.array_equal(m.predict_action_diff(**kw), default) and np.array_equal(m.predict_action_diff(prefill="compact", **kw), compact)
    assert np.array_equal(m.predict_action_diff(prefill="compact", prefill_precision="bf16", **kw), compact)
    compact_other = m.predict_action_diff(prefill="compact", **other)
    same_noise = m.predict_action_diff(prefill="compact", **dict(other, noise=kw["noise"]))
    d_yard, d_cost, d_yard_cost, d_obs = _rel(fp8, yard), _rel(fp8, compact), _rel(yard, compact), _rel(compact_other, compact)
    msg = (f"window {window}: fp8 vs fp8_as_bf16 {d_yard:.3e} (bound {BOUND}); the format's cost: fp8 vs compact bf16 {d_cost:.3e}, "
           f"fp8_as_bf16 vs compact bf16 {d_yard_cost:.3e}; another observation vs this one (compact bf16) {d_obs:.3e}, with this "
           f"one's initial noise {_rel(same_noise, compact):.3e}")
    print(msg)
    assert d_yard < BOUND, msg
    assert d_cost < d_obs, msg
    engines = m.vlm.__dict__["_prefix_engines"]
    assert sum("precision:fp8" in k for k in engines) == 1 and sum("precision:fp8_as_bf16" in k for k in engines) == 1
    assert all(("precision:fp8" in k) == (e._prefill_xq is not None) for k, e in engines.items())


# ------------------------------------------------------------------------------------------------ 3. composition
def test_one_fp8_copy_serves_the_prefill_and_the_suffix_pass(dev, tiny):
    """prefill_precision="fp8" with suffix_weights="bf16" builds the model's FP8 copy; suffix_weights="fp8" then streams the SAME object."""
    m, window, _, kw, _ = tiny
    m.vlm.__dict__.pop("_prefix_engines", None)
    m.vlm.__dict__.pop("_prefix_fp8", None)
    a = m.predict_action_diff(**FP8, **kw)
    shared = m.vlm.__dict__["_prefix_fp8"]
    copy = shared["fp8"]
    (eng_a,) = m.vlm.__dict__["_prefix_engines"].values()
    assert eng_a.suffix_weights == "bf16" and eng_a._suffix is eng_a._packed and eng_a._prefill_layers() is copy
    b = m.predict_action_diff(suffix_weights="fp8", **FP8, **kw)
    assert np.isfinite(b).all() and m.vlm.__dict__["_prefix_fp8"]["fp8"] is copy
    eng_b = next(e for k, e in m.vlm.__dict__["_prefix_engines"].items() if "fp8" in k and "precision:fp8" in k)
    assert eng_b is not eng_a and eng_b._suffix is copy and eng_b._prefill_layers() is copy
    d = _rel(b, a)
    print(f"window {window}: fp8 prefill + fp8 suffix weights vs fp8 prefill + bf16 suffix weights {d:.3e}")
    assert d < BOUND, d
    c = m.predict_action_diff(suffix_weights="fp8_as_bf16", **FP8, **kw)
    assert m.vlm.__dict__["_prefix_fp8"]["fp8"] is copy and _rel(c, b) < BOUND


def test_device_sampler_and_split_attention_on_an_fp8_prefill(dev, tiny):
    """sampler="device" promises the host loop's bits, with either attention launch; suffix_attention="split" is the same function up to
    summation order (the engines' bound)."""
    m, window, _, kw, _ = tiny
    host = m.predict_action_diff(**FP8, **kw)
    assert np.array_equal(m.predict_action_diff(sampler="device", **FP8, **kw), host)
    split = m.predict_action_diff(suffix_attention="split", **FP8, **kw)
    assert np.isfinite(split).all()
    assert np.array_equal(m.predict_action_diff(suffix_attention="split", sampler="device", **FP8, **kw), split)
    d = _rel(split, host)
    print(f"window {window}: fp8 prefill, split vs head attention {d:.3e}")
    assert d < BOUND, d


def test_samples_engine_on_an_fp8_prefill(dev, tiny):
    """predict_action_diff_samples(num_samples=3, prefill="compact", prefill_precision="fp8"): every sample within the bound of its own
    batch-1 fp8 call."""
    m, window, _, kw, _ = tiny
    T, N = window + 1, 3
    noise = torch.randn(N, T, 7, generator=torch.Generator().manual_seed(200 + window))
    skw = {k: v for k, v in kw.items() if k != "noise"}
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, **FP8, **skw)
    assert got.shape == (N, T, 7) and np.isfinite(got).all()
    singles = np.stack([m.predict_action_diff(noise=noise[n:n + 1], **FP8, **skw) for n in range(N)])
    d = [_rel(got[n], singles[n]) for n in range(N)]
    print(f"window {window}: fp8-prefill samples vs their fp8-prefill batch-1 calls {['%.2e' % v for v in d]}")
    assert max(d) < BOUND, d
    engines = m.vlm.__dict__["_prefix_engines_samples"]
    assert any("precision:fp8" in k and e._prefill_xq is not None for k, e in engines.items())


def test_weight_update_reaches_the_fp8_prefill(dev, tiny):
    """An in-place update of one decoder weight (mul_ bumps _version) changes the next fp8-prefill chunk; restoring it restores the bits."""
    m, _, _, kw, _ = tiny
    before = m.predict_action_diff(**FP8, **kw)
    w = m.vlm.llm_backbone.llm.model.layers[4].mlp.down_proj.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    changed = m.predict_action_diff(**FP8, **kw)
    with torch.no_grad():
        w.copy_(saved)
    restored = m.predict_action_diff(**FP8, **kw)
    assert not np.array_equal(changed, before) and np.array_equal(restored, before)


def test_fp8_prefill_refuses_without_the_compact_prefill(dev, tiny):
    m, _, inputs, kw, _ = tiny
    with pytest.raises(ValueError, match="compact"):
        m.predict_action_diff(prefill_precision="fp8", **kw)
    with pytest.raises(ValueError, match="prefill"):
        m.predict_action_diff(reuse_prefix=False, **FP8, **kw)
    ids, image, pc, proprio, _, _ = inputs
    with pytest.raises(NotImplementedError, match="prefill_precision"):
        m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, cur_robot_states=[proprio[0, 0].numpy()] * 2, input_ids=[ids] * 2,
                                    prefill_precision="fp8")
