"""GPU: the opt-in compact prefill of the cached-prefix engines (MLA.predict_action_diff(prefill="compact"), mla_amd/infer.py
_compact_prefill on the row-sized GEMMs of mla_amd/csrc/prefill.hip) against the whole-forward sampler, the default "train" prefill and
an fp32 oracle of the decoder layers; the default path stays bit for bit what it was."""
import numpy as np
import pytest
import torch

from conftest import fro_rel
from oracle import recipe
from oracle import torch_oracle as TO

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BOUND = 3e-2                                             # the cached-prefix engines' bound against the whole-forward sampler


def infer_inputs(T, tag=None):
    g = recipe._gen(tag or f"infer_chunk{T}")
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


@pytest.fixture(scope="module", params=[1, 15], ids=["window1", "window15"])
def tiny(request, dev):
    """hidden 256, 9 layers, 2 heads of 128; window 1: R = 3 suffix rows, window 15: R = 17; fixed noise and FPS start indices."""
    window = request.param
    m = build_model(dev, window)
    inputs = infer_inputs(window + 1)
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    ids, image, pc, proprio, noise, _ = inputs
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, noise=noise, num_ddim_steps=8)
    yield m, window, inputs, kw
    del m
    torch.cuda.empty_cache()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_compact_chunk_matches_whole_forward_and_train_and_leaves_the_default_alone(dev, tiny):
    """prefill="compact" vs the whole-forward sampler and vs the default prefill: within 3e-2 per chunk (measured on MI355X, tiny model:
    see the printed figures). prefill="train" IS the call without the argument, before and after a compact call."""
    m, window, _, kw = tiny
    default = m.predict_action_diff(**kw)
    assert np.array_equal(m.predict_action_diff(prefill="train", **kw), default)
    full = m.predict_action_diff(reuse_prefix=False, **kw)
    compact = m.predict_action_diff(prefill="compact", **kw)
    assert compact.shape == (window + 1, 7) and np.isfinite(compact).all()
    assert np.array_equal(m.predict_action_diff(prefill="train", **kw), default)
    assert np.array_equal(m.predict_action_diff(**kw), default)
    d_full, d_train, d_train_full = _rel(compact, full), _rel(compact, default), _rel(default, full)
    msg = (f"window {window}: compact vs whole-forward {d_full:.3e}, compact vs train {d_train:.3e} (train vs whole-forward "
           f"{d_train_full:.3e}), bound {BOUND}")
    print(msg)
    assert d_full < BOUND, msg
    assert d_train < BOUND, msg
    engines = m.vlm.__dict__["_prefix_engines"]
    comp = [e for k, e in engines.items() if "prefill:compact" in k]
    assert len(comp) == 1 and comp[0].prefill_mode == "compact" and comp[0]._prefill_ws is not None
    assert all(e._prefill_ws is None for k, e in engines.items() if "prefill:compact" not in k)
    assert np.array_equal(m.predict_action_diff(prefill="compact", **kw), compact)          # deterministic


def _engine_kwargs(dev, inputs):
    ids, image, pc, proprio, _, _ = inputs
    return dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")


def _oracle_cache_rows(eng, prefix):
    """fp32 oracle (oracle/torch_oracle.py, CPU) of every layer's post-RoPE q|k|v rows for the prefix rows [1, S_p, H]."""
    x = prefix.float().cpu()
    S_p, nh = x.shape[1], eng.nheads
    D = x.shape[2] // nh
    cos, sin = TO.rope_tables(S_p, D)
    names = ("input_layernorm.weight", "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
             "self_attn.o_proj.weight", "post_attention_layernorm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
             "mlp.down_proj.weight")
    rows = []
    for w in eng._weights():
        p = {n: t.detach().float().cpu() for n, t in zip(names, w)}
        h = TO.rmsnorm(x, p[names[0]], eng.eps)
        q, k, v = (torch.nn.functional.linear(h, p[n]).view(1, S_p, nh, D).transpose(1, 2) for n in names[1:4])
        q, k = TO.apply_rope(q, k, cos, sin)
        rows.append(torch.cat([t.transpose(1, 2).reshape(S_p, nh * D) for t in (q, k, v)], dim=1))
        x = TO.decoder_layer(x, p, cos, sin, nh, eng.eps)
    return rows


def test_cache_rows_against_the_fp32_oracle_layers(dev, tiny):
    """Per layer, the cache rows [:S_p] of the compact engine are as close to the fp32 oracle's post-RoPE q|k|v as the train engine's:
    max|compact - oracle| <= 2 x max|train - oracle| (the existing prefill is the measure). The two caches differ by rounding only."""
    from mla_amd import infer
    m, window, inputs, _ = tiny
    T = window + 1
    kw = _engine_kwargs(dev, inputs)
    with torch.inference_mode():
        eng_t = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **kw)
        eng_c = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, prefill="compact", **kw)
        k = infer.PrefixCachedEps._splice_position(kw["input_ids"])
        prefix = eng_t._prefix_rows(kw["input_ids"], k, kw["images"], kw["point_cloud"], kw["camera_name"], kw["proprio"])
    assert eng_t is not eng_c and eng_t.S_p == eng_c.S_p == prefix.shape[1]
    S_p = eng_t.S_p
    with torch.no_grad():
        oracle = _oracle_cache_rows(eng_t, prefix)
    worst = 0.0
    for l, (ct, cc, ref) in enumerate(zip(eng_t.cache, eng_c.cache, oracle)):
        rt, rc = ct[0, :S_p].float().cpu(), cc[0, :S_p].float().cpu()
        assert torch.isfinite(rc).all()
        e_t, e_c = float((rt - ref).abs().max()), float((rc - ref).abs().max())
        worst = max(worst, e_c / e_t)
        print(f"window {window} layer {l}: max|train - oracle| {e_t:.4e}, max|compact - oracle| {e_c:.4e}, "
              f"max|compact - train| {float((rc - rt).abs().max()):.4e}")
        assert e_c <= 2 * e_t, (l, e_c, e_t)
    print(f"window {window}: worst compact / train error ratio over the layers {worst:.3f}")


def test_samples_engine_with_compact_prefill(dev, tiny):
    """predict_action_diff_samples(num_samples=3, prefill="compact"): every sample within the bound of its own compact batch-1 call."""
    m, window, inputs, kw = tiny
    T, N = window + 1, 3
    g = torch.Generator().manual_seed(100 + window)
    noise = torch.randn(N, T, 7, generator=g)
    skw = {k: v for k, v in kw.items() if k != "noise"}
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, prefill="compact", **skw)
    assert got.shape == (N, T, 7) and np.isfinite(got).all()
    singles = np.stack([m.predict_action_diff(noise=noise[n:n + 1], prefill="compact", **skw) for n in range(N)])
    d = [_rel(got[n], singles[n]) for n in range(N)]
    print(f"window {window}: compact samples vs their compact batch-1 calls {['%.2e' % v for v in d]}")
    assert max(d) < BOUND, d
    engines = m.vlm.__dict__["_prefix_engines_samples"]
    assert any("prefill:compact" in k and e._prefill_ws is not None for k, e in engines.items())


def test_fp8_suffix_weights_on_a_compact_prefill(dev, tiny):
    """suffix_weights="fp8" with prefill="compact": within the fp8 engine's bound (3e-2 per chunk) of its own fp8 "train" call."""
    m, window, _, kw = tiny
    fp8_train = m.predict_action_diff(suffix_weights="fp8", **kw)
    fp8_compact = m.predict_action_diff(suffix_weights="fp8", prefill="compact", **kw)
    assert np.isfinite(fp8_compact).all()
    d = _rel(fp8_compact, fp8_train)
    print(f"window {window}: fp8 + compact vs fp8 + train {d:.3e}")
    assert d < BOUND, d
    assert np.array_equal(m.predict_action_diff(suffix_weights="fp8", **kw), fp8_train)


def test_engine_key_and_graph_reuse(dev, tiny):
    """A second observation on the same compact engine re-runs the prefill and replays the SAME captured graph; the "train" and
    "compact" engines live side by side under different keys."""
    m, window, inputs, kw = tiny
    m.vlm.__dict__.pop("_prefix_engines", None)
    first = m.predict_action_diff(prefill="compact", **kw)
    engines = m.vlm.__dict__["_prefix_engines"]
    (key, eng), = engines.items()
    assert "prefill:compact" in key and eng.graph is not None, eng.graph_error
    graph = eng.graph
    ids, image, pc, proprio, noise, _ = inputs
    other = dict(kw, image=image[0].flip(-1), cur_robot_state=-proprio[0, 0].numpy())
    second = m.predict_action_diff(prefill="compact", **other)
    assert len(engines) == 1 and engines[key] is eng and eng.graph is graph
    assert not np.array_equal(first, second)
    assert np.array_equal(m.predict_action_diff(prefill="compact", **kw), first) and eng.graph is graph
    m.predict_action_diff(**kw)
    assert len(engines) == 2 and sum("prefill:compact" in k for k in engines) == 1
    train = next(e for k, e in engines.items() if "prefill:compact" not in k)
    assert train is not eng and train.prefill_mode == "train" and train.graph is not None and train.graph is not graph


def test_compact_refuses_without_the_cached_prefix(dev, tiny):
    m, window, _, kw = tiny
    with pytest.raises(ValueError, match="prefill"):
        m.predict_action_diff(prefill="compact", reuse_prefix=False, **kw)
    with pytest.raises(ValueError, match="prefill"):
        m.predict_action_diff(prefill="fast", **kw)
    ids, image, pc, proprio, noise, _ = tiny[2]
    with pytest.raises(NotImplementedError, match="compact"):
        m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, cur_robot_states=[proprio[0, 0].numpy()] * 2, input_ids=[ids] * 2,
                                    prefill="compact")


def test_compact_epsilon_at_7b_layer_dimensions(dev):
    """Two decoder layers at 7B widths (hidden 4096, intermediate 11008, 32 heads of 128, ~535 prefix rows): the shapes the kernels are
    sized for, the o and down projections on the split-K path. One cached epsilon against the eval forward, the bound of the existing
    7B-dimension test (2e-2)."""
    from mla_amd import hip, infer
    m = build_model(dev, 15, token_size=4096, hidden_size=4096, intermediate_size=11008, num_attention_heads=32, num_hidden_layers=2)
    T = 16
    inputs = infer_inputs(T)
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    kw = _engine_kwargs(dev, inputs)
    noise = inputs[4].to(dev)
    with torch.inference_mode():
        _, eps_full = m.vlm(noise, torch.tensor([91], device=dev), **kw)
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, prefill="compact", **kw)
        _, eps_c = eng(noise, torch.tensor([91], device=dev))
        eng_t = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **kw)
        _, eps_t = eng_t(noise, torch.tensor([91], device=dev))
    assert hip.plan_gemm_prefill(eng.S_p, 4096, 4096).split > 1 and hip.plan_gemm_prefill(eng.S_p, 4096, 11008).split > 1
    assert eng._prefill_ws.numel() >= hip.gemm_prefill_ws_bytes(eng.S_p, 4096, 11008)
    e_c, e_t = fro_rel(eps_c, eps_full.float().cpu()), fro_rel(eps_t, eps_full.float().cpu())
    print(f"7B widths, S_p {eng.S_p}: compact epsilon vs eval forward {e_c:.3e} (train {e_t:.3e})")
    assert torch.isfinite(eps_c.float()).all() and e_c < 2e-2
    del m
    torch.cuda.empty_cache()
