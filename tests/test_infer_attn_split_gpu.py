"""GPU: MLA.predict_action_diff(suffix_attention="split") -- the sampler steps of PrefixCachedEps on mla_attn_chunk_split.

The mode changes the summation order of the suffix attention and nothing else: the chunk stays within the project's bound of the
whole-forward chunk (3e-2) and of the "head" chunk, one epsilon within 2e-2 of the eval forward; the captured pass replays the eager
bits; sampler="device" gives the host loop's bits; FP8 suffix weights and the compact prefill compose; the "head" engines are untouched."""
import numpy as np
import pytest
import torch

from conftest import fro_rel
from test_inference_chunk_gpu import infer_inputs as chunk_inputs
from test_inference_chunk_gpu import model_7b_dims  # noqa: F401 -- the module-scoped fixture of the chunk tests
from test_sampler_device_gpu import _engines, build_tiny, second_observation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny3(dev):
    return build_tiny(dev, 3)


@pytest.fixture(scope="module")
def tiny15(dev):
    return build_tiny(dev, 15)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _split_engines(m):
    return [e for e in _engines(m) if e.suffix_attention == "split"]


def _eps(dev, m, T, ids, image, pc, proprio, x, **mode):
    """(engine epsilon, whole-forward epsilon, engine) of one sampler call at t = 91."""
    from mla_amd import infer
    kw = dict(input_ids=ids.to(dev), images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    t = torch.tensor([91], device=dev)
    with torch.inference_mode():                                              # as predict_action_diff calls the engine
        _, eps_full = m.vlm(x.to(dev), t, **kw)
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, **mode, **kw)
        _, eps_c = eng(x.to(dev), t)
    return eps_c, eps_full, eng


@pytest.mark.parametrize("which", ["tiny3", "tiny15"], ids=["window3", "window15"])
def test_split_chunk_and_epsilon(dev, request, which, monkeypatch):
    from mla_amd import infer
    m, window, (ids, image, pc, proprio, noise, _), kw = request.getfixturevalue(which)
    T = window + 1
    x = noise[:1]
    full = m.predict_action_diff(reuse_prefix=False, noise=x, **kw)
    head = m.predict_action_diff(noise=x, **kw)
    split = m.predict_action_diff(noise=x, suffix_attention="split", **kw)
    assert split.shape == (T, 7) and np.isfinite(split).all()
    d_full, d_head = rel(split, full), rel(split, head)
    print(f"window {window}: split vs whole-forward chunk {d_full:.3e}, split vs head chunk {d_head:.3e}, head vs whole-forward {rel(head, full):.3e}")
    assert d_full < 3e-2 and d_head < 3e-2
    eng, = _split_engines(m)
    assert eng.R == T + 1 and eng._attn_ws is not None and eng.suffix_weights == "bf16" and eng.prefill_mode == "train"
    # a second observation: the same engine, the same captured pass
    gid = id(eng.graph)
    assert eng.graph is not None, eng.graph_error
    split2 = m.predict_action_diff(noise=x, suffix_attention="split", **second_observation(kw, image))
    assert _split_engines(m) == [eng] and id(eng.graph) == gid and not np.array_equal(split2, split)
    assert rel(split2, m.predict_action_diff(noise=x, **second_observation(kw, image))) < 3e-2
    # one epsilon at t = 91; the captured pass replays the eager launches' bits
    eps_s, eps_full, eng2 = _eps(dev, m, T, ids, image, pc, proprio, x, suffix_attention="split")
    assert eng2 is eng and eng.graph is not None and id(eng.graph) == gid
    e = fro_rel(eps_s, eps_full.float().cpu())
    print(f"window {window}: split epsilon vs eval forward {e:.3e}")
    assert e < 2e-2
    t = torch.tensor([91], device=dev)
    with torch.inference_mode():
        _, again = eng(x.to(dev), t)
        monkeypatch.setattr(infer, "_USE_GRAPH", False)
        _, eager = eng(x.to(dev), t)
        monkeypatch.undo()
    assert torch.equal(eps_s, again) and torch.equal(eps_s, eager)
    # the default path before and after: the same bits
    assert np.array_equal(m.predict_action_diff(noise=x, **kw), head)
    assert np.array_equal(m.predict_action_diff(noise=x, suffix_attention="head", **kw), head)
    assert all(e.suffix_attention == "head" and e._attn_ws is None for e in _engines(m) if e is not eng)


def test_device_sampler_gives_the_host_loops_bits(dev, tiny3):
    m, _, (_, _, _, _, noise, _), kw = tiny3
    host = m.predict_action_diff(noise=noise[1:2], suffix_attention="split", **kw)
    device = m.predict_action_diff(noise=noise[1:2], suffix_attention="split", sampler="device", **kw)
    assert np.array_equal(device, host)
    eng, = _split_engines(m)
    assert all(st.graph is not None for st in eng._ddim.values()) and eng._ddim and eng.graph_error is None


def test_fp8_weights_and_compact_prefill_compose(dev, tiny3):
    m, _, (_, _, _, _, noise, _), kw = tiny3
    x = noise[2:3]
    for extra in (dict(suffix_weights="fp8"), dict(prefill="compact"), dict(suffix_weights="fp8", prefill="compact", sampler="device")):
        head = m.predict_action_diff(noise=x, **extra, **kw)
        split = m.predict_action_diff(noise=x, suffix_attention="split", **extra, **kw)
        d = rel(split, head)
        print(f"{extra}: split vs head chunk {d:.3e}")
        assert np.isfinite(split).all() and d < 3e-2
    modes = {(e.suffix_weights, e.prefill_mode) for e in _split_engines(m)}
    assert ("fp8", "compact") in modes


def test_only_the_selected_attention_wrapper_is_called(dev, tiny3, monkeypatch):
    """Eager launches (no captured pass), so that every attention launch goes through its Python wrapper."""
    from mla_amd import hip, infer
    m, _, (_, _, _, _, noise, _), kw = tiny3
    calls = {"attn_decode": 0, "attn_chunk": 0, "attn_chunk_split": 0}

    def spy(name):
        real = getattr(hip, name)

        def wrapper(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return wrapper
    for name in calls:
        monkeypatch.setattr(hip, name, spy(name))
    monkeypatch.setattr(infer, "_USE_GRAPH", False)
    layers, steps = len(m.vlm.llm_backbone.llm.model.layers), 8
    for extra in (dict(), dict(suffix_weights="fp8")):
        for k in calls:
            calls[k] = 0
        m.predict_action_diff(noise=noise[:1], suffix_attention="split", **extra, **kw)
        assert calls == {"attn_decode": 0, "attn_chunk": 0, "attn_chunk_split": layers * steps}, (extra, calls)
        for k in calls:
            calls[k] = 0
        m.predict_action_diff(noise=noise[:1], **extra, **kw)
        assert calls["attn_chunk_split"] == 0 and calls["attn_decode"] + calls["attn_chunk"] == layers * steps, (extra, calls)


def test_split_errors(dev, tiny3, monkeypatch):
    import warnings
    from mla_amd import infer
    m, _, (_, _, _, _, noise, _), kw = tiny3
    with pytest.raises(ValueError, match="suffix_attention"):
        m.predict_action_diff(suffix_attention="bogus", **kw)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        m.predict_action_diff(suffix_attention="split", reuse_prefix=False, **kw)
    with pytest.raises(NotImplementedError, match="ragged / groups"):
        m.predict_action_diff_samples(num_samples=2, suffix_attention="split", **kw)
    one = m.predict_action_diff_samples(num_samples=1, noise=noise[:1], suffix_attention="split", **kw)          # forwarded
    assert np.array_equal(one[0], m.predict_action_diff(noise=noise[:1], suffix_attention="split", **kw))
    monkeypatch.setattr(infer.PrefixCachedEps, "MAX_ROWS", 4)                # R = 5 suffix rows: the engine does not serve the shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(ValueError, match="does not serve"):
            m.predict_action_diff(suffix_attention="split", noise=noise[:1], **kw)


@pytest.mark.parametrize("R", [2, 17])
def test_split_epsilon_at_7b_layer_dimensions(dev, model_7b_dims, R):  # noqa: F811
    """32 heads of 128: R = 2 is the shape mla_attn_decode serves in "head" mode, R = 17 mla_attn_chunk's; the plan splits both."""
    from mla_amd import hip
    m = model_7b_dims
    T = R - 1
    ids, image, pc, proprio, noise, starts = chunk_inputs(T)
    m.vlm.vision_tower_3d.fps_starts_override = starts
    eps_s, eps_full, eng = _eps(dev, m, T, ids, image, pc, proprio, noise, suffix_attention="split")
    assert eng.graph is not None, eng.graph_error
    assert eng.suffix_attention == "split" and hip.plan_attn_split(1, 32, R, eng.S_cap).splits > 1
    assert torch.isfinite(eps_s.float()).all()
    e = fro_rel(eps_s, eps_full.float().cpu())
    print(f"7B layer dimensions, R {R}, S_kv {eng.S_cap}: split epsilon vs eval forward {e:.3e}")
    assert e < 2e-2
