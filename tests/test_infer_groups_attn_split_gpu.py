"""GPU: groups_attention="split" on MLA.predict_action_diff_samples and MLA.predict_action_diff_batch (with and without num_samples) --
the sampler steps of SampleGroupsEps, BatchedPrefixCachedEps and BatchedSampleGroupsEps on mla_attn_groups_split.

The mode changes the summation order of the suffix attention and nothing else: every route stays within the project's bound (3e-2, as
tests/test_infer_attn_split_gpu.py) of its "head" result, "head" is the call without the keyword bit for bit, only the selected attention
wrapper is launched, sampler="device" gives the host loop's bits, FP8 suffix weights and the compact prefill compose, and one engine with
one captured pass serves a second mix of prompt lengths. Tiny model: 2 heads, 9 layers, window 3 (R = 5), prefixes of about 535 rows --
nine key tiles, which the library's plan cuts into 3 ranges on all three routes."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from oracle import recipe
from test_sampler_device_gpu import _engines, build_tiny, ragged_batch, second_observation

pytestmark = pytest.mark.gpu

ROUTES = ("samples", "batch", "batch_samples")
STORE = {"samples": "_prefix_engines_samples", "batch": "_prefix_engines_batched", "batch_samples": "_prefix_engines_batch_samples"}


@pytest.fixture(scope="module")
def tiny3(dev):
    return build_tiny(dev, 3)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@contextlib.contextmanager
def _fps_starts(m, starts):
    tower = m.vlm.vision_tower_3d
    saved = tower.fps_starts_override
    tower.fps_starts_override = starts
    try:
        yield
    finally:
        tower.fps_starts_override = saved


def _route(tiny, route, other=False):
    """-> call(**modes) of one route on fixed inputs and noise; other=True: another observation (samples) or another mix of prompt
    lengths in the same capacity bucket (the batched routes: 21 / 18 / 24 ids instead of 21 / 14 / 27)."""
    m, window, inputs, kw = tiny
    T, noise = window + 1, inputs[4]
    if route == "samples":
        skw = second_observation(kw, inputs[1]) if other else kw
        return lambda **mode: m.predict_action_diff_samples(num_samples=3, noise=noise[:3], **skw, **mode)
    bkw, starts = ragged_batch(inputs)
    if other:
        ids = list(bkw["input_ids"])
        g = recipe._gen("groups_attn_split_mix")
        ids[1] = torch.cat([ids[1][:-1], torch.randint(3, 29000, (4,), generator=g), ids[1][-1:]])
        ids[2] = torch.cat([ids[2][:23], ids[2][-1:]])
        assert [len(r) for r in ids] == [21, 18, 24]
        bkw = dict(bkw, input_ids=ids)
    if route == "batch":
        extra = dict(noise=noise[:3])
    else:
        extra = dict(num_samples=2, noise=torch.randn(3, 2, T, 7, generator=recipe._gen("groups_attn_split_bs")))

    def call(**mode):
        with _fps_starts(m, starts):
            return m.predict_action_diff_batch(**bkw, **extra, **mode)
    return call


def _split_engines(m, route):
    return [e for e in _engines(m, STORE[route]) if e.suffix_attention == "split"]


@pytest.mark.parametrize("route", ROUTES)
def test_split_on_every_route(dev, tiny3, route):
    m = tiny3[0]
    call = _route(tiny3, route)
    plain = call()
    head = call(groups_attention="head")
    split = call(groups_attention="split")
    assert split.shape == plain.shape and np.isfinite(split).all()
    assert np.array_equal(head, plain)
    d = rel(split, head)
    print(f"{route}: split vs head {d:.3e}")
    assert d < 3e-2 and not np.array_equal(split, head)
    eng, = _split_engines(m, route)
    S_max, plan = eng.attn_plan
    print(f"{route}: S_max {S_max}, plan {plan}")
    assert plan[0] > 1 and eng._attn_ws is not None and eng.graph is not None, eng.graph_error
    assert all(e._attn_ws is None for e in _engines(m, STORE[route]) if e is not eng)
    # another observation / another mix of lengths in the bucket: the same engine, the same captured pass
    gid = id(eng.graph)
    other = _route(tiny3, route, other=True)
    split2 = other(groups_attention="split")
    assert _split_engines(m, route) == [eng] and id(eng.graph) == gid and not np.array_equal(split2, split)
    assert rel(split2, other()) < 3e-2
    assert np.array_equal(call(groups_attention="split"), split)             # and the first inputs again: the first bits
    assert np.array_equal(call(), plain)


@pytest.mark.parametrize("route", ROUTES)
def test_only_the_selected_attention_wrapper_is_called(dev, tiny3, route, monkeypatch):
    """Eager launches (no captured pass), so that every attention launch goes through its Python wrapper."""
    from mla_amd import hip, infer
    m = tiny3[0]
    calls = {"attn_groups_split": 0, "attn_chunk_groups": 0, "attn_chunk_ragged": 0, "attn_chunk_ragged_groups": 0}

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
    head_form = {"samples": "attn_chunk_groups", "batch": "attn_chunk_ragged", "batch_samples": "attn_chunk_ragged_groups"}[route]
    call = _route(tiny3, route)
    call(groups_attention="split")
    assert calls == dict.fromkeys(calls, 0) | {"attn_groups_split": layers * steps}, calls
    for k in calls:
        calls[k] = 0
    call()
    assert calls == dict.fromkeys(calls, 0) | {head_form: layers * steps}, calls


@pytest.mark.parametrize("route", ROUTES)
def test_device_sampler_gives_the_host_loops_bits(dev, tiny3, route):
    call = _route(tiny3, route)
    host = call(groups_attention="split")
    device = call(groups_attention="split", sampler="device")
    assert np.array_equal(device, host)
    eng, = _split_engines(tiny3[0], route)
    assert eng._ddim and all(st.graph is not None for st in eng._ddim.values()) and eng.graph_error is None


@pytest.mark.parametrize("route,extra", [("samples", dict(suffix_weights="fp8")), ("batch_samples", dict(suffix_weights="fp8")),
                                         ("samples", dict(prefill="compact"))], ids=["samples-fp8", "batch_samples-fp8", "samples-compact"])
def test_fp8_weights_and_compact_prefill_compose(dev, tiny3, route, extra):
    call = _route(tiny3, route)
    head = call(**extra)
    split = call(groups_attention="split", **extra)
    d = rel(split, head)
    print(f"{route} {extra}: split vs head {d:.3e}")
    assert np.isfinite(split).all() and d < 3e-2 and not np.array_equal(split, head)
    modes = {(e.suffix_weights, e.prefill_mode) for e in _split_engines(tiny3[0], route)}
    assert (extra.get("suffix_weights", "bf16"), extra.get("prefill", "train")) in modes


def test_one_sample_is_forwarded_as_suffix_attention(dev, tiny3):
    m, _, (_, _, _, _, noise, _), kw = tiny3
    want = m.predict_action_diff(noise=noise[:1], suffix_attention="split", **kw)
    one = m.predict_action_diff_samples(num_samples=1, noise=noise[:1], groups_attention="split", **kw)
    assert np.array_equal(one[0], want)
    bkw = dict(images=[kw["image"]], pointclouds=[kw["pointcloud"]], cur_robot_states=[kw["cur_robot_state"]], input_ids=[kw["input_ids"][0]],
               num_ddim_steps=8)
    assert np.array_equal(m.predict_action_diff_batch(noise=noise[:1], groups_attention="split", **bkw)[0], want)
    assert np.array_equal(m.predict_action_diff_batch(num_samples=1, noise=noise[:1][None], groups_attention="split", **bkw)[0, 0], want)


@pytest.mark.parametrize("route", ROUTES)
def test_split_on_an_unserved_shape_is_an_error_not_a_warning(dev, tiny3, route, monkeypatch):
    from mla_amd import infer
    monkeypatch.setattr(infer._RowGemmEps, "MAX_R", 4)                       # R = 5 suffix rows: the engines do not serve the shape
    call = _route(tiny3, route)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="does not serve"):
            call(groups_attention="split")
    with pytest.raises(ValueError, match="groups_attention"):
        call(groups_attention="bogus")
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        call(groups_attention="split", reuse_prefix=False)
