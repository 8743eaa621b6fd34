"""GPU: the device-resident DDIM loop -- mla_ddim_step / mla_sampler_rows (mla_amd/csrc/sampler.hip), _CachedEpsBase.sample_ddim
(mla_amd/infer.py) and MLA.predict_action_diff*(sampler="device").

The acceptance criterion is bit-identity, not a tolerance: every step of sampler="device" launches the kernels sampler="host" launches, in
the same order, and the DDIM update between them is the host loop's arithmetic one rounded operation at a time
(tests/test_sampler_device_host.py shows that on the CPU). So every comparison here is torch.equal / np.array_equal."""
import warnings

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N = 5


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", [(1, 1, 7), (3, 16, 7), (15, 17, 14)], ids=["n7", "n336", "n3570"])
def test_ddim_step_is_ddim_sample_per_step(dev, shape):
    """Steps 7 .. 0 of ddim8, chained: x, its bf16 cast and the counter after every launch; then a finished counter, stale counters and
    advance=0."""
    from mla_amd import hip
    from mla_amd.diffusion import create_diffusion
    d = create_diffusion("ddim8")
    steps = d.num_timesteps
    coef, ts = d.ddim_tables(dev)
    assert coef.shape == (steps, 4) and coef.is_cuda and ts.tolist() == list(d.timestep_map)
    g = torch.Generator().manual_seed(shape[1] * 100 + shape[2])
    x_ref = (torch.randn(*shape, generator=g) * 3.0).to(dev)
    x = x_ref.clone()
    xb = torch.full(shape, float("nan"), dtype=BF, device=dev)
    step = torch.full((1,), steps - 1, dtype=torch.int32, device=dev)
    for i in reversed(range(steps)):
        eps = (torch.randn(*shape, generator=g) * 3.0).to(BF).to(dev)
        t = torch.tensor([i] * shape[0], device=dev)
        want = d.ddim_sample(lambda xx, tt, eps=eps: (None, eps), x_ref, t, clip_denoised=False, model_kwargs={}, eta=0.0)["sample"]
        hip.ddim_step(x, eps, xb, coef, step)
        assert torch.equal(x, want), f"step {i}: max |diff| {float((x - want).abs().max()):.3e}"
        assert torch.equal(xb, want.to(BF)) and int(step.item()) == i - 1
        x_ref = want
    assert torch.isfinite(x).all() and float(x.abs().max()) > 0.1
    eps = torch.ones(shape, dtype=BF, device=dev)
    for stale in (-1, steps, -7, 1 << 30):                                   # outside the table: nothing is written, the counter stays
        step.fill_(stale)
        before, before_b = x.clone(), xb.clone()
        hip.ddim_step(x, eps, xb, coef, step)
        assert torch.equal(x, before) and torch.equal(xb, before_b) and int(step.item()) == stale
    step.fill_(3)
    t = torch.tensor([3] * shape[0], device=dev)
    want = d.ddim_sample(lambda xx, tt: (None, eps), x, t, clip_denoised=False, model_kwargs={}, eta=0.0)["sample"]
    hip.ddim_step(x, eps, xb, coef, step, advance=False)
    assert torch.equal(x, want) and torch.equal(xb, want.to(BF)) and int(step.item()) == 3


@pytest.mark.parametrize("G,T,H", [(1, 1, 256), (3, 16, 256), (15, 16, 384)])
def test_sampler_rows_is_the_cat_it_replaces(dev, G, T, H):
    from mla_amd import hip
    steps, R, SENT = 8, 1 + T, 777.0                                          # bf16-exact sentinel
    g = torch.Generator().manual_seed(G * 1000 + T * 10 + H)
    t_table = torch.randn(steps, H, generator=g).to(BF).to(dev)
    x_e = torch.randn(G, T, H, generator=g).to(BF).to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for s in (0, 7):
        h_in = torch.full(((G + 2) * R, H), SENT, dtype=BF, device=dev)      # capacity for two more groups
        step.fill_(s)
        hip.sampler_rows(h_in, t_table, x_e, step, G, T)
        want = torch.cat([t_table[s].expand(G, 1, H), x_e], dim=1).reshape(G * R, H)
        assert torch.equal(h_in[:G * R], want) and bool((h_in[G * R:] == SENT).all()) and int(step.item()) == s
        flat = torch.full_like(h_in, SENT)
        hip.sampler_rows(flat, t_table, x_e.reshape(G * T, H), step, G, T)    # the [G T, H] form of x_e
        assert torch.equal(flat, h_in)
    for stale in (-1, steps, 1 << 30):
        h_in = torch.full((G * R, H), SENT, dtype=BF, device=dev)
        step.fill_(stale)
        hip.sampler_rows(h_in, t_table, x_e, step, G, T)
        assert bool((h_in == SENT).all()) and int(step.item()) == stale
    with pytest.raises(ValueError):
        hip.sampler_rows(torch.zeros((G * R - 1, H), dtype=BF, device=dev), t_table, x_e, step, G, T)


# ------------------------------------------------------------------------------------------------ end to end, tiny model
def infer_inputs(T, tag):
    """The recipe of tests/test_infer_samples_gpu.py (copied: that file stays as it is)."""
    g = recipe._gen(tag)
    ids = torch.randint(3, 29000, (1, 20), generator=g)
    ids[0, 0] = 1
    ids = torch.cat([ids, torch.tensor([[29871]])], dim=1)
    image = torch.cat([torch.randn(1, 3, 672, 672, generator=g), torch.ones(1, 1, 672, 672)], dim=1)
    lo, hi = torch.tensor([0.0, -0.4, 0.75]), torch.tensor([0.6, 0.4, 1.25])
    pc = lo + (hi - lo) * torch.rand(1, 1024, 3, generator=g)
    proprio = torch.rand(1, 1, 7, generator=g) * 2 - 1
    starts = [torch.randint(0, 1024, (1,), generator=g), torch.randint(0, 512, (1,), generator=g)]
    noise = torch.randn(N, T, 7, generator=recipe._gen(tag + "_samples"))
    return ids, image, pc, proprio, noise, starts


def build_tiny(dev, window):
    """hidden 256, 9 layers, 2 heads of 128; window 3: R = 5 suffix rows per sample, window 15: R = 17."""
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
    inputs = infer_inputs(window + 1, f"infer_samples{window + 1}")
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    ids, image, pc, proprio, _, _ = inputs
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, num_ddim_steps=8)
    return m, window, inputs, kw


@pytest.fixture(scope="module")
def tiny3(dev):
    return build_tiny(dev, 3)


@pytest.fixture(scope="module")
def tiny15(dev):
    return build_tiny(dev, 15)


def second_observation(kw, image):
    return dict(kw, image=torch.cat([image[0, :3] * 0.5 + 0.1, image[0, 3:]]))


def both(dev, call, seed=1234):
    """call(sampler=...) under the same seed in both modes -> (host, device, equal generator state afterwards)."""
    out, after = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(seed)
        out[mode] = call(sampler=mode)
        after[mode] = torch.randn(4, device=dev)
    assert np.isfinite(out["host"]).all() and out["host"].shape == out["device"].shape
    return out["host"], out["device"], torch.equal(after["host"], after["device"])


def _engines(m, name="_prefix_engines"):
    return list(m.vlm.__dict__[name].values())


@pytest.mark.parametrize("which", ["tiny3", "tiny15"], ids=["window3", "window15"])
def test_predict_action_diff_device_is_host_bit_for_bit(dev, request, which):
    """Window 3 and 15, the initial sample drawn from the seeded generator; a second observation on the same engine exercises the counter
    reset and the reuse of the captured step; the first observation again gives the first result."""
    m, window, (_, image, _, _, noise, _), kw = request.getfixturevalue(which)
    host, device, rng = both(dev, lambda **s: m.predict_action_diff(**kw, **s))
    assert host.shape == (window + 1, 7) and np.array_equal(device, host) and rng
    eng, = [e for e in _engines(m) if e.suffix_weights == "bf16" and e.prefill_mode == "train"]
    st, = eng._ddim.values()
    gid = id(st.graph)
    assert st.graph is not None and eng.graph_error is None
    other = second_observation(kw, image)
    host2, device2, rng2 = both(dev, lambda **s: m.predict_action_diff(**other, **s), seed=99)
    assert np.array_equal(device2, host2) and rng2 and not np.array_equal(host2, host)
    assert id(st.graph) == gid and list(eng._ddim.values()) == [st]
    assert np.array_equal(m.predict_action_diff(noise=noise[1:2], sampler="device", **kw), m.predict_action_diff(noise=noise[1:2], **kw))
    torch.manual_seed(1234)
    assert np.array_equal(m.predict_action_diff(sampler="device", **kw), host)


def test_samples_device_is_host_bit_for_bit(dev, tiny3):
    m, window, (_, image, _, _, noise, _), kw = tiny3
    host, device, rng = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=N, **kw, **s))
    assert host.shape == (N, window + 1, 7) and np.array_equal(device, host) and rng
    other = second_observation(kw, image)
    host2, device2, _ = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=N, noise=noise, **other, **s))
    assert np.array_equal(device2, host2) and not np.array_equal(host2, host)
    one_h, one_d, _ = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=1, noise=noise[:1], **kw, **s))   # forwarded
    assert np.array_equal(one_d, one_h)


def test_sub_batched_samples_keep_one_state_per_group_count(dev, tiny3, monkeypatch):
    """MAX_ROWS = 2 R: passes of 2 + 2 + 1 groups on one engine -- one captured step per distinct G, the same bits as the host loop."""
    from mla_amd import infer
    m, window, (_, _, _, _, noise, _), kw = tiny3
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_ROWS", 2 * (window + 2))
    host, device, _ = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=N, noise=noise, **kw, **s))
    assert np.array_equal(device, host)
    eng, = [e for key, e in m.vlm.__dict__["_prefix_engines_samples"].items() if key[2] == 2]
    assert sorted(b for b, _ in eng._ddim) == [1, 2] and all(st.graph is not None for st in eng._ddim.values())


def ragged_batch(inputs, B=3):
    """B observations with prompts of 21, 14 and 27 ids (ragged), their own images, proprio values and FPS start indices."""
    ids0, image, pc, proprio, _, starts = inputs
    g = recipe._gen("sampler_device_batch")
    ids, images, pcs, proprios = [ids0[0]], [image[0]], [pc[0].numpy()], [proprio[0, 0].numpy()]
    for b, L in zip(range(1, B), (14, 27)):
        row = torch.randint(3, 29000, (L - 1,), generator=g)
        row[0] = 1
        ids.append(torch.cat([row, torch.tensor([29871])]))
        images.append(torch.cat([image[0, :3] * (1.0 - 0.2 * b) + 0.05 * b, image[0, 3:]]))
        pcs.append((pc[0] * (1.0 - 0.01 * b)).numpy())
        proprios.append((proprio[0, 0] * (1.0 - 0.3 * b)).numpy())
    s = [torch.cat([starts[0], torch.randint(0, 1024, (B - 1,), generator=g)]), torch.cat([starts[1], torch.randint(0, 512, (B - 1,), generator=g)])]
    return dict(images=images, pointclouds=pcs, cur_robot_states=proprios, input_ids=ids, num_ddim_steps=8), s


def test_batch_device_is_host_bit_for_bit(dev, tiny3):
    """Three ragged prompts, without and with num_samples=3."""
    m, window, inputs, _ = tiny3
    bkw, starts = ragged_batch(inputs)
    tower = m.vlm.vision_tower_3d
    saved = tower.fps_starts_override
    try:
        tower.fps_starts_override = starts
        host, device, rng = both(dev, lambda **s: m.predict_action_diff_batch(**bkw, **s))
        assert host.shape == (3, window + 1, 7) and np.array_equal(device, host) and rng
        assert not np.array_equal(host[0], host[1])
        host, device, rng = both(dev, lambda **s: m.predict_action_diff_batch(num_samples=3, **bkw, **s))
        assert host.shape == (3, 3, window + 1, 7) and np.array_equal(device, host) and rng
        host2, device2, _ = both(dev, lambda **s: m.predict_action_diff_batch(num_samples=3, **bkw, **s), seed=5)     # the engines again
        assert np.array_equal(device2, host2) and not np.array_equal(host2, host)
    finally:
        tower.fps_starts_override = saved
    for name in ("_prefix_engines_batched", "_prefix_engines_batch_samples"):
        for eng in _engines(m, name):
            assert eng.graph_error is None and all(st.graph is not None for st in eng._ddim.values()) and len(eng._ddim) == 1


def test_fp8_suffix_weights_and_compact_prefill_compose(dev, tiny3):
    m, _, (_, _, _, _, noise, _), kw = tiny3
    for extra in (dict(suffix_weights="fp8"), dict(prefill="compact")):
        host, device, rng = both(dev, lambda **s: m.predict_action_diff(**kw, **extra, **s))
        assert np.array_equal(device, host) and rng, extra
    modes = {(e.suffix_weights, e.prefill_mode) for e in _engines(m) if e._ddim}        # the device loop ran on those engines
    assert {("fp8", "train"), ("bf16", "compact")} <= modes, modes
    assert not np.array_equal(m.predict_action_diff(noise=noise[:1], sampler="device", suffix_weights="fp8", **kw),
                              m.predict_action_diff(noise=noise[:1], sampler="device", **kw))
    host, device, _ = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=3, suffix_weights="fp8", **kw, **s))
    assert np.array_equal(device, host)


def test_eager_steps_equal_the_captured_step(dev, tiny3, monkeypatch):
    from mla_amd import infer
    m, _, (_, _, _, _, noise, _), kw = tiny3
    graphed = m.predict_action_diff(noise=noise[2:3], sampler="device", **kw)
    eng, = [e for e in _engines(m) if e.suffix_weights == "bf16" and e.prefill_mode == "train"]
    assert eng.graph_error is None and all(st.graph is not None for st in eng._ddim.values())
    monkeypatch.setattr(infer, "_USE_GRAPH", False)
    eager = m.predict_action_diff(noise=noise[2:3], sampler="device", **kw)
    assert eng.graph_error is not None and "MLA_INFER_GRAPH" in eng.graph_error
    monkeypatch.undo()
    assert np.array_equal(eager, graphed)
    assert np.array_equal(m.predict_action_diff(noise=noise[2:3], sampler="device", **kw), graphed) and eng.graph_error is None
    assert np.array_equal(graphed, m.predict_action_diff(noise=noise[2:3], **kw))


def test_device_sampler_follows_the_weights(dev, tiny3):
    """In-place updates (mul_ bumps _version, the address stays) of a final_layer and of a t_embedder weight change the device result
    exactly as they change the host result; restoring the weight restores the bits."""
    m, _, (_, _, _, _, noise, _), kw = tiny3
    run = lambda **s: m.predict_action_diff(noise=noise[3:4], **kw, **s)     # noqa: E731
    before = run(sampler="device")
    assert np.array_equal(before, run())
    for w in (m.vlm.final_layer.mlp.fc1.weight, m.vlm.t_embedder.mlp[2].weight):
        saved = w.detach().clone()
        with torch.no_grad():
            w.mul_(1.5)
        changed_d, changed_h = run(sampler="device"), run()
        with torch.no_grad():
            w.copy_(saved)
        assert np.array_equal(changed_d, changed_h) and not np.array_equal(changed_d, before)
        assert np.array_equal(run(sampler="device"), before)


def test_sample_ddim_never_waits_for_the_device(dev, tiny3):
    """Under torch's sync debug mode "error" a call that makes the host wait for the device raises. sample_ddim does not (after one
    warm-up call: the capture and the table builds may wait); the host loop on the same engine does -- the control without which this
    test would show nothing."""
    from mla_amd import infer
    from mla_amd.diffusion import create_diffusion
    m, window, (ids, image, pc, proprio, noise, _), _ = tiny3
    T = window + 1
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("torch.cuda.set_sync_debug_mode(\"error\") does not flag .item() on a device tensor in this build")
    diffusion = create_diffusion("ddim8")
    x0 = noise[:1].to(dev)
    kw = dict(images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    with torch.inference_mode():
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, input_ids=ids.to(dev), **kw)
        warm = eng.sample_ddim(x0, diffusion)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = eng.sample_ddim(x0, diffusion)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert eng.graph_error is None
        host_raised = False
        torch.cuda.set_sync_debug_mode("error")
        try:
            diffusion.ddim_sample_loop(eng, x0.shape, x0, clip_denoised=False, model_kwargs={}, eta=0.0)
        except RuntimeError:
            host_raised = True
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert host_raised, "the host loop did not wait for the device under the sync debug mode: this test shows nothing"
        want = diffusion.ddim_sample_loop(eng, x0.shape, x0, clip_denoised=False, model_kwargs={}, eta=0.0)
    assert torch.equal(got, want) and torch.equal(warm, want) and got.dtype == torch.float32 and got.shape == (1, T, 7)


def test_device_sampler_errors(dev, tiny3, monkeypatch):
    from mla_amd import infer
    m, _, (_, _, _, _, noise, _), kw = tiny3
    with pytest.raises(ValueError, match="sampler"):
        m.predict_action_diff(sampler="bogus", **kw)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        m.predict_action_diff(sampler="device", reuse_prefix=False, **kw)
    with pytest.raises(ValueError, match="DDIM"):
        m.predict_action_diff(sampler="device", use_ddim=False, **kw)
    with pytest.raises(ValueError, match="DDIM"):
        m.predict_action_diff_samples(num_samples=2, sampler="device", **dict(kw, num_ddim_steps=None))
    monkeypatch.setattr(infer.PrefixCachedEps, "MAX_ROWS", 4)                # R = 5 suffix rows: the engine does not serve the shape
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_R", 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(ValueError, match="does not serve"):
            m.predict_action_diff(sampler="device", noise=noise[:1], **kw)
        with pytest.raises(ValueError, match="does not serve"):
            m.predict_action_diff_samples(num_samples=2, sampler="device", noise=noise[:2], **kw)
        assert m.predict_action_diff(noise=noise[:1], **kw).shape == (4, 7)  # "host" still loops over whole forwards
    with torch.inference_mode():
        eng = _engines(m)[0]
        with pytest.raises(ValueError, match="eta"):
            m.ddim_diffusion.ddim_tables(dev, eta=1.0)
        with pytest.raises(AssertionError):
            eng.sample_ddim(torch.zeros(eng.B + 1, eng.T, 7, device=dev), m.ddim_diffusion)
