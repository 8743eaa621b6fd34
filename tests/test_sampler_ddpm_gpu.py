"""GPU: the device-resident DDPM loop -- mla_ddpm_step (mla_amd/csrc/sampler.hip), _CachedEpsBase.sample_ddpm (mla_amd/infer.py) and
MLA.predict_action_diff*(use_ddim=False, ddpm_sampler="device").

The acceptance criterion is bit-identity, not a tolerance: every step of ddpm_sampler="device" launches the kernels ddpm_sampler="host"
launches, in the same order, the posterior update between them is the host loop's arithmetic one rounded operation at a time, and the
steps' normal variates are the host loop's own draws, made up front (tests/test_sampler_ddpm_host.py shows both on the CPU). So every
comparison here is torch.equal / np.array_equal."""
import warnings

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N = 5


# ------------------------------------------------------------------------------------------------ kernel
def _p_sample_with(d, x, eps, i, noise):
    """p_sample(...)["sample"] of step i fed the given eps and the given noise: randn_like is the one draw p_sample makes, so the
    noise is handed over by patching it for the call."""
    real = torch.randn_like
    t = torch.tensor([i] * x.shape[0], device=x.device)
    torch.randn_like = lambda like, *a, **k: noise.view_as(like)
    try:
        return d.p_sample(lambda xx, tt: (None, eps), x, t, clip_denoised=False, model_kwargs={})["sample"]
    finally:
        torch.randn_like = real


@pytest.mark.parametrize("shape", [(1, 1, 7), (3, 16, 7), (15, 17, 14)], ids=["n7", "n336", "n3570"])
@pytest.mark.parametrize("respacing,runs", [("10", [range(9, -1, -1)]), ("", [range(99, 94, -1), range(4, -1, -1)])], ids=["steps10", "steps100"])
def test_ddpm_step_is_p_sample_per_step(dev, respacing, runs, shape):
    """All steps of the respaced 10-step process, the last and the first 5 of the 100-step one, chained: x, its bf16 cast and the counter
    after every launch (step 0 with a non-zero noise row: 0 * noise is added); then stale counters, advance=0 and the wrapper's errors."""
    from mla_amd import hip
    from mla_amd.diffusion import create_diffusion
    d = create_diffusion(respacing)
    steps, n = d.num_timesteps, shape[0] * shape[1] * shape[2]
    coef, ts = d.ddpm_tables(dev)
    assert coef.shape == (steps, 5) and coef.is_cuda and ts.tolist() == list(d.timestep_map) and float(coef[0, 4]) == 0.0
    g = torch.Generator().manual_seed(shape[1] * 100 + shape[2] + steps)
    noise = torch.randn(steps, n, generator=g).to(dev)
    assert float(noise[0].abs().min()) > 0.0
    x_ref = (torch.randn(*shape, generator=g) * 3.0).to(dev)
    x = x_ref.clone()
    xb = torch.full(shape, float("nan"), dtype=BF, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for run in runs:
        step.fill_(run[0])
        for i in run:
            eps = (torch.randn(*shape, generator=g) * 3.0).to(BF).to(dev)
            want = _p_sample_with(d, x_ref, eps, i, noise[i])
            hip.ddpm_step(x, eps, xb, coef, noise, step)
            assert torch.equal(x, want), f"step {i}: max |diff| {float((x - want).abs().max()):.3e}"
            assert torch.equal(torch.signbit(x), torch.signbit(want))
            assert torch.equal(xb, want.to(BF)) and int(step.item()) == i - 1
            x_ref = want
    assert torch.isfinite(x).all() and float(x.abs().max()) > 0.1
    eps = torch.ones(shape, dtype=BF, device=dev)
    for stale in (-1, steps, -7, 1 << 30):                                   # outside the tables: nothing is written, the counter stays
        step.fill_(stale)
        before, before_b = x.clone(), xb.clone()
        hip.ddpm_step(x, eps, xb, coef, noise, step)
        assert torch.equal(x, before) and torch.equal(xb, before_b) and int(step.item()) == stale
    step.fill_(3)
    want = _p_sample_with(d, x, eps, 3, noise[3])
    hip.ddpm_step(x, eps, xb, coef, noise, step, advance=False)
    assert torch.equal(x, want) and torch.equal(xb, want.to(BF)) and int(step.item()) == 3
    for bad in (noise[:, :-1].contiguous(), noise[1:], noise.view(-1), noise.t(), torch.zeros(steps, n + 1, device=dev)):
        with pytest.raises(ValueError):
            hip.ddpm_step(x, eps, xb, coef, bad, step)
    with pytest.raises(TypeError):
        hip.ddpm_step(x, eps, xb, coef, noise.double(), step)
    with pytest.raises(ValueError):
        hip.ddpm_step(x, eps, xb, coef[:, :4].contiguous(), noise, step)     # the DDIM table
    assert torch.equal(x, want) and int(step.item()) == 3                    # no launch behind a refused call


# ------------------------------------------------------------------------------------------------ end to end, tiny model
def infer_inputs(T, tag):
    """The recipe of tests/test_sampler_device_gpu.py (copied: that file stays as it is)."""
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
    """hidden 256, 9 layers, 2 heads of 128; window 3: R = 5 suffix rows per sample, window 15: R = 17. The DDPM loop is the 100-step
    training diffusion's (use_ddim=False)."""
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
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, use_ddim=False)
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
    """call(ddpm_sampler=...) under the same seed in both modes -> (host, device, equal generator state afterwards)."""
    out, after = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(seed)
        out[mode] = call(ddpm_sampler=mode)
        after[mode] = torch.randn(4, device=dev)
    assert np.isfinite(out["host"]).all() and out["host"].shape == out["device"].shape
    return out["host"], out["device"], torch.equal(after["host"], after["device"])


def _engines(m, name="_prefix_engines"):
    return list(m.vlm.__dict__[name].values())


def _plain(m):
    eng, = [e for e in _engines(m) if e.suffix_weights == "bf16" and e.prefill_mode == "train" and e.suffix_attention == "head"]
    return eng


@pytest.mark.parametrize("which", ["tiny3", "tiny15"], ids=["window3", "window15"])
def test_predict_action_diff_device_is_host_bit_for_bit(dev, request, which):
    """Window 3 and 15, the initial sample drawn from the seeded generator; a second observation on the same engine exercises the counter
    reset and the reuse of the captured step and of the noise table; the first observation again gives the first result."""
    m, window, (_, image, _, _, noise, _), kw = request.getfixturevalue(which)
    host, device, rng = both(dev, lambda **s: m.predict_action_diff(**kw, **s))
    assert host.shape == (window + 1, 7) and np.array_equal(device, host) and rng
    eng = _plain(m)
    st, = eng._ddpm.values()
    gid, nid = id(st.graph), st.noise.data_ptr()
    assert st.graph is not None and eng.graph_error is None
    assert st.steps == 100 and st.noise.shape == (100, (window + 1) * 7) and st.diffusion is m.diffusion
    other = second_observation(kw, image)
    host2, device2, rng2 = both(dev, lambda **s: m.predict_action_diff(**other, **s), seed=99)
    assert np.array_equal(device2, host2) and rng2 and not np.array_equal(host2, host)
    assert id(st.graph) == gid and st.noise.data_ptr() == nid and list(eng._ddpm.values()) == [st]
    given_h, given_d, rng3 = both(dev, lambda **s: m.predict_action_diff(noise=noise[1:2], **kw, **s), seed=7)   # a given x0: the steps still draw
    assert np.array_equal(given_d, given_h) and rng3
    torch.manual_seed(1234)
    assert np.array_equal(m.predict_action_diff(ddpm_sampler="device", **kw), host)
    assert id(st.graph) == gid


def test_samples_device_is_host_bit_for_bit(dev, tiny3):
    m, window, (_, image, _, _, noise, _), kw = tiny3
    host, device, rng = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=N, **kw, **s))
    assert host.shape == (N, window + 1, 7) and np.array_equal(device, host) and rng
    other = second_observation(kw, image)
    host2, device2, rng2 = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=N, noise=noise, **other, **s))
    assert np.array_equal(device2, host2) and rng2 and not np.array_equal(host2, host)
    one_h, one_d, _ = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=1, noise=noise[:1], **kw, **s))   # forwarded
    assert np.array_equal(one_d, one_h)


def test_sub_batched_samples_keep_one_state_per_group_count(dev, tiny3, monkeypatch):
    """MAX_ROWS = 2 R: passes of 2 + 2 + 1 groups on one engine -- one captured step and one noise table per distinct G, one sample_ddpm
    per pass in the host path's order: the same bits and the same generator position as the host loops."""
    from mla_amd import infer
    m, window, (_, _, _, _, noise, _), kw = tiny3
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_ROWS", 2 * (window + 2))
    host, device, rng = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=N, noise=noise, **kw, **s))
    assert np.array_equal(device, host) and rng
    eng, = [e for key, e in m.vlm.__dict__["_prefix_engines_samples"].items() if key[2] == 2]
    assert sorted(b for b, _ in eng._ddpm) == [1, 2] and all(st.graph is not None for st in eng._ddpm.values())
    assert sorted(st.noise.shape[1] for st in eng._ddpm.values()) == [(window + 1) * 7, 2 * (window + 1) * 7]


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
    return dict(images=images, pointclouds=pcs, cur_robot_states=proprios, input_ids=ids, use_ddim=False), s


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
            assert eng.graph_error is None and all(st.graph is not None for st in eng._ddpm.values()) and len(eng._ddpm) == 1


def test_fp8_weights_compact_prefill_and_split_attention_compose(dev, tiny3):
    from mla_amd import hip
    m, _, (_, _, _, _, noise, _), kw = tiny3
    for extra in (dict(suffix_weights="fp8"), dict(prefill="compact"), dict(suffix_attention="split")):
        host, device, rng = both(dev, lambda **s: m.predict_action_diff(**kw, **extra, **s))
        assert np.array_equal(device, host) and rng, extra
    modes = {(e.suffix_weights, e.prefill_mode, e.suffix_attention) for e in _engines(m) if e._ddpm}   # the device loop ran on those engines
    assert {("fp8", "train", "head"), ("bf16", "compact", "head"), ("bf16", "train", "split")} <= modes, modes
    split, = [e for e in _engines(m) if e.suffix_attention == "split"]
    assert split._attn_ws is not None and hip.plan_attn_split(1, split.nheads, split.R, split.S_cap).splits > 1   # the plan splits here
    torch.manual_seed(3)
    fp8 = m.predict_action_diff(noise=noise[:1], ddpm_sampler="device", suffix_weights="fp8", **kw)
    torch.manual_seed(3)
    assert not np.array_equal(fp8, m.predict_action_diff(noise=noise[:1], ddpm_sampler="device", **kw))
    host, device, rng = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=3, suffix_weights="fp8", **kw, **s))
    assert np.array_equal(device, host) and rng


def test_ddim_and_ddpm_device_loops_share_an_engine(dev, tiny3):
    """sampler="device" (DDIM) and ddpm_sampler="device" calls alternating on one engine: each keeps its state and captured step, and
    its bits."""
    m, _, (_, _, _, _, noise, _), kw = tiny3
    ddim_kw = dict(kw, use_ddim=True, num_ddim_steps=8, noise=noise[4:5])
    ddim_host = m.predict_action_diff(**ddim_kw)
    torch.manual_seed(11)
    ddpm_host = m.predict_action_diff(noise=noise[4:5], **kw)
    ids = None
    for _ in range(2):
        assert np.array_equal(m.predict_action_diff(sampler="device", **ddim_kw), ddim_host)
        torch.manual_seed(11)
        assert np.array_equal(m.predict_action_diff(noise=noise[4:5], ddpm_sampler="device", **kw), ddpm_host)
        eng = _plain(m)
        (a,), (b,) = eng._ddim.values(), eng._ddpm.values()
        assert a.graph is not None and b.graph is not None and a is not b and a.noise is None and b.noise is not None
        assert a.steps == 8 and b.steps == 100 and eng.graph_error is None
        if ids is None:
            ids = (id(a.graph), id(b.graph))
        assert ids == (id(a.graph), id(b.graph))
    assert not np.array_equal(ddim_host, ddpm_host)


def test_eager_steps_equal_the_captured_step(dev, tiny3, monkeypatch):
    from mla_amd import infer
    m, _, (_, _, _, _, noise, _), kw = tiny3

    def run(**s):
        torch.manual_seed(21)
        return m.predict_action_diff(noise=noise[2:3], **kw, **s)
    graphed = run(ddpm_sampler="device")
    eng = _plain(m)
    assert eng.graph_error is None and all(st.graph is not None for st in eng._ddpm.values())
    monkeypatch.setattr(infer, "_USE_GRAPH", False)
    eager = run(ddpm_sampler="device")
    assert eng.graph_error is not None and "MLA_INFER_GRAPH" in eng.graph_error
    monkeypatch.undo()
    assert np.array_equal(eager, graphed)
    assert np.array_equal(run(ddpm_sampler="device"), graphed) and eng.graph_error is None
    assert np.array_equal(graphed, run())


def test_device_sampler_follows_the_weights(dev, tiny3):
    """In-place updates (mul_ bumps _version, the address stays) of a final_layer and of a t_embedder weight change the device result
    exactly as they change the host result; restoring the weight restores the bits."""
    m, _, (_, _, _, _, noise, _), kw = tiny3

    def run(**s):
        torch.manual_seed(31)
        return m.predict_action_diff(noise=noise[3:4], **kw, **s)
    before = run(ddpm_sampler="device")
    assert np.array_equal(before, run())
    for w in (m.vlm.final_layer.mlp.fc1.weight, m.vlm.t_embedder.mlp[2].weight):
        saved = w.detach().clone()
        with torch.no_grad():
            w.mul_(1.5)
        changed_d, changed_h = run(ddpm_sampler="device"), run()
        with torch.no_grad():
            w.copy_(saved)
        assert np.array_equal(changed_d, changed_h) and not np.array_equal(changed_d, before)
        assert np.array_equal(run(ddpm_sampler="device"), before)


def test_sample_ddpm_never_waits_for_the_device(dev, tiny3):
    """Under torch's sync debug mode "error" a call that makes the host wait for the device raises. sample_ddpm does not (after one
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
    diffusion = create_diffusion("")
    x0 = noise[:1].to(dev)
    kw = dict(images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    with torch.inference_mode():
        eng = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, input_ids=ids.to(dev), **kw)
        torch.manual_seed(41)
        warm = eng.sample_ddpm(x0, diffusion)
        torch.cuda.synchronize()
        torch.manual_seed(41)
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = eng.sample_ddpm(x0, diffusion)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert eng.graph_error is None
        host_raised = False
        torch.cuda.set_sync_debug_mode("error")
        try:
            diffusion.p_sample_loop(eng, x0.shape, x0, clip_denoised=False, model_kwargs={})
        except RuntimeError:
            host_raised = True
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert host_raised, "the host loop did not wait for the device under the sync debug mode: this test shows nothing"
        torch.manual_seed(41)
        want = diffusion.p_sample_loop(eng, x0.shape, x0, clip_denoised=False, model_kwargs={})
    assert torch.equal(got, want) and torch.equal(warm, want) and got.dtype == torch.float32 and got.shape == (1, T, 7)


def test_ddpm_sampler_errors(dev, tiny3, monkeypatch):
    from mla_amd import infer
    m, _, (_, _, _, _, noise, _), kw = tiny3
    with pytest.raises(ValueError, match="ddpm_sampler"):
        m.predict_action_diff(ddpm_sampler="bogus", **kw)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        m.predict_action_diff(ddpm_sampler="device", reuse_prefix=False, **kw)
    with pytest.raises(ValueError, match="DDIM"):
        m.predict_action_diff(ddpm_sampler="device", **dict(kw, use_ddim=True, num_ddim_steps=8))
    with pytest.raises(ValueError, match="DDIM"):
        m.predict_action_diff_samples(num_samples=2, ddpm_sampler="device", **dict(kw, use_ddim=True))
    with pytest.raises(ValueError, match="DDIM"):                            # sampler= keeps its meaning: the DDIM loop
        m.predict_action_diff(sampler="device", **kw)
    monkeypatch.setattr(infer.PrefixCachedEps, "MAX_ROWS", 4)                # R = 5 suffix rows: the engine does not serve the shape
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_R", 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(ValueError, match="does not serve"):
            m.predict_action_diff(ddpm_sampler="device", noise=noise[:1], **kw)
        with pytest.raises(ValueError, match="does not serve"):
            m.predict_action_diff_samples(num_samples=2, ddpm_sampler="device", noise=noise[:2], **kw)
    monkeypatch.undo()
    with torch.inference_mode():
        eng = _engines(m)[0]
        with pytest.raises(AssertionError):
            eng.sample_ddpm(torch.zeros(eng.B + 1, eng.T, 7, device=dev), m.diffusion)
