"""GPU: MLA.predict_action_diff*(solver="dpmpp2m") -- DPM-Solver++(2M) over the respaced process on the host loop
(GaussianDiffusion.dpmpp2m_sample_loop, the definition) and on the device loop (_CachedEpsBase.sample_dpmpp2m, mla_dpmpp2m_step[_pin]).

The acceptance criterion is bit-identity, as for the DDIM and DDPM device loops: "device" against "host" on every route with the same
generator position afterwards, the pinned entries against the known values, solver="ddim" against the call without the keyword, and
the DDIM call against itself with 2M calls in between. One tolerance: the cached-prefix chunk against the whole-forward chunk, the
engines' existing 3e-2. Windows 1 and 15: 2 and 16 chunk rows per sample (the GEMV and the skinny suffix pass); 2, 3 and 4 solver steps:
no, one and two second-order steps."""
import numpy as np
import pytest
import torch

from test_sampler_device_gpu import _engines, build_tiny, ragged_batch
from test_sampler_pinned_gpu import known_rows, pinned_ok

pytestmark = pytest.mark.gpu
STORES = ("_prefix_engines", "_prefix_engines_samples", "_prefix_engines_batched", "_prefix_engines_batch_samples")


@pytest.fixture(scope="module")
def tiny1(dev):
    return build_tiny(dev, 1)


@pytest.fixture(scope="module")
def tiny15(dev):
    return build_tiny(dev, 15)


def both(dev, call, seed=1234):
    """call(sampler=...) under the same seed on the host and on the device -> (host, device, equal torch.cuda generator state)."""
    out, after = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(seed)
        out[mode] = call(sampler=mode)
        after[mode] = torch.cuda.get_rng_state(dev)
    assert np.isfinite(out["host"]).all() and out["host"].shape == out["device"].shape
    return out["host"], out["device"], torch.equal(after["host"], after["device"])


def routes(m, window, inputs, kw, steps):
    """The four sampling routes as (name, call(**keywords), shape), every call with num_ddim_steps = steps; the batch routes need the
    caller to set the FPS start indices of ragged_batch."""
    T = window + 1
    kw = dict(kw, num_ddim_steps=steps)
    bkw, starts = ragged_batch(inputs, B=2)
    bkw = dict(bkw, num_ddim_steps=steps)
    return starts, [("single", lambda **s: m.predict_action_diff(**kw, **s), (T, 7)),
                    ("samples", lambda **s: m.predict_action_diff_samples(num_samples=3, **kw, **s), (3, T, 7)),
                    ("batch", lambda **s: m.predict_action_diff_batch(**bkw, **s), (2, T, 7)),
                    ("batch_samples", lambda **s: m.predict_action_diff_batch(num_samples=2, **bkw, **s), (2, 2, T, 7))]


class fps_starts:
    def __init__(self, m, starts):
        self.tower, self.starts = m.vlm.vision_tower_3d, starts

    def __enter__(self):
        self.saved, self.tower.fps_starts_override = self.tower.fps_starts_override, self.starts

    def __exit__(self, *exc):
        self.tower.fps_starts_override = self.saved


@pytest.mark.parametrize("steps", [2, 3, 4])
@pytest.mark.parametrize("which", ["tiny1", "tiny15"], ids=["window1", "window15"])
def test_device_loop_is_the_host_loop_on_every_route(dev, request, which, steps):
    from mla_amd import infer
    m, window, inputs, kw = request.getfixturevalue(which)
    m.create_ddim(ddim_step=steps)
    assert m.ddim_diffusion.num_timesteps == steps
    starts, calls = routes(m, window, inputs, kw, steps)
    with fps_starts(m, starts):
        for name, call, shape in calls:
            host, device, rng = both(dev, lambda **s: call(solver="dpmpp2m", **s))
            assert host.shape == shape and np.array_equal(device, host) and rng, name
            if steps > 2:                                                     # two steps have no second-order step: DDIM up to rounding
                torch.manual_seed(1234)
                assert not np.array_equal(host, call()), name
    for store in STORES:
        ran = [e for e in _engines(m, store) if e._dpmpp2m]
        assert ran, store
        for eng in ran:
            assert all(st.steps == steps and st.hist is not None and st.noise is None for st in eng._dpmpp2m.values())
            if infer._USE_GRAPH:
                assert eng.graph_error is None and all(st.graph is not None for st in eng._dpmpp2m.values()), store


@pytest.mark.parametrize("which", ["tiny1", "tiny15"], ids=["window1", "window15"])
def test_known_actions_come_back_exactly_on_both_loops(dev, request, which):
    m, window, inputs, kw = request.getfixturevalue(which)
    T = window + 1
    m.create_ddim(ddim_step=3)
    starts, calls = routes(m, window, inputs, kw, 3)
    torch.manual_seed(1234)
    plain = m.predict_action_diff(solver="dpmpp2m", **dict(kw, num_ddim_steps=3))
    for d in sorted({1, T - 1}):
        known = known_rows(d, 10 * T + d)
        for name, call, shape in calls[:2]:
            host, device, rng = both(dev, lambda **s: call(solver="dpmpp2m", known_actions=known, **s))
            assert host.shape == shape and np.array_equal(device, host) and rng, (name, d)
            assert pinned_ok(host, known), (name, d)
            if name == "single":
                assert not np.array_equal(host[d:], plain[d:]), d            # the free steps are steered
        with fps_starts(m, starts):
            for name, call, shape in calls[2:]:
                host, device, rng = both(dev, lambda **s: call(solver="dpmpp2m", known_actions=[known, None], **s))
                assert np.array_equal(device, host) and rng and pinned_ok(host[0], known), (name, d)
    eng, = [e for e in _engines(m) if e.suffix_weights == "bf16" and e.prefill_mode == "train" and e.suffix_attention == "head"]
    pst, = eng._dpmpp2m_pin.values()
    st, = eng._dpmpp2m.values()
    assert pst is not st and pst.pin is not None and st.pin is None and pst.hist is not st.hist


def test_solver_ddim_is_the_call_without_the_keyword(dev, tiny1):
    m, window, inputs, kw = tiny1
    m.create_ddim(ddim_step=4)
    starts, calls = routes(m, window, inputs, kw, 4)
    with fps_starts(m, starts):
        for name, call, _ in calls:
            for sampler in ("host", "device"):
                out, after = [], []
                for extra in ({}, {"solver": "ddim"}):
                    torch.manual_seed(77)
                    out.append(call(sampler=sampler, **extra))
                    after.append(torch.cuda.get_rng_state(dev))
                assert np.array_equal(out[0], out[1]) and torch.equal(after[0], after[1]), (name, sampler)


def test_ddim_keeps_its_state_and_captured_step_across_two_m_calls(dev, tiny15, monkeypatch):
    """The DDIM device call replays the step it always replayed: same state object, same graph, same bits as on a fresh engine. The 2M
    state is its own, its history is zeroed at every reset, and the eager launches give the captured step's bits."""
    from mla_amd import infer
    m, window, inputs, kw = tiny15
    noise = inputs[4]
    kw = dict(kw, num_ddim_steps=4)
    diffusion = m.create_ddim(ddim_step=4)

    def run(**s):
        torch.manual_seed(8)
        return m.predict_action_diff(noise=noise[1:2], sampler="device", **kw, **s)
    m.vlm.__dict__.pop("_prefix_engines", None)
    fresh = run()                                                             # DDIM on a fresh engine
    m.vlm.__dict__.pop("_prefix_engines", None)
    two_m = run(solver="dpmpp2m")                                             # a fresh engine again: 2M first
    eng, = _engines(m)
    assert not eng._ddim and len(eng._dpmpp2m) == 1
    after = run()                                                             # DDIM behind a 2M call
    assert np.array_equal(after, fresh) and not np.array_equal(two_m, fresh)
    st, = eng._ddim.values()
    st2, = eng._dpmpp2m.values()
    gid = id(st.graph)
    assert st is not st2 and st.hist is None and st2.hist is not None and st.coef.shape == (4, 4) and st2.coef.shape == (4, 5)
    if infer._USE_GRAPH:
        assert st.graph is not None and st2.graph is not None and st.graph is not st2.graph and eng.graph_error is None
    st2.hist.fill_(float("nan"))                                              # a stale history must not reach the chunk: zeroed at the reset
    assert np.array_equal(run(solver="dpmpp2m"), two_m)
    assert np.array_equal(run(), fresh) and id(st.graph) == gid and list(eng._ddim.values()) == [st] and list(eng._dpmpp2m.values()) == [st2]
    assert m.ddim_diffusion is diffusion                                      # the cached process is whoever called create_ddim's
    torch.manual_seed(8)
    assert np.array_equal(m.predict_action_diff(noise=noise[1:2], solver="dpmpp2m", **kw), two_m)     # the host loop
    monkeypatch.setattr(infer, "_USE_GRAPH", False)
    eager = run(solver="dpmpp2m")
    assert eng.graph_error is not None and "MLA_INFER_GRAPH" in eng.graph_error
    monkeypatch.undo()
    assert np.array_equal(eager, two_m)
    assert np.array_equal(run(solver="dpmpp2m"), two_m) and (eng.graph_error is None or not infer._USE_GRAPH)


@pytest.mark.parametrize("which", ["tiny1", "tiny15"], ids=["window1", "window15"])
def test_cached_prefix_chunk_is_the_whole_forward_chunk(dev, request, which):
    """reuse_prefix=False runs dpmpp2m_sample_loop around whole forwards: the cached-prefix chunk stays within the engines' bound for
    "same function, other rounding" (3e-2 relative L2 per chunk), on the host and on the device loop."""
    m, window, (_, _, _, _, noise, _), kw = request.getfixturevalue(which)
    kw = dict(kw, num_ddim_steps=4)
    m.create_ddim(ddim_step=4)
    full = m.predict_action_diff(noise=noise[:1], solver="dpmpp2m", reuse_prefix=False, **kw)
    assert np.isfinite(full).all()
    for sampler in ("host", "device"):
        cached = m.predict_action_diff(noise=noise[:1], solver="dpmpp2m", sampler=sampler, **kw)
        d = float(np.linalg.norm(cached - full) / np.linalg.norm(full))
        print(f"window {window}, {sampler}: cached vs whole-forward 2M chunk {d:.3e}")
        assert d < 3e-2, (sampler, d)
    assert not np.array_equal(full, m.predict_action_diff(noise=noise[:1], reuse_prefix=False, **kw))


def test_fp8_weights_and_split_attention_compose(dev, tiny1):
    m, window, _, kw = tiny1
    kw = dict(kw, num_ddim_steps=4)
    m.create_ddim(ddim_step=4)
    for mode in (dict(suffix_weights="fp8"), dict(suffix_attention="split"), dict(suffix_mx="fp4")):
        host, device, rng = both(dev, lambda **s: m.predict_action_diff(solver="dpmpp2m", **kw, **mode, **s))
        assert np.array_equal(device, host) and rng, mode
    ran = {(e.suffix_weights, e.suffix_attention, e.suffix_mx) for e in _engines(m) if e._dpmpp2m}
    assert {("fp8", "head", "off"), ("bf16", "split", "off"), ("bf16", "head", "fp4")} <= ran, ran
