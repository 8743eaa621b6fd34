"""GPU: pinning known actions while sampling a chunk -- mla_ddim_step_pin / mla_ddpm_step_pin (mla_amd/csrc/sampler.hip), the pinned
states of _CachedEpsBase.sample_ddim / sample_ddpm (mla_amd/infer.py) and MLA.predict_action_diff*(known_actions=...).

The acceptance criterion is bit-identity, as for the un-pinned device loops: the kernels against the torch restatement of their
arithmetic (tests/test_sampler_pinned_host.py shows on the CPU that the restatement is the host loop with the reference's denoised_fn
hook), "device" against "host" on every route, the pinned entries of the result against the known values, and the un-pinned call against
itself with pinned calls in between. One tolerance: the cached-prefix chunk against the whole-forward chunk, the engines' existing 3e-2."""
import numpy as np
import pytest
import torch

from test_sampler_device_gpu import _engines, build_tiny, ragged_batch
from test_sampler_pinned_host import pinned_ddim_update, pinned_ddpm_update

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NS = [1, 7, 112, 257, 65536]                                                 # 257: past the 256-thread stride; 65 536: the largest chunk


# ------------------------------------------------------------------------------------------------ kernels
def _coef(dev, kind, steps):
    """The 8-step tables of the real processes; steps = 1: a one-row table holding a middle step (every coefficient non-trivial)."""
    from mla_amd.diffusion import create_diffusion
    coef = create_diffusion("ddim8").ddim_tables(dev)[0] if kind == "ddim" else create_diffusion("8").ddpm_tables(dev)[0]
    assert coef.shape == (8, 4 if kind == "ddim" else 5)
    return coef if steps == 8 else coef[3:4].contiguous()


def _masks(n, g, dev):
    first = torch.arange(n) < max(1, n // 3)
    return [("none", torch.zeros(n, dtype=torch.bool, device=dev)), ("all", torch.ones(n, dtype=torch.bool, device=dev)),
            ("first", first.to(dev)), ("scattered", (torch.rand(n, generator=g) < 0.3).to(dev))]


def _check_step_kernel(dev, kind, n, steps):
    """Every step of the table chained, per mask: x, its bf16 cast and the counter after every launch; then advance = 0, the counters
    -1 and `steps`, and pin all zero against the plain kernel."""
    from mla_amd import hip
    coef = _coef(dev, kind, steps)
    g = torch.Generator().manual_seed(n * 10 + steps)
    x0 = (torch.randn(n, generator=g) * 3.0).to(dev)
    known = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    eps = (torch.randn(steps, n, generator=g) * 3.0).to(BF).to(dev)
    noise = torch.randn(steps, n, generator=g).to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)

    def ref(x, s, mask):
        if kind == "ddim":
            return pinned_ddim_update(x, eps[s].float(), coef[s], known, mask)
        return pinned_ddpm_update(x, eps[s].float(), coef[s], noise[s], known, mask)

    def launch(x, xb, s, pin, advance=True):
        if kind == "ddim":
            hip.ddim_step_pin(x, eps[s], xb, coef, known, pin, step, advance=advance)
        else:
            hip.ddpm_step_pin(x, eps[s], xb, coef, noise, known, pin, step, advance=advance)

    for name, mask in _masks(n, g, dev):
        pin = mask.to(torch.uint8)
        x, want = x0.clone(), x0.clone()
        xb = torch.full((n,), float("nan"), dtype=BF, device=dev)
        step.fill_(steps - 1)
        for s in reversed(range(steps)):
            want = ref(want, s, mask)
            launch(x, xb, s, pin)
            assert torch.equal(x, want), f"{name}, step {s}: max |diff| {float((x - want).abs().max()):.3e}"
            assert torch.equal(xb, want.to(BF)) and int(step.item()) == s - 1, (name, s)
        assert bool(torch.isfinite(x).all())
        if steps == 8:                                                        # row 0 is the last step applied: x = the pinned x0
            assert torch.equal(x[mask], known[mask])
        for stale in (-1, steps):                                             # outside the table: nothing is written, the counter stays
            step.fill_(stale)
            before, before_b = x.clone(), xb.clone()
            launch(x, xb, 0, pin)
            assert torch.equal(x, before) and torch.equal(xb, before_b) and int(step.item()) == stale, (name, stale)
        step.fill_(steps - 1)
        x.copy_(x0)
        launch(x, xb, steps - 1, pin, advance=False)
        want = ref(x0, steps - 1, mask)
        assert torch.equal(x, want) and torch.equal(xb, want.to(BF)) and int(step.item()) == steps - 1, name
    # pin all zero: the bits of the plain kernel
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)
    x, xb, y, yb = x0.clone(), torch.zeros(n, dtype=BF, device=dev), x0.clone(), torch.zeros(n, dtype=BF, device=dev)
    step.fill_(steps - 1)
    launch(x, xb, steps - 1, zero, advance=False)
    if kind == "ddim":
        hip.ddim_step(y, eps[steps - 1], yb, coef, step, advance=False)
    else:
        hip.ddpm_step(y, eps[steps - 1], yb, coef, noise, step, advance=False)
    assert torch.equal(x, y) and torch.equal(xb, yb) and not torch.equal(x, x0)
    # the wrappers' checks are the plain wrappers' plus known / pin
    for bad_known, bad_pin, err in ((known, zero.bool(), TypeError), (known.double(), zero, TypeError), (known[:-1] if n > 1 else known.repeat(2), zero, ValueError),
                                    (known, torch.zeros(n + 1, dtype=torch.uint8, device=dev), ValueError)):
        with pytest.raises(err):
            if kind == "ddim":
                hip.ddim_step_pin(x, eps[0], xb, coef, bad_known, bad_pin, step)
            else:
                hip.ddpm_step_pin(x, eps[0], xb, coef, noise, bad_known, bad_pin, step)
    assert torch.equal(x, y) and int(step.item()) == steps - 1                # no launch behind a refused call


@pytest.mark.parametrize("steps", [1, 8])
@pytest.mark.parametrize("n", NS)
def test_ddim_step_pin_is_the_restatement(dev, n, steps):
    _check_step_kernel(dev, "ddim", n, steps)


@pytest.mark.parametrize("steps", [1, 8])
@pytest.mark.parametrize("n", NS)
def test_ddpm_step_pin_is_the_restatement(dev, n, steps):
    _check_step_kernel(dev, "ddpm", n, steps)


# ------------------------------------------------------------------------------------------------ end to end, tiny model
KINDS = {"ddim": ({}, "sampler", "_ddim"), "ddpm": ({"use_ddim": False}, "ddpm_sampler", "_ddpm")}


def _tiny(dev, window):
    """tests/test_sampler_device_gpu.py's tiny MLA (no norm_stats: the calls return the normalised chunk) with the DDPM loop on a
    respaced 10-step process."""
    from mla_amd.diffusion import create_diffusion
    m, window, inputs, kw = build_tiny(dev, window)
    m.diffusion = create_diffusion("10")
    return m, window, inputs, kw


@pytest.fixture(scope="module")
def pin3(dev):
    return _tiny(dev, 3)


@pytest.fixture(scope="module")
def pin15(dev):
    return _tiny(dev, 15)


def known_rows(d, seed):
    """d known chunk steps in [-1, 1], fp32 values (the sampler's precision: what comes back is what went in)."""
    return (torch.rand(d, 7, generator=torch.Generator().manual_seed(seed)) * 2 - 1).numpy()


def both(dev, call, key, seed=1234):
    """call(<key>=...) under the same seed on the host and on the device -> (host, device, equal generator state afterwards)."""
    out, after = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(seed)
        out[mode] = call(**{key: mode})
        after[mode] = torch.randn(4, device=dev)
    assert np.isfinite(out["host"]).all() and out["host"].shape == out["device"].shape
    return out["host"], out["device"], torch.equal(after["host"], after["device"])


def pinned_ok(chunks, known):
    """The first len(known) steps of every chunk in chunks [..., T, 7] are the known values, exactly."""
    got = chunks[..., :len(known), :]
    return np.array_equal(got, np.broadcast_to(known, got.shape))


def _plain(m):
    eng, = [e for e in _engines(m) if e.suffix_weights == "bf16" and e.prefill_mode == "train" and e.suffix_attention == "head"]
    return eng


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("which", ["pin3", "pin15"], ids=["window3", "window15"])
def test_predict_action_diff_pinned_device_is_host(dev, request, which, kind):
    """d = 1, a value in between and T: "device" == "host" bit for bit with the same generator position, the pinned chunk steps come
    back exactly, the free ones are steered (they differ from the un-pinned call's)."""
    m, window, _, kw = request.getfixturevalue(which)
    extra, key, store = KINDS[kind]
    T = window + 1
    torch.manual_seed(1234)
    plain = m.predict_action_diff(**kw, **extra)
    for d in (1, T // 2, T):
        known = known_rows(d, 10 * T + d)
        host, device, rng = both(dev, lambda **s: m.predict_action_diff(known_actions=known, **kw, **extra, **s), key)
        assert host.shape == (T, 7) and np.array_equal(device, host) and rng, d
        assert pinned_ok(host, known) and not np.array_equal(host, plain), d
        if d < T:
            assert not np.array_equal(host[d:], plain[d:]), d
    eng = _plain(m)
    st, = getattr(eng, store + "_pin").values()
    assert st.graph is not None and eng.graph_error is None and st.pin.dtype == torch.uint8 and int(st.pin.sum()) == T * 7


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("which", ["pin3", "pin15"], ids=["window3", "window15"])
def test_samples_pinned_device_is_host(dev, request, which, kind):
    """N = 3 chunks of one observation share what is known."""
    m, window, _, kw = request.getfixturevalue(which)
    extra, key, _ = KINDS[kind]
    T, d = window + 1, (window + 1) // 2
    known = known_rows(d, 77)
    host, device, rng = both(dev, lambda **s: m.predict_action_diff_samples(num_samples=3, known_actions=known, **kw, **extra, **s), key)
    assert host.shape == (3, T, 7) and np.array_equal(device, host) and rng
    assert pinned_ok(host, known) and not np.array_equal(host[0, d:], host[1, d:])


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("which", ["pin3", "pin15"], ids=["window3", "window15"])
def test_batch_pinned_device_is_host(dev, request, which, kind):
    """B = 2 ragged prompts, without and with num_samples=2: a different d per observation, and one observation with nothing known --
    its chunks are the un-pinned call's (the observations of a pass do not see each other)."""
    m, window, inputs, _ = request.getfixturevalue(which)
    extra, key, _ = KINDS[kind]
    T = window + 1
    bkw, starts = ragged_batch(inputs, B=2)
    bkw = dict(bkw, **extra)
    k1, k2 = known_rows(1, 5), known_rows(T // 2 + 1, 6)
    tower = m.vlm.vision_tower_3d
    saved = tower.fps_starts_override
    try:
        tower.fps_starts_override = starts
        for ns in ({}, {"num_samples": 2}):
            host, device, rng = both(dev, lambda **s: m.predict_action_diff_batch(known_actions=[k1, k2], **bkw, **ns, **s), key)
            assert host.shape == (2,) + (2,) * len(ns) + (T, 7) and np.array_equal(device, host) and rng, ns
            assert pinned_ok(host[0], k1) and pinned_ok(host[1], k2), ns      # [T, 7], or [N, T, 7] with num_samples
            host2, device2, rng2 = both(dev, lambda **s: m.predict_action_diff_batch(known_actions=[None, k2], **bkw, **ns, **s), key)
            assert np.array_equal(device2, host2) and rng2 and np.array_equal(host2[1], host[1]), ns
            torch.manual_seed(1234)
            plain = m.predict_action_diff_batch(**bkw, **ns)
            assert np.array_equal(host2[0], plain[0]) and not np.array_equal(host2[1], plain[1]), ns
    finally:
        tower.fps_starts_override = saved


@pytest.mark.parametrize("kind", list(KINDS))
def test_pinned_eager_steps_equal_the_captured_step(dev, pin3, monkeypatch, kind):
    """MLA_INFER_GRAPH=0: the same launches one by one, the same bits."""
    from mla_amd import infer
    m, window, (_, _, _, _, noise, _), kw = pin3
    extra, key, store = KINDS[kind]
    known = known_rows(2, 21)

    def run(**s):
        torch.manual_seed(8)
        return m.predict_action_diff(noise=noise[2:3], known_actions=known, **kw, **extra, **s)
    graphed = run(**{key: "device"})
    eng = _plain(m)
    assert eng.graph_error is None and all(st.graph is not None for st in getattr(eng, store + "_pin").values())
    monkeypatch.setattr(infer, "_USE_GRAPH", False)
    eager = run(**{key: "device"})
    assert eng.graph_error is not None and "MLA_INFER_GRAPH" in eng.graph_error
    monkeypatch.undo()
    assert np.array_equal(eager, graphed) and np.array_equal(graphed, run()) and np.array_equal(graphed[:2], known)


@pytest.mark.parametrize("kind", list(KINDS))
def test_unpinned_call_is_untouched_by_pinned_calls(dev, pin3, kind):
    """known_actions=None is the call without the keyword, bit for bit, on the host and on the device; the un-pinned device state keeps
    its captured step across a pinned call, which has a state and a step of its own."""
    m, window, inputs, kw = pin3
    noise = inputs[4]
    extra, key, store = KINDS[kind]

    def run(**s):
        torch.manual_seed(8)
        return m.predict_action_diff(noise=noise[1:2], **kw, **extra, **s)
    first = run(**{key: "device"})
    eng = _plain(m)
    st, = getattr(eng, store).values()
    gid = id(st.graph)
    assert st.graph is not None and st.pin is None and st.known is None
    pinned = run(known_actions=known_rows(2, 3), **{key: "device"})
    assert not np.array_equal(pinned, first)
    assert np.array_equal(run(known_actions=None, **{key: "device"}), first) and np.array_equal(run(**{key: "device"}), first)
    assert id(st.graph) == gid and list(getattr(eng, store).values()) == [st]
    pst, = getattr(eng, store + "_pin").values()
    assert pst is not st and pst.graph is not None and pst.graph is not st.graph and pst.known is not None
    assert np.array_equal(run(known_actions=None), first) and np.array_equal(run(), first)
    # the routes with a list: None and a list of None
    bkw, starts = ragged_batch(inputs, B=2)
    tower = m.vlm.vision_tower_3d
    saved = tower.fps_starts_override
    try:
        tower.fps_starts_override = starts
        for ns in ({}, {"num_samples": 2}):
            out = []
            for ka in ({}, {"known_actions": None}, {"known_actions": [None, None]}):
                torch.manual_seed(8)
                out.append(m.predict_action_diff_batch(**bkw, **extra, **ns, **ka, **{key: "device"}))
            assert np.array_equal(out[1], out[0]) and np.array_equal(out[2], out[0]), ns
    finally:
        tower.fps_starts_override = saved
    torch.manual_seed(8)
    samples = m.predict_action_diff_samples(num_samples=3, **kw, **extra, **{key: "device"})
    torch.manual_seed(8)
    assert np.array_equal(m.predict_action_diff_samples(num_samples=3, known_actions=None, **kw, **extra, **{key: "device"}), samples)


@pytest.mark.parametrize("which", ["pin3", "pin15"], ids=["window3", "window15"])
def test_pinned_cached_prefix_chunk_is_the_whole_forward_chunk(dev, request, which):
    """reuse_prefix=False runs the host loop with denoised_fn around whole forwards: the pinned cached-prefix chunk stays within the
    engines' bound for "same function, other rounding" (3e-2 relative L2 per chunk), and both return the pinned steps exactly."""
    m, window, (_, _, _, _, noise, _), kw = request.getfixturevalue(which)
    T = window + 1
    known = known_rows(T // 2, 31)
    full = m.predict_action_diff(noise=noise[:1], known_actions=known, reuse_prefix=False, **kw)
    cached = m.predict_action_diff(noise=noise[:1], known_actions=known, **kw)
    d = float(np.linalg.norm(cached - full) / np.linalg.norm(full))
    print(f"window {window}: pinned cached vs whole-forward chunk {d:.3e}")
    assert np.isfinite(full).all() and d < 3e-2
    assert np.array_equal(full[:T // 2], known) and np.array_equal(cached[:T // 2], known)
    assert not np.array_equal(full, m.predict_action_diff(noise=noise[:1], reuse_prefix=False, **kw))


def test_pinned_fp8_weights_and_split_attention_compose(dev, pin3):
    m, window, _, kw = pin3
    known = known_rows(2, 41)
    for mode in (dict(suffix_weights="fp8"), dict(suffix_attention="split")):
        host, device, rng = both(dev, lambda **s: m.predict_action_diff(known_actions=known, **kw, **mode, **s), "sampler")
        assert np.array_equal(device, host) and rng and np.array_equal(host[:2], known), mode
    ran = {(e.suffix_weights, e.suffix_attention) for e in _engines(m) if e._ddim_pin}
    assert {("fp8", "head"), ("bf16", "split")} <= ran, ran
