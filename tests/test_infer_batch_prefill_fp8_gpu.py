"""GPU: the opt-in FP8 prefill of the batched cached-prefix engines (MLA.predict_action_diff_batch(batch_prefill="fp8"), with and without
num_samples; mla_amd/infer.py _RowGemmEps._batch_compact_prefill on the wide-row GEMMs of mla_amd/csrc/prefill.hip) against the
single-observation FP8 prefill, against its yardstick "fp8_as_bf16" and against the default "train" prefill; the default paths stay bit
for bit what they were. Tiny model (hidden 256, intermediate 512, 9 layers, 2 heads of 128), windows 1 and 15; B = 3 observations with
prompts of three different lengths: S_p = 513 + id length, so the prefill has 3 x 540 = 1620 rows -- beyond the compact GEMMs' 1024."""
import gc

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu
BOUND = 3e-2                                             # the cached-prefix engines' bound for "same function, other rounding" 
LENGTHS = (21, 14, 27)
B = len(LENGTHS)
FP8_SINGLE = dict(prefill="compact", prefill_precision="fp8")


def observations(T, tag):
    """B distinct observations with prompts of LENGTHS ids: per-observation lists, noise [B, T, 7], FPS start indices [[B], [B]]."""
    g = recipe._gen(tag)
    lo, hi = torch.tensor([0.0, -0.4, 0.75]), torch.tensor([0.6, 0.4, 1.25])
    ids, images, pcs, proprios = [], [], [], []
    for n in LENGTHS:
        row = torch.randint(3, 29000, (n - 1,), generator=g)
        row[0] = 1
        ids.append(torch.cat([row, torch.tensor([29871])]))
        images.append(torch.cat([torch.randn(3, 672, 672, generator=g), torch.ones(1, 672, 672)], dim=0))
        pcs.append(lo + (hi - lo) * torch.rand(1024, 3, generator=g))
        proprios.append(torch.rand(7, generator=g) * 2 - 1)
    noise = torch.randn(B, 2, T, 7, generator=g)         # [:, 0] is the noise of the calls without num_samples
    starts = [torch.randint(0, 1024, (B,), generator=g), torch.randint(0, 512, (B,), generator=g)]
    return ids, images, pcs, proprios, noise, starts


@pytest.fixture(scope="module", params=[1, 15], ids=["window1", "window15"])
def tiny(request, dev):
    from test_infer_prefill_fp8_gpu import build_model
    window = request.param
    m = build_model(dev, window)
    yield m, window, observations(window + 1, f"batch_prefill_fp8_chunk{window + 1}")
    for name in [k for k in m.vlm.__dict__ if k.startswith("_prefix")]:       # engines refer back to the vlm: break the cycle
        m.vlm.__dict__.pop(name, None)
    del m
    gc.collect()
    torch.cuda.empty_cache()


def _batched(m, obs, sel=None, num_samples=None, **kw):
    ids, images, pcs, proprios, noise, starts = obs
    sel = list(range(B)) if sel is None else sel
    m.vlm.vision_tower_3d.fps_starts_override = [s[sel] for s in starts]
    noise = noise[sel, 0] if num_samples is None else noise[sel, :num_samples]
    return m.predict_action_diff_batch([images[b] for b in sel], [pcs[b].numpy() for b in sel],
                                       cur_robot_states=[proprios[b].numpy() for b in sel], input_ids=[ids[b] for b in sel], noise=noise,
                                       num_ddim_steps=8, num_samples=num_samples, **kw)


def _single(m, obs, b, num_samples=None, **kw):
    ids, images, pcs, proprios, noise, starts = obs
    m.vlm.vision_tower_3d.fps_starts_override = [s[b:b + 1] for s in starts]
    common = dict(image=images[b], pointcloud=pcs[b].numpy(), cur_robot_state=proprios[b].numpy(), input_ids=ids[b][None], num_ddim_steps=8)
    if num_samples is None:
        return m.predict_action_diff(noise=noise[b, :1], **common, **kw)
    return m.predict_action_diff_samples(num_samples=num_samples, noise=noise[b, :num_samples], **common, **kw)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _engine(m, store, mode):
    (eng,) = [e for k, e in m.vlm.__dict__[store].items() if f"batch_prefill:{mode}" in k and not any(
        str(t).startswith("attention:") or t in ("fp8", "fp8_as_bf16") for t in k)]
    return eng


def _statements(m, window, obs, num_samples, store):
    """What both routes promise of batch_prefill="fp8": finite, deterministic, every observation within the engines' bound of its own
    single-observation FP8-prefill call, the whole batch within the bound of "fp8_as_bf16"; the default call's bits are the same before
    and after; d(fp8, train) -- what the format costs -- is printed and has to be smaller than the distance between two observations'
    chunks (train); the cache's pad rows are finite."""
    T = window + 1
    default = _batched(m, obs, num_samples=num_samples)
    fp8 = _batched(m, obs, num_samples=num_samples, batch_prefill="fp8")
    assert fp8.shape == ((B, T, 7) if num_samples is None else (B, num_samples, T, 7)) and np.isfinite(fp8).all()
    eng = _engine(m, store, "fp8")
    assert eng.batch_prefill == "fp8" and eng._prefill_xq is not None and eng.NB == B
    S_p = (eng.prefix_len if store.endswith("batch_samples") else eng.slot).tolist()
    assert [n - S_p[0] for n in S_p] == [n - LENGTHS[0] for n in LENGTHS] and B * max(S_p) > 1024     # ragged, and beyond the compact GEMMs
    for c in eng.cache:                                                       # prefix rows, pad rows and the rows behind them: all finite
        assert torch.isfinite(c.float()).all()
    assert np.array_equal(_batched(m, obs, num_samples=num_samples, batch_prefill="fp8"), fp8)              # deterministic
    for b in range(B):
        single = _single(m, obs, b, num_samples=num_samples, **FP8_SINGLE)
        d = _rel(fp8[b], single)
        print(f"window {window} N {num_samples}: observation {b} (S_p {S_p[b]}) batch fp8 vs its own fp8-prefill call {d:.3e}")
        assert d < BOUND, (b, d)
    yard = _batched(m, obs, num_samples=num_samples, batch_prefill="fp8_as_bf16")
    assert _engine(m, store, "fp8_as_bf16")._prefill_xq is None
    d_yard, d_cost, d_yard_cost = _rel(fp8, yard), _rel(fp8, default), _rel(yard, default)
    d_obs = min(_rel(default[a], default[b]) for a in range(B) for b in range(B) if a != b)
    msg = (f"window {window} N {num_samples}: batch fp8 vs fp8_as_bf16 {d_yard:.3e} (bound {BOUND}); the format's cost: fp8 vs train "
           f"{d_cost:.3e}, fp8_as_bf16 vs train {d_yard_cost:.3e}; the closest two observations' chunks (train) {d_obs:.3e}")
    print(msg)
    assert d_yard < BOUND, msg
    assert d_cost < d_obs, msg
    assert np.array_equal(_batched(m, obs, num_samples=num_samples), default)                               # the default's bits stay
    assert np.array_equal(_batched(m, obs, num_samples=num_samples, batch_prefill="train"), default)
    return fp8


def test_batch_fp8_prefill_against_singles_yardstick_and_train(dev, tiny):
    m, window, obs = tiny
    _statements(m, window, obs, None, "_prefix_engines_batched")
    assert all(e.batch_prefill == "train" and e._prefill_ws is None for k, e in m.vlm.__dict__["_prefix_engines_batched"].items()
               if not any(str(t).startswith("batch_prefill:") for t in k))


def test_batch_samples_fp8_prefill_against_singles_yardstick_and_train(dev, tiny):
    """num_samples = 2: the same statements against predict_action_diff_samples(prefill="compact", prefill_precision="fp8")."""
    m, window, obs = tiny
    _statements(m, window, obs, 2, "_prefix_engines_batch_samples")


def test_permuting_the_observations_permutes_the_result_bit_for_bit(dev, tiny):
    """Every prefill row is quantised, projected and attended to inside its own sample, and the row count of the launches does not
    change: observations in another order, with their noise and FPS start indices, give the same chunks in that order."""
    m, _, obs = tiny
    perm = [2, 0, 1]
    for n in (None, 2):
        want = _batched(m, obs, num_samples=n, batch_prefill="fp8")
        got = _batched(m, obs, sel=perm, num_samples=n, batch_prefill="fp8")
        assert np.array_equal(got, want[perm])


def test_one_fp8_copy_serves_the_batch_prefill_and_the_suffix_pass(dev, tiny):
    """batch_prefill="fp8" with bf16 suffix weights builds the model's FP8 copy; suffix_weights="fp8" then streams the SAME object."""
    m, window, obs = tiny
    for name in [k for k in m.vlm.__dict__ if k.startswith("_prefix_engines") or k == "_prefix_fp8"]:
        m.vlm.__dict__.pop(name)
    a = _batched(m, obs, num_samples=2, batch_prefill="fp8")
    copy = m.vlm.__dict__["_prefix_fp8"]["fp8"]
    (eng_a,) = m.vlm.__dict__["_prefix_engines_batch_samples"].values()
    assert eng_a.suffix_weights == "bf16" and eng_a._suffix is eng_a._packed
    b = _batched(m, obs, num_samples=2, batch_prefill="fp8", suffix_weights="fp8")
    assert np.isfinite(b).all() and m.vlm.__dict__["_prefix_fp8"]["fp8"] is copy
    eng_b = next(e for k, e in m.vlm.__dict__["_prefix_engines_batch_samples"].items() if "fp8" in k)
    assert eng_b is not eng_a and eng_b._suffix is copy and eng_b.batch_prefill == "fp8"
    d = _rel(b, a)
    print(f"window {window}: fp8 batch prefill + fp8 suffix weights vs + bf16 suffix weights {d:.3e}")
    assert d < BOUND, d
    c = _batched(m, obs, num_samples=2, batch_prefill="fp8", suffix_weights="fp8_as_bf16")
    assert m.vlm.__dict__["_prefix_fp8"]["fp8"] is copy and _rel(c, b) < BOUND


def test_device_sampler_and_split_attention_on_an_fp8_batch_prefill(dev, tiny):
    """sampler="device" promises the host loop's bits; groups_attention="split" is the same function up to summation order (the
    engines' bound). Both routes."""
    m, window, obs = tiny
    for n in (None, 2):
        host = _batched(m, obs, num_samples=n, batch_prefill="fp8")
        assert np.array_equal(_batched(m, obs, num_samples=n, batch_prefill="fp8", sampler="device"), host)
        split = _batched(m, obs, num_samples=n, batch_prefill="fp8", groups_attention="split")
        d = _rel(split, host)
        print(f"window {window} N {n}: fp8 batch prefill, split vs head attention {d:.3e}")
        assert np.isfinite(split).all() and d < BOUND, d


def test_one_observation_forwards_to_the_single_call(dev, tiny):
    """B = 1 IS predict_action_diff / predict_action_diff_samples with prefill="compact", prefill_precision=<the mode>."""
    m, _, obs = tiny
    for mode in ("fp8", "fp8_as_bf16"):
        single = dict(prefill="compact", prefill_precision=mode)
        assert np.array_equal(_batched(m, obs, sel=[1], batch_prefill=mode)[0], _single(m, obs, 1, **single))
        assert np.array_equal(_batched(m, obs, sel=[1], num_samples=2, batch_prefill=mode)[0], _single(m, obs, 1, num_samples=2, **single))


def test_weight_update_reaches_the_fp8_batch_prefill(dev, tiny):
    """An in-place update of one decoder weight (mul_ bumps _version) changes the next chunks; restoring it restores the bits."""
    m, _, obs = tiny
    before = _batched(m, obs, batch_prefill="fp8")
    w = m.vlm.llm_backbone.llm.model.layers[4].mlp.down_proj.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    changed = _batched(m, obs, batch_prefill="fp8")
    with torch.no_grad():
        w.copy_(saved)
    restored = _batched(m, obs, batch_prefill="fp8")
    assert not np.array_equal(changed, before) and np.array_equal(restored, before)


def test_batch_prefill_refuses_without_the_cached_prefix(dev, tiny):
    m, _, obs = tiny
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        _batched(m, obs, batch_prefill="fp8", reuse_prefix=False)
    with pytest.raises(ValueError, match="batch_prefill"):
        _batched(m, obs, num_samples=2, batch_prefill="bf16")
