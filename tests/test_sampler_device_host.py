"""CPU: the host side of the device-resident DDIM loop (MLA.predict_action_diff(sampler="device"), mla_amd/infer.py:sample_ddim).

GaussianDiffusion.ddim_tables gives four fp32 coefficients per step; the update mla_ddim_step applies with them, written here in torch
operations one at a time (each rounded on its own), is ddim_sample(clip_denoised=False, eta=0.0)["sample"] bit for bit -- the statement the
device sampler's bit-identity to the host loop rests on. Plus every argument error of sampler= that is raised before the device is touched."""
import ctypes

import pytest
import torch

from mla_amd.diffusion import create_diffusion

SHAPES = [(1, 1, 7), (3, 16, 7), (15, 17, 14)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def four_coefficient_update(x, eps, row):
    """mla_ddim_step's arithmetic: every product, difference, quotient and sum is one torch operation, i.e. one rounding."""
    a, b, c, d = row[0], row[1], row[2], row[3]
    ax = a * x
    be = b * eps
    px = ax - be
    e2 = (ax - px) / b
    pc = px * c
    de = d * e2
    return pc + de


@pytest.mark.parametrize("steps", [5, 8, 10])
def test_coefficient_table(steps):
    d = create_diffusion(f"ddim{steps}")
    coef, ts = d.ddim_tables("cpu")
    assert coef.shape == (steps, 4) and coef.dtype == torch.float32 and bool(torch.isfinite(coef).all())
    assert float(coef[0, 2]) == 1.0 and float(coef[0, 3]) == 0.0             # the last step applied: x = pred_xstart
    assert bool((coef[:, :2] > 0).all()) and bool((coef[1:, 2:] > 0).all())
    assert ts.dtype == torch.long and ts.tolist() == list(d.timestep_map) and len(d.timestep_map) == steps
    again = d.ddim_tables("cpu")
    assert again[0] is coef and again[1] is ts                                # cached per device, like _tables
    assert d.ddim_tables(torch.device("cpu"), eta=0.0)[0] is coef


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("steps", [5, 8, 10])
def test_four_coefficient_update_is_ddim_sample_bit_for_bit(steps, shape):
    """Every step of the loop, chained as the loop chains them: inputs of magnitude ~3, bf16 epsilons as the model returns them."""
    d = create_diffusion(f"ddim{steps}")
    coef, _ = d.ddim_tables("cpu")
    g = _gen(steps * 1000 + shape[0] * 31 + shape[1])
    x = torch.randn(*shape, generator=g) * 3.0
    x_dev = x.clone()
    for i in reversed(range(steps)):
        eps = (torch.randn(*shape, generator=g) * 3.0).to(torch.bfloat16)
        seen = {}

        def stub(xx, tt, eps=eps, seen=seen):
            seen["t"] = tt
            return None, eps
        t = torch.tensor([i] * shape[0])
        want = d.ddim_sample(stub, x, t, clip_denoised=False, model_kwargs={}, eta=0.0)["sample"]
        assert seen["t"].tolist() == [d.timestep_map[i]] * shape[0]
        x_dev = four_coefficient_update(x_dev, eps.float(), coef[i])
        assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())
        assert torch.equal(x_dev, want), f"step {i}: max |diff| {float((x_dev - want).abs().max()):.3e}"
        x = want
    assert float(x.abs().max()) > 0.1


def test_eta_other_than_zero_raises():
    d = create_diffusion("ddim8")
    with pytest.raises(ValueError, match="eta"):
        d.ddim_tables("cpu", eta=0.5)


def test_check_sampler():
    from mla_amd import infer
    assert infer.MODES["sampler"].values == ("host", "device")
    infer.check_mode("sampler", "host")
    infer.check_mode("sampler", "host", reuse_prefix=False, use_ddim=False, num_ddim_steps=None)      # today's path takes every combination
    infer.check_mode("sampler", "device", True, True, 8)
    for bad in ("bogus", "Device", None, ""):
        with pytest.raises(ValueError, match="sampler"):
            infer.check_mode("sampler", bad)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        infer.check_mode("sampler", "device", reuse_prefix=False)
    with pytest.raises(ValueError, match="DDIM"):
        infer.check_mode("sampler", "device", use_ddim=False)
    with pytest.raises(ValueError, match="DDIM"):
        infer.check_mode("sampler", "device", num_ddim_steps=None)
    with pytest.raises(ValueError, match="does not serve"):
        infer.needs_engine("PrefixCachedEps", 16, sampler="device")
    infer.needs_engine("PrefixCachedEps", 16, sampler="host")


def _public_calls():
    from mla_amd.mla import MLA
    return [("predict_action_diff", lambda **kw: MLA.predict_action_diff(object(), **kw)),
            ("predict_action_diff_samples", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=2, **kw)),
            ("predict_action_diff_samples[1]", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=1, **kw)),
            ("predict_action_diff_batch", lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], **kw)),
            ("predict_action_diff_batch[samples]",
             lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], num_samples=3, **kw))]


@pytest.mark.parametrize("name,call", _public_calls(), ids=[n for n, _ in _public_calls()])
def test_sampler_errors_are_raised_before_anything_is_computed(name, call):
    """object() stands in for the model: the errors are raised before the model, its device or its inputs are touched."""
    with pytest.raises(ValueError, match="sampler"):
        call(sampler="bogus")
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        call(sampler="device", reuse_prefix=False)
    with pytest.raises(ValueError, match="DDIM"):
        call(sampler="device", use_ddim=False)
    with pytest.raises(ValueError, match="DDIM"):
        call(sampler="device", num_ddim_steps=None)
    with pytest.raises(ValueError, match="sampler"):
        call(sampler="bogus", suffix_weights="fp8")


def test_wrappers_reject_host_tensors_and_launchers_reject_bad_sizes():
    """No CPU path; the launchers validate on the host before any launch (safe without a GPU)."""
    from mla_amd import hip
    x = torch.zeros(8)
    with pytest.raises((RuntimeError, TypeError)):
        hip.ddim_step(x, x.to(torch.bfloat16), x.to(torch.bfloat16), torch.zeros(8, 4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises((RuntimeError, TypeError)):
        hip.sampler_rows(torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16),
                         torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32), 2, 1)
    lib = hip.lib()
    P = ctypes.c_void_p(64)
    assert lib.mla_ddim_step(P, P, P, P, None, 8, 8, 1, None) < 0 and b"null" in lib.mla_last_error()
    assert lib.mla_ddim_step(P, P, P, P, P, 65537, 8, 1, None) < 0 and b"65536" in lib.mla_last_error()
    assert lib.mla_ddim_step(P, P, P, P, P, 0, 8, 1, None) < 0
    assert lib.mla_ddim_step(P, P, P, P, P, 8, 0, 1, None) < 0
    assert lib.mla_sampler_rows(P, P, None, P, 1, 1, 256, 8, None) < 0 and b"null" in lib.mla_last_error()
    assert lib.mla_sampler_rows(P, P, P, P, 1, 1, 252, 8, None) < 0 and b"multiple of 8" in lib.mla_last_error()
    assert lib.mla_sampler_rows(P, ctypes.c_void_p(66), P, P, 1, 1, 256, 8, None) < 0
    assert lib.mla_sampler_rows(P, P, P, P, 0, 1, 256, 8, None) < 0 and lib.mla_sampler_rows(P, P, P, P, 1, 1, 256, 0, None) < 0
