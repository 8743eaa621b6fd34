"""CPU: the host side of the device-resident DDPM loop (MLA.predict_action_diff(use_ddim=False, ddpm_sampler="device"),
mla_amd/infer.py:sample_ddpm).

GaussianDiffusion.ddpm_tables gives five fp32 coefficients per step; the update mla_ddpm_step applies with them and the step's normal
variates, written here in torch operations one at a time (each rounded on its own), is p_sample(clip_denoised=False)["sample"] bit for
bit -- and drawing all the steps' variates up front, in the loop's order, gives p_sample_loop's result and generator position. These are
the two statements the device loop's bit-identity to the host loop rests on. Plus every argument error of ddpm_sampler= that is raised
before the device is touched."""
import ctypes
import os
import re

import pytest
import torch

from mla_amd.diffusion import create_diffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 7), (3, 16, 7), (15, 17, 14)]
RESPACINGS = ["", "10"]                                                      # the 100-step training diffusion and a respaced 10-step one


def eight_operation_update(x, eps, row, noise):
    """mla_ddpm_step's arithmetic: every product, difference and sum is one torch operation, i.e. one rounding."""
    a, b, c1, c2, sig = row[0], row[1], row[2], row[3], row[4]
    ax = a * x
    be = b * eps
    px = ax - be
    m1 = c1 * px
    m2 = c2 * x
    mean = m1 + m2
    sn = sig * noise
    return mean + sn


def toy_eps(seed_scale=3.0):
    """A bf16-valued epsilon model with PrismaticVLM.forward's tuple convention: a fixed function of x and the mapped timestep that draws
    nothing from the generator (as the suffix pass draws nothing)."""
    def model(x, ts, **kw):
        e = torch.sin(x * 1.7 + ts.view(-1, 1, 1).float() * 0.37) * seed_scale
        return None, e.to(torch.bfloat16)
    return model


@pytest.mark.parametrize("respacing", RESPACINGS, ids=["steps100", "steps10"])
def test_coefficient_table(respacing):
    d = create_diffusion(respacing)
    steps = d.num_timesteps
    coef, ts = d.ddpm_tables("cpu")
    assert steps == (100 if respacing == "" else 10)
    assert coef.shape == (steps, 5) and coef.dtype == torch.float32 and coef.is_contiguous() and bool(torch.isfinite(coef).all())
    assert ts.dtype == torch.long and ts.tolist() == list(d.timestep_map) and len(d.timestep_map) == steps
    assert float(coef[0, 4]) == 0.0 and bool((coef[1:, 4] > 0).all())         # no noise is added by the last step applied
    assert bool((coef[:, :3] > 0).all()) and float(coef[0, 3]) == 0.0 and bool((coef[1:, 3] > 0).all())
    again = d.ddpm_tables("cpu")
    assert again[0] is coef and again[1] is ts                                # cached per device, like ddim_tables
    assert d.ddpm_tables(torch.device("cpu"))[0] is coef
    assert d.ddim_tables("cpu")[0].shape == (steps, 4)                        # the two tables do not share a cache entry
    assert d.ddpm_tables("cpu")[0] is coef


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("respacing", RESPACINGS, ids=["steps100", "steps10"])
def test_eight_operation_update_is_p_sample_bit_for_bit(respacing, shape):
    """Every step of the loop, chained as the loop chains them: inputs of magnitude ~3, bf16 epsilons as the model returns them, the
    noise aligned through the seed."""
    d = create_diffusion(respacing)
    steps = d.num_timesteps
    coef, _ = d.ddpm_tables("cpu")
    g = torch.Generator().manual_seed(steps * 1000 + shape[0] * 31 + shape[1])
    x = torch.randn(*shape, generator=g) * 3.0
    x_dev = x.clone()
    for i in reversed(range(steps)):
        eps = (torch.randn(*shape, generator=g) * 3.0).to(torch.bfloat16)
        seen = {}

        def stub(xx, tt, eps=eps, seen=seen):
            seen["t"] = tt
            return None, eps
        t = torch.tensor([i] * shape[0])
        torch.manual_seed(7000 + i)
        want = d.p_sample(stub, x, t, clip_denoised=False, model_kwargs={})["sample"]
        assert seen["t"].tolist() == [d.timestep_map[i]] * shape[0]
        torch.manual_seed(7000 + i)
        noise = torch.randn_like(x_dev)
        x_dev = eight_operation_update(x_dev, eps.float(), coef[i], noise)
        assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())
        assert torch.equal(x_dev, want), f"step {i}: max |diff| {float((x_dev - want).abs().max()):.3e}"
        if i == 0:                                                            # 0 * noise is added, not skipped: the zeros' signs too
            assert torch.equal(torch.signbit(x_dev), torch.signbit(want))
        x = want
    assert float(x.abs().max()) > 0.1


@pytest.mark.parametrize("shape", SHAPES[:2], ids=[str(s) for s in SHAPES[:2]])
@pytest.mark.parametrize("respacing", RESPACINGS, ids=["steps100", "steps10"])
def test_noise_drawn_up_front_is_p_sample_loop_bit_for_bit(respacing, shape):
    """sample_ddpm's order of work on the host: all `steps` randn_like draws first, step steps - 1 first, into a [steps, n] table; then
    the chained update reading row s. The result and the generator's state afterwards are p_sample_loop's."""
    d = create_diffusion(respacing)
    steps = d.num_timesteps
    coef, ts = d.ddpm_tables("cpu")
    model = toy_eps()
    x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(5)) * 2.0
    torch.manual_seed(99)
    want = d.p_sample_loop(model, x0.shape, x0, clip_denoised=False, model_kwargs={})
    after_want = torch.randn(4)
    torch.manual_seed(99)
    table = torch.zeros(steps, x0.numel())
    for s in reversed(range(steps)):
        table[s].copy_(torch.randn_like(x0).view(-1))
    x = x0.clone()
    for s in reversed(range(steps)):
        eps = model(x, ts[s].expand(shape[0]))[1].float()
        x = eight_operation_update(x, eps, coef[s], table[s].view_as(x))
    after_got = torch.randn(4)
    assert torch.equal(x, want) and bool(torch.isfinite(want).all())
    assert torch.equal(after_got, after_want)
    assert not torch.equal(want, x0)


def test_check_ddpm_sampler():
    from mla_amd import infer
    assert infer.MODES["ddpm_sampler"].values == ("host", "device")
    assert infer.MODES["sampler"].values == ("host", "device")
    infer.check_mode("ddpm_sampler", "host")
    infer.check_mode("ddpm_sampler", "host", reuse_prefix=False, use_ddim=True, num_ddim_steps=8)     # the default takes every combination
    infer.check_mode("ddpm_sampler", "device", True, False, 8)
    infer.check_mode("ddpm_sampler", "device", True, True, None)      # num_ddim_steps=None runs the DDPM loop
    for bad in ("bogus", "Device", None, ""):
        with pytest.raises(ValueError, match="ddpm_sampler"):
            infer.check_mode("ddpm_sampler", bad)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        infer.check_mode("ddpm_sampler", "device", reuse_prefix=False)
    with pytest.raises(ValueError, match="DDIM"):
        infer.check_mode("ddpm_sampler", "device", True, True, 8)
    with pytest.raises(ValueError, match="does not serve"):
        infer.needs_engine("PrefixCachedEps", 16, ddpm_sampler="device")
    infer.needs_engine("PrefixCachedEps", 16, ddpm_sampler="host")
    with pytest.raises(ValueError, match="DDIM"):                            # sampler= keeps its meaning
        infer.check_mode("sampler", "device", use_ddim=False)


def test_check_modes_accepts_and_forwards_the_keyword():
    from mla_amd.infer import Modes, check_modes
    base = dict(suffix_weights="bf16", prefill="train", sampler="host", suffix_attention="head")
    check_modes(Modes(**base), True, False, 8)                               # the default: "host"
    check_modes(Modes(**base, ddpm_sampler="device"), True, False, 8)
    check_modes(Modes(**base, ddpm_sampler="device"), True, True, None)
    with pytest.raises(ValueError, match="ddpm_sampler"):
        check_modes(Modes(**base, ddpm_sampler="bogus"), True, False, 8)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        check_modes(Modes(**base, ddpm_sampler="device"), False, False, 8)
    with pytest.raises(ValueError, match="DDIM"):
        check_modes(Modes(**base, ddpm_sampler="device"), True, True, 8)
    with pytest.raises(ValueError, match="DDIM"):                            # sampler="device" on a DDPM call raises as before
        check_modes(Modes(suffix_weights="bf16", prefill="train", sampler="device", suffix_attention="head", ddpm_sampler="device"), True, False, 8)


def _public_calls():
    from mla_amd.mla import MLA
    return [("predict_action_diff", lambda **kw: MLA.predict_action_diff(object(), **kw)),
            ("predict_action_diff_samples", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=2, **kw)),
            ("predict_action_diff_samples[1]", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=1, **kw)),
            ("predict_action_diff_batch", lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], **kw)),
            ("predict_action_diff_batch[samples]",
             lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], num_samples=3, **kw))]


@pytest.mark.parametrize("name,call", _public_calls(), ids=[n for n, _ in _public_calls()])
def test_ddpm_sampler_errors_are_raised_before_anything_is_computed(name, call):
    """object() stands in for the model: the errors are raised before the model, its device or its inputs are touched."""
    with pytest.raises(ValueError, match="ddpm_sampler"):
        call(ddpm_sampler="bogus", use_ddim=False)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        call(ddpm_sampler="device", use_ddim=False, reuse_prefix=False)
    with pytest.raises(ValueError, match="DDIM"):
        call(ddpm_sampler="device")                                          # the defaults run DDIM: never silently ignored
    with pytest.raises(ValueError, match="DDIM"):
        call(sampler="device", use_ddim=False)


def test_every_entry_point_has_the_keyword():
    import inspect
    from mla_amd.mla import MLA
    for name in ("predict_action_diff", "predict_action_diff_batch", "predict_action_diff_samples"):
        p = inspect.signature(getattr(MLA, name)).parameters["ddpm_sampler"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "host", name


def test_argtypes_match_the_header_and_the_launcher_rejects_bad_sizes():
    """The ctypes signature has the header's parameter count; no CPU path; the launcher validates on the host before any launch.
    (hip._SIGNATURES is parsed from the header since mla_amd/abi.py, so the count and the pointer positions agree by construction; the
    comparison stays as an independent reading of the one declaration.)"""
    from mla_amd import hip
    txt = open(os.path.join(ROOT, "include", "mla_hip.h")).read()
    m = re.search(r"\bint\s+mla_ddpm_step\s*\(([^)]*)\)\s*;", txt)
    assert m, "mla_ddpm_step is not declared in include/mla_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = hip._SIGNATURES["mla_ddpm_step"]
    assert len(sig) == len(params) == 10
    assert [("*" in p or "stream" in p) for p in params] == [t is ctypes.c_void_p for t in sig]
    x = torch.zeros(8)
    with pytest.raises((RuntimeError, TypeError)):
        hip.ddpm_step(x, x.to(torch.bfloat16), x.to(torch.bfloat16), torch.zeros(8, 5), torch.zeros(8, 8), torch.zeros(1, dtype=torch.int32))
    lib = hip.lib()
    P = ctypes.c_void_p(64)
    assert lib.mla_ddpm_step(P, P, P, P, None, P, 8, 8, 1, None) < 0 and b"null" in lib.mla_last_error()
    assert lib.mla_ddpm_step(P, P, P, P, P, None, 8, 8, 1, None) < 0 and b"null" in lib.mla_last_error()
    assert lib.mla_ddpm_step(P, P, P, P, P, P, 65537, 8, 1, None) < 0 and b"65536" in lib.mla_last_error()
    assert lib.mla_ddpm_step(P, P, P, P, P, P, 0, 8, 1, None) < 0
    assert lib.mla_ddpm_step(P, P, P, P, P, P, 8, 0, 1, None) < 0
