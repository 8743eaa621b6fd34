"""CPU: pinning known actions while sampling a chunk (MLA.predict_action_diff*(known_actions=...)) -- the host side.

The reference's loops hand `denoised_fn` to p_mean_variance, which applies it to the x0 prediction of every step
(models/diffusion/gaussian_diffusion.py:318-321); overwriting a mask of entries there is replacement inpainting. Checked here:
1. mla_amd.diffusion's loops with that hook against vectors captured from the reference (tools/capture_golden_pinned.py);
2. the arithmetic mla_ddim_step_pin / mla_ddpm_step_pin apply, written in torch operations one at a time, chained over all steps, is the
   host loop with the hook bit for bit -- what the device loops' bit-identity rests on (tests/test_sampler_pinned_gpu.py imports the two
   restatements from here);
3. without the hook the loops are what they were, and cond_fn still raises;
4. MLA.normalize_actions against unnormalize_actions, and every argument error of known_actions, raised before the model is touched."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

from mla_amd.diffusion import create_diffusion
from mla_amd.mla import MLA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pinned_ddim_update(x, eps, row, known, mask):
    """mla_ddim_step_pin's arithmetic: one torch operation per rounding, the select right behind px = ax - b eps."""
    a, b, c, d = row[0], row[1], row[2], row[3]
    ax = a * x
    be = b * eps
    px = ax - be
    px = torch.where(mask, known, px)
    e2 = (ax - px) / b
    pc = px * c
    de = d * e2
    return pc + de


def pinned_ddpm_update(x, eps, row, noise, known, mask):
    """mla_ddpm_step_pin's arithmetic, in the same way."""
    a, b, c1, c2, sig = row[0], row[1], row[2], row[3], row[4]
    ax = a * x
    be = b * eps
    px = ax - be
    px = torch.where(mask, known, px)
    m1 = c1 * px
    m2 = c2 * x
    mean = m1 + m2
    sn = sig * noise
    return mean + sn


def _toy_eps(x, t, scale=0.3, **kw):
    """The closed-form epsilon of oracle/capture_golden_infer.py (the golden files' model)."""
    return scale * torch.sin(x * 1.7 + t.float().view(-1, 1, 1) * 0.05) + 0.1 * x


def _bf16_eps(x, ts, **kw):
    """A bf16-valued epsilon model with PrismaticVLM.forward's tuple convention that draws nothing (as the suffix pass draws nothing)."""
    return None, (torch.sin(x * 1.7 + ts.view(-1, 1, 1).float() * 0.37) * 3.0).to(torch.bfloat16)


def _case(shape, seed):
    """x0, known in [-1, 1], and a mask with whole leading chunk steps (a different count per sample) plus scattered entries."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(*shape, generator=g) * 2.0
    known = torch.rand(*shape, generator=g) * 2 - 1
    mask = torch.rand(*shape, generator=g) < 0.15
    for b in range(shape[0]):
        mask[b, :1 + (2 * b) % shape[1]] = True
    return x0, known, mask


# ------------------------------------------------------------------------------------------------ 1. against the reference
def test_pinned_loops_match_the_reference():
    gold = np.load(os.path.join(GOLDEN, "sampler_pinned.npz"))
    x0, known, mask = (torch.from_numpy(gold[k]) for k in ("noise", "known", "mask"))
    assert x0.shape == (2, 16, 7) and mask.dtype == torch.bool
    assert mask[0, :3].all() and not mask[0, 3:].any() and mask[1, :5].all() and not mask[1, 5:].any()
    pin = lambda px: torch.where(mask, known, px)                             # noqa: E731
    for name, rtol, atol in (("ddim8", 1e-5, 1e-6), ("ddim4", 1e-5, 1e-6)):
        torch.manual_seed(5)
        got = create_diffusion(name).ddim_sample_loop(_toy_eps, x0.shape, x0, clip_denoised=False, denoised_fn=pin, model_kwargs={},
                                                      device="cpu", eta=0.0)
        assert np.allclose(got.numpy(), gold[name], rtol=rtol, atol=atol), name
        assert torch.equal(got[mask], known[mask]), name                      # exactly: the last step returns the pinned x0 itself
        assert np.array_equal(gold[name][gold["mask"]], gold["known"][gold["mask"]])
    torch.manual_seed(5)                                                      # the capture's stream: one randn_like per step
    got = create_diffusion("").p_sample_loop(_toy_eps, x0.shape, x0, clip_denoised=False, denoised_fn=pin, model_kwargs={}, device="cpu")
    assert np.allclose(got.numpy(), gold["ddpm100"], rtol=1e-4, atol=1e-5)
    assert torch.equal(got[mask], known[mask]) and np.array_equal(gold["ddpm100"][gold["mask"]], gold["known"][gold["mask"]])
    free = ~gold["mask"]
    assert float(np.abs(gold["ddim8"][free]).max()) > 10 and float(np.abs(gold["ddpm100"][free]).max()) > 1e3    # hence relative tolerances


# ------------------------------------------------------------------------------------------------ 2. the kernels' arithmetic
@pytest.mark.parametrize("shape", [(2, 16, 7), (3, 4, 14)], ids=str)
@pytest.mark.parametrize("steps", [4, 8])
def test_pinned_ddim_update_chained_is_the_host_loop(steps, shape):
    d = create_diffusion(f"ddim{steps}")
    coef, ts = d.ddim_tables("cpu")
    x0, known, mask = _case(shape, 100 * steps + shape[1])
    want = d.ddim_sample_loop(_bf16_eps, x0.shape, x0, clip_denoised=False, denoised_fn=lambda px: torch.where(mask, known, px),
                              model_kwargs={}, eta=0.0)
    x = x0.clone()
    for s in reversed(range(steps)):
        x = pinned_ddim_update(x, _bf16_eps(x, ts[s].expand(shape[0]))[1].float(), coef[s], known, mask)
    assert torch.equal(x, want) and bool(torch.isfinite(want).all())
    assert torch.equal(want[mask], known[mask]) and not torch.equal(want[~mask], x0[~mask])
    plain = d.ddim_sample_loop(_bf16_eps, x0.shape, x0, clip_denoised=False, model_kwargs={}, eta=0.0)
    assert not torch.equal(plain, want)


@pytest.mark.parametrize("shape", [(2, 16, 7), (3, 4, 14)], ids=str)
@pytest.mark.parametrize("respacing", ["", "10"], ids=["steps100", "steps10"])
def test_pinned_ddpm_update_chained_is_the_host_loop(respacing, shape):
    """The draws made up front, in the loop's order, as sample_ddpm makes them: p_sample_loop's result and generator state."""
    d = create_diffusion(respacing)
    steps = d.num_timesteps
    coef, ts = d.ddpm_tables("cpu")
    x0, known, mask = _case(shape, 100 * steps + shape[1])
    torch.manual_seed(99)
    want = d.p_sample_loop(_bf16_eps, x0.shape, x0, clip_denoised=False, denoised_fn=lambda px: torch.where(mask, known, px),
                           model_kwargs={})
    after_want = torch.randn(4)
    torch.manual_seed(99)
    plain = d.p_sample_loop(_bf16_eps, x0.shape, x0, clip_denoised=False, model_kwargs={})
    after_plain = torch.randn(4)
    torch.manual_seed(99)
    table = torch.zeros(steps, x0.numel())
    for s in reversed(range(steps)):
        table[s].copy_(torch.randn_like(x0).view(-1))
    x = x0.clone()
    for s in reversed(range(steps)):
        x = pinned_ddpm_update(x, _bf16_eps(x, ts[s].expand(shape[0]))[1].float(), coef[s], table[s].view_as(x), known, mask)
    after_got = torch.randn(4)
    assert torch.equal(x, want) and bool(torch.isfinite(want).all())
    assert torch.equal(after_got, after_want) and torch.equal(after_plain, after_want)     # the pinned loop draws what the plain one draws
    assert torch.equal(want[mask], known[mask]) and not torch.equal(plain, want)


# ------------------------------------------------------------------------------------------------ 3. the loops without the hook
def test_loops_without_the_hook_are_unchanged_and_cond_fn_raises():
    gold = np.load(os.path.join(GOLDEN, "inference.npz"), allow_pickle=True)
    x0 = torch.from_numpy(gold["toy_noise"])
    d8, full = create_diffusion("ddim8"), create_diffusion("")
    runs = {"ddim": lambda **kw: d8.ddim_sample_loop(_toy_eps, x0.shape, x0, clip_denoised=False, model_kwargs={}, device="cpu", eta=0.0, **kw),
            "ddpm": lambda **kw: full.p_sample_loop(_toy_eps, x0.shape, x0, clip_denoised=False, model_kwargs={}, device="cpu", **kw)}
    for name, run in runs.items():
        out = {}
        for label, kw in (("absent", {}), ("none", {"denoised_fn": None}), ("identity", {"denoised_fn": lambda px: px})):
            torch.manual_seed(5)
            out[label] = run(**kw)
        assert torch.equal(out["none"], out["absent"]) and torch.equal(out["identity"], out["absent"]), name
        with pytest.raises(NotImplementedError, match="cond_fn"):
            run(cond_fn=lambda *a, **k: None)
        with pytest.raises(NotImplementedError, match="cond_fn"):
            run(cond_fn=lambda *a, **k: None, denoised_fn=lambda px: px)
    t = torch.tensor([3] * x0.shape[0])
    for step in (d8.ddim_sample, full.p_sample):                              # the single steps take the hook too; None is no hook
        torch.manual_seed(1)
        a = step(_toy_eps, x0, t, clip_denoised=True, model_kwargs={})
        torch.manual_seed(1)
        b = step(_toy_eps, x0, t, clip_denoised=True, model_kwargs={}, denoised_fn=None)
        torch.manual_seed(1)
        c = step(_toy_eps, x0, t, clip_denoised=True, model_kwargs={}, denoised_fn=lambda px: px + 5.0)   # in front of the clamp
        assert torch.equal(a["sample"], b["sample"]) and torch.equal(a["pred_xstart"], b["pred_xstart"])
        assert bool((c["pred_xstart"] == 1.0).all())


# ------------------------------------------------------------------------------------------------ 4. normalize_actions, argument errors
Q01 = [0.1, -0.7, 0.25, -2.0, 1.0, -0.05, 0.0]
Q99 = [0.9, -0.2, 1.25, -1.0, 3.5, -0.01, 1.0]
MASK = [True, True, True, True, True, True, False]                            # the gripper channel passes through


class StandIn(types.SimpleNamespace):
    """`self` without a model (the stand-in of tests/test_sampling_modes_host.py): an attribute it lacks is the MLA function of that
    name, bound to it; touching the model is an AttributeError."""

    def __getattr__(self, name):
        try:
            attr = inspect.getattr_static(MLA, name)
        except AttributeError:
            raise AttributeError(name) from None
        if isinstance(attr, staticmethod):
            return attr.__func__
        if inspect.isfunction(attr):
            return types.MethodType(attr, self)
        raise AttributeError(name)


def _stand_in(norm_stats="default", window=15):
    if norm_stats == "default":
        norm_stats = {"toy": {"action": {"q01": Q01, "q99": Q99, "mask": MASK}}}
    return StandIn(norm_stats=norm_stats, future_action_window_size=window)


def test_normalize_actions_inverts_unnormalize_actions():
    """Round trip a -> normalize -> unnormalize on the masked dimensions, in float64 as both functions compute: the result is
    a - 1e-8 (a - q01) / (q99 - q01 + 1e-8), so the bound is 1e-8 |a - q01| / (q99 - q01) plus one fp32 ulp of the value (the float64
    rounding of the two maps is orders below it: every |a| here is >= 0.01, its fp32 ulp >= 9e-10)."""
    s = _stand_in()
    lo, hi, mask = np.array(Q01), np.array(Q99), np.array(MASK)
    g = np.random.default_rng(0)
    frac = np.concatenate([np.array([[0.0] * 7, [1.0] * 7, [0.5] * 7]), g.random((13, 7))])
    a = lo + frac * (hi - lo)
    a[:, 6] = (frac[:, 6] > 0.5).astype(np.float64)                           # what the return path leaves in the gripper channel
    n = MLA.normalize_actions(s, a)
    assert n.shape == a.shape and float(n[:, mask].min()) == -1.0 and abs(float(n[:, mask].max()) - 1.0) < 1e-7
    assert np.array_equal(n[:, 6], a[:, 6])
    back = MLA.unnormalize_actions(s, n.copy())
    bound = 1e-8 * np.abs(a - lo) / (hi - lo) + np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    assert float(np.abs(a[:, mask]).min()) >= 0.01
    assert bool((np.abs(back - a)[:, mask] <= bound[:, mask]).all()), float((np.abs(back - a) - bound)[:, mask].max())
    assert np.array_equal(back[:, 6], a[:, 6])
    # clipped outside [q01, q99], like the return path; the other way round on in-range normalised values
    out = MLA.normalize_actions(s, np.stack([lo - 1.0, hi + 1.0]))
    assert np.array_equal(out[:, mask], np.array([[-1.0] * 6, [1.0] * 6]))
    m = g.random((4, 7)) * 1.8 - 0.9
    m[:, 6] = 1.0
    again = MLA.normalize_actions(s, MLA.unnormalize_actions(s, m.copy()))     # (m + 1) shrinks by (q99 - q01) / (q99 - q01 + 1e-8)
    assert bool((np.abs(again - m)[:, mask] <= ((m + 1) * 1e-8 / (hi - lo) + 1e-14)[:, mask]).all()) and np.array_equal(again[:, 6], m[:, 6])
    # without statistics: the identity, like the return path
    plain = _stand_in(norm_stats=None)
    assert np.array_equal(MLA.normalize_actions(plain, a), a)


def test_known_actions_errors_come_before_the_model():
    T, D = 16, 7
    s = _stand_in(norm_stats=None)
    good = np.zeros((3, D))
    nan, inf = good.copy(), good.copy()
    nan[1, 2], inf[0, 0] = np.nan, np.inf
    bad = [(np.zeros((T + 1, D)), "1..16"), (np.zeros((0, D)), "1..16"), (np.zeros((3, D + 1)), "action_dim"), (np.zeros(D), "action_dim"),
           (np.zeros((1, 3, D)), "action_dim"), (nan, "non-finite"), (inf, "non-finite"), ("abc", "numeric")]
    single = [lambda k: MLA.predict_action_diff(s, known_actions=k),
              lambda k: MLA.predict_action_diff(s, known_actions=k, reuse_prefix=False),
              lambda k: MLA.predict_action_diff(s, known_actions=k, use_ddim=False, ddpm_sampler="device"),
              lambda k: MLA.predict_action_diff_samples(s, num_samples=3, known_actions=k),
              lambda k: MLA.predict_action_diff_samples(s, num_samples=1, known_actions=k, sampler="device")]
    rest = {"input_ids": [torch.tensor([1, 5 + b, 29871]) for b in range(2)], "cur_robot_states": [0] * 2}
    batch = [lambda k: MLA.predict_action_diff_batch(s, [None] * 2, [None] * 2, known_actions=k, **rest),
             lambda k: MLA.predict_action_diff_batch(s, [None] * 2, [None] * 2, known_actions=k, num_samples=2, **rest)]
    for call in single:
        for k, msg in bad:
            with pytest.raises(ValueError, match=msg):
                call(k)
        for k in (good, torch.zeros(T, D), [[0.0] * D], None):                # accepted: the call goes on to the model, which is not there
            with pytest.raises(AttributeError):
                call(k)
    for call in batch:
        for k, msg in bad:
            with pytest.raises(ValueError, match=msg):
                call([None, k])
        for k in ([good], [good, None, None], good, "ab", 3):                # one entry per observation, as a list
            with pytest.raises(ValueError, match="one entry"):
                call(k)
        for k in ([good, None], [None, None], (good, good[:1]), np.zeros((2, 4, D)), None):
            with pytest.raises(AttributeError):
                call(k)
    # the helper that builds what the samplers see: chunk steps 0 .. d - 1 of each observation, normalised, repeated over the samples
    st = _stand_in()
    a = np.array(Q01)[None] + np.array([[0.25], [0.5]]) * (np.array(Q99) - np.array(Q01))[None]
    entries = MLA._known_entries([a, None, a[:1]], 3, T, D)
    known, mask = MLA._pin(st, entries, T, D, None, "cpu", repeat=2)
    assert known.shape == (6, T, D) and known.dtype == torch.float32 and mask.dtype == torch.bool
    assert mask[:2, :2].all() and not mask[:2, 2:].any() and not mask[2:4].any() and mask[4:, :1].all() and not mask[4:, 1:].any()
    want = torch.from_numpy(MLA.normalize_actions(st, a).astype(np.float32))
    assert torch.equal(known[0, :2], want) and torch.equal(known[1, :2], want) and torch.equal(known[5, :1], want[:1])
    assert bool((known[~mask] == 0).all()) and MLA._pin(st, [None, None], T, D, None, "cpu") is None
