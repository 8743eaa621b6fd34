"""MI355X: bf16 AdamW moments (FSDPStrategy moments="bf16") through the strategy on the real kernels -- bit-exact resume from the
optimizer file (bf16 moment tensors, the seed of their rounding), refusal of a file of the other moment format in both directions,
half the moment memory, and nothing changed with the keyword off.

Model, batch and helpers are those of tests/test_optimizer_resume_gpu.py (tiny MLA without the point tower, fixed diffusion draws).
No tolerance anywhere."""
import pytest
import torch

import test_optimizer_resume_gpu as RZ

pytestmark = pytest.mark.gpu
DECAY, SEED = 0.9, 0x5EED0123456789
OLD_KEYS = {"format", "step", "step_count", "hyper", "state", "rng"}
EMA_KEYS = {"ema", "ema_updates", "ema_decay", "ema_update_every"}
M16_KEYS = {"moments", "moments_seed"}


def _strategy(m, dev, total, **kw):
    """RZ._strategy's settings at world 1 + the keywords under test."""
    from mla_amd.strategy import FSDPStrategy
    strat = FSDPStrategy(m, dev.index or 0, max_steps=total, global_batch_size=2, per_device_batch_size=2, learning_rate=1e-3,
                         weight_decay=0.01, max_grad_norm=1.0, lr_scheduler_type="linear-warmup+cosine-decay", warmup_ratio=0.5,
                         enable_gradient_checkpointing=False, repeated_diffusion_steps=RZ.R, **kw)
    strat.run_setup(100)
    return strat


def _ema(strat):
    strat.synchronize()
    return [u.ema.clone() for u in strat.sharded.units if u.trainable], strat.sharded.ema_updates


def _moment_bits(snap):
    return [(m.view(torch.int16), v.view(torch.int16)) for _, m, v in snap["shards"]]


def _load_file(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_resume_is_bit_exact_with_bf16_moments(dev, tmp_path):
    """3 steps + save + fresh model from the file + fresh strategy (ANOTHER seed: the file's is adopted) + load + 2 steps == 5 steps in
    one go: masters, bf16 moments, bf16 parameters, EMA and (loss, gradient norm, learning rate) of every step."""
    kw = dict(moments="bf16", moments_seed=SEED, ema_decay=DECAY)
    torch.manual_seed(1234)
    whole = _strategy(RZ._build(dev), dev, 5, **kw)
    assert all(u.exp_avg.dtype == u.exp_avg_sq.dtype == torch.bfloat16 for u in whole.sharded.units if u.trainable)
    log_whole = RZ._steps(whole, whole.vlm, dev, 5)
    want, want_ema = RZ._snapshot(whole), _ema(whole)
    del whole
    torch.manual_seed(1234)
    first = _strategy(RZ._build(dev), dev, 5, **kw)
    log = RZ._steps(first, first.vlm, dev, 3)
    path = first.save_checkpoint(tmp_path, 3, 0, only_trainable=False, save_optimizer=True)
    at_save = RZ._snapshot(first)
    blob = _load_file(RZ._opt_file(path))                     # weights_only=True loads it
    assert set(blob) == OLD_KEYS | EMA_KEYS | M16_KEYS and blob["format"] == "mla_amd.optimizer/1"
    assert (blob["moments"], blob["moments_seed"]) == ("bf16", SEED)
    assert all(d["exp_avg"].dtype == d["exp_avg_sq"].dtype == torch.bfloat16 for d in blob["state"].values())
    assert all(torch.equal(d["exp_avg"].view(torch.int16), at_save["moments"][n][0].cpu().view(torch.int16)) and
               torch.equal(d["exp_avg_sq"].view(torch.int16), at_save["moments"][n][1].cpu().view(torch.int16)) for n, d in blob["state"].items())
    del first
    torch.manual_seed(99)
    resumed = _strategy(RZ._model_from_file(dev, path), dev, 5, **dict(kw, moments_seed=1))
    resumed.load_optimizer_and_scheduler(path)
    assert resumed.step == 3 and resumed.moments_seed == resumed.sharded.moments_seed == SEED
    loaded = RZ._snapshot(resumed)
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(_moment_bits(at_save), _moment_bits(loaded)))
    log += RZ._steps(resumed, resumed.vlm, dev, 2)
    assert log == log_whole, (log, log_whole)
    got = RZ._snapshot(resumed)
    RZ._assert_same(want, got)
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(_moment_bits(want), _moment_bits(got)))
    ema, updates = _ema(resumed)
    assert updates == want_ema[1] == 5 and all(torch.equal(a, b) for a, b in zip(ema, want_ema[0]))
    # another seed is another run: the stored moments differ (the masters follow from step 2 on)
    torch.manual_seed(1234)
    other = _strategy(RZ._build(dev), dev, 5, **dict(kw, moments_seed=SEED + 1))
    RZ._steps(other, other.vlm, dev, 2)
    assert any(not torch.equal(a, c) for (a, _), (c, _) in zip(_moment_bits(RZ._snapshot(other)), _moment_bits(want)))


def test_a_file_of_the_other_format_is_refused_before_any_write(dev, tmp_path):
    torch.manual_seed(1234)
    f32 = _strategy(RZ._build(dev), dev, 4)
    RZ._steps(f32, f32.vlm, dev, 2)
    p32 = f32.save_checkpoint(tmp_path / "fp32", 2, 0, only_trainable=False, save_optimizer=True)
    assert set(_load_file(RZ._opt_file(p32))) == OLD_KEYS             # the keyword off: the file is unchanged, key for key
    torch.manual_seed(1234)
    b16 = _strategy(RZ._build(dev), dev, 4, moments="bf16")
    RZ._steps(b16, b16.vlm, dev, 2)
    p16 = b16.save_checkpoint(tmp_path / "bf16", 2, 0, only_trainable=False, save_optimizer=True)
    for strat, path in ((b16, p32), (f32, p16)):
        before = RZ._snapshot(strat)
        with pytest.raises(ValueError, match="(?s)(fp32.*bf16|bf16.*fp32)"):
            strat.load_optimizer_and_scheduler(path)
        RZ._assert_same(before, RZ._snapshot(strat))
        # the sharded model's own check (a state handed over without the strategy's tag): dtype, before the first write
        state = {n: (d["exp_avg"], d["exp_avg_sq"]) for n, d in _load_file(RZ._opt_file(path))["state"].items()}
        with pytest.raises(ValueError, match="(?s)'fp32'.*'bf16'"):
            strat.sharded.load_optimizer_state(state, 77)
        RZ._assert_same(before, RZ._snapshot(strat))
    # half the moment memory: two moments, 4 -> 2 bytes per trainable element
    n_train = sum(u.n_train for u in b16.sharded.units if u.trainable)
    assert f32.sharded.state_bytes() - b16.sharded.state_bytes() == 4 * n_train
    assert sum(u.exp_avg.numel() * u.exp_avg.element_size() for u in b16.sharded.units if u.trainable) * 2 == \
        sum(u.exp_avg.numel() * u.exp_avg.element_size() for u in f32.sharded.units if u.trainable)


def test_keyword_off_and_environment_switch(dev, monkeypatch):
    """moments="fp32" and no keyword at all give the same step bit for bit; MLA_MOMENTS is read when the keyword is None (and only then);
    an unknown value raises."""
    runs = []
    for kw in ({}, dict(moments="fp32", moments_seed=7)):
        torch.manual_seed(1234)
        strat = _strategy(RZ._build(dev), dev, 3, **kw)
        assert strat.sharded.moments == "fp32"
        runs.append((RZ._steps(strat, strat.vlm, dev, 2), RZ._snapshot(strat), strat.sharded.state_bytes()))
        del strat
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    RZ._assert_same(runs[0][1], runs[1][1])
    monkeypatch.setenv("MLA_MOMENTS", "bf16")
    torch.manual_seed(1234)
    env = _strategy(RZ._build(dev), dev, 3)
    assert env.moments == env.sharded.moments == "bf16" and env.sharded.units[-1].exp_avg.dtype == torch.bfloat16
    log = RZ._steps(env, env.vlm, dev, 2)
    assert log[0] == runs[0][0][0] and log[1][2] == runs[0][0][1][2]      # step 1 starts from the same weights: same loss and norm
    assert _strategy(RZ._build(dev), dev, 3, moments="fp32").sharded.moments == "fp32"      # the keyword wins over the environment
    monkeypatch.setenv("MLA_MOMENTS", "fp8")
    with pytest.raises(ValueError, match="moments must be one of"):
        _strategy(RZ._build(dev), dev, 3)
