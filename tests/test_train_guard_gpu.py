"""MI355X: FSDPStrategy(skip_nonfinite=True) on the real kernels, end to end through a tiny MLA -- a batch with one infinite action
leaves masters, moments, bf16 replica and EMA exactly where they were, and the run continues as if that batch had never been seen.

Model and batch are those of tests/test_optimizer_resume_gpu.py (tiny MLA without the point tower, recipe.make_batch(B=2, R=2)); the
diffusion draws come from the device generator, re-seeded per batch, so that a batch sees the same draws in every run. Batches: b0 the
recipe's, b1 the recipe's with other actions, bad = b1 with actions[0, 0, 0] = inf. Because the bad value enters through the batch,
the non-finite gradient reaches the norm the way it does in training -- through the wgrad epilogues' partial sums -- and the next
backward has to overwrite non-finite main_grad contents (NaN x 0 is NaN: scaling them would poison the step after). The learning rate
is constant: the schedule index advances on a skipped window. No tolerance anywhere."""
import math

import pytest
import torch

import test_optimizer_resume_gpu as RZ

pytestmark = pytest.mark.gpu
DECAY = 0.9
SEEDS = {"b0": 100, "b1": 101, "b2": 102, "bad": 7}


def _strategy(m, dev, **kw):
    from mla_amd.strategy import FSDPStrategy
    strat = FSDPStrategy(m, dev.index or 0, max_steps=8, global_batch_size=2, per_device_batch_size=2, learning_rate=1e-3, weight_decay=0.01,
                         max_grad_norm=1.0, lr_scheduler_type="constant", enable_gradient_checkpointing=False,
                         repeated_diffusion_steps=RZ.R, ema_decay=DECAY, **kw)
    strat.run_setup(100)
    return strat


def _batches():
    from oracle import recipe
    batch, _ = recipe.make_batch(B=2, R=RZ.R, ragged=False)
    b0 = {k: v for k, v in batch.items() if k not in ("images", "point_cloud")}
    b0["images"] = {"front_image": batch["images"]["front_image"]}
    out = {"b0": b0}
    for name, (scale, shift) in (("b1", (0.5, 0.125)), ("b2", (-0.75, 0.25))):
        out[name] = dict(b0, actions=b0["actions"] * scale + shift)
    bad = out["b1"]["actions"].clone()
    bad[0, 0, 0] = float("inf")
    out["bad"] = dict(out["b1"], actions=bad)
    assert all(bool(torch.isfinite(out[k]["actions"]).all()) for k in ("b0", "b1", "b2"))
    return out


def _run(strat, names, batches):
    """train_step on the named batches -> [(loss, grad norm)]"""
    m = strat.vlm
    orig = type(m).forward
    m.forward = lambda **kw: orig(m, **kw)
    log = []
    for name in names:
        torch.manual_seed(SEEDS[name])
        ld = strat.train_step(batches[name])
        log.append((float(ld["total_loss"]), float(strat.sharded._norm)))
    return log


def _snap(strat):
    snap = RZ._snapshot(strat)
    snap["ema"] = [u.ema.clone() for u in strat.sharded.units if u.trainable]
    snap["bits"] = [(m.view(torch.int16) if m.dtype == torch.bfloat16 else m, v.view(torch.int16) if v.dtype == torch.bfloat16 else v)
                    for _, m, v in snap["shards"]]
    snap["counts"] = (strat.sharded.step_count, strat.sharded.ema_updates)
    torch.cuda.synchronize()
    return snap


def _assert_same(a, b, tag):
    a = dict(a, step=b["step"])                  # the schedule index counts windows, skipped or not
    RZ._assert_same(a, b, tag)
    assert a["counts"] == b["counts"], (tag, a["counts"], b["counts"])
    assert all(torch.equal(x, y) for x, y in zip(a["ema"], b["ema"])), (tag, "ema")
    assert all(torch.equal(x, s) and torch.equal(y, t) for (x, y), (s, t) in zip(a["bits"], b["bits"])), (tag, "moment bits")


@pytest.mark.parametrize("moments", ["fp32", "bf16"])
def test_bad_batch_is_as_if_never_seen(dev, moments):
    batches = _batches()
    torch.manual_seed(1234)
    on = _strategy(RZ._build(dev), dev, moments=moments, skip_nonfinite=True)
    assert on.sharded._sq_arena is not None          # the norm's first stage comes from the wgrad epilogues
    log_on = _run(on, ["b0"], batches)
    held = _snap(on)
    log_on += _run(on, ["bad"], batches)
    print("bad step: loss", log_on[1][0], "norm", log_on[1][1])
    assert not math.isfinite(log_on[1][1]), "the logged norm of the bad step is the non-finite norm itself"
    assert on.skipped_steps == 1 and on.step == 2
    _assert_same(_snap(on), held, "the skipped step wrote something")
    assert any(not bool(torch.isfinite(u.grad32).all()) for u in on.sharded.units if u.trainable)      # its gradients stay as they are
    log_on += _run(on, ["b1"], batches)
    torch.manual_seed(1234)
    off = _strategy(RZ._build(dev), dev, moments=moments)
    log_off = _run(off, ["b0", "b1"], batches)
    assert off.skipped_steps == 0 and off.sharded._skip is None
    assert [log_on[0], log_on[2]] == log_off, (log_on, log_off)
    _assert_same(_snap(on), _snap(off), "[b0, bad, b1] guarded against [b0, b1] unguarded")
    assert (on.skipped_steps, on.sharded.step_count, on.sharded.ema_updates, on.step) == (1, 2, 2, 3)
    assert all(bool(torch.isfinite(u.master_train).all()) for u in on.sharded.units if u.trainable)


def test_guard_on_finite_batches_matches_guard_off(dev):
    batches = _batches()
    runs = []
    for kw in (dict(skip_nonfinite=True), {}):
        torch.manual_seed(1234)
        strat = _strategy(RZ._build(dev), dev, **kw)
        runs.append((_run(strat, ["b0", "b1", "b2"], batches), _snap(strat), strat.skipped_steps, strat.step))
        del strat
    assert runs[0][0] == runs[1][0] and runs[0][2:] == runs[1][2:] == (0, 3)
    _assert_same(runs[0][1], runs[1][1], "guard on, finite batches")
