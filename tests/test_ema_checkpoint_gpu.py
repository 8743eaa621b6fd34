"""MI355X: the weight average (EMA) through the strategy on the real kernels -- bit-exact resume including the average, the `-ema.pt`
file in the model file's layout, the `ema_weights()` swap of the bf16 replica and the four load cases.

Model, batch and helpers are those of tests/test_optimizer_resume_gpu.py (tiny MLA without the point tower, fixed diffusion draws).
No tolerance anywhere."""
import warnings

import pytest
import torch

import test_optimizer_resume_gpu as RZ

pytestmark = pytest.mark.gpu
DECAY = 0.9
OLD_KEYS = {"format", "step", "step_count", "hyper", "state", "rng"}
EMA_KEYS = {"ema", "ema_updates", "ema_decay", "ema_update_every"}


def _strategy(m, dev, total, ema_decay=DECAY, every=1):
    """RZ._strategy's settings at world 1 + the two EMA keywords."""
    from mla_amd.strategy import FSDPStrategy
    strat = FSDPStrategy(m, dev.index or 0, max_steps=total, global_batch_size=2, per_device_batch_size=2, learning_rate=1e-3,
                         weight_decay=0.01, max_grad_norm=1.0, lr_scheduler_type="linear-warmup+cosine-decay", warmup_ratio=0.5,
                         enable_gradient_checkpointing=False, repeated_diffusion_steps=RZ.R, ema_decay=ema_decay, ema_update_every=every)
    strat.run_setup(100)
    return strat


def _ema_snapshot(strat):
    sm = strat.sharded
    strat.synchronize()
    snap = dict(shards=[u.ema.clone() for u in sm.units if u.trainable], by_name=dict(sm.iter_ema_state()), updates=sm.ema_updates)
    torch.cuda.synchronize()
    return snap


def _same_ema(a, b):
    assert a["updates"] == b["updates"]
    assert len(a["shards"]) == len(b["shards"]) and all(torch.equal(x, y) for x, y in zip(a["shards"], b["shards"]))
    assert a["by_name"].keys() == b["by_name"].keys() and all(torch.equal(t, b["by_name"][n]) for n, t in a["by_name"].items())


def _trainable(strat):
    return [n for n, p in strat.vlm.named_parameters() if p.requires_grad]


def _load_file(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _resume_case(dev, tmp_path, every):
    """2 steps + save + fresh model from the file + fresh strategy + load + 2 steps == 4 steps in one go: what
    test_optimizer_resume_gpu compares, and the EMA shards and ema_updates. Returns whether the run used collectives."""
    torch.manual_seed(1234)
    whole = _strategy(RZ._build(dev), dev, 4, every=every)
    log_whole = RZ._steps(whole, whole.vlm, dev, 4)
    want, want_ema = RZ._snapshot(whole), _ema_snapshot(whole)
    assert want_ema["updates"] == 4 // every
    masters = dict(whole.sharded.iter_full_state_fp32())
    assert sum(int(not torch.equal(t, masters[n])) for n, t in want_ema["by_name"].items()) > len(want_ema["by_name"]) // 2   # it lags
    del whole
    torch.manual_seed(1234)
    first = _strategy(RZ._build(dev), dev, 4, every=every)
    log = RZ._steps(first, first.vlm, dev, 2)
    path = first.save_checkpoint(tmp_path, 2, 0, only_trainable=False, save_optimizer=True)
    blob = _load_file(RZ._opt_file(path))
    assert set(blob) == OLD_KEYS | EMA_KEYS and blob["format"] == "mla_amd.optimizer/1"
    assert (blob["ema_updates"], blob["ema_decay"], blob["ema_update_every"]) == (2 // every, DECAY, every)
    at_save = _ema_snapshot(first)
    assert list(blob["ema"]) == list(at_save["by_name"]) and set(blob["ema"]) == set(_trainable(first))
    assert all(torch.equal(t, at_save["by_name"][n].cpu()) for n, t in blob["ema"].items())
    del first
    torch.manual_seed(99)
    resumed = _strategy(RZ._model_from_file(dev, path), dev, 4, every=every)
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        resumed.load_optimizer_and_scheduler(path)
    assert not [str(w.message) for w in said if "average" in str(w.message)]          # a matching file loads without a word about it
    assert resumed.step == 2 and resumed.sharded.ema_updates == 2 // every
    _same_ema(at_save, _ema_snapshot(resumed))
    log += RZ._steps(resumed, resumed.vlm, dev, 2)
    assert log == log_whole, (log, log_whole)
    RZ._assert_same(want, RZ._snapshot(resumed))
    _same_ema(want_ema, _ema_snapshot(resumed))
    return bool(resumed.sharded.coll)


@pytest.mark.parametrize("every", [1, 2])
def test_resume_includes_the_average(dev, tmp_path, every):
    assert _resume_case(dev, tmp_path, every) is False


def test_ema_file_has_the_model_files_layout(dev, tmp_path):
    """`<stem>-ema.pt`: the model file's keys in its order; trainable entries = iter_ema_state(), every other entry the model file's;
    loads with strict=True into a fresh module. save_ema=None follows the strategy; without an average no file appears."""
    torch.manual_seed(1234)
    strat = _strategy(RZ._build(dev), dev, 4)
    RZ._steps(strat, strat.vlm, dev, 2)
    path = strat.save_checkpoint(tmp_path, 2, 0, only_trainable=False)
    ema_path = path.with_name(path.stem + "-ema.pt")
    assert ema_path.exists() and not RZ._opt_file(path).exists()
    model, ema = _load_file(path), _load_file(ema_path)
    assert list(model) == list(ema) == ["model"] and list(model["model"]) == list(ema["model"])
    state = {n: t.cpu() for n, t in strat.sharded.iter_ema_state()}
    trainable = set(_trainable(strat))
    assert set(state) == trainable
    seen = moved = 0
    for mkey, sd in model["model"].items():
        assert list(sd) == list(ema["model"][mkey]), mkey
        for leaf, t in sd.items():
            e = ema["model"][mkey][leaf]
            name = f"vlm.{mkey}.{leaf}"
            assert e.dtype == t.dtype and e.shape == t.shape, name
            if name in trainable:
                seen += 1
                moved += int(not torch.equal(e, t))
                assert torch.equal(e, state[name]), name
            else:
                assert torch.equal(e, t), name
    assert seen == len(trainable) and moved > seen // 2
    fresh = RZ._build(dev)
    fresh.load_state_dict({f"vlm.{mk}.{leaf}": v for mk, sd in ema["model"].items() for leaf, v in sd.items()}, strict=True)
    # save_ema=False writes none; a strategy without an average writes none and refuses save_ema=True
    p2 = strat.save_checkpoint(tmp_path, 3, 0, only_trainable=False, save_ema=False)
    assert not p2.with_name(p2.stem + "-ema.pt").exists()
    off = _strategy(RZ._build(dev), dev, 4, ema_decay=None)
    p3 = off.save_checkpoint(tmp_path, 5, 0, only_trainable=False, save_optimizer=True)
    assert not p3.with_name(p3.stem + "-ema.pt").exists() and set(_load_file(RZ._opt_file(p3))) == OLD_KEYS
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.save_checkpoint(tmp_path, 6, 0, save_ema=True)


def _swap_case(dev):
    """Inside ema_weights() every trainable bf16 parameter equals bf16(EMA); after exit flat16 of every unit is bit-identical to before
    entry; every swapped parameter's _version differs across each swap; a train_step after the context gives the loss bits of a run
    that never entered it."""
    torch.manual_seed(1234)
    plain = _strategy(RZ._build(dev), dev, 3)
    log_plain = RZ._steps(plain, plain.vlm, dev, 3)
    want, want_ema = RZ._snapshot(plain), _ema_snapshot(plain)
    del plain
    torch.manual_seed(1234)
    strat = _strategy(RZ._build(dev), dev, 3)
    log = RZ._steps(strat, strat.vlm, dev, 2)
    sm = strat.sharded
    strat.synchronize()
    before = [u.flat16.clone() for u in sm.units]
    ema = dict(sm.iter_ema_state())
    params = dict(strat.vlm.named_parameters())
    v0 = {n: p._version for n, p in params.items()}
    with strat.ema_weights():
        torch.cuda.synchronize()
        v1 = {n: p._version for n, p in params.items()}
        for n, p in params.items():
            if p.requires_grad:
                assert p.dtype == torch.bfloat16 and torch.equal(p.detach(), ema[n].to(torch.bfloat16)), n
                assert v1[n] != v0[n], n
        assert sum(int(not torch.equal(u.flat16, b)) for u, b in zip(sm.units, before)) >= 1
        with pytest.raises(RuntimeError, match="already open"):
            strat.ema_weights().__enter__()
    torch.cuda.synchronize()
    assert all(torch.equal(u.flat16, b) for u, b in zip(sm.units, before))
    assert all(p._version != v1[n] for n, p in params.items() if p.requires_grad)
    log += RZ._steps(strat, strat.vlm, dev, 1)
    assert log == log_plain, (log, log_plain)
    RZ._assert_same(want, RZ._snapshot(strat))
    _same_ema(want_ema, _ema_snapshot(strat))
    return bool(sm.coll)


def test_ema_weights_swap_is_exact_and_invisible_to_training(dev):
    assert _swap_case(dev) is False


CHILD = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import torch.distributed as dist
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
import pathlib
import test_ema_checkpoint_gpu as t
print("COLL", t._swap_case(dev), t._resume_case(dev, pathlib.Path(sys.argv[1]), 2))
dist.destroy_process_group()
"""


def test_swap_and_resume_under_forced_collectives(dev, tmp_path):
    """The sharded layout through the real RCCL entry points at world 1 (MLA_FORCE_COLLECTIVES=1, as
    test_optimizer_resume_gpu forces them): the swap's all-gathers on the side stream, the average gathered over the process group
    on save and sliced on load."""
    import os
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", MLA_FORCE_COLLECTIVES="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path), RZ.ROOT], capture_output=True, text=True, env=env, timeout=600, cwd=RZ.ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "COLL True True" in r.stdout, r.stdout[-1500:]


def test_the_other_three_load_cases_warn(dev, tmp_path):
    """A file without EMA keys into an EMA-on strategy: a warning, the average starts at the loaded masters. EMA keys into an EMA-off
    strategy: a warning, ignored. Another decay or interval: a warning, the current values stay."""
    torch.manual_seed(1234)
    off = _strategy(RZ._build(dev), dev, 4, ema_decay=None)
    RZ._steps(off, off.vlm, dev, 2)
    p_off = off.save_checkpoint(tmp_path / "off", 2, 0, only_trainable=False, save_optimizer=True)
    assert set(_load_file(RZ._opt_file(p_off))) == OLD_KEYS
    del off
    on = _strategy(RZ._model_from_file(dev, p_off), dev, 4)
    with pytest.warns(UserWarning, match="holds no weight average"):
        on.load_optimizer_and_scheduler(p_off)
    masters = dict(on.sharded.iter_full_state_fp32())
    got = dict(on.sharded.iter_ema_state())
    assert on.sharded.ema_updates == 0 and on.step == 2 and set(got) == set(_trainable(on))
    assert all(torch.equal(t, masters[n]) for n, t in got.items())
    RZ._steps(on, on.vlm, dev, 1)
    assert on.sharded.ema_updates == 1
    p_on = on.save_checkpoint(tmp_path / "on", 3, 0, only_trainable=False, save_optimizer=True)
    saved = _ema_snapshot(on)
    del on
    off2 = _strategy(RZ._model_from_file(dev, p_on), dev, 4, ema_decay=None)
    with pytest.warns(UserWarning, match="keeps none"):
        off2.load_optimizer_and_scheduler(p_on)
    assert off2.step == 3 and not any(hasattr(u, "ema") for u in off2.sharded.units)
    del off2
    other = _strategy(RZ._model_from_file(dev, p_on), dev, 4, ema_decay=0.5, every=2)
    with pytest.warns(UserWarning, match="the current values are used"):
        other.load_optimizer_and_scheduler(p_on)
    assert (other.sharded.ema_decay, other.sharded.ema_update_every) == (0.5, 2)
    _same_ema(saved, _ema_snapshot(other))                              # the average itself is restored
