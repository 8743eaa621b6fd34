"""MI355X: bit-exact training resume on the real kernels (HipLocalOps, buffer arenas, the fused two-group AdamW with its bf16 write).

The model and batch are those of tests/test_fsdp_2rank_gpu.py (tiny MLA without the point tower, recipe.make_batch(B=2, R=2)). A run
that is stopped after `before` optimizer steps -- save_checkpoint(save_optimizer=True), a FRESH model filled from the model file, a
fresh strategy, run_setup, load_optimizer_and_scheduler -- and continued for `after` steps must leave the same bits as `before +
after` steps in one go: losses and gradient norms of the continued steps, the fp32 masters, both AdamW moments, and every bf16
compute parameter (the replica the load side casts from the masters == the one AdamW's fused cast wrote). No tolerance anywhere."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_fsdp_2rank_gpu import _build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 2


def _strategy(m, dev, world, total):
    from mla_amd.strategy import FSDPStrategy
    strat = FSDPStrategy(m, dev.index or 0, max_steps=total, global_batch_size=2, per_device_batch_size=2 // world, learning_rate=1e-3,
                         weight_decay=0.01, max_grad_norm=1.0, lr_scheduler_type="linear-warmup+cosine-decay", warmup_ratio=0.5,
                         enable_gradient_checkpointing=False, repeated_diffusion_steps=R)
    assert strat.grad_accumulation_steps == 1
    strat.run_setup(100)
    return strat


def _model_from_file(dev, path):
    """What a resuming script does before run_setup(): a fresh module (its own values scrambled here, so that every value that
    matters has to come from the file) with the model file's fp32 tensors loaded."""
    m = _build(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    ck = torch.load(path, map_location="cpu", weights_only=True)["model"]
    m.load_state_dict({f"vlm.{mk}.{leaf}": v for mk, sd in ck.items() for leaf, v in sd.items()}, strict=True)
    return m


def _steps(strat, m, dev, n, part=None, fixed=True):
    """`n` optimizer steps on both samples (part None) or on sample `part` (a rank's half of the global batch); with `fixed` the
    diffusion draws are injected, otherwise MLA.forward draws them from the device generator. Returns [(loss, grad norm, lr)]."""
    from oracle import recipe
    batch, draws = recipe.make_batch(B=2, R=R, ragged=False)
    sel = slice(None) if part is None else slice(part, part + 1)
    rows = torch.arange(2 * R) if part is None else torch.tensor([part, part + 2])
    b = {k: (v[sel] if torch.is_tensor(v) else v) for k, v in batch.items() if k not in ("images", "point_cloud")}
    b["images"] = {"front_image": batch["images"]["front_image"][sel]}
    orig = type(m).forward
    if fixed:
        m.forward = lambda **kw: orig(m, **kw, noise=draws["noise"][rows].to(dev), timestep=draws["timestep"][rows].to(dev))
    else:
        m.forward = lambda **kw: orig(m, **kw)
    out = []
    for _ in range(n):
        ld = strat.train_step(b)
        out.append((float(ld["total_loss"]), float(strat.sharded._norm), strat.last_lr))
    return out


def _snapshot(strat):
    sm = strat.sharded
    strat.synchronize()
    snap = dict(master={n: t.clone() for n, t in sm.iter_full_state_fp32()},
                moments={n: (mm, vv) for n, mm, vv in sm.iter_optimizer_state()},
                bf16={n: p.detach().clone() for n, p in strat.vlm.named_parameters()},
                flat16=[u.flat16.clone() for u in sm.units],
                shards=[(u.master_train.clone(), u.exp_avg.clone(), u.exp_avg_sq.clone()) for u in sm.units if u.trainable],
                step=strat.step, step_count=sm.step_count)
    torch.cuda.synchronize()
    return snap


def _assert_same(a, b, tag=""):
    assert (a["step"], a["step_count"]) == (b["step"], b["step_count"]), tag
    assert a["master"].keys() == b["master"].keys() and a["moments"].keys() == b["moments"].keys() and a["bf16"].keys() == b["bf16"].keys()
    bad = [("master", n) for n in a["master"] if not torch.equal(a["master"][n], b["master"][n])]
    bad += [("exp_avg", n) for n in a["moments"] if not torch.equal(a["moments"][n][0], b["moments"][n][0])]
    bad += [("exp_avg_sq", n) for n in a["moments"] if not torch.equal(a["moments"][n][1], b["moments"][n][1])]
    bad += [("bf16", n) for n in a["bf16"] if a["bf16"][n].dtype != torch.bfloat16 or not torch.equal(a["bf16"][n], b["bf16"][n])]
    bad += [("flat16 of unit", i) for i, (x, y) in enumerate(zip(a["flat16"], b["flat16"])) if not torch.equal(x, y)]
    bad += [("shards of trainable unit", i) for i, (x, y) in enumerate(zip(a["shards"], b["shards"]))
            if not all(torch.equal(s, t) for s, t in zip(x, y))]
    assert not bad, (tag, len(bad), bad[:8])
    assert sum(int(mm.abs().sum() > 0) for mm, _ in a["moments"].values()) > len(a["moments"]) // 2     # not a comparison of zeros


def _ckpt(run_dir, step):
    return Path(run_dir) / "checkpoints" / f"step-{step:06d}-epoch-00-loss=inf.pt"


def _opt_file(path):
    return path.with_name(path.stem + "-optimizer.pt")


def _resume_case(dev, run_dir, fixed=True, world=1, rank=0, before=2, after=2):
    """`before + after` steps in one go vs `before` + save + fresh model from the file + fresh strategy + load + `after`. With
    `fixed=False` both runs are seeded ONCE at their start and the continued one starts from another seed: only the restored
    generator state can make its draws the uninterrupted run's. Returns a description of the layout the run used."""
    part = None if world == 1 else rank
    total = before + after
    torch.manual_seed(1234)
    whole = _strategy(_build(dev), dev, world, total)
    log_whole = _steps(whole, whole.vlm, dev, total, part, fixed)
    want = _snapshot(whole)
    assert len({lr for _, _, lr in log_whole}) >= 3                      # warm-up, then decay: a restarted schedule would show
    del whole
    torch.manual_seed(1234)
    first = _strategy(_build(dev), dev, world, total)
    log = _steps(first, first.vlm, dev, before, part, fixed)
    path = first.save_checkpoint(run_dir, before, 0, only_trainable=False, save_optimizer=True)
    assert (path == _ckpt(run_dir, before)) if rank == 0 else (path is None)
    path = _ckpt(run_dir, before)
    assert _opt_file(path).exists()
    sm = first.sharded
    layout = dict(coll=bool(sm.coll), inplace=bool(sm.inplace_reduce), arenas=sm._arenas is not None, world=sm.world)
    del first, sm
    torch.manual_seed(99)
    resumed = _strategy(_model_from_file(dev, path), dev, world, total)
    resumed.load_optimizer_and_scheduler(path)
    assert resumed.step == before and resumed.sharded.step_count == before
    log += _steps(resumed, resumed.vlm, dev, after, part, fixed)
    print(f"layout {layout}, fixed draws {fixed}: (loss, grad norm, lr) per step, uninterrupted {log_whole} / resumed {log}")
    assert log == log_whole, (log, log_whole)                            # losses, gradient norms and learning rates, exactly
    _assert_same(want, _snapshot(resumed), f"rank {rank}")
    return layout


# ------------------------------------------------------------------------------------------------ 5. world 1
@pytest.mark.parametrize("fixed", [True, False], ids=["fixed_draws", "device_generator_draws"])
def test_world1_resume_on_the_real_kernels(dev, tmp_path, fixed):
    layout = _resume_case(dev, tmp_path, fixed=fixed)
    assert layout == dict(coll=False, inplace=False, arenas=True, world=1)


def test_device_generator_draws_depend_on_the_restored_state(dev, tmp_path):
    """The generator variant above is not vacuous: the same continuation WITHOUT the saved generator state sees other noise."""
    torch.manual_seed(1234)
    first = _strategy(_build(dev), dev, 1, 3)
    _steps(first, first.vlm, dev, 1, fixed=False)
    path = first.save_checkpoint(tmp_path, 1, 0, only_trainable=False, save_optimizer=True)
    blob = torch.load(_opt_file(path), map_location="cpu", weights_only=True)
    assert blob["rng"]["world"] == 1 and blob["rng"]["device"][0].dtype == torch.uint8
    assert torch.equal(blob["rng"]["device"][0], torch.cuda.get_rng_state(dev))
    nxt = _steps(first, first.vlm, dev, 1, fixed=False)[0]
    losses = {}
    for restore in (True, False):
        torch.manual_seed(99)
        s = _strategy(_model_from_file(dev, path), dev, 1, 3)
        s.load_optimizer_and_scheduler(path, restore_rng=restore)
        losses[restore] = _steps(s, s.vlm, dev, 1, fixed=False)[0]
    assert losses[True] == nxt and losses[False][0] != nxt[0], (nxt, losses)


# ------------------------------------------------------------------------------------------------ 6. arenas and layouts
def test_world1_resume_without_arenas(dev, tmp_path, monkeypatch):
    monkeypatch.setenv("MLA_FSDP_ARENAS", "0")
    layout = _resume_case(dev, tmp_path, fixed=True)
    assert layout == dict(coll=False, inplace=False, arenas=False, world=1)


CHILD = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import torch.distributed as dist
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
import test_optimizer_resume_gpu as t
print("LAYOUT", sorted(t._resume_case(dev, sys.argv[1], fixed=True).items()))
dist.destroy_process_group()
"""


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace_reduce_scatter", "separate_gradient_shards"])
def test_world1_resume_under_forced_collectives(dev, tmp_path, inplace):
    """The sharded layouts through the real RCCL entry points at world 1 (MLA_FORCE_COLLECTIVES=1 over a one-rank nccl group, as
    tests/test_fsdp_rccl_world1_gpu.py forces them): moments gathered over the process group on save, the rank's slice taken on load."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", MLA_FORCE_COLLECTIVES="1")
    if not inplace:
        env["MLA_FSDP_INPLACE_RS"] = "0"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path), ROOT], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    want = sorted(dict(coll=True, inplace=inplace, arenas=True, world=1).items())
    assert f"LAYOUT {want}" in r.stdout, r.stdout[-1500:]
    print(r.stdout[-1500:])


# ------------------------------------------------------------------------------------------------ 7. two gloo ranks on one GPU
def _worker(rank, world, port, run_dir, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = _resume_case(dev, run_dir, fixed=True, world=world, rank=rank, before=2, after=1)
    finally:
        dist.destroy_process_group()


def test_two_ranks_resume_and_load_into_one_process(dev, tmp_path):
    """2 steps + save + resume + 1 step == 3 steps on each of two gloo ranks sharing the GPU; the file they wrote then loads into a
    one-process strategy whose gathered moments are the file's tensors."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, f"rank process failed (exit code {p.exitcode})"
    assert ret[0] == ret[1] == dict(coll=True, inplace=False, arenas=True, world=2)
    path = _ckpt(tmp_path, 2)
    blob = torch.load(_opt_file(path), map_location="cpu", weights_only=True)
    assert blob["rng"]["world"] == 2 and blob["step"] == blob["step_count"] == 2
    one = _strategy(_model_from_file(dev, path), dev, 1, blob["hyper"]["num_training_steps"])
    with pytest.warns(UserWarning, match="generator states of 2"):
        one.load_optimizer_and_scheduler(path)
    assert one.step == 2 and one.sharded.step_count == 2
    got = {n: (m, v) for n, m, v in one.sharded.iter_optimizer_state(to_cpu_on_rank0=True)}
    assert got.keys() == blob["state"].keys()
    bad = [n for n, (m, v) in got.items()
           if not (m.device.type == "cpu" and torch.equal(m, blob["state"][n]["exp_avg"]) and torch.equal(v, blob["state"][n]["exp_avg_sq"]))]
    assert not bad, bad[:8]
    assert sum(int(d["exp_avg"].abs().sum() > 0) for d in blob["state"].values()) > len(got) // 2
