"""CPU: optimizer-state checkpoints and bit-exact resume (FSDPStrategy.save_checkpoint(save_optimizer=True) /
load_optimizer_and_scheduler, ShardedModel.iter_optimizer_state / load_optimizer_state).

The toy models, the injected torch arithmetic and the way ranks are spawned are those of tests/test_fsdp_gloo.py and
tests/test_fsdp_world8_gloo.py; a thin wrapper gives the toys the surface FSDPStrategy drives (MLA's forward signature, the wrapping
policy, module keys). Every comparison is torch.equal: an interrupted and continued run must leave the SAME bits as an
uninterrupted one -- fp32 masters, both AdamW moments, the bf16 compute copies, step counters and the learning rate of every step --
and a state written at one world size must load at another with the gathered moments equal to the file's tensors."""
import os
import socket
import warnings
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import test_fsdp_world8_gloo as w8
from test_fsdp_gloo import Block, TorchLocalOps, _make

ZERO_KEYS = ("img_pc_contrastive_loss", "tactile_contrastive_loss", "image_gen_loss", "point_cloud_gen_loss", "tactile_gen_loss")


class ToyVLA(nn.Module):
    """A plain-torch net behind the surface FSDPStrategy uses: `actions` is the net's input, the loss its mean square output."""
    all_module_keys = trainable_module_keys = ["net"]

    def __init__(self, net, unit_types=(Block,)):
        super().__init__()
        self.net = net
        self._unit_types = tuple(unit_types)
        self.llm_backbone = type("B", (), {"enable_gradient_checkpointing": lambda self: None})()

    def get_fsdp_wrapping_policy(self):
        return lambda m: isinstance(m, self._unit_types)

    def forward(self, actions=None, **kw):
        loss = self.net(actions).float().pow(2).mean()
        out = {"total_loss": loss, "diff_loss": loss}
        out.update({k: torch.zeros(()) for k in ZERO_KEYS})
        return out, None


KINDS = {
    # name: (fresh net from a seed, unit classes, input width, local ops)
    "toy": (_make, (Block,), 10, TorchLocalOps),                       # 4 units; decayed, not decayed and frozen parameters, d = 24
    "w8": (w8._make, (w8.Block, w8.Tower), 7, w8.GroupedOps),          # shards straddling the decay boundary, padding-only shards
}


def _batch(x):
    z = torch.zeros(x.shape[0], 1)
    return {"actions": x, "input_ids": z.long(), "attention_mask": z.bool(), "labels": z.long(), "images": {"front_image": z},
            "proprio": z, "camera_name": "front"}


def _x(step, rank, width):
    return torch.randn(6, width, generator=torch.Generator().manual_seed(100 * step + rank))


def _strategy(kind, net, total_steps, world=1, **kw):
    from mla_amd.strategy import FSDPStrategy
    _, units, _, ops = KINDS[kind]
    args = dict(max_steps=total_steps, global_batch_size=world, per_device_batch_size=1, learning_rate=1e-2, weight_decay=0.1,
                max_grad_norm=1.0, lr_scheduler_type="linear-warmup+cosine-decay", warmup_ratio=0.4,
                enable_gradient_checkpointing=False, local_ops=ops())
    args.update(kw)
    strat = FSDPStrategy(ToyVLA(net, units), "cpu", **args)
    strat.run_setup(100)
    return strat


def _net_from_file(kind, path, seed=7):
    """A fresh net (another initialisation) with the model file loaded: what a resuming script does before run_setup()."""
    net = KINDS[kind][0](seed)
    net.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["model"]["net"])
    return net


def _steps(strat, kind, steps, rank=0, global_rng=False):
    lrs = []
    for s in steps:
        x = torch.randn(6, KINDS[kind][2]) if global_rng else _x(s, rank, KINDS[kind][2])
        strat.train_step(_batch(x))
        lrs.append(strat.last_lr)
    return lrs


def _snapshot(strat):
    sm = strat.sharded
    return dict(master={n: t.clone() for n, t in sm.iter_full_state_fp32()},
                moments={n: (m, v) for n, m, v in sm.iter_optimizer_state()},
                bf16={n: p.detach().clone() for n, p in strat.vlm.named_parameters()},
                shards=[(u.master_train.clone(), u.exp_avg.clone(), u.exp_avg_sq.clone()) for u in sm.units if u.trainable],
                step=strat.step, step_count=sm.step_count)


def _assert_same(a, b, tag=""):
    assert (a["step"], a["step_count"]) == (b["step"], b["step_count"]), tag
    assert a["master"].keys() == b["master"].keys() and a["moments"].keys() == b["moments"].keys() and a["bf16"].keys() == b["bf16"].keys()
    for n in a["master"]:
        assert torch.equal(a["master"][n], b["master"][n]), (tag, "master", n)
        assert a["bf16"][n].dtype == torch.bfloat16 and torch.equal(a["bf16"][n], b["bf16"][n]), (tag, "bf16", n)
    for n in a["moments"]:
        assert torch.equal(a["moments"][n][0], b["moments"][n][0]), (tag, "exp_avg", n)
        assert torch.equal(a["moments"][n][1], b["moments"][n][1]), (tag, "exp_avg_sq", n)
    assert len(a["shards"]) == len(b["shards"])
    for i, (sa, sb) in enumerate(zip(a["shards"], b["shards"])):
        assert all(torch.equal(x, y) for x, y in zip(sa, sb)), (tag, "rank shards of trainable unit", i)


def _ckpt(run_dir, step):
    return Path(run_dir) / "checkpoints" / f"step-{step:06d}-epoch-00-loss=inf.pt"


def _opt_file(path):
    return path.with_name(path.stem + "-optimizer.pt")


def _check_moments_equal_file(strat, blob):
    """Gathered moments == the file's tensors bit for bit, and this rank's shards == its slice of the file laid out flat (padding 0)."""
    sm = strat.sharded
    got = {n: (m, v) for n, m, v in sm.iter_optimizer_state()}
    assert got.keys() == blob["state"].keys()
    nonzero = 0
    for n, (m, v) in got.items():
        assert m.dtype == v.dtype == torch.float32
        assert torch.equal(m, blob["state"][n]["exp_avg"]) and torch.equal(v, blob["state"][n]["exp_avg_sq"]), n
        nonzero += int(m.abs().sum() > 0)
    assert nonzero > len(got) // 2                       # the comparison is not one of zeros
    for u in sm.units:
        if not u.trainable:
            continue
        flat = torch.zeros(2, u.n_train)
        for n, p, o in u.params:
            if p.requires_grad:
                flat[0, o:o + p.numel()] = blob["state"][n]["exp_avg"].reshape(-1)
                flat[1, o:o + p.numel()] = blob["state"][n]["exp_avg_sq"].reshape(-1)
        lo = sm.rank * u.shard_train
        assert torch.equal(u.exp_avg, flat[0, lo:lo + u.shard_train]) and torch.equal(u.exp_avg_sq, flat[1, lo:lo + u.shard_train]), u.name
    assert strat.step == blob["step"] and sm.step_count == blob["step_count"]


# ---------------------------------------------------------------------------------------------------------------- 1. world 1
@pytest.mark.parametrize("global_rng", [False, True], ids=["seeded_batches", "global_generator_batches"])
def test_world1_resume_is_bit_exact(tmp_path, global_rng):
    """5 steps in one go == 3 steps + save + fresh model from the model file + fresh strategy + load + 2 steps. With `global_rng` the
    batches come from torch's global CPU generator, which only `restore_rng` puts back where the saving run left it."""
    whole = _strategy("toy", _make(), 5)
    torch.manual_seed(4321)
    lrs_whole = _steps(whole, "toy", range(5), global_rng=global_rng)
    assert len(set(lrs_whole)) == 5                      # warm-up then decay: restarting the schedule would show
    first = _strategy("toy", _make(), 5)
    torch.manual_seed(4321)
    lrs = _steps(first, "toy", range(3), global_rng=global_rng)
    path = first.save_checkpoint(tmp_path, 3, 0, save_optimizer=True)
    assert path == _ckpt(tmp_path, 3) and _opt_file(path).exists()
    del first
    torch.manual_seed(999)                               # a new process starts from another generator state
    resumed = _strategy("toy", _net_from_file("toy", path), 5)
    resumed.load_optimizer_and_scheduler(path)
    assert resumed.step == 3 and resumed.sharded.step_count == 3
    lrs += _steps(resumed, "toy", range(3, 5), global_rng=global_rng)
    assert lrs == lrs_whole
    _assert_same(_snapshot(whole), _snapshot(resumed))
    if global_rng:
        # and without the generator state the continued run does NOT see the same batches (the variant above is not vacuous)
        torch.manual_seed(999)
        other = _strategy("toy", _net_from_file("toy", path), 5)
        other.load_optimizer_and_scheduler(path, restore_rng=False)
        _steps(other, "toy", range(3, 5), global_rng=True)
        assert not torch.equal(_snapshot(other)["master"]["net.out.weight"], _snapshot(whole)["master"]["net.out.weight"])


# ------------------------------------------------------------------------------------------------ 2. / 3. sharded over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, world, *args):
    ret = mp.Manager().dict()
    mp.spawn(fn, args=(world, _free_port()) + args + (ret,), nprocs=world, join=True)
    assert dict(ret) == {r: "ok" for r in range(world)}, dict(ret)


def _resume_worker(rank, world, port, kind, run_dir, before, after, ret):
    """`before + after` steps uninterrupted vs `before` steps + save + fresh model / strategy + load + `after` steps, on every rank."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)                            # tiny tensors, up to 8 ranks on one host
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        make = KINDS[kind][0]
        total = before + after
        whole = _strategy(kind, make(), total, world)
        lrs_whole = _steps(whole, kind, range(total), rank)
        first = _strategy(kind, make(), total, world)
        lrs = _steps(first, kind, range(before), rank)
        torch.manual_seed(1000 + rank)
        path = first.save_checkpoint(run_dir, before, 0, save_optimizer=True)
        assert (path == _ckpt(run_dir, before)) if rank == 0 else (path is None)
        path = _ckpt(run_dir, before)
        torch.manual_seed(5)
        resumed = _strategy(kind, _net_from_file(kind, path), total, world)
        resumed.load_optimizer_and_scheduler(path)
        assert torch.equal(torch.get_rng_state(), torch.Generator().manual_seed(1000 + rank).get_state())     # this rank's own state
        lrs += _steps(resumed, kind, range(before, total), rank)
        assert lrs == lrs_whole
        _assert_same(_snapshot(whole), _snapshot(resumed), f"rank {rank}")
        # rank-0-only host gather (what save_checkpoint uses)
        got = list(resumed.sharded.iter_optimizer_state(to_cpu_on_rank0=True))
        assert all((m is not None and v is not None) if rank == 0 else (m is None and v is None) for _, m, v in got)
        # same-world load of the file: shards and gathered state equal the file
        blob = torch.load(_opt_file(path), map_location="cpu", weights_only=True)
        again = _strategy(kind, _net_from_file(kind, path), total, world)
        again.load_optimizer_and_scheduler(path)
        _check_moments_equal_file(again, blob)
        if kind == "toy":
            _inplace_layout_round_trip(again.sharded, blob)
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def _inplace_layout_round_trip(src, blob):
    """The in-place reduce-scatter layout (gradient shard inside the gradient buffer) holds its moments like the other two: a
    ShardedModel built that way takes the state and hands the same tensors back."""
    from mla_amd.fsdp import ShardedModel
    sm = ShardedModel(_make(3), lambda mod: isinstance(mod, Block), torch.device("cpu"), ops=TorchLocalOps(), inplace_reduce=True)
    assert sm.inplace_reduce and all(u.inplace_reduce for u in sm.units)
    state = {n[len("net."):]: (m, v) for n, m, v in src.iter_optimizer_state()}        # the bare net's names
    sm.load_optimizer_state(state, 11)
    assert sm.step_count == 11
    for n, m, v in sm.iter_optimizer_state():
        assert torch.equal(m, blob["state"]["net." + n]["exp_avg"]) and torch.equal(v, blob["state"]["net." + n]["exp_avg_sq"]), n


def _load_worker(rank, world, port, kind, path, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)                            # tiny tensors, up to 8 ranks on one host
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = _load_at_other_world(kind, Path(path), world)
    finally:
        dist.destroy_process_group()


def _load_at_other_world(kind, path, world):
    blob = torch.load(_opt_file(path), map_location="cpu", weights_only=True)
    assert blob["rng"]["world"] != world
    strat = _strategy(kind, _net_from_file(kind, path), blob["hyper"]["num_training_steps"], world)
    torch.manual_seed(77)
    before = torch.get_rng_state()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        strat.load_optimizer_and_scheduler(path)
    about_rng = [w for w in seen if "generator states" in str(w.message)]
    assert len(about_rng) == 1, [str(w.message) for w in seen]                # the saved generators are not applied: said once
    assert torch.equal(torch.get_rng_state(), before)
    _check_moments_equal_file(strat, blob)
    return "ok"


@pytest.fixture(scope="module")
def world2_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("world2")
    _spawn(_resume_worker, 2, "toy", str(d), 2, 2)
    return _ckpt(d, 2)


@pytest.fixture(scope="module")
def world8_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("world8")
    _spawn(_resume_worker, 8, "w8", str(d), 2, 1)
    return _ckpt(d, 2)


def test_world2_resume_is_bit_exact_on_every_rank(world2_run):
    """4 steps == 2 + save + resume + 2 at world 2, per-rank shards and gathered state (asserted inside the ranks)."""
    blob = torch.load(_opt_file(world2_run), map_location="cpu", weights_only=True)
    assert blob["step"] == blob["step_count"] == 2 and blob["rng"]["world"] == 2
    assert len(blob["rng"]["cpu"]) == 2 and blob["rng"]["device"] == [None, None]
    for r in range(2):                                                           # every rank's own generator state is in the file
        assert torch.equal(blob["rng"]["cpu"][r], torch.Generator().manual_seed(1000 + r).get_state())


def test_world2_state_loads_at_world1_and_world4(world2_run):
    assert _load_at_other_world("toy", world2_run, 1) == "ok"
    _spawn(_load_worker, 4, "toy", str(world2_run))


def test_world8_layout_round_trips_8_to_8_and_8_to_1(world8_run):
    """The world-8 layout: shards that straddle the decayed / not-decayed boundary, shards of nothing but padding, a 3-element
    parameter. 8 -> 8 (resume equality and file equality, inside the ranks) and 8 -> 1 here."""
    from mla_amd.fsdp import plan_flat_layout
    blob = torch.load(_opt_file(world8_run), map_location="cpu", weights_only=True)
    assert blob["rng"]["world"] == 8 and len(blob["rng"]["cpu"]) == 8
    net = w8._make()
    frozen = {"net." + n for n, p in net.named_parameters() if not p.requires_grad}
    assert frozen and not (frozen & set(blob["state"]))                          # trainable parameters only
    assert blob["state"]["net.scale"]["exp_avg"].shape == (3,)                   # the padding of the flat layout is not in the file
    blk = [(n, p) for n, p in net.layers[0].named_parameters()]
    _, n_decay, n_train, _ = plan_flat_layout(blk, 8)
    assert (n_decay, n_train) == (832, 960)                                      # rank 6 straddles 832, rank 7 is 8 real elements + padding
    assert _load_at_other_world("w8", world8_run, 1) == "ok"


# ------------------------------------------------------------------------------------------------ 4. refusals and defaults
def test_refusals_defaults_and_file_format(tmp_path):
    from mla_amd.strategy import FSDPStrategy
    # ---- a save inside an accumulation window is refused; without the option the same call writes the model file alone
    acc = _strategy("toy", _make(), 6, global_batch_size=2)
    assert acc.grad_accumulation_steps == 2 and acc.save_optimizer_state is False
    acc.train_step(_batch(_x(0, 0, 10)))
    with pytest.raises(RuntimeError, match="accumulation window"):
        acc.save_checkpoint(tmp_path / "acc", 0, 0, save_optimizer=True)
    assert not (tmp_path / "acc").exists()
    acc.save_checkpoint(tmp_path / "acc", 0, 0)
    assert [f.name for f in (tmp_path / "acc" / "checkpoints").iterdir()] == ["step-000000-epoch-00-loss=inf.pt"]
    acc.train_step(_batch(_x(1, 0, 10)))                                         # window closed: allowed again
    acc.save_optimizer_state = True
    p2 = acc.save_checkpoint(tmp_path / "acc2", 1, 0)
    assert {f.name for f in p2.parent.iterdir()} == {p2.name, _opt_file(p2).name}
    assert FSDPStrategy(ToyVLA(_make()), "cpu", save_optimizer_state=True).save_optimizer_state is True

    # ---- the file: plain containers and tensors, no weights
    strat = _strategy("toy", _make(), 5)
    _steps(strat, "toy", range(2))
    path = strat.save_checkpoint(tmp_path, 2, 0, save_optimizer=True)
    assert isinstance(path, Path) and path.name == "step-000002-epoch-00-loss=inf.pt"
    blob = torch.load(_opt_file(path), map_location="cpu", weights_only=True)
    assert set(blob) == {"format", "step", "step_count", "hyper", "state", "rng"} and blob["format"] == "mla_amd.optimizer/1"
    assert blob["step"] == 2 and blob["step_count"] == 2
    assert blob["hyper"] == dict(lr_scheduler_type="linear-warmup+cosine-decay", learning_rate=1e-2, weight_decay=0.1,
                                 num_training_steps=5, num_warmup_steps=2)
    trainable = [n for n, p in strat.vlm.named_parameters() if p.requires_grad]
    assert list(blob["state"]) == [n for n, _ in strat.sharded.iter_full_state_fp32() if n in set(trainable)]
    assert set(blob["state"]) == set(trainable) and "net.frozen.weight" not in blob["state"]
    for n, d in blob["state"].items():
        assert set(d) == {"exp_avg", "exp_avg_sq"}
        assert all(t.dtype == torch.float32 and t.shape == dict(strat.vlm.named_parameters())[n].shape for t in d.values())
    assert blob["rng"]["world"] == 1 and blob["rng"]["cpu"][0].dtype == torch.uint8 and blob["rng"]["device"] == [None]

    # ---- load_optimizer_state validates before it writes: the state afterwards is the state before, bit for bit
    sm = strat.sharded
    good = {n: (m, v) for n, m, v in sm.iter_optimizer_state()}
    victim = "net.layers.1.b.bias"
    other = {n: (torch.full_like(m, 3.0), torch.full_like(v, 5.0)) for n, (m, v) in good.items()}
    cases = {"missing": {n: mv for n, mv in other.items() if n != victim},
             "unexpected": dict(other, **{"net.frozen.weight": (torch.zeros(24, 24), torch.zeros(24, 24))}),
             "wrong shape": dict(other, **{victim: (torch.zeros(25), torch.zeros(24))})}
    before = _snapshot(strat)
    for what, state in cases.items():
        name = "net.frozen.weight" if what == "unexpected" else victim
        with pytest.raises(ValueError) as err:
            sm.load_optimizer_state(state, 40)
        assert f"{what}: {name}" in str(err.value), str(err.value)
        _assert_same(before, _snapshot(strat), what)
    sm.load_optimizer_state(other, 40)                                            # (and a state that fits does go in)
    assert sm.step_count == 40 and all(bool((m == 3.0).all()) and bool((v == 5.0).all()) for _, m, v in sm.iter_optimizer_state())
    assert all(float(u.exp_avg.sum()) == 3.0 * sum(p.numel() for _, p, _ in u.params if p.requires_grad) for u in sm.units if u.trainable)
    sm.load_optimizer_state(good, 2)
    _assert_same(before, _snapshot(strat), "restored")

    # ---- unknown format; load before run_setup; other hyper-parameters
    bad = dict(blob, format="mla_amd.optimizer/2")
    alt = tmp_path / "checkpoints" / "alt.pt"
    torch.save(bad, _opt_file(alt))
    with pytest.raises(ValueError, match="mla_amd.optimizer/2"):
        strat.load_optimizer_and_scheduler(alt)
    _assert_same(before, _snapshot(strat), "unknown format")
    unset = FSDPStrategy(ToyVLA(_make()), "cpu", local_ops=TorchLocalOps(), enable_gradient_checkpointing=False)
    with pytest.raises(RuntimeError, match="run_setup"):
        unset.load_optimizer_and_scheduler(path)
    with pytest.warns(UserWarning, match="Optimizer checkpoint not found"):      # the absent file still only warns, set up or not
        unset.load_optimizer_and_scheduler(tmp_path / "checkpoints" / "nothing-here.pt")
    changed = _strategy("toy", _net_from_file("toy", path), 5, learning_rate=5e-3)
    with pytest.warns(UserWarning, match="hyper-parameters.*learning_rate"):
        changed.load_optimizer_and_scheduler(path)
    assert changed.learning_rate == 5e-3 and changed.step == 2                   # the strategy's own values win
    _check_moments_equal_file(changed, blob)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                            # same hyper-parameters, same world: silent
        _strategy("toy", _net_from_file("toy", path), 5).load_optimizer_and_scheduler(path)


def test_run_vla_training_checkpoint_pairs_and_resumed_loop(tmp_path):
    """The loop's opt-in is the strategy attribute (run_vla_training's signature is the reference's): every checkpoint then comes as a
    pair of files, and a loop continued from the first pair -- model file into the module, run_setup, load_optimizer_and_scheduler,
    the saved step handed to `metrics`, the data from where it stopped -- ends with the uninterrupted loop's weights."""
    from torch.utils.data import IterableDataset
    from mla_amd import strategy as S

    class LoopVLA(nn.Module):
        all_module_keys = trainable_module_keys = ["body"]

        def __init__(self):
            super().__init__()
            self.body = nn.Linear(4, 1)
            self.llm_backbone = type("B", (), {"enable_gradient_checkpointing": lambda self: None})()

        def get_fsdp_wrapping_policy(self):
            return lambda m: False

        def forward(self, actions=None, **kw):
            loss = (self.body(actions.to(self.body.weight.dtype)) ** 2).mean()
            out = {"total_loss": loss, "diff_loss": loss}
            out.update({k: torch.zeros(()) for k in ZERO_KEYS})
            return out, None

    class DS(IterableDataset):
        def __init__(self, start=0):
            self.start = start

        def __iter__(self):
            i = self.start
            while True:
                yield {"actions": torch.randn(4, generator=torch.Generator().manual_seed(i))}
                i += 1

        def __len__(self):
            return 12

    def collate(items):
        z = torch.zeros(len(items), 1)
        return {"actions": torch.stack([it["actions"] for it in items]), "input_ids": z.long(), "attention_mask": z.bool(), "labels": z.long(),
                "images": {"front_image": z}, "next_images": {"front_image": z}, "proprio": z, "point_cloud": z}

    class Metrics:
        def __init__(self, run_dir, global_step=0):
            self.run_dir, self.global_step, self.lrs = run_dir, global_step, []

        def get_status(self):
            return "status"

        def commit(self, **kw):
            if "global_step" in kw:
                self.global_step = kw["global_step"]
                self.lrs.append(kw["lr"])

        def push(self):
            return "status"

    def strategy(vla):
        torch.manual_seed(0)
        strat = S.get_train_strategy("fsdp-full-shard", vla, "cpu", "finetune", epochs=2, max_steps=None, global_batch_size=4,
                                     per_device_batch_size=2, learning_rate=1e-2, weight_decay=0.1, max_grad_norm=1.0,
                                     lr_scheduler_type="linear-warmup+cosine-decay", warmup_ratio=0.34, enable_gradient_checkpointing=False,
                                     reduce_in_full_precision=True)
        strat.local_ops = TorchLocalOps()
        strat.save_optimizer_state = True
        strat.run_setup(run_dir=tmp_path, n_train_examples=12)
        assert strat.grad_accumulation_steps == 2 and strat.num_training_steps == 6 and strat.num_warmup_steps == 2
        return strat

    def loop(strat, metrics, start):
        strat.run_vla_training(DS(start), collate, metrics, save_interval=1, use_diff=True, camera_name="front")

    torch.manual_seed(0)
    whole_vla = LoopVLA()
    whole, m_whole = strategy(whole_vla), Metrics(tmp_path / "whole")
    loop(whole, m_whole, 0)
    assert m_whole.global_step == 6 and whole.step == 6
    files = sorted(f.name for f in (tmp_path / "whole" / "checkpoints").iterdir())
    models = [f for f in files if not f.endswith("-optimizer.pt")]
    assert len(files) == 4 and len(models) == 2, files
    assert models[0].startswith("step-000003-epoch-01") and models[1].startswith("step-000006-epoch-02")
    assert all(f[:-3] + "-optimizer.pt" in files for f in models)
    # resume from the first pair
    first = tmp_path / "whole" / "checkpoints" / models[0]
    vla = LoopVLA()
    vla.body.load_state_dict(torch.load(first, map_location="cpu", weights_only=True)["model"]["body"])
    resumed = strategy(vla)
    resumed.load_optimizer_and_scheduler(first)
    saved_step = torch.load(_opt_file(first), map_location="cpu", weights_only=True)["step"]
    assert saved_step == 3 == resumed.step
    m_res = Metrics(tmp_path / "resumed", global_step=saved_step)
    loop(resumed, m_res, start=saved_step * 4)                                   # 4 samples per optimizer step
    assert m_res.global_step == 6 and resumed.step == 6 and m_res.lrs == m_whole.lrs[3:]
    _assert_same(_snapshot(whole), _snapshot(resumed))
    assert len(list((tmp_path / "resumed" / "checkpoints").iterdir())) == 2       # the step-6 pair
