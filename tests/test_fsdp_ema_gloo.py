"""CPU, gloo at worlds 1, 2 and 8: the sharded weight average (EMA) of mla_amd.fsdp.ShardedModel, BIT FOR BIT against an unsharded
loop that applies the same element-wise ops per parameter.

Model, integer gradients (exact sums in any order) and layout facts are those of tests/test_fsdp_world8_gloo.py: at world 8 a block's
shard straddles the decay boundary (rank 6), one is partly padding (rank 7), `tower` has a frozen tail and `frozen_tower`
no trainable parameter at all. The ops class below is that file's torch implementation + the three EMA methods HipLocalOps has."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_fsdp_world8_gloo as W8

DECAY = 0.99
STEPS = 5
LR, WD, BETAS, EPS, MAX_NORM = 1e-2, 0.1, (0.9, 0.999), 1e-8, 0.05


class _EmaMethods:
    """The weight average: folded into either AdamW call, and as a pass of its own. Every product and the sum are separate rounded
    operations, so an element's result does not depend on where in a buffer it sits."""

    def ema_update(self, ema, p32, decay):
        ema.copy_(ema * decay + p32 * (1.0 - decay))

    def adamw_ema(self, p32, g32, m, v, ema, p16, lr, betas, eps, wd, step, grad_scale, ema_decay):
        self.adamw(p32, g32, m, v, p16, lr, betas, eps, wd, step, grad_scale)
        self.ema_update(ema, p32, ema_decay)

    def adamw_ema_groups(self, p32, g32, m, v, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay):
        self.adamw_groups(p32, g32, m, v, p16, n_decay, lr, betas, eps, wd, step, grad_scale)
        self.ema_update(ema, p32, ema_decay)


class EmaOps(_EmaMethods, W8.GroupedOps):
    pass


class PerRangeEmaOps(_EmaMethods, W8.TorchLocalOps):
    """without adamw_groups: optimizer_step goes range by range through adamw / adamw_ema (adamw_ema_groups is never reached)"""


def _policy(mod):
    return isinstance(mod, (W8.Block, W8.Tower))


def _sharded(ops=None, **kw):
    from mla_amd.fsdp import ShardedModel
    model = W8._make()
    return model, ShardedModel(model, _policy, torch.device("cpu"), ops=ops or EmaOps(), no_decay=W8._no_decay, **kw)


def _real_mask(u, rank):
    """True where the rank's shard of the unit's trainable region holds a parameter element (False: padding)."""
    full = torch.zeros(u.n_train, dtype=torch.bool)
    for _, p, o in u.params:
        if p.requires_grad:
            full[o:o + p.numel()] = True
    return full[rank * u.shard_train:(rank + 1) * u.shard_train]


def _train(rank, world, every, ops):
    """STEPS optimizer steps on the sharded model and on the unsharded per-parameter loop; returns (sm, reference EMA by name)."""
    model, sm = _sharded(ops, ema_decay=DECAY, ema_update_every=every)
    order = list(model.named_parameters())
    ref = W8._make()
    rp = {n: p.detach().clone().float() for n, p in ref.named_parameters()}
    rm = {n: torch.zeros_like(t) for n, t in rp.items()}
    rv = {n: torch.zeros_like(t) for n, t in rp.items()}
    re = {n: rp[n].clone() for n, p in order if p.requires_grad}
    for u in sm.units:
        if u.trainable:
            assert u.ema.dtype == torch.float32 and u.ema.numel() == u.shard_train
            assert torch.equal(u.ema, u.master_train[:u.shard_train]) and u.ema.data_ptr() != u.master_train.data_ptr()
        else:
            assert not hasattr(u, "ema")
    ref_ops = EmaOps()
    for step in range(1, STEPS + 1):
        sm.begin_step()
        for pidx, (n, p) in enumerate(order):
            if p.requires_grad:
                p.main_grad.copy_(W8._int_grad(p.shape, step, rank, pidx))
                p._mg_touched = True
        sm.finish_backward()
        sm.grad_norm_and_clip(MAX_NORM)
        sm.optimizer_step(LR, betas=BETAS, eps=EPS, weight_decay=WD)
        for pidx, (n, p) in enumerate(order):
            if not p.requires_grad:
                continue
            mean = sum(W8._int_grad(p.shape, step, r, pidx) for r in range(world)) / world
            ref_ops.adamw(rp[n], mean, rm[n], rv[n], torch.empty(p.shape, dtype=torch.bfloat16), LR, BETAS, EPS,
                          0.0 if W8._no_decay(n, p) else WD, step, sm._coef * sm.grad_div)
            if step % every == 0:
                ref_ops.ema_update(re[n], rp[n], DECAY)
    full = sm.full_state_dict_fp32()
    assert all(torch.equal(full[n], rp[n]) for n, _ in order), "fp32 masters"
    return sm, re


def _check(sm, re, rank, every):
    assert sm.ema_updates == STEPS // every and sm.step_count == STEPS
    got = dict(sm.iter_ema_state())
    assert list(got) == [n for u in sm.units if u.trainable for n, p, _ in u.params if p.requires_grad] and set(got) == set(re)
    bad = [n for n in re if not (got[n].shape == re[n].shape and torch.equal(got[n], re[n]))]
    assert not bad, (every, bad)
    assert any(not torch.equal(re[n], full) for n, full in sm.full_state_dict_fp32().items() if n in re)      # it lags the masters
    for u in sm.units:
        if u.trainable:
            mask = _real_mask(u, rank)
            assert bool((u.ema[~mask] == 0).all()), (u.name, "padding of the average moved")
            assert bool((u.master_train[:u.shard_train][~mask] == 0).all())
    host = dict(sm.iter_ema_state(to_cpu_on_rank0=True))
    assert list(host) == list(got)
    assert all(torch.equal(host[n], re[n]) for n in re) if rank == 0 else all(v is None for v in host.values())


def _check_load_refusals(sm):
    got = dict(sm.iter_ema_state())
    before = [u.ema.clone() for u in sm.units if u.trainable]
    name = next(iter(got))
    zeros = {n: torch.zeros_like(t) for n, t in got.items()}       # (applied even in part, any of these states would show)
    missing = {n: t for n, t in zeros.items() if n != name}
    extra = dict(zeros, **{"no.such.weight": torch.zeros(3)})
    shape = dict(zeros, **{list(got)[-1]: torch.zeros(got[list(got)[-1]].numel() + 1)})
    for state, word in ((missing, "missing"), (extra, "unexpected"), (shape, "wrong shape")):
        with pytest.raises(ValueError, match=word):
            sm.load_ema_state(state, 77)
        assert sm.ema_updates != 77
        assert all(torch.equal(u.ema, b) for u, b in zip((u for u in sm.units if u.trainable), before)), word


def _check_swap(sm):
    """ema_weights() with real collectives: the replica of every rank holds bf16(average) of ALL shards inside, the former bits after."""
    before = [u.flat16.clone() for u in sm.units]
    ema = dict(sm.iter_ema_state())
    with sm.ema_weights():
        for u in sm.units:
            for n, p, _ in u.params:
                if p.requires_grad:
                    assert torch.equal(p.detach(), ema[n].to(torch.bfloat16)), n
    assert all(torch.equal(u.flat16, b) for u, b in zip(sm.units, before))


def _worker(rank, world, port, out_path, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for every, ops in ((1, EmaOps()), (2, EmaOps()), (2, PerRangeEmaOps())):
            assert hasattr(ops, "adamw_ema_groups") and (type(ops) is EmaOps) == hasattr(ops, "adamw_groups")
            sm, re = _train(rank, world, every, ops)
            _check(sm, re, rank, every)
        _check_load_refusals(sm)
        _check_swap(sm)
        if world == 8:
            blk = sm.units[3]
            assert (blk.n_decay, blk.n_train, blk.shard_train) == (832, 960, 120)         # ranks 6 and 7: see the module docstring
            assert 0 < int(_real_mask(blk, 7).sum()) < blk.shard_train                    # rank 7: part parameters, part padding
            assert [d for _, _, _, d in blk._shard_ranges()] == ([True, False] if rank == 6 else [rank < 6])
        if out_path:
            state = dict(sm.iter_ema_state(to_cpu_on_rank0=True))
            if rank == 0:
                torch.save({"ema": state, "ema_updates": sm.ema_updates}, out_path)
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def _loader(rank, world, port, path, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        blob = torch.load(path, map_location="cpu", weights_only=True)
        _, sm = _sharded(ema_decay=DECAY)
        assert sm.ema_updates == 0
        sm.load_ema_state(blob["ema"], blob["ema_updates"])
        assert sm.ema_updates == blob["ema_updates"] == STEPS // 2
        got = dict(sm.iter_ema_state())
        assert list(got) == list(blob["ema"]) and all(torch.equal(got[n], t) for n, t in blob["ema"].items())
        for u in sm.units:
            if u.trainable:
                assert bool((u.ema[~_real_mask(u, rank)] == 0).all())
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def _spawn(fn, world, *args):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(fn, args=(world, port) + args + (ret,), nprocs=world, join=True)
    assert dict(ret) == {r: "ok" for r in range(world)}


@pytest.mark.parametrize("world", [1, 8])
def test_sharded_ema_bit_exact(world):
    """k = 5 steps, ema_update_every 1 and 2, two-group and per-range launches; padding stays 0; refused loads change nothing."""
    _spawn(_worker, world, None)


def test_sharded_ema_world2_and_its_state_at_worlds_1_and_8(tmp_path):
    """The same at world 2, whose gathered state (written by rank 0) then loads at world 1 and at world 8 to the same tensors."""
    path = str(tmp_path / "ema_world2.pt")
    _spawn(_worker, 2, path)
    for world in (1, 8):
        _spawn(_loader, world, path)


def test_off_by_default_nothing_changes():
    _, off = _sharded()
    _, on = _sharded(ema_decay=DECAY)
    assert off.ema_decay is None and off.ema_updates == 0
    assert not any(hasattr(u, "ema") for u in off.units)
    assert off._arenas is not None and not off._arenas.has("ema") and on._arenas.has("ema")
    # without an average: bf16 replica + fp32 masters, and gradient buffer + two moments over the trainable region (world 1: no shards)
    plain = sum(u.n_total * (2 + 4) + (u.n_train * 4 * 3 if u.trainable else 0) for u in off.units)
    assert off.state_bytes() == plain
    assert on.state_bytes() == plain + 4 * sum(u.n_train for u in on.units if u.trainable)
    for u in on.units:
        if u.trainable:
            assert (u.ema.data_ptr() - on._arenas.buf["ema"].data_ptr()) % (2 << 20) == 0, (u.name, "EMA arena slices: 2 MiB aligned")
    with pytest.raises(RuntimeError, match="ema_decay"):
        next(off.iter_ema_state())
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.load_ema_state({}, 0)
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.ema_weights().__enter__()


def test_ops_without_the_ema_methods_raise_at_construction():
    with pytest.raises(TypeError, match="adamw_ema, adamw_ema_groups, ema_update"):
        _sharded(W8.GroupedOps(), ema_decay=DECAY)

    class Partial(W8.GroupedOps):
        def ema_update(self, ema, p32, decay):
            pass
    with pytest.raises(TypeError, match="lacks adamw_ema, adamw_ema_groups$"):
        _sharded(Partial(), ema_decay=DECAY)
    _sharded(W8.GroupedOps())                                   # without a decay the same ops are fine
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            _sharded(ema_decay=bad)
    with pytest.raises(ValueError):
        _sharded(ema_decay=DECAY, ema_update_every=0)


def test_ema_weights_swaps_the_replica_and_back():
    """World 1 on the CPU: inside the context the bf16 parameters hold bf16(average), afterwards the former bits; every swapped
    parameter's version counter moves both ways; re-entry and an open accumulation window raise."""
    model, sm = _sharded(ema_decay=0.5)
    order = list(model.named_parameters())
    for step in (1, 2):
        sm.begin_step()
        for pidx, (n, p) in enumerate(order):
            if p.requires_grad:
                p.main_grad.copy_(W8._int_grad(p.shape, step, 0, pidx))
                p._mg_touched = True
        sm.finish_backward()
        sm.grad_norm_and_clip(MAX_NORM)
        sm.optimizer_step(LR, weight_decay=WD)
    before = [u.flat16.clone() for u in sm.units]
    ema = dict(sm.iter_ema_state())
    v0 = {n: p._version for n, p in order}
    with sm.ema_weights() as inside:
        assert inside is sm
        v1 = {n: p._version for n, p in order}
        for n, p in order:
            if p.requires_grad:
                assert torch.equal(p.detach(), ema[n].to(torch.bfloat16)) and v1[n] != v0[n], n
            else:
                assert v1[n] == v0[n]
        assert any(not torch.equal(u.flat16, b) for u, b in zip(sm.units, before))
        with pytest.raises(RuntimeError, match="already open"):
            sm.ema_weights().__enter__()
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            sm.optimizer_step(LR)
    assert all(torch.equal(u.flat16, b) for u, b in zip(sm.units, before))
    assert all(p._version != v1[n] for n, p in order if p.requires_grad)
    assert all(torch.equal(t, ema[n]) for n, t in sm.iter_ema_state())           # the average itself was not touched
    sm.defer_reduce = True
    with pytest.raises(RuntimeError, match="accumulation window"):
        sm.ema_weights().__enter__()
    sm.defer_reduce = False
    with sm.ema_weights():
        pass
