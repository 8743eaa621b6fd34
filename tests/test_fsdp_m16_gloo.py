"""CPU, gloo at world 2 (and world 1 in process): bf16 AdamW moments in mla_amd.fsdp.ShardedModel (moments="bf16"), BIT FOR BIT against
ONE emulated pass (tests/adamw_m16_cases.py) over each unit's whole flat trainable region -- the random bits of an element depend on
its position in that region, not on which rank holds it or how a shard is cut into launches.

Model: the blocks and towers of tests/test_fsdp_world8_gloo.py (integer gradients: exact sums in any order) plus a unit `gain` with one
3-element parameter. At world 2 a block's region is 800 decayed + 80 not decayed, shard 440: rank 1's shard [440, 880) straddles the
decay boundary; `gain`'s region is 16 elements, shard 8: rank 1's shard is nothing but padding; `frozen_tower` has no trainable
parameter. The ops class is that file's torch implementation + the EMA methods of tests/test_fsdp_ema_gloo.py + adamw_m16 built on the emulation."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import adamw_m16_cases as M
import test_fsdp_world8_gloo as W8
from test_fsdp_ema_gloo import _EmaMethods

STEPS = 3
SEED = M.SEED
DECAY = 0.99
LR, WD, BETAS, EPS, MAX_NORM = 1e-2, 0.1, (0.9, 0.999), 1e-8, 0.05


class M16Ops(_EmaMethods, W8.GroupedOps):
    """+ the EMA methods and the bf16-moment step HipLocalOps has, the latter as the numpy emulation writes it; records its launches."""

    def __init__(self):
        super().__init__()
        self.m16_calls = []

    def adamw_m16(self, p32, g32, m16, v16, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay, seed, index_base):
        assert m16.dtype == torch.bfloat16 and v16.dtype == torch.bfloat16 and p32.dtype == torch.float32
        self.m16_calls.append((p32.numel(), n_decay, index_base, ema is not None))
        pp, mo, vo, _, _ = M.adamw_m16_emul32(p32, g32, m16, v16, step, wd, None if grad_scale is None else float(grad_scale), n_decay=n_decay,
                                              seed=seed, index_base=index_base, lr=lr, beta1=betas[0], beta2=betas[1], eps=eps)
        p32.copy_(pp)
        m16.copy_(mo)
        v16.copy_(vo)
        p16.copy_(pp.to(torch.bfloat16))
        if ema is not None:
            self.ema_update(ema, p32, ema_decay)


class Gain(nn.Module):
    def __init__(self):
        super().__init__()
        self.g = nn.Parameter(torch.tensor([1.0, 0.5, -2.0]))


class Toy(W8.Toy):
    def __init__(self):
        super().__init__()
        self.gain = Gain()


def _make():
    torch.manual_seed(0)
    m = Toy()
    m.frozen_tower.requires_grad_(False)
    m.tower.tail.requires_grad_(False)
    return m


def _policy(mod):
    return isinstance(mod, (W8.Block, W8.Tower, Gain))


def _sharded(ops=None, **kw):
    from mla_amd.fsdp import ShardedModel
    model = _make()
    return model, ShardedModel(model, _policy, torch.device("cpu"), ops=ops if ops is not None else M16Ops(), no_decay=W8._no_decay, **kw)


def _flat(u, by_name):
    full = torch.zeros(u.n_train)
    for n, p, o in u.params:
        if p.requires_grad:
            full[o:o + p.numel()] = by_name[n].reshape(-1)
    return full


def _run(sm, model, rank, world, steps=STEPS, ref=None):
    """`steps` optimizer steps on the sharded model; with `ref` (per unit: [p, m16, v16] over the flat region) the emulated pass too."""
    order = list(model.named_parameters())
    for step in range(sm.step_count + 1, sm.step_count + steps + 1):
        sm.begin_step()
        for pidx, (n, p) in enumerate(order):
            if p.requires_grad:
                p.main_grad.copy_(W8._int_grad(p.shape, step, rank, pidx))
                p._mg_touched = True
        sm.finish_backward()
        sm.grad_norm_and_clip(MAX_NORM)
        sm.optimizer_step(LR, betas=BETAS, eps=EPS, weight_decay=WD)
        if ref is None:
            continue
        mean = {n: sum(W8._int_grad(p.shape, step, r, pidx) for r in range(world)) / world
                for pidx, (n, p) in enumerate(order) if p.requires_grad}
        for ordinal, u in enumerate(sm.units):
            if u.trainable:
                p0, m0, v0 = ref[u.name]
                out = M.adamw_m16_emul32(p0, _flat(u, mean), m0, v0, step, WD, float(sm._coef * sm.grad_div), n_decay=u.n_decay, seed=SEED,
                                         index_base=ordinal << 40, lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=EPS)
                ref[u.name] = list(out[:3])


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                                                                     b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ops = M16Ops()
        model, sm = _sharded(ops, moments="bf16", moments_seed=SEED, ema_decay=DECAY, ema_update_every=2)
        names = [u.name for u in sm.units]
        assert names == ["frozen_tower", "tower", "gain", "<root>", "layers.0", "layers.1", "layers.2"], names
        blk, gain, frozen = sm.units[4], sm.units[2], sm.units[0]
        assert (blk.n_decay, blk.n_train, blk.shard_train) == (800, 880, 440) and (gain.n_decay, gain.n_train, gain.shard_train) == (0, 16, 8)
        assert [(a, b, d) for a, b, _, d in blk._shard_ranges()] == ([(0, 440, True)] if rank == 0 else [(0, 360, True), (360, 440, False)])
        assert not frozen.trainable and not hasattr(frozen, "exp_avg")
        for u in sm.units:
            if u.trainable:
                assert u.exp_avg.dtype == u.exp_avg_sq.dtype == torch.bfloat16 and u.exp_avg.numel() == u.shard_train
                assert u.ema.dtype == torch.float32 and u.master_train.dtype == torch.float32
        frozen_before = (frozen.master_frozen.clone(), frozen.flat16.clone())
        ref = {u.name: [sm._gather_master(u)[:u.n_train].clone(), torch.zeros(u.n_train, dtype=torch.bfloat16),
                        torch.zeros(u.n_train, dtype=torch.bfloat16)] for u in sm.units if u.trainable}
        _run(sm, model, rank, world, ref=ref)
        # one launch per unit and step where the shard is [decayed | not decayed] back to back (all of these), EMA on even steps
        per_step = sum(u.trainable for u in sm.units)
        assert len(ops.m16_calls) == STEPS * per_step and sum(c[3] for c in ops.m16_calls) == per_step
        assert (440, 360 if rank else 440, (4 << 40) + rank * 440, False) in ops.m16_calls
        assert (8, 0, (2 << 40) + rank * 8, True) in ops.m16_calls
        for u in sm.units:
            if not u.trainable:
                continue
            p, m16, v16 = ref[u.name]
            gm, gv = sm._gather_moments(u)
            assert gm.dtype == torch.bfloat16 and _bits(gm, m16) and _bits(gv, v16), (u.name, "moments differ from the one emulated pass")
            assert torch.equal(sm._gather_master(u)[:u.n_train], p), (u.name, "masters")
            assert int((m16.float() != 0).sum()) > 0
        # the padding-only shard stayed zero in every stream; the frozen unit was not touched
        if rank == 1:
            assert all(bool((t == 0).all()) for t in (gain.master_train, gain.exp_avg.float(), gain.exp_avg_sq.float(), gain.ema))
        assert torch.equal(frozen.master_frozen, frozen_before[0]) and torch.equal(frozen.flat16, frozen_before[1])
        # ---- state helpers: bf16 tensors, the stored bits; the other format is refused before the first write
        state = {n: (a, b) for n, a, b in sm.iter_optimizer_state()}
        assert all(a.dtype == b.dtype == torch.bfloat16 for a, b in state.values())
        host = list(sm.iter_optimizer_state(to_cpu_on_rank0=True))
        assert all((a.dtype == torch.bfloat16 and _bits(a, state[n][0])) if rank == 0 else a is None for n, a, _ in host)
        before = [(u.exp_avg.clone(), u.exp_avg_sq.clone()) for u in sm.units if u.trainable]
        with pytest.raises(ValueError, match="(?s)float32.*bfloat16.*'fp32'.*'bf16'"):
            sm.load_optimizer_state({n: (a.float(), b.float()) for n, (a, b) in state.items()}, 77)
        assert sm.step_count == STEPS
        assert all(_bits(u.exp_avg, b[0]) and _bits(u.exp_avg_sq, b[1]) for u, b in zip((u for u in sm.units if u.trainable), before))
        _, other = _sharded(M16Ops(), moments="bf16", moments_seed=SEED)
        other.load_optimizer_state(state, sm.step_count)
        assert other.step_count == STEPS
        assert all(_bits(a.exp_avg, b.exp_avg) and _bits(a.exp_avg_sq, b.exp_avg_sq) for a, b in zip(other.units, sm.units) if a.trainable)
        _, plain = _sharded(M16Ops())
        with pytest.raises(ValueError, match="(?s)bfloat16.*float32"):
            plain.load_optimizer_state(state, 77)
        assert plain.step_count == 0 and all(bool((u.exp_avg == 0).all()) for u in plain.units if u.trainable)
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_world2_equals_one_emulated_pass_over_the_flat_region():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    assert dict(ret) == {0: "ok", 1: "ok"}


def test_fp32_keyword_is_the_default_bit_for_bit():
    runs = []
    for kw in ({}, dict(moments="fp32", moments_seed=5)):
        ops = M16Ops()
        model, sm = _sharded(ops, **kw)
        _run(sm, model, 0, 1)
        assert not ops.m16_calls and sm.moments == "fp32"
        assert all(u.exp_avg.dtype == torch.float32 for u in sm.units if u.trainable)
        runs.append((sm.full_state_dict_fp32(), {n: (a, b) for n, a, b in sm.iter_optimizer_state()}, [u.flat16.clone() for u in sm.units],
                     sm.state_bytes()))
    a, b = runs
    assert all(torch.equal(a[0][n], b[0][n]) for n in a[0]) and a[0].keys() == b[0].keys()
    assert all(torch.equal(a[1][n][0], b[1][n][0]) and torch.equal(a[1][n][1], b[1][n][1]) for n in a[1]) and a[1].keys() == b[1].keys()
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and a[3] == b[3]


def test_state_bytes_and_arenas_with_bf16_moments():
    from mla_amd.fsdp import plan_sharded_layout
    _, off = _sharded()
    _, on = _sharded(moments="bf16")
    n_train = sum(u.n_train for u in on.units if u.trainable)
    assert off.state_bytes() - on.state_bytes() == 2 * 2 * n_train          # two moments, 4 -> 2 bytes each
    for kind in ("exp_avg", "exp_avg_sq"):
        assert on._arenas.buf[kind].dtype == torch.bfloat16 and off._arenas.buf[kind].dtype == torch.float32
        assert on._arenas.buf[kind].numel() * 2 <= off._arenas.buf[kind].numel() * 4
    for u in on.units:
        if u.trainable:
            assert (u.exp_avg.data_ptr() - on._arenas.buf["exp_avg"].data_ptr()) % (2 << 20) == 0, (u.name, "arena slices: 2 MiB aligned")
    plans = {m: plan_sharded_layout(_make(), _policy, 2, W8._no_decay, moments=m) for m in ("fp32", "bf16")}
    assert sum(u["bytes_moments"] for u in plans["fp32"]) == 2 * sum(u["bytes_moments"] for u in plans["bf16"]) == 8 * sum(u["shard_train"] for u in plans["fp32"])


def test_unknown_format_and_ops_without_the_step_raise():
    with pytest.raises(ValueError, match="moments must be one of"):
        _sharded(moments="fp16")
    with pytest.raises(TypeError, match="lacks adamw_m16"):
        _sharded(W8.GroupedOps(), moments="bf16")
    _sharded(W8.GroupedOps(), moments="fp32")                  # the same ops are fine with fp32 moments
