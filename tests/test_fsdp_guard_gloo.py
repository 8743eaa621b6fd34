"""CPU, gloo at world 2 (and world 1 in process): ShardedModel(skip_nonfinite=True) -- a step whose global gradient norm is +inf or NaN
does nothing on any rank, the counters count applied steps, and the run continues as if the batch had never been seen -- BIT FOR BIT
against an unguarded model that never saw the bad batch.

Model, integer gradients (exact sums in any order) and ops are those of tests/test_fsdp_m16_gloo.py (blocks whose rank-1 shard
straddles the decay boundary, a unit that is nothing but padding on rank 1, a frozen unit); the ops class adds the two guard methods
of tests/guard_cases.py. At world 2 the bad value sits in RANK 1's gradient only, at an element of layers.1.a.weight that the
reduction hands to RANK 0's shard: rank 1's own sum of squares is finite, it skips because the flag is decided after the all-reduce.
The checkpoint tests drive FSDPStrategy over the toys of tests/test_optimizer_state_host.py with real autograd gradients."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import guard_cases as GC
import test_fsdp_m16_gloo as G16
import test_fsdp_world8_gloo as W8
import test_optimizer_state_host as OS

LR, WD, BETAS, EPS, MAX_NORM = G16.LR, G16.WD, G16.BETAS, G16.EPS, G16.MAX_NORM
DECAY = 0.99
BAD_PARAM, BAD_INDEX = "layers.1.a.weight", 5
INF, NAN = float("inf"), float("nan")


class GuardOps(GC.GuardMethods, G16.M16Ops):
    """the ops of the bf16-moment test (torch AdamW, EMA, emulated bf16-moment step) + clip_coef_guard / adamw_guard"""


def _sharded(ops=None, **kw):
    from mla_amd.fsdp import ShardedModel
    model = G16._make()
    return model, ShardedModel(model, G16._policy, torch.device("cpu"), ops=ops if ops is not None else GuardOps(), no_decay=W8._no_decay, **kw)


def _step(sm, model, rank, world, tag, bad=None, clip=True):
    """One optimizer step on the integer gradients of `tag`; `bad` (inf / NaN) goes into the LAST rank's gradient only."""
    sm.begin_step()
    for pidx, (n, p) in enumerate(model.named_parameters()):
        if p.requires_grad:
            g = W8._int_grad(p.shape, tag, rank, pidx)
            if bad is not None and rank == world - 1 and n == BAD_PARAM:
                g.view(-1)[BAD_INDEX] = bad
            p.main_grad.copy_(g)
            p._mg_touched = True
    sm.finish_backward()
    if clip:
        sm.grad_norm_and_clip(MAX_NORM)
    sm.optimizer_step(LR, betas=BETAS, eps=EPS, weight_decay=WD)


def _state(sm):
    out = []
    for u in sm.units:
        out += [u.master_train, u.master_frozen, u.flat16]
        if u.trainable:
            out += [u.exp_avg, u.exp_avg_sq] + ([u.ema] if hasattr(u, "ema") else [])
    return [t.clone() for t in out]


def _same(a, b):
    return len(a) == len(b) and all(G16._bits(x, y) for x, y in zip(a, b))


def _scenario(rank, world, moments, bad):
    kw = dict(moments=moments, moments_seed=G16.SEED, ema_decay=DECAY, ema_update_every=2)
    per_step = 6                                             # trainable units = launches per step (every shard is back to back)
    # ---- [good, bad]: the bad step changes nothing, on either rank
    ops = GuardOps()
    model, sm = _sharded(ops, skip_nonfinite=True, **kw)
    assert sm.skipped_steps == 0 and sm._skip.dtype == torch.int32 and sm._skip.numel() == 1
    _step(sm, model, rank, world, 1)
    assert (sm.step_count, sm.ema_updates, sm.skipped_steps) == (1, 0, 0)
    before = _state(sm)
    _step(sm, model, rank, world, 2, bad=bad)
    assert int(sm._skip) == 1 and float(sm._coef) == 0.0 and not torch.isfinite(sm._norm).item()
    if world == 2 and rank == 1:                             # this rank's own shards held nothing bad
        assert all(bool(torch.isfinite(u.gshard).all()) for u in sm.units if u.trainable)
    assert _same(_state(sm), before), "a skipped step wrote something"
    # launched as step 2 (an EMA step), taken back when the flag is read
    assert sm._skip_pending is not None and sm._step_count == 2
    assert (sm.step_count, sm.ema_updates, sm.skipped_steps) == (1, 0, 1) and sm._skip_pending is None
    # ---- [good, bad, good] == [good, good] unguarded, counters never read in between
    ops = GuardOps()
    model, sm = _sharded(ops, skip_nonfinite=True, **kw)
    for tag, b in ((1, None), (2, bad), (3, None)):
        _step(sm, model, rank, world, tag, bad=b)
    plain_ops = GuardOps()
    pmodel, plain = _sharded(plain_ops, **kw)
    for tag in (1, 3):
        _step(plain, pmodel, rank, world, tag)
    assert not getattr(plain_ops, "guard_calls", []) and plain._skip is None
    assert _same(_state(sm), _state(plain)), "the run did not continue as if the bad batch had never been seen"
    assert all(G16._bits(p, q) for p, q in zip(model.parameters(), pmodel.parameters()))
    assert (sm.step_count, sm.ema_updates, sm.skipped_steps) == (2, 1, 1) and (plain.step_count, plain.ema_updates, plain.skipped_steps) == (2, 1, 0)
    # every range went through the guarded launch; the step after the skipped one reused its number (bias correction, Philox step)
    assert [(c[2], c[4]) for c in ops.guard_calls] == [(1, 0)] * per_step + [(2, 1)] * per_step + [(2, 0)] * per_step
    assert [c[3] for c in ops.guard_calls] == [False] * per_step + [True] * (2 * per_step)
    if moments == "bf16":
        assert len(ops.m16_calls) == 2 * per_step          # the skipped step never reached the bf16-moment step
        assert all(u.exp_avg.dtype == torch.bfloat16 for u in sm.units if u.trainable)
    # ---- guard on, finite gradients only == guard off, 3 steps
    model, sm = _sharded(GuardOps(), skip_nonfinite=True, **kw)
    pmodel, plain = _sharded(GuardOps(), **kw)
    for tag in (1, 2, 3):
        _step(sm, model, rank, world, tag)
        _step(plain, pmodel, rank, world, tag)
        assert G16._bits(sm._norm, plain._norm) and G16._bits(sm._coef, plain._coef)
    assert _same(_state(sm), _state(plain))
    assert (sm.step_count, sm.ema_updates, sm.skipped_steps) == (3, 1, 0)


@pytest.mark.parametrize("bad", [INF, NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("moments", ["fp32", "bf16"])
def test_world1_skipped_step_is_as_if_never_seen(moments, bad):
    _scenario(0, 1, moments, bad)


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for moments in ("fp32", "bf16"):
            for bad in (INF, NAN):
                _scenario(rank, world, moments, bad)
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_world2_both_ranks_skip_when_rank1_holds_the_bad_value():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    assert dict(ret) == {0: "ok", 1: "ok"}


def test_too_many_consecutive_skips_raise():
    model, sm = _sharded(skip_nonfinite=True, max_consecutive_skips=2)
    _step(sm, model, 0, 1, 1, bad=NAN)
    with pytest.raises(RuntimeError, match=r"(?s)2 consecutive.*nan.*max_consecutive_skips=2"):
        for tag in (2, 3):
            _step(sm, model, 0, 1, tag, bad=NAN)
    assert sm.skipped_steps == 2 and sm.step_count == 0
    # a good step in between resets the count
    model, sm = _sharded(skip_nonfinite=True, max_consecutive_skips=2)
    for tag, b in ((1, INF), (2, None), (3, INF), (4, None)):
        _step(sm, model, 0, 1, tag, bad=b)
    assert (sm.skipped_steps, sm.step_count) == (2, 2)
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        _sharded(skip_nonfinite=True, max_consecutive_skips=0)


def test_ops_without_the_guard_methods_raise():
    with pytest.raises(TypeError, match="lacks clip_coef_guard, adamw_guard"):
        _sharded(G16.M16Ops(), skip_nonfinite=True)

    class Half(G16.M16Ops):
        clip_coef_guard = GC.GuardMethods.clip_coef_guard

    with pytest.raises(TypeError, match="lacks adamw_guard"):
        _sharded(Half(), skip_nonfinite=True)
    _, sm = _sharded(G16.M16Ops())                        # the same ops are fine without the guard, which then allocates nothing
    assert not sm.skip_nonfinite and sm._skip is None and sm._skip_host is None and sm.skipped_steps == 0


def test_optimizer_step_without_a_norm_raises():
    model, sm = _sharded(skip_nonfinite=True)
    before = _state(sm)
    with pytest.raises(RuntimeError, match="needs grad_norm_and_clip"):
        _step(sm, model, 0, 1, 1, clip=False)
    assert sm.step_count == 0 and _same(_state(sm), before)
    _step(sm, model, 0, 1, 1)
    with pytest.raises(RuntimeError, match="needs grad_norm_and_clip"):      # the norm of the step before does not count
        sm.optimizer_step(LR, betas=BETAS, eps=EPS, weight_decay=WD)
    assert sm.step_count == 1
    _, plain = _sharded()                                  # without the guard the call is what it always was
    plain.optimizer_step(LR, betas=BETAS, eps=EPS, weight_decay=WD)
    assert plain.step_count == 1


# ---------------------------------------------------------------------------------------------------------------- strategy, checkpoints
class GuardW8Ops(GC.GuardMethods, W8.GroupedOps):
    pass


def _strategy(net, **kw):
    return OS._strategy("w8", net, 8, local_ops=GuardW8Ops(), lr_scheduler_type="constant", warmup_ratio=0.0, **kw)


def _train(strat, tags):
    norms = []
    for tag in tags:
        x = OS._x(abs(tag), 0, 7)
        if tag < 0:                                         # a bad batch: one infinite input value
            x[0, 0] = INF
        strat.train_step(OS._batch(x))
        norms.append(float(strat.sharded._norm))
    return norms


def test_strategy_switch_and_environment(monkeypatch):
    from mla_amd.strategy import FSDPStrategy
    mk = lambda **kw: FSDPStrategy(OS.ToyVLA(W8._make(), (W8.Block, W8.Tower)), "cpu", global_batch_size=1, per_device_batch_size=1,
                                   local_ops=GuardW8Ops(), enable_gradient_checkpointing=False, **kw)
    monkeypatch.delenv("MLA_SKIP_NONFINITE", raising=False)
    assert mk().skip_nonfinite is False and mk(skip_nonfinite=True).skip_nonfinite is True
    monkeypatch.setenv("MLA_SKIP_NONFINITE", "0")
    assert mk().skip_nonfinite is False
    monkeypatch.setenv("MLA_SKIP_NONFINITE", "1")
    assert mk().skip_nonfinite is True and mk(skip_nonfinite=False).skip_nonfinite is False
    monkeypatch.delenv("MLA_SKIP_NONFINITE")
    s = mk()
    assert s.skipped_steps == 0                             # before run_setup
    s.skip_nonfinite, s.max_consecutive_skips = True, 3     # as attributes, the way a scripts/train.py caller sets them
    s.run_setup(100)
    assert s.sharded.skip_nonfinite and s.sharded.max_consecutive_skips == 3


def test_strategy_skips_a_bad_window_and_the_schedule_moves_on():
    """real autograd gradients; the bad window is the middle one, also as one bad micro-batch of a two-batch window"""
    on = _strategy(W8._make(), skip_nonfinite=True)
    norms = _train(on, (1, -2, 3))
    off = _strategy(W8._make())
    _train(off, (1, 3))
    assert norms[0] == norms[0] and abs(norms[0]) != INF and not (abs(norms[1]) < INF)        # the logged norm of the bad step is not finite
    assert (on.skipped_steps, on.sharded.step_count, on.step) == (1, 2, 3) and (off.skipped_steps, off.step) == (0, 2)
    a, b = OS._snapshot(on), OS._snapshot(off)
    a["step"] = b["step"]                                   # the schedule index advanced on the skipped window; everything else is equal
    OS._assert_same(a, b)
    acc = _strategy(W8._make(), skip_nonfinite=True, global_batch_size=2)
    before = OS._snapshot(acc)
    _train(acc, (1, -2))
    assert acc.skipped_steps == 1 and acc.step == 1
    after = OS._snapshot(acc)
    after["step"] = before["step"]
    OS._assert_same(after, before, "a bad micro-batch poisons its window")


def test_checkpoint_after_a_skipped_step_resumes_bit_exact(tmp_path):
    whole = _strategy(W8._make(), skip_nonfinite=True)
    _train(whole, (1, -2, 3, 4))
    first = _strategy(W8._make(), skip_nonfinite=True)
    _train(first, (1, -2))
    assert first.sharded._skip_pending is not None          # the host has not looked at the flag yet
    path = first.save_checkpoint(tmp_path, 2, 0, save_optimizer=True)
    assert first.sharded._skip_pending is None
    blob = torch.load(OS._opt_file(path), map_location="cpu", weights_only=True)
    assert (blob["step"], blob["step_count"], blob["skipped_steps"]) == (2, 1, 1)
    resumed = _strategy(OS._net_from_file("w8", path), skip_nonfinite=True)
    resumed.load_optimizer_and_scheduler(path)
    assert (resumed.step, resumed.sharded.step_count, resumed.skipped_steps) == (2, 1, 1)
    _train(resumed, (3, 4))
    OS._assert_same(OS._snapshot(whole), OS._snapshot(resumed))
    assert whole.skipped_steps == resumed.skipped_steps == 1
    # guard off: the file has no new key, and a guarded run loads it with a count of 0
    off = _strategy(W8._make())
    _train(off, (1, 3))
    p_off = off.save_checkpoint(tmp_path / "off", 2, 0, save_optimizer=True)
    blob_off = torch.load(OS._opt_file(p_off), map_location="cpu", weights_only=True)
    assert "skipped_steps" not in blob_off and set(blob) - set(blob_off) == {"skipped_steps"}
    late = _strategy(OS._net_from_file("w8", p_off), skip_nonfinite=True)
    late.load_optimizer_and_scheduler(p_off)
    assert late.skipped_steps == 0 and late.sharded.step_count == 2


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_guard_signatures_as_derived():
    from ctypes import c_float, c_int, c_longlong, c_ulonglong, c_void_p
    from mla_amd import hip
    P, F, LL, I = c_void_p, c_float, c_longlong, c_int
    assert hip._OPTIM_RESTYPES["mla_clip_coef_guard"] is c_int and hip._OPTIM_RESTYPES["mla_adamw_guard_step"] is c_int
    assert hip._OPTIM_SIGNATURES["mla_clip_coef_guard"] == [P, F, P, P, P, P]
    assert hip._OPTIM_SIGNATURES["mla_adamw_guard_step"] == [P, P, P, P, P, P, LL, LL, F, F, F, F, F, I, P, F, F, I, c_ulonglong, LL, P, P]
    assert "mla_clip_coef_guard" not in hip._SIGNATURES and "mla_adamw_guard_step" not in hip._SIGNATURES


def test_guard_argument_validation_on_the_host():
    """Argument validation happens before any launch -> safe without a GPU."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from mla_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p(256)
    hy = (2e-5, 0.9, 0.999, 1e-8, 0.01)
    for kw in (dict(sumsq=None), dict(coef=None), dict(skip=None)):
        a = dict(dict(sumsq=P, coef=P, skip=P), **kw)
        assert L.mla_clip_coef_guard(a["sumsq"], 1.0, a["coef"], None, a["skip"], None) == -1, kw
        assert b"mla_clip_coef_guard" in L.mla_last_error()

    def call(p=P, g=P, m=P, v=P, ema=None, n=64, n_decay=64, step=1, d=0.0, omd=0.0, m16=0, base=0, skip=P):
        return L.mla_adamw_guard_step(p, g, m, v, ema, None, n, n_decay, *hy, step, None, d, omd, m16, 7, base, skip, None)

    for m16 in (0, 1):
        for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=-1, n_decay=0), dict(step=0), dict(n_decay=-1),
                   dict(n_decay=65), dict(base=-1), dict(skip=None), dict(ema=P, d=1.5, omd=0.0), dict(ema=P, d=0.5, omd=-0.5),
                   dict(ema=P, d=float("nan"), omd=0.5), dict(ema=P, d=0.5, omd=float("nan"))):
            assert call(m16=m16, **kw) == -1, (m16, kw)
            assert b"mla_adamw_guard_step" in L.mla_last_error()
        assert call(m16=m16, n=0, n_decay=0) == 0            # a valid no-op
    for m16 in (2, -1):
        assert call(m16=m16) == -1 and b"moments_bf16" in L.mla_last_error()
