"""CPU, world_size = 2 over gloo: the sharding / collective / optimizer logic of mla_amd.fsdp.ShardedModel.

The local arithmetic is injected (TorchLocalOps below -- test infrastructure; the product always uses HipLocalOps), the
toy model is plain torch so its gradients are copied into the main_grad views the HIP wgrad epilogues would have written.
Checked against a single-process AdamW on the rank-averaged gradients: identical bf16 compute weights on every rank,
identical fp32 master weights after gathering the shards, global grad-norm clip, decay / no-decay split."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn


class TorchLocalOps:
    def cast_to_bf16(self, src32, dst16):
        dst16.copy_(src32.to(torch.bfloat16))

    def adamw(self, p32, g32, m, v, p16, lr, betas, eps, wd, step, grad_scale):
        g = g32 * (grad_scale if grad_scale is not None else 1.0)
        p32.mul_(1 - lr * wd)
        m.mul_(betas[0]).add_(g, alpha=1 - betas[0])
        v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
        bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
        p32.addcdiv_(m, (v.sqrt() / (bc2 ** 0.5)).add_(eps), value=-lr / bc1)
        p16.copy_(p32.to(torch.bfloat16))

    def sumsq(self, x32, out1, accumulate):
        s = (x32.double() ** 2).sum().float()
        out1.copy_(out1 + s if accumulate else s.reshape(1))

    def clip_coef(self, sumsq1, max_norm, coef1, norm1):
        n = sumsq1.sqrt()
        coef1.copy_(torch.clamp(max_norm / (n + 1e-6), max=1.0))
        norm1.copy_(n)

    def stream(self, device):
        return None


class Block(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.self_attn = nn.Identity()          # marks the block as a "decoder layer" unit for the ordering logic
        self.a = nn.Linear(d, d, bias=False)
        self.b = nn.Linear(d, d, bias=True)
        self.norm = nn.LayerNorm(d)
        self._grad_hook = None

    def forward(self, x):
        return x + self.b(torch.tanh(self.a(self.norm(x))))


class Toy(nn.Module):
    def __init__(self, d=24, n=3):
        super().__init__()
        self.inp = nn.Linear(10, d)
        self.frozen = nn.Linear(d, d)
        self.layers = nn.ModuleList([Block(d) for _ in range(n)])
        self.out = nn.Linear(d, 5)

    def forward(self, x):
        x = self.frozen(self.inp(x))
        for l in self.layers:
            x = l(x)
        return self.out(x)


def _make(seed=0):
    torch.manual_seed(seed)
    m = Toy()
    m.frozen.requires_grad_(False)
    return m


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mla_amd.fsdp import ShardedModel
        model = _make()
        ref = _make()                                            # fp32 single-process reference (same init)
        sm = ShardedModel(model, lambda mod: isinstance(mod, Block), torch.device("cpu"), ops=TorchLocalOps())
        assert [u.name for u in sm.units][0] == "<root>" and len(sm.units) == 4
        decay = [p for n, p in ref.named_parameters() if p.requires_grad and not (p.ndim <= 1 or n.endswith(".bias"))]
        nodecay = [p for n, p in ref.named_parameters() if p.requires_grad and (p.ndim <= 1 or n.endswith(".bias"))]
        opt = torch.optim.AdamW([{"params": decay, "weight_decay": 0.1}, {"params": nodecay, "weight_decay": 0.0}], lr=1e-2)
        # the bf16 compute weights start as bf16(init); make the reference start from the same rounded values? no: masters
        # are fp32(init) on both sides, the compute copy is only used for forward/backward
        for step in range(3):
            sm.begin_step()
            xs = [torch.randn(6, 10, generator=torch.Generator().manual_seed(100 * step + r)) for r in range(world)]
            # --- sharded side: this rank's micro-batch through the bf16 compute weights
            out = model(xs[rank].to(torch.bfloat16))
            out.float().pow(2).mean().backward()
            for p in model.parameters():
                if p.requires_grad:
                    p.main_grad.copy_(p.grad.float())
                    p._mg_touched = True
                    p.grad = None
            sm.finish_backward()
            norm = sm.grad_norm_and_clip(0.5)
            sm.optimizer_step(1e-2, weight_decay=0.1)
            # --- reference: same bf16 compute (weights rounded to bf16), gradients averaged over ranks, fp32 AdamW
            grads = None
            for r in range(world):
                shadow = _make()
                shadow.load_state_dict(ref.state_dict())
                shadow.frozen.requires_grad_(False)
                shadow.to(torch.bfloat16)
                shadow(xs[r].to(torch.bfloat16)).float().pow(2).mean().backward()
                g = [p.grad.float() if p.grad is not None else None for p in shadow.parameters()]
                grads = g if grads is None else [a + b if a is not None else None for a, b in zip(grads, g)]
            for p, g in zip(ref.parameters(), grads):
                p.grad = None if g is None else g / world
            total = torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.grad is not None], 0.5)
            opt.step()
            assert abs(float(norm) - float(total)) < 1e-4 * max(1.0, float(total)), (float(norm), float(total))
            full = sm.full_state_dict_fp32()
            for n, p in ref.named_parameters():
                assert torch.allclose(full[n], p.detach(), rtol=2e-5, atol=2e-6), (step, n)
                mine = dict(model.named_parameters())[n]
                assert mine.dtype == torch.bfloat16 and torch.equal(mine.detach(), full[n].to(torch.bfloat16)), (step, n)
        # shards partition the flat buffers and only the trainable region carries optimizer state
        for u in sm.units:
            assert u.n_total % (8 * world) == 0 and u.master_train.numel() * world == u.n_train
            assert u.exp_avg.numel() == u.shard_train
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_sharded_model_world2_gloo():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    assert dict(ret) == {0: "ok", 1: "ok"}


def test_sharded_model_world1_matches_adamw():
    from mla_amd.fsdp import ShardedModel
    model, ref = _make(), _make()
    sm = ShardedModel(model, lambda mod: isinstance(mod, Block), torch.device("cpu"), ops=TorchLocalOps())
    opt = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.0)
    x = torch.randn(4, 10)
    for _ in range(2):
        sm.begin_step()
        model(x.to(torch.bfloat16)).float().pow(2).mean().backward()
        shadow = _make()
        shadow.load_state_dict(ref.state_dict())
        shadow.frozen.requires_grad_(False)
        shadow.to(torch.bfloat16)
        shadow(x.to(torch.bfloat16)).float().pow(2).mean().backward()
        for p, q, s in zip(model.parameters(), ref.parameters(), shadow.parameters()):
            if p.requires_grad:
                p.main_grad.copy_(p.grad.float())
                p._mg_touched = True
                p.grad = None
                q.grad = s.grad.float()
        sm.finish_backward()
        sm.grad_norm_and_clip(None)
        sm.optimizer_step(1e-2)
        opt.step()
    full = sm.full_state_dict_fp32()
    for n, p in ref.named_parameters():
        assert torch.allclose(full[n], p.detach(), rtol=2e-5, atol=2e-6), n
    # a parameter that stops receiving gradients is presented with ZERO gradient (not a stale one)
    sm.begin_step()
    sm.finish_backward()
    assert all(float(p.main_grad.abs().max()) == 0.0 for p in model.parameters() if p.requires_grad)


def test_bench_dump_outputs_writes_the_last_step(tmp_path):
    """bench.py --dump-outputs: the loss dict, the grad norm and seeded samples of the gradient / updated fp32 weights, as float64 /
    float32 .npy files; the positions depend only on the layout, so two dumps of the same state are identical."""
    import bench
    from mla_amd.fsdp import ShardedModel
    model = _make()
    sm = ShardedModel(model, lambda mod: isinstance(mod, Block), torch.device("cpu"), ops=TorchLocalOps())
    sm.begin_step()
    loss = model(torch.randn(4, 10).to(torch.bfloat16)).float().pow(2).mean()
    loss.backward()
    for p in model.parameters():
        if p.requires_grad:
            p.main_grad.copy_(p.grad.float())
            p._mg_touched = True
            p.grad = None
    sm.finish_backward()
    sm.grad_norm_and_clip(1.0)
    sm.optimizer_step(1e-2)
    strat = type("Strat", (), {"sharded": sm})()
    losses = {"total_loss": loss.detach(), "unused": None}
    units = [u for u in sm.units if u.trainable]
    bench.dump_outputs(str(tmp_path / "a"), strat, losses)
    for d in "bc":
        bench.dump_outputs(str(tmp_path / d), strat, losses, max_bytes=(1 << 20) + 2 * 4 * 4 * len(units))
    a = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert set(a) == {"loss_total_loss.npy", "grad_norm.npy", "grad_sample.npy", "param_sample.npy"}
    assert a["loss_total_loss.npy"].dtype == np.float64 and float(a["loss_total_loss.npy"]) == float(loss)
    assert a["grad_norm.npy"].dtype == np.float64 and float(a["grad_norm.npy"]) == float(sm._norm)
    assert a["grad_sample.npy"].dtype == a["param_sample.npy"].dtype == np.float32
    assert a["grad_sample.npy"].size == sum(u.master_train.numel() for u in units)      # small units: every element
    assert np.array_equal(a["param_sample.npy"], torch.cat([u.master_train for u in units]).numpy())
    assert np.array_equal(a["grad_sample.npy"], torch.cat([u.gshard for u in units]).numpy())
    b = {f.name: np.load(f) for f in (tmp_path / "b").iterdir()}
    assert b["grad_sample.npy"].size == 4 * len(units)                                 # the byte budget caps the sample
    assert np.array_equal(b["loss_total_loss.npy"], a["loss_total_loss.npy"])
    assert all(np.array_equal(np.load(tmp_path / "c" / f), b[f]) for f in b)             # seeded positions: same sample again


def test_hook_launched_reduce_scatter_zeroes_stale_gradients_and_locks_the_unit():
    """(advisor, round 4) A decoder-layer unit whose reduce-scatter is launched from its backward hook: a parameter that got no gradient
    in this window but holds one from an earlier step is ZEROED in front of the collective (torch FSDP with use_orig_params presents
    zero gradients for unused parameters; the old code raised), and from the launch on any further main_grad write of the unit raises
    (the same layer run through backward twice in one step would otherwise land on top of the reduced shard)."""
    from mla_amd import ops
    from mla_amd.fsdp import ShardedModel
    model = _make()
    sm = ShardedModel(model, lambda mod: isinstance(mod, Block), torch.device("cpu"), ops=TorchLocalOps())
    u = next(u for u in sm.units if isinstance(getattr(u, "module", None), Block))
    params = [p for _, p, _ in u.params if p.requires_grad]
    sm.begin_step()
    for p in params:                                  # step 1: every parameter of the unit receives a gradient
        p.main_grad.fill_(1.0)
        ops._mark_touched(p)
    sm.finish_backward()
    assert all(p._mg_dirty for p in params)
    sm.begin_step()                                   # step 2: only the first one does
    params[0].main_grad.fill_(2.0)
    ops._mark_touched(params[0])
    u.zero_stale_and_lock()                           # what _launch_reduce_scatter does in front of the collective
    assert float(params[0].main_grad.min()) == 2.0
    assert all(float(p.main_grad.abs().max()) == 0.0 and not p._mg_dirty for p in params[1:])
    with pytest.raises(RuntimeError, match="reduce-scatter was launched"):
        ops._mark_touched(params[1])
    # (advisor, round 5) the writers check BEFORE enqueueing anything into the locked buffer: the wgrad entry points raise without
    # having launched a GEMM -- with CPU tensors a launch would have raised a different error (no CPU path) first
    w2 = next(p for p in params if p.dim() == 2)
    before = w2.main_grad.clone()
    dy, x = torch.zeros(4, w2.shape[0], dtype=torch.bfloat16), torch.zeros(4, w2.shape[1], dtype=torch.bfloat16)
    for fn, args in ((ops.deliver_wgrad, ((w2,), dy, x, (True,))), (ops.deliver_wgrad_nt, ((w2,), dy.t().contiguous(), x.t().contiguous(), (True,))),
                     (ops._gemm_into_main_grad, ((w2,), dy.t().contiguous(), x.t().contiguous(), w2.main_grad, False))):
        with pytest.raises(RuntimeError, match="reduce-scatter was launched"):
            fn(*args)
    assert torch.equal(w2.main_grad, before)
    u.finish_backward(already_reduced=True)           # bookkeeping only; no stale-gradient error any more
    sm.begin_step()
    ops._mark_touched(params[1])                      # a new step unlocks the unit
