"""RCCL-over-xGMI replacement for torch FSDP on the MLA training path.

Reference: training/strategies/fsdp.py:176-306 wraps the model in torch FSDP (HYBRID/FULL shard, MixedPrecision(param
bf16, reduce fp32), use_orig_params, one unit per LlamaDecoderLayer + tokenizers + projectors, model_mla.py:279-303).

MI355X-first redesign (DESIGN.md "sharding"):
* every unit owns ONE flat bf16 compute buffer (all ranks hold the full copy while computing -- 13.5 GB of 288 GB), one
  flat fp32 gradient buffer that the wgrad GEMM epilogues write into directly (``param.main_grad`` views; no zero-fill,
  no bf16->fp32 grad cast pass) and a 1/world shard of fp32 master weights + AdamW moments;
* per step and unit there is ONE bf16 all-gather (after the optimizer step, prefetched in forward order on a side stream
  and awaited right before the unit's first use) instead of FSDP's two (forward + pre-backward), and ONE fp32
  reduce-scatter (mean) launched on the side stream the moment the unit's backward kernels have been enqueued;
* q/k/v (and gate/up) weights are laid out back-to-back so the fused QKV / gate-up GEMMs read one contiguous operand;
* the fused AdamW kernel updates the fp32 shard and writes the refreshed bf16 shard in the same pass.

Local arithmetic (cast, AdamW, sum of squares) goes through an injected ``LocalOps``: the product uses HipLocalOps (HIP
kernels, no fallback); the CPU/gloo unit tests inject a torch implementation from tests/ to exercise the sharding logic.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn


class HipLocalOps:
    """Product implementation: every call is a libmla_hip.so kernel on the current stream."""

    def __init__(self):
        from . import hip
        self.hip = hip

    def cast_to_bf16(self, src32, dst16):
        self.hip.cast_f32_to_bf16(src32, dst16)

    def adamw(self, p32, g32, m, v, p16, lr, betas, eps, wd, step, grad_scale):
        self.hip.adamw_step(p32, g32, m, v, p16, lr, betas[0], betas[1], eps, wd, step, grad_scale)

    def adamw_groups(self, p32, g32, m, v, p16, n_decay, lr, betas, eps, wd, step, grad_scale):
        self.hip.adamw_step_groups(p32, g32, m, v, p16, n_decay, lr, betas[0], betas[1], eps, wd, step, grad_scale)

    # the two steps above with the weight average folded in (ema = (1 - ema_decay) * p_new + ema_decay * ema), and the average as a
    # pass of its own
    def adamw_ema(self, p32, g32, m, v, ema, p16, lr, betas, eps, wd, step, grad_scale, ema_decay):
        self.hip.adamw_ema_step(p32, g32, m, v, ema, p16, lr, betas[0], betas[1], eps, wd, step, grad_scale, ema_decay)

    def adamw_ema_groups(self, p32, g32, m, v, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay):
        self.hip.adamw_ema_step_groups(p32, g32, m, v, ema, p16, n_decay, lr, betas[0], betas[1], eps, wd, step, grad_scale, ema_decay)

    def ema_update(self, ema, p32, decay):
        self.hip.ema_update(ema, p32, decay)

    # adamw_groups / adamw_ema_groups (ema not None) with the moments stored as bf16 and rounded stochastically (ShardedModel
    # moments="bf16"): the random bits of element i are a function of (seed, step, index_base + i)
    def adamw_m16(self, p32, g32, m16, v16, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay, seed, index_base):
        self.hip.adamw_m16_step(p32, g32, m16, v16, ema, p16, n_decay, lr, betas[0], betas[1], eps, wd, step, grad_scale, ema_decay, seed,
                                index_base)

    # skip_nonfinite (ShardedModel): clip_coef that also writes the one-int device flag skip1 (1 = the norm is not finite), and every
    # form of the AdamW launch above behind that flag -- m, v fp32 (seed / index_base unused) or bf16, ema or None -- which touches
    # nothing when the flag is set and writes the bits of the unguarded launch when it is not
    def clip_coef_guard(self, sumsq1, max_norm, coef1, norm1, skip1):
        self.hip.clip_coef_guard(sumsq1, max_norm, coef1, norm1, skip1)

    def adamw_guard(self, p32, g32, m, v, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay, seed, index_base, skip1):
        self.hip.adamw_guard_step(p32, g32, m, v, ema, p16, n_decay, lr, betas[0], betas[1], eps, wd, step, grad_scale, ema_decay, seed,
                                  index_base, skip1)

    def sumsq(self, x32, out1, accumulate):
        self.hip.sumsq(x32, out1, accumulate)

    def sum_partials(self, partials, n, out1, accumulate):
        self.hip.sum_partials(partials, n, out1, accumulate)

    def clip_coef(self, sumsq1, max_norm, coef1, norm1):
        self.hip.clip_coef(sumsq1, max_norm, coef1, norm1)

    def stream(self, device):
        return torch.cuda.Stream(device=device)


class _SqArena:
    """Bump allocator over one fp32 buffer: every wgrad launch of a step takes the slice its sum-of-squares partials go to; the
    gradient norm then sums the used prefix in one launch. Reset at the start of every step."""

    def __init__(self, n: int, device):
        self.buf = torch.zeros(n, dtype=torch.float32, device=device)
        self.used = 0

    def take(self, count: int):
        if self.used + count > self.buf.numel():
            return None
        part = self.buf[self.used:self.used + count]
        self.used += count
        return part


def _round_up(n, m):
    return ((n + m - 1) // m) * m


def apply_rccl_env(environ=None) -> Dict[str, str]:
    """Knobs for the collectives' footprint on the chip, to be applied BEFORE the process group is created (bench.py does; a training
    script would call it next to its init_process_group). RCCL's kernels run on the side stream underneath the backward GEMMs, which
    launch one 512-thread workgroup per CU: every CU a channel occupies is a CU the GEMM rounds do not get.
      MLA_RCCL_MAX_CHANNELS=n  -> NCCL_MAX_NCHANNELS=n (RCCL honours the NCCL_* names): caps the workgroups per collective kernel;
      MLA_GEMM_CUS=n           -> read by libmla_hip.so itself: the GEMMs plan their split-K tails for n CUs instead of all of them.
    Returns what was set (for the bench line)."""
    import os as _os
    env = _os.environ if environ is None else environ
    done = {}
    v = env.get("MLA_RCCL_MAX_CHANNELS")
    if v:
        env["NCCL_MAX_NCHANNELS"] = str(int(v))
        done["NCCL_MAX_NCHANNELS"] = env["NCCL_MAX_NCHANNELS"]
    for k in ("MLA_GEMM_CUS", "MLA_FSDP_INPLACE_RS", "NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS"):
        if env.get(k) is not None:
            done[k] = env[k]
    return done


def default_no_decay(n: str, p) -> bool:
    """The reference's two AdamW parameter groups (training/strategies/fsdp.py:236-256): vectors and biases are not decayed."""
    return p.ndim <= 1 or n.endswith(".bias")


def plan_flat_layout(named_params: Sequence[Tuple[str, nn.Parameter]], world: int, no_decay: Callable = default_no_decay):
    """Where every parameter of ONE sharding unit sits in the unit's flat buffers -- pure arithmetic on shapes and requires_grad (works
    on meta-device modules): returns ``(params, n_decay, n_train, n_total)`` with ``params = [(name, parameter, element offset)]``.
    Order: [trainable & decayed | trainable & not decayed | frozen], each in module order (keeps q|k|v and gate|up adjacent); every
    tensor starts on an 8-element boundary (16 B in bf16, 32 B in fp32) and every region ends on a multiple of 8 x world, so that a
    1/world shard of the trainable or of the frozen region starts 16-B aligned in bf16 on every rank."""
    decay = [(n, p) for n, p in named_params if p.requires_grad and not no_decay(n, p)]
    nodecay = [(n, p) for n, p in named_params if p.requires_grad and no_decay(n, p)]
    frozen = [(n, p) for n, p in named_params if not p.requires_grad]
    align = 8 * world
    params: List[Tuple[str, nn.Parameter, int]] = []
    off = 0
    bounds = []
    for group in (decay, nodecay, frozen):
        for n, p in group:
            params.append((n, p, off))
            off += _round_up(p.numel(), 8)
        off = _round_up(off, align)
        bounds.append(off)
    return params, bounds[0], bounds[1], bounds[2]


def discover_units(model: nn.Module, unit_policy: Callable[[nn.Module], bool]):
    """The sharding units of a model in the order ShardedModel creates them: ``[(unit name, module or None, [(param name, param)])]``.
    Outermost matches of the policy are units; what no unit claims folds into the root unit; forward order = non-decoder units, root
    (the embeddings are needed first), decoder layers."""
    unit_mods: List[Tuple[str, nn.Module]] = []

    def walk(prefix, mod):
        for cn, child in mod.named_children():
            full = f"{prefix}.{cn}" if prefix else cn
            if unit_policy(child):
                unit_mods.append((full, child))
            else:
                walk(full, child)
    walk("", model)
    claimed = set()
    pending = []
    for name, mod in unit_mods:
        named = [(f"{name}.{n}", p) for n, p in mod.named_parameters() if id(p) not in claimed]
        claimed.update(id(p) for _, p in named)
        pending.append((name, mod, named))
    root_named = [(n, p) for n, p in model.named_parameters() if id(p) not in claimed]
    early = [x for x in pending if not hasattr(x[1], "self_attn")]
    layers = [x for x in pending if hasattr(x[1], "self_attn")]
    out = list(early)
    if root_named:
        out.append(("<root>", None, root_named))
    out.extend(layers)
    return [x for x in out if x[2]]


MOMENT_FORMATS = {"fp32": torch.float32, "bf16": torch.bfloat16}      # ShardedModel(moments=...): storage of exp_avg / exp_avg_sq


def plan_sharded_layout(model: nn.Module, unit_policy: Callable[[nn.Module], bool], world: int, no_decay: Callable = default_no_decay,
                        inplace_reduce: bool = True, moments: str = "fp32"):
    """Per-unit layout and per-rank memory of ``ShardedModel(model, unit_policy)`` at ``world`` ranks WITHOUT allocating anything (the
    model may live on the meta device): the audit the 8-GPU run is planned with. Bytes per rank and unit:
    bf16 replica (whole unit: the all-gathered weights stay resident), fp32 gradient buffer (whole trainable region: the in-place
    reduce-scatter leaves the rank's shard inside it), fp32 master + two AdamW moments (1/world of the trainable region), fp32
    master of the frozen region (1/world). ``inplace_reduce=False`` adds the separate fp32 gradient shard of the gloo / out-of-place path.
    ``moments="bf16"`` halves the two moments (ShardedModel's keyword)."""
    moment_bytes = 2 * MOMENT_FORMATS[moments].itemsize
    units = []
    for name, mod, named in discover_units(model, unit_policy):
        params, n_decay, n_train, n_total = plan_flat_layout(named, world, no_decay)
        shard_train, shard_frozen = n_train // world, (n_total - n_train) // world
        ranges = []
        for rank in range(world):
            lo, hi = rank * shard_train, (rank + 1) * shard_train
            ranges.append([(max(a, lo) - lo, min(b, hi) - lo, max(a, lo), dec) for a, b, dec in ((0, n_decay, True), (n_decay, n_train, False))
                           if min(b, hi) > max(a, lo)])
        units.append(dict(name=name, is_layer=mod is not None and hasattr(mod, "self_attn"), params=params, n_decay=n_decay, n_train=n_train,
                          n_total=n_total, shard_train=shard_train, shard_frozen=shard_frozen, shard_ranges=ranges,
                          bytes_bf16_replica=2 * n_total, bytes_grad32=4 * n_train,
                          bytes_master=4 * (shard_train + shard_frozen), bytes_moments=moment_bytes * shard_train,
                          bytes_grad_shard=0 if (inplace_reduce or world == 1) else 4 * shard_train))
    return units


class _Arenas:
    """One allocation per KIND of buffer for all units of a model (bf16 replicas, fp32 gradient buffers, masters, the two AdamW moments,
    separate gradient shards): a unit's buffers are consecutive slices of them. Measured on MI355X (tools/exp_adamw_placement.py): the
    fused AdamW streams five buffers of a unit at once, and with the units' buffers allocated one by one in unit order (the five of a
    unit adjacent in the address space) it runs at 5.5 TB/s; with one arena per kind (the five streams of a unit several GB apart, as
    in the kernel's stand-alone benchmark) at 6.0 TB/s -- the in-step optimizer was the slow case in rounds 1-3."""

    ALIGN_BYTES = 2 << 20      # every slice starts on a 2 MiB boundary, like a separate allocation would: a weight matrix whose rows do
    #                            not start on 128-B lines costs the GEMMs' 1-KiB LDS-DMA reads an extra line each (measured: -3 % on the step)

    def __init__(self, sizes: Dict[str, int], device, slices: int = 0, dtypes: Optional[Dict[str, torch.dtype]] = None):
        """sizes in elements; dtypes: kinds that are not fp32 (the bf16 replica always is bf16; bf16 moments name theirs)."""
        dt = dict({"flat16": torch.bfloat16}, **(dtypes or {}))
        pad = {k: slices * (self.ALIGN_BYTES // dt.get(k, torch.float32).itemsize) for k in sizes}
        self.buf = {k: torch.zeros(max(n + pad[k], 1), dtype=dt.get(k, torch.float32), device=device) for k, n in sizes.items() if n > 0}
        self.used = {k: 0 for k in self.buf}
        self.dtype = {k: b.dtype for k, b in self.buf.items()}

    def has(self, kind: str) -> bool:
        return kind in self.buf

    def take(self, kind: str, n: int):
        if n == 0:
            return torch.zeros(0, dtype=self.dtype[kind], device=next(iter(self.buf.values())).device)
        gran = self.ALIGN_BYTES // self.buf[kind].element_size()
        o = (self.used[kind] + gran - 1) // gran * gran
        assert o + n <= self.buf[kind].numel(), f"arena {kind}: {o} + {n} > {self.buf[kind].numel()}"
        self.used[kind] = o + n
        return self.buf[kind][o:o + n]


class FlatUnit:
    """One sharding unit. Parameter order inside the flat buffers: [trainable & decayed | trainable & not decayed |
    frozen], each in module order (keeps q|k|v and gate|up adjacent), every tensor padded to 8 elements (plan_flat_layout)."""

    def __init__(self, name: str, named_params: Sequence[Tuple[str, nn.Parameter]], device, world: int, rank: int, ops,
                 no_decay: Callable[[str, nn.Parameter], bool], process_group=None, sync_from_rank0: bool = True,
                 collectives: Optional[bool] = None, inplace_reduce: bool = False, arenas: Optional["_Arenas"] = None,
                 with_ema: bool = False, moment_dtype: torch.dtype = torch.float32):
        self.name, self.world, self.rank, self.ops, self.device = name, world, rank, ops, device
        # buffers come from per-kind arenas when the owner provides them (ShardedModel), else from torch one by one
        def take(kind, n, dtype):
            if arenas is not None and arenas.has(kind):
                return arenas.take(kind, n)
            return torch.zeros(n, dtype=dtype, device=device)
        coll = (world > 1) if collectives is None else collectives   # separate shard buffers + real collectives
        self.params, self.n_decay, self.n_train, self.n_total = plan_flat_layout(named_params, world, no_decay)
        self.shard_total = self.n_total // world
        self.shard_train = self.n_train // world
        self.trainable = self.n_train > 0

        # ---- buffers
        full32 = torch.zeros(self.n_total, dtype=torch.float32, device=device)
        for n, p, o in self.params:
            full32[o:o + p.numel()].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
        if coll and sync_from_rank0:
            dist.broadcast(full32, src=0, group=process_group)      # every rank starts from rank 0's weights (FSDP sync_module_states)
        self.flat16 = take("flat16", self.n_total, torch.bfloat16)
        ops.cast_to_bf16(full32, self.flat16)
        # fp32 master weights: the trainable region and the frozen region are each sharded 1/world, so that the weights,
        # gradient shard and AdamW moments of one element always live on the same rank
        nf = (self.n_total - self.n_train) // world
        if not coll and not (arenas is not None and arenas.has("master")):
            self.master_train, self.master_frozen = full32[:self.n_train], full32[self.n_train:]
        else:
            r = rank if coll else 0
            st, sf = (self.shard_train, nf) if coll else (self.n_train, self.n_total - self.n_train)
            self.master_train = take("master", st, torch.float32)
            self.master_frozen = take("master", sf, torch.float32)
            self.master_train.copy_(full32[r * st:(r + 1) * st])
            self.master_frozen.copy_(full32[self.n_train + r * sf:self.n_train + (r + 1) * sf])
        del full32
        self.grad32 = take("grad32", self.n_train, torch.float32) if self.trainable else None
        # inplace_reduce (RCCL): the reduce-scatter writes this rank's shard INTO its own slice of the gradient buffer (NCCL's in-place
        # form, recvbuff == sendbuff + rank * count) as a SUM; the 1 / world of the mean is folded into the norm and into AdamW's
        # gradient scale (ShardedModel.grad_div). No separate shard buffer (27 GB / world at 7B), no copy when world == 1.
        self.inplace_reduce = bool(coll and inplace_reduce)
        if self.trainable:
            if not coll:
                self.gshard = self.grad32
            elif self.inplace_reduce:
                self.gshard = self.grad32[rank * self.shard_train:(rank + 1) * self.shard_train]
            else:
                self.gshard = take("gshard", self.shard_train, torch.float32)
            self.exp_avg = take("exp_avg", self.shard_train, moment_dtype)       # fp32, or bf16 (ShardedModel moments="bf16")
            self.exp_avg_sq = take("exp_avg_sq", self.shard_train, moment_dtype)
            assert self.exp_avg.dtype == moment_dtype and self.exp_avg_sq.dtype == moment_dtype
            if with_ema:
                # weight average of the trainable masters (ShardedModel ema_decay): starts as a copy of this rank's master shard,
                # padding 0 like the master's -- and (1 - d) * 0 + d * 0 keeps it 0. Units without it have no such attribute.
                self.ema = take("ema", self.shard_train, torch.float32)
                self.ema.copy_(self.master_train[:self.shard_train])
        # ---- re-point the module parameters at the bf16 compute storage; install fp32 main_grad views
        # gradient-norm partials delivered by the wgrad GEMM epilogues (ops._gemm_into_main_grad): offset -> (numel, partials, count).
        # Only without collectives: under FSDP the norm is taken over the REDUCED shards, which no local epilogue has seen.
        self.sq_entries: Dict[int, Tuple[int, int, int]] = {}      # offset -> (numel, arena offset, partial count)
        self.sq_arena = None                                        # set by ShardedModel (one arena for all units)
        self._offset_of = {id(p): o for _, p, o in self.params}
        for n, p, o in self.params:
            p.data = self.flat16[o:o + p.numel()].view(p.shape)
            if p.requires_grad:
                p.main_grad = self.grad32[o:o + p.numel()].view(p.shape)
                p._mg_touched = False
                p._mg_dirty = False
                if not coll and hasattr(ops, "sum_partials"):
                    p._sq_sink = self._sq_sink
                    p._sq_invalidate = self._sq_invalidate_param
            p.grad = None
        self.gather_event = None
        self.rs_event = None

    def sq_invalidate(self, off: int, end: int) -> None:
        """main_grad[off:end) is about to be written by something that leaves no sum(dW^2) partials (a plain GEMM, an
        accumulate on an odd shape, an embedding / vector gradient): every recorded range that INTERSECTS it is stale -- dropped
        and its arena slice zeroed, so the norm pass reads those elements from the buffer again (uncovered_ranges)."""
        if not self.sq_entries:
            return
        for k in [k for k, e in self.sq_entries.items() if k < end and off < k + e[0]]:
            e = self.sq_entries.pop(k)
            self.sq_arena.buf[e[1]:e[1] + e[2]].zero_()

    def _sq_invalidate_param(self, p) -> None:
        off = self._offset_of.get(id(p))
        if off is not None:
            self.sq_invalidate(off, off + p.numel())

    def _sq_sink(self, weights, count):
        """A wgrad launch is about to write main_grad of `weights` (adjacent in the flat buffer) and to leave `count` sum(dW^2)
        partials of the final values: returns where they go (a slice of the model-wide arena, summed by ONE launch at clipping
        time) or None when the arena is full. A later launch that touches any part of the range (gradient accumulation, or a
        per-weight launch after a q|k|v-wide one) supersedes the earlier entries: their slices are zeroed."""
        arena = self.sq_arena
        if arena is None:
            return None
        off = self._offset_of[id(weights[0])]
        end = self._offset_of[id(weights[-1])] + weights[-1].numel()
        self.sq_invalidate(off, end)
        part = arena.take(count)
        if part is None:
            return None
        self.sq_entries[off] = (end - off, part.storage_offset(), count)
        return part

    def uncovered_ranges(self) -> List[Tuple[int, int]]:
        """[a, b) pieces of the trainable gradient buffer that no sq_entries range covers (norm weights, biases, embeddings, ...)."""
        out, pos = [], 0
        for off in sorted(self.sq_entries):
            n = self.sq_entries[off][0]
            assert off >= pos, "overlapping gradient-norm ranges"
            if off > pos:
                out.append((pos, off))
            pos = off + n
        if pos < self.n_train:
            out.append((pos, self.n_train))
        return out

    # shard-local [lo, hi) intersections with the decay / no-decay regions (optimizer launches)
    def _shard_ranges(self):
        lo = self.rank * self.shard_train
        hi = lo + self.shard_train
        out = []
        for a, b, decayed in ((0, self.n_decay, True), (self.n_decay, self.n_train, False)):
            s, e = max(a, lo), min(b, hi)
            if e > s:
                out.append((s - lo, e - lo, s, decayed))
        return out

    def begin_step(self):
        self.sq_entries = {}
        for _, p, _ in self.params:
            if p.requires_grad:
                p._mg_touched = False
                p._mg_locked = False
                if hasattr(p, "_mg_regions"):
                    p._mg_regions = {}       # per-region state of parameters used through ops.param_view

    def zero_stale_and_lock(self):
        """Called when the unit's reduce-scatter is about to be launched from its backward hook (see ShardedModel._launch_reduce_scatter)."""
        for _, p, _ in self.params:
            if not p.requires_grad:
                continue
            touched = p._mg_touched or any(getattr(p, "_mg_regions", {}).values())
            if not touched and p._mg_dirty and p.grad is None:
                p.main_grad.zero_()
                p._mg_dirty = False
            p._mg_locked = True

    def collect_autograd_grads(self):
        """Gradients delivered by autograd into ``.grad`` (small broadcast parameters: queries, mask token, position tables) move
        into main_grad; called after every backward so that accumulation over micro-batches happens in fp32."""
        for _, p, o in self.params:
            if p.requires_grad and p.grad is not None:
                self.sq_invalidate(o, o + p.numel())   # an autograd gradient lands on top of a wgrad epilogue's values
                if p._mg_touched:
                    p.main_grad.add_(p.grad.to(torch.float32))
                else:
                    p.main_grad.copy_(p.grad)
                p._mg_touched = True
                p.grad = None

    def finish_backward(self, already_reduced: bool = False):
        """Parameters that received no gradient this step but hold a stale one from an earlier step are zeroed
        (torch FSDP with use_orig_params presents zero gradients for them, and AdamW still applies to them).

        ``already_reduced``: the unit's reduce-scatter was launched from its backward hook (decoder layers). With the in-place
        collective the reduced SUM shard lives INSIDE grad32, so nothing may write main_grad any more -- a late autograd ``.grad``
        or a stale gradient that would need zeroing is an error here, not something to patch up on top of (or racing with) the
        collective's output (advisor, round 3). Only the dirty-flag bookkeeping runs."""
        if already_reduced:
            for n, p, _ in self.params:
                if not p.requires_grad:
                    continue
                if p.grad is not None:
                    raise RuntimeError(f"{self.name}: {n} received an autograd gradient after the unit's reduce-scatter was launched")
                if not p._mg_touched and any(getattr(p, "_mg_regions", {}).values()):
                    p._mg_touched = True
                if not p._mg_touched and p._mg_dirty:        # cannot happen since zero_stale_and_lock(): kept as an invariant check
                    raise RuntimeError(f"{self.name}: {n} holds a stale gradient that was reduced with this step's (untouched this step, "
                                       "but the unit's reduce-scatter fired from its backward hook)")
                if p._mg_touched:
                    p._mg_dirty = True
            return
        self.collect_autograd_grads()
        for _, p, _ in self.params:
            if p.requires_grad:
                if not p._mg_touched and any(getattr(p, "_mg_regions", {}).values()):
                    p._mg_touched = True     # written through its views (packed in_proj weights, conv weights used as matrices)
                if not p._mg_touched and p._mg_dirty:
                    p.main_grad.zero_()
                    p._mg_dirty = False
                elif p._mg_touched:
                    p._mg_dirty = True

    def state_bytes(self):
        n = self.flat16.numel() * 2 + (self.master_train.numel() + self.master_frozen.numel()) * 4
        if self.trainable:
            n += self.grad32.numel() * 4 + (self.exp_avg.numel() + self.exp_avg_sq.numel()) * self.exp_avg.element_size()
            if hasattr(self, "ema"):
                n += self.ema.numel() * 4
            if self.gshard is not self.grad32 and not self.inplace_reduce:
                n += self.gshard.numel() * 4
        return n


class ShardedModel:
    """Owns the FlatUnits of a model and runs the step-level collectives + optimizer."""

    def __init__(self, model: nn.Module, unit_policy: Callable[[nn.Module], bool], device, ops=None,
                 process_group=None, no_decay: Optional[Callable[[str, nn.Parameter], bool]] = None,
                 inplace_reduce: Optional[bool] = None, ema_decay: Optional[float] = None, ema_update_every: int = 1,
                 moments: str = "fp32", moments_seed: int = 0, skip_nonfinite: bool = False, max_consecutive_skips: int = 16):
        """skip_nonfinite (False: nothing changes): when the global gradient norm of a step is +inf or NaN, that optimizer step does
        nothing -- on every rank, for every unit -- and the run goes on as if the batch had never been seen. The verdict is a device
        flag written by the clip-coefficient launch (after the all-reduce of the sum of squares, so every rank sees the same one)
        and read by every AdamW launch: no host round trip. ``step_count`` and ``ema_updates`` count APPLIED steps; the host learns a
        step's flag one step late (an asynchronous copy to pinned memory, resolved before the next step's launches are formed and
        by every read of the counters or of ``skipped_steps``), so it never waits for work of the current step. After
        ``max_consecutive_skips`` skipped steps in a row the resolution raises: weights that are themselves non-finite must not skip
        for ever. Not covered: buffers updated in the forward (BatchNorm statistics) are not rolled back; a finite gradient whose
        sum of squares overflows fp32 counts as non-finite. No counterpart in the reference.
        moments ("fp32": nothing changes): "bf16" stores exp_avg / exp_avg_sq as bf16 -- half their memory, 22 instead of 30 B per
        element through the AdamW pass -- rounded STOCHASTICALLY inside the launch (round-to-nearest cannot hold exp_avg_sq:
        bf16(0.999 v) == v). The random bits of an element are a function of (moments_seed, step_count, unit ordinal, position in the
        unit's flat trainable region): same world size and same seed give bit-exact reruns and resumes; at another world size the
        moments load exactly and the run continues, but on other random bits (plan_flat_layout pads regions to 8 x world, so flat
        positions move). No counterpart in the reference (torch.optim.AdamW keeps fp32); the masters and the EMA stay fp32.
        ema_decay (None: off, nothing changes): keep an exponential moving average of every TRAINABLE fp32 master, sharded like
        the AdamW moments (FlatUnit.ema), advanced inside the AdamW launch of every ``ema_update_every``-th optimizer step
        (reference: update_ema, training/strategies/base_strategy_mla.py:33-41). Frozen parameters have none: theirs is their value."""
        self.model, self.device = model, device
        self.pg = process_group
        import os
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        # MLA_FORCE_COLLECTIVES=1 runs the sharded code path (separate shards, RCCL calls, side stream) even with one rank:
        # used to validate the collective plumbing on a single-GPU box
        self.coll = self.world > 1 or (os.environ.get("MLA_FORCE_COLLECTIVES") == "1" and dist.is_available() and dist.is_initialized())
        self.ops = ops if ops is not None else HipLocalOps()
        if moments not in MOMENT_FORMATS:
            raise ValueError(f"moments must be one of {sorted(MOMENT_FORMATS)}, got {moments!r}")
        if moments == "bf16" and not hasattr(self.ops, "adamw_m16"):      # never a run that quietly keeps fp32 moments
            raise TypeError(f"moments='bf16' but {type(self.ops).__name__} lacks adamw_m16")
        self.moments, self.moments_seed = moments, int(moments_seed)
        self.skip_nonfinite, self.max_consecutive_skips = bool(skip_nonfinite), int(max_consecutive_skips)
        if self.skip_nonfinite:
            lacking = [m for m in ("clip_coef_guard", "adamw_guard") if not hasattr(self.ops, m)]
            if lacking:      # never a run that is quietly unguarded
                raise TypeError(f"skip_nonfinite is set but {type(self.ops).__name__} lacks {', '.join(lacking)}")
            if self.max_consecutive_skips < 1:
                raise ValueError(f"max_consecutive_skips must be >= 1, got {max_consecutive_skips}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_update_every = int(ema_update_every)
        self._ema_updates = 0         # optimizer steps that advanced the average (property ema_updates)
        self._ema_swapped = False     # inside ema_weights()
        if self.ema_decay is not None:
            if not 0.0 <= self.ema_decay <= 1.0:
                raise ValueError(f"ema_decay must lie in [0, 1], got {ema_decay}")
            if self.ema_update_every < 1:
                raise ValueError(f"ema_update_every must be >= 1, got {ema_update_every}")
            lacking = [m for m in ("adamw_ema", "adamw_ema_groups", "ema_update") if not hasattr(self.ops, m)]
            if lacking:      # never a run that quietly keeps no average
                raise TypeError(f"ema_decay is set but {type(self.ops).__name__} lacks {', '.join(lacking)}")
        # RCCL: in-place SUM reduce-scatter, mean folded into the scales (see FlatUnit). gloo (CPU tests) keeps separate mean shards.
        # (inplace_reduce=True with gloo is for the CPU tests: it runs the same SUM-shard bookkeeping over an in-place all-reduce)
        # MLA_FSDP_INPLACE_RS=0: back to an out-of-place reduce-scatter into separate shard buffers (the round-2 layout; a SUM like the
        # in-place form since round 6) -- a pre-wired fallback for the first multi-GPU run, should RCCL's in-place form misbehave there
        if inplace_reduce is None and os.environ.get("MLA_FSDP_INPLACE_RS") == "0":
            inplace_reduce = False
        self.inplace_reduce = bool(self.coll and (dist.get_backend(process_group) == "nccl" if inplace_reduce is None else inplace_reduce))
        # RCCL reduce-scatters are always SUMs, in place or not (round 6): ncclAvg is not used at all. The world-1 RCCL test
        # (tests/test_fsdp_rccl_world1_gpu.py) caught this image's RCCL 2.26.6 dropping the last 8 elements of an out-of-place AVG
        # reduce-scatter of 2^20 + 8 floats (output left untouched there; SUM of the same buffer is exact --
        # profiles/r6_rccl_avg_tail.txt), which silently froze the last bias of the root unit under MLA_FSDP_INPLACE_RS=0.
        self.sum_shards = bool(self.inplace_reduce or (self.coll and dist.get_backend(process_group) == "nccl"))
        self.grad_div = float(self.world) if self.sum_shards else 1.0         # gshard holds grad_div x the mean gradient
        no_decay = no_decay or default_no_decay   # fsdp.py:236-256
        # ---- unit discovery (outermost matches of the policy; the remainder folds into the root unit); forward order: non-decoder
        # units and the root first (embeddings are needed first), decoder layers after -- discover_units()
        self.units: List[FlatUnit] = []
        self.unit_of_module: Dict[int, FlatUnit] = {}
        found = discover_units(model, unit_policy)
        # one arena per kind of buffer, sized from the layout plan (see _Arenas: +10 % AdamW bandwidth against per-unit allocations);
        # MLA_FSDP_ARENAS=0 = the per-unit allocations of rounds 1-3 (A/B switch)
        self._arenas = None
        kinds = [k for k in os.environ.get("MLA_FSDP_ARENAS", "master,exp_avg,exp_avg_sq").split(",") if k and k != "0"]
        if kinds:
            sizes = dict(flat16=0, grad32=0, master=0, exp_avg=0, exp_avg_sq=0, gshard=0)
            for name, mod, named in found:
                _, n_decay, n_train, n_total = plan_flat_layout(named, self.world, no_decay)
                w = self.world if self.coll else 1
                sizes["flat16"] += n_total
                sizes["grad32"] += n_train
                sizes["master"] += n_total // w
                sizes["exp_avg"] += n_train // self.world
                sizes["exp_avg_sq"] += n_train // self.world
                if self.coll and not self.inplace_reduce:
                    sizes["gshard"] += n_train // self.world
                if self.ema_decay is not None:
                    sizes["ema"] = sizes.get("ema", 0) + n_train // self.world
            if self.ema_decay is not None and "exp_avg" in kinds:
                kinds = kinds + ["ema"]      # an eighth stream of the AdamW pass: placed like the moments, and switched with them
            self._arenas = _Arenas({k: v for k, v in sizes.items() if k in kinds}, device, slices=2 * len(found),
                                   dtypes={k: MOMENT_FORMATS[self.moments] for k in ("exp_avg", "exp_avg_sq")})
        for name, mod, named in found:
            self._add_unit(name, mod, named, no_decay)
        # buffers (BatchNorm statistics, ...) just move to the device in fp32 (FSDP buffer_dtype fp32)
        for b in model.buffers():
            b.data = b.data.to(device)
        self._step_count = 0          # applied optimizer steps (property step_count)
        self.defer_reduce = False     # gradient accumulation: micro-batches before the last one only add into main_grad
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=device)
        # arena of the wgrad epilogues' sum-of-squares partials (FlatUnit._sq_sink): ~1.4 K floats per decoder-layer GEMM at 7B
        self._sq_arena = _SqArena(1 << 20, device) if (not self.coll and hasattr(self.ops, "sum_partials") and
                                                       self.device.type == "cuda") else None
        for u in self.units:
            u.sq_arena = self._sq_arena
        self._coef = torch.ones(1, dtype=torch.float32, device=device)
        self._norm = torch.zeros(1, dtype=torch.float32, device=device)
        self.on_gpu = self.device.type == "cuda"
        # ---- skip_nonfinite bookkeeping (all None / 0 and never touched with the guard off)
        self._skipped_steps = 0       # steps whose flag was set (property skipped_steps)
        self._consecutive_skips = 0
        self._norm_fresh = False      # grad_norm_and_clip ran since the last optimizer_step
        self._skip_pending = None     # (event or None, that step advanced the average) of the last step, until its flag is resolved
        self._skip_copied = None      # event behind the flag's copy to the host, between grad_norm_and_clip and optimizer_step
        self._skip = self._skip_host = None
        if self.skip_nonfinite:
            self._skip = torch.zeros(1, dtype=torch.int32, device=device)
            if self.on_gpu:      # [flag, bits of the norm]: where the device's verdict lands, one step late, without a synchronisation
                self._skip_host = torch.zeros(2, dtype=torch.int32).pin_memory()
                self._skip_stage = torch.zeros(2, dtype=torch.int32, device=device)
        if self.on_gpu:
            # every launch of libmla_hip.so goes to the CURRENT device's current stream (hip._stream): the owner of this object
            # must have made `device` current (FSDPStrategy.__init__ does), otherwise kernels would run on another device's stream
            assert torch.cuda.current_device() == (self.device.index or 0), \
                f"torch.cuda.set_device({self.device}) must be called before sharding a model onto it"
        # side stream for the collectives (reduce-scatter launched per unit from the backward, all-gather behind the optimizer).
        # NB (measured, round 2): running AdamW itself on a side stream underneath the next forward -- whole, per layer gated on the
        # forward reaching the layer in front, low stream priority, grid capped to 128..1024 workgroups -- never changed the step
        # time: the GEMMs slow down by exactly the AdamW time hidden (the chip is power-bound either way), so it stays inline.
        self.comm_stream = self.ops.stream(device) if self.coll else None
        self.wait_profile = None      # list of (kind, event, event) when a caller wants the main stream's collective stalls timed
        # consumption: a unit's forward waits for ITS all-gather only, so later layers keep streaming in behind the forward pass
        # instead of being waited for up front. Units without a module (root: embeddings, heads, embedders) are waited for in
        # begin_step AND by a pre-hook on every module that directly owns one of their parameters, so an eval forward /
        # predict_action_diff right after optimizer_step never reads half-gathered weights.
        if self.on_gpu and self.comm_stream is not None:
            for u in self.units:
                mod = getattr(u, "module", None)
                if mod is not None:
                    mod.register_forward_pre_hook(lambda m, inp, uu=u: self.wait_unit(uu))
                    if hasattr(mod, "_gather_wait"):      # the previous decoder layer reads this one's input_layernorm weight (ops.NormFoldIO)
                        mod._gather_wait = (lambda uu=u: self.wait_unit(uu))
                else:
                    owned = {id(p) for _, p, _ in u.params}
                    for m in model.modules():
                        if any(id(p) in owned for p in m.parameters(recurse=False)):
                            m.register_forward_pre_hook(lambda mm, inp, uu=u: self.wait_unit(uu))
        # reduce-scatter launch hooks on the decoder layers (fires when the layer's backward has been enqueued)
        for u in self.units:
            mod = getattr(u, "module", None)
            if mod is not None and hasattr(mod, "_grad_hook") and u.trainable and self.coll:
                mod._grad_hook = (lambda uu=u: self._launch_reduce_scatter(uu))

    # ------------------------------------------------------------------------------------------ applied-step counters
    # Plain integers with the guard off. With skip_nonfinite the last step was counted when it was launched, before the host could
    # know its flag; every read (and write) first settles that.
    @property
    def step_count(self) -> int:
        """AdamW's bias-correction step and the Philox step of bf16 moments: optimizer steps that were APPLIED."""
        self._resolve_skip()
        return self._step_count

    @step_count.setter
    def step_count(self, value: int) -> None:
        self._resolve_skip()
        self._step_count = int(value)

    @property
    def ema_updates(self) -> int:
        self._resolve_skip()
        return self._ema_updates

    @ema_updates.setter
    def ema_updates(self, value: int) -> None:
        self._resolve_skip()
        self._ema_updates = int(value)

    @property
    def skipped_steps(self) -> int:
        """Optimizer steps that did nothing because their gradient norm was not finite (skip_nonfinite); 0 without the guard."""
        self._resolve_skip()
        return self._skipped_steps

    @skipped_steps.setter
    def skipped_steps(self, value: int) -> None:
        self._resolve_skip()
        self._skipped_steps = int(value)

    def _resolve_skip(self) -> None:
        """Settle the counters of the last launched step against its flag. On the GPU the flag was copied to pinned memory right
        after it was written; the wait is for that copy alone (work of the step before the current one when called from
        grad_norm_and_clip, which is where a training loop resolves). On a CPU device the flag is just read."""
        pending = self._skip_pending
        if pending is None:
            return
        self._skip_pending = None
        event, ema_step = pending
        if event is not None:
            event.synchronize()
            flag, norm = int(self._skip_host[0]), float(self._skip_host[1:].view(torch.float32))
        else:
            flag, norm = int(self._skip), float(self._norm)
        if not flag:
            self._consecutive_skips = 0
            return
        self._step_count -= 1         # the step was launched as applied; it was not
        if ema_step:
            self._ema_updates -= 1
        self._skipped_steps += 1
        self._consecutive_skips += 1
        if self._consecutive_skips >= self.max_consecutive_skips:
            raise RuntimeError(f"{self._consecutive_skips} consecutive optimizer steps skipped on a non-finite gradient norm (last norm "
                               f"{norm}; max_consecutive_skips={self.max_consecutive_skips}): the weights or the data are broken")

    def _add_unit(self, name, mod, named, no_decay):
        if not named:
            return
        u = FlatUnit(name, named, self.device, self.world, self.rank, self.ops, no_decay, self.pg, collectives=self.coll,
                     inplace_reduce=self.inplace_reduce, arenas=self._arenas, with_ema=self.ema_decay is not None,
                     moment_dtype=MOMENT_FORMATS[self.moments])
        u.module = mod
        self.units.append(u)

    # ------------------------------------------------------------------------------------------ collectives
    def _launch_reduce_scatter(self, u: FlatUnit):
        if not self.coll or not u.trainable or u.rs_event is not None or self.defer_reduce:
            return
        # (advisor, round 4) Before the collective may read grad32: a parameter of this unit that got NO gradient in this window but
        # still holds one from an earlier step is zeroed HERE, on the compute stream, in front of the event the side stream waits for --
        # torch FSDP with use_orig_params presents zero gradients for unused parameters, and zeroing after the launch would race with
        # the in-place collective. From here on the unit's main_grad is locked: a later write (the same layer run through backward a
        # second time in one step, a late autograd .grad) raises in ops._touch / finish_backward instead of corrupting the reduced shard.
        u.zero_stale_and_lock()
        cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        if cur is not None:
            ev = torch.cuda.Event()
            ev.record(cur)
            with torch.cuda.stream(self.comm_stream):
                self.comm_stream.wait_event(ev)
                self._reduce_scatter(u)
                u.rs_event = torch.cuda.Event()
                u.rs_event.record(self.comm_stream)
        else:
            self._reduce_scatter(u)
            u.rs_event = True

    def _reduce_scatter(self, u: FlatUnit):
        backend = dist.get_backend(self.pg)
        if backend == "nccl":
            # SUM either way (in place: gshard = this rank's own slice of grad32; MLA_FSDP_INPLACE_RS=0: a separate shard buffer); the
            # mean's 1 / world lives in grad_div. Never ncclAvg: see __init__.
            dist.reduce_scatter_tensor(u.gshard, u.grad32, op=dist.ReduceOp.SUM, group=self.pg)
        else:  # gloo (CPU tests): all-reduce + slice
            dist.all_reduce(u.grad32, op=dist.ReduceOp.SUM, group=self.pg)
            if not u.inplace_reduce:            # (in place: gshard IS the rank's slice of grad32 and now holds the SUM)
                u.gshard.copy_(u.grad32[self.rank * u.shard_train:(self.rank + 1) * u.shard_train] / self.world)

    def _all_gather(self, u: FlatUnit):
        """bf16 all-gather of the trainable region (frozen weights never change)."""
        region = u.flat16[:u.n_train]
        shard = region[self.rank * u.shard_train:(self.rank + 1) * u.shard_train]
        if dist.get_backend(self.pg) == "nccl":
            # in place: the input is this rank's slice of the output (NCCL/RCCL in-place all-gather: sendbuff == recvbuff +
            # rank * count) -- no per-unit shard copy / allocation on the side stream every step
            dist.all_gather_into_tensor(region, shard, group=self.pg)
        else:
            parts = [torch.empty_like(shard) for _ in range(self.world)]
            dist.all_gather(parts, shard.clone(), group=self.pg)
            region.copy_(torch.cat(parts))

    def _timed_wait(self, kind: str, event) -> None:
        """main stream waits for `event`; with ``wait_profile`` set (bench.py --gpus N) the stall is bracketed by two events on the
        main stream, so the first multi-GPU run says how long the compute stream sat behind each kind of collective."""
        cur = torch.cuda.current_stream(self.device)
        prof = self.wait_profile
        if prof is None:
            cur.wait_event(event)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        cur.wait_event(event)
        e1.record(cur)
        prof.append((kind, e0, e1))

    def wait_profile_ms(self) -> Dict[str, float]:
        """Sum of the recorded stalls per kind (ms); clears the list. Call after a device synchronisation."""
        out: Dict[str, float] = {}
        for kind, e0, e1 in (self.wait_profile or []):
            out[kind] = out.get(kind, 0.0) + e0.elapsed_time(e1)
        if self.wait_profile is not None:
            self.wait_profile = []
        return out

    def wait_unit(self, u: FlatUnit):
        if u.gather_event is not None and u.gather_event is not True:
            self._timed_wait("gather_event", u.gather_event)
        u.gather_event = None

    def wait_all(self):
        """Main stream waits for every outstanding optimizer update / all-gather (checkpointing, evaluation, state access)."""
        for u in self.units:
            self.wait_unit(u)

    # ------------------------------------------------------------------------------------------ step API
    def begin_step(self):
        if self._sq_arena is not None:
            self._sq_arena.used = 0
        for u in self.units:
            u.begin_step()
            u.rs_event = None
        # the bf16 all-gathers of the previous optimizer step were issued in unit order on the side stream; units that own a
        # module wait in their forward pre-hook, the rest (root unit: embeddings, heads) here
        for u in self.units:
            if getattr(u, "module", None) is None or self.device.type != "cuda":
                self.wait_unit(u)

    def finish_micro_backward(self):
        """End of a backward that is not the last of its accumulation window: no reduction, no optimizer."""
        for u in self.units:
            if u.trainable:
                u.collect_autograd_grads()

    def finish_backward(self):
        if self.on_gpu:
            self.wait_all()   # normally long satisfied (every used unit waited in its forward)
        for u in self.units:
            if u.trainable:
                u.finish_backward(already_reduced=u.rs_event is not None)
        if self.coll:
            for u in self.units:
                if u.trainable and u.rs_event is None:
                    self._launch_reduce_scatter(u)
            if self.device.type == "cuda":
                cur = torch.cuda.current_stream(self.device)
                for u in self.units:
                    if u.trainable and u.rs_event is not None and u.rs_event is not True:
                        self._timed_wait("rs_event", u.rs_event)

    def grad_norm_and_clip(self, max_norm: Optional[float]):
        """Global L2 norm over the reduced gradient shards (+ scalar all-reduce), clip coefficient kept on device."""
        first = True
        small: List[torch.Tensor] = []
        for u in self.units:
            if not u.trainable:
                continue
            if u.sq_entries and not self.coll:
                # the big matrices' contributions come from their wgrad epilogues (arena, below); only what no such launch wrote
                # is read here: large pieces (embeddings) in place, the small ones (norm weights, biases) of all units together
                for a, b in u.uncovered_ranges():
                    if b - a > (1 << 20):
                        self.ops.sumsq(u.gshard[a:b], self._sumsq, not first)
                        first = False
                    else:
                        small.append(u.gshard[a:b])
            else:
                self.ops.sumsq(u.gshard, self._sumsq, not first)
                first = False
        if small:
            self.ops.sumsq(torch.cat(small) if len(small) > 1 else small[0], self._sumsq, not first)
            first = False
        if self._sq_arena is not None and self._sq_arena.used:
            self.ops.sum_partials(self._sq_arena.buf, self._sq_arena.used, self._sumsq, not first)    # every wgrad epilogue's partials
            first = False
        if self.coll:
            dist.all_reduce(self._sumsq, op=dist.ReduceOp.SUM, group=self.pg)
        if self.grad_div != 1.0:
            self._sumsq.mul_(1.0 / (self.grad_div * self.grad_div))     # the shards hold SUMS over ranks: norm of the mean gradient
        if self.skip_nonfinite:
            # the previous step's flag: copied to the host a whole step ago. Settled HERE, before its buffers are reused and before
            # optimizer_step forms this step's number -- a skipped step k means step k + 1 runs under k's number.
            self._resolve_skip()
            # decided after the all-reduce: every rank writes the same flag, whichever rank held the bad value
            self.ops.clip_coef_guard(self._sumsq, float(max_norm) if max_norm is not None else 3.0e38, self._coef, self._norm, self._skip)
            if self._skip_host is not None:
                self._skip_stage[:1].copy_(self._skip)
                self._skip_stage[1:].copy_(self._norm.view(torch.int32))
                self._skip_host.copy_(self._skip_stage, non_blocking=True)
                self._skip_copied = torch.cuda.Event()
                self._skip_copied.record(torch.cuda.current_stream(self.device))
            self._norm_fresh = True
        else:
            self.ops.clip_coef(self._sumsq, float(max_norm) if max_norm is not None else 3.0e38, self._coef, self._norm)
        if self.grad_div != 1.0:
            self._coef.mul_(1.0 / self.grad_div)                        # AdamW's gradient scale = clip coefficient x 1 / world
        return self._norm

    def optimizer_step(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        if self._ema_swapped:
            raise RuntimeError("optimizer_step inside ema_weights(): the bf16 replica holds the average, not the weights")
        if self.skip_nonfinite:
            if not self._norm_fresh:      # the flag would be an earlier step's
                raise RuntimeError("optimizer_step with skip_nonfinite needs grad_norm_and_clip() first: no gradient norm since the last step")
            self._norm_fresh = False
        self.step_count += 1
        # an EMA step runs the same launches over the same ranges with the average as one more stream; every other step (and every
        # step without ema_decay) runs exactly the plain launches
        ema_step = self.ema_decay is not None and self.step_count % self.ema_update_every == 0
        if ema_step:
            self.ema_updates += 1
        if self.skip_nonfinite:
            # counted as applied; _resolve_skip takes it back if the flag (on its way to the host since grad_norm_and_clip) says otherwise
            self._skip_pending = (self._skip_copied, ema_step)
            self._skip_copied = None

        for ordinal, u in enumerate(self.units):
            if not u.trainable:
                continue
            ranges = u._shard_ranges()
            if self.moments == "bf16" or self.skip_nonfinite:
                # the same ranges through the bf16-moment launch (one entry point: n_decay = n or 0 is the one-group case, ema=None
                # the plain step) or, with skip_nonfinite, through the guarded launch of either moment format behind the step's flag.
                # index_base = the element's position in the unit's flat trainable region, under the unit's ordinal: the random bits
                # do not depend on how the ranks cut the region, nor on how a shard is cut into launches
                base = (ordinal << 40) + u.rank * u.shard_train
                ema = u.ema if ema_step else None
                if ranges and ranges[0][0] == 0 and all(ranges[i][1] == ranges[i + 1][0] and
                                                        ranges[i][2] + (ranges[i][1] - ranges[i][0]) == ranges[i + 1][2]
                                                        for i in range(len(ranges) - 1)):
                    merged = [(0, ranges[-1][1], ranges[0][2], sum(le - ls for ls, le, _, dec in ranges if dec))]
                else:
                    merged = [(ls, le, g0, le - ls if dec else 0) for ls, le, g0, dec in ranges]
                for ls, le, g0, n_dec in merged:
                    args = (u.master_train[ls:le], u.gshard[ls:le], u.exp_avg[ls:le], u.exp_avg_sq[ls:le],
                            None if ema is None else ema[ls:le], u.flat16[g0:g0 + (le - ls)], n_dec, lr, betas, eps, weight_decay,
                            self._step_count, self._coef, self.ema_decay, self.moments_seed, base + ls)
                    if self.skip_nonfinite:
                        self.ops.adamw_guard(*args, self._skip)
                    else:
                        self.ops.adamw_m16(*args)
            elif hasattr(self.ops, "adamw_groups") and ranges and ranges[0][0] == 0 and \
                    all(ranges[i][1] == ranges[i + 1][0] and ranges[i][2] + (ranges[i][1] - ranges[i][0]) == ranges[i + 1][2]
                        for i in range(len(ranges) - 1)):
                # the local shard is [decayed | not decayed] back to back: both parameter groups in one launch
                n_local = ranges[-1][1]
                n_dec = sum(le - ls for ls, le, _, dec in ranges if dec)
                g0 = ranges[0][2]
                if ema_step:
                    self.ops.adamw_ema_groups(u.master_train[:n_local], u.gshard[:n_local], u.exp_avg[:n_local], u.exp_avg_sq[:n_local],
                                              u.ema[:n_local], u.flat16[g0:g0 + n_local], n_dec, lr, betas, eps, weight_decay,
                                              self.step_count, self._coef, self.ema_decay)
                else:
                    self.ops.adamw_groups(u.master_train[:n_local], u.gshard[:n_local], u.exp_avg[:n_local], u.exp_avg_sq[:n_local],
                                          u.flat16[g0:g0 + n_local], n_dec, lr, betas, eps, weight_decay, self.step_count, self._coef)
            else:
                for ls, le, g0, decayed in ranges:
                    if ema_step:
                        self.ops.adamw_ema(u.master_train[ls:le], u.gshard[ls:le], u.exp_avg[ls:le], u.exp_avg_sq[ls:le], u.ema[ls:le],
                                           u.flat16[g0:g0 + (le - ls)], lr, betas, eps, weight_decay if decayed else 0.0,
                                           self.step_count, self._coef, self.ema_decay)
                    else:
                        self.ops.adamw(u.master_train[ls:le], u.gshard[ls:le], u.exp_avg[ls:le], u.exp_avg_sq[ls:le],
                                       u.flat16[g0:g0 + (le - ls)], lr, betas, eps, weight_decay if decayed else 0.0, self.step_count,
                                       self._coef)
            if self.coll:
                if self.on_gpu:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self.comm_stream):
                        self.comm_stream.wait_event(ev)
                        self._all_gather(u)
                        u.gather_event = torch.cuda.Event()
                        u.gather_event.record(self.comm_stream)
                else:
                    self._all_gather(u)

    # ------------------------------------------------------------------------------------------ checkpoint helpers
    def iter_full_state_fp32(self, to_cpu_on_rank0: bool = False):
        """Yields ``(name, fp32 tensor)`` for every parameter, ONE UNIT AT A TIME: each unit's master shards are gathered (all ranks
        take part in the collectives), handed out, and freed before the next unit is touched, so the peak extra device memory is
        one unit (<= 0.8 GB for a 7B decoder layer), not the +27 GB of a whole fp32 model. With ``to_cpu_on_rank0`` only rank 0
        receives tensors (already copied to host memory); the other ranks get ``(name, None)`` -- the reference's
        FullStateDictConfig(offload_to_cpu=True, rank0_only=True), training/strategies/fsdp.py:107-110."""
        if self.on_gpu:
            self.wait_all()
        for u in self.units:
            full = self._gather_master(u)
            keep = (not to_cpu_on_rank0) or self.rank == 0
            for n, p, o in u.params:
                if not keep:
                    yield n, None
                    continue
                t = full[o:o + p.numel()].view(p.shape)
                yield n, (t.cpu() if to_cpu_on_rank0 else t.clone())
            del full

    def full_state_dict_fp32(self) -> Dict[str, torch.Tensor]:
        """Full fp32 state dict on the device of every rank (tests / small models; checkpoints use iter_full_state_fp32)."""
        return dict(self.iter_full_state_fp32())

    def _gather_master(self, u: FlatUnit):
        if not self.coll:
            return torch.cat([u.master_train, u.master_frozen])
        full = torch.empty(u.n_total, dtype=torch.float32, device=self.device)
        parts_t = [torch.empty(u.shard_train, dtype=torch.float32, device=self.device) for _ in range(self.world)]
        dist.all_gather(parts_t, u.master_train, group=self.pg)
        full[:u.n_train] = torch.cat(parts_t)
        nf = (u.n_total - u.n_train) // self.world
        if nf:
            parts_f = [torch.empty(nf, dtype=torch.float32, device=self.device) for _ in range(self.world)]
            dist.all_gather(parts_f, u.master_frozen, group=self.pg)
            full[u.n_train:] = torch.cat(parts_f)
        return full

    # ------------------------------------------------------------------------------------------ optimizer state (resume)
    def _gather_moments(self, u: FlatUnit):
        """The unit's two AdamW moments over the whole trainable region (n_train elements each), on the device of every rank."""
        if not self.coll:
            return u.exp_avg, u.exp_avg_sq           # world 1 without collectives: the shard IS the region
        out = []
        for shard in (u.exp_avg, u.exp_avg_sq):
            parts = [torch.empty(u.shard_train, dtype=shard.dtype, device=self.device) for _ in range(self.world)]      # stored dtype
            dist.all_gather(parts, shard, group=self.pg)
            out.append(torch.cat(parts))
        return out[0], out[1]

    def iter_optimizer_state(self, to_cpu_on_rank0: bool = False):
        """Twin of ``iter_full_state_fp32`` for AdamW's moments: yields ``(name, exp_avg, exp_avg_sq)`` as tensors of the stored
        dtype (fp32; bf16 with ``moments="bf16"``: the same bits, never a conversion) in the parameter's shape for every TRAINABLE
        parameter, one unit at a time (every rank takes part in the gathers; the peak extra device memory is
        one unit's two moments). The 8-element padding between tensors is dropped. With ``to_cpu_on_rank0`` only rank 0 receives
        (host) tensors, the other ranks ``(name, None, None)``. The layouts differ only in where the GRADIENT shard lives (no
        collectives / separate shard / in-place reduce-scatter); the moments are 1/world shards of the trainable region in all three."""
        if self.on_gpu:
            self.wait_all()
        keep = (not to_cpu_on_rank0) or self.rank == 0
        for u in self.units:
            if not u.trainable:
                continue
            m, v = self._gather_moments(u)
            for n, p, o in u.params:
                if not p.requires_grad:
                    continue
                if not keep:
                    yield n, None, None
                    continue
                a, b = m[o:o + p.numel()].view(p.shape), v[o:o + p.numel()].view(p.shape)
                # (never a view of the live shard: .cpu() of a host tensor would be one)
                yield (n, a.cpu(), b.cpu()) if (to_cpu_on_rank0 and a.is_cuda) else (n, a.clone(), b.clone())
            del m, v

    def load_optimizer_state(self, state, step_count: int) -> None:
        """Inverse of ``iter_optimizer_state``: ``state`` maps parameter name -> ``(exp_avg, exp_avg_sq)`` as FULL tensors (host or
        device); every rank copies its own ``[rank * shard_train, (rank + 1) * shard_train)`` slice of every unit into its moment
        shards (padding = 0) and ``step_count`` is restored. The mapping is keyed by name, not by shard, so a state written at one
        world size loads at any other. Only the pieces that intersect the rank's shard are moved, tensor by tensor: no rank ever holds
        a unit's full moments on the device. Everything is validated BEFORE the first write: a missing name, an unknown name or a
        shape mismatch raises ValueError and leaves the optimizer state as it was. So does a tensor of another dtype than the
        moments are stored in (``moments``): a state of the other format is refused, never converted in either direction."""
        want = {n: p for u in self.units if u.trainable for n, p, _ in u.params if p.requires_grad}
        missing = [n for n in want if n not in state]
        extra = [n for n in state if n not in want]
        bad, fmt, want_dtype = [], [], MOMENT_FORMATS[self.moments]
        for n, p in want.items():
            if n in state:
                pair = state[n]
                if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(torch.is_tensor(t) for t in pair)):
                    bad.append(f"{n} (not an (exp_avg, exp_avg_sq) pair of tensors)")
                    continue
                for kind, t in zip(("exp_avg", "exp_avg_sq"), pair):
                    if tuple(t.shape) != tuple(p.shape):
                        bad.append(f"{n}.{kind} {tuple(t.shape)} != {tuple(p.shape)}")
                    if t.dtype != want_dtype:
                        fmt.append(f"{n}.{kind}")
        if fmt and not (missing or extra or bad):
            theirs = sorted({str(t.dtype) for pair in state.values() for t in pair})
            raise ValueError(f"optimizer state holds {', '.join(theirs)} moments but this model stores them as {want_dtype} "
                             f"(moments={self.moments!r}; formats: {', '.join(f'{k!r} = {v}' for k, v in MOMENT_FORMATS.items())}): "
                             f"no conversion in either direction ({len(fmt)} tensors, first {fmt[0]})")
        if missing or extra or bad:
            raise ValueError("optimizer state does not match the model's trainable parameters: "
                             + "; ".join(f"{k}: {', '.join(v)}" for k, v in (("missing", missing), ("unexpected", extra), ("wrong shape", bad)) if v))
        if self.on_gpu:
            self.wait_all()
        for u in self.units:
            if not u.trainable:
                continue
            lo = self.rank * u.shard_train
            hi = lo + u.shard_train
            u.exp_avg.zero_()
            u.exp_avg_sq.zero_()
            for n, p, o in u.params:
                if not p.requires_grad:
                    continue
                a, b = max(o, lo), min(o + p.numel(), hi)
                if b <= a:
                    continue
                for dst, src in zip((u.exp_avg, u.exp_avg_sq), state[n]):
                    dst[a - lo:b - lo].copy_(src.detach().reshape(-1)[a - o:b - o])
        self.step_count = int(step_count)

    # ------------------------------------------------------------------------------------------ weight average (EMA)
    def _require_ema(self, what: str) -> None:
        if self.ema_decay is None:
            raise RuntimeError(f"{what} needs a ShardedModel built with ema_decay (this one keeps no weight average)")

    def _gather_ema(self, u: FlatUnit):
        if not self.coll:
            return u.ema
        parts = [torch.empty(u.shard_train, dtype=torch.float32, device=self.device) for _ in range(self.world)]
        dist.all_gather(parts, u.ema, group=self.pg)
        return torch.cat(parts)

    def iter_ema_state(self, to_cpu_on_rank0: bool = False):
        """Twin of ``iter_optimizer_state`` for the weight average: yields ``(name, fp32 tensor in the parameter's shape)`` for every
        TRAINABLE parameter, one unit at a time (every rank takes part in the gathers), padding dropped. With ``to_cpu_on_rank0`` only
        rank 0 receives (host) tensors, the other ranks ``(name, None)``."""
        self._require_ema("iter_ema_state")
        if self.on_gpu:
            self.wait_all()
        keep = (not to_cpu_on_rank0) or self.rank == 0
        for u in self.units:
            if not u.trainable:
                continue
            e = self._gather_ema(u)
            for n, p, o in u.params:
                if not p.requires_grad:
                    continue
                if not keep:
                    yield n, None
                    continue
                t = e[o:o + p.numel()].view(p.shape)
                yield (n, t.cpu()) if (to_cpu_on_rank0 and t.is_cuda) else (n, t.clone())
            del e

    def load_ema_state(self, state, ema_updates: int) -> None:
        """Inverse of ``iter_ema_state``, twin of ``load_optimizer_state``: ``state`` maps parameter name -> FULL fp32 tensor (host or
        device); every rank copies its own slice of every unit (padding = 0) and ``ema_updates`` is restored. Keyed by name: loads at
        any world size. Everything is validated BEFORE the first write: a missing name, an unknown name or a shape mismatch raises
        ValueError and leaves the average as it was."""
        self._require_ema("load_ema_state")
        want = {n: p for u in self.units if u.trainable for n, p, _ in u.params if p.requires_grad}
        missing = [n for n in want if n not in state]
        extra = [n for n in state if n not in want]
        bad = []
        for n, p in want.items():
            if n in state:
                t = state[n]
                if not torch.is_tensor(t):
                    bad.append(f"{n} (not a tensor)")
                elif tuple(t.shape) != tuple(p.shape):
                    bad.append(f"{n} {tuple(t.shape)} != {tuple(p.shape)}")
        if missing or extra or bad:
            raise ValueError("EMA state does not match the model's trainable parameters: "
                             + "; ".join(f"{k}: {', '.join(v)}" for k, v in (("missing", missing), ("unexpected", extra), ("wrong shape", bad)) if v))
        if self.on_gpu:
            self.wait_all()
        for u in self.units:
            if not u.trainable:
                continue
            lo = self.rank * u.shard_train
            hi = lo + u.shard_train
            u.ema.zero_()
            for n, p, o in u.params:
                if not p.requires_grad:
                    continue
                a, b = max(o, lo), min(o + p.numel(), hi)
                if b > a:
                    u.ema[a - lo:b - lo].copy_(state[n].detach().reshape(-1)[a - o:b - o])
        self.ema_updates = int(ema_updates)

    def reset_ema(self) -> None:
        """The average restarts as a copy of the masters, as at construction; ``ema_updates`` = 0."""
        self._require_ema("reset_ema")
        if self.on_gpu:
            self.wait_all()
        for u in self.units:
            if u.trainable:
                u.ema.copy_(u.master_train[:u.shard_train])
        self.ema_updates = 0

    def _swap_replica(self, from_ema: bool) -> None:
        """bf16 replica of every trainable parameter <- bf16(average) or bf16(master): the local shard through the cast the units were
        built with, then the unit's all-gather. The optimizer's writes into the replica go through raw pointers and leave the
        parameters' version counters alone (nothing in optimizer_step touches them), so the counters are advanced here: copies keyed
        on (data_ptr, _version) -- mla_amd/infer.py's packed and FP8 weights and its captured graphs -- rebuild after either swap."""
        if self.on_gpu:
            self.wait_all()
        for u in self.units:
            if not u.trainable:
                continue
            lo = self.rank * u.shard_train
            self.ops.cast_to_bf16(u.ema if from_ema else u.master_train[:u.shard_train], u.flat16[lo:lo + u.shard_train])
            if self.coll:
                if self.on_gpu:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self.comm_stream):
                        self.comm_stream.wait_event(ev)
                        self._all_gather(u)
                        u.gather_event = torch.cuda.Event()
                        u.gather_event.record(self.comm_stream)
                else:
                    self._all_gather(u)
            for _, p, _ in u.params:
                if p.requires_grad:
                    torch.autograd.graph.increment_version(p)
        if self.on_gpu:
            self.wait_all()

    def ema_weights(self):
        """Context manager: inside, the bf16 replica of every trainable parameter holds bf16(average) -- evaluate or sample from the
        averaged policy; on exit it is cast back from the masters, bit-identical to what it held before (the cast equals AdamW's fused
        bf16 write). Masters, moments and the average itself are not touched. Raises inside an open accumulation window and on re-entry."""
        import contextlib

        @contextlib.contextmanager
        def swapped():
            self._require_ema("ema_weights")
            if self._ema_swapped:
                raise RuntimeError("ema_weights() is already open")
            if self.defer_reduce:
                raise RuntimeError("ema_weights() inside an open accumulation window: finish the window's last micro-batch first")
            self._ema_swapped = True
            try:
                self._swap_replica(from_ema=True)
                yield self
            finally:
                self._swap_replica(from_ema=False)
                self._ema_swapped = False
        return swapped()

    def state_bytes(self):
        return sum(u.state_bytes() for u in self.units)
