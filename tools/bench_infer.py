#!/usr/bin/env python
"""Latency of the inference path at 7B scale: MLA.predict_action_diff = 8-step DDIM, batch 1,
548-token sequence per step (672x672 image + 1024 points + prompt). Random-init weights, synthetic inputs.
    python tools/bench_infer.py [--steps 8] [--iters 5] [--chunk C]
    python tools/bench_infer.py --batch B [--chunk C]     MLA.predict_action_diff_batch on B observations with ragged prompts (lengths
                                                          drawn from a fixed seed) AND, in the same process, B sequential
                                                          predict_action_diff calls on the same observations
    python tools/bench_infer.py --suffix-weights fp8      the sampler steps stream the FP8 copy of the decoder weights (infer.py)
    python tools/bench_infer.py --pair-fp8 [--pairs P] [--chunk C] [--kernel-table]
                                                          bf16 and fp8 chunks alternating in one process (same box, same clocks): per-chunk
                                                          latency and the suffix pass alone, per pair, with the 95 % interval of the pair
                                                          differences; --kernel-table adds mla_gemv_w8 vs mla_gemm_skinny_w8 per 7B
                                                          projection shape at M = 2, 5, 8, 17 (the engine's selection rule is set from it)
    python tools/bench_infer.py --pair-mx [--pairs P] [--chunks C[,C..]] [--operand fused|once|both] [--kernel-table]
                                                         bf16 / fp8 / fp4 (suffix_mx="fp4": the MXFP4 copy) chunks with sampler="device",
                                                         alternating in one process, and their captured suffix passes; mean and 95 %
                                                         interval of the pair differences fp8 - bf16, fp4 - bf16 and fp4 - fp8, one
                                                         line per chunk length (and, with "both", a second one with
                                                         suffix_operand="once" where the pass has more than 8 rows);
                                                         --kernel-table adds the _w8 and _w4 kernels per 7B projection shape and M
    python tools/bench_infer.py --samples N[,N..] [--chunks C[,C..]] [--pairs P] [--kernel-table]
                                                          N action chunks for ONE observation, three forms of the same work alternating in
                                                          one process (same box, same clocks), per pair, with the 95 % interval of the pair
                                                          differences: (a) predict_action_diff_samples, (b) predict_action_diff_batch on N
                                                          copies of the observation, (c) N sequential predict_action_diff calls;
                                                          --kernel-table adds mla_attn_chunk_groups alone at 1 / 2 / 4 groups per workgroup
                                                          against mla_attn_chunk_ragged on N copies of the prefix
    python tools/bench_infer.py --samples N[,N..] --pair-fp8 [--chunks C[,C..]] [--pairs P] [--kernel-table]
                                                          predict_action_diff_samples with bf16 and fp8 suffix weights alternating in one
                                                          process, in pairs: per-call latency and the suffix pass alone with the 95 %
                                                          interval of the pair differences; --kernel-table adds mla_gemm_suffix_w8 against
                                                          mla_gemm_suffix_bf16 per 7B projection shape at M = 34, 68, 136, 255
    python tools/bench_infer.py --batch B[,B..] --samples N[,N..] [--pair-fp8] [--chunk C] [--pairs P] [--kernel-table]
                                                          N action chunks for EACH of B observations with ragged prompts (the lists are
                                                          paired element-wise: --batch 2,4 --samples 4,3 measures (2, 4) and (4, 3)): two
                                                          forms of the same work alternating in one process, per pair, with the 95 %
                                                          interval of the pair differences: (a) predict_action_diff_batch(num_samples=N),
                                                          (b) B sequential predict_action_diff_samples calls; --pair-fp8 measures both forms
                                                          with bf16 and with fp8 suffix weights; --kernel-table adds
                                                          mla_attn_chunk_ragged_groups per launch against mla_attn_chunk_groups run per sample
    python tools/bench_infer.py --pair-prefill [--pairs P] [--chunk C] [--kernel-table]
                                                          prefill="train", prefill="compact" and prefill="compact" with
                                                          prefill_precision="fp8" alternating in one process, with bf16 and with fp8 suffix
                                                          weights: per-chunk latency, the whole prefill (encoders + decoder rows) and the
                                                          decoder rows alone, with the 95 % interval of the pair differences (compact -
                                                          train, fp8 - compact, fp8 - train); --kernel-table adds the four projections of a
                                                          7B layer at the prefix's row count, training kernel vs compact kernel vs FP8
                                                          compact kernel (and the activation quantiser it needs), per launch
    python tools/bench_infer.py --pair-sampler [--pairs P] [--chunks C[,C..]]
                                                          sampler="host" and sampler="device" chunks alternating in one process, in pairs,
                                                          for every chunk length (default 1,16) with bf16 and with fp8 suffix weights:
                                                          per-chunk latency with the 95 % interval of the pair differences, the prefill
                                                          (encoders + prefix rows) alone, and the per-step share (chunk - prefill) / steps
                                                          of both arms; also whether the two arms returned the same bits
    python tools/bench_infer.py --pair-ddpm-sampler [--pairs P] [--chunks C[,C..]]
                                                          the same for the DDPM loop: use_ddim=False calls (the 100 steps of the training
                                                          diffusion) with ddpm_sampler="host" and ddpm_sampler="device" alternating in
                                                          one process, in pairs
    python tools/bench_infer.py --pair-pinned [--pairs P] [--chunks C[,C..]]
                                                          sampler="device" chunks without and with known_actions (the first min(3, C)
                                                          chunk steps pinned) alternating in one process, in pairs, for every chunk length
                                                          (default 1,16) with bf16 and with fp8 suffix weights: per-chunk latency with the
                                                          95 % interval of the pair differences; also whether the pinned steps came back
                                                          exactly and whether sampler="host" returns the pinned chunk's bits
    python tools/bench_infer.py --pair-attention [--pairs P] [--chunks C[,C..]] [--kernel-table]
                                                          suffix_attention="head" and "split" chunks alternating in one process, in pairs,
                                                          for every chunk length (default 1,16) with bf16 and with fp8 suffix weights (the
                                                          device sampler in both arms): per-chunk latency and the suffix pass alone with the
                                                          95 % interval of the pair differences; --kernel-table first prints, without the
                                                          model, one launch pair (split + combine) per splits in {1, 2, 3, plan, nT} against
                                                          mla_attn_decode / mla_attn_chunk at 32 heads for (R, S_kv) = (2, 547), (17, 562);
                                                          --pairs 0 stops after the table
    python tools/bench_infer.py --pair-attention --samples N[,N..] [--chunks C[,C..]] [--pairs P] [--kernel-table]
    python tools/bench_infer.py --pair-attention --batch B[,B..] [--samples N[,N..]] [--chunks C[,C..]] [--pairs P] [--kernel-table]
                                                          groups_attention="head" and "split" alternating in one process, in pairs, on
                                                          predict_action_diff_samples / predict_action_diff_batch (the lists paired
                                                          element-wise) with bf16 and with fp8 suffix weights (the device sampler in both
                                                          arms; --batch without --samples takes its fp8 arm through num_samples=1): per-call
                                                          latency and the suffix pass alone with the 95 % interval of the pair differences;
                                                          --kernel-table first prints, without the model, one launch (pair) per splits in
                                                          {1, 2, 3, plan} of mla_attn_groups_split against the route's head launch at 32
                                                          heads and 545 prefix rows; --pairs 0 stops after the table
    python tools/bench_infer.py --pair-operand [--pairs P] [--chunks C[,C..]] [--kernel-table]
                                                          suffix_operand="fused" and "once" chunks alternating in one process, in pairs,
                                                          per chunk length (default 1, 8, 16), with bf16 and fp8 suffix weights, the device
                                                          sampler in both arms: per-chunk latency and the captured suffix pass alone with
                                                          the 95 % interval of the pair differences; --kernel-table first prints, without
                                                          the model, one line per 7B projection shape at M = 9, 17, 33, 64 for bf16 and W8:
                                                          the fused form, the plain form, and for gate|up the SwiGLU-epilogue form against
                                                          plain gate|up + swiglu_fwd; --pairs 0 stops after the table
    python tools/bench_infer.py --batch B[,B..] --pair-batch-prefill [--chunks C[,C..]] [--pairs P] [--kernel-table]
                                                          predict_action_diff_batch with batch_prefill="train" and "fp8" in one process,
                                                          alternating: per-call latency and the engines' prefill behind the encoders
                                                          (embedding + the decoder rows of the B x S_p prefix) with the 95 % interval of
                                                          the pair differences; --kernel-table first prints, without the model, one launch
                                                          per 7B projection shape at M = 1090, 2180 and 4360: the wide-row FP8 GEMM against
                                                          the training kernel and against the 64-row FP8 kernel run in slices of at most
                                                          1024 rows; --pairs 0 stops after the table
    python tools/bench_infer.py --pair-solver [--ddim-steps K] [--pairs P] [--chunks C[,C..]]
                                                          solver="ddim" and solver="dpmpp2m" (DPM-Solver++(2M)) chunks with
                                                          sampler="device", alternating in one process, in pairs, for every chunk length
                                                          (default 1,16) with bf16 and with fp8 suffix weights, two cases per setting: both
                                                          solvers at --steps (what the solver's own update costs), and dpmpp2m at K steps
                                                          (default 4) against ddim at --steps (what the solver is for); per-chunk latency
                                                          with the 95 % interval of the pair differences, and whether sampler="host"
                                                          returns the 2M chunk's bits
    python tools/bench_infer.py --solver dpmpp2m --ddim-steps K [--sampler device] [--chunk C] [--suffix-weights W]
                                                          the single measurement with the solver keyword and create_ddim(ddim_step=K) in
                                                          front of the first call (without --ddim-steps: --steps)
Prints one JSON line per measurement (not the driver's bench contract -- that is bench.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _setup(args_or_chunk=None, B=1, model=None):
    """-> (model, synthetic batch of B observations, prompt ids): MLA-Llama2-7B with random weights cast to bf16 (built once: pass it back
    as `model` for further batches), future_action_window_size = chunk - 1 when a chunk (or the parsed arguments) is given. B = 1: ids
    [1, L] = the synthetic prompt + the tag the splice looks for; B > 1: a list of B ragged prompts, 0 .. 12 ids shorter each (fixed seed)."""
    from bench import build
    from mla_amd.infer import SPLICE_TAG
    from mla_amd.synthetic import make_batch
    dev = torch.device("cuda", 0)
    m = model
    if m is None:
        torch.manual_seed(0)
        m = build(dev, 1)
        m.eval()
        for p in m.parameters():
            p.data = p.data.to(torch.bfloat16)
    chunk = getattr(args_or_chunk, "chunk", args_or_chunk)
    if chunk is not None:
        m.future_action_window_size = m.vlm.future_action_window_size = chunk - 1
    b = make_batch(B=B, device=dev)
    if B == 1:
        return m, b, torch.cat([b["input_ids"][:, :-4], torch.tensor([[SPLICE_TAG]], device=dev)], dim=1)
    drop = torch.randint(0, 13, (B,), generator=torch.Generator().manual_seed(1234)).tolist()
    return m, b, [torch.cat([b["input_ids"][i, :b["input_ids"].shape[1] - 4 - drop[i]], torch.tensor([SPLICE_TAG], device=dev)]) for i in range(B)]


def _observation(b, i=0):
    """Observation i of the synthetic batch as predict_action_diff takes it: (image, pointcloud, cur_robot_state)."""
    return b["images"]["front_image"][i], b["point_cloud"][i], b["proprio"][i, 0].cpu().numpy()


def _engine_kw(b):
    """Observation 0 as an engine's for_inputs / prefill takes it."""
    return dict(images=b["images"]["front_image"][:1], point_cloud=b["point_cloud"][:1], camera_name="rlbench_front", proprio=b["proprio"][:1])


def _time_ms(fn, iters):
    """Host clock around `iters` calls between two device synchronisations -> ms per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def _replay_ms(eng, n=8):
    """Device events around n runs of the engine's (captured) suffix pass -> ms per pass."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        eng._run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1, help="future_action_window_size + 1")
    ap.add_argument("--no-reuse-prefix", action="store_true", help="the reference's control flow: a whole forward per DDIM step")
    ap.add_argument("--batch", type=str, default="0", help="B > 0: predict_action_diff_batch on B observations vs B sequential calls; with "
                    "--samples: B[,B..] paired with N[,N..]")
    ap.add_argument("--suffix-weights", choices=["bf16", "fp8", "fp8_as_bf16"], default="bf16")
    ap.add_argument("--pair-fp8", action="store_true", help="alternate bf16 and fp8 chunks in one process, in pairs")
    ap.add_argument("--pair-mx", action="store_true", help="alternate bf16, fp8 and fp4 (suffix_mx) chunks with sampler=\"device\" in one process, in pairs")
    ap.add_argument("--operand", choices=["fused", "once", "both"], default="fused", help="with --pair-mx: suffix_operand of every arm")
    ap.add_argument("--pair-prefill", action="store_true", help="alternate prefill=\"train\", \"compact\" and \"compact\" with prefill_precision=\"fp8\" in one process")
    ap.add_argument("--pair-sampler", action="store_true", help="alternate sampler=\"host\" and sampler=\"device\" in one process, in pairs")
    ap.add_argument("--pair-ddpm-sampler", action="store_true", help="alternate ddpm_sampler=\"host\" and ddpm_sampler=\"device\" on use_ddim=False calls in one process, in pairs")
    ap.add_argument("--pair-pinned", action="store_true", help="alternate sampler=\"device\" chunks without and with known_actions in one process, in pairs")
    ap.add_argument("--pair-attention", action="store_true", help="alternate suffix_attention=\"head\" and \"split\" in one process, in pairs; with --samples / --batch: groups_attention "
                    "on the multi-row routes")
    ap.add_argument("--pair-operand", action="store_true", help="alternate suffix_operand=\"fused\" and \"once\" in one process, in pairs")
    ap.add_argument("--pair-batch-prefill", action="store_true", help="with --batch: alternate batch_prefill=\"train\" and \"fp8\" in one process, in pairs")
    ap.add_argument("--pair-solver", action="store_true", help="alternate solver=\"ddim\" and solver=\"dpmpp2m\" chunks with sampler=\"device\" in one process, in pairs")
    ap.add_argument("--solver", choices=["ddim", "dpmpp2m"], default="ddim", help="the single measurement: solver of predict_action_diff")
    ap.add_argument("--sampler", choices=["host", "device"], default="host", help="the single measurement: sampler of predict_action_diff")
    ap.add_argument("--ddim-steps", type=int, default=None, help="steps of the respaced process (create_ddim in front of the first call); --pair-solver: "
                    "the step count of the short dpmpp2m arm (default 4)")
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--kernel-table", action="store_true", help="with --pair-fp8: the two _w8 kernels per projection shape and M; with "
                    "--samples: mla_attn_chunk_groups per groups-per-workgroup against mla_attn_chunk_ragged")
    ap.add_argument("--samples", type=str, default="", help="N[,N..]: predict_action_diff_samples vs the batched call on N copies vs N calls")
    ap.add_argument("--chunks", type=str, default="", help="with --samples / --pair-sampler: action chunk lengths to measure in one process (default: --chunk; --pair-sampler: 1,16)")
    args = ap.parse_args()
    if args.pair_sampler or args.pair_ddpm_sampler:
        return main_pair_sampler(args, ddpm=args.pair_ddpm_sampler)
    if args.pair_pinned:
        return main_pair_pinned(args)
    if args.pair_solver:
        return main_pair_solver(args)
    if args.pair_operand:
        return main_pair_operand(args)
    batches = [int(v) for v in args.batch.split(",")]
    if args.pair_batch_prefill:
        return main_pair_batch_prefill(args, batches)
    if args.pair_attention:
        return main_pair_groups_attention(args, batches) if args.samples or batches != [0] else main_pair_attention(args)
    if args.samples and batches != [0]:
        return main_batch_samples(args, batches)
    args.batch = batches[0]
    if args.samples:
        return main_samples_pair(args) if args.pair_fp8 else main_samples(args)
    if args.batch > 0:
        return main_batch(args)
    if args.pair_prefill:
        return main_pair_prefill(args)
    if args.pair_mx:
        return main_pair(args, mx=True)
    if args.pair_fp8:
        return main_pair(args)
    m, b, ids = _setup(args)
    dev = ids.device
    image, pc, state = _observation(b)
    if args.ddim_steps is not None:
        args.steps = args.ddim_steps
        m.create_ddim(ddim_step=args.steps)
    kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps,
              reuse_prefix=not args.no_reuse_prefix, suffix_weights=args.suffix_weights)
    if args.solver != "ddim":
        kw["solver"] = args.solver
    if args.sampler != "host":
        kw["sampler"] = args.sampler
    act = m.predict_action_diff(**kw)
    ms = _time_ms(lambda: m.predict_action_diff(**kw), args.iters)
    parts = {}
    if not args.no_reuse_prefix:
        # where the cached path's time goes: the prefill (encoders + one 545-row pass) and one graph replay over the suffix rows
        from mla_amd.infer import PrefixCachedEps
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        eng = PrefixCachedEps.for_inputs(m.vlm, ids, n_action_rows=args.chunk, suffix_weights=args.suffix_weights, **_engine_kw(b))
        ev[1].record()
        x = torch.randn(1, args.chunk, 7, device=dev)
        t = torch.tensor([91], device=dev)
        eng(x, t)
        ev[2].record()
        pass_ms = _replay_ms(eng)
        wbytes = _stream_bytes(m, args.suffix_weights)
        parts = {"prefill_ms": round(ev[0].elapsed_time(ev[1]), 2), "one_eps_call_ms": round(ev[1].elapsed_time(ev[2]), 2),
                 "suffix_pass_graph_replay_ms": round(pass_ms, 3), "weights_streamed_per_pass_gb": round(wbytes / 1e9, 2),
                 "suffix_pass_weight_stream_tbps": round(wbytes / 1e12 / (pass_ms * 1e-3), 2)}
    print(json.dumps({"metric": "predict_action_diff latency, MLA-Llama2-7B bf16, batch 1", "suffix_weights": args.suffix_weights,
                      "solver": args.solver, "sampler": args.sampler, "value": round(ms, 1), "unit": "ms",
                      "ddim_steps": args.steps, "ms_per_ddim_step": round(ms / args.steps, 1), "seq_len": int(ids.shape[1]) + 513 + 2 + args.chunk,
                      "action_chunk": args.chunk, "reuse_prefix": not args.no_reuse_prefix, **parts, "action": [round(float(v), 4) for v in act.reshape(-1)[:7]], "data": "synthetic"}))


def _stream_bytes(m, mode):
    """Bytes of decoder weights one suffix pass streams in `mode` (a value of suffix_weights / suffix_mx): the byte count of the model's
    coded copy, codes and scales (it exists once a call in that mode has run), or every layer parameter in bf16 (the norm weights are
    noise next to it)."""
    from mla_amd.infer import CODED
    if mode in CODED:
        return sum(w.nbytes for layer in m.vlm.__dict__[CODED[mode].slot][mode] for w in layer if isinstance(w, CODED[mode]))
    return 2 * sum(p.numel() for l in m.vlm.llm_backbone.llm.model.layers for p in l.parameters())


_T95 = {2: 12.71, 3: 4.30, 4: 3.18, 5: 2.78, 6: 2.57, 7: 2.45, 8: 2.36, 9: 2.31, 10: 2.26}      # two-sided Student t, n - 1 degrees of freedom


def _pair_stats(a, b):
    """a, b: the two arms' values per pair -> mean difference b - a and its 95 % interval."""
    d = [y - x for x, y in zip(a, b)]
    n = len(d)
    mean = sum(d) / n
    if n < 2:
        return {"mean_diff": round(mean, 4), "ci95": None}
    se = (sum((v - mean) ** 2 for v in d) / (n - 1)) ** 0.5 / n ** 0.5
    h = _T95.get(n, 1.96) * se
    return {"mean_diff": round(mean, 4), "ci95": [round(mean - h, 4), round(mean + h, 4)], "excludes_zero": bool(mean + h < 0 or mean - h > 0)}


_ARMS = {"bf16": {}, "fp8": {"suffix_weights": "fp8"}, "fp4": {"suffix_mx": "fp4"}}


def _kernel_table(m, dev, modes, Ms):
    """The gemv and skinny projection kernels over the model's coded copies (`modes`: keys of infer.CODED) per projection shape of a 7B
    layer and M, as the engine launches them (the fused input forms, one launch per layer's weights in a captured graph: 32 different
    matrices, 1.6 GB in FP8, nothing stays in the caches; eager launches from Python are host-bound below ~15 us per kernel) -> us per
    launch, the cells "gemv" / "skinny" for one mode and "gemv_w8", ... for several."""
    from mla_amd import hip
    from mla_amd.infer import CODED
    copies = {CODED[mode].fmt: m.vlm.__dict__[CODED[mode].slot][mode] for mode in modes}
    fmt0, first = next(iter(copies.items()))
    names = {1: "qkv(norm)", 2: "o(res)", 4: "gate_up(norm)", 5: "down(swiglu,res)"}
    table = {}
    for M in Ms:
        row = {}
        for idx, name in names.items():
            N, K = first[0][idx].q.shape[0], first[0][idx].q.shape[1] * fmt0.k_per_col
            x = (torch.randn(M, 2 * K if idx == 5 else K, device=dev) * 0.5).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev).to(torch.bfloat16) if idx in (2, 5) else None
            o = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            pre = {"norm_weight": first[0][0], "eps": 1e-5} if idx in (1, 4) else ({"swiglu": True} if idx == 5 else {})
            cell = {}
            for fmt, layers in copies.items():
                for kname, family in (("gemv", "gemv"), ("skinny", "gemm_skinny")):
                    if kname == "gemv" and not hip.gemv_fits(M, K):
                        continue
                    fn = getattr(hip, family + fmt.suffix)
                    for L in layers[:2]:                                    # function attributes, allocator
                        fn(x, *L[idx], o, N, 0, M, res, **pre)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for L in layers:
                            fn(x, *L[idx], o, N, 0, M, res, **pre)
                    g.replay()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(3):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    cell[kname if len(copies) == 1 else f"{kname}_{fmt.name}"] = round(e0.elapsed_time(e1) / (3 * len(layers)) * 1e3, 1)
            row[name] = cell
        table[f"M{M}"] = row
    return table


def main_pair(args, mx=False):
    """--pair-fp8: bf16 / fp8 suffix weights on the host sampler at --chunk. --pair-mx: bf16 / fp8 / fp4, sampler="device", over --chunks
    and --operand. The arms alternate in rounds in one process: chunk latency and the captured suffix pass, one JSON line per case."""
    arms = ("bf16", "fp8", "fp4") if mx else ("bf16", "fp8")
    m = None
    for chunk in ([int(v) for v in args.chunks.split(",")] if mx and args.chunks else [args.chunk]):
        for operand in ((["fused"] + (["once"] if chunk > 7 else []) if args.operand == "both" else [args.operand]) if mx else [None]):
            args.chunk = chunk
            m = _pair_case(args, m, arms, {"sampler": "device", "suffix_operand": operand} if mx else {}, args.kernel_table and m is None)


def _pair_case(args, m, arms, modes, kernel_table):
    from mla_amd.infer import PrefixCachedEps
    m, b, ids = _setup(args, model=m)
    dev = ids.device
    mx = len(arms) > 2
    noise = torch.randn(1, args.chunk, 7, device=dev)
    image, pc, state = _observation(b)
    kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps, noise=noise, **modes)
    mk = dict(input_ids=ids, **{k: v for k, v in modes.items() if k != "sampler"}, **_engine_kw(b))
    acts = {arm: m.predict_action_diff(**_ARMS[arm], **kw) for arm in arms}                      # engines, graphs, packed + quantised weights
    t91 = torch.tensor([91], device=dev)

    def chunk_ms(arm):
        return _time_ms(lambda: m.predict_action_diff(**_ARMS[arm], **kw), args.iters)

    def pass_ms(arm):
        with torch.inference_mode():
            eng = PrefixCachedEps.for_inputs(m.vlm, n_action_rows=args.chunk, **_ARMS[arm], **mk)
            eng(noise, t91)
            return _replay_ms(eng)
    chunk = {arm: [] for arm in arms}
    suffix = {arm: [] for arm in arms}
    for _ in range(args.pairs):                                             # bf16, fp8[, fp4], bf16, ...: same box, interleaved
        for arm in arms:
            chunk[arm].append(chunk_ms(arm))
        for arm in arms:
            suffix[arm].append(pass_ms(arm))
    gb = {arm: _stream_bytes(m, arm) / 1e9 for arm in arms}
    against = [(arm, ref) for i, ref in enumerate(arms) for arm in arms[i + 1:]]                 # fp8 - bf16[, fp4 - bf16, fp4 - fp8]

    def rel(a, ref):
        return round(float(((acts[a] - acts[ref]) ** 2).sum() ** 0.5 / (acts[ref] ** 2).sum() ** 0.5), 4)
    metric = ("predict_action_diff, MLA-Llama2-7B, batch 1, sampler=device: bf16 vs fp8 vs fp4 (MXFP4) suffix weights in alternating rounds"
              if mx else "predict_action_diff, MLA-Llama2-7B, batch 1: bf16 vs fp8 suffix weights in alternating pairs")
    out = {"metric": metric, "action_chunk": args.chunk, "suffix_rows": args.chunk + 1, **({"suffix_operand": modes["suffix_operand"]} if mx else {}),
           "ddim_steps": args.steps, "pairs": args.pairs, "unit": "ms",
           "chunk_ms": {k: [round(v, 2) for v in vs] for k, vs in chunk.items()},
           **{f"chunk_{a}_minus_{ref}": _pair_stats(chunk[ref], chunk[a]) for a, ref in against},
           "suffix_pass_ms": {k: [round(v, 3) for v in vs] for k, vs in suffix.items()},
           **{f"suffix_pass_{a}_minus_{ref}": _pair_stats(suffix[ref], suffix[a]) for a, ref in against},
           "weights_streamed_per_pass_gb": {k: round(v, 2) for k, v in gb.items()},
           "suffix_pass_weight_stream_tbps": {k: round(gb[k] / 1e3 / (min(suffix[k]) * 1e-3), 2) for k in arms},
           **({"chunk_rel_diff_vs_bf16_random_weights": {a: rel(a, "bf16") for a in arms[1:]}} if mx else
              {"fp8_vs_bf16_chunk_rel_diff_random_weights": rel("fp8", "bf16")}),
           "data": "synthetic"}
    if kernel_table:
        out["kernel_us_per_launch" if mx else "w8_kernel_us_per_launch"] = _kernel_table(m, dev, arms[1:], (2, 5, 8, 17, 33, 64) if mx else (2, 5, 8, 17))
    print(json.dumps(out), flush=True)
    return m


def main_pair_sampler(args, ddpm=False):
    """sampler="host" vs sampler="device" on the same box, alternating, per chunk length and suffix-weight mode: predict_action_diff per
    chunk (host clock around `iters` calls that end in a device synchronise), the prefill alone (PrefixCachedEps.for_inputs: encoders +
    prefix rows, the same for both arms) and from the two the per-step share (chunk - prefill) / steps of each arm -- the suffix pass
    plus the sampler's glue, which is what the mode changes. ddpm: the same for ddpm_sampler= on use_ddim=False calls (the steps are the
    training diffusion's; both arms draw the steps' noise, the warm-up calls under the same seed)."""
    from mla_amd.infer import PrefixCachedEps
    m, b, ids = _setup()
    dev = ids.device
    image, pc, state = _observation(b)
    mk = dict(input_ids=ids, **_engine_kw(b))
    arms = ("host", "device")
    word, name = ("ddpm_sampler", "ddpm") if ddpm else ("sampler", "ddim")
    steps = m.diffusion.num_timesteps if ddpm else args.steps
    for C in ([int(v) for v in args.chunks.split(",")] if args.chunks else [1, 16]):
        m.future_action_window_size = m.vlm.future_action_window_size = C - 1
        noise = torch.randn(1, C, 7, device=dev)
        kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps, noise=noise, use_ddim=not ddpm)
        for w in ("bf16", "fp8"):
            acts = {}
            for arm in arms:                                                # engines, graphs, tables; the same seed: the same FPS start indices
                torch.manual_seed(1)
                acts[arm] = m.predict_action_diff(suffix_weights=w, **{word: arm}, **kw)
            with torch.inference_mode():
                eng = PrefixCachedEps.for_inputs(m.vlm, n_action_rows=C, suffix_weights=w, **mk)

            def chunk_ms(arm):
                return _time_ms(lambda: m.predict_action_diff(suffix_weights=w, **{word: arm}, **kw), args.iters)

            def prefill_ms():
                with torch.inference_mode():
                    return _time_ms(lambda: PrefixCachedEps.for_inputs(m.vlm, n_action_rows=C, suffix_weights=w, **mk), args.iters)
            chunk, prefill = {arm: [] for arm in arms}, []
            for _ in range(args.pairs):                                     # host, device, host, device, ...: same box, interleaved
                for arm in arms:
                    chunk[arm].append(chunk_ms(arm))
                prefill.append(prefill_ms())
            step = {arm: [(c - p) / steps for c, p in zip(chunk[arm], prefill)] for arm in arms}
            print(json.dumps({"metric": f"predict_action_diff, MLA-Llama2-7B, batch 1: {word}=host vs {word}=device in alternating pairs",
                              "action_chunk": C, "suffix_rows": C + 1, "suffix_weights": w, f"{name}_steps": steps, "pairs": args.pairs,
                              "iters_per_arm_and_pair": args.iters, "unit": "ms",
                              "chunk_ms": {k: [round(v, 2) for v in vs] for k, vs in chunk.items()},
                              "chunk_device_minus_host": _pair_stats(chunk["host"], chunk["device"]),
                              "prefill_with_encoders_ms": [round(v, 2) for v in prefill],
                              "per_step_share_ms": {k: [round(v, 3) for v in vs] for k, vs in step.items()},
                              "per_step_share_device_minus_host": _pair_stats(step["host"], step["device"]),
                              "same_bits": bool(np.array_equal(acts["host"], acts["device"])),
                              "step_captured": all(st.graph is not None for st in (eng._ddpm if ddpm else eng._ddim).values()),
                              "graph_error": eng.graph_error,
                              "data": "synthetic"}), flush=True)


def main_pair_pinned(args):
    """The un-pinned call vs the call with known_actions on the same box, alternating, per chunk length and suffix-weight mode, the
    device sampler in both arms: predict_action_diff per chunk (host clock around `iters` calls that end in a device synchronise). The
    pinned arm adds the validation and normalisation of the known rows, two small copies to the device per call and one select per
    chunk element in the update kernel (mla_ddim_step_pin on a captured step of its own)."""
    m, b, ids = _setup()
    dev = ids.device
    image, pc, state = _observation(b)
    for C in ([int(v) for v in args.chunks.split(",")] if args.chunks else [1, 16]):
        m.future_action_window_size = m.vlm.future_action_window_size = C - 1
        noise = torch.randn(1, C, 7, device=dev)
        d = min(3, C)
        known = (torch.rand(d, 7, generator=torch.Generator().manual_seed(C)) * 2 - 1).numpy()
        kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps, noise=noise)
        arms = {"plain": {}, "pinned": {"known_actions": known}}
        for w in ("bf16", "fp8"):
            acts = {}
            for arm, extra in arms.items():                                 # engines, graphs, tables; the same seed: the same FPS start indices
                torch.manual_seed(1)
                acts[arm] = m.predict_action_diff(suffix_weights=w, sampler="device", **extra, **kw)
            torch.manual_seed(1)
            host = m.predict_action_diff(suffix_weights=w, sampler="host", known_actions=known, **kw)
            chunk = {arm: [] for arm in arms}
            for _ in range(args.pairs):                                     # plain, pinned, plain, pinned, ...: same box, interleaved
                for arm, extra in arms.items():
                    chunk[arm].append(_time_ms(lambda: m.predict_action_diff(suffix_weights=w, sampler="device", **extra, **kw), args.iters))
            sent = known if m.norm_stats is None else m.unnormalize_actions(m.normalize_actions(known))
            print(json.dumps({"metric": "predict_action_diff, MLA-Llama2-7B, batch 1, sampler=device: without vs with known_actions in alternating pairs",
                              "action_chunk": C, "suffix_rows": C + 1, "pinned_steps": d, "suffix_weights": w, "ddim_steps": args.steps,
                              "pairs": args.pairs, "iters_per_arm_and_pair": args.iters, "unit": "ms",
                              "chunk_ms": {k: [round(v, 2) for v in vs] for k, vs in chunk.items()},
                              "chunk_pinned_minus_plain": _pair_stats(chunk["plain"], chunk["pinned"]),
                              "pinned_steps_max_abs_diff": float(np.abs(acts["pinned"][:d] - sent).max()),
                              "pinned_host_same_bits": bool(np.array_equal(host, acts["pinned"])),
                              "pinned_differs_from_plain": not np.array_equal(acts["pinned"], acts["plain"]),
                              "data": "synthetic"}), flush=True)


def main_pair_solver(args):
    """solver="ddim" vs solver="dpmpp2m" on the same box, alternating, per chunk length and suffix-weight mode, the device sampler in
    both arms: predict_action_diff per chunk (host clock around `iters` calls that end in a device synchronise). Two cases: "same_steps"
    -- both solvers over the --steps process (the 2M update reads and writes one more fp32 array of the chunk's size than DDIM's and
    skips DDIM's unused randn_like per step); "fewer_steps" -- dpmpp2m over --ddim-steps (default 4) against ddim over --steps. The
    two processes are two objects handed to the model per arm (the DDIM and the 2M device states are separate: neither arm
    rebuilds its state or recaptures its step when the other ran)."""
    from mla_amd.diffusion import create_diffusion
    m, b, ids = _setup()
    dev = ids.device
    image, pc, state = _observation(b)
    short = args.ddim_steps or 4
    procs = {n: create_diffusion(timestep_respacing=f"ddim{n}") for n in {args.steps, short}}
    cases = {"same_steps": {"ddim": ("ddim", args.steps), "dpmpp2m": ("dpmpp2m", args.steps)},
             "fewer_steps": {"ddim": ("ddim", args.steps), "dpmpp2m": ("dpmpp2m", short)}}
    for C in ([int(v) for v in args.chunks.split(",")] if args.chunks else [1, 16]):
        m.future_action_window_size = m.vlm.future_action_window_size = C - 1
        noise = torch.randn(1, C, 7, device=dev)
        kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, noise=noise)
        for w in ("bf16", "fp8"):
            for case, arms in cases.items():
                def call(arm, sampler="device"):
                    solver, n = arms[arm]
                    m.ddim_diffusion = procs[n]
                    return m.predict_action_diff(suffix_weights=w, sampler=sampler, solver=solver, num_ddim_steps=n, **kw)
                acts = {}
                for arm in arms:                                            # engines, graphs, tables; the same seed: the same FPS start indices
                    torch.manual_seed(1)
                    acts[arm] = call(arm)
                torch.manual_seed(1)
                host = call("dpmpp2m", sampler="host")
                chunk = {arm: [] for arm in arms}
                for _ in range(args.pairs):                                 # ddim, dpmpp2m, ddim, dpmpp2m, ...: same box, interleaved
                    for arm in arms:
                        chunk[arm].append(_time_ms(lambda: call(arm), args.iters))
                print(json.dumps({"metric": "predict_action_diff, MLA-Llama2-7B, batch 1, sampler=device: solver=ddim vs solver=dpmpp2m in alternating pairs",
                                  "case": case, "action_chunk": C, "suffix_rows": C + 1, "suffix_weights": w,
                                  "steps": {arm: n for arm, (_, n) in arms.items()}, "pairs": args.pairs, "iters_per_arm_and_pair": args.iters,
                                  "unit": "ms", "chunk_ms": {k: [round(v, 2) for v in vs] for k, vs in chunk.items()},
                                  "chunk_ms_mean": {k: round(sum(vs) / len(vs), 2) for k, vs in chunk.items()},
                                  "chunk_dpmpp2m_minus_ddim": _pair_stats(chunk["ddim"], chunk["dpmpp2m"]),
                                  "dpmpp2m_host_same_bits": bool(np.array_equal(host, acts["dpmpp2m"])),
                                  "dpmpp2m_differs_from_ddim": not np.array_equal(acts["dpmpp2m"], acts["ddim"]),
                                  "data": "synthetic"}), flush=True)


def _attn_split_table(dev, shapes=((2, 547), (17, 562)), H=32, layers=32, reps=5, rounds=3):
    """One attention launch of a sampler step at 7B head count, per form: "head" = what the engine picks today (mla_attn_decode where the
    scores fit LDS, else mla_attn_chunk), "split<s>" = mla_attn_chunk_split (both launches; one for s = 1). Every form is captured as
    `layers` launches over `layers` different caches (442 MB at S_kv 562: nothing stays in the caches), the forms alternate per round;
    microseconds per launch (pair) = replay time / layers, median over the rounds and every round's value."""
    import math
    from mla_amd import hip
    table = {}
    for R, S_kv in shapes:
        caches = [(torch.randn(1, S_kv, 3 * H * 128, device=dev) * 0.7).to(torch.bfloat16) for _ in range(layers)]
        scale = 1 / math.sqrt(128)
        nT = -(-S_kv // 64)
        plan = hip.plan_attn_split(1, H, R, S_kv)
        ws = torch.empty(max(hip.attn_split_ws_bytes(1, H, R, S_kv, nT), 16), dtype=torch.uint8, device=dev)
        head = hip.attn_decode if hip.attn_decode_fits(R, S_kv) else hip.attn_chunk
        forms = {"head": lambda c: head(c, 1, H, 128, S_kv, R, scale)}
        for s in sorted({1, 2, 3, plan.splits, nT}):
            forms[f"split{s}"] = lambda c, s=s: hip.attn_chunk_split(c, 1, H, 128, S_kv, R, scale, splits=s, ws=ws)
        graphs = {}
        for name, fn in forms.items():
            for c in caches[:2]:                                           # function attributes, allocator
                fn(c)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for c in caches:
                    fn(c)
            g.replay()
            graphs[name] = g
        us = {name: [] for name in forms}
        for _ in range(rounds):
            for name, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(round(e0.elapsed_time(e1) / (reps * layers) * 1e3, 2))
        ref = hip.attn_chunk(caches[0], 1, H, 128, S_kv, R, scale).float()
        table[f"R{R}_S{S_kv}"] = {"head_kernel": "mla_attn_decode" if head is hip.attn_decode else "mla_attn_chunk", "key_tiles": nT,
                                  "plan_splits": plan.splits, "plan_workgroups": plan.workgroups,
                                  "us_per_launch_median": {k: sorted(v)[len(v) // 2] for k, v in us.items()}, "us_per_launch_rounds": us,
                                  "max_abs_diff_vs_attn_chunk": {k: round(float((fn(caches[0]).float() - ref).abs().max()), 5)
                                                                 for k, fn in forms.items()},
                                  "cache_bytes_per_launch": S_kv * 3 * H * 128 * 2}
    return table


def main_pair_attention(args):
    """suffix_attention="head" vs "split" on the same box, alternating, per chunk length and suffix-weight mode: predict_action_diff per
    chunk with the device sampler in both arms (host clock around `iters` calls that end in a device synchronise) and the captured
    suffix pass alone (device events around 8 replays). Every figure's reference is the "head" arm of the same process."""
    dev = torch.device("cuda", 0)
    if args.kernel_table:
        print(json.dumps({"metric": "suffix attention per launch, 32 heads of 128, batch 1: head vs split forms", "unit": "us",
                          "table": _attn_split_table(dev), "data": "synthetic"}), flush=True)
    if args.pairs < 1:
        return
    from mla_amd import hip
    from mla_amd.infer import PrefixCachedEps
    m, b, ids = _setup()
    image, pc, state = _observation(b)
    mk = dict(input_ids=ids, **_engine_kw(b))
    arms = ("head", "split")
    t91 = torch.tensor([91], device=dev)
    for C in ([int(v) for v in args.chunks.split(",")] if args.chunks else [1, 16]):
        m.future_action_window_size = m.vlm.future_action_window_size = C - 1
        noise = torch.randn(1, C, 7, device=dev)
        kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps, noise=noise, sampler="device")
        for w in ("bf16", "fp8"):
            acts = {}
            for arm in arms:                                                # engines, graphs, tables; the same seed: the same FPS start indices
                torch.manual_seed(1)
                acts[arm] = m.predict_action_diff(suffix_weights=w, suffix_attention=arm, **kw)

            def chunk_ms(arm):
                return _time_ms(lambda: m.predict_action_diff(suffix_weights=w, suffix_attention=arm, **kw), args.iters)

            def pass_ms(arm):
                with torch.inference_mode():
                    eng = PrefixCachedEps.for_inputs(m.vlm, n_action_rows=C, suffix_weights=w, suffix_attention=arm, **mk)
                    eng(noise, t91)
                    return _replay_ms(eng), eng
            chunk, suffix = {arm: [] for arm in arms}, {arm: [] for arm in arms}
            for _ in range(args.pairs):                                     # head, split, head, split, ...: same box, interleaved
                for arm in arms:
                    chunk[arm].append(chunk_ms(arm))
                for arm in arms:
                    suffix[arm].append(pass_ms(arm)[0])
            eng = pass_ms("split")[1]
            plan = hip.plan_attn_split(1, eng.nheads, eng.R, eng.S_cap)
            print(json.dumps({"metric": "predict_action_diff, MLA-Llama2-7B, batch 1: suffix_attention=head vs split in alternating pairs",
                              "action_chunk": C, "suffix_rows": C + 1, "suffix_weights": w, "sampler": "device", "ddim_steps": args.steps,
                              "pairs": args.pairs, "iters_per_arm_and_pair": args.iters, "unit": "ms", "S_kv": eng.S_cap,
                              "plan_splits": plan.splits, "plan_workgroups": plan.workgroups,
                              "chunk_ms": {k: [round(v, 2) for v in vs] for k, vs in chunk.items()},
                              "chunk_split_minus_head": _pair_stats(chunk["head"], chunk["split"]),
                              "suffix_pass_ms": {k: [round(v, 3) for v in vs] for k, vs in suffix.items()},
                              "suffix_pass_split_minus_head": _pair_stats(suffix["head"], suffix["split"]),
                              "split_vs_head_chunk_rel_diff_random_weights":
                                  round(float(((acts["split"] - acts["head"]) ** 2).sum() ** 0.5 / (acts["head"] ** 2).sum() ** 0.5), 5),
                              "pass_captured": eng.graph is not None, "graph_error": eng.graph_error, "data": "synthetic"}), flush=True)


def _operand_kernel_table(dev, Ms=(9, 17, 33, 64), H=4096, I=11008, copies=8, reps=5, rounds=3):
    """The suffix projections of a 7B layer at M rows, per form, bf16 and W8 (e4m3fn codes of the same weights): "fused" = what
    suffix_operand="fused" launches (RMSNorm / SwiGLU in the input staging: mla_gemm_skinny_* pre 1 / 2), "plain" = the same projection
    on a ready operand (pre 0), and for gate|up "swiglu_epilogue" = mla_gemm_skinny_gateup_swiglu_* against "plain+swiglu_fwd" (two
    launches, the packed rows through memory). Every form is captured as `copies` launches over `copies` different weight matrices (at
    least 268 MB per graph: nothing stays in the caches), the forms alternate per round; microseconds per launch (sequence) = replay
    time / copies: the median over the rounds and every round's value. Yields one row per (format, projection, M)."""
    from mla_amd import hip
    bf16 = torch.bfloat16
    ln = torch.ones(H, dtype=bf16, device=dev)
    shapes = (("qkv", 3 * H, H, "norm"), ("gate_up", 2 * I, H, "norm"), ("down", H, I, "swiglu"))
    for fmt in ("bf16", "w8"):
        for name, N, K, pre in shapes:
            Ws = [(torch.randn(N, K, device=dev) * 0.02).to(bf16) for _ in range(copies)]
            if fmt == "w8":
                Ws = [hip.quant_fp8_rows(W) for W in Ws]
            for M in Ms:
                x = (torch.randn(M, K, device=dev) * 0.5).to(bf16)
                x_pre = (torch.randn(M, 2 * K, device=dev) * 0.5).to(bf16) if pre == "swiglu" else x        # the fused form's input
                res = torch.randn(M, N, device=dev).to(bf16) if name == "down" else None
                out = torch.empty(M, N, dtype=bf16, device=dev)
                kw = {"norm_weight": ln, "eps": 1e-5} if pre == "norm" else {"swiglu": True}

                def gemm(xx, W, **k):
                    if fmt == "w8":
                        hip.gemm_skinny_w8(xx, W[0], W[1], out, N, 0, M, res, **k)
                    else:
                        hip.gemm_skinny(xx, W, out, N, 0, M, res, **k)
                forms = {"fused": lambda W: gemm(x_pre, W, **kw), "plain": lambda W: gemm(x, W)}
                if name == "gate_up":
                    act = torch.empty(M, I, dtype=bf16, device=dev)
                    forms["plain+swiglu_fwd"] = lambda W: (gemm(x, W), hip.swiglu_fwd(out))
                    forms["swiglu_epilogue"] = (lambda W: hip.gemm_skinny_gateup_swiglu_w8(x, W[0], W[1], out=act)) if fmt == "w8" else \
                        (lambda W: hip.gemm_skinny_gateup_swiglu(x, W, out=act))
                graphs = {}
                for form, fn in forms.items():
                    for W in Ws[:2]:                                        # function attributes, allocator
                        fn(W)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for W in Ws:
                            fn(W)
                    g.replay()
                    graphs[form] = g
                us = {form: [] for form in forms}
                for _ in range(rounds):
                    for form, g in graphs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            g.replay()
                        e1.record()
                        torch.cuda.synchronize()
                        us[form].append(round(e0.elapsed_time(e1) / (reps * copies) * 1e3, 2))
                med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
                wbytes = N * K * (1 if fmt == "w8" else 2)
                yield {"weights": fmt, "projection": name, "N": N, "K": K, "M": M, "weight_bytes": wbytes, "us_per_launch_median": med,
                       "weight_stream_tbps": {k: round(wbytes / 1e12 / (v * 1e-6), 2) for k, v in med.items()}, "us_per_launch_rounds": us}
                del graphs
            del Ws
            torch.cuda.empty_cache()


def main_pair_operand(args):
    """suffix_operand="fused" vs "once" on the same box, alternating, per chunk length and suffix-weight mode: predict_action_diff per
    chunk with the device sampler in both arms (host clock around `iters` calls that end in a device synchronise) and the captured
    suffix pass alone (device events around 8 replays). Every figure's reference is the "fused" arm of the same process. The two arms
    compute the same bits (asserted); at chunk 1 they launch the same pass."""
    dev = torch.device("cuda", 0)
    if args.kernel_table:
        for row in _operand_kernel_table(dev):
            print(json.dumps({"metric": "suffix projection per launch at 7B layer shapes: fused vs plain operand forms", "unit": "us", **row,
                              "data": "synthetic"}), flush=True)
    if args.pairs < 1:
        return
    from mla_amd.infer import PrefixCachedEps
    m, b, ids = _setup()
    image, pc, state = _observation(b)
    mk = dict(input_ids=ids, **_engine_kw(b))
    arms = ("fused", "once")
    t91 = torch.tensor([91], device=dev)
    for C in ([int(v) for v in args.chunks.split(",")] if args.chunks else [1, 8, 16]):
        m.future_action_window_size = m.vlm.future_action_window_size = C - 1
        noise = torch.randn(1, C, 7, device=dev)
        kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps, noise=noise, sampler="device")
        for w in ("bf16", "fp8"):
            acts = {}
            for arm in arms:                                                # engines, graphs, tables; the same seed: the same FPS start indices
                torch.manual_seed(1)
                acts[arm] = m.predict_action_diff(suffix_weights=w, suffix_operand=arm, **kw)
            assert np.array_equal(acts["fused"], acts["once"]), "suffix_operand=\"once\" must return the bits of \"fused\""

            def chunk_ms(arm):
                return _time_ms(lambda: m.predict_action_diff(suffix_weights=w, suffix_operand=arm, **kw), args.iters)

            def pass_ms(arm):
                with torch.inference_mode():
                    eng = PrefixCachedEps.for_inputs(m.vlm, n_action_rows=C, suffix_weights=w, suffix_operand=arm, **mk)
                    eng(noise, t91)
                    return _replay_ms(eng), eng
            chunk, suffix = {arm: [] for arm in arms}, {arm: [] for arm in arms}
            for _ in range(args.pairs):                                     # fused, once, fused, once, ...: same box, interleaved
                for arm in arms:
                    chunk[arm].append(chunk_ms(arm))
                for arm in arms:
                    suffix[arm].append(pass_ms(arm)[0])
            eng = pass_ms("once")[1]
            print(json.dumps({"metric": "predict_action_diff, MLA-Llama2-7B, batch 1: suffix_operand=fused vs once in alternating pairs",
                              "action_chunk": C, "suffix_rows": C + 1, "suffix_weights": w, "sampler": "device", "ddim_steps": args.steps,
                              "pairs": args.pairs, "iters_per_arm_and_pair": args.iters, "unit": "ms",
                              "chunk_ms": {k: [round(v, 2) for v in vs] for k, vs in chunk.items()},
                              "chunk_once_minus_fused": _pair_stats(chunk["fused"], chunk["once"]),
                              "suffix_pass_ms": {k: [round(v, 3) for v in vs] for k, vs in suffix.items()},
                              "suffix_pass_once_minus_fused": _pair_stats(suffix["fused"], suffix["once"]),
                              "weights_streamed_per_pass_gb": round(_stream_bytes(m, w) / 1e9, 2),
                              "suffix_pass_weight_stream_tbps": {k: round(_stream_bytes(m, w) / 1e12 / (min(v) * 1e-3), 2) for k, v in suffix.items()},
                              "same_bits": True, "pass_captured": eng.graph is not None, "graph_error": eng.graph_error,
                              "data": "synthetic"}), flush=True)


def _groups_split_table(dev, cases, H=32, S_p=545, layers=32, reps=5, rounds=3):
    """One attention launch of a multi-row sampler step at 7B head count, per form, for every (B, G, R) of `cases`: "head" = the engine's
    launch today (mla_attn_chunk_groups for B = 1, mla_attn_chunk_ragged for G = 1, else mla_attn_chunk_ragged_groups), "split<s>" =
    mla_attn_groups_split (both launches; s = 1 is the head form). Prefixes of S_p rows (B > 1: S_p - 3 b). As _attn_split_table:
    `layers` launches over `layers` caches per graph, forms alternating per round, microseconds per launch (pair)."""
    import math
    from mla_amd import hip
    table, scale = {}, 1 / math.sqrt(128)
    for B, G, R in cases:
        ragged = B > 1
        S_cap = -(-(S_p + G * R) // 64) * 64
        shape = (B, S_cap, 3 * H * 128) if ragged else (S_p + G * R, 3 * H * 128)
        caches = [(torch.randn(*shape, device=dev) * 0.7).to(torch.bfloat16) for _ in range(layers)]
        prefix = torch.tensor([S_p - 3 * b for b in range(B)], dtype=torch.int32, device=dev) if ragged else S_p
        S_max, plan = hip.attn_groups_split_plan(B, G, H, R, S_cap if ragged else S_p, ragged)
        counts = sorted({1, 2, 3, plan[0]})
        ws = torch.empty(max(hip.attn_split_ws_bytes(B * G, H, R, S_max, max(counts)), 16), dtype=torch.uint8, device=dev)
        if not ragged:
            forms = {"head": lambda c: hip.attn_chunk_groups(c, G, H, 128, S_p, R, scale)}
        elif G == 1:
            kv_len = prefix + R
            forms = {"head": lambda c: hip.attn_chunk_ragged(c, B, H, 128, kv_len, R, scale)}
        else:
            forms = {"head": lambda c: hip.attn_chunk_ragged_groups(c, B, G, H, 128, prefix, R, scale)}
        for s in counts:
            forms[f"split{s}"] = lambda c, s=s: hip.attn_groups_split(c, B, G, H, 128, prefix, R, scale, splits=s, ws=ws)
        graphs = {}
        for name, fn in forms.items():
            for c in caches[:2]:                                           # function attributes, allocator
                fn(c)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for c in caches:
                    fn(c)
            g.replay()
            graphs[name] = g
        us = {name: [] for name in forms}
        for _ in range(rounds):
            for name, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(round(e0.elapsed_time(e1) / (reps * layers) * 1e3, 2))
        ref = forms["head"](caches[0]).float()
        table[f"B{B}_G{G}_R{R}"] = {"key_tiles": -(-S_max // 64), "plan_splits": plan[0], "plan_workgroups": plan[2],
                                    "head_workgroups": B * G * H * -(-R // 16),
                                    "us_per_launch_median": {k: sorted(v)[len(v) // 2] for k, v in us.items()}, "us_per_launch_rounds": us,
                                    "max_abs_diff_vs_head": {k: round(float((fn(caches[0]).float() - ref).abs().max()), 5)
                                                             for k, fn in forms.items()}}
        del caches, graphs
        torch.cuda.empty_cache()
    return table


def main_pair_groups_attention(args, batches):
    """groups_attention="head" vs "split" on the multi-row routes, on the same box, alternating: --samples N
    (predict_action_diff_samples), --batch B (predict_action_diff_batch; the fp8 arm goes through num_samples=1, the route that serves
    FP8 weights for B >= 2) and --batch B --samples N (the lists paired element-wise), for every chunk length (default: --chunk) with
    bf16 and with fp8 suffix weights, the device sampler in both arms: per-call latency (host clock around `iters` calls that end in a
    device synchronise) and the captured suffix pass alone (device events around 8 replays of the engine the call left prefilled).
    Every figure's reference is the "head" arm of the same process."""
    dev = torch.device("cuda", 0)
    Ns = [int(v) for v in args.samples.split(",")] if args.samples else []
    if batches == [0]:
        cases = [(1, n) for n in Ns]
    else:
        if Ns and len(Ns) != len(batches):
            raise SystemExit("--batch B[,B..] and --samples N[,N..] are paired element-wise: give as many of one as of the other")
        cases = list(zip(batches, Ns if Ns else [None] * len(batches)))
    chunks = [int(v) for v in args.chunks.split(",")] if args.chunks else [args.chunk]
    if args.kernel_table:
        shapes = [(B, N or 1, C + 1) for C in chunks for B, N in cases]
        print(json.dumps({"metric": "multi-row suffix attention per launch, 32 heads of 128, prefixes of 545 rows: head vs split forms",
                          "unit": "us", "table": _groups_split_table(dev, shapes), "data": "synthetic"}), flush=True)
    if args.pairs < 1:
        return
    arms, m = ("head", "split"), None
    stores = ("_prefix_engines_samples", "_prefix_engines_batched", "_prefix_engines_batch_samples")
    for C in chunks:
        for B, N in cases:
            m, b, ids = _setup(C, B, model=m)
            images, pcs, states = (list(v) for v in zip(*(_observation(b, i) for i in range(B))))
            for w in ("bf16", "fp8"):
                if B == 1:
                    route, store = "predict_action_diff_samples", stores[0]
                    noise = torch.randn(N, C, 7, device=dev)

                    def call(arm):
                        return m.predict_action_diff_samples(images[0], pcs[0], cur_robot_state=states[0], num_samples=N, input_ids=ids,
                                                             noise=noise, num_ddim_steps=args.steps, suffix_weights=w, sampler="device",
                                                             groups_attention=arm)
                else:
                    n = N if N is not None else (1 if w == "fp8" else None)
                    route, store = ("predict_action_diff_batch", stores[1]) if n is None else (f"predict_action_diff_batch(num_samples={n})", stores[2])
                    noise = torch.randn(*((B, C, 7) if n is None else (B, n, C, 7)), device=dev)

                    def call(arm):
                        return m.predict_action_diff_batch(images, pcs, cur_robot_states=states, input_ids=list(ids), noise=noise,
                                                           num_ddim_steps=args.steps, suffix_weights=w, sampler="device", num_samples=n,
                                                           groups_attention=arm)

                def engine(arm):
                    eng, = [e for e in m.vlm.__dict__[store].values() if e.suffix_attention == arm and e.suffix_weights == w]
                    return eng
                acts = {}
                for arm in arms:                                            # engines, graphs, tables; the same seed: the same FPS start indices
                    torch.manual_seed(1)
                    acts[arm] = call(arm)
                ms, suffix = {arm: [] for arm in arms}, {arm: [] for arm in arms}
                for _ in range(args.pairs):                                 # head, split, head, split, ...: same box, interleaved
                    for arm in arms:
                        ms[arm].append(_time_ms(lambda: call(arm), args.iters))
                    for arm in arms:
                        with torch.inference_mode():
                            suffix[arm].append(_replay_ms(engine(arm)))
                eng = engine("split")
                S_max, plan = eng.attn_plan
                print(json.dumps({"metric": f"{route}, MLA-Llama2-7B: groups_attention=head vs split in alternating pairs", "batch": B,
                                  "samples": N, "action_chunk": C, "suffix_rows": eng.h_in.shape[0], "suffix_weights": w, "sampler": "device",
                                  "ddim_steps": args.steps, "pairs": args.pairs, "iters_per_arm_and_pair": args.iters, "unit": "ms",
                                  "S_max": S_max, "plan_splits": plan[0], "plan_workgroups": plan[2],
                                  "call_ms": {k: [round(v, 2) for v in vs] for k, vs in ms.items()},
                                  "call_split_minus_head": _pair_stats(ms["head"], ms["split"]),
                                  "suffix_pass_ms": {k: [round(v, 3) for v in vs] for k, vs in suffix.items()},
                                  "suffix_pass_split_minus_head": _pair_stats(suffix["head"], suffix["split"]),
                                  "split_vs_head_rel_diff_random_weights":
                                      round(float(((acts["split"] - acts["head"]) ** 2).sum() ** 0.5 / (acts["head"] ** 2).sum() ** 0.5), 5),
                                  "pass_captured": eng.graph is not None, "graph_error": eng.graph_error, "data": "synthetic"}), flush=True)
                for s in stores:                                            # the caches of this (B, N, C, weights)
                    m.vlm.__dict__.get(s, {}).clear()
                torch.cuda.empty_cache()


def main_pair_prefill(args):
    """prefill="train" vs prefill="compact" vs prefill="compact" with prefill_precision="fp8" (arm "fp8") on the same box, alternating:
    (a) predict_action_diff per chunk with bf16 and with fp8 suffix weights, (b) engine.prefill() = encoders + the decoder rows of the
    prefix, (c) the decoder rows alone on given prefix rows. The chunks of one suffix_weights mode are measured before the other's: three
    engines at a time (a model keeps four)."""
    from mla_amd import hip, ops
    from mla_amd.infer import PrefixCachedEps
    m, b, ids = _setup(args)
    dev = ids.device
    noise = torch.randn(1, args.chunk, 7, device=dev)
    image, pc, state = _observation(b)
    kw = dict(image=image, pointcloud=pc, cur_robot_state=state, input_ids=ids, num_ddim_steps=args.steps, noise=noise)
    mk = dict(input_ids=ids, **_engine_kw(b))
    arms = {"train": dict(prefill="train"), "compact": dict(prefill="compact"), "fp8": dict(prefill="compact", prefill_precision="fp8")}
    modes, weights = tuple(arms), ("bf16", "fp8")
    k = PrefixCachedEps._splice_position(ids)
    with torch.inference_mode():
        eng = {mode: PrefixCachedEps.for_inputs(m.vlm, n_action_rows=args.chunk, **arms[mode], **mk) for mode in modes}
        prefix = eng["train"]._prefix_rows(ids, k, mk["images"], mk["point_cloud"], mk["camera_name"], mk["proprio"])
    S_p, H = eng["train"].S_p, eng["train"].H

    def chunk_ms(w, mode):
        return _time_ms(lambda: m.predict_action_diff(suffix_weights=w, **arms[mode], **kw), args.iters)

    def timed(fn, reps=3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.inference_mode():
            fn()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def layers_only(mode):
        e = eng[mode]
        h = prefix.reshape(S_p, H)
        if mode != "train":
            return lambda: e._compact_prefill(h, 1, S_p, e.cache, e.cache[0].stride(0))

        def train():
            x = h
            for w, c in zip(e._weights(), e.cache):
                x, a = ops.DecoderLayerFn._fwd(x, None, e.cos_p, e.sin_p, 1, S_p, e.nheads, e.eps, w)
                c[:, :S_p].copy_(a.qkv[:S_p].view(1, S_p, 3 * H))
        return train
    chunk = {(w, mode): [] for w in weights for mode in modes}
    prefill = {mode: [] for mode in modes}
    layers = {mode: [] for mode in modes}
    acts = {}
    for w in weights:                                                       # train, compact, fp8, train, ...: same box, interleaved
        for mode in modes:
            acts[(w, mode)] = m.predict_action_diff(suffix_weights=w, **arms[mode], **kw)     # engines, graphs
        for _ in range(args.pairs):
            for mode in modes:
                chunk[(w, mode)].append(chunk_ms(w, mode))
    for _ in range(args.pairs):
        for mode in modes:
            prefill[mode].append(timed(lambda: eng[mode].prefill(ids, k, **{a: v for a, v in mk.items() if a != "input_ids"})))
        for mode in modes:
            layers[mode].append(timed(layers_only(mode)))
    rel = lambda a, b: round(float(((a - b) ** 2).sum() ** 0.5 / (b ** 2).sum() ** 0.5), 4)
    diffs = (("compact", "train"), ("fp8", "compact"), ("fp8", "train"))
    out = {"metric": "predict_action_diff, MLA-Llama2-7B, batch 1: prefill=train vs prefill=compact vs prefill=compact + "
                     "prefill_precision=fp8 (arm \"fp8\") in alternating order",
           "action_chunk": args.chunk, "prefix_rows": S_p, "ddim_steps": args.steps, "pairs": args.pairs, "unit": "ms",
           "chunk_ms": {f"{w}/{mode}": [round(v, 2) for v in vs] for (w, mode), vs in chunk.items()},
           **{f"chunk_{b}_minus_{a}": {w: _pair_stats(chunk[(w, a)], chunk[(w, b)]) for w in weights} for b, a in diffs},
           "prefill_with_encoders_ms": {mode: [round(v, 2) for v in vs] for mode, vs in prefill.items()},
           **{f"prefill_with_encoders_{b}_minus_{a}": _pair_stats(prefill[a], prefill[b]) for b, a in diffs},
           "decoder_rows_only_ms": {mode: [round(v, 2) for v in vs] for mode, vs in layers.items()},
           **{f"decoder_rows_only_{b}_minus_{a}": _pair_stats(layers[a], layers[b]) for b, a in diffs},
           "compact_vs_train_chunk_rel_diff_random_weights": {w: rel(acts[(w, "compact")], acts[(w, "train")]) for w in weights},
           "fp8_vs_compact_chunk_rel_diff_random_weights": {w: rel(acts[(w, "fp8")], acts[(w, "compact")]) for w in weights},
           "data": "synthetic"}
    if args.kernel_table:
        # the four projections of a layer at the prefix's row count, cycling through the 32 layers' weights (nothing stays in the caches),
        # captured into a graph as a run of launches: training kernel vs compact kernel, us per launch
        packed = eng["train"]._weights()
        packed8 = eng["fp8"]._prefill_layers()                                  # per layer (ln1, W8 qkv, W8 o, ln2, W8 gate|up, W8 down)
        ws, ws8 = eng["compact"]._prefill_ws, eng["fp8"]._prefill_ws
        I = packed[0][6].shape[0]
        xh = (torch.randn(S_p, H, device=dev) * 0.5).to(torch.bfloat16)
        xi = (torch.randn(S_p, I, device=dev) * 0.5).to(torch.bfloat16)
        res = torch.randn(S_p, H, device=dev).to(torch.bfloat16)
        qkv = torch.empty(S_p, 3 * H, dtype=torch.bfloat16, device=dev)
        oh = torch.empty(S_p, H, dtype=torch.bfloat16, device=dev)
        act = torch.empty(S_p, I, dtype=torch.bfloat16, device=dev)
        cos, sin = eng["train"].cos_p, eng["train"].sin_p
        (xh8, xhs), (xi8, xis) = hip.quant_fp8_rows(xh), hip.quant_fp8_rows(xi)
        # per form: training kernel, compact kernel (both on the packed bf16 layer L), FP8 compact kernel on the layer's W8 tuple, and
        # the activation quantiser the FP8 launch needs in front of it (mla_quant_fp8_rows on the projection's input rows)
        forms = {
            "qkv_rope": (lambda L: hip.gemm_qkv_rope(xh, ops.cat_view(L[1:4]), qkv, cos, sin, S_p, 2 * H),
                         lambda L: hip.gemm_prefill_qkv_rope(xh, ops.cat_view(L[1:4]), qkv, 3 * H, 0, S_p, (cos, sin, 2 * H), 128, ws=ws),
                         lambda L: hip.gemm_prefill_f8_qkv_rope(xh8, xhs, L[1].q, L[1].scale, qkv, 3 * H, 0, S_p, (cos, sin, 2 * H), 128,
                                                                ws=ws8),
                         lambda L: hip.quant_fp8_rows(xh, xh8, xhs)),
            "o_res": (lambda L: hip.gemm(xh, L[4], oh, residual=res),
                      lambda L: hip.gemm_prefill(xh, L[4], oh, H, 0, S_p, residual=res, ws=ws),
                      lambda L: hip.gemm_prefill_f8(xh8, xhs, L[2].q, L[2].scale, oh, H, 0, S_p, residual=res, ws=ws8),
                      lambda L: hip.quant_fp8_rows(xh, xh8, xhs)),
            "gateup_swiglu": (lambda L: hip.gemm_gateup_swiglu(xh, ops.cat_view(L[6:8]), False),
                              lambda L: hip.gemm_prefill_gateup_swiglu(xh, ops.cat_view(L[6:8]), act, ws=ws),
                              lambda L: hip.gemm_prefill_f8_gateup_swiglu(xh8, xhs, L[4].q, L[4].scale, act, ws=ws8),
                              lambda L: hip.quant_fp8_rows(xh, xh8, xhs)),
            "down_res": (lambda L: hip.gemm(xi, L[8], oh, residual=res),
                         lambda L: hip.gemm_prefill(xi, L[8], oh, H, 0, S_p, residual=res, ws=ws),
                         lambda L: hip.gemm_prefill_f8(xi8, xis, L[5].q, L[5].scale, oh, H, 0, S_p, residual=res, ws=ws8),
                         lambda L: hip.quant_fp8_rows(xi, xi8, xis)),
        }
        table = {}
        for name, fns in forms.items():
            cell = {}
            for kname, fn in zip(("train", "compact", "fp8", "fp8_input_quantiser"), fns):
                layers_w = packed8 if kname == "fp8" else packed
                for L in layers_w[:2]:
                    fn(L)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for L in layers_w:
                        fn(L)
                g.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                cell[kname] = round(e0.elapsed_time(e1) / (3 * len(packed)) * 1e3, 1)
            N, K = {"qkv_rope": (3 * H, H), "o_res": (H, H), "gateup_swiglu": (2 * I, H), "down_res": (H, I)}[name]
            p = hip.plan_gemm_prefill(S_p, N, K)
            cell["compact_plan"] = {"split": p.split, "workgroups": p.workgroups}
            p8 = hip.plan_gemm_prefill_f8(S_p, N, K)
            cell["fp8_plan"] = {"split": p8.split, "workgroups": p8.workgroups}
            cell["fp8_tflops"] = round(2.0 * S_p * N * K / (cell["fp8"] * 1e-6) / 1e12, 1)
            cell["compact_tflops"] = round(2.0 * S_p * N * K / (cell["compact"] * 1e-6) / 1e12, 1)
            cell["train_tflops"] = round(2.0 * S_p * N * K / (cell["train"] * 1e-6) / 1e12, 1)
            table[name] = cell
        out["projection_us_per_launch"] = table
    print(json.dumps(out))


def _attn_groups_table(dev, Ns, chunks, H=32, S_p=545, layers=32, reps=5, rounds=3):
    """mla_attn_chunk_groups alone at the 7B shapes (32 heads, 545 prefix rows), gw = 1 / 2 / 4 groups per workgroup x both work orders, against
    mla_attn_chunk_ragged on N copies of the prefix. As the engines launch them: one launch per layer on that layer's own cache (32
    caches: nothing of a layer's prefix is left in the caches when its turn comes again), captured into a graph; the arms alternate and
    every arm is measured `rounds` times. us per launch, the minimum and all rounds. Algorithmic bytes: the prefix K and V once plus
    every group's rows for the groups kernel, N copies of everything for the ragged one."""
    import math
    from mla_amd import hip
    scale = 1 / math.sqrt(128)
    table = {}
    for chunk in chunks:
        R = chunk + 1
        for N in Ns:
            rows = S_p + N * R
            shared = [(torch.randn(rows, 3 * H * 128, device=dev) * 0.7).to(torch.bfloat16) for _ in range(layers)]
            copies = [(torch.randn(N, S_p + R, 3 * H * 128, device=dev) * 0.7).to(torch.bfloat16) for _ in range(layers)]
            kv_len = torch.full((N,), S_p + R, dtype=torch.int32, device=dev)
            arms = {"ragged_N_copies": lambda c=copies: [hip.attn_chunk_ragged(x, N, H, 128, kv_len, R, scale) for x in c]}
            for gw in (1, 2, 4):                                            # order 0: head-major work items as dispatched, 1: one chunk per XCD
                for order in (0, 1):
                    arms[f"groups_gw{gw}_order{order}"] = lambda gw=gw, order=order, c=shared: [
                        hip.attn_chunk_groups(x, N, H, 128, S_p, R, scale, gw=gw, order=order) for x in c]
            graphs = {}
            for name, fn in arms.items():
                fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep = fn()
                g.replay()
                graphs[name] = (g, keep)
            us = {name: [] for name in arms}
            for _ in range(rounds):
                for name, (g, _) in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    us[name].append(round(e0.elapsed_time(e1) / (reps * layers) * 1e3, 1))
            kv_row = 2 * H * 128 * 2                                        # K and V bytes of one cache row, all heads
            table[f"chunk{chunk}_N{N}"] = {"us_per_launch_min": {k: min(v) for k, v in us.items()}, "us_per_launch_rounds": us,
                                           "algorithmic_kv_mb": {"groups": round((S_p + N * R) * kv_row / 1e6, 2),
                                                                 "ragged_N_copies": round(N * (S_p + R) * kv_row / 1e6, 2)}}
            del graphs, shared, copies
            torch.cuda.empty_cache()
    return table


def main_samples(args):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    Ns = [int(v) for v in args.samples.split(",")]
    chunks = [int(v) for v in args.chunks.split(",")] if args.chunks else [args.chunk]
    if args.kernel_table:
        print(json.dumps({"metric": "mla_attn_chunk_groups vs mla_attn_chunk_ragged on N copies, 32 heads, S_p 545, one launch per layer cache",
                          "unit": "us", "table": _attn_groups_table(dev, Ns, chunks), "data": "synthetic"}), flush=True)
    m, b, ids = _setup()
    image, pc, state = _observation(b)
    for chunk in chunks:
        m.future_action_window_size = m.vlm.future_action_window_size = chunk - 1
        for N in Ns:
            noise = torch.randn(N, chunk, 7, device=dev)
            forms = {
                "a_samples": lambda: m.predict_action_diff_samples(image, pc, cur_robot_state=state, num_samples=N, input_ids=ids, noise=noise,
                                                                   num_ddim_steps=args.steps),
                "b_batch_of_copies": lambda: m.predict_action_diff_batch([image] * N, [pc] * N, cur_robot_states=[state] * N,
                                                                         input_ids=[ids[0]] * N, noise=noise, num_ddim_steps=args.steps),
                "c_sequential": lambda: np.stack([m.predict_action_diff(image, pc, cur_robot_state=state, input_ids=ids, noise=noise[n:n + 1],
                                                                        num_ddim_steps=args.steps) for n in range(N)])}
            outs = {k: fn() for k, fn in forms.items()}                       # engines, graphs, packed weights
            ms = {k: [] for k in forms}
            for _ in range(args.pairs):                                       # a, b, c, a, b, c, ...: same box, interleaved
                for k, fn in forms.items():
                    ms[k].append(_time_ms(fn, args.iters))
            rel = lambda x, y: round(float(((x - y) ** 2).sum() ** 0.5 / (y ** 2).sum() ** 0.5), 5)  # noqa: E731
            eng = next(iter(m.vlm.__dict__.get("_prefix_engines_samples", {}).values()), None)
            print(json.dumps({"metric": "N action chunks for one observation, MLA-Llama2-7B bf16: (a) predict_action_diff_samples, (b) "
                                        "predict_action_diff_batch on N copies, (c) N sequential predict_action_diff calls; alternating",
                              "samples": N, "action_chunk": chunk, "suffix_rows": N * (chunk + 1), "ddim_steps": args.steps, "pairs": args.pairs,
                              "iters_per_timing": args.iters, "unit": "ms", "ms": {k: [round(v, 1) for v in vs] for k, vs in ms.items()},
                              "min_ms": {k: round(min(vs), 1) for k, vs in ms.items()},
                              "a_minus_b": _pair_stats(ms["b_batch_of_copies"], ms["a_samples"]),
                              "a_minus_c": _pair_stats(ms["c_sequential"], ms["a_samples"]),
                              "speedup_vs_b": round(min(ms["b_batch_of_copies"]) / min(ms["a_samples"]), 2),
                              "speedup_vs_c": round(min(ms["c_sequential"]) / min(ms["a_samples"]), 2),
                              "a_vs_c_rel_diff_random_weights": rel(outs["a_samples"], outs["c_sequential"]),
                              "a_vs_b_rel_diff_random_weights": rel(outs["a_samples"], outs["b_batch_of_copies"]),
                              "samples_engine_graph": bool(eng is not None and eng.graph is not None), "data": "synthetic"}), flush=True)
            for store in ("_prefix_engines_samples", "_prefix_engines_batched"):   # the caches of this (N, chunk): 6.5 GB at N = 15 for (b)
                m.vlm.__dict__.get(store, {}).clear()
            torch.cuda.empty_cache()


def _suffix_kernel_table(m, dev, Ms=(34, 68, 136, 255), rounds=3, reps=3):
    """mla_gemm_suffix_w8 against mla_gemm_suffix_bf16 per projection shape of a 7B layer (plain input, as SampleGroupsEps launches them),
    cycling through the 32 layers' weights (nothing stays in the caches), captured into a graph; the arms alternate, us per launch, the
    minimum over `rounds`."""
    from mla_amd import hip, ops
    assert "_prefix_fp8" in m.vlm.__dict__ and "_prefix_packed" in m.vlm.__dict__, "call the model with \"bf16\" and \"fp8\" first: they build the copies"
    fp8 = m.vlm.__dict__["_prefix_fp8"]["fp8"]
    packed = m.vlm.__dict__["_prefix_packed"]["packed"]
    bf16 = [(ops.cat_view(w[1:4]), w[4], ops.cat_view(w[6:8]), w[8]) for w in packed]
    names = ("qkv", "o(res)", "gate_up", "down(res)")
    table = {}
    for M in Ms:
        row = {}
        for i, (name, idx) in enumerate(zip(names, (1, 2, 4, 5))):
            N, K = fp8[0][idx].q.shape
            x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev).to(torch.bfloat16) if "res" in name else None
            o = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            arms = {"bf16": lambda: [hip.gemm_suffix(x, L[i], o, N, 0, M, res) for L in bf16],
                    "w8": lambda: [hip.gemm_suffix_w8(x, L[idx].q, L[idx].scale, o, N, 0, M, res) for L in fp8]}
            graphs = {}
            for k, fn in arms.items():
                fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                g.replay()
                graphs[k] = g
            us = {k: [] for k in arms}
            for _ in range(rounds):
                for k, g in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _rep in range(reps):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    us[k].append(e0.elapsed_time(e1) / (reps * len(fp8)) * 1e3)
            row[name] = {k: round(min(v), 1) for k, v in us.items()}
        table[f"M{M}"] = row
    return table


def main_samples_pair(args):
    from mla_amd.infer import SampleGroupsEps
    Ns = [int(v) for v in args.samples.split(",")]
    chunks = [int(v) for v in args.chunks.split(",")] if args.chunks else [args.chunk]
    m, b, ids = _setup()
    dev = ids.device
    image, pc, state = _observation(b)
    mk = _engine_kw(b)
    modes = ("bf16", "fp8")
    table_done = not args.kernel_table
    for chunk in chunks:
        m.future_action_window_size = m.vlm.future_action_window_size = chunk - 1
        for N in Ns:
            noise = torch.randn(N, chunk, 7, device=dev)
            t91 = torch.full((N,), 91, device=dev)

            def call(mode):
                return m.predict_action_diff_samples(image, pc, cur_robot_state=state, num_samples=N, input_ids=ids, noise=noise,
                                                     num_ddim_steps=args.steps, suffix_weights=mode)

            def call_ms(mode):
                return _time_ms(lambda: call(mode), args.iters)

            def pass_ms(mode):
                with torch.inference_mode():
                    eng, passes = SampleGroupsEps.for_inputs(m.vlm, ids, chunk, N, suffix_weights=mode, **mk)
                    assert len(passes) == 1, "one pass per sampler step: N * (chunk + 1) <= 256"
                    eng.set_groups(N)
                    eng(noise, t91)
                    return _replay_ms(eng), eng.graph is not None
            outs = {mode: call(mode) for mode in modes}                       # engines, graphs, packed + quantised weights
            if not table_done:
                print(json.dumps({"metric": "mla_gemm_suffix_w8 vs mla_gemm_suffix_bf16 per 7B projection shape, one launch per layer's weights",
                                  "unit": "us", "table": _suffix_kernel_table(m, dev), "data": "synthetic"}), flush=True)
                table_done = True
            total = {mode: [] for mode in modes}
            suffix = {mode: [] for mode in modes}
            graphs = {}
            for _ in range(args.pairs):                                       # bf16, fp8, bf16, fp8, ...: same box, interleaved
                for mode in modes:
                    total[mode].append(call_ms(mode))
                for mode in modes:
                    ms, graphs[mode] = pass_ms(mode)
                    suffix[mode].append(ms)
            rel = float(((outs["fp8"] - outs["bf16"]) ** 2).sum() ** 0.5 / (outs["bf16"] ** 2).sum() ** 0.5)
            print(json.dumps({"metric": "predict_action_diff_samples, MLA-Llama2-7B: bf16 vs fp8 suffix weights in alternating pairs",
                              "samples": N, "action_chunk": chunk, "suffix_rows": N * (chunk + 1), "ddim_steps": args.steps, "pairs": args.pairs,
                              "iters_per_timing": args.iters, "unit": "ms",
                              "call_ms": {k: [round(v, 2) for v in vs] for k, vs in total.items()},
                              "call_fp8_minus_bf16": _pair_stats(total["bf16"], total["fp8"]),
                              "call_fp8_minus_bf16_per_sample": round(_pair_stats(total["bf16"], total["fp8"])["mean_diff"] / N, 3),
                              "suffix_pass_ms": {k: [round(v, 3) for v in vs] for k, vs in suffix.items()},
                              "suffix_pass_fp8_minus_bf16": _pair_stats(suffix["bf16"], suffix["fp8"]),
                              "weights_streamed_per_pass_gb": {k: round(_stream_bytes(m, k) / 1e9, 2) for k in modes},
                              "suffix_pass_weight_stream_tbps": {k: round(_stream_bytes(m, k) / 1e12 / (min(suffix[k]) * 1e-3), 2) for k in modes},
                              "engine_graph": graphs, "fp8_vs_bf16_rel_diff_random_weights": round(rel, 4), "data": "synthetic"}), flush=True)
            m.vlm.__dict__.get("_prefix_engines_samples", {}).clear()         # the caches of this (N, chunk)
            torch.cuda.empty_cache()


def _ragged_groups_table(dev, cases, chunk, H=32, layers=32, reps=5, rounds=3):
    """mla_attn_chunk_ragged_groups alone at the 7B shapes (32 heads, prefixes around 545 rows) against mla_attn_chunk_groups launched once
    per sample on that sample's slice (what B predict_action_diff_samples calls issue). As the engines launch them: one launch per layer
    on that layer's own cache, captured into a graph; the arms alternate, every arm is measured `rounds` times. us per layer (one ragged
    launch vs B per-sample launches), the minimum and all rounds."""
    import math
    from mla_amd import hip
    scale = 1 / math.sqrt(128)
    R = chunk + 1
    table = {}
    for B, N in cases:
        S_p = [545 - (5 * b) % 13 for b in range(B)]
        S_cap = -(-(max(S_p) + N * R) // 64) * 64
        caches = [(torch.randn(B, S_cap, 3 * H * 128, device=dev) * 0.7).to(torch.bfloat16) for _ in range(layers)]
        lens = torch.tensor(S_p, dtype=torch.int32, device=dev)
        arms = {"ragged_groups": lambda: [hip.attn_chunk_ragged_groups(c, B, N, H, 128, lens, R, scale) for c in caches],
                "groups_per_sample": lambda: [hip.attn_chunk_groups(c[b], N, H, 128, S_p[b], R, scale) for c in caches for b in range(B)]}
        graphs = {}
        for name, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = fn()
            g.replay()
            graphs[name] = (g, keep)
        us = {name: [] for name in arms}
        for _ in range(rounds):
            for name, (g, _) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(round(e0.elapsed_time(e1) / (reps * layers) * 1e3, 1))
        table[f"B{B}_N{N}_chunk{chunk}"] = {"us_per_layer_min": {k: min(v) for k, v in us.items()}, "us_per_layer_rounds": us,
                                            "launches_per_layer": {"ragged_groups": 1, "groups_per_sample": B}, "prefix_rows": S_p}
        del graphs, caches
        torch.cuda.empty_cache()
    return table


def main_batch_samples(args, batches):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    Ns = [int(v) for v in args.samples.split(",")]
    assert len(Ns) == len(batches) and min(Ns) >= 1 and min(batches) >= 1, "--batch B[,B..] and --samples N[,N..] are paired element-wise"
    cases = list(zip(batches, Ns))
    chunk = args.chunk
    if args.kernel_table:
        print(json.dumps({"metric": "mla_attn_chunk_ragged_groups (one launch) vs mla_attn_chunk_groups per sample (B launches), 32 heads, one "
                                    "layer cache each", "unit": "us", "table": _ragged_groups_table(dev, cases, chunk), "data": "synthetic"}),
              flush=True)
    m = None
    modes = ("bf16", "fp8") if args.pair_fp8 else ("bf16",)
    for B, N in cases:
        m, b, ids = _setup(chunk, B, model=m)                                 # the model once, a batch per case
        ids = list(ids)
        images, pcs, states = (list(v) for v in zip(*(_observation(b, i) for i in range(B))))
        noise = torch.randn(B, N, chunk, 7, device=dev)

        def batched(mode):
            return m.predict_action_diff_batch(images, pcs, cur_robot_states=states, input_ids=ids, noise=noise, num_ddim_steps=args.steps,
                                               num_samples=N, suffix_weights=mode)

        def sequential(mode):
            return np.stack([m.predict_action_diff_samples(images[i], pcs[i], cur_robot_state=states[i], num_samples=N, input_ids=ids[i][None],
                                                           noise=noise[i], num_ddim_steps=args.steps, suffix_weights=mode) for i in range(B)])

        def timed(fn, mode):
            return _time_ms(lambda: fn(mode), args.iters)
        for mode in modes:
            outs = {"a": batched(mode), "b": sequential(mode)}                # engines, graphs, packed (+ quantised) weights
            ms = {"a_batch_samples": [], "b_sequential_samples": []}
            for _ in range(args.pairs):                                       # a, b, a, b, ...: same box, interleaved
                ms["a_batch_samples"].append(timed(batched, mode))
                ms["b_sequential_samples"].append(timed(sequential, mode))
            engines = m.vlm.__dict__.get("_prefix_engines_batch_samples", {})
            rel = float(((outs["a"] - outs["b"]) ** 2).sum() ** 0.5 / (outs["b"] ** 2).sum() ** 0.5)
            print(json.dumps({"metric": "N action chunks for each of B observations, MLA-Llama2-7B: (a) predict_action_diff_batch(num_samples=N), "
                                        "(b) B sequential predict_action_diff_samples calls; alternating", "suffix_weights": mode, "batch": B,
                              "samples": N, "action_chunk": chunk, "suffix_rows": B * N * (chunk + 1), "ddim_steps": args.steps,
                              "pairs": args.pairs, "iters_per_timing": args.iters, "unit": "ms",
                              "ms": {k: [round(v, 1) for v in vs] for k, vs in ms.items()}, "min_ms": {k: round(min(vs), 1) for k, vs in ms.items()},
                              "a_minus_b": _pair_stats(ms["b_sequential_samples"], ms["a_batch_samples"]),
                              "speedup_vs_b": round(min(ms["b_sequential_samples"]) / min(ms["a_batch_samples"]), 2),
                              "ms_per_chunk": round(min(ms["a_batch_samples"]) / (B * N), 1), "prompt_ids": [int(r.numel()) for r in ids],
                              "passes": len(engines), "engine_graph": bool(engines) and all(e.graph is not None for e in engines.values()),
                              "weights_streamed_per_pass_gb": round(_stream_bytes(m, mode) / 1e9, 2), "a_vs_b_rel_diff_random_weights": round(rel, 5),
                              "data": "synthetic"}), flush=True)
            for store in ("_prefix_engines_batch_samples", "_prefix_engines_samples"):     # the caches of this (B, N, mode)
                m.vlm.__dict__.get(store, {}).clear()
            torch.cuda.empty_cache()


def _wide_prefill_table(dev, Ms=(1090, 2180, 4360), H=4096, I=11008, S=545, copies=16, reps=3):
    """One launch per 7B projection shape and row count, us per launch, captured into a graph as a run over `copies` weight matrices
    (268 MB of codes for the smallest projection: nothing stays in the caches): "wide" = mla_gemm_prefill_f8_wide* with the library's
    plan, "train" = the training kernel of the same form on bf16 operands, "fp8_64_sliced" = mla_gemm_prefill_f8* (64-row tiles) in
    slices of at most 1024 rows. Random weights, no model."""
    from mla_amd import hip
    bf16 = torch.bfloat16
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2).float() / 128))
    fr = torch.outer(torch.arange(S).float(), inv)
    cos, sin = fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)
    shapes = {"qkv_rope": (3 * H, H), "o_res": (H, H), "gateup_swiglu": (2 * I, H), "down_res": (H, I)}
    table = {}
    for name, (N, K) in shapes.items():
        Wb = [(torch.randn(N, K, device=dev) * 0.02).to(bf16) for _ in range(copies)]
        W8 = [hip.quant_fp8_rows(w) for w in Wb]
        for M in Ms:
            assert M % S == 0
            x = (torch.randn(M, K, device=dev) * 0.5).to(bf16)
            xq, xs = hip.quant_fp8_rows(x)
            res = torch.randn(M, H, device=dev).to(bf16)
            out = torch.empty(M, I if name == "gateup_swiglu" else N, dtype=bf16, device=dev)
            slices = [(m0, min(1024, M - m0)) for m0 in range(0, M, 1024)]
            ws = torch.empty(max([hip.gemm_prefill_f8_wide_ws_bytes(M, N, K), 16] +
                                 [hip.gemm_prefill_f8_ws_bytes(n, N, K) for n in {S} | {n for _, n in slices}]), dtype=torch.uint8, device=dev)
            if name == "qkv_rope":
                rope = (cos, sin, 2 * H)
                train = lambda i: hip.gemm_qkv_rope(x, Wb[i], out, cos, sin, S, 2 * H)                                   # noqa: E731
                wide = lambda i: hip.gemm_prefill_f8_wide_qkv_rope(xq, xs, *W8[i], out, N, S * N, S, rope, 128, ws=ws)  # noqa: E731
                # a slice of whole samples keeps the table rows right: 545-row samples, at most one per 1024-row slice
                slices = [(m0, S) for m0 in range(0, M, S)]
                sliced = lambda i: [hip.gemm_prefill_f8_qkv_rope(xq[a:a + n], xs[a:a + n], *W8[i], out[a:a + n], N, 0, S, rope, 128, ws=ws)   # noqa: E731
                                    for a, n in slices]
            elif name == "gateup_swiglu":
                train = lambda i: hip.gemm_gateup_swiglu(x, Wb[i], False, want_gu=False) or False                       # noqa: E731
                wide = lambda i: hip.gemm_prefill_f8_wide_gateup_swiglu(xq, xs, *W8[i], out, ws=ws)                     # noqa: E731
                sliced = lambda i: [hip.gemm_prefill_f8_gateup_swiglu(xq[a:a + n], xs[a:a + n], *W8[i], out[a:a + n], ws=ws)   # noqa: E731
                                    for a, n in slices]
            else:
                train = lambda i: hip.gemm(x, Wb[i], out, residual=res)                                                 # noqa: E731
                wide = lambda i: hip.gemm_prefill_f8_wide(xq, xs, *W8[i], out, N, 0, M, residual=res, ws=ws)            # noqa: E731
                sliced = lambda i: [hip.gemm_prefill_f8(xq[a:a + n], xs[a:a + n], *W8[i], out[a:a + n], N, 0, n, residual=res[a:a + n], ws=ws)   # noqa: E731
                                    for a, n in slices]
            cell = {}
            for kname, fn in (("train", train), ("fp8_64_sliced", sliced), ("wide", wide)):
                for i in range(2):
                    assert fn(i) is not False
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for i in range(copies):
                        fn(i)
                g.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                cell[kname] = round(e0.elapsed_time(e1) / (reps * copies) * 1e3, 1)
            p = hip.plan_gemm_prefill_f8_wide(M, N, K)
            cell["wide_plan"] = {"tile_m": p.tile_m, "split": p.split, "workgroups": p.workgroups}
            cell["slices"] = len(slices)
            for kname in ("train", "fp8_64_sliced", "wide"):
                cell[kname + "_tflops"] = round(2.0 * M * N * K / (cell[kname] * 1e-6) / 1e12, 1)
            table[f"{name}/M{M}"] = cell
        del Wb, W8
        torch.cuda.empty_cache()
    return table


def main_pair_batch_prefill(args, batches):
    """predict_action_diff_batch(batch_prefill="train") vs (batch_prefill="fp8") on the same box, alternating, for every B of --batch and
    chunk of --chunks: (a) the call, (b) engine.prefill() behind the encoders = embedding + the decoder rows of the B x S_pmax prefix."""
    from mla_amd.infer import BatchedPrefixCachedEps
    dev = torch.device("cuda", 0)
    if args.kernel_table:
        print(json.dumps({"metric": "wide-row FP8 prefill GEMMs, 7B projection shapes: us per launch", "unit": "us",
                          "projection_us_per_launch": _wide_prefill_table(dev), "data": "synthetic"}), flush=True)
    if args.pairs <= 0:
        return
    chunks = [int(v) for v in args.chunks.split(",")] if args.chunks else [args.chunk]
    modes = ("train", "fp8")
    m = None
    for chunk in chunks:
        for B in batches:
            m, b, ids = _setup(chunk, B, model=m)
            ids = list(ids)
            images, pcs, states = (list(v) for v in zip(*(_observation(b, i) for i in range(B))))
            noise = torch.randn(B, chunk, 7, device=dev)

            def call(mode):
                return m.predict_action_diff_batch(images, pcs, cur_robot_states=states, input_ids=ids, noise=noise, num_ddim_steps=args.steps,
                                                   batch_prefill=mode)
            acts = {mode: call(mode) for mode in modes}                      # engines, graphs, packed weights, the FP8 copy
            mk = dict(images=torch.stack(images), point_cloud=torch.stack(pcs), camera_name="rlbench_front", proprio=b["proprio"][:B])
            rows = [[int(t) for t in r] for r in ids]
            with torch.inference_mode():
                front = BatchedPrefixCachedEps._front_tokens(m.vlm, mk["images"], mk["point_cloud"], mk["camera_name"])
                subs = {mode: list(BatchedPrefixCachedEps.for_batch(m.vlm, rows, chunk, batch_prefill=mode, **mk)) for mode in modes}

            def prefill_ms(mode, reps=3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.inference_mode():
                    e0.record()
                    for _ in range(reps):
                        for sub, eng in subs[mode]:
                            eng.prefill(sub, front[sub.start:sub.stop], mk["proprio"][sub.start:sub.stop])
                    e1.record()
                    torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps
            call_ms, pre_ms = {mode: [] for mode in modes}, {mode: [] for mode in modes}
            for _ in range(args.pairs):
                for mode in modes:
                    call_ms[mode].append(_time_ms(lambda: call(mode), args.iters))
            for mode in modes:
                prefill_ms(mode, 1)
            for _ in range(args.pairs):
                for mode in modes:
                    pre_ms[mode].append(prefill_ms(mode))
            rel = float(((acts["fp8"] - acts["train"]) ** 2).sum() ** 0.5 / (acts["train"] ** 2).sum() ** 0.5)
            print(json.dumps({"metric": "predict_action_diff_batch, MLA-Llama2-7B: batch_prefill=train vs fp8 in alternating order", "batch": B,
                              "action_chunk": chunk, "prefill_rows": [sub.S_pmax * (sub.stop - sub.start) for sub, _ in subs["fp8"]],
                              "ddim_steps": args.steps, "pairs": args.pairs, "unit": "ms",
                              "call_ms": {mode: [round(v, 2) for v in vs] for mode, vs in call_ms.items()},
                              "call_fp8_minus_train": _pair_stats(call_ms["train"], call_ms["fp8"]),
                              "prefill_behind_encoders_ms": {mode: [round(v, 2) for v in vs] for mode, vs in pre_ms.items()},
                              "prefill_behind_encoders_fp8_minus_train": _pair_stats(pre_ms["train"], pre_ms["fp8"]),
                              "fp8_vs_train_chunk_rel_diff_random_weights": round(rel, 4), "data": "synthetic"}), flush=True)


def main_batch(args):
    from mla_amd.infer import BatchedPrefixCachedEps
    B = args.batch
    m, b, ids = _setup(args, B)
    ids, dev = list(ids), ids[0].device
    images, pcs, states = (list(v) for v in zip(*(_observation(b, i) for i in range(B))))
    noise = torch.randn(B, args.chunk, 7, device=dev)

    def batched():
        return m.predict_action_diff_batch(images, pcs, cur_robot_states=states, input_ids=ids, noise=noise, num_ddim_steps=args.steps)

    def sequential():
        return [m.predict_action_diff(image=images[i], pointcloud=pcs[i], cur_robot_state=states[i], input_ids=ids[i][None], noise=noise[i:i + 1],
                                      num_ddim_steps=args.steps) for i in range(B)]

    act = batched()                                                        # engines, graphs, packed weights
    sequential()
    # alternating pairs in one process: batched, sequential, batched, sequential
    ms_b1, ms_s1, ms_b2, ms_s2 = (_time_ms(fn, args.iters) for fn in (batched, sequential, batched, sequential))
    parts = {}
    engines = m.vlm.__dict__.get("_prefix_engines_batched", {})
    if engines:
        # where the batched call's time goes: encoders + planning + the varlen prefill of every sub-batch, and one graph replay per sub-batch
        mk = dict(images=torch.stack(images), point_cloud=torch.stack(pcs), camera_name="rlbench_front", proprio=b["proprio"][:B])
        rows = [[int(t) for t in r] for r in ids]
        wbytes = sum(p.numel() for l in m.vlm.llm_backbone.llm.model.layers for p in l.parameters()) * 2
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        n_sub, pass_ms = 0, 0.0
        with torch.inference_mode():
            for sub, eng in BatchedPrefixCachedEps.for_batch(m.vlm, rows, args.chunk, **mk):
                n_sub += 1
            ev[1].record()
            torch.cuda.synchronize()
            for sub, eng in BatchedPrefixCachedEps.for_batch(m.vlm, rows, args.chunk, **mk):
                eng(noise[sub.start:sub.stop], torch.full((sub.stop - sub.start,), 91, device=dev))
                pass_ms += _replay_ms(eng)
        parts = {"sub_batches": n_sub, "prefill_ms": round(ev[0].elapsed_time(ev[1]), 2), "suffix_pass_graph_replay_ms": round(pass_ms, 3),
                 "weights_streamed_per_pass_gb": round(wbytes * n_sub / 1e9, 2),
                 "suffix_pass_weight_stream_tbps": round(wbytes * n_sub / 1e12 / (pass_ms * 1e-3), 2)}
    print(json.dumps({"metric": "predict_action_diff_batch latency, MLA-Llama2-7B bf16", "batch": B, "action_chunk": args.chunk,
                      "value": round(min(ms_b1, ms_b2), 1), "unit": "ms", "batched_ms": [round(ms_b1, 1), round(ms_b2, 1)],
                      "sequential_ms": [round(ms_s1, 1), round(ms_s2, 1)], "speedup": round(min(ms_s1, ms_s2) / min(ms_b1, ms_b2), 2),
                      "ms_per_observation": round(min(ms_b1, ms_b2) / B, 1), "ddim_steps": args.steps, "prompt_ids": [int(r.numel()) for r in ids],
                      "engine": "batched" if engines else "sequential", **parts, "action": [round(float(v), 4) for v in act.reshape(-1)[:7]],
                      "data": "synthetic"}))


if __name__ == "__main__":
    main()
