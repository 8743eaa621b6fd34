"""What the weight average (EMA) costs next to AdamW: three arms on the in-step pattern of tools/bench_adamw.py -- every launch works
on a different slice (one 7B decoder layer, 202 M elements) of arena-like buffers whose slices start on 2 MiB boundaries, right after a
GEMM burst --
    A  plain      mla_adamw_step_groups                        30 B per element
    B  fused      mla_adamw_ema_step_groups                    38 B (+ the EMA stream, read and written once)
    C  two-launch mla_adamw_step_groups, then mla_ema_update   42 B (the new master is read again)
run as alternating same-box rounds A B C A B C ...; per arm the time per slice and the bandwidth, per pair of arms the paired difference
with the 95 % interval of tools/ab_pairs.py, scaled to the trainable elements of a BASELINE configs[1] step.
    python tools/bench_adamw_ema.py [--rounds 10] [--slices 8] [--out profiles/adamw_ema.txt]"""
import argparse, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mla_amd import hip
from tools.ab_pairs import T95

N = 202_383_360            # one decoder layer's parameters
N_DECAY = N - 8192         # its two norm weights are not decayed
STEP_ELEMENTS = 6.75e9     # trainable elements of a configs[1] step: AdamW 33.6 ms at 6.03 TB/s and 30 B per element
GRAN = (2 << 20) // 4      # fp32 elements per 2 MiB: the arenas' slice alignment (mla_amd/fsdp.py _Arenas)
BYTES = {"plain": 30, "fused": 38, "two-launch": 42}
HYPER = (1e-4, 0.9, 0.999, 1e-8, 0.01, 3)
DECAY = 0.9999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--elements", type=int, default=N)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_ema needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    n, L = args.elements, args.slices
    n_decay = min(N_DECAY, n) // 4 * 4
    stride = (n + GRAN - 1) // GRAN * GRAN
    bufs = [torch.randn(stride * L, device=dev) for _ in range(5)]            # p, g, m, v, ema: one allocation per kind
    bufs[3].abs_()
    p16 = torch.empty(stride * L, dtype=torch.bfloat16, device=dev)
    coef = torch.ones(1, device=dev)
    a = torch.randn(17536, 4096, device=dev).to(torch.bfloat16)
    w = torch.randn(22016, 4096, device=dev).to(torch.bfloat16)

    def views(l):
        return [b[l * stride:l * stride + n] for b in bufs] + [p16[l * stride:l * stride + n]]

    def plain(l):
        p, g, m, v, _, q = views(l)
        hip.adamw_step_groups(p, g, m, v, q, n_decay, *HYPER, coef)

    def fused(l):
        p, g, m, v, e, q = views(l)
        hip.adamw_ema_step_groups(p, g, m, v, e, q, n_decay, *HYPER, coef, DECAY)

    def two(l):
        p, g, m, v, e, q = views(l)
        hip.adamw_step_groups(p, g, m, v, q, n_decay, *HYPER, coef)
        hip.ema_update(e, p, DECAY)

    arms = (("plain", plain), ("fused", fused), ("two-launch", two))

    def measure(fn):
        """ms per slice of one sweep over the L slices, right after ~30 ms of GEMMs (the optimizer follows the backward)."""
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(12):
            hip.gemm(a, w)
        s.record()
        for l in range(L):
            fn(l)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / L

    for _, fn in arms:                                                        # warm-up: code objects, every slice touched
        measure(fn)
    ms = {name: [] for name, _ in arms}
    props = torch.cuda.get_device_properties(0)
    lines = [f"box: 1 x {props.name} ({props.gcnArchName}, {props.multi_processor_count} CUs, {props.total_memory / 2 ** 30:.0f} GiB), "
             f"torch {torch.__version__}, hip {torch.version.hip}; {L} distinct slices of {n} elements "
             f"(stride {stride}: 2 MiB-aligned), n_decay {n_decay}, each sweep right after 12 GEMMs 17536 x 22016 x 4096; EMA decay {DECAY}; "
             f"{args.rounds} alternating rounds A B C in one process"]
    for r in range(args.rounds):
        for name, fn in arms:
            ms[name].append(measure(fn))
        lines.append(f"round {r + 1}: " + "   ".join(f"{name} {ms[name][-1]:7.3f} ms/slice" for name, _ in arms))
        print(lines[-1], flush=True)
    for name, _ in arms:
        med = statistics.median(ms[name])
        lines.append(f"{name:<10} median {med:7.3f} ms/slice (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})  {n * BYTES[name] / med / 1e9:5.2f} TB/s "
                     f"at {BYTES[name]} B/element  -> {med / n * STEP_ELEMENTS:6.2f} ms per configs[1] step ({STEP_ELEMENTS:.3g} trainable elements)")

    def paired(b, a_):
        d = [(y - x) / n * STEP_ELEMENTS for x, y in zip(ms[a_], ms[b])]
        mean = statistics.mean(d)
        half = T95.get(len(d), 2.0) * statistics.stdev(d) / math.sqrt(len(d)) if len(d) > 1 else float("nan")
        verdict = "excludes 0" if (mean - half) * (mean + half) > 0 else "INCLUDES 0"
        return f"{b} - {a_}: mean {mean:+.2f} ms per configs[1] step, 95 % CI [{mean - half:+.2f}, {mean + half:+.2f}] over {len(d)} pairs -> {verdict}"

    lines += [paired("fused", "plain"), paired("two-launch", "plain"), paired("fused", "two-launch")]
    print("\n".join(lines[-6:]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
