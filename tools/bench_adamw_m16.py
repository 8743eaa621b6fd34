"""What bf16 AdamW moments with stochastic rounding cost or save in the AdamW pass: four arms on the in-step pattern of
tools/bench_adamw_ema.py -- every launch works on a different slice (one 7B decoder layer, 202 M elements) of arena-like buffers whose
slices start on 2 MiB boundaries, right after a GEMM burst --
    A  fp32        mla_adamw_step_groups                  30 B per element
    B  m16         mla_adamw_m16_step, ema = NULL         22 B (both moments read and written as bf16, one Philox call per four elements)
    C  fp32+ema    mla_adamw_ema_step_groups              38 B
    D  m16+ema     mla_adamw_m16_step with the average    30 B
run as alternating same-box rounds A B C D A B C D ...; per arm the time per slice and the achieved bytes/s, per pair (B - A, D - C) the
paired difference with the 95 % interval of tools/ab_pairs.py, scaled to the trainable elements of a BASELINE configs[1] step. The
yardstick of the m16 arms is the fp32 arm of the SAME build in the SAME run: from the byte counts B should take 22/30 of A and D 30/38
of C; where the m16 rate falls below the fp32 arm's own round-to-round spread, the generator is not hiding under the memory time.
    python tools/bench_adamw_m16.py [--rounds 10] [--slices 8] [--out profiles/adamw_m16.txt]"""
import argparse, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mla_amd import hip
from tools.ab_pairs import T95

N = 202_383_360            # one decoder layer's parameters
N_DECAY = N - 8192         # its two norm weights are not decayed
STEP_ELEMENTS = 6.75e9     # trainable elements of a configs[1] step
GRAN = (2 << 20) // 4      # fp32 elements per 2 MiB: the arenas' slice alignment (mla_amd/fsdp.py _Arenas; the bf16 arenas' slices are 2 MiB
#                            aligned too: a stride that is a multiple of GRAN elements is a multiple of 1 MiB in bf16 -- rounded up to even below)
BYTES = {"fp32": 30, "m16": 22, "fp32+ema": 38, "m16+ema": 30}
HYPER = (1e-4, 0.9, 0.999, 1e-8, 0.01, 3)
DECAY = 0.9999
SEED = 0x1234ABCD5678EF01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--elements", type=int, default=N)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_m16 needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    n, L = args.elements, args.slices
    n_decay = min(N_DECAY, n) // 4 * 4
    stride = (n + 2 * GRAN - 1) // (2 * GRAN) * (2 * GRAN)
    bufs = [torch.randn(stride * L, device=dev) for _ in range(5)]            # p, g, m, v, ema: one allocation per kind
    bufs[3].abs_()
    m16 = bufs[2].to(torch.bfloat16)
    v16 = bufs[3].to(torch.bfloat16)
    p16 = torch.empty(stride * L, dtype=torch.bfloat16, device=dev)
    coef = torch.ones(1, device=dev)
    a = torch.randn(17536, 4096, device=dev).to(torch.bfloat16)
    w = torch.randn(22016, 4096, device=dev).to(torch.bfloat16)

    def views(l):
        return [b[l * stride:l * stride + n] for b in bufs + [m16, v16, p16]]

    def fp32(l):
        p, g, m, v, _, _, _, q = views(l)
        hip.adamw_step_groups(p, g, m, v, q, n_decay, *HYPER, coef)

    def fp32_ema(l):
        p, g, m, v, e, _, _, q = views(l)
        hip.adamw_ema_step_groups(p, g, m, v, e, q, n_decay, *HYPER, coef, DECAY)

    def m16_plain(l):
        p, g, _, _, _, mm, vv, q = views(l)
        hip.adamw_m16_step(p, g, mm, vv, None, q, n_decay, *HYPER, coef, DECAY, SEED, l * stride)

    def m16_ema(l):
        p, g, _, _, e, mm, vv, q = views(l)
        hip.adamw_m16_step(p, g, mm, vv, e, q, n_decay, *HYPER, coef, DECAY, SEED, l * stride)

    arms = (("fp32", fp32), ("m16", m16_plain), ("fp32+ema", fp32_ema), ("m16+ema", m16_ema))

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
             f"(stride {stride}: 2 MiB-aligned in fp32 and in bf16), n_decay {n_decay}, each sweep right after 12 GEMMs 17536 x 22016 x 4096; "
             f"EMA decay {DECAY}; {args.rounds} alternating rounds A B C D in one process"]
    for r in range(args.rounds):
        for name, fn in arms:
            ms[name].append(measure(fn))
        lines.append(f"round {r + 1}: " + "   ".join(f"{name} {ms[name][-1]:7.3f} ms/slice" for name, _ in arms))
        print(lines[-1], flush=True)
    for name, _ in arms:
        med = statistics.median(ms[name])
        lines.append(f"{name:<9} median {med:7.3f} ms/slice (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})  {n * BYTES[name] / med / 1e9:5.2f} TB/s "
                     f"at {BYTES[name]} B/element  -> {med / n * STEP_ELEMENTS:6.2f} ms per configs[1] step ({STEP_ELEMENTS:.3g} trainable elements)")

    def paired(b, a_):
        d = [(y - x) / n * STEP_ELEMENTS for x, y in zip(ms[a_], ms[b])]
        mean = statistics.mean(d)
        half = T95.get(len(d), 2.0) * statistics.stdev(d) / math.sqrt(len(d)) if len(d) > 1 else float("nan")
        verdict = "excludes 0" if (mean - half) * (mean + half) > 0 else "INCLUDES 0"
        ratio = statistics.median(ms[b]) / statistics.median(ms[a_])
        return (f"{b} - {a_}: mean {mean:+.2f} ms per configs[1] step, 95 % CI [{mean - half:+.2f}, {mean + half:+.2f}] over {len(d)} pairs -> "
                f"{verdict}; time ratio {ratio:.3f} (bytes ratio {BYTES[b] / BYTES[a_]:.3f})")

    lines += [paired("m16", "fp32"), paired("m16+ema", "fp32+ema")]
    for name in ("fp32", "fp32+ema"):
        rates = [n * BYTES[name] / t / 1e9 for t in ms[name]]
        lines.append(f"{name} round-to-round spread of the rate: {min(rates):.2f} .. {max(rates):.2f} TB/s")
    print("\n".join(lines[-8:]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
