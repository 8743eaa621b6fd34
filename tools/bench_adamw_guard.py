"""What the skip_nonfinite guard costs in the AdamW pass: the guarded launch (mla_adamw_guard_step, flag clear) against the launch it
wraps, on the in-step pattern of tools/bench_adamw_m16.py -- every launch works on a different slice (one 7B decoder layer, 202 M
elements) of arena-like buffers whose slices start on 2 MiB boundaries, right after a GEMM burst --
    A  fp32          mla_adamw_step_groups                           30 B per element
    B  fp32+guard    mla_adamw_guard_step, fp32 moments, flag 0      30 B + one scalar load per workgroup
    C  m16           mla_adamw_m16_step                              22 B
    D  m16+guard     mla_adamw_guard_step, bf16 moments, flag 0      22 B + one scalar load per workgroup
    E  skipped       mla_adamw_guard_step, fp32 moments, flag 1      nothing: every workgroup returns at once
run as alternating same-box rounds A B C D E A B ...; per arm the time per slice, per pair (B - A, D - C) the paired difference with the
95 % interval of tools/ab_pairs.py, scaled to the trainable elements of a BASELINE configs[1] step. mla_clip_coef_guard against
mla_clip_coef (one thread each) is timed over 200 back-to-back launches.
    python tools/bench_adamw_guard.py [--rounds 10] [--slices 8] [--out profiles/adamw_guard.txt]"""
import argparse, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mla_amd import hip
from tools.ab_pairs import T95
from tools.bench_adamw_m16 import DECAY, GRAN, HYPER, N, N_DECAY, SEED, STEP_ELEMENTS

BYTES = {"fp32": 30, "fp32+guard": 30, "m16": 22, "m16+guard": 22}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--elements", type=int, default=N)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamw_guard needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    n, L = args.elements, args.slices
    n_decay = min(N_DECAY, n) // 4 * 4
    stride = (n + 2 * GRAN - 1) // (2 * GRAN) * (2 * GRAN)
    bufs = [torch.randn(stride * L, device=dev) for _ in range(4)]            # p, g, m, v: one allocation per kind
    bufs[3].abs_()
    m16 = bufs[2].to(torch.bfloat16)
    v16 = bufs[3].to(torch.bfloat16)
    p16 = torch.empty(stride * L, dtype=torch.bfloat16, device=dev)
    coef = torch.ones(1, device=dev)
    flags = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    go, skip = flags[0:1], flags[1:2]
    a = torch.randn(17536, 4096, device=dev).to(torch.bfloat16)
    w = torch.randn(22016, 4096, device=dev).to(torch.bfloat16)

    def views(l):
        return [b[l * stride:l * stride + n] for b in bufs + [m16, v16, p16]]

    def fp32(l):
        p, g, m, v, _, _, q = views(l)
        hip.adamw_step_groups(p, g, m, v, q, n_decay, *HYPER, coef)

    def fp32_guard(l, flag=go):
        p, g, m, v, _, _, q = views(l)
        hip.adamw_guard_step(p, g, m, v, None, q, n_decay, *HYPER, coef, DECAY, SEED, l * stride, flag)

    def m16_plain(l):
        p, g, _, _, mm, vv, q = views(l)
        hip.adamw_m16_step(p, g, mm, vv, None, q, n_decay, *HYPER, coef, DECAY, SEED, l * stride)

    def m16_guard(l):
        p, g, _, _, mm, vv, q = views(l)
        hip.adamw_guard_step(p, g, mm, vv, None, q, n_decay, *HYPER, coef, DECAY, SEED, l * stride, go)

    arms = (("fp32", fp32), ("fp32+guard", fp32_guard), ("m16", m16_plain), ("m16+guard", m16_guard),
            ("skipped", lambda l: fp32_guard(l, skip)))

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
             f"{args.rounds} alternating rounds A B C D E in one process"]
    for r in range(args.rounds):
        for name, fn in arms:
            ms[name].append(measure(fn))
        lines.append(f"round {r + 1}: " + "   ".join(f"{name} {ms[name][-1]:7.3f} ms/slice" for name, _ in arms))
        print(lines[-1], flush=True)
    for name, _ in arms:
        med = statistics.median(ms[name])
        rate = f"  {n * BYTES[name] / med / 1e9:5.2f} TB/s at {BYTES[name]} B/element" if name in BYTES else ""
        lines.append(f"{name:<11} median {med:7.3f} ms/slice (min {min(ms[name]):.3f}, max {max(ms[name]):.3f}){rate}  -> "
                     f"{med / n * STEP_ELEMENTS:6.2f} ms per configs[1] step ({STEP_ELEMENTS:.3g} trainable elements)")

    def paired(b, a_):
        d = [(y - x) / n * STEP_ELEMENTS for x, y in zip(ms[a_], ms[b])]
        mean = statistics.mean(d)
        half = T95.get(len(d), 2.0) * statistics.stdev(d) / math.sqrt(len(d)) if len(d) > 1 else float("nan")
        verdict = "excludes 0" if (mean - half) * (mean + half) > 0 else "INCLUDES 0"
        return (f"{b} - {a_}: mean {mean:+.3f} ms per configs[1] step, 95 % CI [{mean - half:+.3f}, {mean + half:+.3f}] over {len(d)} pairs -> "
                f"{verdict}; time ratio {statistics.median(ms[b]) / statistics.median(ms[a_]):.4f}")

    lines += [paired("fp32+guard", "fp32"), paired("m16+guard", "m16")]
    # the clip-coefficient launch: one thread either way
    sumsq, norm = torch.full((1,), 4.0e4, device=dev), torch.zeros(1, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    per = {}
    for name, fn in (("mla_clip_coef", lambda: hip.clip_coef(sumsq, 1.0, coef, norm)),
                     ("mla_clip_coef_guard", lambda: hip.clip_coef_guard(sumsq, 1.0, coef, norm, flag))):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(2):
            s.record()
            for _ in range(200):
                fn()
            e.record()
            torch.cuda.synchronize()
        per[name] = s.elapsed_time(e) / 200 * 1e3
    lines.append("clip coefficient, 200 back-to-back launches: " + ", ".join(f"{k} {v:.2f} us per launch" for k, v in per.items()))
    print("\n".join(lines[-8:]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
