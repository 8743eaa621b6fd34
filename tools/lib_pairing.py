"""What the two-library experiment tools share (exp_suffix_attn_bits.py, exp_suffix_proj_bits.py): microseconds per launch from graph
replays, and the paired comparison of two builds of libmla_hip.so in alternating child processes, each child timing every kernel of the
tool under MLA_HIP_LIB and printing one JSON line with "us_per_launch"."""
import json, math, os, subprocess, sys

T95 = {2: 12.706, 3: 4.303, 4: 3.182, 5: 2.776, 6: 2.571, 7: 2.447, 8: 2.365, 9: 2.306, 10: 2.262, 11: 2.228, 12: 2.201}


def _interval(d):
    n, mean = len(d), sum(d) / len(d)
    half = T95.get(n, 1.96) * math.sqrt(sum((x - mean) ** 2 for x in d) / (n - 1) / n) if n > 1 else float("nan")
    return {"mean": round(mean, 3), "lo": round(mean - half, 3), "hi": round(mean + half, 3)}


def pair_libs(script, metric, lib_a, lib_b, pairs, child_timeout=300):
    """Child processes a, b, a, a of `script --time` per round: the paired difference b - a per kernel with its 95 % interval, beside the
    a - a null's. Prints one JSON line; returns 1 when some kernel's b - a interval lies wholly above its null's interval."""
    def child(lib):
        r = subprocess.run([sys.executable, os.path.abspath(script), "--time"], env=dict(os.environ, MLA_HIP_LIB=os.path.abspath(lib)),
                           capture_output=True, text=True, timeout=child_timeout)
        if r.returncode != 0:
            sys.exit(f"child on {lib} ended with {r.returncode}: {r.stderr[-800:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])["us_per_launch"]
    diff, null, level = {}, {}, {}
    for rnd in range(pairs):
        a0, b0, a1, a2 = child(lib_a), child(lib_b), child(lib_a), child(lib_a)
        print(f"round {rnd + 1} of {pairs} done", file=sys.stderr, flush=True)
        for k in a0:
            diff.setdefault(k, []).append(b0[k] - a0[k])
            null.setdefault(k, []).append(a2[k] - a1[k])
            level.setdefault(k, []).append(a0[k])
    table = {k: {"a_us": round(sum(level[k]) / pairs, 2), "b_minus_a": _interval(diff[k]), "a_minus_a": _interval(null[k]),
                 "b_interval_wholly_above_null": _interval(diff[k])["lo"] > _interval(null[k])["hi"]} for k in diff}
    print(json.dumps({"metric": metric, "unit": "us", "a": lib_a, "b": lib_b, "pairs": pairs, "table": table, "data": "synthetic"}))
    return 1 if any(v["b_interval_wholly_above_null"] for v in table.values()) else 0


def _us_per_launch(fn, caches, window_ms=150.0):
    """`len(caches)` launches over as many caches per graph; device events around enough replays to fill the window, after warm-up"""
    import torch
    for c in caches[:2]:                                                   # function attributes, allocator
        fn(c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in caches:
            fn(c)

    def run(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    run(3)
    reps = max(3, int(window_ms / max(run(3) / 3, 1e-3)))
    return run(reps) / (reps * len(caches)) * 1e3
