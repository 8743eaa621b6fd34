"""Dump the outputs of every suffix-attention entry point (attn_chunk, attn_chunk_ragged, attn_chunk_groups, attn_chunk_ragged_groups,
attn_chunk_split, attn_groups_split; seeded inputs, small shapes plus the 7B sampler shapes once) so that two library builds can be
compared bit for bit, workspace states of the split forms included:
    MLA_HIP_LIB=<a> python tools/exp_suffix_attn_bits.py a.pt;  MLA_HIP_LIB=<b> python tools/exp_suffix_attn_bits.py b.pt
    python tools/exp_suffix_attn_bits.py a.pt b.pt                       compares; exit status 1 on any difference
    python tools/exp_suffix_attn_bits.py --time                          one JSON line: microseconds per launch of the six entry points at
                                                                         the 7B sampler shapes (device events around graph replays)
    python tools/exp_suffix_attn_bits.py --pair-libs <a> <b> [--pairs 6] child processes a, b, a, a per round: the paired difference b - a
                                                                         per kernel with its 95 % interval, beside the a - a null's"""
import argparse, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lib_pairing import _us_per_launch, pair_libs

METRIC = "suffix attention, microseconds per launch at the 7B sampler shapes: library b - library a, paired"

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("paths", nargs="*", metavar="FILE.pt", help="one path: dump under MLA_HIP_LIB; two paths: compare the dumps")
ap.add_argument("--time", action="store_true", help="time the six entry points under MLA_HIP_LIB")
ap.add_argument("--pair-libs", nargs=2, metavar=("A", "B"), help="time library B against library A in alternating child processes")
ap.add_argument("--pairs", type=int, default=6, help="rounds of --pair-libs (default 6)")
args = ap.parse_args()
if not args.time and not args.pair_libs and len(args.paths) not in (1, 2):
    ap.error("give one path to dump, two to compare, --time or --pair-libs A B")
if args.pair_libs:
    sys.exit(pair_libs(__file__, METRIC, args.pair_libs[0], args.pair_libs[1], args.pairs))

import torch

if len(args.paths) == 2:
    a, b = torch.load(args.paths[0]), torch.load(args.paths[1])
    bad = [k for k in a if k not in b or not torch.equal(a[k], b[k])] + [k for k in b if k not in a]
    print(f"{len(a)} tensors compared, {len(bad)} differ: {bad[:8]}")
    sys.exit(1 if bad else 0)

from mla_amd import hip
dev = torch.device("cuda:0")
D, BF = 128, torch.bfloat16
scale = 1 / math.sqrt(D)


def _rand(shape, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * 0.7).to(BF)


def _ws(nbytes):
    return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dev)


def _bits(t):
    return t.view(torch.int16).cpu()


def dump_chunk(out, H, R, S_kv, seed):
    """attn_chunk, attn_chunk_ragged (B = 3: one length below R, one above the capacity) and attn_chunk_split with its states"""
    tag = f"H{H}_R{R}_S{S_kv}"
    cache = _rand((1, S_kv, 3 * H * D), seed)
    out[f"chunk_{tag}"] = _bits(hip.attn_chunk(cache, 1, H, D, S_kv, R, scale))
    cache3 = _rand((3, S_kv, 3 * H * D), seed + 1)
    kv_len = torch.tensor([R - 1, S_kv + 5, (R + S_kv + 1) // 2], dtype=torch.int32, device=dev)
    out[f"chunk_ragged_{tag}"] = _bits(hip.attn_chunk_ragged(cache3, 3, H, D, kv_len, R, scale))
    nT = -(-S_kv // 64)
    for sp in sorted({s for s in (1, 2, 3, nT) if s <= nT}) + [None]:
        n = hip.attn_split_plan(1, H, R, S_kv)[0] if sp is None else sp
        need = hip.attn_split_ws_bytes(1, H, R, S_kv, n)
        ws = _ws(need)
        out[f"chunk_split{'_plan' if sp is None else sp}_{tag}"] = _bits(hip.attn_chunk_split(cache, 1, H, D, S_kv, R, scale, splits=sp, ws=ws))
        if n > 1:
            out[f"chunk_split{'_plan' if sp is None else sp}_{tag}_ws"] = ws[:need].view(torch.int32).cpu()


def dump_groups(out, H, R, G, S_p, seed, gws=(1, 2, 4)):
    """attn_chunk_groups / attn_chunk_ragged_groups in every launch form, attn_groups_split plain and ragged with its states"""
    tag = f"H{H}_R{R}_G{G}_P{S_p}"
    cache = _rand((S_p + G * R, 3 * H * D), seed)
    out[f"groups_{tag}"] = _bits(hip.attn_chunk_groups(cache, G, H, D, S_p, R, scale))
    for gw in gws:
        for order in (0, 1):
            out[f"groups_gw{gw}_o{order}_{tag}"] = _bits(hip.attn_chunk_groups(cache, G, H, D, S_p, R, scale, gw=gw, order=order))
    S_cap = S_p + G * R + 7
    cache3 = _rand((3, S_cap, 3 * H * D), seed + 1)
    prefix = torch.tensor([-3, S_cap, S_p], dtype=torch.int32, device=dev)        # clamped to 0 and to S_cap - G R
    out[f"ragged_groups_{tag}"] = _bits(hip.attn_chunk_ragged_groups(cache3, 3, G, H, D, prefix, R, scale))
    for gw in gws:
        out[f"ragged_groups_gw{gw}_{tag}"] = _bits(hip.attn_chunk_ragged_groups(cache3, 3, G, H, D, prefix, R, scale, gw=gw))
    for ragged, B, c, p, S in ((False, 1, cache, S_p, S_p), (True, 3, cache3, prefix, S_cap)):
        S_max, plan = hip.attn_groups_split_plan(B, G, H, R, S, ragged)
        nT = -(-S_max // 64)
        for sp in sorted({s for s in (1, 2) if s <= nT}) + [None]:
            n = plan[0] if sp is None else sp
            need = hip.attn_split_ws_bytes(B * G, H, R, S_max, n)
            ws = _ws(need)
            name = f"groups_split{'_plan' if sp is None else sp}_{'ragged_' if ragged else ''}{tag}"
            out[name] = _bits(hip.attn_groups_split(c, B, G, H, D, p, R, scale, splits=sp, ws=ws))
            if n > 1:
                out[name + "_ws"] = ws[:need].view(torch.int32).cpu()


def time_entries(H=32, S_p=547, G=8, layers=32):
    us = {}
    for R in (2, 17):
        S_kv = S_p + R
        one = [_rand((1, S_kv, 3 * H * D), 100 + i) for i in range(layers)]
        kv_len = torch.tensor([S_kv - 3 * b for b in range(4)], dtype=torch.int32, device=dev)
        us[f"attn_chunk_R{R}"] = _us_per_launch(lambda c: hip.attn_chunk(c, 1, H, D, S_kv, R, scale), one)
        ws = _ws(hip.attn_split_ws_bytes(1, H, R, S_kv, 0))
        us[f"attn_chunk_split_R{R}"] = _us_per_launch(lambda c: hip.attn_chunk_split(c, 1, H, D, S_kv, R, scale, ws=ws), one)
        del one
        four = [_rand((4, S_kv, 3 * H * D), 200 + i) for i in range(layers)]
        us[f"attn_chunk_ragged_B4_R{R}"] = _us_per_launch(lambda c: hip.attn_chunk_ragged(c, 4, H, D, kv_len, R, scale), four)
        del four
        grp = [_rand((S_p + G * R, 3 * H * D), 300 + i) for i in range(layers)]
        us[f"attn_chunk_groups_G{G}_R{R}"] = _us_per_launch(lambda c: hip.attn_chunk_groups(c, G, H, D, S_p, R, scale), grp)
        S_max, _ = hip.attn_groups_split_plan(1, G, H, R, S_p, False)
        wsg = _ws(hip.attn_split_ws_bytes(G, H, R, S_max, 0))
        us[f"attn_groups_split_G{G}_R{R}"] = _us_per_launch(lambda c: hip.attn_groups_split(c, 1, G, H, D, S_p, R, scale, ws=wsg), grp)
        del grp
        S_cap = S_p + G * R
        prefix = torch.tensor([S_p, S_p - 3], dtype=torch.int32, device=dev)
        rg = [_rand((2, S_cap, 3 * H * D), 400 + i) for i in range(layers)]
        us[f"attn_chunk_ragged_groups_B2_G{G}_R{R}"] = _us_per_launch(lambda c: hip.attn_chunk_ragged_groups(c, 2, G, H, D, prefix, R, scale), rg)
        del rg
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "suffix attention per launch, 32 heads of 128, 547 prefix rows", "unit": "us", "library": hip._LIB_PATH,
                      "us_per_launch": {k: round(v, 3) for k, v in us.items()}, "data": "synthetic"}))


if args.time:
    time_entries()
    sys.exit(0)
out, seed = {}, 0
for R in (1, 9, 16, 17, 64):
    for S_kv in sorted({R, 65, 130, 565}):
        seed += 2
        dump_chunk(out, 2, R, S_kv, seed)
    for G in (1, 3, 5):
        for S_p in (0, 63, 64, 200):
            seed += 2
            dump_groups(out, 2, R, G, S_p, seed)
for R in (2, 17):                                                          # the 7B sampler shapes, once
    dump_chunk(out, 32, R, 547 + R, 1000 + R)
    dump_groups(out, 32, R, 8, 547, 2000 + R, gws=(1, 2, 4))
torch.cuda.synchronize()
torch.save(out, args.paths[0])
print("saved", len(out), "tensors")
