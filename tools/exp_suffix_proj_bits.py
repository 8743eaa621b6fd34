"""Dump the output digests of every suffix projection entry point (gemv, gemm_skinny, gemm_skinny_gateup_swiglu, gemm_suffix; bf16 and
FP8 weights: the cases of tests/test_infer_proj_golden_gpu.py plus the 7B projection shapes once) so that two library builds can be
compared bit for bit, and time them:
    MLA_HIP_LIB=<a> python tools/exp_suffix_proj_bits.py a.pt;  MLA_HIP_LIB=<b> python tools/exp_suffix_proj_bits.py b.pt
    python tools/exp_suffix_proj_bits.py a.pt b.pt                       compares; exit status 1 on any difference
    python tools/exp_suffix_proj_bits.py --time                          one JSON line: microseconds per launch at the 7B projection shapes,
                                                                         M = 2, 17, 48, 64 through the single-sample entry points (plain,
                                                                         norm, swiglu, gateup) and M = 17, 48, 64, 136, 256 through the
                                                                         batched ones (device events around graph replays over weight
                                                                         copies that together exceed the last-level cache)
    python tools/exp_suffix_proj_bits.py --pair-libs <a> <b> [--pairs 6] child processes a, b, a, a per round: the paired difference b - a
                                                                         per kernel with its 95 % interval, beside the a - a null's"""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lib_pairing import _us_per_launch, pair_libs

METRIC = "suffix projections, microseconds per launch at the 7B shapes: library b - library a, paired"

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("paths", nargs="*", metavar="FILE.pt", help="one path: dump under MLA_HIP_LIB; two paths: compare the dumps")
ap.add_argument("--time", action="store_true", help="time the entry points under MLA_HIP_LIB")
ap.add_argument("--pair-libs", nargs=2, metavar=("A", "B"), help="time library B against library A in alternating child processes")
ap.add_argument("--pairs", type=int, default=6, help="rounds of --pair-libs (default 6)")
args = ap.parse_args()
if not args.time and not args.pair_libs and len(args.paths) not in (1, 2):
    ap.error("give one path to dump, two to compare, --time or --pair-libs A B")
if args.pair_libs:
    sys.exit(pair_libs(__file__, METRIC, args.pair_libs[0], args.pair_libs[1], args.pairs, child_timeout=600))

import torch

if len(args.paths) == 2:
    a, b = torch.load(args.paths[0]), torch.load(args.paths[1])
    bad = [k for k in a if a[k] != b.get(k)] + [k for k in b if k not in a]
    print(f"{len(a)} digests compared, {len(bad)} differ: {bad[:8]}")
    sys.exit(1 if bad else 0)

from mla_amd import hip
dev = torch.device("cuda:0")
BF = torch.bfloat16
# the 7B decoder layer's projections, [N, K]
SHAPES = {"qkv": (12288, 4096), "o": (4096, 4096), "gateup": (22016, 4096), "down": (4096, 11008)}
# the single-sample forms each projection is timed in (the suffix pass's own: RMSNorm in front of q|k|v and gate|up, SwiGLU in front of
# down or behind gate|up, and the plain form of suffix_operand="once")
SINGLE = {"qkv": ("plain", "norm"), "o": ("plain",), "gateup": ("plain", "norm", "gateup"), "down": ("plain", "swiglu")}
CACHE_BYTES = 600 << 20                                                     # weight copies per graph: more than the last-level cache


def _rand(shape, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * 0.7).to(BF)


def _weights(proj, w8, copies):
    N, K = SHAPES[proj]
    Ws = [_rand((N, K), 10 * i + len(proj)) * 0.05 for i in range(copies)]
    return [hip.quant_fp8_rows(W) for W in Ws] if w8 else [(W, None) for W in Ws]


def entries(proj, w8, copies):
    """(name, launch(weight copy), out) of every timed form of one projection"""
    N, K = SHAPES[proj]
    Ws = _weights(proj, w8, copies)
    tag = "w8" if w8 else "bf16"
    for M in (2, 17, 48, 64):
        for form in SINGLE[proj]:
            x = _rand((M, 2 * K if form == "swiglu" else K), M)
            if form == "gateup":
                out = torch.empty((M, N // 2), dtype=BF, device=dev)
                fn = (lambda Wc, x=x, out=out: hip.gemm_skinny_gateup_swiglu_w8(x, Wc[0], Wc[1], out)) if w8 else \
                     (lambda Wc, x=x, out=out: hip.gemm_skinny_gateup_swiglu(x, Wc[0], out))
            else:
                out = torch.empty((M, N), dtype=BF, device=dev)
                kw = dict(norm_weight=_rand((K,), 7) if form == "norm" else None, eps=1e-5, swiglu=form == "swiglu")
                fn = (lambda Wc, x=x, out=out, kw=kw, M=M: hip.gemm_skinny_w8(x, Wc[0], Wc[1], out, N, 0, M, **kw)) if w8 else \
                     (lambda Wc, x=x, out=out, kw=kw, M=M: hip.gemm_skinny(x, Wc[0], out, N, 0, M, **kw))
            yield f"skinny_{form}_{proj}_{tag}_M{M}", fn, Ws, out
    for M in (17, 48, 64, 136, 256):
        x, out = _rand((M, K), M), torch.empty((M, N), dtype=BF, device=dev)
        fn = (lambda Wc, x=x, out=out, M=M: hip.gemm_suffix_w8(x, Wc[0], Wc[1], out, N, 0, M)) if w8 else \
             (lambda Wc, x=x, out=out, M=M: hip.gemm_suffix(x, Wc[0], out, N, 0, M))
        yield f"suffix_{proj}_{tag}_M{M}", fn, Ws, out


def _digest(t):
    return hashlib.sha256(t.cpu().view(torch.int16).numpy().tobytes()).hexdigest()


def each_projection(copies_of):
    for proj, (N, K) in SHAPES.items():
        for w8 in (False, True):
            yield from entries(proj, w8, copies_of(N * K * (1 if w8 else 2)))
            torch.cuda.empty_cache()


if args.time:
    us = {name: _us_per_launch(fn, Ws, window_ms=40.0) for name, fn, Ws, _ in each_projection(lambda nbytes: max(2, -(-CACHE_BYTES // nbytes)))}
    print(json.dumps({"metric": "suffix projections per launch, 7B shapes", "unit": "us", "library": hip._LIB_PATH,
                      "us_per_launch": {k: round(v, 3) for k, v in us.items()}, "data": "synthetic"}))
    sys.exit(0)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_infer_proj_golden_gpu as golden
out = {name: digest for family in golden.FAMILIES for name, digest in golden.run(family)}
for name, fn, Ws, o in each_projection(lambda nbytes: 1):                    # the 7B shapes, once
    o.fill_(float("nan"))
    fn(Ws[0])
    out[name] = _digest(o)
torch.save(out, args.paths[0])
print("saved", len(out), "digests")
