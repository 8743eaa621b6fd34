"""The bits of the cached-prefix sampler's projections (gemv, gemm_skinny, gemm_skinny_gateup_swiglu, gemm_suffix; bf16 and FP8 weights),
pinned from outside the code under test.

tests/golden/infer_proj_digests.json was recorded on an MI355X (`PYTHONPATH=. python tests/test_infer_proj_golden_gpu.py --record`) from
the commit that adds this file, where gemm_skinny_kernel and gemm_suffix_kernel (infer.hip) are two kernels kept equal by hand. It is the
anchor for folding them: once the skinny and the suffix entry points launch the same kernel, the tests that compare one with the other
compare a kernel with itself, and this record is what ties both to the arithmetic they have as two. Only mla_amd.hip's public wrappers
are called, so the file runs unchanged on either side of such a change; re-record only on a commit whose bits are meant to change.

A case: inputs from a seeded CPU generator (randn -> bf16 -> device; FP8 weights by the CPU statement hip.quant_fp8_rows documents, so no
kernel sits between the seed and the operand), an output buffer pre-filled with bf16 NaN, and the sha256 of the WHOLE buffer behind the
call -- guard rows, guard columns and rows the kernel must not write included. The shapes are the smallest at which each form can go
wrong: every x-block count and both block edges, waves without a K step (K 48), a ragged last step (528), more than one batch of steps in
flight per wave (4112), a ragged last W tile (N 7) and more than one workgroup (520), all seven launch forms of the suffix entry."""
import functools
import hashlib
import json
import os

import pytest
import torch

from mla_amd import hip

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer_proj_digests.json")
BF = torch.bfloat16
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _cpu(tag, *shape):
    """bf16 standard normals of a seed that depends on (tag, shape) alone"""
    seed = int.from_bytes(hashlib.sha256(repr((tag, shape)).encode()).digest()[:4], "little")
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF)


@functools.lru_cache(maxsize=None)
def _dev(tag, *shape):
    return _cpu(tag, *shape).cuda()


@functools.lru_cache(maxsize=None)
def _weights(w8, N, K):
    """(W, w_scale or None) on the device; FP8: quant_fp8_rows' CPU statement on the bf16 matrix"""
    W = _cpu("W", N, K)
    if not w8:
        return W.cuda(), None
    amax = W.float().abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    q = (W.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q.cuda(), scale.cuda()


@functools.lru_cache(maxsize=None)
def _tables(rows):
    g = torch.Generator().manual_seed(1000 + rows)
    ang = torch.rand(rows, 64, generator=g) * 6.2831853
    return ang.cos().cuda(), ang.sin().cuda()


def _nan(n):
    return torch.full((n,), float("nan"), dtype=BF, device="cuda")


def _digest(buf):
    return hashlib.sha256(buf.cpu().view(torch.int16).numpy().tobytes()).hexdigest()


def _single(fn, fn_w8, w8, M, N, K, pre, res, rope_cols=0, rpb=None, out_col=0):
    """gemv / gemm_skinny and their _w8 forms: one argument list"""
    W, ws = _weights(w8, N, K)
    x = _dev("x", 64, 2 * K if pre == 2 else K)[:M]
    rpb = M if rpb is None else rpb
    nb = -(-M // rpb)
    ldo = N + out_col + 3                                                    # guard columns behind every row
    obs = (rpb + 2) * ldo + 16 if nb > 1 else 0                              # guard rows behind every sample
    out = _nan((nb - 1) * obs + (rpb + 2) * ldo)
    kw = dict(residual=_dev("res", 64, N)[:M] if res else None, out_col=out_col, norm_weight=_dev("nw", K) if pre == 1 else None, eps=EPS,
              swiglu=pre == 2, rope=_tables(rpb) + (rope_cols,) if rope_cols else None)
    if w8:
        fn_w8(x, W, ws, out, ldo, obs, rpb, **kw)
    else:
        fn(x, W, out, ldo, obs, rpb, **kw)
    return _digest(out)


def _single_cases(family, fn, fn_w8, Ms, Ks, qkv_Ms):
    for w8 in (False, True):
        for M in Ms:
            for pre in (0, 1, 2):
                for res in (False, True):
                    for K in Ks:
                        for N in (7, 520):
                            yield f"{family} w8={w8} M={M} pre={pre} res={res} K={K} N={N}", lambda a=(w8, M, N, K, pre, res): _single(fn, fn_w8, *a)
        # the fused q|k|v form: rotary columns [0, 256) of N = 384, several samples of rows_per_batch < M rows, a strided batch
        for M in qkv_Ms:
            for pre in (0, 1):
                for K in Ks[:2]:
                    rpb = max(1, (M + 2) // 3)
                    yield (f"{family} w8={w8} qkv M={M} pre={pre} K={K} rpb={rpb}",
                           lambda a=(w8, M, 384, K, pre, False, 256, rpb): _single(fn, fn_w8, *a))
        yield f"{family} w8={w8} out_col=5", lambda w8=w8: _single(fn, fn_w8, w8, Ms[-1] // 2 + 1, 7, 528, 0, True, out_col=5)


def skinny_cases():
    yield from _single_cases("skinny", hip.gemm_skinny, hip.gemm_skinny_w8, (1, 16, 17, 33, 64), (48, 528, 4112), (1, 16, 17, 33, 64))


def gemv_cases():
    yield from _single_cases("gemv", hip.gemv, hip.gemv_w8, (1, 8), (48, 528), (1, 8))


def _gateup(w8, M, I, K, ldo):
    W, ws = _weights(w8, 2 * I, K)
    x = _dev("x", 64, K)[:M]
    out = _nan((M + 2) * ldo)
    if w8:
        hip.gemm_skinny_gateup_swiglu_w8(x, W, ws, out, ldo)
    else:
        hip.gemm_skinny_gateup_swiglu(x, W, out, ldo)
    return _digest(out)


def gateup_cases():
    for w8 in (False, True):
        for M in (1, 16, 17, 33, 64):
            for I in (8, 264):
                for K in (48, 528):
                    yield f"gateup w8={w8} M={M} I={I} K={K}", lambda a=(w8, M, I, K, I): _gateup(*a)
        yield f"gateup w8={w8} ldo>I", lambda w8=w8: _gateup(w8, 33, 264, 528, 264 + 6)


def _suffix(w8, M, N, K, res, form=None):
    """form None: one sample of M rows; "slot": ragged q|k|v rows at slot[b]; "pos": the same with separate rotary positions"""
    W, ws = _weights(w8, N, K)
    x = _dev("x", 256, K)[:M]
    fn = (lambda *a, **k: hip.gemm_suffix_w8(a[0], a[1], ws, *a[2:], **k)) if w8 else hip.gemm_suffix
    ldo = N + 3
    if form is None:
        out = _nan((M + 2) * ldo)
        fn(x, W, out, ldo, 0, M, residual=_dev("res", 256, N)[:M] if res else None)
        return _digest(out)
    rpb, cap, rope_rows = 17, 40, 30
    nb = -(-M // rpb)
    obs = (cap + 2) * ldo + 16
    out = _nan(nb * obs)
    # sample 1's rows run past cap_rows, the last sample's begin in front of row 0: neither part is written
    slot = [(7 * b) % (cap - rpb + 1) for b in range(nb)]
    pos = [(5 * b) % (rope_rows - rpb + 1) for b in range(nb)]
    if nb > 1:
        slot[1] = cap - 5
    if nb > 2:
        slot[-1] = -4
        pos[2] = rope_rows - 3                                               # positions past the tables: those rows are not written
    if nb > 3:
        pos[3] = -2
    kw = dict(slot=torch.tensor(slot, dtype=torch.int32, device="cuda"), cap_rows=cap)
    if form == "pos":
        kw.update(rope_pos=torch.tensor(pos, dtype=torch.int32, device="cuda"), rope_rows=rope_rows)
    fn(x, W, out, ldo, obs, rpb, rope=_tables(rope_rows if form == "pos" else cap) + (256,), **kw)
    return _digest(out)


def suffix_cases():
    for w8 in (False, True):
        for M in (1, 17, 48, 64, 65, 96, 97, 128, 129, 256):
            for K in (48, 528):
                for N in (7, 520):
                    for res in (False, True):
                        yield f"suffix w8={w8} M={M} K={K} N={N} res={res}", lambda a=(w8, M, N, K, res): _suffix(*a)
            for form in ("slot", "pos"):
                yield f"suffix w8={w8} M={M} qkv {form}", lambda a=(w8, M, 384, 528, False, form): _suffix(*a)


FAMILIES = {"skinny": skinny_cases, "gateup": gateup_cases, "suffix": suffix_cases, "gemv": gemv_cases}


def run(family):
    got = [(name, case()) for name, case in FAMILIES[family]()]
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("family", list(FAMILIES))
def test_digests_are_the_recorded_ones(family):
    with open(GOLDEN) as f:
        golden = json.load(f)[family]
    got = run(family)
    assert [name for name, _ in got] == [name for name, _ in golden], "the generated cases are the recorded ones, in order, none dropped"
    wrong = [name for (name, digest), (_, want) in zip(got, golden) if digest != want]
    assert len(got) == len(golden) and not wrong, f"{len(wrong)} of {len(got)} cases differ from the record; the first: {wrong[:5]}"


def test_the_record_covers_what_it_is_meant_to():
    """The record itself: every family in both weight formats, and no two cases of a family with one digest (a buffer nobody wrote, or
    a case that ignores one of its parameters, would repeat)."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden) == set(FAMILIES)
    for family, cases in golden.items():
        names, digests = [n for n, _ in cases], [d for _, d in cases]
        assert len(names) == len(list(FAMILIES[family]())) and len(set(names)) == len(names)
        assert any("w8=True" in n for n in names) and any("w8=False" in n for n in names)
        assert len(set(digests)) == len(digests), family


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"], "usage: PYTHONPATH=. python tests/test_infer_proj_golden_gpu.py --record (on the parent commit, on the GPU)"
    record = {family: [[name, digest] for name, digest in run(family)] for family in FAMILIES}
    with open(GOLDEN, "w") as f:
        json.dump(record, f, separators=(",", ":"))
    print({family: len(record[family]) for family in record})
