"""The hand-scheduled main loop of gemm256 on reduction-major operands (gemm256_kloop_rm<a><b>.inc, gemm256_kernel<AM, BM_, 0, true>):
the generated files are what the generator writes and keep the loop's shape (CPU); on the GPU the loop gives the bits of the
compiler-scheduled loop of the same modes on every output form the wgrad uses, agrees with an fp64 product of the bf16 inputs within the
bounds of test_kernels_gpu.py::test_gemm256_modes (fp32: Frobenius-relative 2e-4, max-relative 1e-3; bf16: Frobenius-relative 4e-3),
and repeats bit for bit."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import fro_rel, max_rel, poison_free_memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
MODES = [(1, 1), (1, 0), (0, 1)]


def bfr(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def test_reduction_major_loops_are_what_the_generator_writes(tmp_path):
    """Committed gemm256_kloop_rm*.inc == the generator's output; the loop body keeps the properties of the k-contiguous loop: three
    barriers per K-tile, no vmcnt(0), 8 loads per K-tile, at most two non-MFMA instructions per MFMA gap; a reduction-major side reads
    every fragment with two ds_read_b64_tr_b16 and no ds_read_b128."""
    env = dict(os.environ, GEN_OUT_DIR=str(tmp_path))
    for k in ("GEN256_FLAGS", "GEN8W_FLAGS", "GEN4W_FLAGS"):
        env.pop(k, None)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gemm_asm.py")], check=True, env=env, capture_output=True)
    for n in ["gemm256_kloop_rm11.inc", "gemm256_kloop_rm10.inc", "gemm256_kloop_rm01.inc", "gemm256_kloop_rm_clobbers.inc"]:
        assert open(tmp_path / n).read() == open(os.path.join(ROOT, "mla_amd", "csrc", n)).read(), f"{n}: run python tools/gen_gemm_asm.py"
    for am, bm in MODES:
        body = [ln.strip('"\\n \n') for ln in open(tmp_path / f"gemm256_kloop_rm{am}{bm}.inc") if ln.startswith('"')]
        loop = body[body.index("1:") + 1:body.index("4:")]          # two K-tiles per iteration
        assert sum(ln == "s_barrier" for ln in loop) == 6 and not any(ln.startswith("s_waitcnt vmcnt(0)") for ln in loop)
        assert sum(ln.startswith("v_mfma") for ln in loop) == 128 and sum(ln.startswith("global_load_lds") for ln in loop) == 16
        # per K-tile and wave: 16 A fragments + 8 B fragments; two transposed reads per fragment of a reduction-major side
        assert sum(ln.startswith("ds_read_b64_tr_b16") for ln in loop) == 2 * 2 * (16 * am + 8 * bm)
        assert sum(ln.startswith("ds_read_b128") for ln in loop) == 2 * (16 * (1 - am) + 8 * (1 - bm))
        gap = worst = 0
        for ln in loop:
            if ln.startswith("v_mfma"):
                gap = 0
            elif not ln.startswith((";", "s_sub_u32 s46", "s_cmp", "s_cbranch")):
                gap += 1
                worst = max(worst, gap)
        assert worst <= 2, worst


@pytest.fixture(scope="module")
def cases(dev):
    """(label, M, N, K, planned CUs): two K-tiles; an odd number of K-tile pairs; ragged edge tiles in both directions; 9 tiles on 8
    planned CUs at K = 512 (a ninth tile in a second round: the launch keeps >= 8 K-tiles per slice, so 8 K-tiles are NOT split) and at
    K = 1024, where the ninth tile IS cut into two K-slices of 8 K-tiles (asserted below: 8 + 64 sum-of-squares partials).
    Operands and the fp64 product are made once per shape."""
    out = {}
    for label, M, N, K, cus in (("k128", 256, 256, 128, 0), ("k384", 256, 256, 384, 0), ("ragged", 320, 264, 128, 0),
                                ("tail9", 768, 768, 512, 8), ("splitk", 768, 768, 1024, 8)):
        a, b = bfr(M, K, seed=11), bfr(N, K, seed=12, scale=0.1)
        out[label] = dict(M=M, N=N, K=K, cus=cus, a=a.to(dev), b=b.to(dev), ref=(a.double() @ b.double().t()).float(),
                          base=(torch.randn(M, N, generator=torch.Generator().manual_seed(13)) * 0.1).to(dev))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("am,bm", MODES)
@pytest.mark.parametrize("label", ["k128", "k384", "ragged", "tail9", "splitk"])
def test_rm_assembly_loop_is_the_compiler_loop_bit_for_bit(dev, cases, label, am, bm):
    from mla_amd import hip
    c = cases[label]
    M, N = c["M"], c["N"]
    aa = c["a"] if am == 0 else c["a"].t().contiguous()
    bb = c["b"] if bm == 0 else c["b"].t().contiguous()

    def run():
        poison_free_memory(0.25)
        out = {"bf16": hip.gemm(aa, bb, a_mode=am, b_mode=bm), "f32": hip.gemm(aa, bb, a_mode=am, b_mode=bm, out_dtype=torch.float32)}
        acc = c["base"].clone()
        hip.gemm(aa, bb, out=acc, a_mode=am, b_mode=bm, accumulate=True)
        out["acc"] = acc
        for accumulate in (False, True):        # the wgrad call: fp32 into the gradient buffer + sum-of-squares partials
            o = c["base"].clone()
            r = hip.gemm_sq(aa, bb, o, accumulate, a_mode=am, b_mode=bm)
            assert r is not None
            if label == "splitk":       # the tail was split: 8 whole tiles + 64 fix-up workgroups of the ninth (unsplit: 9 partials)
                assert r[1] == 8 + 64, r[1]
            out[f"sq_out{int(accumulate)}"], out[f"sq_part{int(accumulate)}"] = o, r[0][:r[1]].clone()
        return out

    prev_loop, prev_cus = hip.gemm_kloop(-1), hip.gemm_cus(-1)
    try:
        if c["cus"]:
            assert hip.gemm_cus(c["cus"]) == c["cus"]
        assert hip.gemm_kloop(1) == 1
        asm, again = run(), run()
        assert hip.gemm_kloop(0) == 0
        ref = run()
    finally:
        hip.gemm_kloop(prev_loop)
        hip.gemm_cus(prev_cus if prev_cus >= 8 and prev_cus % 8 == 0 else 0)
    for k in ref:
        assert torch.equal(asm[k], ref[k]), (k, float((asm[k].float() - ref[k].float()).abs().max()))
        assert torch.equal(asm[k], again[k]), k
    want = c["ref"]
    assert fro_rel(asm["f32"], want) < 2e-4 and max_rel(asm["f32"], want) < 1e-3
    assert fro_rel(asm["bf16"], want) < 4e-3
    assert fro_rel(asm["acc"], want + c["base"].cpu()) < 2e-4
    assert torch.equal(asm["sq_out1"], asm["acc"]) and torch.equal(asm["sq_out0"], asm["f32"])
    sq = float(asm["sq_part1"].double().sum())
    assert abs(sq - float(asm["acc"].double().pow(2).sum())) <= 1e-5 * sq


@pytest.mark.gpu
@pytest.mark.parametrize("kloop", [1, 0])
def test_dact_swiglu_bwd_without_the_transposed_output(dev, kloop):
    """mla_gemm_dact_swiglu_bwd with a null dguT (the wgrad reads dgu as stored): dgu is bit for bit the dgu of the launch that also
    writes dgu^T, on both main loops; T = 320 (a ragged second row tile), I = 512, K = 128."""
    from mla_amd import hip
    T, I, K = 320, 512, 128
    dy, wT, gu = bfr(T, K, seed=21).to(dev), bfr(I, K, seed=22, scale=0.1).to(dev), bfr(T, 2 * I, seed=23).to(dev)
    prev = hip.gemm_kloop(-1)
    try:
        assert hip.gemm_kloop(kloop) == kloop
        poison_free_memory(0.25)
        both = hip.gemm_dact_swiglu_bwd(dy, wT, gu)
        only = hip.gemm_dact_swiglu_bwd(dy, wT, gu, want_t=False)
    finally:
        hip.gemm_kloop(prev)
    assert both is not None and only is not None and only[1] is None
    assert torch.equal(only[0], both[0]) and torch.equal(both[1], both[0].t())
    assert not bool(torch.isnan(only[0].float()).any())


@pytest.mark.gpu
def test_rmsnorm_apply_is_the_forward_bit_for_bit(dev):
    """mla_rmsnorm_apply (the normalised input rebuilt row-major from the SAVED rstd, for MLA_WGRAD_RM = 1): the bits of mla_rmsnorm_fwd,
    and the transpose of mla_rmsnorm_apply_t; rows not a multiple of the block's chunk count, H = 512."""
    from mla_amd import hip
    x, w = bfr(197, 512, seed=31).to(dev), (1.0 + 0.1 * bfr(512, seed=32).float()).to(BF).to(dev)
    y, rstd = hip.rmsnorm_fwd(x, w, 1e-5)
    got = hip.rmsnorm_apply(x, w, rstd)
    assert torch.equal(got, y)
    x8 = x[:192].contiguous()
    assert torch.equal(hip.rmsnorm_apply_t(x8, w, rstd[:192].contiguous()).t(), got[:192])


# ---------------------------------------------------------------------------------------------- decoder layer, MLA_WGRAD_RM
LAYER_NAMES = ["input_layernorm.weight", "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
               "self_attn.o_proj.weight", "post_attention_layernorm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
               "mlp.down_proj.weight"]
LH, LI, LNH, LB, LS = 512, 1024, 4, 2, 64          # 2 x 64 tokens: the wgrad reduction is 128 = two K-tiles of the 256x256 kernel


@pytest.fixture(scope="module")
def layer_ref():
    """Inputs of the tiny layer and the fp32 oracle's gradients, dense and ragged; made once."""
    from oracle import recipe
    from oracle import torch_oracle as O
    shapes = [(LH,), (LH, LH), (LH, LH), (LH, LH), (LH, LH), (LH,), (LI, LH), (LI, LH), (LH, LI)]
    p32 = {n: recipe.det_weight("layer." + n, s).to(BF).float() for n, s in zip(LAYER_NAMES, shapes)}
    x = recipe.det_randn("x", (LB, LS, LH), 1.0).to(BF)
    dy = recipe.det_randn("dy", (LB, LS, LH), 1.0).to(BF)
    cos, sin = O.rope_tables(LS, LH // LNH)
    grads = {}
    for key, lens in (("dense", None), ("ragged", [64, 37])):
        seqlens = torch.tensor(lens) if lens else None
        xr = x.float().requires_grad_(True)
        pr = {n: v.clone().requires_grad_(True) for n, v in p32.items()}
        O.decoder_layer(xr, pr, cos, sin, LNH, 1e-5, seqlens).backward(dy.float())
        grads[key] = (seqlens, {n: pr[n].grad for n in LAYER_NAMES})
    return p32, x, dy, cos, sin, grads


def _run_layer(dev, layer_ref, save_level, key, spec, record=None):
    from mla_amd import ops
    p32, x, dy, cos, sin, grads = layer_ref
    seqlens = grads[key][0]
    prev = ops.set_wgrad_rm(spec)
    real_empty = torch.empty
    try:
        xd = x.to(dev).requires_grad_(True)
        wd = [p32[n].to(BF).to(dev).requires_grad_(True) for n in LAYER_NAMES]
        out = ops.decoder_layer(xd, seqlens.to(dev).int() if seqlens is not None else None, cos.to(dev), sin.to(dev), LNH, 1e-5, save_level, wd)
        if record is not None:           # allocation bookkeeping of the backward: every torch.empty the wrappers issue
            def rec_empty(*a, **k):
                t = real_empty(*a, **k)
                record.append(tuple(t.shape))
                return t
            torch.empty = rec_empty
        out.backward(dy.to(dev))
    finally:
        torch.empty = real_empty
        ops.set_wgrad_rm(prev)
    return out.detach(), xd.grad, {n: w.grad for n, w in zip(LAYER_NAMES, wd)}


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["dense", "ragged"])
@pytest.mark.parametrize("save_level", [0, 1, 2])
def test_decoder_layer_wgrad_rm_on_is_off_bit_for_bit(dev, layer_ref, save_level, key):
    """MLA_WGRAD_RM all-on and the shipped default against all-off: the switch changes only the operands of the weight-gradient GEMMs,
    and the generated loop keeps the k-slot map and K order of the k-contiguous one, so EVERYTHING is bit-equal -- output, dh, norm-weight
    gradients and the weight gradients themselves (maximum on-vs-off difference per weight: 0). Each weight gradient also meets the fp32
    oracle within the bound of test_model_gpu.py::test_decoder_layer_fwd_bwd (Frobenius-relative 2e-2). With the switch all-on the
    backward allocates no transposed activation buffer ([H, T], [I, T], [2I, T], [3H, T])."""
    from mla_amd import ops
    off = _run_layer(dev, layer_ref, save_level, key, "0")
    rec = []
    on = _run_layer(dev, layer_ref, save_level, key, "1", record=rec)
    dflt = _run_layer(dev, layer_ref, save_level, key, dict(ops._parse_wgrad_rm(os.environ.get("MLA_WGRAD_RM", "wd=1,wgu=a,wo=a"))))
    T = LB * LS
    transposed = [s for s in rec if s in ((LH, T), (LI, T), (2 * LI, T), (3 * LH, T))]
    assert not transposed, transposed
    rec_off = []
    _run_layer(dev, layer_ref, save_level, key, "0", record=rec_off)      # the bookkeeping sees today's copies: it is not blind
    assert any(s in ((LH, T), (LI, T), (2 * LI, T), (3 * LH, T)) for s in rec_off)
    want = layer_ref[5][key][1]
    for got in (on, dflt):
        assert torch.equal(got[0], off[0]) and torch.equal(got[1], off[1])
        for n in LAYER_NAMES:
            assert torch.equal(got[2][n], off[2][n]), (n, float((got[2][n].float() - off[2][n].float()).abs().max()))
    for n in LAYER_NAMES:
        assert fro_rel(on[2][n], want[n]) < 2e-2, n
