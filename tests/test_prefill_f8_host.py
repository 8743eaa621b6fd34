"""CPU: the FP8 prefill's host side -- the `prefill_precision` argument of the samplers, the launch plan of the FP8 prefill GEMMs
(mla_amd/csrc/prefill.hip; hip.plan_gemm_prefill_f8 mirrors the launcher, mla_gemm_prefill_f8_plan is the launcher's own answer), their
argument checks, and the quantiser fact the exact GPU test rests on. Nothing here launches a kernel."""
import ctypes

import pytest
import torch


def test_prefill_precision_is_a_named_argument_and_checked():
    """Validated in front of everything else (no model, no GPU needed to see the error): an unknown value, "fp8" on the "train" prefill
    and "fp8" without the cached prefix are ValueErrors; the batched call refuses everything but "bf16" with NotImplementedError."""
    from mla_amd import infer
    from mla_amd.mla import MLA
    assert infer.MODES["prefill_precision"].values == ("bf16", "fp8", "fp8_as_bf16")
    assert infer.MODES["prefill"].values == ("train", "compact")
    for mode in infer.MODES["prefill_precision"].values:
        infer.check_mode("prefill_precision", mode, prefill="compact")
    infer.check_mode("prefill_precision", "bf16", prefill="train")
    with pytest.raises(ValueError, match="prefill_precision"):
        MLA.predict_action_diff(object(), prefill="compact", prefill_precision="fp16")
    with pytest.raises(ValueError, match="prefill_precision"):
        MLA.predict_action_diff_samples(object(), prefill="compact", prefill_precision="FP8", num_samples=2)
    with pytest.raises(ValueError, match="prefill_precision"):
        MLA.predict_action_diff_batch(object(), [None], [None], prefill_precision="nonsense")
    for mode in ("fp8", "fp8_as_bf16"):
        with pytest.raises(ValueError, match="compact"):
            MLA.predict_action_diff(object(), prefill_precision=mode)                    # prefill="train" is the default
        with pytest.raises(ValueError, match="compact"):
            MLA.predict_action_diff(object(), prefill="train", prefill_precision=mode)
        with pytest.raises(ValueError, match="compact"):
            MLA.predict_action_diff_samples(object(), prefill="train", prefill_precision=mode, num_samples=3)
        with pytest.raises(ValueError, match="compact"):
            infer.check_mode("prefill_precision", mode, prefill="train")
        with pytest.raises(ValueError, match="reuse_prefix=True"):
            MLA.predict_action_diff(object(), prefill="compact", prefill_precision=mode, reuse_prefix=False)
        with pytest.raises(ValueError, match="reuse_prefix=True"):
            MLA.predict_action_diff_samples(object(), prefill="compact", prefill_precision=mode, reuse_prefix=False, num_samples=3)
        with pytest.raises(ValueError):
            MLA.predict_action_diff(object(), prefill_precision=mode, reuse_prefix=False)
        with pytest.raises(NotImplementedError, match="prefill_precision"):
            MLA.predict_action_diff_batch(object(), [None], [None], prefill_precision=mode)
        with pytest.raises(NotImplementedError, match="prefill_precision"):
            MLA.predict_action_diff_batch(object(), [None, None], [None, None], prefill_precision=mode, suffix_weights="fp8", num_samples=2)
    with pytest.raises(ValueError, match="prefill_precision"):
        infer.PrefixCachedEps.for_inputs(object(), None, prefill="compact", prefill_precision="int8")
    with pytest.raises(ValueError, match="compact"):
        infer.PrefixCachedEps.for_inputs(object(), None, prefill_precision="fp8")
    with pytest.raises(ValueError, match="compact"):
        infer.SampleGroupsEps.for_inputs(object(), None, 16, 2, prefill_precision="fp8")


def test_a_precision_mode_has_an_engine_of_its_own():
    """The engine key gains "precision:<mode>" for the non-default modes only: the default call keeps the engine it had."""
    from types import SimpleNamespace
    from mla_amd import infer

    class Eng(infer._CachedEpsBase):
        def __init__(self, vlm, *ctor):
            self.ctor = ctor
    vlm = SimpleNamespace()
    a = Eng._engine(vlm, "store", ("k",), (1,), prefill="compact")
    b = Eng._engine(vlm, "store", ("k",), (2,), prefill="compact", prefill_precision="fp8")
    c = Eng._engine(vlm, "store", ("k",), (3,), prefill="compact", prefill_precision="fp8_as_bf16")
    assert a is not b and b is not c and a is Eng._engine(vlm, "store", ("k",), (1,), prefill="compact", prefill_precision="bf16")
    assert set(vlm.store) == {("k", "prefill:compact"), ("k", "prefill:compact", "precision:fp8"),
                              ("k", "prefill:compact", "precision:fp8_as_bf16")}


def _lib_plan(M, N, K, cus=256):
    from mla_amd import hip
    out = (ctypes.c_int * 4)()
    rc = hip.lib().mla_gemm_prefill_f8_plan(M, N, K, cus, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, hip.lib().mla_last_error()
    return tuple(out)


# (M, N, K) -> (split, workgroups, rows covered, workspace bytes), worked by hand from the rule: 64 x 128 tiles, K tiles of 128, split doubled
# while tiles x split < 512, split < 16 and ktiles // (2 split) >= 8.
#   (545, 12288, 4096): 9 x 96 = 864 tiles >= 512                                         -> no split
#   (545, 4096, 4096):  9 x 32 = 288 tiles, 32 K tiles: 288 < 512 and 32 // 2 = 16 >= 8   -> 2; 576 >= 512 stops
#   (545, 22016, 4096): 9 x 172 = 1548 tiles                                              -> no split
#   (545, 4096, 11008): 288 tiles, 86 K tiles: 86 // 2 = 43 >= 8                          -> 2; 576 >= 512 stops
#   (1, 128, 128):      1 tile, 1 K tile: 1 // 2 = 0 < 8                                  -> no split
HAND_PLANS = {
    (545, 12288, 4096): (1, 864, 576, 0),
    (545, 4096, 4096): (2, 576, 576, 2 * 576 * 4096 * 4),
    (545, 22016, 4096): (1, 1548, 576, 0),
    (545, 4096, 11008): (2, 576, 576, 2 * 576 * 4096 * 4),
    (1, 128, 128): (1, 1, 64, 0),
}


@pytest.mark.parametrize("shape", sorted(HAND_PLANS))
def test_plan_matches_the_hand_worked_plans_and_the_launcher(shape):
    from mla_amd import hip
    M, N, K = shape
    p = hip.plan_gemm_prefill_f8(M, N, K)
    assert (p.tile_m, p.tile_n) == (64, 128)
    assert (p.split, p.workgroups, p.rows_covered, p.ws_bytes) == HAND_PLANS[shape]
    assert (p.tile_m, p.tile_n, p.split, p.workgroups) == _lib_plan(M, N, K)
    assert p.ws_bytes == hip.gemm_prefill_f8_ws_bytes(M, N, K)
    assert bool(p.note) == (p.workgroups < 256)


@pytest.mark.parametrize("M", [1, 64, 65, 545, 1024])
@pytest.mark.parametrize("N,K", [(128, 128), (256, 384), (128, 256), (256, 4096), (128, 11008), (768, 256), (1024, 256), (256, 512)])
def test_plan_is_the_launchers(M, N, K):
    """The pure-Python plan and the library's launcher agree at the row-count edges, for 256 CUs and for another count."""
    from mla_amd import hip
    p = hip.plan_gemm_prefill_f8(M, N, K)
    assert (p.tile_m, p.tile_n, p.split, p.workgroups) == _lib_plan(M, N, K)
    assert p.ws_bytes == hip.gemm_prefill_f8_ws_bytes(M, N, K)
    q = hip.plan_gemm_prefill_f8(M, N, K, cus=64)
    assert (q.tile_m, q.tile_n, q.split, q.workgroups) == _lib_plan(M, N, K, 64) and q.split <= p.split
    if p.split > 1:
        assert (K // 128) // p.split >= 8 and p.split <= 16              # every slice keeps at least 8 K tiles


def test_the_gpu_tests_split_shapes_split():
    from mla_amd import hip
    assert hip.plan_gemm_prefill_f8(545, 256, 4096).split == 4           # 18 tiles, 32 K tiles: 32 // 8 = 4 < 8 stops at 4
    p = hip.plan_gemm_prefill_f8(64, 128, 11008)                         # 1 tile, 86 K tiles: 86 // 16 = 5 < 8 stops at 8
    assert p.split == 8 and -(-86 // 8) * 7 < 86 < -(-86 // 8) * 8       # slices of 11 K tiles, the last one holds 9
    assert hip.plan_gemm_prefill_f8(65, 256, 384).split == 1 and hip.plan_gemm_prefill_f8(129, 128, 256).split == 1


def test_shapes_outside_the_contract_are_refused():
    from mla_amd import hip
    assert hip.gemm_prefill_f8_fits(1024, 4096, 4096) and hip.gemm_prefill_f8_fits(1, 128, 128)
    assert hip.gemm_prefill_f8_fits(545, 22016, 4096) and hip.gemm_prefill_f8_fits(545, 4096, 11008)       # 7B: 11008 = 86 x 128
    assert hip.gemm_prefill_f8_fits(20, 1024, 256) and hip.gemm_prefill_f8_fits(20, 256, 512)              # the tiny model
    for M, N, K in ((0, 4096, 4096), (1025, 4096, 4096), (545, 192, 4096), (545, 4096, 192)):
        assert not hip.gemm_prefill_f8_fits(M, N, K)
        with pytest.raises(ValueError, match="1 <= M <= 1024"):
            hip.plan_gemm_prefill_f8(M, N, K)
        assert hip.gemm_prefill_f8_ws_bytes(M, N, K) == -1
        out = (ctypes.c_int * 4)()
        assert hip.lib().mla_gemm_prefill_f8_plan(M, N, K, 256, ctypes.cast(out, ctypes.c_void_p)) < 0
        assert b"K % 128 == 0" in hip.lib().mla_last_error()


def test_launchers_check_their_arguments_on_the_host():
    """Argument validation happens before any launch -> safe without a GPU (the pointers are never dereferenced)."""
    from mla_amd import hip
    lib = hip.lib()
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    ok = dict(M=545, N=256, K=4096)

    def plain(x=P, xs=P, W=P, wsc=P, out=P, res=None, ws=P, ws_bytes=1 << 40, ldo=256, ldx=None, **kw):
        d = ok | kw
        return lib.mla_gemm_prefill_f8(x, d["K"] if ldx is None else ldx, xs, W, d["K"], wsc, out, ldo, 0, d["M"], res, 256, d["M"], d["N"],
                                       d["K"], ws, ws_bytes, None)
    need = hip.gemm_prefill_f8_ws_bytes(545, 256, 4096)
    assert need == 4 * 576 * 256 * 4
    assert plain(M=1025) == -1 and b"1 <= M <= 1024" in lib.mla_last_error()
    assert plain(M=0) == -1 and b"1 <= M <= 1024" in lib.mla_last_error()
    assert plain(K=192) == -1 and b"K % 128 == 0" in lib.mla_last_error()
    assert plain(N=192) == -1 and b"N % 128 == 0" in lib.mla_last_error()
    assert plain(x=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(xs=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(wsc=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(out=Q) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(ldo=260) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(ldx=4096 + 8) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(res=Q) == -1 and b"residual" in lib.mla_last_error()
    assert plain(ws_bytes=need - 1) == -1 and b"workspace" in lib.mla_last_error()
    assert plain(ws=None) == -1 and b"workspace" in lib.mla_last_error()

    def rope(cos=P, sin=P, rope_cols=128, head_dim=128):
        return lib.mla_gemm_prefill_f8_qkv_rope(P, 256, P, P, 256, P, P, 384, 0, 65, 130, 384, 256, cos, sin, rope_cols, head_dim, None, 0, None)
    assert rope(head_dim=64) == -1 and b"head_dim must be 128" in lib.mla_last_error()
    assert rope(rope_cols=64) == -1 and b"rope_cols" in lib.mla_last_error()
    assert rope(rope_cols=512) == -1 and b"rope_cols" in lib.mla_last_error()
    assert rope(sin=None) == -1 and b"tables" in lib.mla_last_error()
    rc = lib.mla_gemm_prefill_f8_gateup_swiglu(P, 256, P, P, 256, P, P, 96, 0, 65, 65, 96, 256, None, 0, None)
    assert rc == -1 and b"I % 64 == 0" in lib.mla_last_error()


def test_the_quantiser_statement_keeps_integer_rows_with_amax_448():
    """hip.quant_fp8_rows's CPU statement on integer-valued rows whose amax is 448: scale = 448 / 448 = 1 and every small integer is an
    e4m3 value, so the codes ARE the integers -- which lets the GPU test feed exact integer codes and expect exact integer sums."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (7, 64), generator=g).float()
    x[:, 0] = 448.0
    x[3, 0] = -448.0
    xb = x.to(torch.bfloat16)
    assert torch.equal(xb.float(), x)
    s = xb.float().abs().amax(dim=1) / 448.0
    assert bool((s == 1.0).all())
    q = (xb.float() / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), x)
    assert torch.equal((q.float() * s[:, None]).to(torch.bfloat16), xb)
    # and every integer in [-8, 8] -- the GPU test's codes -- is an e4m3fn value
    r = torch.arange(-8, 9).float()
    assert torch.equal(r.to(torch.float8_e4m3fn).float(), r)
