"""CPU: the host side of the wide-row FP8 prefill -- the launch plan of mla_gemm_prefill_f8_wide* (mla_amd/csrc/prefill.hip;
hip.plan_gemm_prefill_f8_wide mirrors the launcher, mla_gemm_prefill_f8_wide_plan is the launcher's own answer), their argument checks,
the `batch_prefill` argument of MLA.predict_action_diff_batch and the engine key. Nothing here launches a kernel."""
import ctypes

import pytest

NK = [(128, 128), (256, 384), (128, 256), (256, 4096), (128, 11008), (768, 256), (1024, 256), (256, 512)]   # test_prefill_f8_host.py's
SEVEN_B = {"qkv": (12288, 4096), "o": (4096, 4096), "gate|up": (22016, 4096), "down": (4096, 11008)}


def _lib_plan(M, N, K, cus=256):
    from mla_amd import hip
    out = (ctypes.c_int * 4)()
    rc = hip.lib().mla_gemm_prefill_f8_wide_plan(M, N, K, cus, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, hip.lib().mla_last_error()
    return tuple(out)


@pytest.mark.parametrize("M", [1, 64, 1024, 1025, 1090, 2180, 4360, 65536])
@pytest.mark.parametrize("N,K", NK + sorted(SEVEN_B.values()))
def test_plan_is_the_launchers(M, N, K):
    """The pure-Python plan and the library's launcher agree at the row-count edges, for 256 CUs and for 64 CUs."""
    from mla_amd import hip
    p = hip.plan_gemm_prefill_f8_wide(M, N, K)
    assert (p.tile_m, p.tile_n, p.split, p.workgroups) == _lib_plan(M, N, K)
    assert p.ws_bytes == hip.gemm_prefill_f8_wide_ws_bytes(M, N, K)
    assert p.tile_m in (64, 128) and p.rows_covered == -(-M // p.tile_m) * p.tile_m
    assert p.ws_bytes == (p.split * p.rows_covered * N * 4 if p.split > 1 else 0)
    q = hip.plan_gemm_prefill_f8_wide(M, N, K, cus=64)
    assert (q.tile_m, q.tile_n, q.split, q.workgroups) == _lib_plan(M, N, K, 64) and q.split <= p.split
    if p.split > 1:
        assert (K // 128) // p.split >= 8 and p.split <= 16              # every slice keeps at least 8 K tiles


# The rule: row tile 128 when M > 1024 and ceil(M / 128) * (N / 128) >= 3 * 256, else 64 (the threshold started at 2 * 256; the measured
# per-launch table moved it: 576 tiles of 128 rows lose against 1120 of 64 rows, from 864 on they win); on the chosen tile the compact
# split rule (doubled while tiles x split < 512, split < 16 and ktiles // (2 split) >= 8).
#   M = 1090: 9 row tiles of 128, 18 of 64
#     qkv      9 x 96  = 864  >= 768 -> 128, no split, 864 workgroups
#     o        9 x 32  = 288  <  768 -> 64: 18 x 32 = 576 >= 512 -> no split, 576 workgroups
#     gate|up  9 x 172 = 1548        -> 128, no split
#     down     9 x 32  = 288         -> 64: 576 tiles -> no split
#   M = 2180: 18 row tiles of 128 (17.03), 35 of 64 (34.06)
#     qkv      18 x 96  = 1728       -> 128
#     o        18 x 32  = 576 < 768  -> 64: 35 x 32 = 1120 tiles -> no split, 2240 rows covered
#     gate|up  18 x 172 = 3096       -> 128
#     down     576                   -> 64: 1120 tiles -> no split
HAND_PLANS = {  # (M, projection) -> (row tile, split, workgroups, rows covered, workspace bytes)
    (1090, "qkv"): (128, 1, 864, 1152, 0),
    (1090, "o"): (64, 1, 576, 1152, 0),
    (1090, "gate|up"): (128, 1, 1548, 1152, 0),
    (1090, "down"): (64, 1, 576, 1152, 0),
    (2180, "qkv"): (128, 1, 1728, 2304, 0),
    (2180, "o"): (64, 1, 1120, 2240, 0),
    (2180, "gate|up"): (128, 1, 3096, 2304, 0),
    (2180, "down"): (64, 1, 1120, 2240, 0),
}


@pytest.mark.parametrize("case", sorted(HAND_PLANS))
def test_plan_matches_the_hand_worked_plans_of_the_7b_projections(case):
    from mla_amd import hip
    M, (N, K) = case[0], SEVEN_B[case[1]]
    p = hip.plan_gemm_prefill_f8_wide(M, N, K)
    assert (p.tile_m, p.split, p.workgroups, p.rows_covered, p.ws_bytes) == HAND_PLANS[case]
    assert (p.tile_m, p.tile_n, p.split, p.workgroups) == _lib_plan(M, N, K)


@pytest.mark.parametrize("M", [1, 64, 65, 545, 1024])
@pytest.mark.parametrize("N,K", NK + sorted(SEVEN_B.values()))
def test_up_to_1024_rows_the_wide_plan_is_the_compact_plan(M, N, K):
    """Same tile, split, workgroups and workspace as mla_gemm_prefill_f8*: the wide entry points then launch the same kernel instantiation
    over the same slices, hence the same bits (tests/test_prefill_f8_wide_gpu.py compares them)."""
    from mla_amd import hip
    assert hip.plan_gemm_prefill_f8_wide(M, N, K) == hip.plan_gemm_prefill_f8(M, N, K)
    assert hip.plan_gemm_prefill_f8_wide(M, N, K, cus=64) == hip.plan_gemm_prefill_f8(M, N, K, cus=64)
    assert hip.gemm_prefill_f8_wide_ws_bytes(M, N, K) == hip.gemm_prefill_f8_ws_bytes(M, N, K)


def test_a_128_row_plan_never_splits_under_this_rule():
    """The 128-row tile is chosen once its tiles alone reach 3 x CUs; the split rule stops doubling at 2 x CUs: a 128-row plan has
    split 1 and no workspace (the 64-row plan of the same shape would not split either, so both tiles sum every output's K tiles in
    the same order)."""
    from mla_amd import hip
    seen = set()
    for M in (1025, 1090, 1605, 2049, 2180, 4360, 8192, 65536):
        for N, K in NK + sorted(SEVEN_B.values()) + [(11008, 128), (9856, 384)]:
            for cus in (64, 256):
                p = hip.plan_gemm_prefill_f8_wide(M, N, K, cus)
                seen.add(p.tile_m)
                if p.tile_m == 128:
                    assert p.split == 1 and p.ws_bytes == 0 and p.workgroups >= 3 * cus and M > 1024
                else:
                    assert -(-M // 128) * (N // 128) < 3 * cus
    assert seen == {64, 128}


def test_shapes_outside_the_contract_are_refused():
    from mla_amd import hip
    assert hip.gemm_prefill_f8_wide_fits(65536, 4096, 4096) and hip.gemm_prefill_f8_wide_fits(1, 128, 128)
    assert hip.gemm_prefill_f8_wide_fits(1025, 4096, 4096) and not hip.gemm_prefill_f8_fits(1025, 4096, 4096)
    for M, N, K in ((0, 4096, 4096), (65537, 4096, 4096), (2180, 192, 4096), (2180, 4096, 192)):
        assert not hip.gemm_prefill_f8_wide_fits(M, N, K)
        with pytest.raises(ValueError, match="1 <= M <= 65536"):
            hip.plan_gemm_prefill_f8_wide(M, N, K)
        assert hip.gemm_prefill_f8_wide_ws_bytes(M, N, K) == -1
        out = (ctypes.c_int * 4)()
        assert hip.lib().mla_gemm_prefill_f8_wide_plan(M, N, K, 256, ctypes.cast(out, ctypes.c_void_p)) < 0
        assert b"1 <= M <= 65536" in hip.lib().mla_last_error() and b"K % 128 == 0" in hip.lib().mla_last_error()
    # the compact entry points keep their limit and their message
    out = (ctypes.c_int * 4)()
    assert hip.lib().mla_gemm_prefill_f8_plan(1025, 4096, 4096, 256, ctypes.cast(out, ctypes.c_void_p)) < 0
    assert b"1 <= M <= 1024" in hip.lib().mla_last_error()


def test_launchers_check_their_arguments_on_the_host():
    """Argument validation happens before any launch -> safe without a GPU (the pointers are never dereferenced). M = 2049, N = 256,
    K = 4096 is a plan that splits (64-row tiles, split 4), so the workspace checks are live."""
    from mla_amd import hip
    lib = hip.lib()
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    ok = dict(M=2049, N=256, K=4096)

    def plain(x=P, xs=P, W=P, wsc=P, out=P, res=None, ws=P, ws_bytes=1 << 40, ldo=256, ldx=None, **kw):
        d = ok | kw
        return lib.mla_gemm_prefill_f8_wide(x, d["K"] if ldx is None else ldx, xs, W, d["K"], wsc, out, ldo, 0, d["M"], res, 256, d["M"],
                                            d["N"], d["K"], ws, ws_bytes, None)
    need = hip.gemm_prefill_f8_wide_ws_bytes(2049, 256, 4096)
    assert need == 4 * 2112 * 256 * 4                                     # 33 x 2 tiles of 64 rows, 32 K tiles: split 4
    assert plain(M=65537) == -1 and b"1 <= M <= 65536" in lib.mla_last_error()
    assert plain(M=0) == -1 and b"1 <= M <= 65536" in lib.mla_last_error()
    assert plain(K=192) == -1 and b"K % 128 == 0" in lib.mla_last_error()
    assert plain(N=192) == -1 and b"N % 128 == 0" in lib.mla_last_error()
    assert plain(x=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(xs=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(wsc=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(out=Q) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(ldo=260) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(res=Q) == -1 and b"residual" in lib.mla_last_error()
    assert plain(ws_bytes=need - 1) == -1 and b"workspace" in lib.mla_last_error()      # a short workspace
    assert plain(ws=None) == -1 and b"workspace" in lib.mla_last_error()                # a null workspace
    assert plain(ws=Q) == -1 and b"workspace" in lib.mla_last_error()                   # a misaligned workspace

    def rope(cos=P, sin=P, rope_cols=128, head_dim=128, M=1070):
        return lib.mla_gemm_prefill_f8_wide_qkv_rope(P, 256, P, P, 256, P, P, 384, 0, 535, M, 384, 256, cos, sin, rope_cols, head_dim, None,
                                                     0, None)
    assert rope(head_dim=64) == -1 and b"head_dim must be 128" in lib.mla_last_error()
    assert rope(rope_cols=64) == -1 and b"rope_cols" in lib.mla_last_error()
    assert rope(rope_cols=512) == -1 and b"rope_cols" in lib.mla_last_error()
    assert rope(sin=None) == -1 and b"tables" in lib.mla_last_error()
    assert rope(M=65537) == -1 and b"1 <= M <= 65536" in lib.mla_last_error()
    rc = lib.mla_gemm_prefill_f8_wide_gateup_swiglu(P, 256, P, P, 256, P, P, 96, 0, 1070, 1070, 96, 256, None, 0, None)
    assert rc == -1 and b"I % 64 == 0" in lib.mla_last_error()


def test_batch_prefill_is_a_named_argument_and_checked():
    """Validated in check_modes' position, before `self` is touched (no model, no GPU needed to see the error): an unknown value and
    anything but "train" without the cached prefix are ValueErrors, on both routes; what the existing tests pin for the batched call
    stays."""
    from mla_amd import infer
    from mla_amd.mla import MLA
    assert infer.MODES["batch_prefill"].values == ("train", "fp8", "fp8_as_bf16")
    assert infer.MODES["prefill"].values == ("train", "compact")
    for mode in infer.MODES["batch_prefill"].values:
        infer.check_mode("batch_prefill", mode)
    infer.check_mode("batch_prefill", "train", reuse_prefix=False)
    for kw in ({}, {"num_samples": 2}):
        with pytest.raises(ValueError, match="batch_prefill"):
            MLA.predict_action_diff_batch(object(), [None, None], [None, None], batch_prefill="int8", **kw)
        with pytest.raises(ValueError, match="batch_prefill"):
            MLA.predict_action_diff_batch(object(), [None], [None], batch_prefill="FP8", **kw)
        for mode in ("fp8", "fp8_as_bf16"):
            with pytest.raises(ValueError, match="reuse_prefix=True"):
                MLA.predict_action_diff_batch(object(), [None, None], [None, None], batch_prefill=mode, reuse_prefix=False, **kw)
            with pytest.raises(NotImplementedError, match="prefill"):
                MLA.predict_action_diff_batch(object(), [None, None], [None, None], batch_prefill=mode, prefill="compact", **kw)
            with pytest.raises(NotImplementedError, match="prefill_precision"):
                MLA.predict_action_diff_batch(object(), [None, None], [None, None], batch_prefill=mode, prefill_precision="fp8", **kw)
    with pytest.raises(ValueError, match="batch_prefill"):
        infer.check_mode("batch_prefill", "compact")
    for mode in ("fp8", "fp8_as_bf16"):
        with pytest.raises(ValueError, match="does not serve"):
            infer.needs_engine("BatchedPrefixCachedEps", 70, batch_prefill=mode)
    infer.needs_engine("BatchedPrefixCachedEps", 70, batch_prefill="train")


def test_a_batch_prefill_mode_has_an_engine_of_its_own():
    """The engine key gains "batch_prefill:<mode>" for the non-default modes only: the default call keeps the engine -- and the key --
    it had."""
    from types import SimpleNamespace
    from mla_amd import infer

    class Eng(infer._CachedEpsBase):
        def __init__(self, vlm, *ctor):
            self.ctor = ctor
    vlm = SimpleNamespace()
    a = Eng._engine(vlm, "store", ("k",), (1,))
    b = Eng._engine(vlm, "store", ("k",), (2,), batch_prefill="fp8")
    c = Eng._engine(vlm, "store", ("k",), (3,), batch_prefill="fp8_as_bf16")
    d = Eng._engine(vlm, "store", ("k",), (4,), suffix_weights="fp8", suffix_attention="split", batch_prefill="fp8")
    assert len({id(e) for e in (a, b, c, d)}) == 4 and a is Eng._engine(vlm, "store", ("k",), (1,), batch_prefill="train")
    assert set(vlm.store) == {("k",), ("k", "batch_prefill:fp8"), ("k", "batch_prefill:fp8_as_bf16"),
                              ("k", "fp8", "attention:split", "batch_prefill:fp8")}


def test_the_batch_engines_size_and_refuse_on_the_host():
    """What the engines check before any launch: more than 65 536 prefill rows in a sub-batch ("fp8") and more than 1024 prefix rows
    per sample (the per-sample yardstick) are ValueErrors that name the limit."""
    from mla_amd import infer
    eng = infer.BatchedPrefixCachedEps.__new__(infer.BatchedPrefixCachedEps)
    eng.batch_prefill = "train"
    eng._check_batch_prefill(1 << 20, 1 << 20)
    eng.batch_prefill = "fp8"
    eng._check_batch_prefill(120, 546)                                    # 65 520 rows
    with pytest.raises(ValueError, match="65536"):
        eng._check_batch_prefill(121, 546)
    eng.batch_prefill = "fp8_as_bf16"
    eng._check_batch_prefill(121, 1024)
    with pytest.raises(ValueError, match="1024"):
        eng._check_batch_prefill(2, 1025)
