"""CPU: the compact prefill's host side -- the launch plan of the row-sized GEMMs (mla_amd/csrc/prefill.hip; hip.plan_gemm_prefill mirrors
the launcher, mla_gemm_prefill_plan is the launcher's own answer), their argument checks, and the `prefill` argument of the samplers.
Nothing here launches a kernel."""
import ctypes

import pytest

SHAPES_7B = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)]          # q|k|v, o, gate|up (2 I), down: N x K


def _lib_plan(M, N, K, cus=256):
    from mla_amd import hip
    out = (ctypes.c_int * 4)()
    rc = hip.lib().mla_gemm_prefill_plan(M, N, K, cus, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, hip.lib().mla_last_error()
    return tuple(out)


@pytest.mark.parametrize("N,K", SHAPES_7B)
def test_plan_fills_the_chip_at_one_observation(N, K):
    """M = 545 (one observation's prefix rows): every 7B projection puts at least one workgroup on each of the 256 CUs (or says why
    not), covers all rows, and asks for split x rows_covered x N x 4 workspace bytes -- none without split-K."""
    from mla_amd import hip
    M = 545
    p = hip.plan_gemm_prefill(M, N, K)
    assert p.workgroups >= 256 or p.note, p
    assert p.rows_covered >= M and p.rows_covered % p.tile_m == 0 and p.rows_covered - M < p.tile_m
    assert N % p.tile_n == 0
    assert p.workgroups == (p.rows_covered // p.tile_m) * (N // p.tile_n) * p.split
    assert p.ws_bytes == (p.split * p.rows_covered * N * 4 if p.split > 1 else 0)
    assert (p.split == 1) == (p.ws_bytes == 0)
    # the two N = 4096 projections are the ones the training tiles starve (48 workgroups): they split
    assert (p.split > 1) == (N == 4096), p


@pytest.mark.parametrize("M", [1, 64, 65, 545, 1024])
@pytest.mark.parametrize("N,K", SHAPES_7B + [(128, 256), (384, 256), (256, 4096), (128, 352), (128, 11008), (768, 256)])
def test_plan_is_the_launchers(M, N, K):
    """The pure-Python plan and the library's launcher agree on tile, split and workgroups, and on the workspace bytes, at the row-count
    edges (one row, a full tile, one row more, the full range) -- for 256 CUs (what the launcher plans for) and for another count."""
    from mla_amd import hip
    p = hip.plan_gemm_prefill(M, N, K)
    assert (p.tile_m, p.tile_n, p.split, p.workgroups) == _lib_plan(M, N, K)
    assert p.ws_bytes == hip.gemm_prefill_ws_bytes(M, N, K)
    assert p.rows_covered == -(-M // 64) * 64
    q = hip.plan_gemm_prefill(M, N, K, cus=64)
    assert (q.tile_m, q.tile_n, q.split, q.workgroups) == _lib_plan(M, N, K, 64) and q.split <= p.split
    if p.split > 1:
        assert -(-K // 64) // p.split >= 8 and p.split <= 16           # every slice keeps at least 8 K tiles


def test_narrow_and_long_k_shapes_take_the_split_path():
    """The GPU test's two split shapes: a narrow N at K = 4096 and the down projection's K = 11008."""
    from mla_amd import hip
    assert hip.plan_gemm_prefill(545, 256, 4096).split == 8
    assert hip.plan_gemm_prefill(545, 128, 11008).split == 16
    assert hip.plan_gemm_prefill(1024, 128, 352).split == 1              # 6 K tiles: nothing to split
    assert "K tiles" in hip.plan_gemm_prefill(1024, 128, 352).note


def test_shapes_outside_the_contract_are_refused():
    from mla_amd import hip
    assert hip.gemm_prefill_fits(1024, 4096, 4096) and hip.gemm_prefill_fits(1, 128, 32)
    assert not hip.gemm_prefill_fits(1025, 4096, 4096)
    assert not hip.gemm_prefill_fits(0, 4096, 4096)
    assert not hip.gemm_prefill_fits(545, 4096, 48)
    assert not hip.gemm_prefill_fits(545, 4000, 4096)
    with pytest.raises(ValueError, match="1 <= M <= 1024"):
        hip.plan_gemm_prefill(1025, 4096, 4096)
    assert hip.gemm_prefill_ws_bytes(1025, 4096, 4096) == -1
    lib = hip.lib()
    out = (ctypes.c_int * 4)()
    assert lib.mla_gemm_prefill_plan(1025, 4096, 4096, 256, ctypes.cast(out, ctypes.c_void_p)) < 0
    assert b"1 <= M <= 1024" in lib.mla_last_error()


def test_launchers_check_their_arguments_on_the_host():
    """Argument validation happens before any launch -> safe without a GPU (the pointers are never dereferenced)."""
    from mla_amd import hip
    lib = hip.lib()
    P, Q = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)
    ok = dict(M=545, N=256, K=4096)

    def plain(x=P, W=P, out=P, res=None, ws=P, ws_bytes=1 << 40, ldo=256, **kw):
        d = ok | kw
        return lib.mla_gemm_prefill_bf16(x, d["K"], W, d["K"], out, ldo, 0, d["M"], res, 256, d["M"], d["N"], d["K"], ws, ws_bytes, None)
    need = hip.gemm_prefill_ws_bytes(545, 256, 4096)
    assert need == 8 * 576 * 256 * 4
    assert plain(M=1025) == -1 and b"1 <= M <= 1024" in lib.mla_last_error()
    assert plain(K=48) == -1 and b"K % 32 == 0" in lib.mla_last_error()
    assert plain(N=200) == -1 and b"N % 128 == 0" in lib.mla_last_error()
    assert plain(x=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert plain(out=Q) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(ldo=260) == -1 and b"16-B aligned" in lib.mla_last_error()
    assert plain(res=Q) == -1 and b"residual" in lib.mla_last_error()
    assert plain(ws_bytes=need - 1) == -1 and b"workspace" in lib.mla_last_error()
    assert plain(ws=None) == -1 and b"workspace" in lib.mla_last_error()

    def rope(cos=P, sin=P, rope_cols=128, head_dim=128):
        return lib.mla_gemm_prefill_qkv_rope(P, 256, P, 256, P, 384, 0, 65, 130, 384, 256, cos, sin, rope_cols, head_dim, None, 0, None)
    assert rope(head_dim=64) == -1 and b"head_dim must be 128" in lib.mla_last_error()
    assert rope(rope_cols=64) == -1 and b"rope_cols" in lib.mla_last_error()
    assert rope(rope_cols=512) == -1 and b"rope_cols" in lib.mla_last_error()
    assert rope(sin=None) == -1 and b"tables" in lib.mla_last_error()
    rc = lib.mla_gemm_prefill_gateup_swiglu(P, 256, P, 256, P, 96, 0, 65, 65, 96, 256, None, 0, None)
    assert rc == -1 and b"I % 64 == 0" in lib.mla_last_error()


def test_prefill_is_a_named_argument_and_checked():
    """The mode is validated in front of everything else (no model, no GPU needed to see the error): an unknown mode and "compact"
    without the cached prefix are ValueErrors, the batched call refuses "compact" with NotImplementedError."""
    from mla_amd import infer
    from mla_amd.mla import MLA
    assert infer.MODES["prefill"].values == ("train", "compact")
    for mode in infer.MODES["prefill"].values:
        infer.check_mode("prefill", mode)
    with pytest.raises(ValueError, match="prefill"):
        MLA.predict_action_diff(object(), prefill="nonsense")
    with pytest.raises(ValueError, match="prefill"):
        MLA.predict_action_diff_samples(object(), prefill="Compact", num_samples=2)
    with pytest.raises(ValueError, match="prefill"):
        MLA.predict_action_diff_batch(object(), [None], [None], prefill="nonsense")
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        MLA.predict_action_diff(object(), prefill="compact", reuse_prefix=False)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        MLA.predict_action_diff_samples(object(), prefill="compact", reuse_prefix=False, num_samples=3)
    with pytest.raises(NotImplementedError, match="compact"):
        MLA.predict_action_diff_batch(object(), [None], [None], prefill="compact")
    with pytest.raises(NotImplementedError, match="compact"):
        MLA.predict_action_diff_batch(object(), [None, None], [None, None], prefill="compact", suffix_weights="fp8", num_samples=2)
    with pytest.raises(ValueError, match="prefill"):
        infer.PrefixCachedEps.for_inputs(object(), None, prefill="fast")
    with pytest.raises(ValueError, match="prefill"):
        infer.SampleGroupsEps.for_inputs(object(), None, 16, 2, prefill="fast")


def test_compact_engine_refuses_what_it_does_not_serve():
    """More than 1024 prefix rows or head_dim != 128 is an error of the engine, never a silent "train" prefill."""
    from types import SimpleNamespace
    from mla_amd import infer
    eng = infer._CachedEpsBase.__new__(infer._CachedEpsBase)
    eng.prefill_mode, eng.nheads = "compact", 32
    eng.cfg = SimpleNamespace(hidden_size=4096, intermediate_size=11008)
    eng._check_compact(1024)
    with pytest.raises(ValueError, match="1024 prefix rows"):
        eng._check_compact(1025)
    eng.nheads = 64                                                       # head_dim 64
    with pytest.raises(ValueError, match="head_dim"):
        eng._check_compact(545)
    eng.prefill_mode = "train"
    eng._check_compact(5000)
