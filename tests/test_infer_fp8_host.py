"""CPU: the host side of the FP8 suffix-weight path -- argument validation of mla_gemv_w8 / mla_gemm_skinny_w8 / mla_quant_fp8_rows (on the
host, before any launch: no GPU needed) and the `suffix_weights` argument of MLA.predict_action_diff / predict_action_diff_batch."""
import ctypes
import inspect

import pytest

P = ctypes.c_void_p(16)


def _proj(lib, name, x=P, W=P, w_scale=P, out=P, M=2, N=64, K=4096, pre=0):
    return getattr(lib, name)(x, K, W, K, w_scale, out, N, 0, M, None, 0, M, N, K, pre, None, 1e-5, None, None, 0, None)


@pytest.mark.parametrize("name,mmax", [("mla_gemv_w8", 8), ("mla_gemm_skinny_w8", 64)])
def test_w8_projections_reject_bad_arguments(name, mmax):
    from mla_amd import hip
    lib = hip.lib()
    rng = f"1 <= M <= {mmax}".encode()
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(w_scale=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(K=4104), b"K % 16 == 0"), (dict(K=8), b"K % 16 == 0"), (dict(M=0), rng),
                    (dict(M=mmax + 1), rng), (dict(pre=1), b"pre must be"), (dict(pre=3), b"pre must be")]:
        rc = _proj(lib, name, **kw)
        assert rc < 0 and name.encode() in lib.mla_last_error() and msg in lib.mla_last_error(), (kw, lib.mla_last_error())
    rc = getattr(lib, name)(P, 4096, P, 4096, P, P, 64, 0, 2, None, 0, 2, 64, 4096, 0, None, 1e-5, ctypes.c_void_p(64), None, 64, None)
    assert rc < 0 and b"RoPE epilogue needs both tables" in lib.mla_last_error()
    # a weight row of fp8 must start on 16 B: ldw is in elements = bytes
    rc = getattr(lib, name)(P, 4096, P, 4104, P, P, 64, 0, 2, None, 0, 2, 64, 4096, 0, None, 1e-5, None, None, 0, None)
    assert rc < 0 and b"16-B aligned" in lib.mla_last_error()


def test_gemv_w8_keeps_the_lds_limit_of_the_bf16_rows():
    from mla_amd import hip
    lib = hip.lib()
    assert not hip.gemv_fits(8, 11008)
    rc = _proj(lib, "mla_gemv_w8", M=8, K=11008)
    assert rc < 0 and b"must fit the 160 KiB of LDS" in lib.mla_last_error()


def test_quantiser_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()

    def q(W=P, qq=P, scale=P, N=4, K=64, ldw=None, ldq=None):
        return lib.mla_quant_fp8_rows(W, K if ldw is None else ldw, qq, K if ldq is None else ldq, scale, N, K, None)
    for kw, msg in [(dict(W=None), b"null pointer"), (dict(qq=None), b"null pointer"), (dict(scale=None), b"null pointer"),
                    (dict(K=24), b"K % 16 == 0"), (dict(K=0), b"K % 16 == 0"), (dict(N=0), b"N >= 1"), (dict(ldw=60), b"16-B aligned"),
                    (dict(ldq=72), b"16-B aligned")]:
        rc = q(**kw)
        assert rc < 0 and b"mla_quant_fp8_rows" in lib.mla_last_error() and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


def test_suffix_weights_is_a_named_argument_and_checked():
    """Before this argument existed an unknown keyword fell into **kwargs and was ignored; the value is validated in front of everything
    else (no model, no GPU needed to see the error)."""
    from mla_amd import infer
    from mla_amd.mla import MLA
    for fn in (MLA.predict_action_diff, MLA.predict_action_diff_batch):
        p = inspect.signature(fn).parameters["suffix_weights"]
        assert p.default == "bf16" and p.kind in (p.KEYWORD_ONLY, p.POSITIONAL_OR_KEYWORD)
    assert infer.MODES["suffix_weights"].values == ("bf16", "fp8", "fp8_as_bf16")
    with pytest.raises(ValueError, match="suffix_weights"):
        MLA.predict_action_diff(object(), suffix_weights="int4")
    with pytest.raises(ValueError, match="suffix_weights"):
        MLA.predict_action_diff_batch(object(), [None], [None], suffix_weights="FP8")
    with pytest.raises(ValueError, match="suffix_weights"):
        infer.PrefixCachedEps.for_inputs(object(), None, suffix_weights="e5m2")
    for mode in infer.MODES["suffix_weights"].values:
        infer.check_mode("suffix_weights", mode)
