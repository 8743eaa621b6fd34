"""CPU: the host side of FP8 suffix weights for N-sample action drawing -- argument validation of mla_gemm_suffix_w8 (on the host, before any
launch: no GPU needed) and the `suffix_weights` argument of MLA.predict_action_diff_samples / SampleGroupsEps.for_inputs."""
import ctypes
import inspect

import pytest

P = ctypes.c_void_p(16)
NAME = b"mla_gemm_suffix_w8"


def _suffix(lib, x=P, W=P, w_scale=P, out=P, M=136, N=128, K=4096, ldw=None, slot=None, cap=0, res=None, cos=None, sin=None, rope_cols=0, rpb=17):
    return lib.mla_gemm_suffix_w8(x, K, W, K if ldw is None else ldw, w_scale, out, N, 0, rpb, slot, cap, res, 0, M, N, K, cos, sin, rope_cols,
                                  None)


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(w_scale=None), b"null pointer"), (dict(out=None), b"null pointer"),
    (dict(M=0), b"1 <= M <= 256"), (dict(M=257), b"1 <= M <= 256"),
    (dict(K=8), b"K % 16 == 0"), (dict(K=4104), b"K % 16 == 0"),
    (dict(ldw=4104), b"16-B aligned"),                                       # an fp8 row must start on 16 B: ldw is in elements = bytes
    (dict(cos=P), b"RoPE epilogue needs both tables"),
    (dict(cos=P, sin=P, rope_cols=128, res=P), b"RoPE epilogue needs both tables"),
    (dict(slot=P, cap=16), b"cap_rows (16) must hold the 17 rows"),
], ids=["x", "W", "w_scale", "out", "M0", "M257", "K8", "K4104", "ldw4104", "one_table", "rope_and_residual", "cap_rows"])
def test_gemm_suffix_w8_rejects_bad_arguments(kw, msg):
    from mla_amd import hip
    lib = hip.lib()
    rc = _suffix(lib, **kw)
    err = lib.mla_last_error()
    assert rc < 0 and NAME in err and msg in err, (kw, rc, err)


def test_gemm_suffix_w8_is_bound():
    from mla_amd import hip
    assert "mla_gemm_suffix_w8" in hip._SIGNATURES and callable(hip.gemm_suffix_w8)
    a = list(inspect.signature(hip.gemm_suffix_w8).parameters)
    b = list(inspect.signature(hip.gemm_suffix).parameters)
    assert a == b[:2] + ["w_scale"] + b[2:]
    assert hip.lib().mla_query(0) == 1


def test_samples_suffix_weights_is_a_named_argument_and_checked():
    """The mode is validated in front of everything else: no model and no GPU are needed to see the error."""
    from mla_amd import infer
    from mla_amd.mla import MLA
    p = inspect.signature(MLA.predict_action_diff_samples).parameters["suffix_weights"]
    assert p.default == "bf16" and p.kind == p.KEYWORD_ONLY
    with pytest.raises(ValueError, match="suffix_weights"):
        MLA.predict_action_diff_samples(object(), suffix_weights="int4")
    with pytest.raises(ValueError, match="suffix_weights"):
        infer.SampleGroupsEps.for_inputs(object(), None, 1, 2, suffix_weights="e5m2")
    p = inspect.signature(infer.SampleGroupsEps.__init__).parameters["modes"]
    assert p.default.suffix_weights == "bf16"
