"""CPU: host-side argument validation of the action-chunk inference kernels (mla_gemm_skinny_bf16, mla_attn_chunk) and the
cached-prefix engine's capability rule -- no launch happens, so no GPU is needed."""
import ctypes
import types

import pytest

P = ctypes.c_void_p(16)


def _skinny(lib, x=P, W=P, out=P, M=17, N=64, K=4096, pre=0, pre_w=None):
    return lib.mla_gemm_skinny_bf16(x, K, W, K, out, N, 0, M, None, 0, M, N, K, pre, pre_w, 1e-5, None, None, 0, None)


def _chunk(lib, q=P, R=17, head_dim=128, S_kv=565):
    return lib.mla_attn_chunk(q, P, P, P, 1, 32, head_dim, S_kv, R, 3 * 4096, 3 * 4096 * S_kv, 4096, 0.088, None)


def test_gemm_skinny_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(M=65), b"1 <= M <= 64"),
                    (dict(M=0), b"1 <= M <= 64"), (dict(K=4100), b"K % 8 == 0"), (dict(pre=1), b"pre must be"),
                    (dict(pre=3), b"pre must be")]:
        rc = _skinny(lib, **kw)
        assert rc < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())
    rc = lib.mla_gemm_skinny_bf16(P, 4096, P, 4096, P, 64, 0, 17, None, 0, 17, 64, 4096, 0, None, 1e-5, ctypes.c_void_p(64), None, 64, None)
    assert rc < 0 and b"RoPE epilogue needs both tables" in lib.mla_last_error()


def test_attn_chunk_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()
    for kw, msg in [(dict(q=None), b"null pointer"), (dict(R=65), b"1 <= R <= 64"), (dict(R=0), b"1 <= R <= 64"),
                    (dict(R=17, S_kv=16), b"R <= S_kv"), (dict(head_dim=64), b"head_dim must be 128")]:
        rc = _chunk(lib, **kw)
        assert rc < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


def test_engine_selection_rule():
    """The GEMV keeps every shape it accepts (M <= 8 and the M x K rows in its 160 KiB of LDS), the decode attention every R <= 8 whose
    scores fit; the 7B down projection (K = 11008) leaves the GEMV from 8 rows on."""
    from mla_amd import hip
    assert hip.gemv_fits(8, 4096) and hip.gemv_fits(7, 11008) and not hip.gemv_fits(8, 11008) and not hip.gemv_fits(9, 512)
    assert hip.attn_decode_fits(8, 565) and hip.attn_decode_fits(2, 4096) and not hip.attn_decode_fits(9, 565)
    assert not hip.attn_decode_fits(8, 8192)


def _vlm(hidden, heads):
    cfg = types.SimpleNamespace(hidden_size=hidden, num_attention_heads=heads)
    llm = types.SimpleNamespace(config=cfg)
    return types.SimpleNamespace(llm_backbone=types.SimpleNamespace(llm=llm))


def test_prefix_engine_capability_check_warns_once():
    from mla_amd.infer import PrefixCachedEps
    assert PrefixCachedEps.supports(_vlm(4096, 32), 1, 16) and PrefixCachedEps.supports(_vlm(256, 2), 1, 63)
    v = _vlm(256, 2)
    with pytest.warns(RuntimeWarning, match="65 suffix rows"):
        assert not PrefixCachedEps.supports(v, 1, 64)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not PrefixCachedEps.supports(v, 1, 64)                     # once per shape
    with pytest.warns(RuntimeWarning, match="head_dim 64"):
        assert not PrefixCachedEps.supports(_vlm(256, 4), 1, 3)
