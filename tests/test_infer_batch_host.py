"""CPU: the host side of batched action sampling (MLA.predict_action_diff_batch) -- the pure planning function of
mla_amd/infer.py (splice positions, prompt tails, prefix lengths, cache slots, capacity bucket, sub-batch split), the fp64 reference of
the ragged suffix attention the GPU tests use (tests/infer_batch_cases.py), and the argument validation of the two new C-ABI entry
points (no launch happens, so no GPU is needed)."""
import ctypes
import types

import pytest
import torch

import attention_cases as ac
import infer_batch_cases as ibc

TAG = 29871
P = ctypes.c_void_p(16)


# ------------------------------------------------------------------------------------------------ plan_batch
def test_plan_mixed_lengths_and_tails():
    from mla_amd.infer import PROMPT_TAIL, SPLICE_TAG, plan_batch
    assert SPLICE_TAG == TAG and PROMPT_TAIL == (29871, 32001, 32002, 29871)
    rows = [[1, 5, 6, 7, TAG],                 # tail already there: kept as it is, k = 4
            [1, 5, 6],                         # no tail: [1, 5, 6, TAG], k = 3
            [1, 9, TAG, 4, 4, 4],              # a tag in the middle but not at the end: the tail is appended, the LAST tag counts -> k = 6
            [1, 2, 3, 4, 5, 6, 7, 8, TAG]]     # k = 8
    (p,) = plan_batch(rows, n_action_rows=16, n_front=513)
    assert p.ids == ((1, 5, 6, 7, TAG), (1, 5, 6, TAG), (1, 9, TAG, 4, 4, 4, TAG), (1, 2, 3, 4, 5, 6, 7, 8, TAG))
    assert p.k == (4, 3, 6, 8) and (p.start, p.stop, p.R) == (0, 4, 17)
    # prefix rows: BOS + 513 front tokens + text[1:k] + proprio
    assert p.S_p == (518, 517, 520, 522) and p.slot == p.S_p and p.kv_len == (535, 534, 537, 539)
    assert p.S_pmax == 522 and p.S_cap == 576                                 # roundup(522 + 17, 64)
    # the same ids as tensors, as the public method hands them over
    (q,) = plan_batch([torch.tensor(r) for r in rows], 16, 513)
    assert q == p


def test_plan_without_tail_handling_and_row_without_tag():
    from mla_amd.infer import plan_batch
    (p,) = plan_batch([[1, 5, TAG, 8, 9], [1, TAG]], 3, 10, add_tail=False)
    assert p.ids == ((1, 5, TAG, 8, 9), (1, TAG)) and p.k == (2, 1) and p.S_p == (13, 12)
    with pytest.raises(IndexError, match="row 1 without the splice tag"):
        plan_batch([[1, 5, TAG], [1, 5, 6]], 3, 10, add_tail=False)
    with pytest.raises(IndexError, match="must not be the first id"):
        plan_batch([[TAG, 5]], 3, 10, add_tail=False)
    with pytest.raises(ValueError):
        plan_batch([], 3, 10)
    with pytest.raises(ValueError, match="exceed"):
        plan_batch([[1, TAG]], 256, 10)                                      # 257 rows per sample


def test_plan_capacity_bucket():
    from mla_amd.infer import plan_batch
    mk = lambda L: [1] + [7] * (L - 2) + [TAG]  # noqa: E731 -- L ids, k = L - 1, S_p = n_front + L
    for L, want in [(30, 576), (42, 576), (43, 640), (106, 640), (107, 704)]:      # S_pmax + 17 = 530+L ... : 559 -> 576, 576 -> 576 | 577 -> 640
        (p,) = plan_batch([mk(20), mk(L)], 16, 517)
        assert p.S_pmax == 517 + L and p.S_cap == want and p.S_cap % 64 == 0 and p.S_cap >= p.S_pmax + 17, (L, p)
    # two length mixes in one bucket plan the same engine key, other device tables
    (a,) = plan_batch([mk(21), mk(14), mk(27)], 3, 513)
    (b,) = plan_batch([mk(18), mk(26), mk(15)], 3, 513)
    assert (a.S_cap, a.R) == (b.S_cap, b.R) and a.slot != b.slot and a.S_pmax != b.S_pmax
    (c,) = plan_batch([mk(21), mk(14)], 3, 513, bucket=16)
    assert c.S_cap == 544                                                     # roundup(534 + 4, 16)


def test_plan_sub_batch_split():
    from mla_amd.infer import plan_batch
    mk = lambda L: [1] + [7] * (L - 2) + [TAG]  # noqa: E731
    # B * R = 256 exactly: one pass
    plans = plan_batch([mk(10 + b) for b in range(16)], 15, 513)
    assert len(plans) == 1 and (plans[0].start, plans[0].stop) == (0, 16) and plans[0].R == 16
    # 257 rows of samples with R = 1 ... is B = 257; with R = 16, 17 samples = 272 rows: 16 + 1
    plans = plan_batch([mk(10 + b) for b in range(17)], 15, 513)
    assert [(p.start, p.stop) for p in plans] == [(0, 16), (16, 17)]
    assert plans[1].ids == (tuple(mk(26)),) and plans[1].S_pmax == 513 + 26 and plans[0].S_pmax == 513 + 25
    # R = 1 (no action rows is not a use case, but the arithmetic): 257 samples -> 256 + 1
    plans = plan_batch([mk(5)] * 257, 0, 4)
    assert [(p.start, p.stop) for p in plans] == [(0, 256), (256, 257)]
    # the default chunk: R = 17 -> 15 samples (255 rows) per pass
    plans = plan_batch([mk(12)] * 31, 16, 513)
    assert [(p.start, p.stop) for p in plans] == [(0, 15), (15, 30), (30, 31)]
    # a row cap patched down
    plans = plan_batch([mk(12), mk(13), mk(14)], 3, 513, max_rows=8)
    assert [(p.start, p.stop) for p in plans] == [(0, 2), (2, 3)] and plans[1].slot == (513 + 14,)


# ------------------------------------------------------------------------------------------------ the fp64 ragged reference
def test_ragged_reference_is_the_per_sample_decode_reference():
    """ragged_attn_r64 on a poisoned ragged cache == attention_cases.r64 (decode form, n_query = R) on each sample's own rows.
    (A test of the test helper itself: the one new test that does not depend on the feature.)"""
    B, H, R, S_cap = 3, 2, 5, 40
    kv_len = [5, 33, 40]
    cache = ibc.make_ragged_cache(B, H, S_cap, kv_len, seed=3)
    assert torch.isnan(cache[0, 5:].float()).all() and torch.isfinite(cache[1, :33].float()).all()
    got = ibc.ragged_attn_r64(cache, kv_len, R, H)
    assert got.shape == (B * R, H * ac.D) and got.dtype == torch.float64 and torch.isfinite(got).all()
    for b, n in enumerate(kv_len):
        q, k, v = (t[b:b + 1, :, :n] for t in ibc.split_cache(cache, H))
        ref = ac.r64(q, k, v, ac.make_dout(1, H, R, 1).double(), ac.allowed_mask(1, n, n_query=R))["o"]
        assert torch.allclose(got[b * R:(b + 1) * R], ac.rows2d(ref), rtol=1e-12, atol=1e-13)
    al = ibc.ragged_allowed(kv_len, R, S_cap)
    assert al.shape == (B, R, S_cap) and al[0, 0].sum() == 1 and al[0, 4].sum() == 5 and al[1, 0].sum() == 29 and al[2, 4].all()
    # first query of the shortest sample sees key 0 only: its output is v[0]
    v0 = cache[0, 0, 2 * H * ac.D:].double()
    assert torch.equal(got[0], v0)


# ------------------------------------------------------------------------------------------------ argument validation, no launch
def _suffix(lib, x=P, W=P, out=P, M=136, N=64, K=4096, slot=None, cap=0, res=None, cos=None, sin=None, rope_cols=0, rpb=17):
    return lib.mla_gemm_suffix_bf16(x, K, W, K, out, N, 0, rpb, slot, cap, res, 0, M, N, K, cos, sin, rope_cols, None)


def test_gemm_suffix_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(M=257), b"1 <= M <= 256"), (dict(M=0), b"1 <= M <= 256"),
                    (dict(K=4100), b"K % 8 == 0"), (dict(slot=P, cap=16), b"cap_rows (16) must hold the 17 rows"),
                    (dict(cos=P), b"RoPE epilogue needs both tables"), (dict(cos=P, sin=P, rope_cols=64), b"RoPE epilogue needs both tables"),
                    (dict(cos=P, sin=P, rope_cols=128, N=128, res=P), b"RoPE epilogue needs both tables"),
                    (dict(x=ctypes.c_void_p(8)), b"16-B aligned")]:
        rc = _suffix(lib, **kw)
        assert rc < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


def test_attn_chunk_ragged_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()

    def call(q=P, kv=P, R=17, head_dim=128, S_cap=576):
        return lib.mla_attn_chunk_ragged(q, P, P, P, 3, 32, head_dim, kv, S_cap, R, 3 * 4096, 3 * 4096 * S_cap, 4096, 0.088, None)
    for kw, msg in [(dict(q=None), b"null pointer"), (dict(kv=None), b"null pointer"), (dict(R=65), b"1 <= R <= 64"), (dict(R=0), b"1 <= R <= 64"),
                    (dict(R=17, S_cap=16), b"R <= S_cap"), (dict(head_dim=64), b"head_dim must be 128")]:
        rc = call(**kw)
        assert rc < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


def _vlm(hidden, heads):
    cfg = types.SimpleNamespace(hidden_size=hidden, num_attention_heads=heads)
    return types.SimpleNamespace(llm_backbone=types.SimpleNamespace(llm=types.SimpleNamespace(config=cfg)))


def test_batched_engine_capability_rule():
    import warnings
    from mla_amd.infer import BatchedPrefixCachedEps, PrefixCachedEps
    assert BatchedPrefixCachedEps.MAX_ROWS == 256 and PrefixCachedEps.MAX_ROWS == 64       # the batch-1 engine's rule is unchanged
    # the two engines share a base, not each other's entry points
    assert not issubclass(BatchedPrefixCachedEps, PrefixCachedEps) and not hasattr(BatchedPrefixCachedEps, "for_inputs")
    assert BatchedPrefixCachedEps.supports_batch(_vlm(4096, 32), 16) and BatchedPrefixCachedEps.supports_batch(_vlm(256, 2), 63)
    v = _vlm(256, 4)
    with pytest.warns(RuntimeWarning, match="head_dim 64"):
        assert not BatchedPrefixCachedEps.supports_batch(v, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not BatchedPrefixCachedEps.supports_batch(v, 3)                     # once per shape
    with pytest.warns(RuntimeWarning, match="65 suffix rows per sample"):
        assert not BatchedPrefixCachedEps.supports_batch(_vlm(256, 2), 64)


def test_public_method_exists_with_the_documented_signature():
    import inspect
    from mla_amd.mla import MLA
    sig = inspect.signature(MLA.predict_action_diff_batch)
    assert list(sig.parameters)[:10] == ["self", "images", "pointclouds", "instructions", "cur_robot_states", "unnorm_key", "cfg_scale",
                                         "use_ddim", "num_ddim_steps", "action_dim"]
    for name in ("input_ids", "noise", "camera_name", "reuse_prefix"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["reuse_prefix"].default is True and sig.parameters["num_ddim_steps"].default == 8
