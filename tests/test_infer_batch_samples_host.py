"""CPU: the host side of N action chunks for each of B observations -- plan_batch_samples (mla_amd/infer.py), the argument errors of
MLA.predict_action_diff_batch(num_samples=...) that need no device, and the argument validation of the new C-ABI entry points (no launch
happens, so no GPU is needed)."""
import ctypes
import types

import pytest
import torch

import infer_batch_samples_cases as bsc

TAG = 29871
P = ctypes.c_void_p(16)
mk = lambda L: [1] + [7] * (L - 2) + [TAG]  # noqa: E731 -- L ids, k = L - 1, S_p = n_front + L


def _spans(plans):
    return [(p.start, p.stop) for p in plans]


def test_plan_pass_boundaries():
    from mla_amd.infer import plan_batch_samples
    # (B, N, R, max_rows) = (3, 2, 5, 20): 4 groups per pass -> 2 observations with both groups each, then 1
    plans = plan_batch_samples([mk(12), mk(13), mk(14)], 4, 513, 2, max_rows=20)
    assert _spans(plans) == [(0, 2), (2, 3)] and all(p.G == 2 and p.R == 5 for p in plans)
    # (5, 3, 17, 256): 15 groups per pass -> 5 observations
    plans = plan_batch_samples([mk(10 + b) for b in range(5)], 16, 513, 3)
    assert _spans(plans) == [(0, 5)] and plans[0].G == 3 and plans[0].R == 17 and len(plans[0].slot) == 15
    # 6 observations: 5 + 1; per // N rounds down (256 // 17 = 15, N = 4 -> 3 observations per pass)
    assert _spans(plans_6 := plan_batch_samples([mk(12)] * 6, 16, 513, 3)) == [(0, 5), (5, 6)] and len(plans_6[1].slot) == 3
    assert _spans(plan_batch_samples([mk(12)] * 7, 16, 513, 4)) == [(0, 3), (3, 6), (6, 7)]
    # N = 1 is plan_batch's split
    assert _spans(plan_batch_samples([mk(12)] * 31, 16, 513, 1)) == [(0, 15), (15, 30), (30, 31)]


def test_plan_reports_more_groups_than_a_pass_holds():
    from mla_amd.infer import BatchedSampleGroupsEps, plan_batch_samples
    assert plan_batch_samples([mk(12), mk(13)], 16, 513, 16) is None            # per = 15 < 16
    assert plan_batch_samples([mk(12), mk(13)], 16, 513, 15) is not None
    assert plan_batch_samples([mk(12), mk(13)], 4, 513, 3, max_rows=10) is None   # the end-to-end test's patch: MAX_ROWS = 2 R
    assert BatchedSampleGroupsEps.fits_pass(16, 15) and not BatchedSampleGroupsEps.fits_pass(16, 16)
    assert BatchedSampleGroupsEps.fits_pass(63, 4) and not BatchedSampleGroupsEps.fits_pass(63, 5)
    with pytest.raises(IndexError):                                             # the rows' errors come first either way
        plan_batch_samples([mk(12), [1, 5, 6]], 16, 513, 16, add_tail=False)


def test_plan_capacity_bucket():
    from mla_amd.infer import plan_batch_samples
    # S_cap = roundup(S_pmax + N R, bucket): S_pmax = 517 + L, N R = 51
    for L, want in [(8, 576), (9, 640), (72, 640), (73, 704)]:                  # 525 + 51 = 576 | 577 -> 640 | 640 | 641 -> 704
        (p,) = plan_batch_samples([mk(5), mk(L)], 16, 517, 3)
        assert p.S_pmax == 517 + L and p.S_cap == want and p.S_cap >= p.S_pmax + 3 * 17, (L, p)
    (p,) = plan_batch_samples([mk(21), mk(14)], 3, 513, 3, bucket=16)
    assert p.S_cap == 560                                                       # roundup(534 + 15, 16)
    # two length mixes in one bucket plan the same engine key, other device tables
    (a,) = plan_batch_samples([mk(21), mk(14), mk(27)], 3, 513, 3)
    (b,) = plan_batch_samples([mk(18), mk(26), mk(15)], 3, 513, 3)
    assert (a.S_cap, a.R, a.G) == (b.S_cap, b.R, b.G) and a.slot != b.slot and a.prefix_len != b.prefix_len


def test_plan_device_arrays_are_the_layout():
    from mla_amd.infer import plan_batch_samples
    rows = [mk(21), mk(14), mk(27), mk(16), mk(30)]
    for N, max_rows in [(3, 256), (2, 20), (1, 256)]:
        for p in plan_batch_samples(rows, 4, 513, N, max_rows=max_rows):
            B = p.stop - p.start
            assert p.S_p == tuple(513 + len(r) for r in rows[p.start:p.stop]) and p.prefix_len == p.S_p
            assert list(p.slot) == [b * p.S_cap + p.S_p[b] + g * p.R for b in range(B) for g in range(N)]
            assert list(p.rope_pos) == [p.S_p[b] for b in range(B) for g in range(N)]
            assert (list(p.prefix_len), list(p.slot), list(p.rope_pos)) == tuple(bsc.layout(p.S_p, N, p.R, p.S_cap))
            assert max(p.slot) + p.R <= B * p.S_cap                             # the last group's rows are inside the flat cache
    # the prompt handling is plan_batch's: tail appended, the LAST tag counts
    (p,) = plan_batch_samples([[1, 5, 6], [1, 9, TAG, 4, 4, 4]], 16, 513, 2)
    assert p.ids == ((1, 5, 6, TAG), (1, 9, TAG, 4, 4, 4, TAG)) and p.k == (3, 6) and p.S_p == (517, 520)


def test_plan_rejects_bad_arguments():
    from mla_amd.infer import plan_batch_samples
    with pytest.raises(IndexError, match="row 1 without the splice tag"):
        plan_batch_samples([[1, 5, TAG], [1, 5, 6]], 3, 10, 2, add_tail=False)
    for n in (0, -2):
        with pytest.raises(ValueError, match="num_samples must be >= 1"):
            plan_batch_samples([mk(12)], 3, 10, n)
    with pytest.raises(ValueError, match="exceed"):
        plan_batch_samples([mk(12)], 256, 10, 1)                                # 257 rows per group
    with pytest.raises(ValueError):
        plan_batch_samples([], 3, 10, 2)


def _stub():
    """An MLA stand-in that reaches the argument checks of predict_action_diff_batch(num_samples=...) and nothing behind them."""
    from mla_amd.mla import MLA
    stub = types.SimpleNamespace(future_action_window_size=3)
    stub._predict_action_diff_batch_samples = types.MethodType(MLA._predict_action_diff_batch_samples, stub)
    stub._check_cfg_scale = MLA._check_cfg_scale
    return MLA, stub


def test_public_call_argument_errors_without_a_device():
    MLA, stub = _stub()
    ids = [torch.tensor(mk(9)), torch.tensor(mk(12))]
    kw = dict(images=[None, None], pointclouds=None, cur_robot_states=[None, None], input_ids=ids)
    for n in (0, -1):
        with pytest.raises(ValueError, match="num_samples must be >= 1"):
            MLA.predict_action_diff_batch(stub, num_samples=n, **kw)
    good = (2, 3, 4, 7)                                                         # [B, N, T, action_dim]
    for bad in [(2, 4, 7), (3, 2, 4, 7), (2, 2, 4, 7), (2, 3, 3, 7), (2, 3, 4, 6), (6, 4, 7)]:
        assert bad != good
        with pytest.raises(ValueError, match=r"noise must be \[B, N, T, action_dim\]"):
            MLA.predict_action_diff_batch(stub, num_samples=3, noise=torch.zeros(bad), **kw)
    with pytest.raises(ValueError, match="one entry per sample"):
        MLA.predict_action_diff_batch(stub, num_samples=3, **dict(kw, input_ids=ids[:1]))
    with pytest.raises(NotImplementedError):                                    # behind the noise check, in front of any device work
        MLA.predict_action_diff_batch(stub, num_samples=3, noise=torch.zeros(good), cfg_scale=1.5, **kw)
    with pytest.raises(ValueError, match="suffix_weights"):
        MLA.predict_action_diff_batch(stub, num_samples=3, suffix_weights="int4", **kw)


def test_public_method_signature():
    import inspect
    from mla_amd.mla import MLA
    p = inspect.signature(MLA.predict_action_diff_batch).parameters["num_samples"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY


def _vlm(hidden, heads):
    cfg = types.SimpleNamespace(hidden_size=hidden, num_attention_heads=heads)
    return types.SimpleNamespace(llm_backbone=types.SimpleNamespace(llm=types.SimpleNamespace(config=cfg)))


def test_engine_capability_rule():
    import warnings
    from mla_amd.infer import BatchedPrefixCachedEps, BatchedSampleGroupsEps, SampleGroupsEps
    E = BatchedSampleGroupsEps
    assert (E.MAX_ROWS, E.MAX_R, E.BUCKET) == (256, 64, 64)
    assert not issubclass(E, BatchedPrefixCachedEps) and not issubclass(E, SampleGroupsEps)
    assert E.supports_batch_samples(_vlm(4096, 32), 16) and E.supports_batch_samples(_vlm(256, 2), 63)
    v = _vlm(256, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not E.supports_batch_samples(v, 3, warn=False)                   # the plain predicate never warns
    with pytest.warns(RuntimeWarning, match="head_dim 64"):
        assert not E.supports_batch_samples(v, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not E.supports_batch_samples(v, 3)                               # once per shape
    with pytest.warns(RuntimeWarning, match="65 suffix rows per sample"):
        assert not E.supports_batch_samples(_vlm(256, 2), 64)


# ------------------------------------------------------------------------------------------------ argument validation, no launch
def test_attn_chunk_ragged_groups_validates_on_the_host():
    from mla_amd import hip
    lib = hip.lib()
    assert "mla_attn_chunk_ragged_groups" in hip._SIGNATURES and callable(hip.attn_chunk_ragged_groups)

    def rc(q=P, pl=P, B=3, G=3, H=2, head_dim=128, S_cap=128, R=17, ld=768, bs=768 * 128, ld_o=256):
        return lib.mla_attn_chunk_ragged_groups(q, P, P, P, B, G, H, head_dim, pl, S_cap, R, ld, bs, ld_o, 0.1, None)
    for kw, msg in [(dict(q=None), b"null pointer"), (dict(pl=None), b"null pointer"), (dict(head_dim=64), b"head_dim must be 128"),
                    (dict(R=65), b"1 <= R <= 64"), (dict(R=0), b"1 <= R <= 64"), (dict(G=0), b"G >= 1"), (dict(B=0), b"B >= 1"),
                    (dict(S_cap=50), b"S_cap (50) must hold the G * R suffix rows"), (dict(ld=770), b"16-B aligned"),
                    (dict(bs=12), b"sample stride"), (dict(q=ctypes.c_void_p(18)), b"16-B aligned")]:
        assert rc(**kw) < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())
    gw = lambda g, o: lib.mla_attn_chunk_ragged_groups_gw(P, P, P, P, 3, 3, 2, 128, P, 128, 17, 768, 768 * 128, 256, 0.1, g, o, None)  # noqa: E731
    assert gw(3, -1) < 0 and b"groups per workgroup" in lib.mla_last_error()
    assert gw(2, 2) < 0 and b"order must be" in lib.mla_last_error()


def test_gemm_suffix_pos_validates_on_the_host():
    from mla_amd import hip
    lib = hip.lib()
    assert "mla_gemm_suffix_bf16_pos" in hip._SIGNATURES and "mla_gemm_suffix_w8_pos" in hip._SIGNATURES

    def bf(x=P, M=136, N=256, K=4096, slot=P, cap=64, cos=P, sin=P, rope_cols=128, pos=P, rope_rows=64, rpb=17):
        return lib.mla_gemm_suffix_bf16_pos(x, K, P, K, P, N, 0, rpb, slot, cap, None, 0, M, N, K, cos, sin, rope_cols, pos, rope_rows, None)

    def w8(scale=P, M=136, N=256, K=4096, pos=P, rope_rows=64, cos=P, sin=P):
        return lib.mla_gemm_suffix_w8_pos(P, K, P, K, scale, P, N, 0, 17, P, 64, None, 0, M, N, K, cos, sin, 128, pos, rope_rows, None)
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(M=257), b"1 <= M <= 256"), (dict(cap=16), b"cap_rows (16) must hold the 17 rows"),
                    (dict(cos=None, sin=None, rope_cols=0), b"rope_pos needs the RoPE tables"), (dict(rope_rows=0), b"rope_rows >= 1"),
                    (dict(cos=None), b"RoPE epilogue needs both tables")]:
        assert bf(**kw) < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())
    for kw, msg in [(dict(scale=None), b"null pointer"), (dict(K=4104), b"K % 16 == 0"), (dict(rope_rows=-3), b"rope_rows >= 1"),
                    (dict(cos=None, sin=None), b"rope_pos needs the RoPE tables")]:
        assert w8(**kw) < 0 and msg in lib.mla_last_error(), (kw, lib.mla_last_error())
