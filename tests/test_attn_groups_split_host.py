"""CPU: the host side of the split-key attention of the multi-row engines (mla_attn_groups_split,
MLA.predict_action_diff_batch / predict_action_diff_samples(groups_attention="split")).

The plan is mla_attn_chunk_split_plan at (B * G, H, R, S_max); every argument error of the launcher is raised on the host before any launch
(the pointers handed in here are never dereferenced); the argument errors of groups_attention= are raised before the model is touched."""
import ctypes
import inspect

import pytest


def test_plan_helper_is_the_split_plan_at_the_groups_shape():
    from mla_amd import hip
    n = 0
    for H in (2, 32):
        for R in (1, 2, 9, 16, 17, 64):
            for G in (1, 2, 3, 5):
                for S_p in (0, 47, 128, 545):                                 # one prefix, G groups behind it
                    S_max, plan = hip.attn_groups_split_plan(1, G, H, R, S_p, False)
                    assert S_max == S_p + R and plan == hip.attn_split_plan(G, H, R, S_max), (G, H, R, S_p)
                    n += 1
                for B in (1, 2, 3):
                    for S_cap in (G * R, 320, 640):                           # B samples, the lengths in device memory
                        if S_cap < G * R:
                            continue
                        S_max, plan = hip.attn_groups_split_plan(B, G, H, R, S_cap, True)
                        assert S_max == S_cap - (G - 1) * R and plan == hip.attn_split_plan(B * G, H, R, S_max), (B, G, H, R, S_cap)
                        n += 1
    assert n > 500
    with pytest.raises(ValueError):
        hip.attn_groups_split_plan(2, 2, 32, 2, 545, False)                   # one sample without prefix_len
    with pytest.raises(ValueError):
        hip.attn_groups_split_plan(2, 3, 32, 17, 50, True)                    # S_cap < G * R
    with pytest.raises(ValueError):
        hip.attn_groups_split_plan(1, 0, 32, 2, 545, False)


@pytest.mark.parametrize("BG,R,S_kv,splits", [(2, 2, 547, 3), (4, 2, 547, 2), (5, 2, 547, 1), (2, 17, 562, 2), (3, 17, 562, 1)])
def test_where_the_plan_splits_at_7b(BG, R, S_kv, splits):
    """The issue's table (H = 32, 256 CUs): the form acts for B G <= 4 at R <= 16 and B G <= 2 at 17 <= R <= 32."""
    from mla_amd import hip
    assert hip.attn_groups_split_plan(1, BG, 32, R, S_kv - R, False) == (S_kv, hip.attn_split_plan(BG, 32, R, S_kv))
    assert hip.attn_groups_split_plan(1, BG, 32, R, S_kv - R, False)[1][0] == splits
    assert hip.attn_groups_split_plan(BG, 1, 32, R, S_kv, True)[1][0] == splits          # G = 1: S_max = S_cap
    assert hip.plan_attn_split(BG, 32, R, S_kv).splits == splits


def test_launcher_refuses_bad_arguments_on_the_host():
    """P is not a device pointer: a launcher that got past its checks would fault here, not return."""
    from mla_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p(64)

    def run(q=P, k=P, v=P, o=P, B=2, G=2, H=2, D=128, prefix_len=P, S=320, R=9, ld=768, bs=768 * 320, ld_o=256, splits=2, ws=P,
            ws_bytes=1 << 22):
        return lib.mla_attn_groups_split(q, k, v, o, B, G, H, D, prefix_len, S, R, ld, bs, ld_o, 0.088, splits, ws, ws_bytes, None)

    def refused(word, **kw):
        rc = run(**kw)
        msg = lib.mla_last_error()
        assert rc < 0 and b"mla_attn_groups_split" in msg and word in msg, (kw, rc, msg)

    refused(b"null", q=None)
    refused(b"null", o=None)
    refused(b"head_dim", D=64)
    refused(b"R 0", R=0)
    refused(b"R 65", R=65, S=640)
    refused(b"G 0", G=0)
    refused(b"B 0", B=0)
    refused(b"S_cap", S=17, R=9)                                          # ragged: S_cap < G * R
    refused(b"one sample", prefix_len=None, B=2, S=100)                   # B != 1 without prefix_len
    refused(b"S_p", prefix_len=None, B=1, S=-1)
    refused(b"splits", splits=-1)
    refused(b"[0, 5]", splits=6)                                          # S_max = 320 - 9 = 311: five tiles
    refused(b"[0, 2]", prefix_len=None, B=1, S=100, splits=3)             # S_max = 109: two tiles
    refused(b"workspace", ws=None)
    refused(b"workspace", ws=None, ws_bytes=0, splits=3)
    refused(b"workspace", ws_bytes=2 * 2 * 2 * 9 * 2 * 130 * 4 - 1)       # B G H R splits states of 130 words, one byte short
    refused(b"workspace", ws=ctypes.c_void_p(68))
    refused(b"aligned", ld=772)
    refused(b"aligned", q=ctypes.c_void_p(72))
    refused(b"aligned", o=ctypes.c_void_p(66))
    refused(b"stride", bs=768 * 320 + 4)
    # the plan splits (splits = 0): the workspace is needed, and checked, before any launch
    refused(b"workspace", B=2, G=1, H=32, R=2, S=547, ld=96 * 128, bs=96 * 128 * 547, ld_o=4096, splits=0, ws=None, ws_bytes=0)
    refused(b"workspace", prefix_len=None, B=1, G=2, H=32, R=2, S=545, ld=96 * 128, bs=0, ld_o=4096, splits=0,
            ws_bytes=hip.attn_split_ws_bytes(2, 32, 2, 547) - 1)


def test_wrapper_rejects_host_tensors():
    import torch
    from mla_amd import hip
    with pytest.raises((RuntimeError, TypeError)):
        hip.attn_groups_split(torch.zeros(70, 768, dtype=torch.bfloat16), 1, 2, 2, 128, 66, 2, 0.088)
    with pytest.raises((RuntimeError, TypeError)):
        hip.attn_groups_split(torch.zeros(2, 70, 768), 2, 2, 2, 128, torch.zeros(2, dtype=torch.int32), 2, 0.088)


def test_check_groups_attention():
    from mla_amd import infer
    assert infer.MODES["groups_attention"].values == ("head", "split")
    assert infer.MODES["suffix_attention"].values == ("head", "split")
    infer.check_mode("groups_attention", "head")
    infer.check_mode("groups_attention", "head", reuse_prefix=False)
    infer.check_mode("groups_attention", "split")
    for bad in ("bogus", "Split", None, ""):
        with pytest.raises(ValueError, match="groups_attention"):
            infer.check_mode("groups_attention", bad)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        infer.check_mode("groups_attention", "split", reuse_prefix=False)
    with pytest.raises(ValueError, match="does not serve"):
        infer.needs_engine("SampleGroupsEps", 70, groups_attention="split")
    infer.needs_engine("SampleGroupsEps", 70, groups_attention="head")


def test_engines_take_the_mode():
    from mla_amd import infer
    for fn in (infer.BatchedPrefixCachedEps.for_batch, infer.SampleGroupsEps.for_inputs, infer.BatchedSampleGroupsEps.for_batch):
        assert inspect.signature(fn).parameters["suffix_attention"].default == "head"
    with pytest.raises(ValueError, match="groups_attention"):
        infer.SampleGroupsEps.for_inputs(object(), None, 1, 2, suffix_attention="bogus")
    with pytest.raises(ValueError, match="groups_attention"):
        next(infer.BatchedPrefixCachedEps.for_batch(object(), [[1]], 1, suffix_attention="bogus"))
    with pytest.raises(ValueError, match="groups_attention"):
        next(infer.BatchedSampleGroupsEps.for_batch(object(), [[1]], 1, 2, suffix_attention="bogus"))


def _public_calls():
    from mla_amd.mla import MLA
    return [("predict_action_diff_samples", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=2, **kw)),
            ("predict_action_diff_samples[1]", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=1, **kw)),
            ("predict_action_diff_batch", lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], **kw)),
            ("predict_action_diff_batch[1]", lambda **kw: MLA.predict_action_diff_batch(object(), [None], [None], **kw)),
            ("predict_action_diff_batch[samples]",
             lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], num_samples=3, **kw))]


def test_the_keyword_is_keyword_only_with_default_head():
    from mla_amd.mla import MLA
    for fn in (MLA.predict_action_diff_batch, MLA.predict_action_diff_samples):
        p = inspect.signature(fn).parameters["groups_attention"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "head"
    assert "groups_attention" not in inspect.signature(MLA.predict_action_diff).parameters


@pytest.mark.parametrize("name,call", _public_calls(), ids=[n for n, _ in _public_calls()])
def test_groups_attention_errors_are_raised_before_anything_is_computed(name, call):
    """object() stands in for the model: the errors are raised before the model, its device or its inputs are touched."""
    with pytest.raises(ValueError, match="groups_attention"):
        call(groups_attention="bogus")
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        call(groups_attention="split", reuse_prefix=False)
    with pytest.raises(ValueError, match="groups_attention"):
        call(groups_attention="bogus", suffix_weights="fp8", sampler="device")


@pytest.mark.parametrize("name,call", _public_calls(), ids=[n for n, _ in _public_calls()])
def test_split_gets_past_the_argument_checks_on_every_route(name, call):
    """ "split" is accepted on all routes and only then reaches for the model (object() has none); the suffix_attention refusal of the
    multi-row routes stays what it was."""
    with pytest.raises(AttributeError):
        call(groups_attention="split")
    with pytest.raises(AttributeError):
        call(groups_attention="split", suffix_weights="fp8", sampler="device")
    if not name.endswith("[1]"):
        with pytest.raises(NotImplementedError, match="ragged / groups"):
            call(suffix_attention="split", groups_attention="split")
