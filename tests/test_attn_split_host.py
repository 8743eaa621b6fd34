"""CPU: the host side of the split-key suffix attention (mla_attn_chunk_split, MLA.predict_action_diff(suffix_attention="split")).

The launcher's plan is a pure host function and hip.plan_attn_split mirrors it; every argument error of the launcher is raised on the
host before any launch (the pointers handed in here are never dereferenced); the argument errors of suffix_attention= are raised before
the model is touched."""
import ctypes

import pytest

BS, HS = (1, 3), (2, 32)
RS = (1, 2, 8, 9, 16, 17, 64)
CUS = (256, 64)


def _skvs(R):
    return sorted({R, 63, 64, 65, 130, 547, 2100} - {s for s in (63, 64, 65, 130, 547, 2100) if s < R})


def test_plan_mirror_is_the_librarys_plan():
    from mla_amd import hip
    n = 0
    for cus in CUS:
        for B in BS:
            for H in HS:
                for R in RS:
                    for S_kv in _skvs(R):
                        p = hip.plan_attn_split(B, H, R, S_kv, cus)
                        assert tuple(p)[:4] == hip.attn_split_plan(B, H, R, S_kv, cus), (B, H, R, S_kv, cus)
                        nT, base = -(-S_kv // 64), B * H * -(-R // 16)
                        assert 1 <= p.splits <= nT
                        assert p.tiles_per_split == -(-nT // p.splits)         # the larger ranges'; sizes differ by at most one tile
                        assert p.workgroups == base * p.splits
                        assert (p.splits == 1) == (p.ws_bytes == 0) == (p.combine_workgroups == 0)
                        if cus == 256:                                   # the launcher plans for 256 CUs
                            assert hip.attn_split_ws_bytes(B, H, R, S_kv) == p.ws_bytes
                        if p.splits > 1:
                            assert p.ws_bytes == B * H * R * p.splits * 130 * 4 and p.combine_workgroups == -(-B * H * R // 4)
                            assert base * p.splits <= cus                # one workgroup per CU at the most
                            assert -(-nT // (p.splits - 1)) > hip.ATTN_SPLIT_WAVES      # one range fewer would need a second pass
                            assert nT // p.splits >= 2                   # every range keeps at least two tiles
                        elif nT > hip.ATTN_SPLIT_WAVES:
                            assert 2 * base > cus                        # more than one pass and no split: the chip is full
                        if base >= 2 * cus:
                            assert p.splits == 1
                        n += 1
    assert n == 2 * 2 * 2 * sum(len(_skvs(R)) for R in RS)


def test_plan_splits_the_batch_1_step_and_not_a_full_grid():
    from mla_amd import hip
    p = hip.plan_attn_split(1, 32, 2, 547)
    assert p.splits > 1 and p.workgroups == 32 * p.splits
    assert hip.plan_attn_split(1, 32, 17, 562).splits > 1
    for B, H, R, cus in [(16, 32, 2, 256), (4, 32, 64, 256), (2, 32, 17, 64), (3, 32, 64, 64)]:
        assert B * H * -(-R // 16) >= 2 * cus
        assert hip.plan_attn_split(B, H, R, 2100, cus).splits == 1
    assert hip.plan_attn_split(1, 32, 2, 63).splits == 1                  # one tile: nothing to cut
    with pytest.raises(ValueError):
        hip.plan_attn_split(1, 32, 65, 547)
    with pytest.raises(ValueError):
        hip.plan_attn_split(1, 32, 8, 7)


def test_explicit_splits_workspace_bytes():
    from mla_amd import hip
    assert hip.attn_split_ws_bytes(1, 32, 2, 547, 1) == 0
    assert hip.attn_split_ws_bytes(1, 32, 2, 547, 9) == 32 * 2 * 9 * 130 * 4
    assert hip.attn_split_ws_bytes(2, 2, 64, 130, 3) == 2 * 2 * 64 * 3 * 130 * 4
    assert hip.attn_split_ws_bytes(1, 32, 2, 547, 10) == -1 and b"splits" in hip.lib().mla_last_error()
    assert hip.attn_split_ws_bytes(1, 32, 2, 547, -1) == -1
    assert hip.attn_split_ws_bytes(1, 32, 65, 547, 0) == -1
    assert hip.attn_split_ws_bytes(1, 32, 9, 8, 0) == -1
    assert hip.attn_split_ws_bytes(0, 32, 2, 547, 0) == -1


def test_launcher_refuses_bad_arguments_on_the_host():
    """P is not a device pointer: a launcher that got past its checks would fault here, not return."""
    from mla_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p(64)

    def run(q=P, k=P, v=P, o=P, B=1, H=2, D=128, S_kv=130, R=2, ld=768, bs=768 * 133, ld_o=256, splits=2, ws=P, ws_bytes=1 << 20):
        return lib.mla_attn_chunk_split(q, k, v, o, B, H, D, S_kv, R, ld, bs, ld_o, 0.088, splits, ws, ws_bytes, None)

    def refused(word, **kw):
        rc = run(**kw)
        msg = lib.mla_last_error()
        assert rc < 0 and b"mla_attn_chunk_split" in msg and word in msg, (kw, rc, msg)

    refused(b"null", q=None)
    refused(b"null", k=None)
    refused(b"null", v=None)
    refused(b"null", o=None)
    refused(b"head_dim", D=64)
    refused(b"R 0", R=0)
    refused(b"R 65", R=65, S_kv=547)
    refused(b"S_kv 5", R=8, S_kv=5)
    refused(b"R 2", B=0)
    refused(b"R 2", H=0)
    refused(b"aligned", q=ctypes.c_void_p(72))
    refused(b"aligned", ld=772)
    refused(b"aligned", o=ctypes.c_void_p(66))
    refused(b"splits", splits=-1)
    refused(b"[0, 3]", splits=4)                                          # S_kv 130: three tiles
    refused(b"[0, 1]", splits=2, S_kv=64)
    refused(b"workspace", ws=None)
    refused(b"workspace", ws=None, ws_bytes=0, splits=3)
    refused(b"workspace", ws_bytes=2 * 2 * 2 * 130 * 4 - 1)               # B H R splits states of 130 words, one byte short
    refused(b"workspace", ws=ctypes.c_void_p(68))
    refused(b"workspace", B=1, H=32, R=2, S_kv=547, bs=96 * 128 * 550, ld=96 * 128, ld_o=4096, splits=0, ws=None, ws_bytes=0)   # the plan splits
    refused(b"workspace", B=1, H=32, R=2, S_kv=547, bs=96 * 128 * 550, ld=96 * 128, ld_o=4096, splits=0,
            ws_bytes=hip.attn_split_ws_bytes(1, 32, 2, 547) - 1)
    out = (ctypes.c_int * 4)()
    assert lib.mla_attn_chunk_split_plan(1, 32, 2, 547, 256, None) < 0 and b"null" in lib.mla_last_error()
    assert lib.mla_attn_chunk_split_plan(1, 32, 65, 547, 256, out) < 0 and b"R 65" in lib.mla_last_error()
    assert lib.mla_attn_chunk_split_plan(1, 32, 2, 547, 0, out) < 0 and b"cus 0" in lib.mla_last_error()
    assert lib.mla_attn_chunk_split_plan(1, 32, 2, 1, 256, out) < 0


def test_wrapper_rejects_host_tensors():
    import torch
    from mla_amd import hip
    with pytest.raises((RuntimeError, TypeError)):
        hip.attn_chunk_split(torch.zeros(1, 70, 768, dtype=torch.bfloat16), 1, 2, 128, 66, 2, 0.088)
    with pytest.raises((RuntimeError, TypeError)):
        hip.attn_chunk_split(torch.zeros(1, 70, 768), 1, 2, 128, 66, 2, 0.088)


def test_check_suffix_attention():
    from mla_amd import infer
    assert infer.MODES["suffix_attention"].values == ("head", "split")
    infer.check_mode("suffix_attention", "head")
    infer.check_mode("suffix_attention", "head", reuse_prefix=False)   # today's path takes every combination
    infer.check_mode("suffix_attention", "split")
    infer.check_mode("suffix_attention", "split", True)
    for bad in ("bogus", "Split", None, "", "decode"):
        with pytest.raises(ValueError, match="suffix_attention"):
            infer.check_mode("suffix_attention", bad)
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        infer.check_mode("suffix_attention", "split", reuse_prefix=False)
    with pytest.raises(ValueError, match="does not serve"):
        infer.needs_engine("PrefixCachedEps", 70, suffix_attention="split")
    infer.needs_engine("PrefixCachedEps", 70, suffix_attention="head")
    with pytest.raises(NotImplementedError, match="ragged / groups"):
        infer.suffix_attention_single_only("split", "predict_action_diff_batch with 2 observations")
    infer.suffix_attention_single_only("head", "anything")


def test_engine_key_and_constructor_take_the_mode():
    """The mode is a constructor argument of every engine's base and part of PrefixCachedEps.for_inputs' signature; an unknown value is
    refused before the model is read."""
    import inspect
    from mla_amd import infer
    assert inspect.signature(infer.PrefixCachedEps.for_inputs).parameters["suffix_attention"].default == "head"
    assert inspect.signature(infer._CachedEpsBase.__init__).parameters["modes"].default.suffix_attention == "head"
    with pytest.raises(ValueError, match="suffix_attention"):
        infer.PrefixCachedEps(object(), 1, infer.engine_modes(suffix_weights="bf16", prefill="train", suffix_attention="bogus"))
    with pytest.raises(ValueError, match="suffix_attention"):
        infer.PrefixCachedEps.for_inputs(object(), None, suffix_attention="bogus")


def _public_calls():
    from mla_amd.mla import MLA
    return [("predict_action_diff", lambda **kw: MLA.predict_action_diff(object(), **kw)),
            ("predict_action_diff_samples", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=2, **kw)),
            ("predict_action_diff_samples[1]", lambda **kw: MLA.predict_action_diff_samples(object(), num_samples=1, **kw)),
            ("predict_action_diff_batch", lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], **kw)),
            ("predict_action_diff_batch[1]", lambda **kw: MLA.predict_action_diff_batch(object(), [None], [None], **kw)),
            ("predict_action_diff_batch[samples]",
             lambda **kw: MLA.predict_action_diff_batch(object(), [None, None], [None, None], num_samples=3, **kw))]


@pytest.mark.parametrize("name,call", _public_calls(), ids=[n for n, _ in _public_calls()])
def test_suffix_attention_errors_are_raised_before_anything_is_computed(name, call):
    """object() stands in for the model: the errors are raised before the model, its device or its inputs are touched."""
    with pytest.raises(ValueError, match="suffix_attention"):
        call(suffix_attention="bogus")
    with pytest.raises(ValueError, match="reuse_prefix=True"):
        call(suffix_attention="split", reuse_prefix=False)
    with pytest.raises(ValueError, match="suffix_attention"):
        call(suffix_attention="bogus", suffix_weights="fp8", sampler="device")


@pytest.mark.parametrize("name", ["predict_action_diff_samples", "predict_action_diff_batch", "predict_action_diff_batch[samples]"])
def test_split_on_the_batch_and_samples_routes_is_not_implemented(name):
    call = dict(_public_calls())[name]
    with pytest.raises(NotImplementedError, match="ragged / groups"):
        call(suffix_attention="split")
    with pytest.raises(NotImplementedError, match="predict_action_diff"):
        call(suffix_attention="split", suffix_weights="fp8", sampler="device")


@pytest.mark.parametrize("name", ["predict_action_diff", "predict_action_diff_samples[1]", "predict_action_diff_batch[1]"])
def test_split_is_accepted_where_the_call_is_predict_action_diff(name):
    """These routes get past the argument checks with "split" and only then reach for the model (object() has none)."""
    call = dict(_public_calls())[name]
    with pytest.raises(AttributeError):
        call(suffix_attention="split")
    with pytest.raises(AttributeError):
        call(suffix_attention="head")


def test_new_kernels_use_no_scratch_and_the_object_keeps_no_state(tmp_path):
    """The compiler's resource report for gfx950 (device-only compile of attn_split.hip with the build's flags): three kernels -- the
    state launch plain (attn_chunk_split_kernel) and with groups (attn_groups_split_kernel), and the combine launch -- and no scratch;
    there is no finishing form: one split is mla_attn_chunk itself, which the object imports. The built object references no
    allocation, memset or memcpy entry point of the HIP runtime, no std::map and no mutex."""
    import os
    import re
    import subprocess
    import __graft_entry__ as g
    g.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "mla_amd", "csrc", "attn_split.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "attn_split_dev.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    report, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            report[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in report.items()
               if "attn_chunk_split_kernel" in k or "attn_groups_split_kernel" in k or "attn_split_combine_kernel" in k}
    print(kernels)
    assert len(kernels) == 3 and len(report) == 3, list(report)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    obj = os.path.join(root, "mla_amd", "csrc", "build", "attn_split.o")
    und = subprocess.run(["nm", "-u", "-C", obj], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bmla_attn_chunk$", und, re.M), und                   # splits == 1 is the head form's own launch
    bad = [ln.strip() for ln in und.splitlines()
           if re.search(r"hipMalloc|hipFree|hipMemset|hipMemcpy|hipHostMalloc|std::_Rb_tree|pthread_mutex|std::mutex", ln)]
    assert not bad, bad
