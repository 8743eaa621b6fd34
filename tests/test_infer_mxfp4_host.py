"""CPU: the host side of the MXFP4 suffix-weight path -- the CPU statement of the format (mxfp4_quant / mxfp4_dequant, shared with
tests/test_infer_mxfp4_gpu.py) and its own properties, argument validation of mla_quant_mxfp4_rows and the five `_w4` projections (on the
host, before any launch: no GPU needed), and the `suffix_mx` keyword of MLA.predict_action_diff / _samples / _batch."""
import ctypes
import inspect

import pytest
import torch

BF = torch.bfloat16
P = ctypes.c_void_p(16)
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)                              # the e2m1 magnitudes, by 3-bit index
TIES = ((0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0))     # value / 2^e -> grid value


# ------------------------------------------------------------------------------------------------ the CPU statement of the format
def mxfp4_quant(W):
    """OCP MXFP4 of W [N, K] bf16 (CPU, K % 32 == 0) -> (q [N, K / 2] uint8, s [N, K / 32] uint8). Per block of 32 consecutive k of a row:
    amax = m * 2^E (1 <= m < 2, E from the exponent bits), e = clamp(E - 2, -125, 125), s = e + 127 (127 and codes +0 for an all-zero
    block); |w| / 2^e to the nearest of GRID, ties to the even mantissa bit, saturating at 6; nibble = sign (8) | index; element 2 j in the
    low nibble of byte j."""
    assert W.dtype == BF and W.dim() == 2 and W.shape[1] % 32 == 0
    N, K = W.shape
    bits = W.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = (bits & 0x7FFF).view(N, K // 32, 32)
    amax = mag.amax(dim=-1)
    e = ((amax >> 7) - 127 - 2).clamp(-125, 125)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    a = W.double().abs().view(N, K // 32, 32) * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double())[..., None]   # exact
    idx = ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int() + (a >= 1.75).int() + (a > 2.5).int() + (a >= 3.5).int() + (a > 5.0).int())
    nib = idx | (((bits >> 15) & 1).view(N, K // 32, 32) << 3)
    nib = torch.where((amax == 0)[..., None], torch.zeros_like(nib), nib).view(N, K)
    q = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8)
    return q, (e + 127).to(torch.uint8)


def mxfp4_dequant(q, s):
    """(q [N, K / 2], s [N, K / 32]) uint8 (CPU) -> the decoded matrix [N, K] fp64: sign * GRID[index] * 2^(s - 127)."""
    N, K = q.shape[0], q.shape[1] * 2
    q = q.to(torch.int32)
    nib = torch.stack([q & 15, q >> 4], dim=-1).view(N, K)
    val = torch.tensor(GRID, dtype=torch.float64)[nib & 7] * torch.where((nib & 8) != 0, -1.0, 1.0).double()
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), s.double() - 127)
    return (val.view(N, K // 32, 32) * scale[..., None]).view(N, K)


def _rand(shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def quant_case(case):
    """The quantiser's test matrices (bf16, CPU); "strided" is a row block inside a wider buffer (row stride 768 > K = 256)."""
    if case == "300x512":
        W = _rand((300, 512), 1, 0.05)
        W[7] = 0.0                                       # all-zero row: every block byte 127, every code +0
        W[11] *= 0.01                                    # std 5e-4 beside a 40.0 outlier: that block's small values round to 0 / 0.5 steps
        W[11, 17] = 40.0
        return W.to(BF)
    if case == "7x32":
        return _rand((7, 32), 3, 0.05).to(BF)            # one block per row
    return _rand((40, 768), 2, 0.05).to(BF)[3:23, 128:384]


def test_decoded_values_are_bf16_and_zero_blocks_have_no_code():
    for case in ("300x512", "7x32", "strided"):
        W = quant_case(case)
        q, s = mxfp4_quant(W)
        assert q.shape == (W.shape[0], W.shape[1] // 2) and s.shape == (W.shape[0], W.shape[1] // 32)
        d = mxfp4_dequant(q, s)
        assert torch.equal(d.to(BF).double(), d), "a decoded value is not a bf16"
        assert not bool((s == 255).any())
        zero = (W.float().view(W.shape[0], -1, 32).abs().amax(-1) == 0)
        assert bool((s[zero] == 127).all()) and not bool(q.view(W.shape[0], -1, 16)[zero].any())
        # round to nearest: no grid point of the block's scale is closer than the chosen one (saturation: beyond 6 the nearest is 6)
        scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), s.double() - 127).repeat_interleave(32, dim=1)
        cand = torch.tensor(GRID, dtype=torch.float64)[None, None, :] * scale[..., None]
        best = (W.double().abs()[..., None] - cand).abs().amin(-1)
        assert torch.equal((W.double().abs() - d.abs()).abs(), best)
        assert bool(((d == 0) | (torch.sign(d) == torch.sign(W.double()))).all())
    q, s = mxfp4_quant(quant_case("300x512"))
    assert bool((s[7] == 127).all()) and not bool(q[7].any())
    nib = torch.stack([q & 15, q >> 4], dim=-1).view(-1)
    assert sorted(set(nib.tolist())) == list(range(16)), "the test matrix does not use all eight magnitudes with both signs"
    # 40 = 1.25 * 2^5: scale 2^3, 40 / 8 = 5 ties to 4; beside it every small value of the block rounds to zero
    assert int(s[11, 0]) == 5 - 2 + 127 and int((q[11, :16] & 7 != 0).sum() + (q[11, :16] >> 4 & 7 != 0).sum()) == 1
    assert float(mxfp4_dequant(q, s)[11, 17]) == 32.0


@pytest.mark.parametrize("e", [-3, 0, 4])
def test_ties_round_to_the_even_mantissa_bit_and_the_maximum_clips(e):
    """A block whose maximum is 4 * 2^e (so the scale is 2^e) with every tie threshold in it, both signs; then maxima in [6, 8) * 2^e."""
    row = torch.zeros(64, dtype=torch.float64)
    row[0] = 4.0
    for i, (t, _) in enumerate(TIES):
        row[1 + i], row[9 + i] = t, -t
    row[32] = 7.5                                                            # second block: the maximum lies in [6, 8) * 2^e and clips to 6
    row[33], row[34], row[35] = 6.0, -7.0, 5.0
    W = (row * 2.0 ** e)[None, :].to(BF)
    assert torch.equal(W.double(), (row * 2.0 ** e)[None, :])                # every input is a bf16
    q, s = mxfp4_quant(W)
    assert s.tolist() == [[e + 127, e + 127]]
    d = mxfp4_dequant(q, s)[0] / 2.0 ** e
    assert float(d[0]) == 4.0
    for i, (t, want) in enumerate(TIES):
        assert float(d[1 + i]) == want and float(d[9 + i]) == -want, (t, float(d[1 + i]))
    assert [float(v) for v in d[32:36]] == [6.0, 6.0, -6.0, 4.0]
    # the sign survives a magnitude that rounds to zero
    assert int(q[0, (9 + 0) // 2] >> 4) == 8                                  # element 9 = -0.25 -> -0: high nibble of byte 4


def test_scale_exponent_is_clamped():
    W = torch.zeros(2, 32, dtype=torch.float64)
    W[0, 0], W[0, 1] = 2.0 ** -126, 2.0 ** -127                              # E - 2 = -128 -> e = -125
    W[1, 0] = 1.5 * 2.0 ** 127                                               # E - 2 = 125
    q, s = mxfp4_quant(W.to(BF))
    assert s.tolist() == [[2], [252]]
    d = mxfp4_dequant(q, s)
    assert float(d[0, 0]) == 2.0 ** -126 and float(d[1, 0]) == 1.5 * 2.0 ** 127


# ------------------------------------------------------------------------------------------------ argument checks, on the host
def _proj(lib, name, x=P, W=P, w_scale=P, out=P, M=2, N=64, K=4096, pre=0, ldw=None, lds=None):
    return getattr(lib, name)(x, K, W, K // 2 if ldw is None else ldw, w_scale, K // 32 if lds is None else lds, out, N, 0, M, None, 0, M, N, K,
                              pre, None, 1e-5, None, None, 0, None)


@pytest.mark.parametrize("name,mmax", [("mla_gemv_w4", 8), ("mla_gemm_skinny_w4", 64)])
def test_w4_projections_reject_bad_arguments(name, mmax):
    from mla_amd import hip
    lib = hip.lib()
    rng = f"1 <= M <= {mmax}".encode()
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(w_scale=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(K=4112), b"K % 32 == 0"), (dict(K=16), b"K % 32 == 0"), (dict(M=0), rng),
                    (dict(M=mmax + 1), rng), (dict(pre=1), b"pre must be"), (dict(pre=3), b"pre must be"),
                    (dict(ldw=2056), b"16-B aligned"), (dict(ldw=1024), b"16-B aligned"), (dict(lds=64), b"scale row shorter")]:
        rc = _proj(lib, name, **kw)
        assert rc < 0 and name.encode() in lib.mla_last_error() and msg in lib.mla_last_error(), (kw, lib.mla_last_error())
    rc = getattr(lib, name)(P, 4096, P, 2048, P, 128, P, 64, 0, 2, None, 0, 2, 64, 4096, 0, None, 1e-5, ctypes.c_void_p(64), None, 64, None)
    assert rc < 0 and b"RoPE epilogue needs both tables" in lib.mla_last_error()


def test_gemv_w4_keeps_the_lds_limit_of_the_bf16_rows():
    from mla_amd import hip
    lib = hip.lib()
    rc = _proj(lib, "mla_gemv_w4", M=8, K=11008)
    assert rc < 0 and b"must fit the 160 KiB of LDS" in lib.mla_last_error()


def test_gateup_w4_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()
    name = "mla_gemm_skinny_gateup_swiglu_w4"

    def gu(x=P, W=P, s=P, out=P, M=17, I=64, K=512, ldw=None, lds=None, ldo=None):
        return getattr(lib, name)(x, K, W, K // 2 if ldw is None else ldw, s, K // 32 if lds is None else lds, out, I if ldo is None else ldo,
                                  M, I, K, None)
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(s=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(K=528), b"K % 32 == 0"), (dict(M=0), b"1 <= M <= 64"), (dict(M=65), b"1 <= M <= 64"),
                    (dict(I=60), b"I % 8 == 0"), (dict(ldw=264), b"16-B aligned"), (dict(ldw=128), b"16-B aligned"),
                    (dict(lds=8), b"scale row shorter"), (dict(ldo=32), b"ldo")]:
        rc = gu(**kw)
        assert rc < 0 and name.encode() in lib.mla_last_error() and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


@pytest.mark.parametrize("name", ["mla_gemm_suffix_w4", "mla_gemm_suffix_w4_pos"])
def test_suffix_w4_rejects_bad_arguments(name):
    from mla_amd import hip
    lib = hip.lib()
    pos = name.endswith("_pos")

    def sx(x=P, W=P, s=P, out=P, M=85, N=64, K=512, ldw=None, lds=None, rpb=17, slot=None, cap=0, cos=None, sin=None, rope_cols=0, rope_pos=None,
           rope_rows=0):
        tail = (rope_pos, rope_rows, None) if pos else (None,)
        return getattr(lib, name)(x, K, W, K // 2 if ldw is None else ldw, s, K // 32 if lds is None else lds, out, N, 0, rpb, slot, cap, None, 0,
                                  M, N, K, cos, sin, rope_cols, *tail)
    cases = [(dict(x=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(s=None), b"null pointer"), (dict(out=None), b"null pointer"),
             (dict(K=528), b"K % 32 == 0"), (dict(K=0), b"K % 32 == 0"), (dict(M=0), b"1 <= M <= 256"), (dict(M=257), b"1 <= M <= 256"),
             (dict(ldw=264), b"16-B aligned"), (dict(ldw=128), b"16-B aligned"), (dict(lds=8), b"scale row shorter"),
             (dict(slot=P, cap=5), b"cap_rows"), (dict(cos=P), b"RoPE epilogue needs both tables")]
    if pos:
        cases.append((dict(rope_pos=P, rope_rows=4), b"rope_pos needs the RoPE tables"))
    for kw, msg in cases:
        rc = sx(**kw)
        assert rc < 0 and name.encode() in lib.mla_last_error() and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


def test_mxfp4_quantiser_rejects_bad_arguments():
    from mla_amd import hip
    lib = hip.lib()

    def q(W=P, qq=P, s=P, N=4, K=64, ldw=None, ldq=None, lds=None):
        return lib.mla_quant_mxfp4_rows(W, K if ldw is None else ldw, qq, K // 2 if ldq is None else ldq, s, K // 32 if lds is None else lds, N, K,
                                        None)
    for kw, msg in [(dict(W=None), b"null pointer"), (dict(qq=None), b"null pointer"), (dict(s=None), b"null pointer"),
                    (dict(K=48), b"K % 32 == 0"), (dict(K=0), b"K % 32 == 0"), (dict(N=0), b"N >= 1"), (dict(ldw=60), b"16-B aligned"),
                    (dict(ldq=40), b"16-B aligned"), (dict(ldq=16), b"16-B aligned"), (dict(lds=1), b"16-B aligned")]:
        rc = q(**kw)
        assert rc < 0 and b"mla_quant_mxfp4_rows" in lib.mla_last_error() and msg in lib.mla_last_error(), (kw, lib.mla_last_error())


# ------------------------------------------------------------------------------------------------ the keyword
def test_suffix_mx_is_a_named_argument_and_checked():
    from mla_amd import infer
    from mla_amd.mla import MLA
    methods = (MLA.predict_action_diff, MLA.predict_action_diff_samples, MLA.predict_action_diff_batch)
    for fn in methods:
        p = inspect.signature(fn).parameters["suffix_mx"]
        assert p.default == "off" and p.kind in (p.KEYWORD_ONLY, p.POSITIONAL_OR_KEYWORD)
    mode = infer.MODES["suffix_mx"]
    assert mode.values == ("off", "fp4", "fp4_as_bf16") and mode.needs == "reuse_prefix" and mode.tag == "mx:"
    assert list(infer.MODES)[-1] == "suffix_mx" and infer.Modes._fields[-1] == "suffix_mx"
    order = infer.CHECK_ORDER
    assert order.index("suffix_mx") == order.index("suffix_weights") + 1
    with pytest.raises(ValueError, match="suffix_mx"):
        MLA.predict_action_diff(object(), suffix_mx="int4")
    with pytest.raises(ValueError, match="suffix_mx"):
        MLA.predict_action_diff_samples(object(), None, None, None, suffix_mx="FP4")
    with pytest.raises(ValueError, match="suffix_mx"):
        MLA.predict_action_diff_batch(object(), [None], [None], suffix_mx="nvfp4")
    with pytest.raises(ValueError, match="suffix_mx"):
        infer.PrefixCachedEps.for_inputs(object(), None, suffix_mx="e2m1")
    for value in mode.values:
        infer.check_mode("suffix_mx", value)


@pytest.mark.parametrize("mx", ["fp4", "fp4_as_bf16"])
def test_suffix_mx_refuses_other_suffix_weights_and_the_whole_forward_sampler(mx):
    """Both keywords choose what the suffix pass streams: together they are an error that names suffix_mx, before the model is touched;
    so is the whole-forward sampler."""
    from mla_amd.mla import MLA
    for sw in ("fp8", "fp8_as_bf16"):
        with pytest.raises(ValueError, match="suffix_mx"):
            MLA.predict_action_diff(object(), suffix_mx=mx, suffix_weights=sw)
        with pytest.raises(ValueError, match="suffix_mx"):
            MLA.predict_action_diff_samples(object(), None, None, None, suffix_mx=mx, suffix_weights=sw)
        with pytest.raises(ValueError, match="suffix_mx"):
            MLA.predict_action_diff_batch(object(), [None], [None], suffix_mx=mx, suffix_weights=sw)
    with pytest.raises(ValueError, match="suffix_mx"):
        MLA.predict_action_diff(object(), suffix_mx=mx, reuse_prefix=False)
    with pytest.raises(ValueError, match="suffix_mx"):
        MLA.predict_action_diff_samples(object(), None, None, None, suffix_mx=mx, reuse_prefix=False)
    with pytest.raises(ValueError, match="suffix_mx"):
        MLA.predict_action_diff_batch(object(), [None], [None], suffix_mx=mx, reuse_prefix=False)


def test_engine_key_gains_the_mx_tag_only_off_the_default():
    from mla_amd import infer

    class Vlm:
        pass

    class Eng(infer._CachedEpsBase):
        def __init__(self, vlm, *ctor):
            self.ctor = ctor
    vlm = Vlm()
    for value, tags in (("off", ()), ("fp4", ("mx:fp4",)), ("fp4_as_bf16", ("mx:fp4_as_bf16",))):
        Eng._engine(vlm, "_store", ("k",), (), **infer.Modes(suffix_mx=value)._asdict())
        assert ("k",) + tags in vlm.__dict__["_store"], (value, list(vlm.__dict__["_store"]))
    assert len(vlm.__dict__["_store"]) == 3
    Eng._engine(vlm, "_store", ("k",), (), **infer.Modes(suffix_mx="fp4", prefill="compact")._asdict())
    assert ("k", "prefill:compact", "mx:fp4") in vlm.__dict__["_store"]       # appended behind the existing tags
