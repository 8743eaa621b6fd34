"""hip.WEIGHT_FORMATS, the one table of the suffix projections' weight formats (CPU, no library): every row x every kernel family has its
wrapper here and its declaration in include/mla_hip.h, the wrapper calls that symbol with the declared number of arguments, and it
refuses operands that are not the row's -- TypeError for a dtype, AssertionError for a scale of another shape and, for block scales, a K
off the row's granularity (the K granularity of bf16 and w8 is the launchers' refusal: tests/test_infer_suffix_operand_gpu.py). The
device check of _req is taken out (dtype only) and hip.call records instead of launching."""
import pytest
import torch

from mla_amd import hip, infer

M, N, K = 4, 16, 64
BF16 = torch.bfloat16
CASES = [(family, fmt) for family in hip.PROJ_FAMILIES for fmt in hip.WEIGHT_FORMATS.values()]
IDS = [f"{family}-{fmt.name}" for family, fmt in CASES]


@pytest.fixture
def calls(monkeypatch):
    def req(t, dtype, name):
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    made = []
    monkeypatch.setattr(hip, "_req", req)
    monkeypatch.setattr(hip, "call", lambda name, *args: made.append((name, args)))
    return made


def operands(fmt, K=K):
    """x, W and the scale (None for bf16) of an [N, K] weight as the row describes them."""
    W = torch.zeros((N, K // fmt.k_per_col), dtype=fmt.dtype)
    scale = None
    if fmt.scale_dtype is not None:
        scale = torch.zeros((N, K // fmt.scale_block) if fmt.scale_block else N, dtype=fmt.scale_dtype)
    return torch.zeros((M, K), dtype=BF16), W, scale


def launch(family, fmt, x, W, scale, **kw):
    fn = getattr(hip, family + fmt.suffix)
    ws = () if fmt.scale_dtype is None else (scale,)
    if family == "gemm_skinny_gateup_swiglu":
        return fn(x, W, *ws)
    return fn(x, W, *ws, torch.zeros((M, N), dtype=BF16), N, 0, M, **kw)


def test_the_rows():
    assert list(hip.WEIGHT_FORMATS) == ["bf16", "w8", "w4"]
    assert [f.suffix for f in hip.WEIGHT_FORMATS.values()] == ["", "_w8", "_w4"]
    bf16, w8, w4 = hip.WEIGHT_FORMATS.values()
    assert (bf16.dtype, bf16.k_per_col, bf16.scale_dtype) == (BF16, 1, None)
    assert (w8.dtype, w8.k_per_col, w8.scale_dtype, w8.scale_block, w8.k_gran) == (torch.float8_e4m3fn, 1, torch.float32, 0, 16)
    assert (w4.dtype, w4.k_per_col, w4.scale_dtype, w4.scale_block, w4.k_gran) == (torch.uint8, 2, torch.uint8, 32, 32)
    assert infer.W8.fmt is w8 and infer.W4.fmt is w4 and infer.CODED == {"fp8": infer.W8, "fp4": infer.W4}


@pytest.mark.parametrize("family,fmt", CASES, ids=IDS)
def test_wrapper_and_declaration_exist_and_agree(calls, family, fmt):
    symbol = f"mla_{family}_{fmt.name}"
    assert callable(getattr(hip, family + fmt.suffix)) and symbol in hip.exported_symbols()
    launch(family, fmt, *operands(fmt))
    (name, args), = calls
    assert name == symbol and len(args) == len(hip._SIGNATURES[symbol]) - 1, "hip.call appends the stream"
    if fmt.scale_block:
        assert args[5] == K // fmt.scale_block, "the scale's row stride follows its pointer"
    if family == "gemm_suffix":
        assert symbol + "_pos" in hip.exported_symbols()
        del calls[:]
        launch(family, fmt, *operands(fmt), rope=(torch.zeros((8, 64)), torch.zeros((8, 64)), N), rope_pos=torch.zeros(1, dtype=torch.int32),
               rope_rows=8)
        (name, args), = calls
        assert name == symbol + "_pos" and len(args) == len(hip._SIGNATURES[name]) - 1


@pytest.mark.parametrize("family,fmt", CASES, ids=IDS)
def test_operands_of_another_dtype_are_refused(calls, family, fmt):
    x, W, scale = operands(fmt)
    with pytest.raises(TypeError, match=" x"):
        launch(family, fmt, x.float(), W, scale)
    with pytest.raises(TypeError, match=" W"):
        launch(family, fmt, x, W.to(torch.float16), scale)
    for other in hip.WEIGHT_FORMATS.values():
        if other.dtype != fmt.dtype:
            with pytest.raises(TypeError, match=" W"):
                launch(family, fmt, x, operands(other)[1], scale)
    if scale is not None:
        with pytest.raises(TypeError, match=" w_scale"):
            launch(family, fmt, x, W, scale.to(torch.float64))
    assert calls == []


@pytest.mark.parametrize("family,fmt", [c for c in CASES if c[1].scale_dtype is not None], ids=[i for i in IDS if not i.endswith("bf16")])
def test_a_scale_of_another_shape_is_refused(calls, family, fmt):
    x, W, scale = operands(fmt)
    wrong = [torch.zeros(N + 1, dtype=fmt.scale_dtype)]
    if fmt.scale_block:
        wrong += [torch.zeros((N, K // fmt.scale_block + 1), dtype=fmt.scale_dtype), torch.zeros((N + 1, K // fmt.scale_block), dtype=fmt.scale_dtype),
                  torch.zeros((N, 2 * K // fmt.scale_block), dtype=fmt.scale_dtype)[:, ::2]]
    for s in wrong:
        with pytest.raises(AssertionError):
            launch(family, fmt, x, W, s)
    assert calls == []


@pytest.mark.parametrize("family,fmt", [c for c in CASES if c[1].scale_block], ids=[i for i in IDS if i.endswith("w4")])
def test_a_block_scaled_k_off_the_granularity_is_refused(calls, family, fmt):
    bad = K + fmt.k_gran // 2
    with pytest.raises(AssertionError):
        launch(family, fmt, *operands(fmt, bad))
    assert calls == []


def test_a_k_that_differs_from_the_inputs_is_refused(calls):
    for family, fmt in CASES:
        x, W, scale = operands(fmt)
        with pytest.raises(AssertionError):
            launch(family, fmt, torch.zeros((M, 2 * K), dtype=BF16), W, scale)
    assert calls == []
