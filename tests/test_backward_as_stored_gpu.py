"""DecoderLayerFn's backward with every GEMM operand read as stored (MLA_DGRAD_RM, MLA_WGRAD_RM = 1, kept normalised inputs at save
level 1) against the copying path (both switches 0). Reading an operand reduction-major keeps the K order, so every comparison is
torch.equal: dh, the nine weight gradients (bf16 .grad route and the fp32 main_grad + sum(dW^2) partials route, norm included, with an
accumulating second micro-batch). One layer at H = 256, I = 512, 2 heads of 128, B = 2, S = 136 (272 rows, padded to 320 inside:
two row tiles with a partial one), ragged sequence lengths (136, 100), RoPE on; the weights lie in one flat buffer (q|k|v and gate|up
back to back) as the sharded model keeps them."""
import pytest
import torch

BF = torch.bfloat16
NAMES = ["ln1", "wq", "wk", "wv", "wo", "ln2", "wg", "wu", "wd"]
H, I, NH, B, S = 256, 512, 2, 2, 136
LENS = (136, 100)
DGRAD = ("dqkv", "do", "dgu", "dd")
WGRAD = ("wd", "wgu", "wo", "wqkv")


def _shapes():
    return [(H,), (H, H), (H, H), (H, H), (H, H), (H,), (I, H), (I, H), (H, I)]


@pytest.fixture(scope="module")
def inputs():
    """Weights, two micro-batches of activations / output gradients and the RoPE tables (host tensors, made once)."""
    g = torch.Generator().manual_seed(1234)
    p = {n: ((1.0 + 0.1 * torch.randn(s, generator=g)) if len(s) == 1 else 0.05 * torch.randn(s, generator=g)).to(BF)
         for n, s in zip(NAMES, _shapes())}
    xs = [torch.randn(B, S, H, generator=g).to(BF) for _ in range(2)]
    dys = [torch.randn(B, S, H, generator=g).to(BF) for _ in range(2)]
    D = H // NH
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.outer(torch.arange(S).float(), inv)            # half tables [S, D / 2], fp32, as the layer takes them
    return p, xs, dys, ang.cos().contiguous(), ang.sin().contiguous()


def _packed(p, dev):
    offs, n = {}, 0
    for name in NAMES:
        offs[name] = n
        n += p[name].numel()
    flat = torch.empty(n, dtype=BF, device=dev)
    for name in NAMES:
        flat[offs[name]:offs[name] + p[name].numel()] = p[name].to(dev).reshape(-1)
    flat.requires_grad_(True)
    return [flat[offs[name]:offs[name] + p[name].numel()].view(p[name].shape) for name in NAMES], flat


class _Switches:
    def __init__(self, dgrad, wgrad):
        self.dgrad, self.wgrad = dgrad, wgrad

    def __enter__(self):
        from mla_amd import ops
        self.prev = (ops.set_dgrad_rm(self.dgrad), ops.set_wgrad_rm(self.wgrad))

    def __exit__(self, *a):
        from mla_amd import ops
        ops.set_dgrad_rm(self.prev[0])
        ops.set_wgrad_rm(self.prev[1])


def _run(dev, inputs, level, dgrad, wgrad, lens=LENS, seq=S, count=None):
    """One forward + backward on the packed weights: (out, dh, flat bf16 gradient of the nine weights)."""
    from mla_amd import hip, ops
    p, xs, dys, cos, sin = inputs
    real = {n: getattr(hip, n) for n in ("transpose", "rmsnorm_apply", "rmsnorm_apply_t")}
    with _Switches(dgrad, wgrad):
        w, flat = _packed(p, dev)
        x = xs[0][:, :seq].contiguous().to(dev).requires_grad_(True)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        out = ops.decoder_layer(x, sl, cos[:seq].to(dev), sin[:seq].to(dev), NH, 1e-5, level, w)
        try:
            if count is not None:
                for n, f in real.items():
                    setattr(hip, n, lambda *a, _n=n, _f=f, **k: (count.append(_n), _f(*a, **k))[1])
            out.backward(dys[0][:, :seq].contiguous().to(dev))
        finally:
            for n, f in real.items():
                setattr(hip, n, f)
    return out.detach(), x.grad, flat.grad


@pytest.fixture(scope="module")
def copying(dev, inputs):
    """The copying path (both switches off) per save level: computed once, never written."""
    return {lvl: _run(dev, inputs, lvl, "0", "0") for lvl in (0, 1, 2)}


def _assert_same(got, ref):
    assert torch.equal(got[0], ref[0]), "layer output"
    assert torch.equal(got[1], ref[1]), "dh"
    assert torch.equal(got[2], ref[2]), float((got[2].float() - ref[2].float()).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2])
def test_all_operands_as_stored_is_the_copying_path_bit_for_bit(dev, inputs, copying, level):
    """All switches on against all off at save levels 0, 1 and 2; with all on the backward runs no tile transpose and rebuilds no
    normalised input (the copying path does: the bookkeeping is not blind)."""
    calls = []
    on = _run(dev, inputs, level, "1", "1", count=calls)
    _assert_same(on, copying[level])
    assert calls == [], calls
    calls_off = []
    _run(dev, inputs, level, "0", "0", count=calls_off)
    assert "transpose" in calls_off


@pytest.mark.gpu
@pytest.mark.parametrize("switch", [f"d:{n}" for n in DGRAD] + [f"w:{n}" for n in WGRAD])
def test_each_switch_alone(dev, inputs, copying, switch):
    kind, name = switch.split(":")
    got = _run(dev, inputs, 1, name if kind == "d" else "0", name if kind == "w" else "0")
    _assert_same(got, copying[1])


@pytest.mark.gpu
def test_token_count_not_a_multiple_of_8(dev, inputs):
    """B * S = 270 rows (S = 135: S % 4 != 0 as well, so the attention backward writes no transposed outputs): the layer pads its rows
    and runs without error, on against off bit for bit."""
    off = _run(dev, inputs, 1, "0", "0", lens=(135, 99), seq=135)
    on = _run(dev, inputs, 1, "1", "1", lens=(135, 99), seq=135)
    _assert_same(on, off)


class _Layer(torch.nn.Module):
    def __init__(self, p):
        super().__init__()
        for n in NAMES:
            setattr(self, n, torch.nn.Parameter(p[n].clone()))


def _main_grad_run(dev, inputs, dgrad, wgrad):
    """Two accumulating micro-batches into fp32 main_grad through a one-process ShardedModel (the wgrad epilogues leave the sum(dW^2)
    partials the clipping norm is summed from): (gradient buffer, norm, dh of the second micro-batch)."""
    from mla_amd import ops
    from mla_amd.fsdp import ShardedModel
    p, xs, dys, cos, sin = inputs
    layer = _Layer(p)
    sm = ShardedModel(layer, lambda m: False, dev)
    sm.begin_step()
    sl = torch.tensor(LENS, dtype=torch.int32, device=dev)
    with _Switches(dgrad, wgrad):
        for i in range(2):
            x = xs[i].to(dev).requires_grad_(True)
            out = ops.decoder_layer(x, sl, cos.to(dev), sin.to(dev), NH, 1e-5, 1, [getattr(layer, n) for n in NAMES])
            out.backward(dys[i].to(dev))
            if i == 0:
                sm.finish_micro_backward()
        sm.finish_backward()
        norm = sm.grad_norm_and_clip(None).clone()
    assert any(u.sq_entries for u in sm.units), "the wgrad epilogues left no sum-of-squares partials: the route under test did not run"
    return torch.cat([u.grad32 for u in sm.units if u.trainable]).clone(), norm, x.grad


@pytest.mark.gpu
def test_main_grad_route_with_a_second_micro_batch(dev, inputs):
    off = _main_grad_run(dev, inputs, "0", "0")
    on = _main_grad_run(dev, inputs, "1", "1")
    assert torch.equal(on[0], off[0]), float((on[0] - off[0]).abs().max())
    assert torch.equal(on[1], off[1]), (float(on[1]), float(off[1]))
    assert torch.equal(on[2], off[2])


def test_dgrad_rm_parser_and_setter():
    from mla_amd import ops
    assert ops._parse_dgrad_rm("0") == dict.fromkeys(DGRAD, 0)
    assert ops._parse_dgrad_rm(" 1 ") == dict.fromkeys(DGRAD, 1)
    assert ops._parse_dgrad_rm("dqkv, dd=1,do=0") == {"dqkv": 1, "do": 0, "dgu": 0, "dd": 1}
    assert ops._parse_dgrad_rm("") == dict.fromkeys(DGRAD, 0)
    for bad in ("dx", "dd=2", "dd=a", "wqkv=1", "dqkv;dd"):
        with pytest.raises(ValueError, match="MLA_DGRAD_RM"):
            ops._parse_dgrad_rm(bad)
    cur = dict(ops._DGRAD_RM)
    prev = ops.set_dgrad_rm("dgu")
    try:
        assert prev == cur and ops._DGRAD_RM == {"dqkv": 0, "do": 0, "dgu": 1, "dd": 0}
        assert ops.set_dgrad_rm(prev) == {"dqkv": 0, "do": 0, "dgu": 1, "dd": 0}
        assert ops._DGRAD_RM == cur
    finally:
        ops.set_dgrad_rm(cur)
