"""GPU: FP8 suffix weights for N-sample action drawing on one cached prefix -- mla_gemm_suffix_w8 (the e4m3fn form of mla_gemm_suffix_bf16:
1 <= M <= 256 rows, ragged / "groups" slot addressing, residual or q|k rotary epilogue) and suffix_weights= of SampleGroupsEps /
MLA.predict_action_diff_samples.

The kernel's parity statement is an identity: every 64-row slice is bit for bit what mla_gemm_skinny_w8 (plain input) writes for it, in every
launch form. Bounds: 4e-3 Frobenius-relative against the fp64 product over the dequantised weights is the project's bound for one bf16
rounding of fp32 sums (the existing `_w8` kernels measure 1.6-2.0e-3); 3e-2 relative L2 per chunk is the bound for "same function, other
rounding". Weights come from hip.quant_fp8_rows and are checked against quant_ref, the CPU statement of tests/test_infer_fp8_gpu.py."""
import numpy as np
import pytest
import torch

from conftest import fro_rel
from oracle import recipe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
SENT = 777.0                                                                 # bf16-exact
MS = [1, 17, 33, 49, 64, 65, 96, 97, 128, 129, 255, 256]                     # every launch form (NT, MB) and a partial last x block


def _rand(shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tables(S, dev, D=128):
    fr = torch.outer(torch.arange(S).float(), 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))
    return fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)


def quant_ref(W):
    """The CPU statement of the format: W bf16 [N, K] -> (codes float8_e4m3fn, scales fp32)."""
    f = W.float()
    amax = f.abs().amax(dim=1)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    return (f / s[:, None]).clamp(-448, 448).to(F8), s


_WEIGHTS = {}


def _quantised(N, K, dev):
    """(codes, scales, fp64 dequantised W) of one deterministic [N, K] matrix: quantised on the device once per shape, compared with
    quant_ref, shared by every test and left unchanged."""
    if (N, K) not in _WEIGHTS:
        from mla_amd import hip
        W = _rand((N, K), N + K, 0.05).to(BF)
        q, s = hip.quant_fp8_rows(W.to(dev))
        q_ref, s_ref = quant_ref(W)
        assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32)) and torch.equal(q.cpu().float(), q_ref.float())
        _WEIGHTS[(N, K)] = (q, s, q.float().double() * s.double()[:, None])
    return _WEIGHTS[(N, K)]


def _x(M, K, seed, dev, scale=0.5):
    """M rows inside a larger buffer whose rows >= M are NaN: a load beyond the rows of the call shows in the output."""
    buf = torch.full((M + 16, K), float("nan"), dtype=BF, device=dev)
    buf[:M] = _rand((M, K), seed, scale).to(BF).to(dev)
    return buf[:M]


def _plain(x, q, s, res=None):
    from mla_amd import hip
    M, N = x.shape[0], q.shape[0]
    out = torch.full((M, N), float("nan"), dtype=BF, device=x.device)
    hip.gemm_suffix_w8(x, q, s, out, N, 0, M, res)
    return out


# ------------------------------------------------------------------------------------------------ decode pins the format
@pytest.mark.parametrize("M", [2, 70])
def test_decode_of_every_code_is_ocp_e4m3fn(dev, M):
    """Row n of W is filled with byte code n (the two NaN codes replaced by 0); one-hot x rows pick single products, all exactly
    representable: the output is scale * coeff * value(code). M = 70 is the two-tile form (NT = 2)."""
    codes = torch.arange(256, dtype=torch.uint8)
    codes[0x7F] = 0
    codes[0xFF] = 0
    W = codes[:, None].repeat(1, 64).contiguous().to(dev).view(F8)
    coeff = torch.tensor([1.0, 0.5, -2.0, 0.25])[torch.arange(M) % 4]
    x = torch.zeros(M, 64)
    x[torch.arange(M), (torch.arange(M) * 7 + 3) % 64] = coeff
    val = codes.view(F8).float()
    for sc in (1.0, 0.125):
        out = _plain(x.to(BF).to(dev), W, torch.full((256,), sc, device=dev))
        assert torch.equal(out.float().cpu(), sc * coeff[:, None] * val[None, :]), (M, sc)


# ------------------------------------------------------------------------------------------------ projection vs fp64
def _parity_case(dev, M, N, K):
    q, s, Wd = _quantised(N, K, dev)
    x = _x(M, K, M * 1000 + N, dev)
    r = _rand((M, N), M + N, 1.0).to(BF).to(dev) if M % 2 == 1 else None     # residual on odd M
    want = x.double() @ Wd.t() + (r.double() if r is not None else 0)
    a, b = _plain(x, q, s, r), _plain(x, q, s, r)
    assert torch.isfinite(a.float()).all()
    e = fro_rel(a, want)
    print(f"mla_gemm_suffix_w8 M {M} N {N} K {K} res {r is not None}: fro_rel vs fp64 {e:.3e}")
    assert e < 4e-3                                                           # one bf16 rounding of the fp32 sums
    assert torch.equal(a, b)


@pytest.mark.parametrize("N,K", [(96, 48), (520, 4112)])
@pytest.mark.parametrize("M", MS)
def test_gemm_suffix_w8_matches_fp64_reference(dev, M, N, K):
    """K = 48 is below one 64-wide K step, 4112 ends inside one; N = 520 is 32.5 tiles: the last two-tile workgroup has a tile beyond N."""
    _parity_case(dev, M, N, K)


@pytest.mark.parametrize("M", [85, 256])
def test_gemm_suffix_w8_matches_fp64_reference_at_the_7b_down_projection(dev, M):
    _parity_case(dev, M, 1000, 11008)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("M", MS)
def test_every_64_row_slice_is_the_skinny_w8_kernel_bit_for_bit(dev, M, res):
    from mla_amd import hip
    N, K = 520, 4112
    q, s, _ = _quantised(N, K, dev)
    x = _x(M, K, M * 1000 + N, dev)
    r = _rand((M, N), M + N, 1.0).to(BF).to(dev) if res else None
    got = _plain(x, q, s, r)
    for m0 in range(0, M, 64):
        m1 = min(m0 + 64, M)
        want = torch.full((m1 - m0, N), float("nan"), dtype=BF, device=dev)
        hip.gemm_skinny_w8(x[m0:m1], q, s, want, N, 0, m1 - m0, None if r is None else r[m0:m1])
        assert torch.isfinite(want.float()).all() and torch.equal(got[m0:m1], want), (M, m0)


def test_scale_multiplies_the_finished_sum(dev):
    """Doubling every scale doubles every output bit for bit (outputs of order 1: far from the ends of the bf16 range); a zero scale
    gives an exactly zero column."""
    M, N, K = 85, 80, 256
    q, _, _ = _quantised(N, K, dev)
    s = (0.5 + torch.rand(N, generator=torch.Generator().manual_seed(4))).to(dev) / 448
    s[5] = 0.0
    x = _x(M, K, 21, dev)
    a, b = _plain(x, q, s), _plain(x, q, 2 * s)
    assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0
    assert torch.equal(b.float(), 2 * a.float())
    assert float(a[:, 5].float().abs().max()) == 0 and float(b[:, 5].float().abs().max()) == 0


# ------------------------------------------------------------------------------------------------ ragged slots, rotation, groups
def test_ragged_slots_equal_plain_projection_plus_rope(dev):
    """Unequal slot[b]: the fused output == the dense projection written at each sample's slot, then rope_inplace at positions slot[b] + p,
    bit for bit (the scales differ per W row, so the rotation partner's scale is pinned too); v columns unrotated; everything else keeps
    the sentinel. With a slot raised so that its last rows reach cap_rows, those rows are not written."""
    from mla_amd import hip
    B, R, nh, K, cap = 3, 17, 2, 512, 46
    H = nh * 128
    M, ld = B * R, 3 * H + 64
    slots = [11, 29, 20]
    q, s, _ = _quantised(3 * H, K, dev)
    n = torch.arange(2 * H)
    assert float((s.cpu()[n] != s.cpu()[n ^ 64]).float().mean()) > 0.5         # a rotary row's scale is not its partner's (d <-> d + 64)
    x = _x(M, K, 7, dev, 1.1)
    cos, sin = _tables(cap, dev)
    dense = _plain(x, q, s)
    assert torch.isfinite(dense.float()).all()

    def run(sl):
        got = torch.full((B, cap + 4, ld), SENT, dtype=BF, device=dev)       # 4 guard rows per sample behind cap_rows
        hip.gemm_suffix_w8(x, q, s, got, ld, got.stride(0), R, rope=(cos, sin, 2 * H),
                           slot=torch.tensor(sl, dtype=torch.int32, device=dev), cap_rows=cap)
        return got

    def want(sl):
        ref = torch.full((B, cap + 4, ld), SENT, dtype=BF, device=dev)
        for b, s0 in enumerate(sl):
            n = min(R, cap - s0)                                              # rows that fit [0, cap_rows)
            ref[b, s0:s0 + n, :3 * H] = dense[b * R:b * R + n]
            hip.rope_inplace(ref[b, s0:s0 + n], cos[s0:s0 + n].contiguous(), sin[s0:s0 + n].contiguous(), n, nh, 128, 0, H)
        return ref
    got, ref = run(slots), want(slots)
    assert torch.equal(got, ref)
    for b, s0 in enumerate(slots):
        assert torch.equal(got[b, s0:s0 + R, 2 * H:3 * H], dense[b * R:(b + 1) * R, 2 * H:])           # v: unrotated
        assert not torch.equal(got[b, s0:s0 + R, :2 * H], dense[b * R:(b + 1) * R, :2 * H])
        assert bool((got[b, :s0] == SENT).all()) and bool((got[b, s0 + R:] == SENT).all()) and bool((got[b, :, 3 * H:] == SENT).all())
    raised = [11, 32, 20]                                                     # sample 1: rows 32 .. 45 fit, 46, 47, 48 do not
    got = run(raised)
    assert torch.equal(got, want(raised))
    assert bool((got[1, cap:] == SENT).all()) and not bool((got[1, 32:cap, :3 * H] == SENT).any())


@pytest.mark.parametrize("G,R", [(3, 17), (15, 17)])
def test_group_rows_land_behind_one_prefix(dev, G, R):
    """The "groups" form SampleGroupsEps uses (out_batch_stride = R ld, every slot S_p, cap_rows = S_p + R): row p of group g lands at
    S_p + g R + p, rotated at position S_p + p; prefix rows and pad columns keep the sentinel. (15, 17) is 255 rows."""
    from mla_amd import hip
    nh, K, S_p, PAD = 2, 512, 29, 64
    H = nh * 128
    M, ld = G * R, 3 * H + PAD
    q, s, _ = _quantised(3 * H, K, dev)
    x = _x(M, K, G * 100 + R, dev, 1.1)
    cos, sin = _tables(S_p + R, dev)
    slot = torch.full((G,), S_p, dtype=torch.int32, device=dev)
    got = torch.full((S_p + M + 3, ld), SENT, dtype=BF, device=dev)
    hip.gemm_suffix_w8(x, q, s, got, ld, R * ld, R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=S_p + R)
    dense = _plain(x, q, s)
    ref = dense.clone()
    for g in range(G):
        hip.rope_inplace(ref[g * R:(g + 1) * R], cos[S_p:].contiguous(), sin[S_p:].contiguous(), R, nh, 128, 0, H)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got[S_p:S_p + M, :3 * H], ref)
    assert not torch.equal(ref[:, :2 * H], dense[:, :2 * H]) and torch.equal(ref[:, 2 * H:], dense[:, 2 * H:])
    assert bool((got[:S_p] == SENT).all()) and bool((got[S_p + M:] == SENT).all()) and bool((got[:, 3 * H:] == SENT).all())


def test_gemm_suffix_w8_graph_replay(dev):
    """Captured once, replayed after x was rewritten: the eager launch on the new x, bit for bit."""
    from mla_amd import hip
    M, N, K = 85, 520, 4112
    q, s, _ = _quantised(N, K, dev)
    x = _rand((M, K), 5, 0.5).to(BF).to(dev)
    first = _plain(x, q, s)                                                  # also the warm-up outside the capture
    out = torch.empty((M, N), dtype=BF, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.gemm_suffix_w8(x, q, s, out, N, 0, M)
    x.copy_(_rand((M, K), 6, 0.5).to(BF))
    eager = _plain(x, q, s)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and not torch.equal(eager, first)


# ------------------------------------------------------------------------------------------------ end to end, tiny model
N = 5


def infer_inputs(T, tag):
    """The recipe of tests/test_infer_samples_gpu.py; the N initial samples come from their own generator."""
    g = recipe._gen(tag)
    ids = torch.randint(3, 29000, (1, 20), generator=g)
    ids[0, 0] = 1
    ids = torch.cat([ids, torch.tensor([[29871]])], dim=1)
    image = torch.cat([torch.randn(1, 3, 672, 672, generator=g), torch.ones(1, 1, 672, 672)], dim=1)
    lo, hi = torch.tensor([0.0, -0.4, 0.75]), torch.tensor([0.6, 0.4, 1.25])
    pc = lo + (hi - lo) * torch.rand(1, 1024, 3, generator=g)
    proprio = torch.rand(1, 1, 7, generator=g) * 2 - 1
    starts = [torch.randint(0, 1024, (1,), generator=g), torch.randint(0, 512, (1,), generator=g)]
    noise = torch.randn(N, T, 7, generator=recipe._gen(tag + "_samples"))
    return ids, image, pc, proprio, noise, starts


@pytest.fixture(scope="module", params=[3, 15], ids=["window3", "window15"])
def tiny(request, dev):
    """hidden 256, 9 layers, 2 heads of 128; window 3: R = 5 suffix rows per sample, window 15: R = 17. The one-pass "fp8" result of the
    N initial samples is computed once and shared."""
    from mla_amd.backbones import LLaMa2LLMBackbone
    from mla_amd.llama import LlamaConfig
    from mla_amd.mla import MLA
    from mla_amd.prismatic import PrismaticVLM
    window = request.param
    bb = LLaMa2LLMBackbone(config=LlamaConfig(**(recipe.TINY_LLAMA | {"vocab_size": 32000})))
    vlm = PrismaticVLM("tiny", bb, token_size=recipe.TOKEN_SIZE, use_diff=True, use_pointcloud=True, use_contrastive=True,
                       use_generation=False, future_action_window_size=window)
    m = MLA(vlm, None, token_size=recipe.TOKEN_SIZE, future_action_window_size=window, use_diff=True, use_pointcloud=True,
            use_contrastive=True)
    m.load_state_dict({k: recipe.det_weight(k, v.shape) for k, v in m.state_dict().items()}, strict=True)
    m.eval().to(dev)
    for p in m.parameters():
        p.data = p.data.to(BF)
    inputs = infer_inputs(window + 1, f"infer_samples{window + 1}")
    m.vlm.vision_tower_3d.fps_starts_override = inputs[5]
    ids, image, pc, proprio, noise, _ = inputs
    kw = dict(image=image[0], pointcloud=pc[0].numpy(), cur_robot_state=proprio[0, 0].numpy(), input_ids=ids, num_ddim_steps=8)
    default = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)             # bf16, before any fp8 call on this model
    fp8 = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8", **kw)
    default.setflags(write=False)
    fp8.setflags(write=False)
    return m, window, inputs, kw, default, fp8


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _count_prefill_layers(monkeypatch):
    from mla_amd import ops
    calls = []
    orig = ops.DecoderLayerFn._fwd

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(ops.DecoderLayerFn, "_fwd", staticmethod(counted))
    return calls


def test_fp8_samples_are_the_fp8_batch_one_calls(dev, tiny):
    """Sample n within 3e-2 of its own predict_action_diff(suffix_weights="fp8") call and of "fp8_as_bf16" through the same call; "bf16"
    is the default call bit for bit before and after fp8 calls (engines and graphs are per mode); "fp8" is not "bf16"."""
    m, window, (_, _, _, _, noise, _), kw, default, fp8 = tiny
    T = window + 1
    assert fp8.shape == (N, T, 7) and np.isfinite(fp8).all()
    singles = np.stack([m.predict_action_diff(suffix_weights="fp8", noise=noise[n:n + 1], **kw) for n in range(N)])
    ref = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8_as_bf16", **kw)
    d1 = [_rel(fp8[n], singles[n]) for n in range(N)]
    d2 = [_rel(fp8[n], ref[n]) for n in range(N)]
    print(f"window {window}: fp8 samples vs batch-1 fp8 calls {['%.2e' % d for d in d1]}, vs fp8_as_bf16 {['%.2e' % d for d in d2]}; "
          f"bit-identical to the batch-1 fp8 calls: {np.array_equal(fp8, singles)}; NOT gated: fp8 vs bf16 {_rel(fp8, default):.3e}")
    assert max(d1) < 3e-2 and max(d2) < 3e-2
    assert np.array_equal(m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="bf16", **kw), default)
    assert np.array_equal(m.predict_action_diff_samples(num_samples=N, noise=noise, **kw), default)
    assert not np.array_equal(fp8, default) and not np.array_equal(fp8[0], fp8[1])
    engines = m.vlm.__dict__["_prefix_engines_samples"]
    by_mode = {e.suffix_weights: e for key, e in engines.items() if key[2] == N}
    assert set(by_mode) == {"bf16", "fp8", "fp8_as_bf16"} and len({id(e) for e in by_mode.values()}) == 3
    for e in by_mode.values():
        assert e.graph is not None and e.graph_error is None, (e.suffix_weights, e.graph_error)
    assert len({id(e.graph) for e in by_mode.values()}) == 3


def test_fp8_graph_replay_is_the_eager_launches(dev, tiny, monkeypatch):
    from mla_amd import infer
    m, _, (_, _, _, _, noise, _), kw, _, fp8 = tiny
    monkeypatch.setattr(infer, "_USE_GRAPH", False)
    assert np.array_equal(m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8", **kw), fp8)


def test_fp8_call_has_one_prefill_and_sub_batches_keep_the_bits(dev, tiny, monkeypatch):
    """n_layers decoder-layer forwards per fp8 call; with MAX_ROWS = 2 R the passes are 2 + 2 + 1 groups on the same prefill and -- every
    output row depends on its own rows only, in every launch form -- the result is the one-pass result bit for bit."""
    from mla_amd import infer
    m, window, (_, _, _, _, noise, _), kw, _, fp8 = tiny
    n_layers = len(m.vlm.llm_backbone.llm.model.layers)
    calls = _count_prefill_layers(monkeypatch)
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8", **kw)
    assert len(calls) == n_layers and np.array_equal(got, fp8)
    R = window + 2
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_ROWS", 2 * R)
    assert infer.plan_sample_groups(N, R, 2 * R) == [(0, 2), (2, 4), (4, 5)]
    del calls[:]
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8", **kw)
    assert len(calls) == n_layers, len(calls)
    assert np.array_equal(got, fp8)
    eng = [e for key, e in m.vlm.__dict__["_prefix_engines_samples"].items() if key[2] == 2]
    assert len(eng) == 1 and eng[0].suffix_weights == "fp8" and sorted(eng[0]._graphs) == [1, 2]


def test_one_fp8_sample_is_predict_action_diff(dev, tiny):
    m, window, (_, _, _, _, noise, _), kw, _, _ = tiny
    one = m.predict_action_diff_samples(num_samples=1, noise=noise[2:3], suffix_weights="fp8", **kw)
    assert one.shape == (1, window + 1, 7)
    assert np.array_equal(one[0], m.predict_action_diff(suffix_weights="fp8", noise=noise[2:3], **kw))


def test_fp8_samples_follow_the_weights(dev, tiny):
    """An in-place update of one decoder weight (mul_ bumps _version) changes the next fp8 result; restoring it restores the bits."""
    m, _, (_, _, _, _, noise, _), kw, _, fp8 = tiny
    w = m.vlm.llm_backbone.llm.model.layers[4].mlp.down_proj.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    changed = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8", **kw)
    with torch.no_grad():
        w.copy_(saved)
    restored = m.predict_action_diff_samples(num_samples=N, noise=noise, suffix_weights="fp8", **kw)
    assert not np.array_equal(changed, fp8) and np.array_equal(restored, fp8)


def test_fp8_refusals_raise(dev, tiny, monkeypatch, recwarn):
    """No silent bf16 fallback and no warned loop of batch-1 calls: fp8 without the cached prefix, or at a shape the shared-prefix engine
    refuses, raises; predict_action_diff_batch with B = 2 still names the batched engine."""
    from mla_amd import infer
    m, _, (ids, image, pc, proprio, noise, _), kw, _, _ = tiny
    with pytest.raises(ValueError, match="suffix_weights"):
        m.predict_action_diff_samples(num_samples=2, noise=noise[:2], suffix_weights="fp8", reuse_prefix=False, **kw)
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_R", 2)
    with pytest.raises(ValueError, match="suffix_weights"):
        m.predict_action_diff_samples(num_samples=2, noise=noise[:2], suffix_weights="fp8", **kw)
    assert not [w for w in recwarn.list if issubclass(w.category, RuntimeWarning) and "SampleGroupsEps" in str(w.message)]
    monkeypatch.undo()
    bkw = dict(cur_robot_states=[proprio[0, 0].numpy()] * 2, input_ids=[ids, ids], noise=noise[:2], num_ddim_steps=8)
    with pytest.raises(NotImplementedError, match="BatchedPrefixCachedEps"):
        m.predict_action_diff_batch([image[0]] * 2, [pc[0].numpy()] * 2, suffix_weights="fp8", **bkw)
