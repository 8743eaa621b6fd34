"""GPU: N action chunks for ONE observation on one cached prefix -- mla_attn_chunk_groups (G groups of R suffix rows that see the shared
prefix and, causally, their own rows), mla_gemm_suffix_bf16 addressing the groups' rows, mla_amd/infer.py:SampleGroupsEps and
MLA.predict_action_diff_samples.

The kernel's parity statement is an identity: group g's output rows are bit for bit what mla_attn_chunk (B = 1, S_kv = S_p + R) writes on
cat(cache[:S_p], cache[S_p + g R : S_p + (g + 1) R]). 5e-3 Frobenius-relative against fp32 is test_attn_chunk_matches_fp32_reference's
bound; 3e-2 relative L2 per chunk is the project's bound for "same function, other rounding" (the batched path measured 2.7e-3 .. 8.2e-3)."""
import math

import numpy as np
import pytest
import torch

import infer_samples_cases as isc
from conftest import fro_rel
from oracle import recipe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 1 / math.sqrt(128)


def _rand(shape, seed, scale, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(BF)


def _tables(S, dev, D=128):
    fr = torch.outer(torch.arange(S).float(), 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))
    return fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)


def _cache(dev, G, R, S_p, H, extra_rows=2):
    return _rand((S_p + G * R + extra_rows, 3 * H * 128), S_p * 100 + R * 7 + G + H, 0.7, dev)


def _per_group_chunk(cache, G, H, S_p, R):
    from mla_amd import hip
    return torch.cat([hip.attn_chunk(isc.gather_group(cache, g, R, S_p)[None].contiguous(), 1, H, 128, S_p + R, R, SCALE) for g in range(G)])


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("G,R,S_p,H", [c + (2,) for c in isc.KERNEL_CASES] + [isc.H3_CASE + (3,)])
def test_attn_chunk_groups_is_attn_chunk_per_group_bit_for_bit(dev, G, R, S_p, H):
    from mla_amd import hip
    cache = _cache(dev, G, R, S_p, H)
    o = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)
    assert o.shape == (G * R, H * 128) and torch.isfinite(o.float()).all()
    want = _per_group_chunk(cache, G, H, S_p, R)
    for g in range(G):
        assert torch.equal(o[g * R:(g + 1) * R], want[g * R:(g + 1) * R]), f"group {g}"
    e = fro_rel(o, isc.attn_ref(cache, G, H, S_p, R))
    print(f"mla_attn_chunk_groups G {G} R {R} S_p {S_p} H {H}: fro_rel vs fp32 {e:.3e}")
    assert e < 5e-3
    assert torch.equal(o, hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE))
    assert torch.equal(o, hip.attn_chunk_groups(cache[None], G, H, 128, S_p, R, SCALE))       # [1, rows, 3H] form
    for gw in (1, 2, 4):                                                     # every launch form: the bits depend on neither the sharing
        for order in (0, 1):                                                 # nor the work order (grids of 8 k blocks and others)
            got = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE, gw=gw, order=order)
            assert torch.equal(o, got), f"gw {gw} order {order}"
    if S_p == 0:                                                             # no prefix: G independent samples of R rows
        view = cache[:G * R].view(G, R, 3 * H * 128)
        assert torch.equal(o, hip.attn_chunk(view, G, H, 128, R, R, SCALE))


@pytest.mark.parametrize("G,R,S_p", isc.ISOLATION_CASES)
def test_attn_chunk_groups_never_reads_another_groups_rows(dev, G, R, S_p):
    """Every row of all groups but g set to NaN (q, k and v parts): group g's output is bit-unchanged and finite -- masked-key and
    padding loads stay inside the query's own key set."""
    from mla_amd import hip
    H = 2
    cache = _cache(dev, G, R, S_p, H, extra_rows=0)
    clean = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)
    for gw in (None, 1, 2, 4):
        for g in range(G):
            hostile = torch.full_like(cache, float("nan"))
            hostile[:S_p] = cache[:S_p]
            hostile[S_p + g * R:S_p + (g + 1) * R] = cache[S_p + g * R:S_p + (g + 1) * R]
            o = hip.attn_chunk_groups(hostile, G, H, 128, S_p, R, SCALE, gw=gw)
            mine = o[g * R:(g + 1) * R]
            assert torch.isfinite(mine.float()).all() and torch.equal(mine, clean[g * R:(g + 1) * R]), (gw, g)


def test_attn_chunk_groups_graph_replay(dev):
    """Captured once, replayed after the prefix rows were rewritten: the eager launch on the new rows, bit for bit."""
    from mla_amd import hip
    G, R, S_p, H = 3, 17, 130, 2
    cache = _cache(dev, G, R, S_p, H)
    hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)                   # function attributes outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)
    first = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)
    cache[:S_p].copy_(_rand((S_p, 3 * H * 128), 99, 0.7, dev))
    eager = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)
    o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, eager) and not torch.equal(eager, first)


# ------------------------------------------------------------------------------------------------ projection addressing
@pytest.mark.parametrize("G,R,nh,K", isc.PROJECTION_CASES)
def test_gemm_suffix_writes_group_rows_behind_one_prefix(dev, G, R, nh, K):
    """mla_gemm_suffix_bf16 with the "samples" overlapping (batch stride R rows, every slot S_p, cap_rows S_p + R): row p of group g lands
    at cache row S_p + g R + p and is the plain projection rotated at position S_p + p (the comparison of
    test_gemm_suffix_ragged_slots_equal_plain_projection_plus_rope); prefix rows and the columns outside the projection keep the sentinel."""
    from mla_amd import hip
    H, S_p, PAD = nh * 128, 29, 64
    M, ld = G * R, 3 * H + PAD
    x = _rand((M, K), G * 100 + R, 1.1, dev)
    W = _rand((3 * H, K), nh + K + G, 0.06, dev)
    cos, sin = _tables(S_p + R, dev)
    slot = torch.full((G,), S_p, dtype=torch.int32, device=dev)
    SENT = 777.0                                                              # bf16-exact
    got = torch.full((S_p + M + 3, ld), SENT, dtype=BF, device=dev)
    hip.gemm_suffix(x, W, got, ld, R * ld, R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=S_p + R)
    dense = torch.full((M, 3 * H), float("nan"), dtype=BF, device=dev)
    hip.gemm_suffix(x, W, dense, 3 * H, 0, M)
    ref = dense.clone()
    for g in range(G):
        hip.rope_inplace(ref[g * R:(g + 1) * R], cos[S_p:].contiguous(), sin[S_p:].contiguous(), R, nh, 128, 0, H)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got[S_p:S_p + M, :3 * H], ref)
    assert not torch.equal(ref[:, :2 * H], dense[:, :2 * H]) and torch.equal(ref[:, 2 * H:], dense[:, 2 * H:])
    assert bool((got[:S_p] == SENT).all()) and bool((got[S_p + M:] == SENT).all()) and bool((got[:, 3 * H:] == SENT).all())


# ------------------------------------------------------------------------------------------------ end to end, tiny model
N = 5


def infer_inputs(T, tag):
    """The recipe of tests/test_infer_fp8_gpu.py; the N initial samples come from their own generator."""
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
    """hidden 256, 9 layers, 2 heads of 128; window 3: R = 5 suffix rows per sample, window 15: R = 17. The batch-1 chunks of the N
    initial samples are computed once and shared."""
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
    singles = np.stack([m.predict_action_diff(noise=noise[n:n + 1], **kw) for n in range(N)])
    singles.setflags(write=False)
    return m, window, inputs, kw, singles


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


def test_samples_are_the_batch_one_calls(dev, tiny, monkeypatch):
    """N = 5 samples on one prefix: each within 3e-2 of predict_action_diff on its initial sample and of predict_action_diff_batch on 5
    copies of the observation; ONE prefill (n_layers decoder-layer forwards) for the whole call."""
    m, window, (ids, image, pc, proprio, noise, _), kw, singles = tiny
    T = window + 1
    m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)          # engine and graph exist before the launches are counted
    calls = _count_prefill_layers(monkeypatch)
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)
    assert len(calls) == len(m.vlm.llm_backbone.llm.model.layers), len(calls)
    monkeypatch.undo()
    assert got.shape == (N, T, 7) and np.isfinite(got).all()
    tower = m.vlm.vision_tower_3d
    starts = tower.fps_starts_override
    try:                                                                     # N copies of the observation: one start index per copy
        tower.fps_starts_override = [s.repeat(N) for s in starts]
        batch = m.predict_action_diff_batch([image[0]] * N, [pc[0].numpy()] * N, cur_robot_states=[proprio[0, 0].numpy()] * N,
                                            input_ids=[ids] * N, noise=noise, num_ddim_steps=8)
    finally:
        tower.fps_starts_override = starts
    d1 = [_rel(got[n], singles[n]) for n in range(N)]
    d2 = [_rel(got[n], batch[n]) for n in range(N)]
    print(f"window {window}: samples vs batch-1 calls {['%.2e' % d for d in d1]}, vs predict_action_diff_batch {['%.2e' % d for d in d2]}")
    assert max(d1) < 3e-2 and max(d2) < 3e-2
    assert not np.array_equal(got[0], got[1]) and _rel(got[0], got[1]) > 1e-3
    engines = m.vlm.__dict__["_prefix_engines_samples"]
    assert len(engines) == 1 and all(e.graph is not None and e.graph_error is None for e in engines.values())


def test_one_sample_is_predict_action_diff(dev, tiny):
    m, window, (_, _, _, _, noise, _), kw, singles = tiny
    one = m.predict_action_diff_samples(num_samples=1, noise=noise[2:3], **kw)
    assert one.shape == (1, window + 1, 7) and np.array_equal(one[0], singles[2])


def test_sub_batches_share_one_prefill(dev, tiny, monkeypatch):
    """MAX_ROWS = 2 R (34 at window 15): passes of 2 + 2 + 1 groups on one cache; still n_layers prefill calls, every sample within the bound."""
    from mla_amd import infer
    m, window, (_, _, _, _, noise, _), kw, singles = tiny
    R = window + 2
    monkeypatch.setattr(infer.SampleGroupsEps, "MAX_ROWS", 2 * R)             # 34 at window 15
    assert infer.plan_sample_groups(N, R, 2 * R) == [(0, 2), (2, 4), (4, 5)]
    calls = _count_prefill_layers(monkeypatch)
    got = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)
    assert len(calls) == len(m.vlm.llm_backbone.llm.model.layers), len(calls)
    d = [_rel(got[n], singles[n]) for n in range(N)]
    print(f"window {window}: sub-batched samples vs batch-1 calls {['%.2e' % x for x in d]}")
    assert got.shape == (N, window + 1, 7) and max(d) < 3e-2
    eng = [e for key, e in m.vlm.__dict__["_prefix_engines_samples"].items() if key[2] == 2]
    assert len(eng) == 1 and sorted(eng[0]._graphs) == [1, 2] and eng[0].cache[0].shape[0] == eng[0].S_p + 2 * R


def test_engine_and_graph_are_reused_for_a_new_observation(dev, tiny):
    m, window, (_, image, _, _, noise, _), kw, _ = tiny
    first = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)
    engines = m.vlm.__dict__["_prefix_engines_samples"]
    (key, eng), = [(k, e) for k, e in engines.items() if k[2] == N]
    gid = id(eng.graph)
    assert eng.graph is not None and eng.graph_error is None
    other = dict(kw, image=torch.cat([image[0, :3] * 0.5 + 0.1, image[0, 3:]]))
    second = m.predict_action_diff_samples(num_samples=N, noise=noise, **other)
    assert engines[key] is eng and id(eng.graph) == gid and eng.graph is not None and eng.graph_error is None
    assert not np.array_equal(first, second)
    assert np.array_equal(m.predict_action_diff_samples(num_samples=N, noise=noise, **kw), first)


def test_epsilon_graph_replay_is_the_eager_launches(dev, tiny):
    from mla_amd import infer
    m, window, (ids, image, pc, proprio, noise, _), _, _ = tiny
    T = window + 1
    kw = dict(images=image.to(dev), point_cloud=pc.to(dev), proprio=proprio.to(dev), camera_name="rlbench_front")
    t = torch.full((N,), 91, device=dev)
    with torch.inference_mode():
        eng, passes = infer.SampleGroupsEps.for_inputs(m.vlm, ids.to(dev), T, N, **kw)
        assert passes == [(0, N)] and eng.R == T + 1
        eng.set_groups(N)
        _, eps = eng(noise.to(dev), t)
        assert eng.graph is not None, f"the suffix pass was not captured into a graph: {eng.graph_error}"
        _, eps2 = eng(noise.to(dev), t)                                      # replay
        old = infer._USE_GRAPH
        try:
            infer._USE_GRAPH = False
            _, eps_e = eng(noise.to(dev), t)                                 # eager launches on the same cache
        finally:
            infer._USE_GRAPH = old
        one = infer.PrefixCachedEps.for_inputs(m.vlm, n_action_rows=T, input_ids=ids.to(dev), **kw)
        _, eps_1 = one(noise[3:4].to(dev), t[:1])
    assert eps.shape == (N, T, 7) and torch.isfinite(eps.float()).all()
    assert torch.equal(eps, eps2) and torch.equal(eps, eps_e)
    e = fro_rel(eps[3:4], eps_1)
    print(f"window {window}: sample 3's epsilon vs the batch-1 engine {e:.3e}")
    assert e < 2e-2                                                          # the epsilon bound of the cached-vs-whole-forward tests


def test_samples_follow_the_weights(dev, tiny):
    """An in-place update of one decoder weight (mul_ bumps _version) changes the next result; restoring it restores the result."""
    m, _, (_, _, _, _, noise, _), kw, _ = tiny
    before = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)
    w = m.vlm.llm_backbone.llm.model.layers[4].mlp.down_proj.weight
    saved = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    changed = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)
    with torch.no_grad():
        w.copy_(saved)
    restored = m.predict_action_diff_samples(num_samples=N, noise=noise, **kw)
    assert not np.array_equal(changed, before) and np.array_equal(restored, before)


def test_without_prefix_reuse_it_is_the_loop_of_whole_forward_calls(dev, tiny):
    m, window, (_, _, _, _, noise, _), kw, _ = tiny
    n = 2
    loop = np.stack([m.predict_action_diff(noise=noise[i:i + 1], reuse_prefix=False, **kw) for i in range(n)])
    got = m.predict_action_diff_samples(num_samples=n, noise=noise[:n], reuse_prefix=False, **kw)
    assert got.shape == (n, window + 1, 7) and np.array_equal(got, loop)


def test_rng_draws_are_those_of_n_calls(dev, tiny):
    """Without `noise`: randn(1, T, D) then the unused randint per sample, in the order N predict_action_diff calls draw them."""
    m, window, _, kw, _ = tiny
    T = window + 1
    torch.manual_seed(1234)
    draws = []
    for _ in range(2):
        draws.append(torch.randn(1, T, 7, device=dev))
        torch.randint(0, m.diffusion.num_timesteps, (T,), device=dev)
    torch.manual_seed(1234)
    got = m.predict_action_diff_samples(num_samples=2, **kw)
    assert np.array_equal(got, m.predict_action_diff_samples(num_samples=2, noise=torch.cat(draws).cpu(), **kw))
    torch.manual_seed(1234)
    first = m.predict_action_diff(**kw)                                      # the first of the N calls draws the same initial sample
    assert _rel(got[0], first) < 3e-2


def test_argument_errors(dev, tiny):
    m, window, (_, _, _, _, noise, _), kw, _ = tiny
    T = window + 1
    with pytest.raises(NotImplementedError):
        m.predict_action_diff_samples(num_samples=2, noise=noise[:2], cfg_scale=1.5, **kw)
    with pytest.raises(ValueError):
        m.predict_action_diff_samples(num_samples=0, **kw)
    for bad in (noise[:3], noise[:2, :T - 1], noise[:2, :, :6], noise[0]):
        with pytest.raises(ValueError):
            m.predict_action_diff_samples(num_samples=2, noise=bad, **kw)
