"""GPU: N action chunks for each of B observations on one cached-prefix pass -- mla_attn_chunk_ragged_groups (G groups of R suffix rows
behind every sample's own prefix, lengths on the device), mla_gemm_suffix_bf16_pos / mla_gemm_suffix_w8_pos (cache row and rotary position
from two device arrays), mla_amd/infer.py:BatchedSampleGroupsEps and MLA.predict_action_diff_batch(num_samples=N).

The attention kernel's parity statement is an identity: the rows of (b, g) are bit for bit mla_attn_chunk (B = 1, S_kv = S_p[b] + R) on
cat(prefix rows of b, rows of group g), and mla_attn_chunk_groups on sample b's slice. 5e-3 Frobenius-relative against fp32 is
mla_attn_chunk_groups' bound; 3e-2 relative L2 per chunk is the project's bound for the batch and samples engines."""
import math

import numpy as np
import pytest
import torch

import infer_batch_samples_cases as bsc
import infer_samples_cases as isc
from conftest import fro_rel
from oracle import recipe

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 1 / math.sqrt(128)
SENT = 777.0                                                                  # bf16-exact


def _rand(shape, seed, scale, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(BF)


def _tables(S, dev, D=128):
    fr = torch.outer(torch.arange(S).float(), 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))
    return fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)


def _i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def _cache(dev, S_p, G, R, H, nan_tail=True):
    """[B, S_cap, 3 H 128]; the rows behind S_p[b] + G R are NaN: reading one would show."""
    S_cap = bsc.s_cap(S_p, G, R)
    cache = _rand((len(S_p), S_cap, 3 * H * 128), sum(S_p) * 10 + R * 7 + G + H, 0.7, dev)
    if nan_tail:
        for b, s in enumerate(S_p):
            cache[b, s + G * R:] = float("nan")
    return cache


def _per_sample_groups(cache, S_p, G, H, R):
    from mla_amd import hip
    return torch.cat([hip.attn_chunk_groups(cache[b], G, H, 128, s, R, SCALE) for b, s in enumerate(S_p)])


# ------------------------------------------------------------------------------------------------ attention kernel
@pytest.mark.parametrize("S_p,GR,H", [(m, s, 2) for m in bsc.PREFIX_MIXES for s in bsc.GROUP_SHAPES] + [bsc.H3_CASE + (3,)])
def test_attn_chunk_ragged_groups_is_the_per_sample_per_group_launch_bit_for_bit(dev, S_p, GR, H):
    from mla_amd import hip
    (G, R), B = GR, len(S_p)
    cache = _cache(dev, S_p, G, R, H)
    o = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, _i32(S_p, dev), R, SCALE)
    assert o.shape == (B * G * R, H * 128) and torch.isfinite(o.float()).all()
    for b, s in enumerate(S_p):
        for g in range(G):
            blk = o[(b * G + g) * R:(b * G + g + 1) * R]
            one = hip.attn_chunk(isc.gather_group(cache[b], g, R, s)[None].contiguous(), 1, H, 128, s + R, R, SCALE)
            assert torch.equal(blk, one), f"sample {b} group {g} vs mla_attn_chunk"
    groups = _per_sample_groups(cache, S_p, G, H, R)
    for b in range(B):
        assert torch.equal(o[b * G * R:(b + 1) * G * R], groups[b * G * R:(b + 1) * G * R]), f"sample {b} vs mla_attn_chunk_groups"
    e = fro_rel(o, bsc.attn_ref(cache, S_p, G, H, R))
    print(f"mla_attn_chunk_ragged_groups S_p {S_p} G {G} R {R} H {H}: fro_rel vs fp32 {e:.3e}")
    assert e < 5e-3
    assert torch.equal(o, hip.attn_chunk_ragged_groups(cache, B, G, H, 128, _i32(S_p, dev), R, SCALE))   # a second launch: the same bits
    for gw in (1, 2, 4):                                                     # every launch form: the bits depend on neither the sharing
        for order in (0, 1):                                                 # nor the work order
            got = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, _i32(S_p, dev), R, SCALE, gw=gw, order=order)
            assert torch.equal(o, got), f"gw {gw} order {order}"


@pytest.mark.parametrize("S_p", bsc.PREFIX_MIXES)
@pytest.mark.parametrize("G,R", bsc.ISOLATION_SHAPES)
def test_attn_chunk_ragged_groups_reads_only_the_prefix_and_the_own_group(dev, S_p, G, R):
    """Every cache row outside prefix_b and group (b, g) set to NaN (other groups, other samples, sample b's tail rows; q, k and v parts):
    the block of (b, g) is finite and bit-unchanged, for the library's launch form and the group-sharing ones."""
    from mla_amd import hip
    H, B = 2, len(S_p)
    cache = _cache(dev, S_p, G, R, H, nan_tail=False)
    lens = _i32(S_p, dev)
    clean = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, lens, R, SCALE)
    assert torch.isfinite(clean.float()).all()
    for b in range(B):
        for g in range(G):
            hostile = bsc.hostile(cache, S_p, G, R, b, g)
            for gw in (None, 2, 4):
                o = hip.attn_chunk_ragged_groups(hostile, B, G, H, 128, lens, R, SCALE, gw=gw)
                mine = o[(b * G + g) * R:(b * G + g + 1) * R]
                assert torch.isfinite(mine.float()).all() and torch.equal(mine, clean[(b * G + g) * R:(b * G + g + 1) * R]), (b, g, gw)


def test_attn_chunk_ragged_groups_graph_survives_a_new_length_mix(dev):
    """The lengths are read from device memory: one captured graph, two length mixes."""
    from mla_amd import hip
    B, G, R, H = 3, 3, 17, 2
    first, second = (47, 200, 545), (130, 64, 1)
    S_cap = bsc.s_cap(first, G, R)
    cache = _rand((B, S_cap, 3 * H * 128), 11, 0.7, dev)
    lens = _i32(first, dev)
    hip.attn_chunk_ragged_groups(cache, B, G, H, 128, lens, R, SCALE)           # function attributes outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, lens, R, SCALE)
    g.replay()
    torch.cuda.synchronize()
    one = o.clone()
    assert torch.equal(one, _per_sample_groups(cache, first, G, H, R))
    lens.copy_(torch.tensor(second, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, _per_sample_groups(cache, second, G, H, R)) and not torch.equal(o, one)


def test_attn_chunk_ragged_groups_clamps_the_lengths(dev):
    """prefix_len above S_cap - G R (or below 0) behaves as the clamped value: compared with the clamped launch on a finite cache."""
    from mla_amd import hip
    B, G, R, H, S_cap = 3, 3, 17, 2, 128
    room = S_cap - G * R
    cache = _rand((B, S_cap, 3 * H * 128), 12, 0.7, dev)
    got = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, _i32([room + 1, 2 ** 31 - 1, -5], dev), R, SCALE)
    want = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, _i32([room, room, 0], dev), R, SCALE)
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    assert torch.equal(want, _per_sample_groups(cache, [room, room, 0], G, H, R))


# ------------------------------------------------------------------------------------------------ projection addressing
def _projection_case(dev, G, R, nh, K):
    S_p, B = bsc.PROJECTION_S_P, len(bsc.PROJECTION_S_P)
    H, S_cap, M = nh * 128, bsc.s_cap(S_p, G, R), B * G * R
    x = _rand((M, K), G * 100 + R, 1.1, dev)
    W = _rand((3 * H, K), nh + K + G, 0.06, dev)
    _, slot, pos = bsc.layout(S_p, G, R, S_cap)
    return S_p, B, H, S_cap, M, x, W, slot, pos


def _check_pos_projection(dev, G, R, nh, K, w8):
    """Row p of group (b, g) lands at flat cache row b S_cap + S_p[b] + g R + p and is the dense launch's row rotated at position
    S_p[b] + p; v columns are not rotated; everything else keeps the sentinel."""
    from mla_amd import hip
    S_p, B, H, S_cap, M, x, W, slot, pos = _projection_case(dev, G, R, nh, K)
    if w8:
        q, sc = hip.quant_fp8_rows(W)
        gemm = lambda *a, **k: hip.gemm_suffix_w8(x, q, sc, *a, **k)  # noqa: E731
    else:
        gemm = lambda *a, **k: hip.gemm_suffix(x, W, *a, **k)  # noqa: E731
    ld = 3 * H + 64
    cos, sin = _tables(S_cap, dev)
    got = torch.full((B * S_cap + 2, ld), SENT, dtype=BF, device=dev)
    gemm(got, ld, 0, R, rope=(cos, sin, 2 * H), slot=_i32(slot, dev), cap_rows=B * S_cap, rope_pos=_i32(pos, dev), rope_rows=S_cap)
    dense = torch.full((M, 3 * H), float("nan"), dtype=BF, device=dev)
    gemm(dense, 3 * H, 0, M)
    ref = dense.clone()
    for s in range(B * G):
        hip.rope_inplace(ref[s * R:(s + 1) * R], cos[pos[s]:pos[s] + R].contiguous(), sin[pos[s]:pos[s] + R].contiguous(), R, nh, 128, 0, H)
    assert torch.isfinite(ref.float()).all()
    assert not torch.equal(ref[:, :2 * H], dense[:, :2 * H]) and torch.equal(ref[:, 2 * H:], dense[:, 2 * H:])
    written = torch.zeros(B * S_cap + 2, dtype=torch.bool, device=dev)
    for s in range(B * G):
        assert torch.equal(got[slot[s]:slot[s] + R, :3 * H], ref[s * R:(s + 1) * R]), f"group {s} (sample {s // G})"
        written[slot[s]:slot[s] + R] = True
    assert int(written.sum()) == M                                            # no two groups share a row
    assert bool((got[~written] == SENT).all()) and bool((got[:, 3 * H:] == SENT).all())


@pytest.mark.parametrize("G,R,nh,K", bsc.PROJECTION_CASES)
def test_gemm_suffix_pos_writes_group_rows_behind_every_samples_prefix(dev, G, R, nh, K):
    _check_pos_projection(dev, G, R, nh, K, w8=False)


@pytest.mark.parametrize("G,R,nh,K", bsc.PROJECTION_CASES)
def test_gemm_suffix_w8_pos_writes_group_rows_behind_every_samples_prefix(dev, G, R, nh, K):
    _check_pos_projection(dev, G, R, nh, K, w8=True)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_gemm_suffix_pos_without_positions_is_the_old_entry(dev, w8):
    """rope_pos == NULL through the new entry point: the old entry's bits on a ragged case (unequal slots, rotation at the cache row)."""
    from ctypes import c_void_p
    from mla_amd import hip
    B, R, nh, K = 8, 17, 2, 512
    H, M = nh * 128, B * R
    slots = [3 + (7 * b * b + 5 * b) % 41 for b in range(B)]
    S_cap = max(slots) + R + 2
    x, W = _rand((M, K), 31, 1.1, dev), _rand((3 * H, K), 32, 0.06, dev)
    cos, sin = _tables(S_cap, dev)
    slot = _i32(slots, dev)
    old = torch.full((B, S_cap, 3 * H), SENT, dtype=BF, device=dev)
    new = old.clone()
    if w8:
        q, sc = hip.quant_fp8_rows(W)
        hip.gemm_suffix_w8(x, q, sc, old, 3 * H, old.stride(0), R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=S_cap)
        wargs, sym = (c_void_p(q.data_ptr()), K, c_void_p(sc.data_ptr())), "mla_gemm_suffix_w8_pos"
    else:
        hip.gemm_suffix(x, W, old, 3 * H, old.stride(0), R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=S_cap)
        wargs, sym = (c_void_p(W.data_ptr()), K), "mla_gemm_suffix_bf16_pos"
    hip.call(sym, c_void_p(x.data_ptr()), K, *wargs, c_void_p(new.data_ptr()), 3 * H, new.stride(0), R, c_void_p(slot.data_ptr()), S_cap,
             None, 0, M, 3 * H, K, c_void_p(cos.data_ptr()), c_void_p(sin.data_ptr()), 2 * H, None, 0)
    assert torch.isfinite(new.float()).all() and torch.equal(new, old) and not bool((new == SENT).all())


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_gemm_suffix_pos_outside_the_tables_writes_nothing(dev, w8):
    """A rotary position outside [0, rope_rows) (a host bug) leaves the whole row's sentinel in place, v columns included."""
    from mla_amd import hip
    G, R, nh, K = 2, 5, 1, 512
    S_p, B, H, S_cap, M, x, W, slot, pos = _projection_case(dev, G, R, nh, K)
    pos = list(pos)
    pos[1], pos[4] = S_cap - 2, -1                   # group 1: positions S_cap - 2 .. S_cap + 2, rows 2 .. 4 fall out; group 4: row 0 does
    cos, sin = _tables(S_cap, dev)
    kw = dict(rope=(cos, sin, 2 * H), slot=_i32(slot, dev), cap_rows=B * S_cap, rope_pos=_i32(pos, dev), rope_rows=S_cap)
    got = torch.full((B * S_cap, 3 * H), SENT, dtype=BF, device=dev)
    if w8:
        q, sc = hip.quant_fp8_rows(W)
        hip.gemm_suffix_w8(x, q, sc, got, 3 * H, 0, R, **kw)
    else:
        hip.gemm_suffix(x, W, got, 3 * H, 0, R, **kw)
    for s in range(B * G):
        for p in range(R):
            row = got[slot[s] + p]
            inside = 0 <= pos[s] + p < S_cap
            assert bool((row == SENT).all()) != inside, (s, p)
            assert not inside or torch.isfinite(row.float()).all()
    assert [(s, p) for s in range(B * G) for p in range(R) if not 0 <= pos[s] + p < S_cap] == [(1, 2), (1, 3), (1, 4), (4, 0)]


# ------------------------------------------------------------------------------------------------ end to end, tiny model
N = 3
ENGINES = "_prefix_engines_batch_samples"


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _noise(B, T, tag):
    return torch.randn(B, N, T, 7, generator=recipe._gen(tag))


def _build(dev, window, B):
    """hidden 256, 9 layers, 2 heads of 128 (the existing fixtures' recipe); B ragged observations of test_infer_batch_gpu.batch_inputs."""
    from test_infer_batch_gpu import batch_inputs
    from test_inference_chunk_gpu import build_model
    m = build_model(dev, window)
    ids, images, pcs, proprios, _, starts = batch_inputs(B)
    return m, (ids, images, pcs, proprios, starts), _noise(B, window + 1, f"infer_batch_samples{window}")


def _drop(m):
    import gc
    for name in (ENGINES, "_prefix_engines_batched", "_prefix_engines_samples", "_prefix_engines", "_prefix_packed", "_prefix_fp8"):
        m.vlm.__dict__.pop(name, None)                                       # engines refer back to the vlm: break the cycle
    del m
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tiny3(dev):
    m, obs, noise = _build(dev, 3, 3)
    yield m, 3, obs, noise, {}
    _drop(m)


@pytest.fixture(scope="module")
def tiny15(dev):
    m, obs, noise = _build(dev, 15, 2)
    yield m, 15, obs, noise, {}
    _drop(m)


def _obs_kw(obs, b):
    ids, images, pcs, proprios, _ = obs
    return dict(image=images[b], pointcloud=pcs[b].numpy(), cur_robot_state=proprios[b].numpy(), input_ids=ids[b][None], num_ddim_steps=8)


def _single(m, obs, b, noise_bn, **kw):
    m.vlm.vision_tower_3d.fps_starts_override = [s[b:b + 1] for s in obs[4]]
    return m.predict_action_diff(noise=noise_bn[None], **_obs_kw(obs, b), **kw)


def _samples(m, obs, b, noise_b, **kw):
    m.vlm.vision_tower_3d.fps_starts_override = [s[b:b + 1] for s in obs[4]]
    return m.predict_action_diff_samples(num_samples=noise_b.shape[0], noise=noise_b, **_obs_kw(obs, b), **kw)


def _batched(m, obs, noise, sel=None, num_samples="noise", **kw):
    ids, images, pcs, proprios, starts = obs
    sel = list(range(len(ids))) if sel is None else sel
    m.vlm.vision_tower_3d.fps_starts_override = [s[sel] for s in starts]
    if num_samples == "noise":
        num_samples = noise.shape[1]
    return m.predict_action_diff_batch([images[b] for b in sel], [pcs[b].numpy() for b in sel], cur_robot_states=[proprios[b].numpy() for b in sel],
                                       input_ids=[ids[b] for b in sel], noise=None if noise is None else noise[sel], num_ddim_steps=8,
                                       num_samples=num_samples, **kw)


def _refs(tiny, mode="bf16"):
    """predict_action_diff per (b, n) in the given mode, computed once per module and left unchanged."""
    m, _, obs, noise, memo = tiny
    if mode not in memo:
        kw = {} if mode == "bf16" else {"suffix_weights": mode}
        memo[mode] = np.stack([np.stack([_single(m, obs, b, noise[b, n], **kw) for n in range(noise.shape[1])]) for b in range(noise.shape[0])])
        memo[mode].setflags(write=False)
    return memo[mode]


def _count_prefill_layers(monkeypatch):
    from mla_amd import ops
    calls = []
    orig = ops.DecoderLayerFn._fwd

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(ops.DecoderLayerFn, "_fwd", staticmethod(counted))
    return calls


@pytest.mark.parametrize("fixture", ["tiny3", "tiny15"])
def test_batch_of_sample_groups_matches_the_single_calls(dev, request, fixture):
    """Window 3: B = 3 ragged prompts (id lengths 21 / 14 / 27), N = 3, R = 5. Window 15: B = 2, N = 3, R = 17 -- 102 rows, the M > 64
    projection forms. Every out[b, n] within 3e-2 of predict_action_diff on observation b with noise[b, n] and of
    predict_action_diff_samples(observation b)[n]; two samples of one observation differ."""
    tiny = request.getfixturevalue(fixture)
    m, window, obs, noise, _ = tiny
    B, T = noise.shape[0], window + 1
    got = _batched(m, obs, noise)
    assert got.shape == (B, N, T, 7) and np.isfinite(got).all()
    singles = _refs(tiny)
    d1 = [[_rel(got[b, n], singles[b, n]) for n in range(N)] for b in range(B)]
    d2 = []
    for b in range(B):
        s = _samples(m, obs, b, noise[b])
        d2.append([_rel(got[b, n], s[n]) for n in range(N)])
    fmt = lambda d: [["%.2e" % v for v in row] for row in d]  # noqa: E731
    print(f"window {window} B {B} N {N}: vs predict_action_diff {fmt(d1)}, vs predict_action_diff_samples {fmt(d2)}")
    assert max(max(r) for r in d1) < 3e-2 and max(max(r) for r in d2) < 3e-2
    for b in range(B):
        assert _rel(got[b, 0], got[b, 1]) > 1e-3
    (eng,) = [e for e in m.vlm.__dict__[ENGINES].values() if (e.NB, e.G) == (B, N)]
    assert eng.R == window + 2 and eng.graph is not None and eng.graph_error is None, eng.graph_error
    assert eng.prefix_len.tolist() == [s for s in eng.rope_pos.tolist()[::N]] and eng.S_cap % 64 == 0
    assert eng.slot.tolist() == bsc.layout(eng.prefix_len.tolist(), N, eng.R, eng.S_cap)[1]


def test_one_prefill_per_pass_and_a_second_length_mix_reuses_engine_and_graph(dev, tiny3, monkeypatch):
    """n_layers decoder-layer forwards per call (ONE varlen prefill for the three observations), the pass from a captured graph; another
    mix of id lengths in the same bucket: the same engine object, the same graph, new device tables, results within the bound."""
    from test_infer_batch_gpu import batch_inputs
    m, window, obs, noise, _ = tiny3
    _batched(m, obs, noise)                                                  # engine and graph exist before the launches are counted
    engines = m.vlm.__dict__[ENGINES]
    (key,) = [k for k, e in engines.items() if (e.NB, e.G) == (3, N) and len(k) == 5]
    eng, g0, lens0 = engines[key], engines[key].graph, engines[key].prefix_len.tolist()
    assert g0 is not None and eng.graph_error is None
    calls = _count_prefill_layers(monkeypatch)
    again = _batched(m, obs, noise)
    assert len(calls) == len(m.vlm.llm_backbone.llm.model.layers), len(calls)
    ids, images, pcs, proprios, _, starts = batch_inputs(3, lengths=[21, 27, 16])
    other = (ids, images, pcs, proprios, starts)
    del calls[:]
    got = _batched(m, other, noise)
    assert len(calls) == len(m.vlm.llm_backbone.llm.model.layers), len(calls)
    monkeypatch.undo()
    assert engines[key] is eng and eng.graph is g0 and eng.graph_error is None and eng.prefix_len.tolist() != lens0
    assert [k for k, e in engines.items() if (e.NB, e.G) == (3, N) and len(k) == 5] == [key]
    for b in range(3):
        s = _samples(m, other, b, noise[b])
        d = [_rel(got[b, n], s[n]) for n in range(N)]
        print(f"second mix, observation {b} (ids {len(ids[b])}): vs predict_action_diff_samples {['%.2e' % v for v in d]}")
        assert max(d) < 3e-2
    assert np.array_equal(_batched(m, obs, noise), again)                    # back to the first mix: the first result


def test_batch_of_one_is_predict_action_diff_samples_bit_for_bit(dev, tiny3):
    m, window, obs, noise, _ = tiny3
    for b in (0, 2):
        got = _batched(m, obs, noise, sel=[b])
        assert got.shape == (1, N, window + 1, 7) and np.array_equal(got[0], _samples(m, obs, b, noise[b]))


def test_one_sample_per_observation_is_the_batched_call(dev, tiny3):
    """N = 1, B = 3: [3, 1, T, D], within 3e-2 of predict_action_diff_batch without num_samples (another engine, the same function)."""
    m, window, obs, noise, _ = tiny3
    got = _batched(m, obs, noise[:, :1])
    assert got.shape == (3, 1, window + 1, 7)
    ids, images, pcs, proprios, starts = obs
    m.vlm.vision_tower_3d.fps_starts_override = list(starts)
    want = m.predict_action_diff_batch(images, [p.numpy() for p in pcs], cur_robot_states=[p.numpy() for p in proprios], input_ids=ids,
                                       noise=noise[:, 0], num_ddim_steps=8)
    d = [_rel(got[b, 0], want[b]) for b in range(3)]
    print(f"N = 1 vs predict_action_diff_batch {['%.2e' % v for v in d]}")
    assert want.shape == (3, window + 1, 7) and max(d) < 3e-2


def test_row_cap_patched_down_serves_sub_batches(dev, tiny3, monkeypatch):
    """MAX_ROWS = 20 at R = 5, B = 3, N = 2: passes of 2 + 1 observations; every sample within the bound."""
    from mla_amd import infer
    tiny = tiny3
    m, window, obs, noise, _ = tiny
    monkeypatch.setattr(infer.BatchedSampleGroupsEps, "MAX_ROWS", 20)
    m.vlm.__dict__.pop(ENGINES, None)
    got = _batched(m, obs, noise[:, :2])
    singles = _refs(tiny)
    d = [[_rel(got[b, n], singles[b, n]) for n in range(2)] for b in range(3)]
    print(f"sub-batched 2 + 1: vs predict_action_diff {[['%.2e' % v for v in r] for r in d]}")
    assert got.shape == (3, 2, window + 1, 7) and max(max(r) for r in d) < 3e-2
    assert sorted((e.NB, e.G) for e in m.vlm.__dict__[ENGINES].values()) == [(1, 2), (2, 2)]


def test_more_samples_than_a_pass_loops_predict_action_diff_samples(dev, tiny3, monkeypatch):
    """MAX_ROWS = 2 R, N = 3, B = 2: np.array_equal to the loop of predict_action_diff_samples calls; no batched engine is built. (The
    looped form runs batch-1 calls: both observations are observation 0, so that one start-index override serves every call.)"""
    from mla_amd import infer
    m, window, obs, noise, _ = tiny3
    ids, images, pcs, proprios, starts = obs
    monkeypatch.setattr(infer.BatchedSampleGroupsEps, "MAX_ROWS", 2 * (window + 2))
    m.vlm.__dict__.pop(ENGINES, None)
    want = np.stack([_samples(m, obs, 0, noise[b]) for b in range(2)])
    m.vlm.vision_tower_3d.fps_starts_override = [s[0:1] for s in starts]
    got = m.predict_action_diff_batch([images[0]] * 2, [pcs[0].numpy()] * 2, cur_robot_states=[proprios[0].numpy()] * 2, input_ids=[ids[0]] * 2,
                                      noise=noise[:2], num_ddim_steps=8, num_samples=N)
    assert got.shape == (2, N, window + 1, 7) and np.array_equal(got, want)
    assert not m.vlm.__dict__.get(ENGINES)


def test_fp8_suffix_weights_for_a_batch(dev, tiny3, monkeypatch):
    """suffix_weights="fp8", B = 3, N = 3: within 3e-2 of predict_action_diff(suffix_weights="fp8") per (b, n); not the bf16 result; the
    pass issues mla_gemm_suffix_w8 for its four projections per layer and no bf16 suffix GEMM (wrapper calls of the eager warm-up and of
    the capture that follows it: two passes). "fp8_as_bf16" stays within the bound of "fp8"."""
    from mla_amd import hip
    tiny = tiny3
    m, window, obs, noise, _ = tiny
    bf16 = _batched(m, obs, noise)
    m.vlm.__dict__.pop(ENGINES, None)                                         # a fresh engine: warm-up and capture happen in this call
    counts = {"w8": 0, "bf16": 0}
    w8_orig, bf_orig = hip.gemm_suffix_w8, hip.gemm_suffix

    def w8(*a, **k):
        counts["w8"] += 1
        return w8_orig(*a, **k)

    def bf(*a, **k):
        counts["bf16"] += 1
        return bf_orig(*a, **k)
    monkeypatch.setattr(hip, "gemm_suffix_w8", w8)
    monkeypatch.setattr(hip, "gemm_suffix", bf)
    got = _batched(m, obs, noise, suffix_weights="fp8")
    monkeypatch.undo()
    (eng,) = m.vlm.__dict__[ENGINES].values()
    assert eng.suffix_weights == "fp8" and eng.graph is not None and eng.graph_error is None, eng.graph_error
    n_layers = len(m.vlm.llm_backbone.llm.model.layers)
    assert counts == {"w8": 2 * 4 * n_layers, "bf16": 0}, counts
    refs = _refs(tiny, "fp8")
    d = [[_rel(got[b, n], refs[b, n]) for n in range(N)] for b in range(3)]
    print(f"fp8 B 3 N {N}: vs predict_action_diff(fp8) {[['%.2e' % v for v in r] for r in d]}; vs the bf16 batch {_rel(got, bf16):.2e}")
    assert got.shape == (3, N, window + 1, 7) and max(max(r) for r in d) < 3e-2
    assert not np.array_equal(got, bf16)
    twin = _batched(m, obs, noise, suffix_weights="fp8_as_bf16")
    d = [[_rel(twin[b, n], got[b, n]) for n in range(N)] for b in range(3)]
    print(f"fp8_as_bf16 vs fp8 {[['%.2e' % v for v in r] for r in d]}")
    assert max(max(r) for r in d) < 3e-2
    assert sorted(k[5:] for k in m.vlm.__dict__[ENGINES]) == [("fp8",), ("fp8_as_bf16",)]


def test_the_default_path_is_unchanged(dev, tiny3):
    """num_samples=None: B >= 2 with "fp8" still raises NotImplementedError naming BatchedPrefixCachedEps; bf16 keeps [B, T, D] and is
    reproducible; no BatchedSampleGroupsEps engine appears."""
    m, window, obs, noise, _ = tiny3
    m.vlm.__dict__.pop(ENGINES, None)
    with pytest.raises(NotImplementedError, match="BatchedPrefixCachedEps"):
        _batched(m, obs, noise[:, 0], num_samples=None, suffix_weights="fp8")
    a = _batched(m, obs, noise[:, 0], num_samples=None)
    b = _batched(m, obs, noise[:, 0], num_samples=None)
    assert a.shape == (3, window + 1, 7) and np.isfinite(a).all() and np.array_equal(a, b)
    assert not m.vlm.__dict__.get(ENGINES)


def test_other_argument_behaviour(dev, tiny3):
    m, window, obs, noise, _ = tiny3
    for mode in ("fp8", "fp8_as_bf16"):
        with pytest.raises(ValueError, match="reuse_prefix"):
            _batched(m, obs, noise, reuse_prefix=False, suffix_weights=mode)
    with pytest.raises(NotImplementedError):
        _batched(m, obs, noise, cfg_scale=1.5)
    with pytest.raises(ValueError):
        _batched(m, obs, noise, num_samples=0)
    with pytest.raises(ValueError):
        _batched(m, obs, noise, num_samples=2)                               # noise is [3, 3, T, D]


def test_without_prefix_reuse_it_is_the_loop_of_whole_forward_calls(dev, tiny3):
    """reuse_prefix=False: the reference's control flow per (b, n). Both observations are observation 0 (one start-index override)."""
    m, window, obs, noise, _ = tiny3
    ids, images, pcs, proprios, starts = obs
    want = np.stack([np.stack([_single(m, obs, 0, noise[b, n], reuse_prefix=False) for n in range(2)]) for b in range(2)])
    m.vlm.vision_tower_3d.fps_starts_override = [s[0:1] for s in starts]
    got = m.predict_action_diff_batch([images[0]] * 2, [pcs[0].numpy()] * 2, cur_robot_states=[proprios[0].numpy()] * 2, input_ids=[ids[0]] * 2,
                                      noise=noise[:2, :2], num_ddim_steps=8, num_samples=2, reuse_prefix=False)
    assert got.shape == (2, 2, window + 1, 7) and np.array_equal(got, want)


def test_rng_draws_are_those_of_b_calls_of_n_samples(dev, tiny3):
    """Without `noise`: for b: for n: randn(1, T, D), then the unused randint."""
    m, window, obs, _, _ = tiny3
    T = window + 1
    torch.manual_seed(4321)
    draws = []
    for _ in range(3 * 2):
        draws.append(torch.randn(1, T, 7, device=dev))
        torch.randint(0, m.diffusion.num_timesteps, (T,), device=dev)
    torch.manual_seed(4321)
    got = _batched(m, obs, None, num_samples=2)
    want = _batched(m, obs, torch.cat(draws).view(3, 2, T, 7).cpu())
    assert got.shape == (3, 2, T, 7) and np.array_equal(got, want)
