"""GPU: batched action sampling -- B observations with ragged prompts on one cached-prefix pass (mla_gemm_suffix_bf16,
mla_attn_chunk_ragged through the C-ABI wrappers; mla_amd/infer.py:BatchedPrefixCachedEps; MLA.predict_action_diff_batch).
Semantics: predict_action_diff_batch on B observations == B independent predict_action_diff calls (FPS start indices given)."""
import math
import os

import numpy as np
import pytest
import torch

import infer_batch_cases as ibc
from conftest import fro_rel
from oracle import recipe

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
BF = torch.bfloat16


def _rand(shape, seed, scale, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(BF)


def _tables(S, dev, D=128):
    fr = torch.outer(torch.arange(S).float(), 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D)))
    return fr.cos().contiguous().to(dev), fr.sin().contiguous().to(dev)


# ------------------------------------------------------------------------------------------------ suffix GEMM
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("N,K", [(4096, 512), (1536, 4096), (1000, 4096), (520, 11008), (7, 512)])
@pytest.mark.parametrize("M", [1, 17, 64, 65, 136, 255, 256])
def test_gemm_suffix_matches_fp32_reference(dev, M, N, K, res):
    """out[m] = x[m] @ W^T (+ residual) for 1 <= M <= 256, every kernel form (1 / 2 / 4 W tiles per workgroup, one or two row groups),
    N not a multiple of 16 / 32 / 64, K not a multiple of the 32-wide step split over the waves. Frobenius-relative <= 4e-3, the
    per-kernel bf16 bound."""
    from mla_amd import hip
    x = _rand((M, K), M * 7 + K, 0.5, dev)
    W = _rand((N, K), N + K, 0.05, dev)
    r = _rand((M, N), M + N, 1.0, dev) if res else None
    want = x.float() @ W.float().t() + (r.float() if res else 0)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    hip.gemm_suffix(x, W, out, N, 0, M, r)
    assert torch.isfinite(out.float()).all()
    e = fro_rel(out, want)
    print(f"gemm_suffix M {M} N {N} K {K} res {res}: fro_rel {e:.3e}")
    assert e <= 4e-3


@pytest.mark.parametrize("M,N,K", [(1, 1536, 4096), (17, 1000, 4096), (33, 520, 11008), (64, 4096, 512), (48, 7, 520)])
def test_gemm_suffix_up_to_64_rows_is_gemm_skinny_bit_for_bit(dev, M, N, K):
    """M <= 64: the same K split over 8 waves and the same fixed-order partial sum as mla_gemm_skinny_bf16 -- plain and residual forms,
    dense and batch-strided outputs."""
    from mla_amd import hip
    x = _rand((M, K), M + K, 0.5, dev)
    W = _rand((N, K), N + K + 1, 0.05, dev)
    r = _rand((M, N), M + N + 2, 1.0, dev)
    for res in (None, r):
        a, b = (torch.full((M, N), float("nan"), dtype=BF, device=dev) for _ in range(2))
        hip.gemm_skinny(x, W, a, N, 0, M, res)
        hip.gemm_suffix(x, W, b, N, 0, M, res)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("B,R,nh,K", [(1, 17, 4, 4096), (4, 16, 2, 4096), (3, 17, 2, 512), (1, 64, 3, 512)])
def test_gemm_suffix_uniform_slots_rope_is_gemm_skinny_bit_for_bit(dev, B, R, nh, K):
    """Rotary form with every slot[b] equal (M <= 64): bit-identical to mla_gemm_skinny_bf16 writing at that slot with the tables
    sliced there; also with slot = None (the skinny addressing itself). The rotation really happened; nothing else is touched."""
    from mla_amd import hip
    H = nh * 128
    M, S_p = B * R, 11
    S_cap = S_p + R + 5
    x = _rand((M, K), nh * 10 + R, 1.1, dev)
    W = _rand((3 * H, K), nh + K, 0.06, dev)
    cos, sin = _tables(S_cap, dev)
    ref = torch.zeros((B, S_cap, 3 * H), dtype=BF, device=dev)
    hip.gemm_skinny(x, W, ref[:, S_p:], 3 * H, ref.stride(0), R, rope=(cos[S_p:S_p + R].contiguous(), sin[S_p:S_p + R].contiguous(), 2 * H))
    plain = torch.zeros_like(ref)
    hip.gemm_skinny(x, W, plain[:, S_p:], 3 * H, plain.stride(0), R)
    got = torch.zeros_like(ref)
    slot = torch.full((B,), S_p, dtype=torch.int32, device=dev)
    hip.gemm_suffix(x, W, got, 3 * H, got.stride(0), R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=S_cap)
    assert torch.isfinite(got.float()).all() and torch.equal(got, ref)
    assert not torch.equal(got[:, S_p:S_p + R, :2 * H], plain[:, S_p:S_p + R, :2 * H]) and torch.equal(got[:, :, 2 * H:], plain[:, :, 2 * H:])
    got2 = torch.zeros_like(ref)
    hip.gemm_suffix(x, W, got2[:, S_p:], 3 * H, got2.stride(0), R, rope=(cos[S_p:S_p + R].contiguous(), sin[S_p:S_p + R].contiguous(), 2 * H))
    assert torch.equal(got2, ref)


@pytest.mark.parametrize("B,R,nh,K", [(3, 4, 2, 512), (3, 17, 2, 4096), (8, 17, 2, 4096), (15, 17, 1, 512), (4, 64, 1, 512)])
def test_gemm_suffix_ragged_slots_equal_plain_projection_plus_rope(dev, B, R, nh, K):
    """Unequal slot[b] (M = 12 .. 256, every kernel form): the fused output == the plain projection written at each sample's slot followed
    by rope_inplace at that sample's positions, bit for bit; cache rows outside the addressed slots keep the sentinel."""
    from mla_amd import hip
    H = nh * 128
    M = B * R
    slots = [3 + (7 * b * b + 5 * b) % 41 for b in range(B)]
    S_cap = max(slots) + R + 2
    x = _rand((M, K), B * 100 + R, 1.1, dev)
    W = _rand((3 * H, K), nh + K + B, 0.06, dev)
    cos, sin = _tables(S_cap, dev)
    slot = torch.tensor(slots, dtype=torch.int32, device=dev)
    SENT = 777.0                                                              # bf16-exact
    got = torch.full((B, S_cap, 3 * H), SENT, dtype=BF, device=dev)
    hip.gemm_suffix(x, W, got, 3 * H, got.stride(0), R, rope=(cos, sin, 2 * H), slot=slot, cap_rows=S_cap)
    ref = torch.full((B, S_cap, 3 * H), SENT, dtype=BF, device=dev)
    hip.gemm_suffix(x, W, ref, 3 * H, ref.stride(0), R, slot=slot, cap_rows=S_cap)             # plain, ragged addressing
    dense = torch.full((M, 3 * H), float("nan"), dtype=BF, device=dev)
    hip.gemm_suffix(x, W, dense, 3 * H, 0, M)
    for b, s in enumerate(slots):
        assert torch.equal(ref[b, s:s + R], dense[b * R:(b + 1) * R])         # the ragged addressing moves rows, nothing else
        rows = ref[b, s:s + R]
        hip.rope_inplace(rows, cos[s:s + R].contiguous(), sin[s:s + R].contiguous(), R, nh, 128, 0, H)
    assert torch.isfinite(got.float()).all() and torch.equal(got, ref)
    for b, s in enumerate(slots):
        assert bool((got[b, :s] == SENT).all()) and bool((got[b, s + R:] == SENT).all())
        assert not torch.equal(got[b, s:s + R, :2 * H], dense[b * R:(b + 1) * R, :2 * H])


def test_gemm_suffix_rows_beyond_the_capacity_are_not_written(dev):
    """A slot that would put rows outside [0, cap_rows) (a host bug) writes nothing there."""
    from mla_amd import hip
    B, R, N, K, S_cap = 2, 4, 256, 512, 10
    x, W = _rand((B * R, K), 1, 1.0, dev), _rand((N, K), 2, 0.05, dev)
    buf = torch.full((B + 1, S_cap, N), 5.0, dtype=BF, device=dev)
    slot = torch.tensor([8, 2], dtype=torch.int32, device=dev)               # sample 0: rows 8, 9 fit, 10 and 11 do not
    hip.gemm_suffix(x, W, buf, N, buf.stride(0), R, slot=slot, cap_rows=S_cap)
    assert bool((buf[0, :8] == 5.0).all()) and not bool((buf[0, 8:] == 5.0).any())
    assert bool((buf[1, :2] == 5.0).all()) and bool((buf[1, 6:] == 5.0).all()) and bool((buf[2] == 5.0).all())


# ------------------------------------------------------------------------------------------------ ragged chunk attention
@pytest.mark.parametrize("H", [2, 32])
@pytest.mark.parametrize("R,kv_len", [(17, [17, 63, 64, 65, 1030]), (4, [4, 128, 129, 1030, 7]), (1, [1, 64, 65]), (64, [64, 127, 128, 129, 1030]),
                                      (16, [562, 548, 575, 562])])
def test_attn_chunk_ragged_is_attn_chunk_per_sample(dev, R, kv_len, H):
    """kv_len mixes with kv_len = R, lengths on both sides of a 64-key tile edge and 1030: per sample bit-identical to mla_attn_chunk at
    B = 1 with S_kv = kv_len[b] on that sample's rows; <= 4e-3 against the fp64 reference. Rows at and behind kv_len[b] are NaN: reading
    one would show."""
    from mla_amd import hip
    B, S_cap = len(kv_len), -(-max(kv_len) // 64) * 64
    cache = ibc.make_ragged_cache(B, H, S_cap, kv_len, seed=sum(kv_len) + R + H).to(dev)
    kv = torch.tensor(kv_len, dtype=torch.int32, device=dev)
    scale = 1 / math.sqrt(128)
    o = hip.attn_chunk_ragged(cache, B, H, 128, kv, R, scale)
    assert o.shape == (B * R, H * 128) and torch.isfinite(o.float()).all()
    for b, n in enumerate(kv_len):
        one = hip.attn_chunk(cache[b:b + 1], 1, H, 128, n, R, scale)
        assert torch.equal(o[b * R:(b + 1) * R], one), (b, n)
    e = fro_rel(o, ibc.ragged_attn_r64(cache.cpu(), kv_len, R, H).float())
    print(f"attn_chunk_ragged R {R} kv_len {kv_len} H {H}: fro_rel vs fp64 {e:.3e}")
    assert e <= 4e-3


def test_attn_chunk_ragged_graph_survives_a_new_length_mix(dev):
    """The lengths are read from device memory: one captured graph, two length mixes."""
    from mla_amd import hip
    B, H, R, S_cap = 3, 4, 17, 640
    scale = 1 / math.sqrt(128)
    cache = _rand((B, S_cap, 3 * H * 128), 5, 0.7, dev)
    kv = torch.tensor([600, 17, 320], dtype=torch.int32, device=dev)
    eager = hip.attn_chunk_ragged(cache, B, H, 128, kv, R, scale)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = hip.attn_chunk_ragged(cache, B, H, 128, kv, R, scale)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, eager)
    mix = [65, 640, 129]
    kv.copy_(torch.tensor(mix, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    for b, n in enumerate(mix):
        assert torch.equal(o[b * R:(b + 1) * R], hip.attn_chunk(cache[b:b + 1], 1, H, 128, n, R, scale))


# ------------------------------------------------------------------------------------------------ end to end on the tiny model
def batch_inputs(B, T=4, lengths=None):
    """B distinct observations; sample 0 is tests/test_inference_gpu.py:infer_inputs() (the sample of golden/inference.npz)."""
    from test_inference_gpu import infer_inputs
    ids0, image0, pc0, proprio0, noise0, starts0 = infer_inputs()
    lengths = lengths or [21, 14, 27]
    lengths = [lengths[b % len(lengths)] + (b // len(lengths)) for b in range(B)]
    lengths[0] = 21
    g = recipe._gen(f"infer_batch{B}")
    ids, images, pcs, proprios, noises, s0, s1 = [ids0[0]], [image0[0]], [pc0[0]], [proprio0[0, 0]], [noise0[0]], [starts0[0]], [starts0[1]]
    lo, hi = torch.tensor([0.0, -0.4, 0.75]), torch.tensor([0.6, 0.4, 1.25])
    for b in range(1, B):
        row = torch.randint(3, 29000, (lengths[b] - 1,), generator=g)
        row[0] = 1
        ids.append(torch.cat([row, torch.tensor([29871])]))
        images.append(torch.cat([torch.randn(3, 672, 672, generator=g), torch.ones(1, 672, 672)], dim=0))
        pcs.append(lo + (hi - lo) * torch.rand(1024, 3, generator=g))
        proprios.append(torch.rand(7, generator=g) * 2 - 1)
        noises.append(torch.randn(T, 7, generator=g))
        s0.append(torch.randint(0, 1024, (1,), generator=g))
        s1.append(torch.randint(0, 512, (1,), generator=g))
    assert [len(r) for r in ids] == lengths
    return ids, images, pcs, proprios, torch.stack(noises), [torch.cat(s0), torch.cat(s1)]


@pytest.fixture(scope="module")
def model(dev):
    import gc
    from test_inference_chunk_gpu import build_model
    m = build_model(dev, 3)
    yield m, np.load(os.path.join(G, "inference.npz"), allow_pickle=True)
    for name in ("_prefix_engines_batched", "_prefix_engines", "_prefix_packed"):   # engines refer back to the vlm: break the cycle
        m.vlm.__dict__.pop(name, None)
    del m
    gc.collect()
    torch.cuda.empty_cache()


def _single(m, inp, b, **kw):
    ids, images, pcs, proprios, noise, starts = inp
    m.vlm.vision_tower_3d.fps_starts_override = [s[b:b + 1] for s in starts]
    return m.predict_action_diff(image=images[b], pointcloud=pcs[b].numpy(), cur_robot_state=proprios[b].numpy(), input_ids=ids[b][None],
                                 noise=noise[b:b + 1], num_ddim_steps=8, **kw)


def _batched(m, inp, sel=None, **kw):
    ids, images, pcs, proprios, noise, starts = inp
    sel = list(range(len(ids))) if sel is None else sel
    m.vlm.vision_tower_3d.fps_starts_override = [s[sel] for s in starts]
    return m.predict_action_diff_batch([images[b] for b in sel], [pcs[b].numpy() for b in sel], cur_robot_states=[proprios[b].numpy() for b in sel],
                                       input_ids=[ids[b] for b in sel], noise=noise[sel], num_ddim_steps=8, **kw)


def _check_against_singles(m, gold, inp, got, label, sel=None):
    sel = list(range(len(inp[0]))) if sel is None else sel
    assert got.shape == (len(sel), 4, 7) and np.isfinite(got).all()
    worst = 0.0
    for i, b in enumerate(sel):
        full = _single(m, inp, b, reuse_prefix=False)
        d = np.linalg.norm(got[i] - full) / np.linalg.norm(full)
        print(f"{label}: sample {b} (ids {len(inp[0][b])}) batched vs whole-forward batch-1 chunk {d:.3e}")
        worst = max(worst, d)
        assert d <= 3e-2, (label, b, d)
    if sel[0] == 0:
        ref = gold["mla_ddim8_actions"][0]
        e = np.linalg.norm(got[0] - ref) / np.linalg.norm(ref)
        print(f"{label}: sample 0 vs reference golden {e:.3e}")
        assert e <= 1e-1
    return worst


def test_batch_of_three_ragged_prompts_matches_batch_1_calls(dev, model):
    """B = 3, id lengths 21 / 14 / 27, everything distinct per sample: each sample within 3e-2 of predict_action_diff(reuse_prefix=False)
    on that sample alone, sample 0 within 1e-1 of the reference golden; the pass runs from a captured graph."""
    m, gold = model
    inp = batch_inputs(3)
    got = _batched(m, inp)
    _check_against_singles(m, gold, inp, got, "B=3")
    (eng,) = [e for e in m.vlm.__dict__["_prefix_engines_batched"].values() if e.B == 3]
    assert eng.R == 5 and eng.graph is not None, eng.graph_error
    slot = eng.slot.tolist()
    assert [s - slot[0] for s in slot] == [0, 14 - 21, 27 - 21]               # prefix length = front tokens + id length
    assert eng.kv_len.tolist() == [s + 5 for s in slot] and eng.S_cap % 64 == 0 and eng.S_cap >= max(slot) + 5


def test_second_length_mix_in_the_bucket_reuses_engine_and_graph(dev, model):
    """Another mix of id lengths with the same longest prompt (so certainly the same capacity bucket): the same engine object, the same
    captured graph, new device tables; the results still meet the bound. So does a permutation of the first mix."""
    m, gold = model
    inp = batch_inputs(3)
    _batched(m, inp)
    engines = m.vlm.__dict__["_prefix_engines_batched"]
    (key,) = [k for k, e in engines.items() if e.B == 3]
    eng, g0 = engines[key], engines[key].graph
    assert g0 is not None
    slot0 = eng.slot.tolist()
    other = batch_inputs(3, lengths=[21, 27, 16])
    got = _batched(m, other)
    assert [k for k, e in engines.items() if e.B == 3] == [key] and engines[key] is eng and eng.graph is g0
    assert eng.slot.tolist() != slot0
    _check_against_singles(m, gold, other, got, "B=3, second mix")
    got2 = _batched(m, inp, sel=[2, 0, 1])
    assert engines[key] is eng and eng.graph is g0
    _check_against_singles(m, gold, inp, got2, "B=3, permuted", sel=[2, 0, 1])


def test_batch_of_fourteen_takes_the_wide_projection(dev, model):
    """B = 14: 70 suffix rows, beyond the 64 rows of the skinny form (two W tiles per workgroup)."""
    m, gold = model
    inp = batch_inputs(14)
    got = _batched(m, inp)
    _check_against_singles(m, gold, inp, got, "B=14")
    eng = [e for e in m.vlm.__dict__["_prefix_engines_batched"].values() if e.B == 14]
    assert len(eng) == 1 and eng[0].graph is not None


def test_row_cap_patched_down_serves_sub_batches(dev, model, monkeypatch):
    """MAX_ROWS = 10 with R = 5: B = 5 is served as sub-batches of 2 + 2 + 1 samples; the results meet the same bound."""
    from mla_amd import infer
    m, gold = model
    monkeypatch.setattr(infer.BatchedPrefixCachedEps, "MAX_ROWS", 10)
    m.vlm.__dict__.pop("_prefix_engines_batched", None)
    inp = batch_inputs(5)
    got = _batched(m, inp)
    _check_against_singles(m, gold, inp, got, "B=5 as 2+2+1")
    assert sorted(e.B for e in m.vlm.__dict__["_prefix_engines_batched"].values()) in ([1, 2], [1, 2, 2])


def test_batch_of_one_is_predict_action_diff_bit_for_bit(dev, model):
    m, gold = model
    inp = batch_inputs(3)
    for b in (0, 2):
        one = _single(m, inp, b)
        got = _batched(m, inp, sel=[b])
        assert got.shape == (1, 4, 7) and np.array_equal(got[0], one)


def test_reuse_prefix_false_loops_the_reference_control_flow_and_cfg_raises(dev, model):
    m, gold = model
    inp = batch_inputs(3)
    ids, images, pcs, proprios, noise, starts = inp
    # the looped form calls predict_action_diff per sample: give every call sample b's start indices through a batch-1 override
    full = [_single(m, inp, b, reuse_prefix=False) for b in range(2)]
    m.vlm.vision_tower_3d.fps_starts_override = [s[0:1] for s in starts]
    got = m.predict_action_diff_batch([images[0]] * 2, [pcs[0]] * 2, cur_robot_states=[proprios[0].numpy()] * 2, input_ids=[ids[0]] * 2,
                                      noise=noise[[0, 0]], reuse_prefix=False)
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[0])
    with pytest.raises(NotImplementedError):
        _batched(m, inp, cfg_scale=1.5)
    with pytest.raises(ValueError):
        m.predict_action_diff_batch(images, [p.numpy() for p in pcs], cur_robot_states=[p.numpy() for p in proprios], noise=noise)


def test_unsupported_shape_warns_once_and_loops_whole_forwards(dev, model, monkeypatch):
    """The capability rule refusing the shape (head_dim != 128 cannot be built as a model: LlamaConfig rejects it; here the rows-per-sample
    limit patched below R = 5) -> one warning, then a loop over whole-forward batch-1 calls: the results ARE reuse_prefix=False's."""
    from mla_amd import infer
    m, gold = model
    monkeypatch.setattr(infer.BatchedPrefixCachedEps, "MAX_R", 2)
    m.vlm.__dict__.pop("_prefix_engines_batched", None)
    m.vlm.__dict__.pop("_prefix_unsupported", None)
    inp = batch_inputs(2)
    ids, images, pcs, proprios, noise, starts = inp
    m.vlm.vision_tower_3d.fps_starts_override = [s[0:1] for s in starts]
    kw = dict(cur_robot_states=[proprios[0].numpy()] * 2, input_ids=[ids[0]] * 2, noise=noise[[0, 0]])
    with pytest.warns(RuntimeWarning, match="5 suffix rows per sample"):
        got = m.predict_action_diff_batch([images[0]] * 2, [pcs[0]] * 2, **kw)
    full = _single(m, inp, 0, reuse_prefix=False)
    assert np.array_equal(got[0], full) and np.array_equal(got[1], full)
    assert not m.vlm.__dict__.get("_prefix_engines_batched")
