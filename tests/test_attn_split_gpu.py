"""GPU: mla_attn_chunk_split (mla_amd/csrc/attn_split.hip) -- mla_attn_chunk with every head's key tiles cut over several workgroups and
a second launch that merges the partial softmax states in a fixed order.

splits = 1 is mla_attn_chunk bit for bit; every other split count keeps mla_attn_chunk's bound against the fp32 reference (5e-3) and stays
within twice mla_attn_chunk's own error on the same inputs; the result does not depend on what the workspace or the rows behind S_kv held,
nothing outside the workspace bytes and the B * R output rows is written, and a captured graph replays the eager bits."""
import math
from ctypes import c_void_p

import pytest
import torch

from conftest import fro_rel
from test_inference_chunk_gpu import _attn_ref, _rand

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SCALE = 1 / math.sqrt(128)


def _cache(dev, B, H, S_kv, R):
    return _rand((B, S_kv + 3, 3 * H * 128), S_kv * 100 + R + B + H, 0.7, dev)       # 3 rows behind S_kv, as the chunk tests allocate


def _split_counts(B, H, R, S_kv):
    from mla_amd import hip
    nT = -(-S_kv // 64)
    plan = hip.plan_attn_split(B, H, R, S_kv).splits
    assert plan == hip.attn_split_plan(B, H, R, S_kv)[0]
    return sorted({s for s in (2, 3, nT, plan) if s <= nT}), plan


@pytest.mark.parametrize("S_kv", [None, 77, 565])
@pytest.mark.parametrize("R", [1, 9, 17, 64])
def test_one_split_is_attn_chunk_bit_for_bit(dev, R, S_kv):
    from mla_amd import hip
    S_kv = R if S_kv is None else S_kv
    for B, H in ((1, 2), (2, 2)):
        cache = _cache(dev, B, H, S_kv, R)
        want = hip.attn_chunk(cache, B, H, 128, S_kv, R, SCALE)
        got = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=1)       # ws=None: one split is attn_chunk's own launch, no workspace
        assert torch.equal(got, want), (B, H, float((got.float() - want.float()).abs().max()))


CASES = [(R, S_kv) for R in (1, 2, 8, 9, 16, 17, 64) for S_kv in (65, 130, 547, 565)] + [(64, 64), (17, 17)]   # R = S_kv: no prefix


@pytest.mark.parametrize("R,S_kv", CASES, ids=[f"R{r}-S{s}" for r, s in CASES])
def test_split_matches_fp32_reference_and_attn_chunk_error(dev, R, S_kv):
    """splits in {2, 3, nT, plan} (those <= nT; R = S_kv has one tile, i.e. the plan's 1 only): finite, fro_rel < 5e-3 against the fp32
    reference (mla_attn_chunk's bound), and <= 2 x the error mla_attn_chunk itself has on these inputs. (R 64, S_kv 130, splits 3): the
    last range holds keys 128, 129, behind the causal limit of queries 0 .. 61 -- their state there is the empty one."""
    from mla_amd import hip
    B, H = (2, 2) if (R + S_kv) % 2 else (1, 2)
    cache = _cache(dev, B, H, S_kv, R)
    ref = _attn_ref(cache, B, H, S_kv, R)
    e_old = fro_rel(hip.attn_chunk(cache, B, H, 128, S_kv, R, SCALE), ref)
    counts, plan = _split_counts(B, H, R, S_kv)
    if S_kv == R:
        counts = [1]
    assert counts and ((R, S_kv) != (64, 130) or 3 in counts)
    for splits in counts:
        o = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits)
        assert o.shape == (B * R, H * 128) and torch.isfinite(o.float()).all()
        e_new = fro_rel(o, ref)
        print(f"B {B} H {H} R {R} S_kv {S_kv} splits {splits}{' (plan)' if splits == plan else ''}: fro_rel {e_new:.3e}, attn_chunk {e_old:.3e}")
        assert e_new < 5e-3
        assert e_new <= 2 * e_old


def test_split_at_32_heads_batch_2(dev):
    """The 7B head count once: the plan's count (the batch-1 sampler step's shape, twice) and every tile on its own."""
    from mla_amd import hip
    B, H, R, S_kv = 2, 32, 2, 547
    cache = _cache(dev, B, H, S_kv, R)
    ref = _attn_ref(cache, B, H, S_kv, R)
    e_old = fro_rel(hip.attn_chunk(cache, B, H, 128, S_kv, R, SCALE), ref)
    plan = hip.plan_attn_split(B, H, R, S_kv).splits
    assert plan > 1
    for splits in (plan, 9):
        o = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits)
        e_new = fro_rel(o, ref)
        print(f"H 32 B 2 R 2 S_kv 547 splits {splits}: fro_rel {e_new:.3e}, attn_chunk {e_old:.3e}")
        assert torch.isfinite(o.float()).all() and e_new < 5e-3 and e_new <= 2 * e_old
    assert torch.equal(hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE), hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=plan))


@pytest.mark.parametrize("R,S_kv,splits", [(2, 547, 4), (17, 565, 9), (64, 130, 3), (9, 130, 2)])
def test_isolation_and_determinism(dev, R, S_kv, splits):
    """A second call, a call on a workspace full of NaN and a call with NaN in the rows at and behind S_kv give the same bits; the bytes
    behind ws_bytes and the rows of o outside B * R keep theirs."""
    from mla_amd import hip
    B, H = 2, 2
    cache = _cache(dev, B, H, S_kv, R)
    need = hip.attn_split_ws_bytes(B, H, R, S_kv, splits)
    assert need == B * H * R * splits * 130 * 4
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    first = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws[:need])
    assert torch.equal(first, hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws[:need]))
    ws[:need].view(torch.float32).fill_(float("nan"))
    assert torch.equal(first, hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws[:need]))
    assert torch.isfinite(ws[:need].view(torch.float32)[:B * H * R * splits * 128]).all()          # every sum of every state was written
    assert bool((ws[need:] == 0xA5).all())
    poisoned = cache.clone()
    poisoned[:, S_kv:] = float("nan")
    assert torch.equal(first, hip.attn_chunk_split(poisoned, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws[:need]))
    assert bool((ws[need:] == 0xA5).all())
    # the launcher on an output with rows to spare: only rows [0, B * R) are written
    HD = H * 128
    o = torch.full((B * R + 5, HD), 7.0, dtype=BF, device=dev)
    base = cache.data_ptr()
    hip.call("mla_attn_chunk_split", c_void_p(base), c_void_p(base + 2 * HD), c_void_p(base + 4 * HD), c_void_p(o.data_ptr()), B, H, 128, S_kv, R,
             cache.stride(1), cache.stride(0), HD, SCALE, splits, c_void_p(ws.data_ptr()), need)
    assert torch.equal(o[:B * R], first) and bool((o[B * R:] == 7.0).all())
    assert bool((ws[need:] == 0xA5).all())


def test_graph_replay_is_eager_also_after_the_cache_changes(dev):
    from mla_amd import hip
    B, H, R, S_kv, splits = 1, 2, 17, 565, 3
    cache = _cache(dev, B, H, S_kv, R)
    ws = torch.empty(hip.attn_split_ws_bytes(B, H, R, S_kv, splits), dtype=torch.uint8, device=dev)
    eager = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws)
    o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, eager)
    cache.copy_(_rand(tuple(cache.shape), 4242, 0.7, dev))
    g.replay()
    torch.cuda.synchronize()
    replayed = o.clone()
    again = hip.attn_chunk_split(cache, B, H, 128, S_kv, R, SCALE, splits=splits, ws=ws)
    assert torch.equal(replayed, again) and not torch.equal(again, eager)
    assert fro_rel(again, _attn_ref(cache, B, H, S_kv, R)) < 5e-3
