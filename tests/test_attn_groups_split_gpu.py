"""GPU: mla_attn_groups_split (mla_amd/csrc/attn_split.hip) -- the split-key form of mla_attn_chunk_groups / mla_attn_chunk_ragged_groups
(and, with one group per sample, of mla_attn_chunk_ragged).

One split is the head form bit for bit. Every (sample, group) block with splits <= its own tile count is bit for bit mla_attn_chunk_split
(B = 1, the same splits) on cat(the sample's prefix rows, the group's rows); a block with fewer tiles than splits (its trailing ranges
write the empty state) keeps the bounds of tests/test_attn_split_gpu.py: fro_rel < 5e-3 against the fp32 reference and <= 2 x the head
form's own error on the same inputs. The result depends on nothing but a block's own key set, nothing outside the workspace bytes and the
B * G * R output rows is written, and one captured graph serves a new mix of lengths."""
import math
from ctypes import c_void_p

import pytest
import torch

from conftest import fro_rel
from test_inference_chunk_gpu import _attn_ref, _rand

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SCALE = 1 / math.sqrt(128)


def _block(cache_b, S_p, g, R):
    """[1, S_p + R, 3H]: what group g of a sample sees -- its prefix rows, then its own rows."""
    return torch.cat([cache_b[:S_p], cache_b[S_p + g * R:S_p + (g + 1) * R]], 0)[None].contiguous()


def _plain(dev, H, S_p, G, R, seed=0):
    return _rand((S_p + G * R + 3, 3 * H * 128), S_p * 100 + G * 10 + R + H + seed, 0.7, dev)     # 3 rows behind the last group


def _ragged(dev, B, H, S_cap, seed=0):
    return _rand((B, S_cap, 3 * H * 128), S_cap * 100 + B + H + seed, 0.7, dev)


def _lens(dev, values):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def _counts(BG, H, R, S_max):
    from mla_amd import hip
    nT = -(-S_max // 64)
    plan = hip.attn_split_plan(BG, H, R, S_max)[0]
    return sorted({s for s in (2, 3, nT, plan) if 1 < s <= nT}), plan


# ------------------------------------------------------------------------------------------------ one split: the head forms' bits
@pytest.mark.parametrize("R", [1, 9, 17, 64])
def test_one_split_is_attn_chunk_groups_bit_for_bit(dev, R):
    from mla_amd import hip
    H = 2
    for G in (1, 3, 5):
        for S_p in (0, 47, 128, 548):
            cache = _plain(dev, H, S_p, G, R)
            want = hip.attn_chunk_groups(cache, G, H, 128, S_p, R, SCALE)
            got = hip.attn_groups_split(cache, 1, G, H, 128, S_p, R, SCALE, splits=1)          # ws=None: no workspace is touched
            assert torch.equal(got, want), (G, R, S_p)


def test_one_split_is_the_ragged_head_forms_bit_for_bit(dev):
    from mla_amd import hip
    H, R = 2, 9
    B, G, S_cap = 3, 2, 320
    cache = _ragged(dev, B, H, S_cap)
    pl = _lens(dev, [250, 0, 131])
    want = hip.attn_chunk_ragged_groups(cache, B, G, H, 128, pl, R, SCALE)
    assert torch.equal(hip.attn_groups_split(cache, B, G, H, 128, pl, R, SCALE, splits=1), want)
    kv = _lens(dev, [259, 9, 140])                                            # one group per sample: mla_attn_chunk_ragged
    want1 = hip.attn_chunk_ragged(cache, B, H, 128, kv, R, SCALE)
    assert torch.equal(hip.attn_groups_split(cache, B, 1, H, 128, kv - R, R, SCALE, splits=1), want1)


# ------------------------------------------------------------------------------------------------ several splits: mla_attn_chunk_split's bits
SHAPES = [(100, 17, None), (128, 9, None), (66, 64, 3), (548, 2, None)]


@pytest.mark.parametrize("S_p,R,only", SHAPES, ids=[f"Sp{s}-R{r}" for s, r, _ in SHAPES])
def test_split_blocks_are_attn_chunk_split_bit_for_bit(dev, S_p, R, only):
    """(100, 17): a tile straddles the prefix / group boundary; (128, 9): the boundary sits on a tile edge; (66, 64, 3 splits): the last
    range lies behind most queries' causal limit; (548, 2): the sampler step's shape. Both addressing forms, splits in {2, 3, plan, nT}."""
    from mla_amd import hip
    H, G = 2, 3
    S_kv = S_p + R
    counts, plan = _counts(G, H, R, S_kv)
    if only is not None:
        assert only in counts
        counts = [only]
    assert counts
    cache = _plain(dev, H, S_p, G, R)
    B, S_cap = 2, S_p + G * R + 7
    rag = _ragged(dev, B, H, S_cap)
    pl = _lens(dev, [S_p, S_p])
    S_max = S_cap - (G - 1) * R
    for splits in counts + [None]:
        o = hip.attn_groups_split(cache, 1, G, H, 128, S_p, R, SCALE, splits=splits)
        assert o.shape == (G * R, H * 128)
        s_eff = plan if splits is None else splits
        if s_eff > 1:
            for g in range(G):
                want = hip.attn_chunk_split(_block(cache, S_p, g, R), 1, H, 128, S_kv, R, SCALE, splits=s_eff)
                assert torch.equal(o[g * R:(g + 1) * R], want), (splits, g)
        if splits is None or splits > -(-S_max // 64):
            continue
        o = hip.attn_groups_split(rag, B, G, H, 128, pl, R, SCALE, splits=splits)
        for b in range(B):
            for g in range(G):
                want = hip.attn_chunk_split(_block(rag[b], S_p, g, R), 1, H, 128, S_kv, R, SCALE, splits=splits)
                assert torch.equal(o[(b * G + g) * R:(b * G + g + 1) * R], want), (splits, b, g)


# ------------------------------------------------------------------------------------------------ ragged lengths
RB, RG, RH, RR, RCAP, RSPLITS = 3, 2, 2, 9, 320, 3
RLENS = [250, 10, 131]                                                        # tiles per group: 5, 1 (two empty ranges), 3


@pytest.fixture(scope="module")
def ragged_case(dev):
    from mla_amd import hip
    cache = _ragged(dev, RB, RH, RCAP)
    pl = _lens(dev, RLENS)
    need = hip.attn_split_ws_bytes(RB * RG, RH, RR, RCAP - (RG - 1) * RR, RSPLITS)
    assert need == RB * RG * RH * RR * RSPLITS * 130 * 4
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    first = hip.attn_groups_split(cache, RB, RG, RH, 128, pl, RR, SCALE, splits=RSPLITS, ws=ws[:need]).clone()
    return cache, pl, ws, need, first


def test_ragged_lengths_with_empty_ranges(dev, ragged_case):
    from mla_amd import hip
    cache, pl, ws, need, first = ragged_case
    head = hip.attn_chunk_ragged_groups(cache, RB, RG, RH, 128, pl, RR, SCALE)
    assert torch.isfinite(first.float()).all()
    for b, S_p in enumerate(RLENS):
        nT = -(-(S_p + RR) // 64)
        for g in range(RG):
            rows = slice((b * RG + g) * RR, (b * RG + g + 1) * RR)
            blk = _block(cache[b], S_p, g, RR)
            if RSPLITS <= nT:
                assert torch.equal(first[rows], hip.attn_chunk_split(blk, 1, RH, 128, S_p + RR, RR, SCALE, splits=RSPLITS)), (b, g)
            else:
                assert (b, nT) == (1, 1)
                ref = _attn_ref(blk, 1, RH, S_p + RR, RR)
                e_new, e_old = fro_rel(first[rows], ref), fro_rel(head[rows], ref)
                print(f"sample {b} group {g} (1 tile, 2 empty ranges): fro_rel {e_new:.3e}, head form {e_old:.3e}")
                assert e_new < 5e-3
                assert e_new <= 2 * e_old


def test_prefix_lengths_are_clamped_to_the_rows_the_caller_owns(dev, ragged_case):
    from mla_amd import hip
    cache, _, ws, need, _ = ragged_case
    got = hip.attn_groups_split(cache, RB, RG, RH, 128, _lens(dev, [-5, 10000, 131]), RR, SCALE, splits=RSPLITS, ws=ws[:need])
    want = hip.attn_groups_split(cache, RB, RG, RH, 128, _lens(dev, [0, RCAP - RG * RR, 131]), RR, SCALE, splits=RSPLITS, ws=ws[:need])
    assert torch.equal(got, want)
    assert bool((ws[need:] == 0xA5).all())


def test_isolation_and_determinism(dev, ragged_case):
    """A second call, a call on a workspace full of NaN and a call with NaN in every row behind a sample's groups give the same bits;
    new values in one group leave every other group's rows alone; the bytes behind ws_bytes and the rows of o outside B * G * R keep
    theirs; every sum word of every state is written."""
    from mla_amd import hip
    cache, pl, ws, need, first = ragged_case

    def run(c):
        return hip.attn_groups_split(c, RB, RG, RH, 128, pl, RR, SCALE, splits=RSPLITS, ws=ws[:need])

    assert torch.equal(first, run(cache))
    ws[:need].view(torch.float32).fill_(float("nan"))
    assert torch.equal(first, run(cache))
    assert torch.isfinite(ws[:need].view(torch.float32)[:RB * RG * RH * RR * RSPLITS * 128]).all()
    assert bool((ws[need:] == 0xA5).all())
    poisoned = cache.clone()
    for b, S_p in enumerate(RLENS):
        poisoned[b, S_p + RG * RR:] = float("nan")
    assert torch.equal(first, run(poisoned))
    for b, gp in ((0, 1), (1, 0), (2, 1)):                                    # re-randomise group gp of sample b
        changed = cache.clone()
        lo = RLENS[b] + gp * RR
        changed[b, lo:lo + RR] = _rand((RR, 3 * RH * 128), 999 + b, 0.7, dev)
        o = run(changed)
        own = slice((b * RG + gp) * RR, (b * RG + gp + 1) * RR)
        keep = torch.ones(RB * RG * RR, dtype=torch.bool, device=dev)
        keep[own] = False
        assert torch.equal(o[keep], first[keep]) and not torch.equal(o[own], first[own]), (b, gp)
    assert bool((ws[need:] == 0xA5).all())
    HD = RH * 128
    o = torch.full((RB * RG * RR + 5, HD), 7.0, dtype=BF, device=dev)
    base = cache.data_ptr()
    hip.call("mla_attn_groups_split", c_void_p(base), c_void_p(base + 2 * HD), c_void_p(base + 4 * HD), c_void_p(o.data_ptr()), RB, RG, RH, 128,
             c_void_p(pl.data_ptr()), RCAP, RR, cache.stride(1), cache.stride(0), HD, SCALE, RSPLITS, c_void_p(ws.data_ptr()), need)
    assert torch.equal(o[:RB * RG * RR], first) and bool((o[RB * RG * RR:] == 7.0).all())
    assert bool((ws[need:] == 0xA5).all())


def test_plain_form_ignores_the_rows_behind_the_last_group_and_other_groups(dev):
    from mla_amd import hip
    H, G, R, S_p, splits = 2, 3, 17, 100, 2
    cache = _plain(dev, H, S_p, G, R)
    first = hip.attn_groups_split(cache, 1, G, H, 128, S_p, R, SCALE, splits=splits)
    poisoned = cache.clone()
    poisoned[S_p + G * R:] = float("nan")
    assert torch.equal(first, hip.attn_groups_split(poisoned, 1, G, H, 128, S_p, R, SCALE, splits=splits))
    changed = cache.clone()
    changed[S_p + R:S_p + 2 * R] = _rand((R, 3 * H * 128), 4711, 0.7, dev)
    o = hip.attn_groups_split(changed, 1, G, H, 128, S_p, R, SCALE, splits=splits)
    assert torch.equal(o[:R], first[:R]) and torch.equal(o[2 * R:], first[2 * R:]) and not torch.equal(o[R:2 * R], first[R:2 * R])


# ------------------------------------------------------------------------------------------------ graph
def test_one_graph_serves_a_new_mix_of_lengths(dev):
    from mla_amd import hip
    cache = _ragged(dev, RB, RH, RCAP, seed=5)
    pl = _lens(dev, RLENS)
    ws = torch.empty(hip.attn_split_ws_bytes(RB * RG, RH, RR, RCAP - (RG - 1) * RR, RSPLITS), dtype=torch.uint8, device=dev)

    def run():
        return hip.attn_groups_split(cache, RB, RG, RH, 128, pl, RR, SCALE, splits=RSPLITS, ws=ws)

    eager = run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = run()
    o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, eager)
    pl.copy_(_lens(dev, [3, 302, 64]))
    cache.copy_(_ragged(dev, RB, RH, RCAP, seed=6))
    g.replay()
    torch.cuda.synchronize()
    replayed = o.clone()
    again = run()
    assert torch.equal(replayed, again) and not torch.equal(again, eager)
    assert torch.equal(hip.attn_groups_split(cache, RB, RG, RH, 128, pl, RR, SCALE, splits=1), hip.attn_chunk_ragged_groups(cache, RB, RG, RH, 128, pl, RR, SCALE))
    for b, S_p in enumerate([3, 302, 64]):
        for gi in range(RG):
            ref = _attn_ref(_block(cache[b], S_p, gi, RR), 1, RH, S_p + RR, RR)
            assert fro_rel(again[(b * RG + gi) * RR:(b * RG + gi + 1) * RR], ref) < 5e-3


# ------------------------------------------------------------------------------------------------ the 7B head count
def test_split_at_32_heads(dev):
    """B = 2, G = 1 and B = 1, G = 2 at R = 2, S_p = 545: the plan is 3, the plan's bits are splits=3's, and the bounds hold."""
    from mla_amd import hip
    H, R, S_p = 32, 2, 545
    S_kv = S_p + R
    cache = _plain(dev, H, S_p, 2, R)
    assert hip.attn_groups_split_plan(1, 2, H, R, S_p, False) == (S_kv, hip.attn_split_plan(2, H, R, S_kv))
    assert hip.attn_groups_split_plan(1, 2, H, R, S_p, False)[1][0] == 3
    o = hip.attn_groups_split(cache, 1, 2, H, 128, S_p, R, SCALE)
    assert torch.equal(o, hip.attn_groups_split(cache, 1, 2, H, 128, S_p, R, SCALE, splits=3))
    head = hip.attn_chunk_groups(cache, 2, H, 128, S_p, R, SCALE)
    for g in range(2):
        ref = _attn_ref(_block(cache, S_p, g, R), 1, H, S_kv, R)
        e_new, e_old = fro_rel(o[g * R:(g + 1) * R], ref), fro_rel(head[g * R:(g + 1) * R], ref)
        print(f"H 32 G 2 group {g}: fro_rel {e_new:.3e}, head form {e_old:.3e}")
        assert torch.isfinite(o.float()).all() and e_new < 5e-3 and e_new <= 2 * e_old
    rag = _ragged(dev, 2, H, S_kv)                                            # B = 2, G = 1: S_max = S_cap = 547
    pl = _lens(dev, [S_p, 300])
    assert hip.attn_groups_split_plan(2, 1, H, R, S_kv, True)[1][0] == 3
    o = hip.attn_groups_split(rag, 2, 1, H, 128, pl, R, SCALE)
    assert torch.equal(o, hip.attn_groups_split(rag, 2, 1, H, 128, pl, R, SCALE, splits=3))
    head = hip.attn_chunk_ragged(rag, 2, H, 128, pl + R, R, SCALE)
    for b, n in enumerate([S_p, 300]):
        ref = _attn_ref(_block(rag[b], n, 0, R), 1, H, n + R, R)
        e_new, e_old = fro_rel(o[b * R:(b + 1) * R], ref), fro_rel(head[b * R:(b + 1) * R], ref)
        print(f"H 32 B 2 sample {b}: fro_rel {e_new:.3e}, head form {e_old:.3e}")
        assert torch.isfinite(o.float()).all() and e_new < 5e-3 and e_new <= 2 * e_old
