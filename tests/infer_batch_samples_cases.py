"""Shared cases and CPU statements for the tests of N action chunks for each of B observations (mla_attn_chunk_ragged_groups,
mla_gemm_suffix_bf16_pos / _w8_pos, mla_amd/infer.py:BatchedSampleGroupsEps, MLA.predict_action_diff_batch(num_samples=N)). Plain module:
imported by test_infer_batch_samples_host.py (CPU) and test_infer_batch_samples_gpu.py.

Cache layout [B, S_cap, 3 H D]: in sample b rows [0, S_p[b]) are the prefix, row S_p[b] + g * R + p is suffix row p of group g, rows behind
S_p[b] + G * R are never read. Query (b, g, p) sees the logical keys 0 .. S_p[b] + p of its sample (infer_samples_cases.key_rows)."""
import torch

import infer_samples_cases as isc

# prefix length mixes (B = 3) on both sides of the 64-key tile edges -- the shared / per-group tile boundary moves per sample -- and
# across the wave rotation (tile t on wave t % 4: 255 / 256 / 257 is the fourth tile's edge; 545 runs every wave more than twice)
PREFIX_MIXES = [(63, 64, 65), (0, 1, 130), (47, 200, 545), (255, 256, 257)]
# (G, R): one group; three groups of the default chunk; tiny groups; R = 64 (four query blocks); R = 1; G = 4 (a whole GW = 4 workgroup)
GROUP_SHAPES = [(1, 17), (3, 17), (5, 2), (2, 64), (7, 1), (4, 5)]
H3_CASE = ((63, 64, 65), (3, 17))                       # also run with 3 heads
ISOLATION_SHAPES = [(3, 17), (4, 5)]
# (G, R, nheads, K) of the projection tests with B = 3 samples: 153 rows (10 row blocks, two heads), 30 rows (one W tile per workgroup),
# 255 rows (the (2, 16) form filled to its last block)
PROJECTION_S_P = (29, 7, 40)
PROJECTION_CASES = [(3, 17, 2, 512), (2, 5, 1, 512), (5, 17, 1, 512)]


def s_cap(S_p, G, R, bucket=64):
    return -(-(max(S_p) + G * R) // bucket) * bucket


def layout(S_p, G, R, S_cap):
    """-> (prefix_len [B], slot [B * G], rope_pos [B * G]): the engine's addressing, s = b * G + g."""
    slot = [b * S_cap + S_p[b] + g * R for b in range(len(S_p)) for g in range(G)]
    rope_pos = [S_p[b] for b in range(len(S_p)) for g in range(G)]
    return list(S_p), slot, rope_pos


def attn_ref(cache, S_p, G, H, R):
    """fp32 reference on [B, S_cap, 3 H D] -> [B * G * R, H D], row (b * G + g) * R + p: infer_samples_cases.attn_ref per sample."""
    return torch.cat([isc.attn_ref(cache[b, :S_p[b] + G * R], G, H, S_p[b], R) for b in range(len(S_p))], dim=0)


def hostile(cache, S_p, G, R, b, g):
    """The cache with every row outside prefix_b and group (b, g) set to NaN: other groups, other samples, sample b's tail rows."""
    out = torch.full_like(cache, float("nan"))
    out[b, :S_p[b]] = cache[b, :S_p[b]]
    lo = S_p[b] + g * R
    out[b, lo:lo + R] = cache[b, lo:lo + R]
    return out
