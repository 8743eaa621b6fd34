"""Shared cases and CPU statements for the tests of N action chunks per observation on one cached prefix (mla_attn_chunk_groups,
mla_amd/infer.py:SampleGroupsEps, MLA.predict_action_diff_samples). Plain module: imported by test_infer_samples_host.py (CPU) and
test_infer_samples_gpu.py.

Cache layout of ONE sample: rows [0, S_p) the prefix, row S_p + g * R + p suffix row p of group g. Query (g, p) sees the logical keys
0 .. S_p + p; logical key j is memory row j (j < S_p) or j + g * R."""
import math

import torch

# (G, R, S_p): one group at the 7B prefix length; S_p just below / on / above a 64-key tile (the shared / per-group tile boundary); a
# prefix of two whole tiles + 2 with tiny groups; S_p + R = 64 exactly (one tile, nothing shared) with 15 groups (odd for GW = 2, 4);
# R = 64 (four query blocks) behind a one-row prefix; R = 1; more than 16 tiles (every wave runs several iterations of shared tiles);
# no prefix at all.
KERNEL_CASES = [(1, 17, 545), (3, 17, 63), (3, 17, 64), (3, 17, 65), (5, 2, 130), (15, 17, 47), (4, 64, 1), (7, 1, 200), (5, 5, 1030),
                (6, 9, 0)]
H3_CASE = (3, 17, 65)                                    # also run with 3 heads
ISOLATION_CASES = [(3, 17, 65), (5, 2, 130)]
PROJECTION_CASES = [(3, 17, 2, 512), (15, 17, 1, 512)]   # (G, R, nheads, K)


def key_rows(g, p, R, S_p):
    """Memory rows of the keys query (g, p) sees, in logical order."""
    return [j if j < S_p else j + g * R for j in range(S_p + p + 1)]


def gather_group(cache, g, R, S_p):
    """[prefix | group g] of a [S_p + G * R, C] cache -> [S_p + R, C]: the cache a batch-1 call on group g alone would hold."""
    return torch.cat([cache[:S_p], cache[S_p + g * R:S_p + (g + 1) * R]], dim=0)


def attn_ref(cache, G, H, S_p, R, D=128):
    """fp32 reference on the packed q|k|v cache [S_p + G * R, 3 H D] -> [G * R, H D]; every query's key set is key_rows()."""
    c = cache.float()
    out = []
    for g in range(G):
        cg = gather_group(c, g, R, S_p)
        S_kv = S_p + R
        q = cg[S_p:, :H * D].view(R, H, D).transpose(0, 1)
        k = cg[:, H * D:2 * H * D].view(S_kv, H, D).transpose(0, 1)
        v = cg[:, 2 * H * D:3 * H * D].view(S_kv, H, D).transpose(0, 1)
        s = q @ k.transpose(-1, -2) / math.sqrt(D)
        mask = torch.arange(S_kv, device=c.device)[None, :] > (S_p + torch.arange(R, device=c.device))[:, None]
        s = s.masked_fill(mask, float("-inf"))
        out.append((torch.softmax(s, -1) @ v).transpose(0, 1).reshape(R, H * D))
    return torch.cat(out, dim=0)
