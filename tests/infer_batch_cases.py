"""Host-only helpers of tests/test_infer_batch_gpu.py (batched action sampling: mla_attn_chunk_ragged, mla_gemm_suffix_bf16): ragged
packed caches and an fp64 reference of the ragged suffix attention, in the convention of tests/attention_cases.py (head_dim 128, scale
1 / sqrt(128), q / k / v as [B, H, S, 128] tensors with bf16-exact values, `allowed` [B, Rq, S] bool masks). Nothing here touches the GPU;
tests/test_infer_batch_host.py checks it.

Ragged suffix attention: the packed q|k|v cache is [B, S_cap, 3 * H * 128]; sample b owns rows [0, kv_len[b]); its R queries are rows
[kv_len[b] - R, kv_len[b]); query r sees keys [0, kv_len[b] - R + r]. Rows at and behind kv_len[b] belong to nobody (the tests fill them
with NaN: a kernel that reads them fails)."""
import torch

from attention_cases import BF, D, SCALE


def ragged_allowed(kv_len, R, S_cap):
    """[B, R, S_cap] bool: query r of sample b sees keys [0, kv_len[b] - R + r]."""
    idx = torch.arange(S_cap)
    out = torch.zeros((len(kv_len), R, S_cap), dtype=torch.bool)
    for b, n in enumerate(kv_len):
        assert R <= n <= S_cap, (R, n, S_cap)
        out[b] = idx[None, :] <= (n - R + torch.arange(R))[:, None]
    return out


def make_ragged_cache(B, H, S_cap, kv_len, seed, scale=0.7, poison=True):
    """bf16 [B, S_cap, 3 * H * D] of randn * scale; rows >= kv_len[b] are NaN when `poison`."""
    g = torch.Generator().manual_seed(seed)
    cache = (torch.randn(B, S_cap, 3 * H * D, generator=g) * scale).to(BF)
    if poison:
        for b, n in enumerate(kv_len):
            cache[b, n:] = float("nan")
    return cache


def split_cache(cache, H):
    """packed [B, S, 3 * H * D] -> q, k, v as fp64 [B, H, S, D]."""
    B, S, _ = cache.shape
    return tuple(cache[:, :, i * H * D:(i + 1) * H * D].double().view(B, S, H, D).transpose(1, 2) for i in range(3))


def ragged_attn_r64(cache, kv_len, R, H):
    """fp64 reference of the ragged suffix attention -> o [B * R, H * D] (row b * R + r = query r of sample b)."""
    B, S_cap, _ = cache.shape
    q, k, v = split_cache(torch.nan_to_num(cache.float(), nan=0.0), H)      # rows nobody owns carry probability exactly 0
    allowed = ragged_allowed(kv_len, R, S_cap)
    out = torch.zeros((B, R, H * D), dtype=torch.float64)
    for b, n in enumerate(kv_len):
        qb = q[b, :, n - R:n]                                                 # [H, R, D]
        s = (qb @ k[b].transpose(-1, -2)) * SCALE                            # [H, R, S_cap]
        s = s.masked_fill(~allowed[b][None], float("-inf"))
        out[b] = (torch.softmax(s, -1) @ v[b]).transpose(0, 1).reshape(R, H * D)
    return out.reshape(B * R, H * D)
