"""CPU: the host side of N action chunks per observation on one cached prefix -- plan_sample_groups, the logical-key -> memory-row map
the kernel tests rest on, and mla_attn_chunk_groups' argument validation (on the host, before any launch: safe without a GPU)."""
import ctypes

import pytest
import torch

import infer_samples_cases as isc


def _check_plan(N, R, max_rows):
    from mla_amd.infer import plan_sample_groups
    passes = plan_sample_groups(N, R, max_rows)
    per = max_rows // R
    assert passes[0][0] == 0 and passes[-1][1] == N
    for (a, b), nxt in zip(passes, passes[1:] + [None]):
        assert 1 <= b - a <= per
        if nxt is not None:
            assert nxt[0] == b and b - a == per                              # consecutive, no overlap, only the last pass is short
    return passes


def test_plan_sample_groups_covers_the_samples_in_order():
    for R in (1, 2, 5, 17, 33, 64):
        per = 256 // R
        for N in (1, 2, per - 1, per, per + 1, 2 * per, 2 * per + 1, 100):
            if N >= 1:
                _check_plan(N, R, 256)
    assert _check_plan(1, 17, 256) == [(0, 1)]
    assert _check_plan(15, 17, 256) == [(0, 15)]                             # N = G_max
    assert _check_plan(16, 17, 256) == [(0, 15), (15, 16)]                   # N = G_max + 1
    assert _check_plan(9, 64, 256) == [(0, 4), (4, 8), (8, 9)]               # R = 64: G_max = 4
    assert _check_plan(5, 17, 34) == [(0, 2), (2, 4), (4, 5)]


def test_plan_sample_groups_rejects_bad_arguments():
    from mla_amd.infer import plan_sample_groups
    for n in (0, -3):
        with pytest.raises(ValueError):
            plan_sample_groups(n, 17, 256)
    with pytest.raises(ValueError):
        plan_sample_groups(2, 65, 64)                                        # a group does not fit a pass


@pytest.mark.parametrize("G,R,S_p", isc.KERNEL_CASES)
def test_key_map_is_prefix_plus_own_group(G, R, S_p):
    for g in range(G):
        for p in range(R):
            rows = isc.key_rows(g, p, R, S_p)
            assert rows == list(range(S_p)) + list(range(S_p + g * R, S_p + g * R + p + 1))
            assert max(rows) < S_p + G * R
    cache = torch.arange((S_p + G * R) * 2).view(S_p + G * R, 2)
    for g in range(G):
        got = isc.gather_group(cache, g, R, S_p)
        assert got.shape[0] == S_p + R
        for p in range(R):                                                   # the gathered cache holds query (g, p)'s keys as rows 0 .. S_p + p
            assert got[:S_p + p + 1, 0].tolist() == [2 * r for r in isc.key_rows(g, p, R, S_p)]


def test_attn_ref_ignores_other_groups():
    """The fp32 reference is a statement about [prefix | own group] only."""
    G, R, S_p, H = 3, 4, 5, 1
    cache = torch.randn(S_p + G * R, 3 * H * 128, generator=torch.Generator().manual_seed(0))
    ref = isc.attn_ref(cache, G, H, S_p, R)
    other = cache.clone()
    other[S_p + R:S_p + 2 * R] = 1e4                                         # group 1
    ref2 = isc.attn_ref(other, G, H, S_p, R)
    assert torch.equal(ref[:R], ref2[:R]) and torch.equal(ref[2 * R:], ref2[2 * R:]) and not torch.equal(ref[R:2 * R], ref2[R:2 * R])
    rows = isc.key_rows(2, 1, R, S_p)                                        # query (2, 1) by hand over its key rows
    w = torch.softmax(cache[S_p + 2 * R + 1, :128] @ cache[rows, 128:256].t() / 128 ** 0.5, -1)
    assert torch.allclose(ref[2 * R + 1], w @ cache[rows, 256:], atol=1e-5)


def test_attn_chunk_groups_validates_on_the_host():
    from mla_amd import hip
    lib = hip.lib()
    P = ctypes.c_void_p(16)

    def rc(G=3, H=2, head_dim=128, S_p=65, R=17, ld=768, ld_o=256, p=P):
        return lib.mla_attn_chunk_groups(p, P, P, P, G, H, head_dim, S_p, R, ld, ld_o, 0.1, None)
    assert rc(head_dim=64) < 0 and b"head_dim must be 128" in lib.mla_last_error(), lib.mla_last_error()
    assert rc(R=65) < 0 and b"1 <= R <= 64" in lib.mla_last_error(), lib.mla_last_error()
    assert rc(R=0) < 0 and rc(G=0) < 0 and b"G >= 1" in lib.mla_last_error(), lib.mla_last_error()
    assert rc(S_p=-1) < 0
    assert rc(p=None) < 0 and b"null pointer" in lib.mla_last_error()
    assert rc(ld=770) < 0 and b"16-B aligned" in lib.mla_last_error()
    assert rc(p=ctypes.c_void_p(18)) < 0 and b"16-B aligned" in lib.mla_last_error()
    assert lib.mla_attn_chunk_groups_gw(P, P, P, P, 3, 2, 128, 65, 17, 768, 256, 0.1, 3, -1, None) < 0 and b"groups per workgroup" in lib.mla_last_error()
    assert lib.mla_attn_chunk_groups_gw(P, P, P, P, 3, 2, 128, 65, 17, 768, 256, 0.1, 2, 2, None) < 0 and b"order must be" in lib.mla_last_error()
