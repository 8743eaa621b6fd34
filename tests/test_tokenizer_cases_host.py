"""CPU checks of tests/tokenizer_cases.py: the references and conditions tests/test_tokenizer_kernels_gpu.py holds the kernels to are
themselves checked here, against the oracle (oracle/torch_oracle.py) and against seeded wrong answers, and the fp32-vs-fp64 slack of
the lga_prep and batch-norm references is measured and printed (run with -s to see the figures)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tokenizer_cases as TC
from oracle import torch_oracle as TO

BF = torch.bfloat16


def _bf_exact(t):
    return torch.equal(t.float().to(BF).float(), t.float())


@pytest.mark.parametrize("cloud,N,G", [("uniform", 1024, 512), ("lattice16", 1000, 300), ("offset", 777, 100), ("planar", 257, 257)])
def test_fps_reference_equals_oracle(cloud, N, G):
    xyz = TC.make_cloud(cloud, 3, N)
    for kind in TC.FPS_STARTS:
        start = TC.fps_start(kind, 3, N)
        assert torch.equal(TC.fps_ref(xyz, G, start), TO.furthest_point_sample(xyz, G, start)), (cloud, kind)


def test_fps_reference_duplicates_repeat_lowest_index():
    """lattice16 at N = 1000 holds duplicate points: once every distinct point is taken all distances are 0 and the first maximum is
    index 0, for the rest of the selection."""
    xyz, start, ref = TC.fps_case("lattice16", 1000, "random")
    distinct = [len({tuple(p.tolist()) for p in xyz[b]}) for b in range(3)]
    assert all(d < 1000 for d in distinct)
    for b in range(3):
        assert bool((ref[b, distinct[b]:] == 0).all()) and len(set(ref[b, :distinct[b]].tolist())) == distinct[b]


@pytest.mark.parametrize("cloud,N,G", [("uniform", 1024, 512), ("lattice16", 1000, 300), ("offset", 777, 100), ("planar", 512, 100)])
def test_oracle_fp32_knn_lies_inside_the_band(cloud, N, G, capsys):
    xyz = TC.make_cloud(cloud, TC.KNN_B, N)
    centres, _ = TC.knn_centres(xyz, G)
    for k in (1, 33, 81, N):
        idx = TO.knn_point(k, xyz, centres)
        v = TC.knn_violations(idx, xyz, centres)
        share = TC.knn_match_share(idx, xyz, centres)
        with capsys.disabled():
            print(f"\nKNN-BAND {cloud:<10} N {N} G {G} k {k}: violations {v}  fp64 top-k set matched in {100 * share:.1f}% of groups")
        assert not any(v.values()), (cloud, k, v)


def test_knn_band_rejects_wrong_answers():
    xyz = TC.make_cloud("uniform", 1, 512)
    centres, _ = TC.knn_centres(xyz, 100)
    good = TC.knn_exact(xyz, centres, 33)
    assert not any(TC.knn_violations(good, xyz, centres).values())
    far = torch.from_numpy(np.argsort(TC.knn_d64(xyz, centres).numpy(), axis=-1)[..., -1])
    bad = good.clone(); bad[0, 5, 7] = far[0, 5]                                  # one far point in one group
    v = TC.knn_violations(bad, xyz, centres)
    assert v["chosen_far"] == 1 and v["unchosen_near"] == 1
    dup = good.clone(); dup[0, 3, 1] = dup[0, 3, 0]
    assert TC.knn_violations(dup, xyz, centres)["distinct"] > 0
    oob = good.clone(); oob[0, 0, 0] = 512
    assert TC.knn_violations(oob, xyz, centres)["range"] == 1
    nxt = torch.from_numpy(np.argsort(TC.knn_d64(xyz, centres).numpy(), axis=-1, kind="stable")[..., 33])
    off1 = good.clone(); off1[0, :, 32] = nxt[0]                                  # the (k+1)-th for the k-th: outside the band on uniform
    assert TC.knn_violations(off1, xyz, centres)["chosen_far"] > 90


@pytest.mark.parametrize("N", TC.KNN_N)
def test_lattice16_arithmetic_is_exact(N):
    xyz = TC.make_cloud("lattice16", TC.KNN_B, N)
    centres, _ = TC.knn_centres(xyz, 100)
    d32 = TO.square_distance(centres, xyz)
    assert d32.dtype == torch.float32 and torch.equal(d32.double(), TC.knn_d64(xyz, centres))
    # and the FPS distances
    d = xyz[:, :, None, :] - xyz[:, None, :64, :]
    assert torch.equal((d * d).sum(-1).double(), (d.double() ** 2).sum(-1))
    if N >= 512:                                                                 # ties are the point of the cloud
        d64 = TC.knn_d64(xyz, centres)
        assert int((d64.sort(-1).values.diff(dim=-1) == 0).sum()) > d64.shape[0] * d64.shape[1]


def test_inputs_are_bf16_exact_where_they_are_bf16():
    for C, K in TC.LGA_CK:
        assert _bf_exact(TC.lga_case("uniform", C, K)[1])
    for fam in ("zero_mean", "offset"):
        for t in TC.bn_inputs(2047, 96, fam):
            assert _bf_exact(t)
    x = TC.bn_inputs(2047, 96, "offset")[0].double()
    ratio = (x.mean(0).abs() / x.std(0).clamp(min=1e-30))[:-1]
    assert bool(((ratio[0::2] - 8).abs() < 1).all()) and bool(((ratio[1::2] - 64).abs() < 6).all())
    assert float(x[:, -1].var()) == 0.0
    assert _bf_exact(TC.ce_inputs("bf16", 1000, 1024)[0]) and not _bf_exact(TC.ce_inputs("fp32", 1000, 1024)[0])
    assert TC.pool_inputs(81, 27).dtype == BF and bool((TC.pool_inputs(81, 27)[:, ::3] < 0).all())


def test_lga_cases_select_both_kernels():
    """The dispatch condition of mla_lga_prep (pointcloud.hip): the 8-wide kernel needs fd = 2C / 6 a multiple of 8."""
    for C, K in TC.LGA_CK:
        assert (2 * C) % 6 == 0 and K <= 128 and K <= TC.LGA_N
        assert (((2 * C // 6) % 8 != 0) or C % 8 != 0) == ((C, K) in TC.LGA_SCALAR_CK)


def test_lga_reference_fp32_equals_the_oracle_composition_and_planar_closed_form():
    xyz, feats, fps_idx, knn_idx = TC.lga_case("planar", 24, 9)
    rows, lc = TC.lga_prep_ref(xyz, feats, fps_idx, knn_idx)
    assert torch.equal(lc.float(), TO.index_points(xyz, fps_idx))
    sl, exp = TC.planar_expected(xyz, feats, fps_idx, knn_idx)
    assert torch.equal(rows[:, sl].to(BF), exp)
    # the x / y channels are NOT feature + {0, 1}
    assert not torch.equal(rows[:, :sl.start].to(BF), TC.lga_prep_ref(xyz, feats, fps_idx, knn_idx, beta=0.0)[0][:, :sl.start].to(BF))


def test_measured_slack(capsys):
    lga, bn = TC.measured_slack("lga"), TC.measured_slack("bn")
    with capsys.disabled():
        print(f"\nSLACK lga_prep  max |fp32 ref - fp64 ref| = {lga:.3e}   (GPU test allows 2^-8 |ref| + 4 x this)")
        print(f"SLACK batchnorm max |fp32 ref - fp64 ref| = {bn:.3e}   (GPU test allows 2^-8 |ref| + 4 x this)")
    # fp32 evaluation of sin / cos at |argument| <= beta = 100: a handful of 2^-24 relative roundings of the argument
    assert 0 < lga < 100 * 2.0 ** -24 * 16
    assert 0 < bn < 1e-4


def test_offset_column_yardstick(capsys):
    """torch's own fp32 batch norm, rounded to bf16, against fp64 on the offset columns: the figure the kernel pair may double."""
    for rows in (2047, 6145):
        x, w, b, res = TC.bn_inputs(rows, 96, "offset")
        ref = TC.bn_ref(x, w, b)
        y = TC.bn_torch32(x, w, b).double()
        e = (y - ref).abs()[:, :-1]
        with capsys.disabled():
            print(f"\nBN-OFFSET yardstick rows {rows}: max |err| {float(e.max()):.3e}  fro {TC.fro(y[:, :-1], ref[:, :-1]):.3e}")
        assert float(e.max()) < 2.0 ** -7 * float(ref.abs().max())


def test_vision_references():
    g = torch.Generator().manual_seed(1)
    pix = torch.randn(2, 4, 28, 42, generator=g)
    wt = torch.randn(5, 3, 14, 14, generator=g)
    rows = TC.im2col_ref(pix.to(BF), 14, 640)
    assert rows.shape == (2 * 2 * 3, 640) and bool((rows[:, 588:] == 0).all())
    conv = F.conv2d(pix[:, :3].to(BF).double(), wt.double(), stride=14).permute(0, 2, 3, 1).reshape(-1, 5)
    assert torch.allclose(rows[:, :588].double() @ wt.double().reshape(5, -1).t(), conv, atol=1e-9)
    x = torch.randn(2 * 6 * 4, 16, generator=g).to(BF)
    assert torch.equal(TC.avgpool_ref(x, 2, 6, 4, 1), x.double())
    # window attention: against the oracle's formulation (q * C^-0.5 * k).sum(-1).softmax, one window at a time
    B, gh, gw, cs, C = 2, 4, 6, 2, 256
    q, kv, do = TC.attn_inputs(B, gh, gw, C, cs)
    out, dq, dkv = TC.local_attn_ref(q, kv, do, B, gh, gw, cs, C ** -0.5)
    kvw = TC.window_rows(kv.double(), B, gh, gw, cs).view(-1, cs * cs, 2, TC.HEADS, C // TC.HEADS)
    qh = q.double().view(-1, 1, TC.HEADS, C // TC.HEADS)
    attn = (qh * C ** -0.5 * kvw[:, :, 0]).sum(-1).softmax(dim=1)
    assert torch.allclose((attn.unsqueeze(-1) * kvw[:, :, 1]).sum(1).reshape(-1, C), out, atol=1e-12)
    assert dq.shape == q.shape and dkv.shape == kv.shape
    a = torch.zeros(3, 4); r = torch.zeros(3, 4); r[1, 2] = 2.0; a[1, 2] = 2.5
    assert TC.per_window_max_rel(a, r) == (0.25, 1)
    a[0, 0] = 1e-9
    assert TC.per_window_max_rel(a, r)[0] == float("inf")


def test_ce_reference_and_grid_sizes():
    logits, labels = TC.ce_inputs("fp32", 1000, 1024)
    d = TC.ce_bwd_ref(logits, labels, 1000, 0.25, 2.0)
    assert bool((d[[1, 4, 6]] == 0).all()) and abs(float(d[0].sum())) < 1e-5 and float(d[0, 0]) < 0
    assert TC.BN_BIG_ROWS == 172037 and TC.BN_BIG_ROWS * 96 * 2 < 35e6
    assert 3 * 48 * 48 * 640 > 16384 * 256
    assert [TC.grid_for((6, 12), cs) for cs in TC.ATTN_CS] == [(6, 12), (6, 12), (6, 12), (4, 12)]
