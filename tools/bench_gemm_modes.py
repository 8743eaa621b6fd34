"""gemm256 on reduction-major operands (ds_read_b64_tr_b16 fragments, untracked LDS-DMA staging) against the all-NT formulation it
would replace (k-contiguous operands + the explicit transposes that make them). Decoder-layer backward shapes, random data.
Usage: python tools/bench_gemm_modes.py [tokens]
       python tools/bench_gemm_modes.py pairs [tokens]    per wgrad GEMM of a decoder layer: the reduction-major assembly launch on row-major
           dY and X against the k-contiguous launch plus what that GEMM's transposed copies cost today, alternating on one GPU
           (medians of 7 rounds); then one decision line per dgrad (B as stored against NT + its W^T pass, the fused d(act) launch as
           <0,1,2> against <0,0,2> + its transpose), the attention backward with / without its transposed outputs and what wqkv / wo /
           wgu = 1 gain from them and from the kept normalised inputs; -> profiles/backward_as_stored_gemm_pairs.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mla_amd import hip

PAIRS = len(sys.argv) > 1 and sys.argv[1] == "pairs"      # the per-GEMM decision table of the MLA_WGRAD_RM switch (below)
if PAIRS:
    del sys.argv[1]
T = int(sys.argv[1]) if len(sys.argv) > 1 else 17536
dev = torch.device("cuda:0")
H, I = 4096, 11008


def timeit(fn, iters=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def alternating(fns, rounds=7, iters=4):
    """Median ms per call of every fn, measured round-robin so that clock / temperature drift hits all of them alike."""
    for f in fns.values():
        f()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                f()
            e.record()
            torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e) / iters)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def pairs():
    print(f"wgrad pairs at T = {T}: dW[Nout, Kin] (fp32, accumulate) = dY^T X. NT = k-contiguous launch on dY^T, X^T; RM = (1, 1) on row-major "
          f"dY, X: asm = generated main loop, cc = compiler-scheduled loop; (1, 0) / (0, 1) = one side as stored. ms, medians of 7 alternating rounds")
    rows = {}
    for name, nout, kin in (("wd", H, I), ("wg|wu", 2 * I, H), ("wo", H, H), ("wq|wk|wv", 3 * H, H)):
        dy, x = rnd(T, nout), rnd(T, kin)
        dyt, xt = hip.transpose(dy), hip.transpose(x)
        out = torch.zeros(nout, kin, dtype=torch.float32, device=dev)

        def rm(am, bm, loop):
            def f():
                hip.gemm_kloop(loop)
                hip.gemm(dy if am else dyt, x if bm else xt, out=out, a_mode=am, b_mode=bm, accumulate=True)
                hip.gemm_kloop(1)
            return f
        r = alternating({"nt": lambda: hip.gemm(dyt, xt, out=out, accumulate=True), "rm_asm": rm(1, 1, 1), "rm_cc": rm(1, 1, 0),
                         "a_rm": rm(1, 0, 1), "b_rm": rm(0, 1, 1), "dyT": lambda: hip.transpose(dy), "xT": lambda: hip.transpose(x)})
        rows[name] = r
        fl = 2.0 * T * nout * kin / 1e9
        print(f"  {name:9s} NT {r['nt']:6.3f} ({fl / r['nt']:5.0f} TF/s) | RM asm {r['rm_asm']:6.3f} ({fl / r['rm_asm']:5.0f} TF/s, {100 * (r['rm_asm'] / r['nt'] - 1):+5.1f} %)"
              f" | RM cc {r['rm_cc']:6.3f} ({100 * (r['rm_cc'] / r['nt'] - 1):+5.1f} %) | (1,0) {r['a_rm']:6.3f} ({100 * (r['a_rm'] / r['nt'] - 1):+5.1f} %)"
              f" | (0,1) {r['b_rm']:6.3f} ({100 * (r['b_rm'] / r['nt'] - 1):+5.1f} %) | tile_transpose dY {r['dyT']:6.3f}, X {r['xT']:6.3f}", flush=True)
        del dy, x, dyt, xt, out
    print("producer epilogues with and without their transposed output (the copy's price where no stand-alone transpose makes it)")
    x, wgu = rnd(T, H), rnd(2 * I, H, scale=0.02)
    r = alternating({"t": lambda: hip.gemm_gateup_swiglu(x, wgu, True), "n": lambda: hip.gemm_gateup_swiglu(x, wgu, False)})
    print(f"  gate|up + SwiGLU (<0,0,1>): with act^T {r['t']:6.3f} | without {r['n']:6.3f} | act^T costs {1e3 * (r['t'] - r['n']):6.1f} us", flush=True)
    act_t = 1e3 * (r["t"] - r["n"])
    dy, wdT, gu = rnd(T, H), rnd(I, H, scale=0.02), rnd(T, 2 * I)
    r = alternating({"t": lambda: hip.gemm_dact_swiglu_bwd(dy, wdT, gu), "n": lambda: hip.gemm_dact_swiglu_bwd(dy, wdT, gu, want_t=False)})
    print(f"  d(act) + SwiGLU bwd (<0,0,2>): with dgu^T {r['t']:6.3f} | without {r['n']:6.3f} | dgu^T costs {1e3 * (r['t'] - r['n']):6.1f} us", flush=True)
    dgu_t = 1e3 * (r["t"] - r["n"])
    del x, wgu, dy, wdT, gu
    # decision: RM asm against NT + today's copies of that GEMM. wd: tile_transpose(d2) + act^T from <0,0,1>; wg|wu: dgu^T from <0,0,2>
    # (xn2^T comes from rmsnorm_apply_t, the same bytes as the row-major re-application: no saving counted); wo: tile_transpose(dh1)
    # (o^T comes out of the attention backward, +123 us per layer together with dqkv^T by DESIGN 3.2, NOT measured here: credited to
    # neither so that a win does not rest on it); wq|wk|wv: nothing measured here (dqkv^T as for wo, xn1^T as xn2^T)
    # two candidates per GEMM: "1" = dy and x as stored (every copy above goes), "a" = dy as stored and x^T kept (only dy's copy goes:
    # tile_transpose(d2), dgu^T, tile_transpose(dh1); act^T stays for wd). The setting with the lower net is the one MLA_WGRAD_RM ships.
    print("decision per GEMM: launch penalty against the measured price of the copies that setting removes (us per layer; negative net wins)")
    c11 = {"wd": 1e3 * rows["wd"]["dyT"] + act_t, "wg|wu": dgu_t, "wo": 1e3 * rows["wo"]["dyT"], "wq|wk|wv": 0.0}
    c10 = {"wd": 1e3 * rows["wd"]["dyT"], "wg|wu": dgu_t, "wo": 1e3 * rows["wo"]["dyT"], "wq|wk|wv": 0.0}
    for name, r in rows.items():
        n11, n10 = 1e3 * (r["rm_asm"] - r["nt"]) - c11[name], 1e3 * (r["a_rm"] - r["nt"]) - c10[name]
        pick = "0" if min(n11, n10) >= 0 else "1" if n11 <= n10 else "a"
        print(f"  {name:9s} '1' (1,1): penalty {1e3 * (r['rm_asm'] - r['nt']):+7.1f} - copies {c11[name]:6.1f} = net {n11:+7.1f} us | "
              f"'a' (1,0): penalty {1e3 * (r['a_rm'] - r['nt']):+7.1f} - copies {c10[name]:6.1f} = net {n10:+7.1f} us -> {pick}", flush=True)
    print("dgrad shapes, B as stored (b_mode 1, generated main loop) against NT on W^T")
    drows = {}
    for name, nout, kin in (("qkv", 3 * H, H), ("o", H, H), ("gate|up", 2 * I, H), ("down", H, I)):
        dy, w = rnd(T, nout), rnd(nout, kin, scale=0.02)
        wt = hip.transpose(w)
        o = torch.empty(T, kin, dtype=torch.bfloat16, device=dev)
        r = alternating({"nt": lambda: hip.gemm(dy, wt, out=o), "nn": lambda: hip.gemm(dy, w, out=o, b_mode=1), "wT": lambda: hip.transpose(w)})
        fl = 2.0 * T * nout * kin / 1e9
        print(f"  {name:8s} NT {r['nt']:6.3f} ({fl / r['nt']:5.0f} TF/s) | (0,1) {r['nn']:6.3f} ({fl / r['nn']:5.0f} TF/s, {100 * (r['nn'] / r['nt'] - 1):+5.1f} %) | W^T {r['wT']:6.3f}", flush=True)
        drows[name] = r
        del dy, w, wt, o
    # the fused d(act) + SwiGLU-backward launch: <0,1,2> on W_down [H, I] as stored against <0,0,2> on W^T + the tile transpose that makes it
    # (row-major d(gate|up) only, as the wg|wu wgrad reads it today; and with the transposed strip)
    dy, w, gu = rnd(T, H), rnd(H, I, scale=0.02), rnd(T, 2 * I)
    wt = hip.transpose(w)
    r = alternating({"nt": lambda: hip.gemm_dact_swiglu_bwd(dy, wt, gu, want_t=False), "nn": lambda: hip.gemm_dact_swiglu_bwd_rm(dy, w, gu, want_t=False),
                     "nt_t": lambda: hip.gemm_dact_swiglu_bwd(dy, wt, gu), "nn_t": lambda: hip.gemm_dact_swiglu_bwd_rm(dy, w, gu),
                     "wT": lambda: hip.transpose(w)})
    fl = 2.0 * T * H * I / 1e9
    print(f"  down+bwd <0,0,2> {r['nt']:6.3f} ({fl / r['nt']:5.0f} TF/s) | <0,1,2> {r['nn']:6.3f} ({fl / r['nn']:5.0f} TF/s, {100 * (r['nn'] / r['nt'] - 1):+5.1f} %)"
          f" | with dgu^T: <0,0,2> {r['nt_t']:6.3f} | <0,1,2> {r['nn_t']:6.3f} ({100 * (r['nn_t'] / r['nt_t'] - 1):+5.1f} %) | W^T {r['wT']:6.3f}", flush=True)
    drows["down+bwd"] = r
    del dy, w, gu, wt
    print("decision per dgrad (MLA_DGRAD_RM): launch penalty of B as stored against the W^T pass it removes (us per layer; negative net wins)")
    for key, name in (("dqkv", "qkv"), ("do", "o"), ("dgu", "gate|up"), ("dd", "down+bwd"), ("dd (plain)", "down")):
        r = drows[name]
        pen, copy = 1e3 * (r["nn"] - r["nt"]), 1e3 * r["wT"]
        print(f"  {key:10s} penalty {pen:+7.1f} - W^T {copy:6.1f} = net {pen - copy:+7.1f} us -> {'1' if pen - copy < 0 else '0'}", flush=True)
    # the attention backward with and without its transposed outputs (dqkv^T, o^T): what wqkv = 1 and wo = 1 together remove
    nh, D, Bq = H // 128, 128, 32
    Sq = T // Bq
    if Sq * Bq == T and Sq % 4 == 0:
        qkv = rnd(T, 3 * H, scale=0.5)
        q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
        sc = D ** -0.5
        o, lse = hip.attn_fwd(q, k, v, Bq, Sq, nh, D, 3 * H, None, sc)
        do, dqkv = rnd(T, H), torch.empty_like(qkv)
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev).float() / D))
        ang = torch.outer(torch.arange(Sq, device=dev).float(), inv)
        cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
        tr = (torch.empty(3 * H, T, dtype=torch.bfloat16, device=dev), torch.empty(H, T, dtype=torch.bfloat16, device=dev))

        def bwd(t):
            return lambda: hip.attn_bwd(q, k, v, o, do, lse, None, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], Bq, Sq, nh, D, 3 * H, sc,
                                        rope_cos=cos, rope_sin=sin, transposed=t)
        r = alternating({"t": bwd(tr), "n": bwd(None)})
        tcost = 1e3 * (r["t"] - r["n"])
        print(f"attention backward (B = {Bq}, S = {Sq}): with dqkv^T, o^T {r['t']:6.3f} | without {r['n']:6.3f} | the transposed outputs cost {tcost:6.1f} us", flush=True)
        del qkv, o, do, dqkv, tr
        # level 1 keeps xn1 / xn2 row-major when wqkv / wgu = 1: the rmsnorm_apply_t pass that rebuilt x^T goes as well
        h, g = rnd(T, H), rnd(H)
        _, rstd = hip.rmsnorm_fwd(h, g, 1e-5)
        napply = 1e3 * alternating({"t": lambda: hip.rmsnorm_apply_t(h, g, rstd)})["t"]
        pq, po, pg = rows["wq|wk|wv"], rows["wo"], rows["wg|wu"]
        pen = 1e3 * ((pq["rm_asm"] - pq["nt"]) + (po["rm_asm"] - po["a_rm"]))
        net = pen - tcost - napply
        print(f"  wqkv 0 -> 1 and wo a -> 1 (no dqkv^T / o^T, xn1 kept): launch penalty {pen:+7.1f} - transposed outputs {tcost:6.1f} - rmsnorm_apply_t {napply:6.1f}"
              f" = net {net:+7.1f} us -> {'wqkv=1,wo=1' if net < 0 else 'wqkv=0,wo=a'}", flush=True)
        pen = 1e3 * (pg["rm_asm"] - pg["a_rm"])
        print(f"  wgu a -> 1 (xn2 kept): launch penalty {pen:+7.1f} - rmsnorm_apply_t {napply:6.1f} = net {pen - napply:+7.1f} us -> {'wgu=1' if pen - napply < 0 else 'wgu=a'}", flush=True)


if PAIRS:
    pairs()
    sys.exit(0)

print("dgrad  dX[T, Kin] = dY[T, Nout] W[Nout, Kin]:  NT needs W^T (transpose pass), NN reads W as stored (b_mode 1)")
for name, nout, kin in (("qkv", 3 * H, H), ("o", H, H), ("gate|up", 2 * I, H), ("down", H, I)):
    dy, w = rnd(T, nout), rnd(nout, kin, scale=0.02)
    out_nt, out_nn = torch.empty(T, kin, dtype=torch.bfloat16, device=dev), torch.empty(T, kin, dtype=torch.bfloat16, device=dev)
    wt = hip.transpose(w)
    t_tr = timeit(lambda: hip.transpose(w))
    t_nt = timeit(lambda: hip.gemm(dy, wt, out=out_nt))
    t_nn = timeit(lambda: hip.gemm(dy, w, out=out_nn, b_mode=1))
    err = float((out_nn.float() - out_nt.float()).abs().max() / out_nt.float().abs().max())
    fl = 2.0 * T * nout * kin
    print(f"  {name:8s} NT {t_nt:7.3f} ms ({fl / t_nt / 1e9:6.0f} TF/s) + W^T {t_tr:6.3f} ms | NN {t_nn:7.3f} ms ({fl / t_nn / 1e9:6.0f} TF/s) | "
          f"NN - (NT + W^T) = {(t_nn - t_nt - t_tr) * 1e3:7.1f} us   max rel diff {err:.1e}", flush=True)

print("wgrad  dW[Nout, Kin] = dY[T, Nout]^T X[T, Kin]:  NT needs dY^T and X^T, TN reads both as stored (a_mode 1, b_mode 1)")
for name, nout, kin in (("qkv", 3 * H, H), ("o", H, H), ("gate|up", 2 * I, H), ("down", H, I)):
    dy, x = rnd(T, nout), rnd(T, kin)
    dyt, xt = hip.transpose(dy), hip.transpose(x)
    out_nt, out_tn = torch.empty(nout, kin, dtype=torch.float32, device=dev), torch.empty(nout, kin, dtype=torch.float32, device=dev)
    t_tr = timeit(lambda: (hip.transpose(dy), hip.transpose(x)))
    t_nt = timeit(lambda: hip.gemm(dyt, xt, out=out_nt))
    t_tn = timeit(lambda: hip.gemm(dy, x, out=out_tn, a_mode=1, b_mode=1))
    err = float((out_tn - out_nt).abs().max() / out_nt.abs().max())
    fl = 2.0 * T * nout * kin
    print(f"  {name:8s} NT {t_nt:7.3f} ms ({fl / t_nt / 1e9:6.0f} TF/s) + dY^T, X^T {t_tr:6.3f} ms | TN {t_tn:7.3f} ms ({fl / t_tn / 1e9:6.0f} TF/s) | "
          f"TN - NT = {(t_tn - t_nt) * 1e3:7.1f} us   max rel diff {err:.1e}", flush=True)

print("reduction-major operands: gemm256 (force_generic 3) vs gemm128 (force_generic 2)")
for name, M, N, K, am, bm in (("qkv wgrad TN", 3 * H, H, T, 1, 1), ("down dgrad NN", T, I, H, 0, 1), ("o dgrad NN", T, H, H, 0, 1),
                              ("heads 8192 NN", 4096, 8192, 4096, 0, 1), ("heads TN", 8192, 4096, 4096, 1, 1)):
    a = rnd(*((M, K) if am == 0 else (K, M)))
    b = rnd(*((N, K) if bm == 0 else (K, N)))
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    t3 = timeit(lambda: hip.gemm(a, b, out=out, a_mode=am, b_mode=bm, force_generic=3))
    t2 = timeit(lambda: hip.gemm(a, b, out=out, a_mode=am, b_mode=bm, force_generic=2))
    fl = 2.0 * M * N * K
    print(f"  {name:14s} gemm256 {t3:7.3f} ms ({fl / t3 / 1e9:6.0f} TF/s) | gemm128 {t2:7.3f} ms ({fl / t2 / 1e9:6.0f} TF/s)", flush=True)

print("wgrad with ONE reduction-major operand (the other one k-contiguous, as the producers' fused transposed outputs provide it)")
for name, nout, kin in (("qkv", 3 * H, H), ("o", H, H), ("gate|up", 2 * I, H), ("down", H, I)):
    dy, x = rnd(T, nout), rnd(T, kin)
    dyt, xt = hip.transpose(dy), hip.transpose(x)
    o0 = torch.empty(nout, kin, dtype=torch.float32, device=dev)
    t00 = timeit(lambda: hip.gemm(dyt, xt, out=o0))
    t10 = timeit(lambda: hip.gemm(dy, xt, out=o0, a_mode=1))
    t01 = timeit(lambda: hip.gemm(dyt, x, out=o0, b_mode=1))
    print(f"  {name:8s} NT {t00:7.3f} ms | A as stored (a_mode 1) {t10:7.3f} ms ({(t10 - t00) * 1e3:+7.1f} us) | "
          f"B as stored (b_mode 1) {t01:7.3f} ms ({(t01 - t00) * 1e3:+7.1f} us)", flush=True)
