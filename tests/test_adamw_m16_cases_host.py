"""CPU, no library call: the numpy model of the bf16-moment AdamW step (tests/adamw_m16_cases.py) that the GPU tests compare the
kernels with bit for bit -- the generator against its published known answers, the rounding on hand cases, why the rounding has to be
stochastic, and that a range may be cut into launches anywhere."""
import numpy as np
import torch

import adamw_m16_cases as M
import trunk_cases as T


def test_philox_known_answers():
    for counter, key, want in M.PHILOX_KAT:
        got = tuple(int(w[0]) for w in M.philox4x32_10(counter, key))
        assert got == want, (counter, key, [hex(x) for x in got])
    # vectorised == one at a time
    c0 = np.array([0, 1, 0xFFFFFFFF, 12345], dtype=np.uint64)
    vec = M.philox4x32_10((c0, 7, 3, 0), (0xDEADBEEF, 0x01234567))
    for j, c in enumerate(c0):
        one = M.philox4x32_10((int(c), 7, 3, 0), (0xDEADBEEF, 0x01234567))
        assert [int(w[j]) for w in vec] == [int(w[0]) for w in one]


def test_element_to_counter_and_word():
    step = 9
    want = {0: ((0, 0, step, 0), 0), 3: ((0, 0, step, 0), 3), 4: ((1, 0, step, 0), 0), 2 ** 34 + 5: ((1, 1, step, 0), 1)}
    for e, (counter, word) in want.items():
        assert M.element_counter(e, step) == (counter, word), e
        # the words random_words hands out are those of that counter, whatever the range around the element
        r = int(M.philox4x32_10(counter, (M.SEED & 0xFFFFFFFF, M.SEED >> 32))[word][0])
        assert int(M.random_words(1, M.SEED, step, e)[0]) == r, e
        if e >= 2:
            assert int(M.random_words(7, M.SEED, step, e - 2)[2]) == r, e
    # hi32 of the group index is used: the same low word, another stream
    assert int(M.random_words(1, M.SEED, step, 5)[0]) != int(M.random_words(1, M.SEED, step, 2 ** 34 + 5)[0])
    # seed halves are the key in this order
    assert int(M.random_words(1, 0x0000000100000002, 1, 0)[0]) == int(M.philox4x32_10((0, 0, 1, 0), (2, 1))[0][0])


def _f(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)


def test_sr16_hand_cases():
    x = _f(0x3F808001)                                     # 1.0 + 2^-7 + 2^-23: inexact in bf16
    assert int(M.sr16(x, 0)[0]) == 0x3F80                   # r16 = 0 truncates
    assert int(M.sr16(x, 0xFFFF)[0]) == 0x3F81              # r16 = 0xffff rounds any inexact value away from zero
    assert int(M.sr16(x, 0x7FFE)[0]) == 0x3F80 and int(M.sr16(x, 0x7FFF)[0]) == 0x3F81      # up exactly when dropped + r16 >= 2^16
    exact = _f(0x3F810000)
    assert int(M.sr16(exact, 0)[0]) == int(M.sr16(exact, 0xFFFF)[0]) == 0x3F81             # an exact value is unchanged
    neg = _f(0xBF808001)
    assert int(M.sr16(neg, 0)[0]) == 0xBF80 and int(M.sr16(neg, 0xFFFF)[0]) == 0xBF81      # sign-magnitude: away from zero
    below2 = _f(0x3FFFFFFF)                                 # just below 2.0: the carry runs into the exponent
    assert int(M.sr16(below2, 0xFFFF)[0]) == 0x4000 and int(M.sr16(below2, 0)[0]) == 0x3FFF
    assert float(M.decode(M.sr16(below2, 0xFFFF))[0]) == 2.0
    for r16 in (0, 1, 0xFFFF):                              # inf / NaN pass through
        assert int(M.sr16(_f(0x7F800000), r16)[0]) == 0x7F80 and int(M.sr16(_f(0xFF800000), r16)[0]) == 0xFF80
        assert np.isnan(M.decode(M.sr16(_f(0x7FC00001), r16))[0]) and np.isnan(M.decode(M.sr16(_f(0x7F800001), r16))[0])
    assert int(M.sr16(_f(0), 0xFFFF)[0]) == 0 and int(M.sr16(_f(0x80000000), 0xFFFF)[0]) == 0x8000      # zeros stay zeros
    # only the low 16 bits of r16 count
    assert int(M.sr16(x, 0xABCD0000)[0]) == 0x3F80


def test_emulation_is_adamw_emul32_on_decoded_moments():
    n, n_decay, step, wd = 37, 21, 3, 0.01
    p, g, m16, v16 = M.m16_state("unit", n)
    pp, mo, vo, mm, vv = M.adamw_m16_emul32(p, g, m16, v16, step, wd, T.ADAMW_GS, n_decay=n_decay, seed=M.SEED, index_base=8)
    a = T.adamw_emul32(p, g, m16.float(), v16.float(), step, wd, T.ADAMW_GS)
    b = T.adamw_emul32(p, g, m16.float(), v16.float(), step, 0.0, T.ADAMW_GS)
    assert T.bits_equal(mm, a[1]) and T.bits_equal(vv, a[2]) and T.bits_equal(a[1], b[1])
    assert T.bits_equal(pp[:n_decay], a[0][:n_decay]) and T.bits_equal(pp[n_decay:], b[0][n_decay:])
    assert not T.bits_equal(a[0], b[0])
    # stored moments: within one bf16 spacing of the unrounded ones, never on the far side
    for out, full in ((mo, mm), (vo, vv)):
        d = np.abs(out.float().numpy().astype(np.float64) - full.numpy().astype(np.float64))
        assert (d < M.ulp16_of(full.numpy())).all()
    assert mo.dtype == torch.bfloat16 and vo.dtype == torch.bfloat16


def test_why_stochastic_rounding(capsys):
    """4096 elements, v0 = 1, g = 0, 200 steps: exp_avg_sq must decay as beta2^200. Stochastic rounding is unbiased (the mean lands
    within 6 standard errors, the bound computed from the sample); round-to-nearest bf16 never moves off 1.0."""
    n, steps = 4096, 200
    p, g = torch.zeros(n), torch.zeros(n)
    one = torch.ones(n).to(torch.bfloat16)
    m_sr, v_sr, m_rn, v_rn = one * 0, one.clone(), one * 0, one.clone()
    for step in range(1, steps + 1):
        _, m_sr, v_sr, _, _ = M.adamw_m16_emul32(p, g, m_sr, v_sr, step, 0.0, None, seed=0, index_base=0)
        _, m_rn, v_rn, _, _ = M.adamw_m16_emul32(p, g, m_rn, v_rn, step, 0.0, None, rounding="rne")
    want = np.float32(1.0)
    for _ in range(steps):
        want = np.float32(np.float32(0.999) * want)         # beta2^200 in fp32 arithmetic
    v = v_sr.float().numpy().astype(np.float64)
    mean, std = v.mean(), v.std(ddof=1)
    bound = 6 * std / np.sqrt(n)
    with capsys.disabled():
        print(f"\nv after {steps} steps from 1.0: stochastic mean {mean:.5f} (fp32 {float(want):.5f}, sample std {std:.4f}, bound {bound:.5f}); "
              f"round-to-nearest min {float(v_rn.float().min())} max {float(v_rn.float().max())}")
    assert std > 0 and abs(mean - float(want)) <= bound, (mean, float(want), std, bound)
    assert bool((v_rn.float() == 1.0).all()), "round-to-nearest bf16 was expected to hold v at exactly 1.0"


def test_split_invariance_of_the_emulation():
    n, n_decay, step, wd, base = 4100, 3000, 4, 0.01, 2 ** 34 + 4
    p, g, m16, v16 = M.m16_state("unit", n)
    whole = M.adamw_m16_emul32(p, g, m16, v16, step, wd, T.ADAMW_GS, n_decay=n_decay, seed=M.SEED, index_base=base)
    for cut in (2048, 1001):                               # a multiple of 4 and an odd index
        a = M.adamw_m16_emul32(p[:cut], g[:cut], m16[:cut], v16[:cut], step, wd, T.ADAMW_GS, n_decay=min(n_decay, cut), seed=M.SEED,
                               index_base=base)
        b = M.adamw_m16_emul32(p[cut:], g[cut:], m16[cut:], v16[cut:], step, wd, T.ADAMW_GS, n_decay=max(n_decay - cut, 0), seed=M.SEED,
                               index_base=base + cut)
        for w, x, y in zip(whole, a, b):
            assert T.bits_equal(w, torch.cat([x, y])), cut
    # the second range without the advanced base is another stream
    c = M.adamw_m16_emul32(p[2048:], g[2048:], m16[2048:], v16[2048:], step, wd, T.ADAMW_GS, n_decay=n_decay - 2048, seed=M.SEED, index_base=base)
    assert not T.bits_equal(c[2], whole[2][2048:])
