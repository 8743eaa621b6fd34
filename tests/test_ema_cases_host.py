"""CPU: the numpy emulation of the weight average (tests/ema_cases.py), which tests/test_adamw_ema_gpu.py holds the kernels to bit for
bit, against the update in fp64 -- within 2 fp32 ulp (one rounding for the product, one for the fma) on every family; and two wrong
emulations (the average of the bf16-rounded weight; `decay` in place of `1 - decay`) far outside that bound."""
import numpy as np
import pytest
import torch

import ema_cases as E
import trunk_cases as T

N = 4100


def _new_p(family):
    """The master an EMA step sees: adamw_state's p after one emulated AdamW step (step 3, weight decay, clip coefficient)."""
    st = T.adamw_state(family, N)
    return T.adamw_emul32(*st, 3, 0.01, T.ADAMW_GS)[0]


@pytest.mark.parametrize("family", T.ADAMW_FAMILIES)
def test_ema_emulation(family, capsys):
    p, e = _new_p(family), E.ema_start(family, N)
    assert int((e == 0).sum()) == (N + 3) // 4 and int(((e != 0) & (e.abs() < 1e-4)).sum()) >= N // 4 - 1
    worst = {}
    for decay in E.DECAYS + (0.999, 0.5):
        ref, bound = E.ema_ref64(e, p, decay)
        got = E.ema_emul32(e, p, decay)
        worst[decay] = E.ema_ratio(got, ref, bound)
        assert worst[decay] <= 1, (family, decay, worst[decay])
        if decay == 1.0:
            assert T.bits_equal(got, e)
        if decay == 0.0:
            assert T.bits_equal(got, p)
    # the average runs on the fp32 master: fed the bf16 copy it is off by (1 - decay) * 2^-9 |p|, thousands of ulp where the average
    # itself is small (the zero and 1e-6 quarters)
    ref, bound = E.ema_ref64(e, p, 0.9999)
    from_bf16 = E.ema_ratio(E.ema_emul32(e, p.to(T.BF).to(T.F32), 0.9999), ref, bound)
    assert from_bf16 > 100, (family, from_bf16)
    # decay where 1 - decay belongs: the new weight enters with 0.9999 instead of 1e-4
    d32, _ = E.ema_factors32(0.9999)
    swapped = E.ema_ratio(E.ema_emul32(e, p, 0.9999, factors=(d32, d32)), ref, bound)
    assert swapped > 1e5, (family, swapped)
    with capsys.disabled():
        print(f"\nema {family:<5} emulation: worst of the bound by decay " + " ".join(f"{d}:{r:.3f}" for d, r in worst.items())
              + f"; from the bf16 copy {from_bf16:.0f}, decay for 1 - decay {swapped:.0f}")


def test_factors_follow_the_header_convention():
    """1 - decay is formed in double and cast once: at 0.9999 the fp32 difference 1 - fl32(0.9999) is another number."""
    d32, omd = E.ema_factors32(0.9999)
    assert omd == np.float32(1.0 - 0.9999) and omd != np.float32(1.0) - d32
    from mla_amd import hip
    d, o = hip.ema_factors(0.9999)
    assert (np.float32(d), np.float32(o)) == (d32, omd)
    for bad in (-1e-9, 1.0000001, float("nan")):
        with pytest.raises(ValueError):
            hip.ema_factors(bad)
