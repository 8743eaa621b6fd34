"""CPU: the host models of tests/guard_cases.py against torch -- the finite cases are clip_grad_norm_'s coefficient, the verdict is
"not finite", and a guarded step is the step or the identity."""
import numpy as np
import torch

import guard_cases as GC
import trunk_cases as T


def test_clip_model_matches_torch_and_flags_exactly_the_nonfinite_cases():
    seen = set()
    for sumsq, max_norm in GC.CLIP_CASES:
        coef, nrm, skip = GC.clip_coef_guard_model(sumsq, max_norm)
        seen.add(skip)
        assert skip == int(not np.isfinite(np.float32(sumsq))) and coef.dtype == nrm.dtype == np.float32
        if skip:
            assert coef == 0.0 and not np.isfinite(nrm)
            continue
        n = torch.tensor(sumsq, dtype=torch.float32).sqrt()
        want = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (n + 1e-6), max=1.0)
        assert np.float32(want) == coef and np.float32(n) == nrm and GC.clip_coef_model(sumsq, max_norm) == (coef, nrm)
    assert seen == {0, 1}
    assert GC.clip_coef_guard_model(4.0e4, 1.0)[0] == np.float32(1.0) / np.float32(np.float32(200.0) + np.float32(1e-6))
    # the largest finite fp32 is finite; a sum that overflowed is not
    with np.errstate(over="ignore"):
        overflowed = np.float32(3e38) * np.float32(2)
    assert GC.clip_coef_guard_model(np.finfo(np.float32).max, 1.0)[2] == 0 and GC.clip_coef_guard_model(overflowed, 1.0)[2] == 1


def test_guarded_step_is_the_step_or_the_identity():
    p, g, m, v = T.adamw_state("unit", 37)
    step = lambda p, g, m, v: T.adamw_emul32(p, g, m, v, 3, 0.01, T.ADAMW_GS, **T.ADAMW_HYPER)
    out = GC.guarded_step(0, step, p, g, m, v)
    assert all(T.bits_equal(a, b) for a, b in zip(out, step(p, g, m, v))) and not T.bits_equal(out[0], p)
    g_bad = g.clone()
    g_bad[GC.bad_positions(37)[-1]] = float("inf")
    held = GC.guarded_step(1, step, p, g_bad, m, v, None)
    assert held[4] is None and all(T.bits_equal(a, b) and a is not b for a, b in zip(held[:4], (p, g_bad, m, v)))
    assert GC.bad_positions(37) == [0, 36] and GC.bad_positions(4) == [0, 3] and GC.bad_positions(1) == [0] and GC.bad_positions(4100) == [0, 4099]
    assert GC.bad_positions(4095) == [0, 4092, 4094]
