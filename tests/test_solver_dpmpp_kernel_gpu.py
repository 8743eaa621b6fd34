"""GPU: mla_dpmpp2m_step / mla_dpmpp2m_step_pin (mla_amd/csrc/sampler.hip) against the torch restatement of their arithmetic, one
operation per rounding (tests/test_solver_dpmpp_host.py shows on the CPU that the restatement, chained, is dpmpp2m_sample_loop).

Bit-identity, not a tolerance: x, its bf16 cast, the history and the counter after every launch of a walk through a table of random
finite coefficients (every coefficient non-trivial at every step, which the real tables' first and last rows are not)."""
import pytest
import torch

from test_solver_dpmpp_host import dpmpp2m_update

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
STEPS = [1, 2, 3, 8]
NS = [1, 7, 112, 255, 256, 257, 1792]                                        # around the 256-thread stride; 1 792 = 16 chunks of 16 x 7


def _walk(dev, n, steps, pinned):
    from mla_amd import hip
    g = torch.Generator().manual_seed(1000 * steps + n + (7 if pinned else 0))
    coef = (torch.randn(steps, 5, generator=g) * 1.5).to(dev).contiguous()
    x0 = (torch.randn(n, generator=g) * 3.0).to(dev)
    h0 = (torch.randn(n, generator=g) * 2.0).to(dev)                          # a non-zero history: the kernel reads what it is given
    eps = (torch.randn(steps, n, generator=g) * 3.0).to(BF).to(dev)
    known = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    mask = (torch.rand(n, generator=g) < 0.4).to(dev)
    if pinned and n > 1:
        mask[0], mask[-1] = True, False                                       # both kinds of entry at every n > 1
    pin = mask.to(torch.uint8)
    step = torch.full((1,), steps - 1, dtype=torch.int32, device=dev)

    def launch(x, xb, hist, s, advance=True):
        if pinned:
            hip.dpmpp2m_step_pin(x, eps[s], xb, hist, coef, known, pin, step, advance=advance)
        else:
            hip.dpmpp2m_step(x, eps[s], xb, hist, coef, step, advance=advance)

    def ref(x, hist, s):
        return dpmpp2m_update(x, eps[s].float(), coef[s], hist, *((known, mask) if pinned else ()))

    x, hist, xb = x0.clone(), h0.clone(), torch.full((n,), float("nan"), dtype=BF, device=dev)
    want, want_h = x0.clone(), h0.clone()
    for s in reversed(range(steps)):
        want, want_h = ref(want, want_h, s)
        launch(x, xb, hist, s)
        assert torch.equal(x, want), f"step {s}: max |diff| {float((x - want).abs().max()):.3e}"
        assert torch.equal(hist, want_h) and torch.equal(xb, want.to(BF)) and int(step.item()) == s - 1, s
        if pinned:
            assert torch.equal(hist[mask], known[mask]), s
    assert bool(torch.isfinite(x).all()) and not torch.equal(x, x0)
    for stale in (-1, steps):                                                 # outside the table: nothing is written, the counter stays
        step.fill_(stale)
        before, before_b, before_h = x.clone(), xb.clone(), hist.clone()
        launch(x, xb, hist, 0)
        assert torch.equal(x, before) and torch.equal(xb, before_b) and torch.equal(hist, before_h) and int(step.item()) == stale, stale
    step.fill_(steps - 1)
    x.copy_(x0)
    hist.copy_(h0)
    launch(x, xb, hist, steps - 1, advance=False)
    want, want_h = ref(x0, h0, steps - 1)
    assert torch.equal(x, want) and torch.equal(xb, want.to(BF)) and torch.equal(hist, want_h) and int(step.item()) == steps - 1
    return x0, h0, eps, coef, known, step


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("n", NS)
def test_dpmpp2m_step_is_the_restatement(dev, n, steps):
    _walk(dev, n, steps, pinned=False)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("n", NS)
def test_dpmpp2m_step_pin_is_the_restatement(dev, n, steps):
    from mla_amd import hip
    x0, h0, eps, coef, known, step = _walk(dev, n, steps, pinned=True)
    # pin all zero: the bits of the plain kernel
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)
    x, xb, h, y, yb, hy = x0.clone(), torch.zeros(n, dtype=BF, device=dev), h0.clone(), x0.clone(), torch.zeros(n, dtype=BF, device=dev), h0.clone()
    hip.dpmpp2m_step_pin(x, eps[steps - 1], xb, h, coef, known, zero, step, advance=False)
    hip.dpmpp2m_step(y, eps[steps - 1], yb, hy, coef, step, advance=False)
    assert torch.equal(x, y) and torch.equal(xb, yb) and torch.equal(h, hy) and not torch.equal(x, x0)


def test_real_table_first_step_ignores_a_zero_history_and_last_step_returns_the_prediction(dev):
    """The real 4-step table: k1 = 0 at the first step (a zeroed history adds a zero), and row 0 = (., ., 0, 1, 0) returns the x0
    prediction, the pinned entries exactly."""
    from mla_amd import hip
    from mla_amd.diffusion import create_diffusion
    coef, _ = create_diffusion("ddim4").dpmpp2m_tables(dev)
    assert coef.shape == (4, 5) and float(coef[3, 4]) == 0.0 and coef[0, 2:].tolist() == [0.0, 1.0, 0.0]
    n = 112
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, generator=g) * 2).to(dev)
    eps = torch.randn(4, n, generator=g).to(BF).to(dev)
    known = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    mask = (torch.arange(n) < 35).to(dev)
    hist, xb = torch.zeros(n, device=dev), torch.zeros(n, dtype=BF, device=dev)
    step = torch.full((1,), 3, dtype=torch.int32, device=dev)
    for s in (3, 2, 1, 0):
        hip.dpmpp2m_step_pin(x, eps[s], xb, hist, coef, known, mask.to(torch.uint8), step)
    assert int(step.item()) == -1 and torch.equal(x, hist) and torch.equal(x[mask], known[mask]) and bool(torch.isfinite(x).all())
    # the wrappers' checks
    with pytest.raises(ValueError):
        hip.dpmpp2m_step(x, eps[0], xb, hist[:-1], coef, step)
    with pytest.raises(ValueError):
        hip.dpmpp2m_step(x, eps[0], xb, hist, coef[:, :4].contiguous(), step)
    with pytest.raises(TypeError):
        hip.dpmpp2m_step(x, eps[0], xb, hist.double(), coef, step)
    with pytest.raises(TypeError):
        hip.dpmpp2m_step_pin(x, eps[0], xb, hist, coef, known, mask, step)
