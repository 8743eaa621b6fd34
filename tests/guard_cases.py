"""The skip_nonfinite guard (mla_clip_coef_guard / mla_adamw_guard_step, include/mla_hip_optim.h) as host models -- shared by
tests/test_guard_cases_host.py, test_adamw_guard_gpu.py, test_fsdp_guard_gloo.py and test_train_guard_gpu.py.

  clip_coef_guard_model: clip_coef_kernel's fp32 arithmetic in numpy plus the verdict: skip = (exponent bits of sumsq all ones).
  guarded_step: "a guarded step is today's step, or the identity" -- the step function is whatever models the unguarded launch
  (trunk_cases.adamw_emul32, adamw_m16_cases.adamw_m16_emul32, or the launch itself).
  GuardMethods: clip_coef_guard / adamw_guard for a host LocalOps class, built on that class's own unguarded methods."""
import numpy as np
import torch

# (sumsq, max_norm): no gradient, no clipping, clipping by 1 / 200, the largest finite norms, and the two non-finite verdicts
CLIP_CASES = ((0.0, 1.0), (1.0, 1.0), (4.0e4, 1.0), (3.0e38, 1.0), (float("inf"), 1.0), (float("nan"), 1.0),
              (0.0, 3.0e38), (4.0e4, 3.0e38), (float("inf"), 3.0e38), (float("nan"), 3.0e38))
# where a step's inf sits in g for the flag-1 cases of a size n: first element, last element, inside the n % 4 tail
def bad_positions(n):
    return sorted({0, n - 1} | ({n - n % 4} if n % 4 else set()))


def is_nonfinite32(x) -> bool:
    return (int(np.float32(x).view(np.uint32)) & 0x7F800000) == 0x7F800000


def clip_coef_model(sumsq, max_norm):
    """mla_clip_coef: (coef, norm) as np.float32 -- coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) in fp32, a NaN quotient gives 1."""
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float32(sumsq), dtype=np.float32)
        c = np.float32(max_norm) / np.float32(nrm + np.float32(1e-6))
    return (c if c < np.float32(1.0) else np.float32(1.0)), nrm


def clip_coef_guard_model(sumsq, max_norm):
    """mla_clip_coef_guard: (coef, norm, skip). Finite sumsq: clip_coef_model and 0; +inf / NaN: coef 0, the non-finite norm, 1."""
    coef, nrm = clip_coef_model(sumsq, max_norm)
    bad = is_nonfinite32(sumsq)
    return (np.float32(0.0) if bad else coef), nrm, int(bad)


def guarded_step(skip, step_fn, *streams):
    """Streams after a guarded launch: step_fn(*streams) (a tuple of the new streams) with the flag clear, clones of the old ones with
    it set. step_fn must not write its arguments."""
    if skip:
        return tuple(None if t is None else t.clone() for t in streams)
    return tuple(step_fn(*streams))


class GuardMethods:
    """Mix-in for a host LocalOps class that has clip_coef, adamw_groups and (for the forms it is used with) adamw_ema_groups /
    adamw_m16: the two methods HipLocalOps gains for skip_nonfinite, as "the unguarded method, or nothing". Records its calls."""

    def clip_coef_guard(self, sumsq1, max_norm, coef1, norm1, skip1):
        assert skip1.dtype == torch.int32 and skip1.numel() == 1
        coef, nrm, skip = clip_coef_guard_model(float(sumsq1), max_norm)
        if not skip:
            self.clip_coef(sumsq1, max_norm, coef1, norm1)      # the class's own arithmetic: guard on / off compare bit for bit
        else:
            coef1.fill_(0.0)
            norm1.copy_(torch.from_numpy(np.asarray([nrm])))
        skip1.fill_(skip)

    def adamw_guard(self, p32, g32, m, v, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay, seed, index_base, skip1):
        self.guard_calls = getattr(self, "guard_calls", [])
        self.guard_calls.append((p32.numel(), n_decay, step, ema is not None, int(skip1)))
        if int(skip1):
            return
        if m.dtype == torch.bfloat16:
            self.adamw_m16(p32, g32, m, v, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay, seed, index_base)
        elif ema is not None:
            self.adamw_ema_groups(p32, g32, m, v, ema, p16, n_decay, lr, betas, eps, wd, step, grad_scale, ema_decay)
        else:
            self.adamw_groups(p32, g32, m, v, p16, n_decay, lr, betas, eps, wd, step, grad_scale)
