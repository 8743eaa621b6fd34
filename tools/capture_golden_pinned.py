"""Golden vectors for pinned sampling (MLA.predict_action_diff*(known_actions=...)) from the REAL reference -- build container only.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_pinned.py

The reference's sampling loops hand `denoised_fn` to p_mean_variance, which applies it to the x0 prediction of every step
(models/diffusion/gaussian_diffusion.py:318-321, :442-518, :608-688). Here the hook overwrites a mask of chunk entries with known values
(replacement inpainting) and the loops run over the closed-form toy epsilon of oracle/capture_golden_infer.py, so the sampler
arithmetic with the hook is pinned independently of any network: ddim_sample_loop at eta = 0 on "ddim8" and "ddim4", p_sample_loop on
the 100-step process under torch.manual_seed(5), clip_denoised=False throughout (what predict_action_diff passes).
Writes tests/golden/sampler_pinned.npz: noise [2, 16, 7], known, mask (the first 3 chunk steps of sample 0, the first 5 of sample 1, the
rest free) and the three results."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from oracle.capture_golden_infer import toy_eps  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampler_pinned.npz")
PINNED_STEPS = (3, 5)


def main():
    ref_import.setup()
    from models.diffusion import create_diffusion
    make = lambda respacing: create_diffusion(timestep_respacing=respacing, noise_schedule="squaredcos_cap_v2", diffusion_steps=100,  # noqa: E731
                                              sigma_small=True, learn_sigma=False)
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(2, 16, 7, generator=g)
    known = torch.rand(2, 16, 7, generator=g) * 2 - 1                          # normalised actions live in [-1, 1]
    mask = torch.zeros(2, 16, 7, dtype=torch.bool)
    for b, d in enumerate(PINNED_STEPS):
        mask[b, :d] = True
    pin = lambda px: torch.where(mask, known, px)                              # noqa: E731
    res = {"noise": noise.numpy(), "known": known.numpy(), "mask": mask.numpy()}
    for name in ("ddim8", "ddim4"):
        torch.manual_seed(5)
        res[name] = make(name).ddim_sample_loop(toy_eps, noise.shape, noise, clip_denoised=False, denoised_fn=pin, model_kwargs={},
                                                progress=False, device="cpu", eta=0.0).numpy()
    torch.manual_seed(5)
    res["ddpm100"] = make("").p_sample_loop(toy_eps, noise.shape, noise, clip_denoised=False, denoised_fn=pin, model_kwargs={},
                                            progress=False, device="cpu").numpy()
    for name in ("ddim8", "ddim4", "ddpm100"):
        assert np.array_equal(res[name][res["mask"]], res["known"][res["mask"]]), name   # the last step returns the pinned x0 itself
    np.savez_compressed(OUT, **res)
    print("sampler_pinned.npz:", {k: (v.shape, float(np.abs(v).max())) for k, v in res.items()})


if __name__ == "__main__":
    main()
