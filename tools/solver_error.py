#!/usr/bin/env python
"""Solver error of DDIM and DPM-Solver++(2M) on an analytic model, from the code under test (CPU, no library call):
GaussianDiffusion.ddim_sample_loop and dpmpp2m_sample_loop over the project's schedule (squaredcos_cap_v2, 100 steps, "ddimN"
respacing) with the exact epsilon model of Gaussian data x0 ~ N(mu, s^2) per coordinate,
    eps*(x, t) = sigma_t (x - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2),
against the exact probability-flow solution from the first kept timestep,
    x0 = mu + (x_t - alpha_t mu) s / sqrt(alpha_t^2 s^2 + sigma_t^2).
112 coordinates ([1, 16, 7]: one chunk of 16 actions), mu ~ U(-0.6, 0.6), s ~ U(0.05, 0.5) from default_rng(0); RMS error over the
coordinates, for 32 starting points x_T = default_rng(100 + k).standard_normal(112). The model is evaluated in float64 and handed to
the loops as fp32; the loops run in fp32 as they do under MLA.predict_action_diff (tests/test_solver_dpmpp_host.py asserts the
conditions printed at the end).
    python tools/solver_error.py [--steps 4,5,8,10,20,25,50] [--out profiles/solver_dpmpp_error.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from mla_amd.diffusion import create_diffusion
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="4,5,8,10,20,25,50")
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    mu = torch.from_numpy(rng.uniform(-0.6, 0.6, 112)).view(1, 16, 7)
    s = torch.from_numpy(rng.uniform(0.05, 0.5, 112)).view(1, 16, 7)
    acp = torch.from_numpy(create_diffusion("").alphas_cumprod)
    x_Ts = [torch.from_numpy(np.random.default_rng(100 + k).standard_normal(112)).view(1, 16, 7).float() for k in range(args.draws)]

    def eps(x, ts, **kw):
        ab = acp[ts].view(-1, 1, 1)
        return ((1 - ab).sqrt() * (x.double() - ab.sqrt() * mu) / (ab * s ** 2 + (1 - ab))).float()

    def errors(solver, n):
        d = create_diffusion(f"ddim{n}")
        loop = d.dpmpp2m_sample_loop if solver == "dpmpp2m" else d.ddim_sample_loop
        ab = acp[d.timestep_map[-1]]
        out = []
        for x_T in x_Ts:
            exact = mu + (x_T.double() - ab.sqrt() * mu) * s / (ab * s ** 2 + (1 - ab)).sqrt()
            got = loop(eps, x_T.shape, x_T, clip_denoised=False, model_kwargs={}, device="cpu")
            out.append(float(((got.double() - exact) ** 2).mean().sqrt()))
        return np.array(out)

    steps = [int(v) for v in args.steps.split(",")]
    err = {(solver, n): errors(solver, n) for solver in ("ddim", "dpmpp2m") for n in steps}
    lines = ["RMS error against the exact probability-flow solution, analytic Gaussian model (tools/solver_error.py), "
             f"mean over {args.draws} starting points; fp32 loops",
             "| steps | DDIM (order 1) | DPM-Solver++(2M) | ratio |", "|---|---|---|---|"]
    for n in steps:
        a, b = err["ddim", n].mean(), err["dpmpp2m", n].mean()
        lines.append(f"| {n} | {a:.4f} | {b:.4f} | {a / b:.2f} |")
    if 4 in steps and 8 in steps:
        r = err["dpmpp2m", 4] / err["ddim", 8]
        lines.append(f"2M at 4 steps / DDIM at 8 steps, per starting point: {r.min():.2f} .. {r.max():.2f} "
                     f"({int((r < 1).sum())} of {len(r)} below 1)")
    if 25 in steps and 50 in steps:
        lines.append(f"err(25) / err(50): DPM-Solver++(2M) {err['dpmpp2m', 25].mean() / err['dpmpp2m', 50].mean():.2f} (order 2: 4), "
                     f"DDIM {err['ddim', 25].mean() / err['ddim', 50].mean():.2f} (order 1: 2)")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
