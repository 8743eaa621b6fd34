"""A smoke signal, not a claim about a trained policy: 200 SFT steps of the tiny MLA on synthetic batches with bf16 AdamW moments
(stochastic rounding, FSDPStrategy moments="bf16") and with fp32 moments, from the same weights on the same data; a second fp32 run on
another data seed gives the spread the difference is to be read against. Prints the mean total loss of every 20-step window per run (recorded at the end of profiles/adamw_m16.txt).
    python tools/exp_m16_convergence.py [--steps 200] [--out FILE]"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

R, POOL = 2, 8


def build(dev):
    from mla_amd.backbones import LLaMa2LLMBackbone
    from mla_amd.llama import LlamaConfig
    from mla_amd.mla import MLA
    from mla_amd.prismatic import PrismaticVLM
    from oracle import recipe
    bb = LLaMa2LLMBackbone(config=LlamaConfig(**recipe.TINY_LLAMA, activation_save_level=1), pad_to_multiple_of=1)
    vlm = PrismaticVLM("tiny", bb, token_size=recipe.TOKEN_SIZE, use_diff=True, use_pointcloud=False, use_contrastive=False, use_generation=False)
    m = MLA(vlm, None, token_size=recipe.TOKEN_SIZE, future_action_window_size=0, use_diff=True, use_pointcloud=False, use_contrastive=False)
    m.load_state_dict({k: recipe.det_weight(k, v.shape) for k, v in m.state_dict().items()}, strict=True)
    m.freeze_backbones("finetune")
    return m


def run(dev, moments, data_seed, steps):
    from mla_amd.strategy import FSDPStrategy
    from oracle import recipe
    torch.manual_seed(1234 + data_seed)                      # the diffusion draws (device generator)
    strat = FSDPStrategy(build(dev), dev.index or 0, max_steps=steps, global_batch_size=2, per_device_batch_size=2, learning_rate=1e-3,
                         weight_decay=0.01, max_grad_norm=1.0, lr_scheduler_type="linear-warmup+cosine-decay", warmup_ratio=0.1,
                         enable_gradient_checkpointing=False, repeated_diffusion_steps=R, moments=moments, moments_seed=7)
    strat.run_setup(100)
    pool = []
    for k in range(POOL):
        batch, _ = recipe.make_batch(B=2, R=R, ragged=False, seed=1000 * data_seed + k)
        b = {key: v for key, v in batch.items() if key not in ("images", "point_cloud")}
        b["images"] = {"front_image": batch["images"]["front_image"]}
        pool.append(b)
    return [float(strat.train_step(pool[s % POOL])["total_loss"]) for s in range(steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exp_m16_convergence needs the GPU")
    dev = torch.device("cuda:0")
    runs = (("fp32 moments, data seed 0", "fp32", 0), ("bf16 moments, data seed 0", "bf16", 0), ("fp32 moments, data seed 1", "fp32", 1))
    curves = {name: run(dev, moments, seed, args.steps) for name, moments, seed in runs}
    lines = [f"tiny MLA (no point tower), {args.steps} SFT steps, batch 2 x {R} diffusion repeats, pool of {POOL} synthetic batches per data seed, "
             "lr 1e-3 warm-up + cosine, wd 0.01, clip 1.0; mean total loss per 20-step window. A smoke signal: no trained policy is involved."]
    for name, c in curves.items():
        lines.append(f"{name}: " + " ".join(f"{statistics.mean(c[i:i + 20]):.4f}" for i in range(0, len(c), 20)))
    a, b, c = (curves[name] for name, _, _ in runs)
    tail = max(len(a) // 4, 1)
    lines.append(f"last {tail} steps, mean loss: fp32 {statistics.mean(a[-tail:]):.4f}, bf16 {statistics.mean(b[-tail:]):.4f}, fp32 on the other "
                 f"data seed {statistics.mean(c[-tail:]):.4f}; |bf16 - fp32| {abs(statistics.mean(a[-tail:]) - statistics.mean(b[-tail:])):.4f} "
                 f"against |fp32 - fp32 other seed| {abs(statistics.mean(a[-tail:]) - statistics.mean(c[-tail:])):.4f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
