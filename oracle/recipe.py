"""Deterministic weights and synthetic batches shared by oracle/capture_golden.py (build container, real reference)
and the tests (GPU box, no reference): everything is a function of the tensor's NAME and a seed, so no large weight or
image files have to be committed -- only the captured outputs are stored under tests/golden/."""
import zlib

import numpy as np
import torch

TINY_LLAMA = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=9, num_attention_heads=2,
                  rms_norm_eps=1e-5)
TOKEN_SIZE = 256
# post-training generation heads of the tiny model (BASELINE config[3] scaled down; S of the LLM memory is not a multiple of 32)
GEN_TINY = dict(num_image_gen_queries=32, image_decoder_layers=2, image_decoder_heads=8, pointcloud_trans_dim=256,
                pointcloud_decoder_layers=2, pointcloud_decoder_heads=8, pointcloud_group_size=8, pointcloud_num_groups=16)
PAD_ID = 512  # tokenizer.pad_token_id == base vocab size (llama2.py:75-77); embedding table has vocab + 1 rows


def _gen(name: str, seed: int = 0) -> torch.Generator:
    return torch.Generator().manual_seed((zlib.crc32(name.encode()) + 1000003 * seed) & 0x7FFFFFFF)


def det_randn(name, shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=_gen(name, seed)) * scale


def det_weight(name: str, shape, seed: int = 0) -> torch.Tensor:
    """Initialisation recipe by parameter role (all fp32)."""
    shape = tuple(shape)
    leaf = name.split(".")[-1]
    if leaf == "num_batches_tracked":
        return torch.zeros(shape, dtype=torch.long)
    if leaf == "running_mean":
        return torch.zeros(shape)
    if leaf == "running_var":
        return torch.ones(shape)
    if len(shape) <= 1 and leaf == "weight":                      # norm / BatchNorm scales
        return 1.0 + det_randn(name, shape, 0.1, seed)
    if leaf == "bias" or leaf.endswith("_bias"):                   # incl. nn.MultiheadAttention.in_proj_bias
        return det_randn(name, shape, 0.05, seed)
    if leaf in ("image_gen_queries", "mae_mask_token", "mae_pos_embed"):
        return det_randn(name, shape, 0.5, seed)
    if leaf in ("cls_token", "pos_embed", "class_embedding", "split_embedding"):
        return det_randn(name, shape, 0.02, seed)
    if "embed_tokens" in name:
        return det_randn(name, shape, 0.5, seed)
    fan_in = 1
    for s in shape[1:]:
        fan_in *= s
    return det_randn(name, shape, fan_in ** -0.5, seed)


def grad_slice(g):
    """The per-parameter gradient sample stored in the end-to-end goldens (round 6, VERDICT r5 next #3: strict parity on EVERY
    parameter, not 11): the tensor as a matrix [shape[0], rest] (vectors: one row) -- whole when it has at most 4 096 elements, else
    its fixed 64 x 64 corner (a 1-row vector: its first 4 096 elements). Used by the capture scripts (on the reference's gradients)
    and by the GPU tests / tools/parity_table.py (on ours), so both sides cut the same elements."""
    g2 = g.reshape(g.shape[0], -1) if g.dim() >= 2 else g.reshape(1, -1)
    if g2.numel() <= 4096:
        return g2
    return g2[:64, :64] if g2.shape[0] > 1 else g2[:, :4096]


def make_state_dict(shapes: dict, seed: int = 0) -> dict:
    return {k: det_weight(k, s, seed) for k, s in shapes.items()}


def make_batch(B: int = 2, L: int = 16, R: int = 2, ragged: bool = True, seed: int = 0, vocab: int = 512, n_points: int = 1024,
               img: int = 672, with_next: bool = False, with_tactile: bool = False):
    """Synthetic batch with the collator's schema (util/data_utils.py:179-193) + the random draws of one step."""
    g = _gen("batch", seed)
    rgb = torch.randn(B, 3, img, img, generator=g)
    images = torch.cat([rgb, torch.ones(B, 1, img, img)], dim=1)
    lo = torch.tensor([0.0, -0.4, 0.75])
    hi = torch.tensor([0.6, 0.4, 1.25])
    pc = lo + (hi - lo) * torch.rand(B, n_points, 3, generator=g)
    ids = torch.randint(3, vocab - 12, (B, L), generator=g)
    ids[:, 0] = 1
    lens = [L] * B
    if ragged and B > 1:
        lens[1] = L - 3
    for b in range(B):
        ids[b, lens[b] - 1] = 2
        ids[b, lens[b]:] = PAD_ID
    attention_mask = ids != PAD_ID
    labels = torch.full_like(ids, -100)
    for b in range(B):
        labels[b, lens[b] - 1] = 2        # diffusion mode keeps only the final </s> (datasets.py:158-164)
    actions = torch.rand(B, 1, 7, generator=g) * 2 - 1
    proprio = torch.rand(B, 1, 7, generator=g) * 2 - 1
    Bp = B * R
    draws = dict(noise=torch.randn(Bp, 1, 7, generator=g), timestep=torch.randint(0, 100, (Bp,), generator=g),
                 fps_start0=torch.randint(0, n_points, (Bp,), generator=g),
                 fps_start1=torch.randint(0, n_points // 2, (Bp,), generator=g))
    batch = dict(input_ids=ids, attention_mask=attention_mask, labels=labels, images={"front_image": images}, point_cloud=pc,
                 actions=actions, proprio=proprio, action_masks=torch.ones(B, 1, dtype=torch.bool), camera_name="rlbench_front")
    if with_tactile:      # one arm: 12 tactile channels, gripper position inside the workspace box, next reading for the generation head
        gt = _gen("tactile", seed)
        batch["tactile"] = torch.rand(B, 12, generator=gt) * 2 - 1
        batch["gripper_xyz"] = lo + (hi - lo) * torch.rand(B, 3, generator=gt)
        batch["next_tactile"] = torch.rand(B, 12, generator=gt) * 2 - 1
    if with_next:
        batch["next_images"] = torch.randn(B, 3, img, img, generator=_gen("next_images", seed))
        batch["next_point_cloud"] = lo + (hi - lo) * torch.rand(B, n_points, 3, generator=_gen("next_pc", seed))
    return batch, draws


# ------------------------------------------------------------------------------------------------- data-side fixtures
class ToyTokenizer:
    """Stand-in for the Llama tokenizer (absent from the image) with the three calls the data transform makes: ``decode`` /
    ``batch_decode`` print id i as "<i>", ``__call__`` maps "<i>" back to i, "</s>" to 2, any other character to 3 + ord % 200, and
    prepends BOS (1) with add_special_tokens. One id per action token, like the real vocabulary tail."""
    vocab_size, pad_token_id, padding_side = 1000, 999, "right"

    def decode(self, ids):
        return "".join(f"<{int(i)}>" for i in ids)

    def batch_decode(self, rows):
        return [self.decode(r) for r in rows]

    def __call__(self, text, add_special_tokens=True):
        import re
        ids = [1] if add_special_tokens else []
        for tok in re.findall(r"</s>|<\d+>|.", text, flags=re.S):
            ids.append(2 if tok == "</s>" else int(tok[1:-1]) if (len(tok) > 2 and tok[1:-1].isdigit()) else 3 + ord(tok) % 200)
        return type("Enc", (), {"input_ids": ids})()


class ToyImageTransform:
    """Deterministic stand-in for CLIPImageProcessor.preprocess (its arithmetic has its own fixture, tests/golden/preprocess.npz):
    nearest-neighbour 224 -> 672 and /255, returned the way HF does ({"pixel_values": [tensor]})."""

    def preprocess(self, img, return_tensors="pt"):
        a = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float() / 255.0
        return {"pixel_values": [a.repeat_interleave(3, 1).repeat_interleave(3, 2)]}


def make_rlds_sample(window: int = 1, with_wrist: bool = False, with_tactile: bool = False, with_pc: bool = False, seed: int = 0):
    """One sample in the layout RLDSBatchTransform reads (vla/datasets/datasets.py:39-110)."""
    rng = np.random.default_rng(seed)
    img = lambda: rng.integers(0, 256, (1, 224, 224, 3), dtype=np.uint8)  # noqa: E731
    obs = {"image_primary": img(), "image_next_primary": img(), "proprio": rng.uniform(-1.2, 1.2, (window, 7)).astype(np.float32)}
    if with_wrist:
        obs["image_wrist_right"], obs["image_wrist_left"] = img(), img()
    if with_tactile:
        for k in ("tactile_right", "tactile_left", "next_tactile_right", "next_tactile_left"):
            t = rng.integers(0, 400, (1, 6)).astype(np.float32)
            t[0, rng.integers(0, 6)] = 65535
            obs[k] = t
        obs["gripper_xyz"] = rng.uniform(0, 1, (1, 3)).astype(np.float32)
    if with_pc:
        obs["point_cloud"] = rng.uniform(0, 1, (1, 64, 3)).astype(np.float32)
        obs["next_point_cloud"] = rng.uniform(0, 1, (1, 64, 3)).astype(np.float32)
    return {"dataset_name": b"rlbench", "action": rng.uniform(-1.3, 1.3, (window, 7)).astype(np.float32), "observation": obs,
            "task": {"language_instruction": b"Close The Jar <image> now"}, "action_mask": np.ones((window, 7), dtype=bool)}


RLDS_CASES = {"plain": dict(), "window3_wrist": dict(window=3, with_wrist=True), "tactile_pc": dict(with_tactile=True, with_pc=True),
              "no_action_tok": dict(), "no_stop": dict(window=2)}


def collator_batches(seed: int = 0) -> dict:
    """Instances for PaddedCollatorForActionPrediction (util/data_utils.py:88-196), model_max_length 12, pad id 512: three of
    lengths 9 / 14 / 5 (one padded, one truncated) without and with the tactile fields. {tactile: [instance, ...]}; the golden
    tests/golden/collator.npz holds the reference collator's output on exactly these (oracle/capture_golden_collator.py)."""
    g = torch.Generator().manual_seed(seed)

    def inst(n, tactile):
        d = dict(input_ids=torch.randint(3, 100, (n,), generator=g), labels=torch.randint(3, 100, (n,), generator=g),
                 images={"front_image": torch.randn(4, 8, 8, generator=g)}, next_images={"front_image": torch.randn(3, 8, 8, generator=g)},
                 point_cloud=torch.randn(16, 3, generator=g), next_point_cloud=torch.randn(16, 3, generator=g),
                 actions=torch.randn(1, 7, generator=g), action_masks=torch.ones(1, dtype=torch.bool), proprio=torch.randn(1, 7, generator=g),
                 dataset_name="rlbench")
        if tactile:
            d.update(tactile=torch.randn(12, generator=g), gripper_xyz=torch.randn(3, generator=g), next_tactile=torch.randn(12, generator=g))
        return d
    return {tactile: [inst(9, tactile), inst(14, tactile), inst(5, tactile)] for tactile in (False, True)}


def collator_to_arrays(out: dict, prefix: str) -> dict:
    """A collated batch as plain numpy arrays (no pickled objects): tensors as they are, dict fields per key, None as the string
    "None", lists as string arrays; `<prefix>::__keys__` lists the batch's keys."""
    res = {f"{prefix}::__keys__": np.array(sorted(out))}
    for k, v in out.items():
        if torch.is_tensor(v):
            res[f"{prefix}::{k}"] = v.numpy()
        elif isinstance(v, dict):
            for kk, t in v.items():
                res[f"{prefix}::{k}.{kk}"] = t.numpy()
        elif v is None:
            res[f"{prefix}::{k}"] = np.array("None")
        else:
            res[f"{prefix}::{k}"] = np.array([str(x) for x in v])
    return res
