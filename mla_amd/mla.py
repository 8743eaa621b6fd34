"""MLA wrapper (reference: models/mla/model_mla.py:47-309): diffusion branch of forward + wrap policy + freeze."""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

import torch
import torch.nn as nn

from .action_tokenizer import ActionTokenizer
from .diffusion import create_diffusion
from .prismatic import PrismaticVLM

IGNORE_INDEX = -100


class MLA(nn.Module):
    def __init__(self, vlm: PrismaticVLM, action_tokenizer: Optional[ActionTokenizer] = None, token_size: int = 4096,
                 action_dim: int = 7, future_action_window_size: int = 15, past_action_window_size: int = 0, use_ema: bool = False,
                 norm_stats=None, use_diff: bool = False, use_pointcloud: bool = False, use_tactile: bool = False,
                 use_contrastive: bool = False, use_generation: bool = False, gen_image: bool = False, use_roi: bool = False,
                 gen_pointcloud: bool = False, gen_tactile: bool = False, **kwargs) -> None:
        super().__init__()
        self.action_tokenizer = action_tokenizer
        self.use_diff, self.use_pointcloud, self.use_tactile = use_diff, use_pointcloud, use_tactile
        self.use_contrastive, self.use_generation = use_contrastive, use_generation
        self.gen_image, self.use_roi, self.gen_pointcloud, self.gen_tactile = gen_image, use_roi, gen_pointcloud, gen_tactile
        self.vlm = vlm
        self.future_action_window_size = future_action_window_size
        self.vlm.future_action_window_size = future_action_window_size
        self.past_action_window_size = past_action_window_size
        self.all_module_keys = ["vlm." + k for k in self.vlm.all_module_keys]
        if use_ema:
            raise NotImplementedError("use_ema is non-functional in the reference (no ema_diffusion is ever built, "
                                      "model_mla.py:47-97, 305-309); keep it False. A weight average of the trainable parameters "
                                      "is a strategy option here: FSDPStrategy(ema_decay=0.9999)")
        self.use_ema = use_ema
        self.norm_stats = norm_stats
        self._trainable_module_keys: List[str] = []
        self.last_diff_mse = None
        if self.use_diff:
            self.ddim_diffusion = None
            # round 6, opt-in: run the R diffusion copies of a sample as ONE [prefix | R suffix groups] sequence where the prefix does not depend
            # on the copy (PrismaticVLM.shared_prefix_ok(): the scripts/pretrain.sh configuration); see _forward_shared_prefix
            self.share_prefix = False
            # opt-in (round 6): in the diffusion branch only the action read-out rows of the final hidden state are read; with this
            # flag the last decoder layer computes its row-wise half (o_proj, MLP) on those rows alone (ops.ReadoutLayerFn)
            self.readout_rows_only = os.environ.get("MLA_READOUT_ROWS", "0") != "0"
            self.diffusion_steps = 100
            self.diffusion = create_diffusion(timestep_respacing="", noise_schedule="squaredcos_cap_v2", diffusion_steps=100,
                                              sigma_small=True, learn_sigma=False)

    @classmethod
    def from_pretrained(cls, action_tokenizer, pretrained_checkpoint, model_id: str, llm_backbone, enable_mixed_precision_training: bool = True,
                        arch_specifier: str = "gelu-mlp", freeze_weights: bool = True, action_dim: int = 7,
                        future_action_window_size: int = 15, past_action_window_size: int = 0, use_ema: bool = False, norm_stats=None,
                        class_dropout_prob: float = 0.0, use_diff: bool = False, use_pointcloud: bool = False, use_tactile: bool = False,
                        use_contrastive: bool = False, use_generation: bool = False, gen_image: bool = False, use_roi: bool = False,
                        gen_pointcloud: bool = False, gen_tactile: bool = False, **kwargs) -> "MLA":
        """model_mla.py:311-492: build the VLM, then load the per-module state dicts of a ``{"model": {...}}`` checkpoint with
        the reference's rules (missing optional modules keep their initialisation; the LLM loads non-strictly; embedders load
        only when their input width matches ``action_dim``; generation sub-modules load by key prefix)."""
        token_size = llm_backbone.llm.lm_head.in_features
        vlm = PrismaticVLM(model_id, llm_backbone, enable_mixed_precision_training=enable_mixed_precision_training,
                           class_dropout_prob=class_dropout_prob, use_diff=use_diff, action_dim=action_dim, token_size=token_size,
                           use_pointcloud=use_pointcloud, use_tactile=use_tactile, use_contrastive=use_contrastive,
                           use_generation=use_generation, gen_image=gen_image, use_roi=use_roi, gen_pointcloud=gen_pointcloud,
                           gen_tactile=gen_tactile, **kwargs)
        sd = torch.load(pretrained_checkpoint, map_location="cpu")["model"]
        loaded = []

        def load(name, module, strict=True):
            module.load_state_dict(sd[name], strict=strict)
            loaded.append(name)

        if "vision_tower_2d" in sd:
            load("vision_tower_2d", vlm.vision_tower_2d)
        if "projector_2d" in sd:
            load("projector_2d", vlm.projector_2d)
        if use_pointcloud and "vision_tower_3d" in sd:
            load("vision_tower_3d", vlm.vision_tower_3d)
        if use_pointcloud and "projector_3d" in sd:
            load("projector_3d", vlm.projector_3d)
        assert "llm_backbone" in sd, "PrismaticVLM `from_pretrained` expects checkpoint with keys for `llm_backbone`!"
        load("llm_backbone", vlm.llm_backbone, strict=False)
        if "proprio_embedder" in sd and sd["proprio_embedder"]["mlp.fc1.weight"].shape[-1] == action_dim:
            load("proprio_embedder", vlm.proprio_embedder)
        tactile_dim = 24 if action_dim == 14 else 12                                         # model_mla.py:405-409
        if use_tactile and "tactile_embedder" in sd and sd["tactile_embedder"]["mlp.fc1.weight"].shape[-1] == tactile_dim:
            load("tactile_embedder", vlm.tactile_embedder)
        if use_diff and all(k in sd for k in ("x_embedder", "t_embedder", "final_layer")):
            if sd["x_embedder"]["mlp.fc1.weight"].shape[-1] == action_dim:
                for k in ("x_embedder", "t_embedder", "final_layer"):
                    load(k, getattr(vlm, k))
        if use_generation and "generation_manager" in sd:
            for flag, sub in ((gen_image, "image_gen_module"), (gen_pointcloud, "pointcloud_gen_module"), (gen_tactile, "tactile_gen_module")):
                part = {k[len(sub) + 1:]: v for k, v in sd["generation_manager"].items() if k.startswith(sub + ".")}
                if flag and part:
                    getattr(vlm.generation_manager, sub).load_state_dict(part)
                    loaded.append("generation_manager." + sub)
        if freeze_weights:
            vlm.requires_grad_(False)
            vlm.eval()
        model = cls(vlm, action_tokenizer, token_size=token_size, action_dim=action_dim,
                    future_action_window_size=future_action_window_size, past_action_window_size=past_action_window_size, use_ema=use_ema,
                    norm_stats=norm_stats, use_diff=use_diff, use_pointcloud=use_pointcloud, use_tactile=use_tactile,
                    use_contrastive=use_contrastive, use_generation=use_generation, gen_image=gen_image, use_roi=use_roi,
                    gen_pointcloud=gen_pointcloud, gen_tactile=gen_tactile)
        model.loaded_module_keys = loaded
        return model

    @property
    def trainable_module_keys(self) -> List[str]:
        return ["vlm." + k for k in self.vlm.trainable_module_keys] + self._trainable_module_keys

    @property
    def llm_backbone(self):
        return self.vlm.llm_backbone

    def freeze_backbones(self, stage):
        self.vlm.freeze_backbones(stage)

    def get_fsdp_wrapping_policy(self) -> Callable:
        """model_mla.py:279-303 (same class sets as the VLM's policy)."""
        return self.vlm.get_fsdp_wrapping_policy()

    def forward(self, input_ids=None, attention_mask=None, images=None, next_images=None, camera_name=None, point_cloud=None,
                next_point_cloud=None, tactile=None, next_tactile=None, labels=None, actions=None, proprio=None, gripper_xyz=None,
                inputs_embeds=None, past_key_values=None, use_cache=None, output_attentions=None, output_hidden_states=None,
                return_dict=None, repeated_diffusion_steps: int = 4, action_masks=None, use_diff: Optional[bool] = None,
                noise: Optional[torch.Tensor] = None, timestep: Optional[torch.Tensor] = None) -> Tuple[Dict, object]:
        """model_mla.py:118-234. ``noise`` / ``timestep`` (not in the reference signature) let tests inject the random
        draws; when omitted they are drawn in the reference's order: randn_like(actions_future) then randint (:178-179)."""
        if use_diff is not None:
            self.use_diff = use_diff
        if not self.use_diff:
            raise NotImplementedError("the autoregressive branch is dead code in the reference (SURVEY Appendix A #15)")
        R = repeated_diffusion_steps
        rep = lambda v: v.repeat(R, *([1] * (v.ndimension() - 1)))  # noqa: E731
        if getattr(self, "share_prefix", False) and R > 1 and self.training and self.vlm.shared_prefix_ok():
            return self._forward_shared_prefix(input_ids, attention_mask, images, camera_name, labels, actions, proprio, R, noise, timestep)
        self.vlm.readout_rows_only = bool(getattr(self, "readout_rows_only", False))
        proprio = rep(proprio)
        actions = rep(actions)
        actions_future = actions[:, -(self.future_action_window_size + 1):, :]
        input_ids, attention_mask, labels = rep(input_ids), rep(attention_mask), rep(labels)
        if action_masks is not None:
            action_masks = rep(action_masks)
        images = {k_: rep(v) for k_, v in images.items()} if isinstance(images, dict) else rep(images)
        if self.use_generation and self.gen_image:
            next_images = rep(next_images)
        if self.use_pointcloud:
            point_cloud = rep(point_cloud)
        if self.use_pointcloud and self.use_generation and self.gen_pointcloud:
            next_point_cloud = rep(next_point_cloud)
        if self.use_tactile:                                              # model_mla.py:172-176
            tactile, gripper_xyz = rep(tactile), rep(gripper_xyz)
        if self.use_generation and self.gen_tactile:                     # (the reference tiles it only when use_tactile is set too)
            next_tactile = rep(next_tactile)
        if noise is None:
            noise = torch.randn_like(actions_future)
        if timestep is None:
            timestep = torch.randint(0, self.diffusion.num_timesteps, (actions_future.size(0),), device=actions.device)
        x = self.diffusion.q_sample(actions_future, timestep, noise)

        self.vlm.image_repeat_hint = R
        try:
            output, noise_pred, generation_outputs, generation_losses = self.vlm(
                input_ids=input_ids, attention_mask=attention_mask, images=images, next_images=next_images,
                camera_name=camera_name, point_cloud=point_cloud if self.use_pointcloud else None,
                next_point_cloud=next_point_cloud, tactile=tactile, next_tactile=next_tactile, labels=labels, x=x, t=timestep,
                proprio=proprio, gripper_xyz=gripper_xyz, use_cache=use_cache, output_attentions=output_attentions,
                output_hidden_states=output_hidden_states, return_dict=return_dict, use_diff=self.use_diff)
        finally:
            self.vlm.image_repeat_hint = 1
        assert noise_pred.shape == noise.shape == actions_future.shape
        zero = lambda: torch.tensor(0, dtype=torch.float32)  # noqa: E731
        loss_dict = {"total_loss": zero(), "img_pc_contrastive_loss": zero(), "tactile_contrastive_loss": zero(),
                     "diff_loss": zero(), "image_gen_loss": zero(), "point_cloud_gen_loss": zero(), "tactile_gen_loss": zero()}
        diff_loss = ((noise_pred.float() - noise.float()) ** 2).mean()
        self.last_diff_mse = diff_loss.detach().clone()
        total = diff_loss
        if self.use_generation and self.gen_image:                       # model_mla.py:218-223 (generation terms come first)
            loss_dict["image_gen_loss"] = generation_losses["image_gen_loss"]
            total = total + generation_losses["image_gen_loss"].float()
        if self.use_generation and self.gen_pointcloud:
            loss_dict["point_cloud_gen_loss"] = generation_losses["point_cloud_gen_loss"]
            total = total + generation_losses["point_cloud_gen_loss"].float()
        if self.use_generation and self.gen_tactile:
            loss_dict["tactile_gen_loss"] = generation_losses["tactile_gen_loss"]
            total = total + generation_losses["tactile_gen_loss"].float()
        if self.use_contrastive:
            loss_dict["img_pc_contrastive_loss"] = output.img_pc_contrastive_loss
            total = total + output.img_pc_contrastive_loss.float()
            if self.use_tactile:
                loss_dict["tactile_contrastive_loss"] = output.tactile_contrastive_loss
                total = total + output.tactile_contrastive_loss.float()
        # the reference's `total_loss` and `diff_loss` are one tensor mutated in place (model_mla.py:215-229), so the
        # reported diff_loss equals total_loss; the true diffusion MSE is kept in self.last_diff_mse
        loss_dict["total_loss"] = total
        loss_dict["diff_loss"] = total
        return loss_dict, output

    def _forward_shared_prefix(self, input_ids, attention_mask, images, camera_name, labels, actions, proprio, R, noise, timestep):
        """Opt-in (`mla.share_prefix = True`; round 6): the diffusion branch without tiling the sample R times. Only the actions are
        tiled -- noise and timesteps are drawn exactly like in forward() (randn_like(actions_future) then randint, :178-179), so the
        same RNG stream gives the same x_t per copy -- and PrismaticVLM.forward_shared_prefix runs [prefix | R suffix groups] once per
        sample. The loss dict is forward()'s for this configuration (no contrastive / generation terms); `output` is in the shared
        layout."""
        rep = lambda v: v.repeat(R, *([1] * (v.ndimension() - 1)))  # noqa: E731
        actions_future = rep(actions)[:, -(self.future_action_window_size + 1):, :]
        if noise is None:
            noise = torch.randn_like(actions_future)
        if timestep is None:
            timestep = torch.randint(0, self.diffusion.num_timesteps, (actions_future.size(0),), device=actions.device)
        x = self.diffusion.q_sample(actions_future, timestep, noise)
        self.vlm.image_repeat_hint = 1
        output, noise_pred = self.vlm.forward_shared_prefix(x, timestep, R, proprio, input_ids, attention_mask, images, camera_name, labels)
        assert noise_pred.shape == noise.shape == actions_future.shape
        zero = lambda: torch.tensor(0, dtype=torch.float32)  # noqa: E731
        loss_dict = {"total_loss": zero(), "img_pc_contrastive_loss": zero(), "tactile_contrastive_loss": zero(),
                     "diff_loss": zero(), "image_gen_loss": zero(), "point_cloud_gen_loss": zero(), "tactile_gen_loss": zero()}
        total = ((noise_pred.float() - noise.float()) ** 2).mean()
        self.last_diff_mse = total.detach().clone()
        loss_dict["total_loss"] = total
        loss_dict["diff_loss"] = total
        return loss_dict, output

    # ------------------------------------------------------------------------------------------ inference
    def create_ddim(self, ddim_step=10, noise_schedule="squaredcos_cap_v2", diffusion_steps=100):
        """model_mla.py:1166-1173."""
        self.ddim_diffusion = create_diffusion(timestep_respacing="ddim" + str(ddim_step), noise_schedule=noise_schedule,
                                               diffusion_steps=diffusion_steps, sigma_small=True, learn_sigma=False)
        return self.ddim_diffusion

    @staticmethod
    def _check_unnorm_key(norm_stats, unnorm_key):
        if unnorm_key is None:
            assert len(norm_stats) == 1, ("Your model was trained on more than one dataset, please pass a `unnorm_key` from the "
                                          f"following options to choose the statistics used for un-normalizing actions: {norm_stats.keys()}")
            unnorm_key = next(iter(norm_stats.keys()))
        assert unnorm_key in norm_stats, f"The `unnorm_key` you chose is not in the set of available dataset statistics, please choose from: {norm_stats.keys()}"
        return unnorm_key

    def get_action_dim(self, unnorm_key=None):
        return len(self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]["q01"])

    def get_proprio_stats(self, unnorm_key=None):
        return self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["proprio"]

    def get_action_stats(self, unnorm_key=None):
        return self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]

    def normalize_proprio(self, cur_robot_state, unnorm_key=None) -> np.ndarray:
        """model_mla.py:667-677: q01/q99 -> [-1, 1] on the masked dimensions, clipped."""
        st = self.get_proprio_stats(unnorm_key)
        mask = st.get("mask", np.ones_like(st["q01"], dtype=bool))
        hi, lo = np.array(st["q99"]), np.array(st["q01"])
        return np.clip(np.where(mask, 2 * (cur_robot_state - lo) / (hi - lo + 1e-8) - 1, cur_robot_state), -1, 1)

    def unnormalize_actions(self, normalized_actions: np.ndarray, unnorm_key=None) -> np.ndarray:
        """model_mla.py:679-704: clip to [-1, 1], binarise the gripper channel(s) at 0.5, map back through q01/q99."""
        st = self.get_action_stats(unnorm_key)
        mask = st.get("mask", np.ones_like(st["q01"], dtype=bool))
        hi, lo = np.array(st["q99"]), np.array(st["q01"])
        a = np.clip(normalized_actions, -1, 1)
        width = a.shape[-1] if a.ndim >= 1 else 0
        for g in ((6,) if width == 7 else (6, 13) if width == 14 else ()):
            a[..., g] = np.where(a[..., g] < 0.5, 0, 1)
        return np.where(mask, 0.5 * (a + 1) * (hi - lo) + lo, a)

    def normalize_actions(self, actions, unnorm_key=None) -> np.ndarray:
        """The inverse of unnormalize_actions (no counterpart in model_mla.py; the form of normalize_proprio): on the masked dimensions
        2 (a - q01) / (q99 - q01 + 1e-8) - 1, clipped to [-1, 1]; the other dimensions pass through (a binarised gripper channel stays
        0 / 1 and comes back as it is). Without ``norm_stats`` it is the identity, like the return path of predict_action_diff. The round
        trip through unnormalize_actions returns a - 1e-8 (a - q01) / (q99 - q01 + 1e-8) on a masked dimension, for q01 <= a <= q99."""
        a = np.asarray(actions)
        if self.norm_stats is None:
            return a
        st = self.get_action_stats(unnorm_key)
        mask = st.get("mask", np.ones_like(st["q01"], dtype=bool))
        hi, lo = np.array(st["q99"]), np.array(st["q01"])
        return np.where(mask, np.clip(2 * (a - lo) / (hi - lo + 1e-8) - 1, -1, 1), a)

    # ---- known_actions of the four sampling entry points: validated before the model is touched, then one (known, mask) pair per call
    @staticmethod
    def _known_entry(entry, T, action_dim, who="known_actions"):
        """One observation's known actions -> float64 [d, action_dim] (None stays None); ValueError for anything else."""
        if entry is None:
            return None
        try:
            a = np.asarray(entry.detach().cpu().numpy() if torch.is_tensor(entry) else entry, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{who}: not a numeric array [d, {action_dim}]: {e}") from None
        if a.ndim != 2 or a.shape[1] != action_dim or not 1 <= a.shape[0] <= T:
            raise ValueError(f"{who} must be [d, action_dim] = [1..{T}, {action_dim}] (the first d steps of the chunk), got {tuple(a.shape)}")
        if not np.isfinite(a).all():
            raise ValueError(f"{who} has non-finite values")
        return a

    @staticmethod
    def _known_entries(known_actions, B, T, action_dim):
        """predict_action_diff_batch's known_actions -> a list of B validated entries (None: B times None)."""
        if known_actions is None:
            return [None] * B
        if (isinstance(known_actions, np.ndarray) or torch.is_tensor(known_actions)) and known_actions.ndim == 3:
            known_actions = list(known_actions)                                # a stacked [B, d, action_dim] array: the same d everywhere
        if not isinstance(known_actions, (list, tuple)) or len(known_actions) != B:
            raise ValueError(f"known_actions must be a list with one entry ([d, action_dim] or None) per observation, {B} here")
        return [MLA._known_entry(k, T, action_dim, f"known_actions[{b}]") for b, k in enumerate(known_actions)]

    @staticmethod
    def _fwd_known(entry):
        """The keyword of a call that ends in another public method: handed on only when given."""
        return {} if entry is None else {"known_actions": entry}

    def _pin(self, entries, T, action_dim, unnorm_key, device, repeat=1):
        """Validated entries, one per observation -> None (nothing known) or (known [B * repeat, T, action_dim] fp32, mask bool) on
        `device`: chunk steps 0 .. d - 1 of observation b hold its entry in the sampler's (normalised) units, each observation's rows
        `repeat` times (the N chunks of an observation share what is known)."""
        if all(e is None for e in entries):
            return None
        known = np.zeros((len(entries), T, action_dim), dtype=np.float32)
        mask = np.zeros((len(entries), T, action_dim), dtype=bool)
        for b, e in enumerate(entries):
            if e is not None:
                known[b, :e.shape[0]] = MLA.normalize_actions(self, e, unnorm_key)
                mask[b, :e.shape[0]] = True
        known, mask = torch.from_numpy(known).to(device), torch.from_numpy(mask).to(device)
        if repeat != 1:
            known, mask = known.repeat_interleave(repeat, dim=0), mask.repeat_interleave(repeat, dim=0)
        return known.contiguous(), mask.contiguous()

    # ---- the per-sample preprocessing of predict_action_diff, shared with predict_action_diff_batch
    def _prompt_ids(self, instruction, who):
        # :626-632 -- prompt text from the backbone's builder, ids from the backbone's tokenizer (the Llama tokenizer files are not
        # in this image: attach one as vlm.llm_backbone.tokenizer, or pass input_ids)
        tokenizer = getattr(self.vlm.llm_backbone, "tokenizer", None)
        if instruction is None or tokenizer is None or not callable(tokenizer):
            raise ValueError(f"{who} needs `input_ids`, or `instruction` plus a callable vlm.llm_backbone.tokenizer")
        builder = self.vlm.llm_backbone.prompt_builder_fn("openvla")
        builder.add_turn(role="human", message=f"What action should the robot take to {instruction.lower()}?")
        return tokenizer(builder.get_prompt(), truncation=True, return_tensors="pt").input_ids

    @staticmethod
    def _check_cfg_scale(cfg_scale):
        if cfg_scale > 1.0:
            raise NotImplementedError("classifier-free guidance: the reference calls self.vlm.forward_with_cfg (model_mla.py:718-729), which "
                                      "PrismaticVLM does not define -- cfg_scale > 1 raises there too; the shipped evaluation uses cfg_scale=0")

    def _preprocessed_image(self, image):
        if not (torch.is_tensor(image) and image.is_floating_point()):
            # PIL image / uint8 HWC frame: the reference's CLIPImageProcessor step (:656-657), PIL-exact on the GPU
            image = self.vlm.get_vision_tower_2d().image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0]
        return image

    @staticmethod
    def _ids_with_tail(input_ids, device):
        from .infer import PROMPT_TAIL, SPLICE_TAG
        input_ids = input_ids.to(device)
        if not bool(torch.all(input_ids[:, -1] == SPLICE_TAG)):
            tail = torch.tensor([PROMPT_TAIL], dtype=torch.long, device=device)
            input_ids = torch.cat((input_ids, tail), dim=1)[:, :-3]
        return input_ids

    @staticmethod
    def _image_batch(image, device):
        img = image.to(device)
        if img.dim() == 3:
            img = img.unsqueeze(0)
        if img.shape[1] == 3:
            img = torch.cat([img, torch.ones_like(img[:, :1])], dim=1)
        return img

    @staticmethod
    def _pointcloud_batch(pointcloud, device):
        if isinstance(pointcloud, np.ndarray):
            pointcloud = torch.from_numpy(pointcloud)
        if pointcloud is not None:
            pointcloud = pointcloud.to(device).contiguous()
            if pointcloud.dim() == 2:
                pointcloud = pointcloud.unsqueeze(0)
        return pointcloud

    def _proprio_token(self, cur_robot_state, unnorm_key, device):
        if cur_robot_state is None:
            raise ValueError("cur_robot_state is required: the proprio token is always spliced in (prismatic.py:985-990)")
        st = self.normalize_proprio(np.asarray(cur_robot_state), unnorm_key) if self.norm_stats is not None else np.asarray(cur_robot_state)
        return torch.tensor(st, dtype=torch.float32).reshape(1, 1, -1).to(device)

    # ---- what the four sampling entry points share (their mode keywords: infer.Modes, validated by infer.check_modes before `self` is
    # touched)
    def _draw_x0(self, given, T, action_dim, device):
        """The initial samples [len(given), T, action_dim] fp32 and the RNG draws of one predict_action_diff call per chunk, in call order
        (:707-708): randn(1, T, D) unless the chunk's noise row [1, T, D] is given, then the unused randint."""
        draws = []
        for noise in given:
            draws.append(torch.randn(1, T, action_dim, device=device) if noise is None else noise.to(device))
            _ = torch.randint(0, self.diffusion.num_timesteps, (T,), device=device)
        return torch.cat(draws, dim=0).float()

    SOLVERS = ("ddim", "dpmpp2m")

    @staticmethod
    def _check_solver(solver, use_ddim, num_ddim_steps):
        """``solver`` of the sampling entry points, validated before the model is touched: never silently ignored, never a silent DDIM."""
        if solver not in MLA.SOLVERS:
            raise ValueError(f"solver={solver!r}: unknown value, choose from {MLA.SOLVERS}")
        if solver != "ddim" and not (use_ddim and num_ddim_steps is not None):
            raise ValueError(f"solver={solver!r} runs the respaced process of the DDIM sampler (use_ddim=True and num_ddim_steps); this "
                             "call runs the DDPM loop of the training diffusion, which has no deterministic solver")

    @staticmethod
    def _fwd_solver(solver):
        """The keyword of a call that ends in another public method: handed on only when it is not the default (as _fwd_known)."""
        return {} if solver == "ddim" else {"solver": solver}

    def _sample(self, eps_model, x0, sampler, use_ddim, num_ddim_steps, model_kwargs, ddpm_sampler="host", pin=None, solver="ddim"):
        """x0 [B, T, D] -> samples: the DDIM loop (eta = 0) on the device (an engine's sample_ddim) or on the host, solver "dpmpp2m" the
        DPM-Solver++(2M) loop over the same respaced process on the device (sample_dpmpp2m) or on the host (dpmpp2m_sample_loop), or
        the DDPM loop of the training diffusion on the device (sample_ddpm) or on the host. pin = (known, mask) shaped like x0 (see
        _pin): the device loops' pin=, the host loops' denoised_fn = where(mask, known, .); None is the call without it."""
        device = x0.device
        on_device = {} if pin is None else {"pin": pin}
        on_host = {} if pin is None else {"denoised_fn": lambda px: torch.where(pin[1], pin[0], px)}
        MLA._check_solver(solver, use_ddim, num_ddim_steps)
        if use_ddim and num_ddim_steps is not None:
            if self.ddim_diffusion is None:
                self.create_ddim(ddim_step=num_ddim_steps)
            if solver == "dpmpp2m":
                if sampler == "device":
                    return eps_model.sample_dpmpp2m(x0, self.ddim_diffusion, **on_device)
                return self.ddim_diffusion.dpmpp2m_sample_loop(eps_model, x0.shape, x0, clip_denoised=False, model_kwargs=model_kwargs,
                                                               progress=False, device=device, **on_host)
            if sampler == "device":
                return eps_model.sample_ddim(x0, self.ddim_diffusion, **on_device)
            return self.ddim_diffusion.ddim_sample_loop(eps_model, x0.shape, x0, clip_denoised=False, model_kwargs=model_kwargs,
                                                        progress=False, device=device, eta=0.0, **on_host)
        if ddpm_sampler == "device":
            return eps_model.sample_ddpm(x0, self.diffusion, **on_device)
        return self.diffusion.p_sample_loop(eps_model, x0.shape, x0, clip_denoised=False, model_kwargs=model_kwargs, progress=False,
                                            device=device, **on_host)

    @staticmethod
    def _pin_rows(pin, start, stop):
        """The rows [start, stop) of a call's (known, mask) pair for one pass or sub-batch."""
        return None if pin is None else (pin[0][start:stop].contiguous(), pin[1][start:stop].contiguous())

    def _actions(self, chunks, unnorm_key):
        """The sampled chunks of a call, in order (numpy, stacked on axis 0) -> un-normalised actions."""
        normalized = np.concatenate(chunks, axis=0)
        return self.unnormalize_actions(normalized, unnorm_key) if self.norm_stats is not None else normalized

    def _batch_prompts(self, B, instructions, input_ids, pointclouds, cur_robot_states):
        """The argument checks of a batched call -> (input_ids, pointclouds), one entry per observation each. Called as
        MLA._batch_prompts(self, ...): the host tests reach these errors with a stand-in `self` that has no methods of its own."""
        if input_ids is None:
            if instructions is None or len(instructions) != B:
                raise ValueError("predict_action_diff_batch needs `input_ids` (one tensor per sample), or B `instructions` plus a callable "
                                 "vlm.llm_backbone.tokenizer")
            input_ids = [self._prompt_ids(ins, "predict_action_diff_batch") for ins in instructions]
        if pointclouds is None:
            pointclouds = [None] * B
        if not (len(input_ids) == B and len(pointclouds) == B and cur_robot_states is not None and len(cur_robot_states) == B):
            raise ValueError("predict_action_diff_batch: images, pointclouds, cur_robot_states and input_ids / instructions need one entry per sample")
        return input_ids, pointclouds

    def _batch_inputs(self, images, pointclouds, cur_robot_states, ids_rows, unnorm_key, camera_name):
        """B observations stacked for an engine's for_batch -> (device, prompt id lists, its keyword arguments). Every per-sample step is
        predict_action_diff's; the prompt tail per row is infer.plan_batch's (:640-645)."""
        self.vlm.eval()
        device = next(self.vlm.parameters()).device
        pre = [self._preprocessed_image(im) for im in images]
        ids_rows = [ids.reshape(-1).tolist() for ids in ids_rows]
        img = torch.cat([self._image_batch(im, device) for im in pre], dim=0)
        pcs = [self._pointcloud_batch(pc, device) for pc in pointclouds]
        pc = None if any(p is None for p in pcs) else torch.cat(pcs, dim=0)
        proprio = torch.cat([self._proprio_token(st, unnorm_key, device) for st in cur_robot_states], dim=0)
        return device, ids_rows, {"images": img, "point_cloud": pc, "camera_name": camera_name, "proprio": proprio}

    @torch.inference_mode()
    def predict_action_diff(self, image=None, pointcloud=None, instruction: Optional[str] = None, cur_robot_state=None,
                            unnorm_key: Optional[str] = None, cfg_scale: float = 0.0, use_ddim: bool = True, num_ddim_steps: int = 8,
                            action_dim: int = 7, *, input_ids: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                            camera_name: str = "rlbench_front", reuse_prefix: bool = True, suffix_weights: str = "bf16",
                            prefill: str = "train", sampler: str = "host", suffix_attention: str = "head",
                            prefill_precision: str = "bf16", ddpm_sampler: str = "host", suffix_operand: str = "fused",
                            known_actions=None, suffix_mx: str = "off", solver: str = "ddim", **kwargs) -> np.ndarray:
        """model_mla.py:592-775: 8-step DDIM (eta = 0) over the action chunk with the VLM as the epsilon model, then
        un-normalisation.
        * ``image`` is a PIL image / uint8 HWC frame (pre-processed here like the reference does, :656-660) or an already
          pre-processed float tensor [3|4, 672, 672]; a ones mask channel is appended when missing;
        * the prompt is built from ``instruction`` with the backbone's prompt builder and tokenizer like the reference does
          (:626-632; the Llama tokenizer files are not in this image, so a tokenizer has to be attached), or arrives tokenised as
          ``input_ids`` [1, L]; [29871, 32001, 32002, 29871] is appended unless the last id already is 29871 and the last three ids
          are dropped again (:640-645, :711-713).
        ``reuse_prefix`` (default, round 6): the encoders and the decoder rows in front of the [t, x] tokens are computed ONCE per action
        chunk and every sampler step runs over the 1 + T suffix rows against the cached keys / values (mla_amd/infer.py: same function,
        FPS start indices drawn once per chunk instead of once per step); False = the reference's control flow, a whole forward per step.
        ``noise`` optionally fixes the initial sample (the reference draws it with torch.randn, :707). ``camera_name``: the shipped
        method does not forward it, so the reference's get_camera_params(None) raises (camera.py:54-56); it is an explicit
        argument here (the evaluation scripts use the RLBench front camera).
        ``suffix_weights`` (opt-in, cached prefix only): "bf16" (default) | "fp8": the sampler steps stream a per-row e4m3fn copy of the
        decoder weights (mla_gemv_w8 / mla_gemm_skinny_w8: half the bytes per step; the prefill keeps the bf16 weights) | "fp8_as_bf16":
        the bf16 kernels on the dequantised copy -- what the format costs on a checkpoint, without the FP8 kernels. Anything but "bf16"
        raises when the cached prefix is off or does not serve the shape: there is no silent bf16 fallback.
        ``prefill`` (opt-in, cached prefix only): "train" (default) runs the prefix rows on the training kernels; "compact" on the
        row-sized GEMMs of mla_amd/csrc/prefill.hip (q|k|v + RoPE written straight into the cache, gate|up + SwiGLU writing the product
        only): the same function up to summation order and rounding points. "compact" raises ValueError when ``reuse_prefix=False``, the
        cached-prefix engine does not serve the shape, the prefix has more than 1024 rows or head_dim is not 128: no silent fallback.
        ``sampler`` (opt-in, cached prefix only): "host" (default) runs the reference's DDIM loop in torch expressions on the host;
        "device" keeps the loop on the device (mla_amd/infer.py:_CachedEpsBase.sample_ddim): one captured sampler step replayed
        ``num_ddim_steps`` times with the step index in device memory, no copy to the device and no host wait between the steps, the same
        bits. It composes with every ``suffix_weights`` and ``prefill`` mode; it raises ValueError when ``reuse_prefix=False``, the
        cached-prefix engine does not serve the shape, ``use_ddim=False`` or ``num_ddim_steps=None`` (the DDPM loop has its own keyword,
        ``ddpm_sampler``), and for an unknown value.
        ``ddpm_sampler`` (opt-in, cached prefix only): who runs the DDPM loop of ``use_ddim=False`` / ``num_ddim_steps=None`` (the 100-step
        p_sample_loop of the training diffusion). "host" (default) runs it in torch expressions on the host, with a device wait in every
        step; "device" keeps it on the device (mla_amd/infer.py:_CachedEpsBase.sample_ddpm): the steps' randn_like draws are enqueued up
        front, in the host loop's order, into a device table, then one captured sampler step (its update is mla_ddpm_step) is replayed
        once per step with the step index in device memory -- no copy to the device, no host wait between the steps, the same bits and
        the same generator position afterwards. It composes with every ``suffix_weights``, ``prefill``, ``prefill_precision`` and
        ``suffix_attention`` mode; it raises ValueError when ``reuse_prefix=False``, the cached-prefix engine does not serve the shape,
        the call runs the DDIM sampler (``use_ddim=True`` with ``num_ddim_steps``: the keyword is never silently ignored), and for an
        unknown value.
        ``suffix_attention`` (opt-in, cached prefix only): "head" (default) runs the sampler steps' attention as one workgroup per (head,
        16 queries) (mla_attn_decode / mla_attn_chunk); "split" cuts every head's key range over several workgroups and merges the partial
        softmax states in a fixed order with a second launch (mla_attn_chunk_split with the library's plan): the same function up to
        summation order. It composes with every ``suffix_weights``, ``prefill`` and ``sampler`` mode; it raises ValueError for an unknown
        value, and for "split" when ``reuse_prefix=False`` or the cached-prefix engine does not serve the shape: no silent fallback.
        ``prefill_precision`` (opt-in, ``prefill="compact"`` only): "bf16" (default) | "fp8": the four projections of every prefill layer
        run over e4m3fn codes of BOTH operands on the K = 128 MFMA (mla_amd/csrc/prefill.hip) -- the model's FP8 weight copy (one per
        model, shared with ``suffix_weights="fp8"``) and the projection inputs quantised per row; attention, cache and residual stream
        stay bf16 | "fp8_as_bf16": the bf16 compact kernels on the dequantised weight codes and on quantised-and-dequantised inputs --
        the same function as "fp8" up to rounding, and what the format costs on a checkpoint. The effect on a trained policy is not
        measured. It composes with every ``suffix_weights``, ``sampler`` and ``suffix_attention`` mode; it raises ValueError for an
        unknown value and for anything but "bf16" unless ``prefill="compact"`` (hence also when ``reuse_prefix=False``): there is never
        a silent bf16 prefill.
        ``suffix_operand`` (opt-in, cached prefix only): how a sampler step over MORE than 8 suffix rows (window >= 8) forms the RMSNorm
        and SwiGLU operands of its projections. "fused" (default): inside the projections' input staging (mla_gemm_skinny_* pre 1 / 2),
        five launches per layer, every workgroup re-forms the operand. "once": each RMSNorm operand once per pass by the stand-alone
        kernel, every projection on the plain skinny form, SwiGLU in the gate|up projection's epilogue
        (mla_gemm_skinny_gateup_swiglu_*: the packed gate|up rows never reach memory) -- seven launches per layer, the same bits as
        "fused". Up to 8 suffix rows both values run the same pass (the GEMV stages its input once per workgroup already). It composes
        with every ``suffix_weights``, ``suffix_attention``, ``sampler``, ``ddpm_sampler``, ``prefill`` and ``prefill_precision`` mode; it
        is validated in front of every other mode and raises ValueError for an unknown value, and for "once" when ``reuse_prefix=False``
        or the cached-prefix engine does not serve the shape: no silent fallback.
        ``suffix_mx`` (opt-in, cached prefix only): "off" (default) | "fp4": the sampler steps stream the model's OCP MXFP4 copy of the
        decoder weights (e2m1 codes with one e8m0 scale byte per 32 elements of a weight row; mla_gemv_w4 / mla_gemm_skinny_w4 /
        mla_gemm_suffix_w4: a quarter of the bf16 bytes per step, decoded exactly in registers; the prefill keeps the bf16 weights) |
        "fp4_as_bf16": the bf16 kernels on the dequantised copy -- the same function as "fp4" up to summation order, and what the
        format costs on a checkpoint, without the 4-bit kernels. The weight error of the format is a 4-bit one: relative Frobenius error
        0.11 on Gaussian weights (round to nearest), against 0.012 for ``suffix_weights="fp8"``; the effect on a trained policy is not
        measured. It composes with every ``sampler``, ``ddpm_sampler``, ``suffix_attention`` / ``groups_attention``, ``suffix_operand``,
        ``prefill`` and ``prefill_precision`` mode and with ``known_actions``; together with ``suffix_weights`` other than "bf16" it
        raises ValueError (both choose what the suffix pass streams), as it does for an unknown value, when ``reuse_prefix=False`` and
        when the cached-prefix engine does not serve the shape: no silent fallback.
        ``known_actions`` (default None: the call without the keyword, bit for bit): an array [d, action_dim], 1 <= d <= T, in the units
        of the return value -- the first d steps of this chunk are already decided (the robot is executing them while this call runs) and
        the sampler pins them: in every sampler step the x0 prediction of chunk steps 0 .. d - 1 is replaced by the given values
        (normalize_actions of them when the model has ``norm_stats``: values outside [q01, q99] are clipped as the return path clips),
        the reference's ``denoised_fn`` hook (gaussian_diffusion.py:318-321) used as replacement inpainting; the keyword itself has no
        counterpart in model_mla.py. The initial sample is the call's noise on the pinned rows too, every draw is the un-pinned call's,
        and the sampled normalised chunk equals the given values on the pinned entries exactly; the free steps see them only through
        the model's attention over the chunk rows. Indexing: when the previous chunk was sampled from an observation taken k control
        steps ago, new chunk step j is old chunk step j + k, so ``known_actions = old_chunk[k:k + d]``. It composes with every mode
        keyword, with ``sampler`` / ``ddpm_sampler`` "host" and "device" (mla_ddim_step_pin / mla_ddpm_step_pin on a captured step of
        its own) and with ``reuse_prefix=False`` (the host loop with ``denoised_fn``). A wrong shape, d > T or non-finite values raise
        ValueError before the model is touched. What pinning does to a trained policy is not measured.
        ``solver`` (default "ddim": the call without the keyword, bit for bit -- the same launches, the same captured step, the same
        generator position): which deterministic solver walks the respaced process of ``num_ddim_steps`` steps. "dpmpp2m":
        DPM-Solver++(2M) (Lu et al. 2022; no counterpart in model_mla.py), the second-order multistep solver in its data-prediction
        form -- one model call per step like DDIM, the previous step's x0 prediction reused, the last step first order
        (GaussianDiffusion.dpmpp2m_sample_loop is the definition; its coefficients are formed in float64 from the process's
        alphas_cumprod). On an analytic Gaussian model four 2M steps are closer to the exact solution than eight DDIM steps
        (profiles/solver_dpmpp_error.txt), which is what it is for: fewer suffix passes per chunk (``create_ddim(ddim_step=4)`` in
        front of the call, as for any other step count). The effect on a trained policy is not measured. It runs on the host loop
        (``reuse_prefix=False`` and the warned whole-forward fallback included) and, with ``sampler="device"``, on the device
        (sample_dpmpp2m: a state and a captured step of its own, mla_dpmpp2m_step[_pin], the host loop's bits); it draws nothing in the
        loop, so the generator stays where the initial draw left it (DDIM's unused randn_like per step is DDIM's). It composes with
        every mode keyword and with ``known_actions`` (the pinned entries come back exactly). An unknown value, and "dpmpp2m" with
        ``use_ddim=False`` or ``num_ddim_steps=None``, raise ValueError before the model is touched: there is never a silent DDIM."""
        from .infer import Modes, PrefixCachedEps, check_modes, needs_engine
        check_modes(Modes(suffix_weights=suffix_weights, prefill=prefill, suffix_attention=suffix_attention, prefill_precision=prefill_precision,
                          suffix_operand=suffix_operand, sampler=sampler, ddpm_sampler=ddpm_sampler, suffix_mx=suffix_mx),
                    reuse_prefix, use_ddim, num_ddim_steps)
        MLA._check_solver(solver, use_ddim, num_ddim_steps)
        if prefill != "train" and not reuse_prefix:
            raise ValueError(f"prefill={prefill!r} needs the cached-prefix engine (reuse_prefix=True); the whole-forward sampler has no "
                             "separate prefill")
        T = self.future_action_window_size + 1
        known_actions = MLA._known_entry(known_actions, T, action_dim)
        self.vlm.eval()
        device = next(self.vlm.parameters()).device
        if input_ids is None:
            input_ids = self._prompt_ids(instruction, "predict_action_diff")
        self._check_cfg_scale(cfg_scale)
        image = self._preprocessed_image(image)
        input_ids = self._ids_with_tail(input_ids, device)
        img = self._image_batch(image, device)
        pointcloud = self._pointcloud_batch(pointcloud, device)
        model_kwargs = {"input_ids": input_ids, "images": img, "point_cloud": pointcloud, "camera_name": camera_name}
        model_kwargs["proprio"] = self._proprio_token(cur_robot_state, unnorm_key, device)
        x0 = self._draw_x0([noise], T, action_dim, device)
        eps_model = self.vlm.forward
        if reuse_prefix:
            reuse_prefix = PrefixCachedEps.supports(self.vlm, int(input_ids.shape[0]), T)
        if suffix_weights != "bf16" and not reuse_prefix:
            raise ValueError(f"suffix_weights={suffix_weights!r} needs the cached-prefix engine (reuse_prefix=True and a shape "
                             "PrefixCachedEps.supports); the whole-forward sampler has bf16 weights only")
        if reuse_prefix:
            eps_model = PrefixCachedEps.for_inputs(self.vlm, n_action_rows=T, suffix_weights=suffix_weights, prefill=prefill,
                                                   suffix_attention=suffix_attention, prefill_precision=prefill_precision,
                                                   suffix_operand=suffix_operand, suffix_mx=suffix_mx, **model_kwargs)
        else:
            needs_engine("PrefixCachedEps", T, suffix_mx=suffix_mx, prefill=prefill, sampler=sampler, ddpm_sampler=ddpm_sampler,
                         suffix_attention=suffix_attention, suffix_operand=suffix_operand)
        pin = MLA._pin(self, [known_actions], T, action_dim, unnorm_key, device)
        samples = self._sample(eps_model, x0, sampler, use_ddim, num_ddim_steps, model_kwargs, ddpm_sampler, pin, solver)
        return self._actions([samples[:1].float().cpu().numpy()], unnorm_key)[0]

    @torch.inference_mode()
    def predict_action_diff_batch(self, images, pointclouds, instructions=None, cur_robot_states=None, unnorm_key: Optional[str] = None,
                                  cfg_scale: float = 0.0, use_ddim: bool = True, num_ddim_steps: int = 8, action_dim: int = 7, *,
                                  input_ids=None, noise: Optional[torch.Tensor] = None, camera_name: str = "rlbench_front",
                                  reuse_prefix: bool = True, suffix_weights: str = "bf16",
                                  num_samples: Optional[int] = None, prefill: str = "train", sampler: str = "host",
                                  suffix_attention: str = "head", prefill_precision: str = "bf16",
                                  groups_attention: str = "head", batch_prefill: str = "train",
                                  ddpm_sampler: str = "host", suffix_operand: str = "fused", known_actions=None,
                                  suffix_mx: str = "off", solver: str = "ddim") -> np.ndarray:
        """B observations -> [B, T, action_dim]: by definition B independent `predict_action_diff` calls (the reference's
        `predict_action_batch`, model_mla.py:994, is dead code), computed on ONE cached prefix pass per DDIM step
        (mla_amd/infer.py:BatchedPrefixCachedEps): the prompts may have different lengths, the FPS start indices are drawn once per chunk.
        ``images`` / ``pointclouds`` / ``cur_robot_states``: sequences of B per-sample values in the forms predict_action_diff takes (or
        stacked arrays); ``input_ids``: a list of B tensors ([L_b] or [1, L_b]) of different lengths, or ``instructions`` (B strings) plus
        the attached tokenizer; ``noise``: [B, T, action_dim]. Every per-sample step (image pre-processing, mask channel, prompt tail,
        proprio normalisation, un-normalisation) is predict_action_diff's. B = 1 IS predict_action_diff; ``reuse_prefix=False`` loops the
        reference's control flow; more than 256 suffix rows are served as consecutive sub-batches; head_dim != 128 warns once and loops
        over whole-forward batch-1 calls. ``suffix_weights``: predict_action_diff's, forwarded for B = 1; the batched engine has bf16
        weights only, so B >= 2 with another mode raises NotImplementedError (unless ``num_samples`` is given).
        ``num_samples`` = N >= 1 (default None: everything above, unchanged): N action chunks for EACH observation -> [B, N, T, action_dim],
        by definition ``out[b] == predict_action_diff_samples(observation b, num_samples=N, noise=noise[b])``, computed on one prefill
        over the B prefixes and one pass per sampler step over the B * N * (1 + T) suffix rows (mla_amd/infer.py:BatchedSampleGroupsEps;
        at most 256 rows per pass, more observations are served as consecutive sub-batches). ``noise``: [B, N, T, action_dim]; RNG: for b:
        for n: randn(1, T, D), then the unused randint. B = 1 IS predict_action_diff_samples; ``reuse_prefix=False`` loops the reference's
        control flow; N > 256 // (1 + T) loops predict_action_diff_samples per observation (it splits its passes on one prefill); a shape
        the engine does not serve warns once and loops the same way. All three ``suffix_weights`` modes are accepted (N = 1 included: this
        is how B >= 2 observations get FP8 suffix weights); anything but "bf16" raises ValueError when ``reuse_prefix=False`` or the
        engine does not serve the shape.
        ``suffix_mx``: predict_action_diff's ("fp4": the MXFP4 copy through the `_w4` kernels, "fp4_as_bf16": the bf16 kernels on the
        dequantised copy; a 4-bit weight error, the effect on a trained policy is not measured), on the routes of ``suffix_weights``:
        forwarded for B = 1; B >= 2 without ``num_samples`` raises NotImplementedError; with ``num_samples`` (N = 1 included) every
        pass streams the copy through mla_gemm_suffix_w4_pos. Together with ``suffix_weights`` other than "bf16", with
        ``reuse_prefix=False`` or on a shape the engine does not serve it raises ValueError.
        ``prefill``: only "train" -- the one-observation compact prefill is predict_action_diff's / predict_action_diff_samples';
        "compact" raises NotImplementedError (the batched engines take their FP8 prefill from ``batch_prefill``).
        ``prefill_precision``: only "bf16", for the same reason; "fp8" / "fp8_as_bf16" raise NotImplementedError, an unknown value
        ValueError.
        ``batch_prefill`` (opt-in, cached prefix only), with and without ``num_samples``: "train" (default) prefills the B x S_p prefix
        rows of a pass on the training kernels | "fp8": every prefill layer runs once over all right-padded prefix rows of the pass with
        its four projections on e4m3fn codes of BOTH operands -- the wide-row GEMMs of mla_amd/csrc/prefill.hip
        (mla_gemm_prefill_f8_wide*: up to 65 536 rows, 64- or 128-row tiles on the K = 128 MFMA), the model's FP8 weight copy (one per
        model, shared with ``suffix_weights="fp8"``) and the projection inputs quantised per row; attention, cache and residual stream
        stay bf16 | "fp8_as_bf16": per observation, the bf16 compact kernels on the dequantised weight codes and on
        quantised-and-dequantised inputs -- the same function as "fp8" up to rounding, slow, the yardstick of "fp8" and what the format
        costs on a checkpoint. The effect on a trained policy is not measured. Only the prefill changes: it composes with every
        ``suffix_weights`` (with ``num_samples``), ``sampler`` and ``groups_attention`` mode; where the call ends in a single-observation
        method (B = 1, N beyond a pass) it is forwarded as ``prefill="compact", prefill_precision=<value>``; it raises ValueError for an
        unknown value, for anything but "train" when ``reuse_prefix=False`` or the batched engine does not serve the shape (never the
        warned loop), for more than 65 536 prefill rows in a sub-batch ("fp8") and for more than 1024 prefix rows per observation
        ("fp8_as_bf16"): there is never a silent bf16 prefill.
        ``sampler``: predict_action_diff's, with and without ``num_samples``: "device" runs every pass's DDIM loop on the device (the same
        bits) and raises ValueError where "host" would loop over whole-forward calls (``reuse_prefix=False``, a shape the batched engine
        does not serve) or run the DDPM sampler.
        ``ddpm_sampler``: predict_action_diff's, with and without ``num_samples``: "device" runs the DDPM loop (``use_ddim=False``) of
        every pass or sub-batch on the device, one sample_ddpm each in the order the host path runs its p_sample_loop calls (the same
        bits and generator position); it raises ValueError where "host" would loop over whole-forward calls or the call runs DDIM.
        ``suffix_attention``: predict_action_diff's, forwarded for B = 1; B >= 2 with "split" raises NotImplementedError (the ragged and
        groups engines take their split-key form from ``groups_attention``).
        ``groups_attention`` (opt-in, cached prefix only), with and without ``num_samples``: "head" (default) runs the sampler steps'
        attention as one workgroup per (sample, group, head, 16 queries) (mla_attn_chunk_ragged / mla_attn_chunk_ragged_groups); "split"
        cuts every (sample, group, head)'s key range over several workgroups and merges the partial softmax states in a fixed order with
        a second launch (mla_attn_groups_split with the library's plan at the engine's capacity): the same function up to summation
        order. The plan splits while the launch fits the chip -- at 7B for B * N <= 4 chunks at window <= 15 and B * N <= 2 up to window
        31; beyond, "split" is the head launch by construction. It composes with every ``suffix_weights`` and ``sampler`` mode; where the
        call ends in predict_action_diff (B = 1, no ``num_samples`` or N = 1) it is forwarded as ``suffix_attention="split"``; it raises
        ValueError for an unknown value, and for "split" when ``reuse_prefix=False`` or the batched engine does not serve the shape: it is
        never the warned loop.
        ``suffix_operand``: predict_action_diff's, forwarded where the call ends in it (B = 1, no ``num_samples`` or N = 1). The batched
        engines (B >= 2, or N >= 2 chunks per observation) form every operand once per pass already (stand-alone RMSNorm / SwiGLU
        kernels in front of the row GEMMs): they accept both values and launch what they launch without the keyword. An unknown value,
        and "once" with ``reuse_prefix=False``, raise ValueError.
        ``known_actions``: predict_action_diff's, as a list with one entry per observation -- an array [d_b, action_dim] (its own d_b) or
        None (nothing of that chunk is pinned); with ``num_samples`` the N chunks of an observation share its entry. None, or a list of
        only None, is the call without the keyword, bit for bit. A list of another length raises ValueError before the model is
        touched.
        ``solver``: predict_action_diff's, with and without ``num_samples``: "dpmpp2m" runs DPM-Solver++(2M) over every pass's or
        sub-batch's respaced process, on the host loop or (``sampler="device"``) on the device, the same bits; handed on where the
        call ends in another public method. An unknown value, and "dpmpp2m" where the call runs the DDPM sampler, raise ValueError."""
        from .infer import BatchedPrefixCachedEps, Modes, check_mode, check_modes, needs_engine, suffix_attention_single_only
        modes = Modes(suffix_weights=suffix_weights, prefill=prefill, suffix_attention=suffix_attention, groups_attention=groups_attention,
                      batch_prefill=batch_prefill, suffix_operand=suffix_operand, sampler=sampler, ddpm_sampler=ddpm_sampler,
                      suffix_mx=suffix_mx)
        check_modes(modes, reuse_prefix, use_ddim, num_ddim_steps)
        MLA._check_solver(solver, use_ddim, num_ddim_steps)
        check_mode("prefill_precision", prefill_precision)                    # an unknown value only: no mode but "bf16" is served here
        check_mode("batch_prefill", batch_prefill, reuse_prefix)
        if prefill != "train":
            raise NotImplementedError(f"prefill={prefill!r}: the batched engines prefill B x S rows on the training GEMMs; the compact "
                                      "prefill serves one observation (predict_action_diff, predict_action_diff_samples)")
        if prefill_precision != "bf16":
            raise NotImplementedError(f"prefill_precision={prefill_precision!r}: the batched engines prefill B x S rows on the training "
                                      "GEMMs; the compact prefill serves one observation (predict_action_diff, "
                                      "predict_action_diff_samples)")
        B = len(images)
        if B != 1:
            suffix_attention_single_only(suffix_attention, f"predict_action_diff_batch with {B} observations")
        T = self.future_action_window_size + 1
        known = MLA._known_entries(known_actions, B, T, action_dim)
        if num_samples is not None:
            return self._predict_action_diff_batch_samples(images, pointclouds, instructions, cur_robot_states, unnorm_key, cfg_scale, use_ddim,
                                                           num_ddim_steps, action_dim, input_ids, noise, camera_name, reuse_prefix,
                                                           num_samples, modes, known, solver)
        input_ids, pointclouds = MLA._batch_prompts(self, B, instructions, input_ids, pointclouds, cur_robot_states)
        if noise is not None and tuple(noise.shape[:2]) != (B, T):
            raise ValueError(f"noise must be [B, T, action_dim] = [{B}, {T}, ...], got {tuple(noise.shape)}")
        self._check_cfg_scale(cfg_scale)
        ids_rows = [ids.reshape(1, -1) for ids in input_ids]

        def one(b, **kw):
            return self.predict_action_diff(images[b], pointclouds[b], None, cur_robot_states[b], unnorm_key, cfg_scale, use_ddim, num_ddim_steps,
                                            action_dim, input_ids=ids_rows[b], noise=None if noise is None else noise[b:b + 1],
                                            camera_name=camera_name, **MLA._fwd_known(known[b]), **MLA._fwd_solver(solver), **kw)
        if B == 1:
            return one(0, reuse_prefix=reuse_prefix,
                       **modes.forwarded("suffix_weights", "suffix_mx", "sampler", "ddpm_sampler", "suffix_attention", "suffix_operand"))[None]
        if suffix_mx != "off":
            raise NotImplementedError(f"suffix_mx={suffix_mx!r}: the batched engine (BatchedPrefixCachedEps, mla_gemm_suffix_bf16) streams "
                                      "bf16 weights only; sample B >= 2 observations with \"off\", one at a time, or pass `num_samples` "
                                      "(BatchedSampleGroupsEps serves every mode)")
        if suffix_weights != "bf16":
            raise NotImplementedError(f"suffix_weights={suffix_weights!r}: the batched engine (BatchedPrefixCachedEps, mla_gemm_suffix_bf16) "
                                      "streams bf16 weights only; sample B >= 2 observations with \"bf16\", one at a time, or pass "
                                      "`num_samples` (BatchedSampleGroupsEps serves every mode)")
        if reuse_prefix and not BatchedPrefixCachedEps.supports_batch(self.vlm, T, warn=False):
            needs_engine("BatchedPrefixCachedEps", T, groups_attention=groups_attention, batch_prefill=batch_prefill, sampler=sampler,
                         ddpm_sampler=ddpm_sampler)                              # raised, not a warned loop of batch-1 calls
            reuse_prefix = BatchedPrefixCachedEps.supports_batch(self.vlm, T)   # warns once
        if not reuse_prefix:
            return np.stack([one(b, reuse_prefix=False) for b in range(B)])
        device, ids_rows, inputs = self._batch_inputs(images, pointclouds, cur_robot_states, ids_rows, unnorm_key, camera_name)
        x0 = self._draw_x0([None if noise is None else noise[b:b + 1] for b in range(B)], T, action_dim, device)
        pin = MLA._pin(self, known, T, action_dim, unnorm_key, device)
        out = []
        for sub, eng in BatchedPrefixCachedEps.for_batch(self.vlm, ids_rows, T, suffix_attention=groups_attention,
                                                         batch_prefill=batch_prefill, **inputs):
            samples = self._sample(eng, x0[sub.start:sub.stop].contiguous(), sampler, use_ddim, num_ddim_steps, {}, ddpm_sampler,
                                   MLA._pin_rows(pin, sub.start, sub.stop), solver)
            out.append(samples.float().cpu().numpy())
        return self._actions(out, unnorm_key)

    def _predict_action_diff_batch_samples(self, images, pointclouds, instructions, cur_robot_states, unnorm_key, cfg_scale, use_ddim,
                                           num_ddim_steps, action_dim, input_ids, noise, camera_name, reuse_prefix, num_samples, modes,
                                           known, solver="ddim"):
        """predict_action_diff_batch(num_samples=N) -> [B, N, T, action_dim] (called inside its inference mode; see its docstring).
        modes: its keywords as infer.Modes, known: its known_actions as one entry per observation, solver: its solver, all validated
        there."""
        from .infer import BatchedSampleGroupsEps, needs_engine
        B, N, T = len(images), int(num_samples), self.future_action_window_size + 1
        if N < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        input_ids, pointclouds = MLA._batch_prompts(self, B, instructions, input_ids, pointclouds, cur_robot_states)
        if noise is not None and tuple(noise.shape) != (B, N, T, action_dim):
            raise ValueError(f"noise must be [B, N, T, action_dim] = [{B}, {N}, {T}, {action_dim}], got {tuple(noise.shape)}")
        self._check_cfg_scale(cfg_scale)
        ids_rows = [ids.reshape(1, -1) for ids in input_ids]

        def samples_of(b, **kw):
            return self.predict_action_diff_samples(images[b], pointclouds[b], None, cur_robot_states[b], unnorm_key, N, cfg_scale, use_ddim,
                                                    num_ddim_steps, action_dim, input_ids=ids_rows[b], noise=None if noise is None else noise[b],
                                                    camera_name=camera_name, **MLA._fwd_known(known[b]), **MLA._fwd_solver(solver), **kw)
        if B == 1:
            return samples_of(0, reuse_prefix=reuse_prefix, **modes.forwarded("suffix_weights", "suffix_mx", "sampler", "ddpm_sampler",
                                                                              "suffix_attention", "groups_attention", "suffix_operand"))[None]
        if modes.suffix_weights != "bf16" and not reuse_prefix:
            raise ValueError(f"suffix_weights={modes.suffix_weights!r} needs the cached prefix (reuse_prefix=True); the whole-forward sampler "
                             "has bf16 weights only")
        if reuse_prefix:
            if not BatchedSampleGroupsEps.supports_batch_samples(self.vlm, T, warn=False):
                needs_engine("BatchedSampleGroupsEps", T, sampler=modes.sampler, ddpm_sampler=modes.ddpm_sampler,
                             groups_attention=modes.groups_attention, batch_prefill=modes.batch_prefill, suffix_weights=modes.suffix_weights,
                             suffix_mx=modes.suffix_mx)
            if not BatchedSampleGroupsEps.supports_batch_samples(self.vlm, T) or not BatchedSampleGroupsEps.fits_pass(T, N):
                # one observation at a time: predict_action_diff_samples serves (or refuses) the shape and the mode itself
                return np.stack([samples_of(b, **modes.forwarded("suffix_weights", "suffix_mx", "sampler", "ddpm_sampler", "groups_attention"))
                                 for b in range(B)])
        else:
            return np.stack([samples_of(b, reuse_prefix=False) for b in range(B)])
        device, ids_rows, inputs = self._batch_inputs(images, pointclouds, cur_robot_states, ids_rows, unnorm_key, camera_name)
        x0 = self._draw_x0([None if noise is None else noise[b, n:n + 1] for b in range(B) for n in range(N)], T, action_dim, device)   # rows (b, n)
        pin = MLA._pin(self, known, T, action_dim, unnorm_key, device, repeat=N)
        out = []
        for sub, eng in BatchedSampleGroupsEps.for_batch(self.vlm, ids_rows, T, N, modes.suffix_weights,
                                                         suffix_attention=modes.groups_attention, batch_prefill=modes.batch_prefill,
                                                         suffix_mx=modes.suffix_mx, **inputs):
            samples = self._sample(eng, x0[sub.start * N:sub.stop * N].contiguous(), modes.sampler, use_ddim, num_ddim_steps, {},
                                   modes.ddpm_sampler, MLA._pin_rows(pin, sub.start * N, sub.stop * N), solver)
            out.append(samples.float().cpu().numpy().reshape(sub.stop - sub.start, N, T, -1))
        return self._actions(out, unnorm_key)

    @torch.inference_mode()
    def predict_action_diff_samples(self, image=None, pointcloud=None, instruction: Optional[str] = None, cur_robot_state=None,
                                    unnorm_key: Optional[str] = None, num_samples: int = 1, cfg_scale: float = 0.0, use_ddim: bool = True,
                                    num_ddim_steps: int = 8, action_dim: int = 7, *, input_ids: Optional[torch.Tensor] = None,
                                    noise: Optional[torch.Tensor] = None, camera_name: str = "rlbench_front",
                                    reuse_prefix: bool = True, suffix_weights: str = "bf16", prefill: str = "train",
                                    sampler: str = "host", suffix_attention: str = "head",
                                    prefill_precision: str = "bf16", groups_attention: str = "head",
                                    ddpm_sampler: str = "host", suffix_operand: str = "fused", known_actions=None,
                                    suffix_mx: str = "off", solver: str = "ddim") -> np.ndarray:
        """N action chunks for ONE observation -> [N, T, action_dim]: by definition N independent `predict_action_diff` calls on the same
        observation with the initial samples ``noise[n]`` (critic / best-of-N choice, uncertainty estimates, temporal ensembling), computed
        on ONE cached prefix (mla_amd/infer.py:SampleGroupsEps): the encoders and the decoder prefill run once per call, every sampler step
        is one pass over the N * (1 + T) suffix rows (mla_attn_chunk_groups: every sample sees the prefix and its own rows), the FPS start
        indices are drawn once per call. Every per-observation step (image pre-processing, mask channel, prompt tail, proprio
        normalisation, un-normalisation) is predict_action_diff's. RNG: the draws of N calls in their order (randn(1, T, D), then the
        unused randint, per sample). ``num_samples=1`` IS predict_action_diff; ``reuse_prefix=False``, head_dim != 128 or more than 64
        suffix rows per sample loop N predict_action_diff calls (a shape reason warns once); more than 256 suffix rows are served as
        consecutive passes on the same prefill.
        ``suffix_weights`` (opt-in): predict_action_diff's modes. "fp8": every pass streams the per-row e4m3fn copy of the decoder weights
        (mla_gemm_suffix_w8: half the weight bytes per sampler step; the prefill and the prefix keys / values keep the bf16 weights);
        "fp8_as_bf16": the bf16 kernel on the dequantised copy. Forwarded for ``num_samples=1``. Anything but "bf16" raises ValueError
        when ``reuse_prefix=False`` or the shared-prefix engine does not serve the shape: no silent bf16 fallback, no silent loop.
        ``suffix_mx`` (opt-in): predict_action_diff's modes. "fp4": every pass streams the model's MXFP4 copy of the decoder weights
        (mla_gemm_suffix_w4: a quarter of the bf16 weight bytes per sampler step, gemm_skinny_w4's summation order, so every sample is
        what its own predict_action_diff(suffix_mx="fp4") call computes up to the attention launch); "fp4_as_bf16": the bf16 kernel on
        the dequantised copy. A 4-bit weight error (0.11 relative Frobenius on Gaussian weights); the effect on a trained policy is not
        measured. Forwarded for ``num_samples=1``. Anything but "off" raises ValueError together with ``suffix_weights`` other than
        "bf16", when ``reuse_prefix=False`` or when the shared-prefix engine does not serve the shape.
        ``prefill`` (opt-in): predict_action_diff's modes; "compact" runs the one prefill of the call on the row-sized GEMMs. Forwarded
        for ``num_samples=1``; raises ValueError when ``reuse_prefix=False``, the shared-prefix engine does not serve the shape, the prefix
        has more than 1024 rows or head_dim is not 128.
        ``sampler`` (opt-in): predict_action_diff's modes; "device" runs the DDIM loop of every pass on the device (the same bits).
        Forwarded for ``num_samples=1``; raises ValueError when ``reuse_prefix=False``, the shared-prefix engine does not serve the shape,
        ``use_ddim=False`` or ``num_ddim_steps=None``.
        ``ddpm_sampler`` (opt-in): predict_action_diff's modes; "device" runs the DDPM loop (``use_ddim=False``) of every pass on the
        device, one sample_ddpm per pass in the host path's order (the same bits and generator position). Forwarded for
        ``num_samples=1``; raises ValueError when ``reuse_prefix=False``, the shared-prefix engine does not serve the shape, or the call
        runs the DDIM sampler.
        ``suffix_attention``: predict_action_diff's, forwarded for ``num_samples=1``; more samples with "split" raise NotImplementedError
        (the groups engine keeps mla_attn_chunk_groups).
        ``prefill_precision`` (opt-in, ``prefill="compact"`` only): predict_action_diff's modes; "fp8" runs the projections of the one
        prefill of the call over e4m3fn codes of both operands. Forwarded for ``num_samples=1``; raises ValueError for an unknown value
        and for anything but "bf16" unless ``prefill="compact"``.
        ``groups_attention`` (opt-in): predict_action_diff_batch's modes; "split" runs every pass's attention as mla_attn_groups_split
        with the library's plan (at 7B it splits for N <= 4 at window <= 15 and N <= 2 up to window 31; beyond, it is the head launch).
        It composes with every ``suffix_weights``, ``sampler``, ``prefill`` and ``prefill_precision`` mode; forwarded as
        ``suffix_attention="split"`` for ``num_samples=1``; raises ValueError for an unknown value, and for "split" when
        ``reuse_prefix=False`` or the shared-prefix engine does not serve the shape.
        ``suffix_operand``: predict_action_diff's, forwarded for ``num_samples=1``. With more samples the shared-prefix engine forms every
        operand once per pass already: both values are accepted and launch what is launched without the keyword. An unknown value, and
        "once" with ``reuse_prefix=False``, raise ValueError.
        ``known_actions``: predict_action_diff's -- one array [d, action_dim] for the observation, pinned in every one of the N chunks
        (the engine sees it repeated over the samples). None is the call without the keyword, bit for bit.
        ``solver``: predict_action_diff's; "dpmpp2m" runs DPM-Solver++(2M) over every pass's respaced process, on the host loop or
        (``sampler="device"``) on the device, the same bits. Handed on for ``num_samples=1`` and in the loops over predict_action_diff.
        An unknown value, and "dpmpp2m" with ``use_ddim=False`` or ``num_ddim_steps=None``, raise ValueError."""
        from .infer import Modes, SampleGroupsEps, check_modes, needs_engine, suffix_attention_single_only
        modes = Modes(suffix_weights=suffix_weights, prefill=prefill, suffix_attention=suffix_attention, groups_attention=groups_attention,
                      prefill_precision=prefill_precision, suffix_operand=suffix_operand, sampler=sampler, ddpm_sampler=ddpm_sampler,
                      suffix_mx=suffix_mx)
        check_modes(modes, reuse_prefix, use_ddim, num_ddim_steps)
        MLA._check_solver(solver, use_ddim, num_ddim_steps)
        if int(num_samples) != 1:
            suffix_attention_single_only(suffix_attention, f"predict_action_diff_samples with num_samples={num_samples}")
        if prefill != "train" and not reuse_prefix:
            raise ValueError(f"prefill={prefill!r} needs the cached prefix (reuse_prefix=True); the whole-forward sampler has no separate "
                             "prefill")
        N = int(num_samples)
        T = self.future_action_window_size + 1
        if N < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        if noise is not None and tuple(noise.shape) != (N, T, action_dim):
            raise ValueError(f"noise must be [N, T, action_dim] = [{N}, {T}, {action_dim}], got {tuple(noise.shape)}")
        known_actions = MLA._known_entry(known_actions, T, action_dim)
        self._check_cfg_scale(cfg_scale)

        def one(n, **kw):
            return self.predict_action_diff(image, pointcloud, instruction, cur_robot_state, unnorm_key, cfg_scale, use_ddim, num_ddim_steps,
                                            action_dim, input_ids=input_ids, noise=None if noise is None else noise[n:n + 1],
                                            camera_name=camera_name, **MLA._fwd_known(known_actions), **MLA._fwd_solver(solver), **kw)
        if N == 1:
            return one(0, reuse_prefix=reuse_prefix, **modes.forwarded("suffix_weights", "suffix_mx", "prefill", "sampler", "ddpm_sampler",
                                                                       "suffix_attention", "prefill_precision", "suffix_operand"))[None]
        if suffix_weights != "bf16" and not reuse_prefix:
            raise ValueError(f"suffix_weights={suffix_weights!r} needs the cached prefix (reuse_prefix=True); the whole-forward sampler has "
                             "bf16 weights only")
        if reuse_prefix:
            if not SampleGroupsEps.supports_samples(self.vlm, T, warn=False):       # raised, not a warned loop of batch-1 calls
                needs_engine("SampleGroupsEps", T, sampler=sampler, ddpm_sampler=ddpm_sampler, groups_attention=groups_attention,
                             prefill=prefill, suffix_weights=suffix_weights, suffix_mx=suffix_mx)
            reuse_prefix = SampleGroupsEps.supports_samples(self.vlm, T)
        if not reuse_prefix:
            return np.stack([one(n, reuse_prefix=False) for n in range(N)])
        self.vlm.eval()
        device = next(self.vlm.parameters()).device
        if input_ids is None:
            input_ids = self._prompt_ids(instruction, "predict_action_diff_samples")
        image = self._preprocessed_image(image)
        input_ids = self._ids_with_tail(input_ids, device)
        model_kwargs = {"images": self._image_batch(image, device), "point_cloud": self._pointcloud_batch(pointcloud, device),
                        "camera_name": camera_name, "proprio": self._proprio_token(cur_robot_state, unnorm_key, device)}
        x0 = self._draw_x0([None if noise is None else noise[n:n + 1] for n in range(N)], T, action_dim, device)
        pin = MLA._pin(self, [known_actions], T, action_dim, unnorm_key, device, repeat=N)
        eng, passes = SampleGroupsEps.for_inputs(self.vlm, input_ids, T, N, suffix_weights=suffix_weights, prefill=prefill,
                                                 prefill_precision=prefill_precision, suffix_attention=groups_attention, suffix_mx=suffix_mx,
                                                 **model_kwargs)
        out = []
        for start, stop in passes:                                           # one prefill, then the passes' sampler loops one after the other
            eng.set_groups(stop - start)
            samples = self._sample(eng, x0[start:stop].contiguous(), sampler, use_ddim, num_ddim_steps, {}, ddpm_sampler,
                                   MLA._pin_rows(pin, start, stop), solver)
            out.append(samples.float().cpu().numpy())
        return self._actions(out, unnorm_key)
