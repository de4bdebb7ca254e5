"""A complete training step on the HIP kernels: ``Trainer`` assembles the differentiable forward (``conditioning_grad``,
``unet_grad``, ``grad_ops.mse_rows``), the optimizer (``optim.ParamArena`` + ``optim.FusedAdamW``: clip, ``16-mixed``
loss scale, EMA, 16-bit working copy) and the one-launch re-layout of the data-gradient weights (``optim.DgradRelayout``)
around a ``DiffusionModuleWithIP``.

The module stays what it is: its frozen parts (VAE encoder, CLIP tower, noise schedule) serve the trainer as they serve
``training_step()``, and ``training_step()`` / ``configure_optimizers()`` keep their behaviour.  The trainer owns its own
fp32 masters, taken from the module's state dict once; the module's inference plans do not follow them.
``export_state_dict()`` gives the trained weights back in the reference layout, which ``DiffusionModuleWithIP(cfg,
state_dict=...)`` loads.

Operands are fp16: the conditioning front-end's attention (d = 96) has no bf16 forward, so bf16 is refused here.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import conditioning_grad as CG
from . import grad_ops as G
from . import optim as O
from . import unet_grad as UG
from .lr_scheduler import warmup_cosine_lr

_GATES = ("processor.anat_gate", "processor.dis_gate")
_FROZEN = ("vae.", "image_encoder.")


def _get(node, name, default):
    return getattr(node, name, default) if node is not None else default


class Trainer:
    """``Trainer(module, lr)``: masters from ``module``'s state dict (UNet weights in the library layout), the reference's
    four parameter groups (``optim.reference_param_groups``; the routing gates are not trained and stay outside), a
    ``ParamArena`` with the 16-bit working copy and the EMA, ``FusedAdamW`` with the clip of ``cfg.training.
    gradient_clip_val`` and - for ``precision: 16-mixed`` - the loss scale, and the re-layout owner.  Read from
    ``cfg.training`` with the reference's defaults where the key is missing: ``gradient_clip_val`` 1.0, ``ema_decay``
    0.999, ``update_starting_at_step`` 100, ``update_every_n_steps`` 4, ``max_epochs`` 150, ``use_min_snr_weighting``;
    from ``cfg.optimizer`` ``betas`` / ``weight_decay`` and from ``cfg.scheduler`` ``warmup_epochs`` / ``min_lr``.
    ``prepared=False`` runs every product on the masters alone (cast and torch re-layout per call)."""

    def __init__(self, module, lr: float, *, prepared: bool = True, operand_dtype: torch.dtype = torch.float16,
                 init_scale: Optional[float] = None, growth_interval: int = 2000):
        if operand_dtype != torch.float16:
            raise ValueError(f"Trainer runs in fp16: the conditioning front-end's attention (d = 96) has no {operand_dtype} "
                             "forward, so a training step in that type is not available")
        UG.check_latent_side(module.latent_side, module.latent_side)
        self.module, self.be, self.device, self.dtype = module, module.be, module.device, operand_dtype
        cfg, dc = module.cfg, module.diff_cfg
        tr, opt, sch = _get(cfg, "training", None), _get(cfg, "optimizer", None), _get(cfg, "scheduler", None)
        self.base_lr = float(lr)
        self.max_epochs = int(_get(tr, "max_epochs", 150))
        self.warmup_epochs = int(_get(sch, "warmup_epochs", 0))
        self.eta_min = float(_get(sch, "min_lr", 0.0))
        self.ema_decay = float(_get(tr, "ema_decay", 0.999))
        self.ema_start = int(_get(tr, "update_starting_at_step", 100))
        self.ema_every = max(1, int(_get(tr, "update_every_n_steps", 4)))
        if init_scale is None:
            init_scale = 65536.0 if str(_get(tr, "precision", "16-mixed")) == "16-mixed" else 0.0
        self.loss_scaling = float(init_scale) > 0.0      # (a scale of 0 in the state block means: no loss scaling)

        sd = module._sd
        masters: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        unet = UG.masters_from_state_dict(sd)
        for k, v in sd.items():
            if k.startswith(_FROZEN):
                continue
            masters[k] = (unet[k] if k in unet else v.detach().float()).to(self.device)
        self.gates: Dict[str, torch.Tensor] = {k: v for k, v in masters.items() if k.endswith(_GATES)}
        trained = OrderedDict((k, v) for k, v in masters.items() if k not in self.gates)
        self.groups = O.reference_param_groups(list(trained), self.base_lr, float(_get(opt, "weight_decay", 0.01)))
        self.arena = O.arena_from_groups(trained, self.groups, device=self.device, working_dtype=operand_dtype, ema=True)
        self.optimizer = O.FusedAdamW(self.be, self.arena, self.groups, betas=tuple(_get(opt, "betas", (0.9, 0.999))),
                                      max_grad_norm=float(_get(tr, "gradient_clip_val", 1.0)), ema_decay=self.ema_decay,
                                      init_scale=float(init_scale), growth_interval=growth_interval)
        # the leaves autograd sees: views of the arena's p whose .grad is the arena's g
        self.params: Dict[str, torch.Tensor] = {k: torch.empty(0, device=self.device).requires_grad_(True) for k in trained}
        for k, t in self.params.items():
            t.data = self.arena.param(k)
        self.arena.attach(self.params)
        self.params.update(self.gates)
        self.relayout = O.DgradRelayout(self.be, self.arena, UG.relayout_entries(trained)) if prepared else None
        if self.relayout is not None:
            self.relayout.refresh()
        self.steps = 0
        self.epoch = 0
        self._lrs = None
        self.set_epoch(0)

    # -- schedule
    def lrs(self, epoch: int):
        """The four groups' rates of ``epoch``: ``lr_scheduler.warmup_cosine_lr`` over the groups' base rates."""
        return warmup_cosine_lr(epoch, [g["lr"] for g in self.groups], self.warmup_epochs, self.max_epochs,
                                self.base_lr * 0.01, self.eta_min)

    def set_epoch(self, epoch: int) -> None:
        """The schedule is per epoch, as in the reference; the rates reach the device when they change."""
        self.epoch = int(epoch)
        lrs = self.lrs(self.epoch)
        if lrs != self._lrs:
            self.optimizer.set_lrs(lrs)
            self._lrs = lrs

    # -- forward
    def loss(self, batch, *, noise=None, t=None, drop_mask=None, latent_noise=None, is_training: bool = True):
        """The forward of ``DiffusionModuleWithIP.training_step`` with the same injectable draws, WITH autograd history:
        frozen VAE encode and CLIP tower through the module (no history), AOE / image projection / purifier through
        ``conditioning_grad`` in fp16, CFG dropout and ``cat`` in torch, ``unet_grad.unet_forward``, ``mse_rows`` x Min-SNR
        -> mean."""
        mod, be, P = self.module, self.be, self.params
        dc = mod.diff_cfg
        images, labels, structure_images = batch
        b = images.shape[0]
        with torch.no_grad():
            dist = mod.vae.encode(images).latent_dist
            latents = dist.sample(noise=latent_noise, scale=dc.latent_scale)
            if noise is None:
                noise = torch.randn_like(latents)
            noise = noise.to(device=self.device, dtype=torch.float32).contiguous()
            if t is None:
                t = mod._sample_timesteps(b)
            t = t.to(self.device)
            noisy = mod._q_sample(latents, t, noise)
            if dc.use_image_projection_plus:
                feats = mod.image_encoder.get_hidden_states(structure_images)
            else:
                feats = mod.image_encoder(structure_images)
            feats = feats.to(self.dtype)
            weight = mod._min_snr_weight(t)
        labels = labels.to(device=self.device, dtype=torch.float32)
        aoe = CG.ordinal_embedder(be, P, labels, is_training=is_training, num_tokens=dc.num_aoe_tokens)
        if aoe.dim() == 2:
            aoe = aoe.unsqueeze(1)
        if dc.use_image_projection_plus:
            img = CG.image_projection_plus(be, P, feats)
        else:
            img = CG.image_projection(be, P, feats, num_tokens=dc.num_image_tokens)
        if mod.feature_purifier is not None:
            img = CG.feature_purifier(be, P, img, aoe.to(self.dtype), heads=dc.purifier_num_heads)
        img = img.float()
        if drop_mask is None:
            drop_mask = torch.rand(b, device=self.device) < getattr(mod.cfg.model, "cfg_drop_prob", 0.1)
        img = torch.where(drop_mask.to(self.device).view(-1, 1, 1).expand_as(img), torch.zeros_like(img), img)
        cond = torch.cat([aoe, img, torch.zeros_like(aoe)] if dc.use_routing_gates else [aoe, img], dim=1)
        pred = UG.unet_forward(be, P, noisy, t, cond, use_routing_gates=dc.use_routing_gates,
                               delta_scale=mod.unet.unet.delta_scale() if dc.use_routing_gates else 0.0, dtype=self.dtype,
                               prepared=self.relayout)
        return (weight * G.mse_rows(be, pred, noise)).mean()

    # -- the step
    def step(self, batch, **draws) -> torch.Tensor:
        """loss x loss scale -> backward (into the arena's gradient buffer) -> ``FusedAdamW.step`` (with the EMA on the
        reference's cadence) -> re-layout refresh -> learning rates.  No host synchronisation; returns the unscaled loss
        (detached, on the device)."""
        loss = self.loss(batch, **draws)
        scale = self.optimizer.scale()          # a device scalar: no sync
        (loss * scale if self.loss_scaling else loss).backward()
        self.steps += 1
        update_ema = self.steps >= self.ema_start and self.steps % self.ema_every == 0
        self.optimizer.step(update_ema=update_ema, zero_grad=True)
        if self.relayout is not None:
            self.relayout.refresh()
        self.set_epoch(self.epoch)
        return loss.detach()

    # -- export
    def export_state_dict(self, ema: bool = False) -> "OrderedDict[str, torch.Tensor]":
        """The reference-layout fp32 state dict on the CPU: the trained weights (or their EMA) with the UNet's convs back
        in OIHW, the gates, and the module's frozen tensors.  Synchronises."""
        self.be.synchronize()
        torch.cuda.synchronize(self.device)
        view = self.arena.ema_param if ema else self.arena.param
        masters = OrderedDict()
        for k in self.module._sd:
            if k.startswith(_FROZEN):
                masters[k] = self.module._sd[k].detach().cpu()
            elif k in self.gates:
                masters[k] = self.gates[k].detach().cpu()
            else:
                masters[k] = view(k).detach().cpu()
        return UG.state_dict_from_masters(masters)
