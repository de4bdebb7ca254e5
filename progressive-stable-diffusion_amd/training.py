"""A complete training step on the HIP kernels: ``Trainer`` assembles the differentiable forward (``conditioning_grad``,
``unet_grad``, ``grad_ops.mse_rows``), the optimizer (``optim.ParamArena`` + ``optim.FusedAdamW``: clip, ``16-mixed``
loss scale, EMA, 16-bit working copy) and the one-launch re-layout of the data-gradient weights (``optim.DgradRelayout``)
around a ``DiffusionModuleWithIP``.

The module stays what it is: its frozen parts (VAE encoder, CLIP tower, noise schedule) serve the trainer as they serve
``training_step()``, and ``training_step()`` / ``configure_optimizers()`` keep their behaviour.  The trainer owns its own
fp32 masters, taken from the module's state dict once.  ``sync_module("ema" | "raw")`` hands them to the module's live
inference plans and conditioning modules in place, by one refresh launch (``optim.PlanRefresh``, csrc/plan_refresh.hip):
weight buffers keep their addresses, so captured ``DdimLoop`` graphs sample with the new weights.
``export_state_dict()`` gives the trained weights back in the reference layout, which ``DiffusionModuleWithIP(cfg,
state_dict=...)`` loads.

Operands are fp16: the conditioning front-end's attention (d = 96) has no bf16 forward, so bf16 is refused here.

A run on top of the step: ``backward()`` / ``optimizer_step()`` / ``flush()`` accumulate micro-batches
(``accumulate_grad_batches``), a small device block collects the run's numbers until ``pop_metrics()`` fetches them with
one synchronisation, ``state()`` / ``load_state()`` / ``save_checkpoint()`` / ``resume()`` keep everything an exact
continuation needs in the layout of ``training_io``, and ``fit()`` is the epoch loop over any re-iterable of batches.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import conditioning_grad as CG
from . import checkpoint as CK
from . import grad_ops as G
from . import lib as L
from . import optim as O
from . import training_io as IO
from . import unet_grad as UG
from .backend import on_backend
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
    ``prepared=False`` runs every product on the masters alone (cast and torch re-layout per call).  ``accumulate``:
    micro-batches per optimizer step; ``None`` reads ``cfg.training.accumulate_grad_batches`` (default 1)."""

    def __init__(self, module, lr: float, *, prepared: bool = True, operand_dtype: torch.dtype = torch.float16,
                 init_scale: Optional[float] = None, growth_interval: int = 2000, accumulate: Optional[int] = None):
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
        self.accumulate = int(_get(tr, "accumulate_grad_batches", 1) if accumulate is None else accumulate)
        if self.accumulate < 1:
            raise ValueError(f"accumulate_grad_batches must be at least 1, got {self.accumulate}")
        self.log_every = max(1, int(_get(tr, "log_every_n_steps", 50)))
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
        self.pending = 0                    # micro-batches in the arena's g that no optimizer step has taken yet
        self.ema_latest_step = 0            # the optimizer step of the last EMA update (the callback's latest_update_step)
        self.next_epoch = 0                 # where fit() starts: 0, or the epoch after a loaded state's
        # the run's numbers, on the device: sum of micro losses, sum of CFG drop rates, micro-batches, skipped steps
        self._metrics = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._sums = [self._metrics[i] for i in range(3)]       # views, made once: one fused add per micro-batch
        self._skipped = self._metrics[3:4]
        self._one = torch.ones((), dtype=torch.float32, device=self.device)
        self._found_inf = self.optimizer.state[L.OptimState.found_inf.offset // 4:L.OptimState.found_inf.offset // 4 + 1]
        self._last_drop = None
        self._writer = IO.BackgroundWriter()
        self._refresher = None              # sync_module: (owners, recipes per owner, PlanRefresh) of the last call
        self._copy_stream = None
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
        self._last_drop = drop_mask
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
        (detached, on the device).
        With ``accumulate`` = k > 1 every call runs the backward with its loss weighted 1 / k and every k-th call the
        optimizer step; ``flush()`` steps for a short last group."""
        loss = self.backward(batch, weight=1.0 / self.accumulate, **draws)
        if IO.optimizer_step_due(self.pending, self.accumulate):
            self.optimizer_step()
        return loss

    def backward(self, batch, *, weight: float = 1.0, **draws) -> torch.Tensor:
        """One micro-batch: ``loss()``, then ``(loss * weight * loss scale).backward()``, which ADDS into the arena's
        gradient buffer (``ParamArena.attach``).  No optimizer call; the micro-batch counts as pending until
        ``optimizer_step()``.  Returns the unscaled, unweighted loss (detached, on the device) and adds it to the run's
        numbers.  No host synchronisation."""
        loss = self.loss(batch, **draws)
        factor = self.optimizer.scale() if self.loss_scaling else None      # a device scalar: no sync
        if weight != 1.0:
            factor = weight if factor is None else factor * weight
        (loss if factor is None else loss * factor).backward()
        self.pending += 1
        out = loss.detach()
        drop = self._last_drop.to(self.device).mean(dtype=torch.float32)
        torch._foreach_add_(self._sums, [out, drop, self._one])
        return out

    def optimizer_step(self) -> None:
        """The optimizer step on what the pending micro-batches left in the gradient buffer: ``FusedAdamW.step`` (clip,
        unscale, AdamW, 16-bit copy, zeroed gradient; the EMA when ``training_io.ema_due`` says so - ``steps`` and the
        cadence count optimizer steps, not micro-batches), re-layout refresh, learning rates.  No host synchronisation."""
        if self.pending == 0:
            raise RuntimeError("optimizer_step(): no micro-batch is pending (backward() first)")
        self.steps += 1
        update_ema = IO.ema_due(self.steps, self.ema_start, self.ema_every)
        self.optimizer.step(update_ema=update_ema, zero_grad=True)
        if update_ema:
            self.ema_latest_step = self.steps
        if self.relayout is not None:
            self.relayout.refresh()
        self._skipped.add_(self._found_inf)             # 1 when the step was skipped for a non-finite gradient
        self.set_epoch(self.epoch)
        self.pending = 0

    def flush(self) -> bool:
        """The optimizer step for a short last group (fewer than ``accumulate`` micro-batches pending, as at the end of
        an epoch whose length is no multiple of k); nothing when none is pending.  The group keeps the weight 1 / k per
        micro-batch: its gradient is the sum over its j < k losses divided by k, not by j, so a short group weighs j / k
        of a full one - what Lightning's ``accumulate_grad_batches`` does with the last batches of an epoch, and the rule
        under which a sample counts the same wherever it falls.  -> whether a step ran."""
        if self.pending == 0:
            return False
        self.optimizer_step()
        return True

    # -- the run's numbers
    METRIC_KEYS = ("loss", "cfg_drop_rate", "micro_batches", "skipped_steps", "step", "grad_norm", "coef", "found_inf",
                   "scale", "growth_tracker", "lr", "epoch", "global_step")

    def pop_metrics(self) -> dict:
        """What the run has collected since the last call, and one synchronisation to fetch it: ``loss`` (mean of the
        unscaled micro losses) and ``cfg_drop_rate`` (mean share of dropped samples) over ``micro_batches``,
        ``skipped_steps`` (optimizer steps the loss scaler skipped), ``optimizer.stats()``' ``step, grad_norm, coef,
        found_inf, scale, growth_tracker`` of the last step, ``lr`` (group name -> the rate in the state block now),
        ``epoch`` and ``global_step`` (optimizer steps of the run).  The device block is zeroed; means of an empty block
        are NaN."""
        be, words = self.be, self.optimizer.state.numel()
        be.wait_current()                   # half a hand-off: the .cpu() below is the sync, nothing to release
        with be.ctx():
            blob = torch.cat([self.optimizer.state, self._metrics.view(torch.int32)]).cpu()     # the one sync
        self._metrics.zero_()
        h = L.OptimState.from_buffer_copy(blob[:words].numpy().tobytes())
        loss_sum, drop_sum, n, skipped = blob[words:].view(torch.float32).tolist()
        return {"loss": loss_sum / n if n else float("nan"), "cfg_drop_rate": drop_sum / n if n else float("nan"),
                "micro_batches": int(n), "skipped_steps": int(skipped), "step": h.step, "grad_norm": h.grad_norm,
                "coef": h.coef, "found_inf": bool(h.found_inf), "scale": h.scale, "growth_tracker": h.growth_tracker,
                "lr": {g["name"]: float(h.lr[i]) for i, g in enumerate(self.groups)}, "epoch": self.epoch,
                "global_step": self.steps}

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

    # -- trained weights -> the module's live plans
    def _plan_refresh(self, owners) -> "O.PlanRefresh":
        bad = [(type(o).__name__, o.unrefreshable[:3]) for o in owners if o.unrefreshable]
        if bad:
            raise RuntimeError(f"sync_module: weight uploads without a recipe, they cannot be refreshed in place: {bad}")
        return O.PlanRefresh(self.be, self.arena, [r for o in owners for r in o.recipes])

    def _sync_plan(self, plan) -> None:
        """``module._plan_sync``: a plan built after a ``sync_module`` takes the weights the source synced last holds NOW,
        not those of the moment of that sync: if optimizer steps ran in between, the new plan is ahead of the older live
        plans until the next ``sync_module`` brings all to one state.  Its table is built, used once and dropped (plans
        are built rarely; the kept table of ``sync_module`` covers the set that was live then).  The hook belongs to the
        trainer whose ``sync_module`` ran last on the module."""
        self._plan_refresh([plan]).refresh(self.module._synced)
        plan.weights_gen += 1

    def sync_module(self, which: str = "ema") -> None:
        """Hand the trained weights - their EMA (``"ema"``) or the raw masters (``"raw"``) - to the module's live inference
        plans (every ``UNetPlan`` in ``module._unets``) and its conditioning modules (ordinal embedder, image projection,
        feature purifier), in place: one refresh launch per 16-bit type (``optim.PlanRefresh``), no host copy, no
        synchronisation.  Weight buffers keep their addresses, so an already captured ``DdimLoop`` graph stays valid and
        samples with the new weights.  Each plan gets ``_a2_dirty`` and an advanced ``cond_gen`` / ``weights_gen``: the
        projected K/V, the attn2 fold and a ``DdimLoop``'s time-row table are rebuilt at the next ``set_cond`` /
        ``prepare_attn2`` / ``prepare``.  The module remembers the source: a plan it
        builds later is refreshed before it is handed out.  ``module._sd`` is not rewritten (``export_state_dict()``
        stays the way to a state dict); VAE, CLIP tower and routing gates are not trained and not touched.  Raises
        ``RuntimeError`` while micro-batches are pending, like ``state()``."""
        if which not in ("ema", "raw"):
            raise ValueError(f"sync_module: which must be 'ema' or 'raw', got {which!r}")
        if self.pending:
            raise RuntimeError(f"{self.pending} micro-batch(es) are pending: flush() or optimizer_step() before the weights "
                               "are handed to the module")
        mod = self.module
        plans = [u._plan for u in mod._unets.values()]
        conds = [m for m in (mod.ordinal_embedder, mod.image_projection, mod.feature_purifier) if m is not None]
        owners, counts = plans + conds, [len(o.recipes) for o in plans + conds]
        last = self._refresher
        # the tables are kept while the same plans and modules are live and none has packed a new tensor since
        if last is None or len(last[0]) != len(owners) or any(a is not b for a, b in zip(last[0], owners)) or last[1] != counts:
            last = self._refresher = (owners, counts, self._plan_refresh(owners))
        last[2].refresh(which)
        for plan in plans:
            plan._a2_dirty = True
            plan.cond_gen += 1
            plan.weights_gen += 1           # DdimLoop rebuilds its time-row table
        mod._synced, mod._plan_sync = which, self._sync_plan

    # -- state and checkpoints
    def _untrained(self) -> List[str]:
        return [k for k in self.module._sd if k.startswith(_FROZEN) or k in self.gates]

    @staticmethod
    def _to_masters(sd) -> Dict[str, torch.Tensor]:
        out = dict(sd)
        out.update(UG.masters_from_state_dict(sd))
        return out

    def state(self, device="cpu", parts: Sequence[str] = IO.PARTS) -> dict:
        """Everything an exact continuation needs, as the dict of ``training_io`` with copies of every tensor on
        ``device``: ``state_dict`` (the EMA; equal to ``export_state_dict(ema=True)``), ``current_model_state`` (the raw
        weights; equal to ``export_state_dict()``), ``optimizer_states`` (moments, step, rates, loss scale and growth
        tracker), the EMA bookkeeping, ``epoch`` / ``global_step`` and the states of torch's CPU generator and of this
        device's.  ``parts`` leaves out what a reader does not need (``("ema",)`` is a weights-only file); only all three
        restore a run.  The copies are taken on the backend's stream, behind every step issued so far; torch's stream
        waits for them and for nothing else.  Raises ``RuntimeError`` while micro-batches are pending: their gradient is
        not part of the state.  Synchronises (the optimizer's scalars go through the host)."""
        if self.pending:
            raise RuntimeError(f"{self.pending} micro-batch(es) are pending: flush() or optimizer_step() before the state is "
                               "taken (the accumulated gradient is not part of it)")
        device, be, sd = torch.device(device), self.be, self.module._sd
        with on_backend(be), be.ctx(), torch.no_grad():
            shared = {k: (self.gates[k] if k in self.gates else sd[k]).detach().to(device=device, copy=True)
                      for k in self._untrained()}

            def export(view):
                # the layout change on the arena's device is the copy; .to() moves it when ``device`` is another one
                trained = UG.state_dict_from_masters(OrderedDict((k, view(k)) for k in self.arena.names))
                for k, t in trained.items():
                    if t._base is not None:     # a 1x1 conv's OIHW form is a view of the arena (already contiguous): copy it
                        trained[k] = t.clone()
                return OrderedDict((k, shared[k] if k in shared else trained[k].to(device)) for k in sd)
            out = IO.pack(self.arena, self.optimizer, epoch=self.epoch, global_step=self.steps,
                          latest_update_step=self.ema_latest_step, accumulate=self.accumulate, parts=parts, device=device,
                          export=export, generators=IO.default_generators(self.device))
        if device.type == "cuda":           # allocated on the backend's stream, read by the caller on torch's
            cur = torch.cuda.current_stream(self.device)
            for part in (out["state_dict"], out.get("current_model_state", {})):
                for t in part.values():
                    t.record_stream(cur)
            for st in (out["optimizer_states"][0]["state"].values() if "optimizer_states" in out else ()):
                st["exp_avg"].record_stream(cur)
                st["exp_avg_sq"].record_stream(cur)
        return out

    def load_state(self, state) -> None:
        """Continue from a dict of ``state()`` (or a file of it read with ``checkpoint.read_raw``).  Names, shapes,
        parameter groups, the operand type and the format tag are checked against this trainer first; a mismatch raises
        ``ValueError`` naming the first offenders and changes nothing.  Restores the masters, the moments, the EMA, the
        optimizer's step count, rates, loss scale and growth tracker, ``steps``, ``epoch``, the EMA bookkeeping and both
        generators, then rebuilds the 16-bit working copy and the re-laid weights.  The step that follows computes what
        the run that saved the state would have computed; ``fit()`` continues at the epoch after the state's (at the
        state's own when it was taken before the first optimizer step)."""
        if self.pending:
            raise RuntimeError(f"{self.pending} micro-batch(es) are pending: flush() before a state is loaded")
        # half a hand-off: the copies run on torch's stream, after what the backend still does; the next step's bracket waits
        self.be.release_to_current()
        info = IO.load(state, self.arena, self.optimizer, to_masters=self._to_masters, ignore=self._untrained(),
                       generators=IO.default_generators(self.device))
        with torch.no_grad():
            raw = state["current_model_state"]
            for k, g in self.gates.items():
                g.copy_(raw[k])
            self.arena.g.zero_()
            self._metrics.zero_()
        self.steps, self.epoch = info["global_step"], info["epoch"]
        self.next_epoch = self.epoch + (1 if self.steps > 0 else 0)      # a state from before the first step starts its epoch
        self.ema_latest_step = info["latest_update_step"]
        self._lrs = None                    # the rates are the file's until the next set_epoch()
        if self.relayout is not None:
            self.relayout.refresh()

    def save_checkpoint(self, path, parts: Sequence[str] = IO.PARTS, wait: bool = True) -> str:
        """``state()`` -> ``path``, written to ``path + ".tmp"`` and moved into place (``training_io.write_checkpoint``).
        ``DiffusionModuleWithIP.load_from_checkpoint(path, which="ema" | "raw")`` and ``resume()`` read the file.

        ``wait=False`` keeps the run going while the file is written: the state is snapshotted on the device (copies on
        the backend's stream: the three parts are about 15 GB at full size, held until they have reached the host), and
        one background thread brings the snapshot to the host and writes it.  Torch's stream waits for the snapshot
        copies only.  A later save and ``close()`` wait for the write first; what the thread raised surfaces there."""
        path = str(path)
        self._writer.join()
        if wait:
            return IO.write_checkpoint(self.state("cpu", parts), path)
        box = [self.state(self.device, parts)]
        done = torch.cuda.Event()
        done.record(self.be.stream)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        device, stream = self.device, self._copy_stream

        def job():
            with torch.cuda.device(device):
                done.synchronize()          # the writer waits for the snapshot, not the run
                with torch.cuda.stream(stream):
                    host = IO.to_host(box.pop())
            IO.write_checkpoint(host, path)
        self._writer.submit(job)
        return path

    def resume(self, path) -> None:
        """``load_state`` of a file that ``save_checkpoint`` wrote with all three parts."""
        self.load_state(CK.read_raw(str(path)))

    def close(self) -> None:
        """Wait for a background checkpoint write; re-raises what it raised."""
        self._writer.join()

    # -- the run
    def fit(self, batches, *, epochs: Optional[int] = None, on_log: Optional[Callable[[dict], None]] = None,
            log_every: Optional[int] = None, ckpt_dir=None, resume=None,
            preview: Optional[Callable[["Trainer", int], None]] = None, preview_every: int = 1) -> List[dict]:
        """Train over ``batches`` - any re-iterable of ``(images, labels, clip_pixel_values)``, iterated once per epoch -
        up to epoch ``epochs`` (exclusive; default ``cfg.training.max_epochs``).  Per epoch: ``set_epoch``, ``step()``
        per batch, ``flush()``, and with ``ckpt_dir`` a background ``save_checkpoint(ckpt_dir/last.ckpt)``.  After every
        ``log_every``-th optimizer step (default ``cfg.training.log_every_n_steps``, 50) ``pop_metrics()`` is taken,
        handed to ``on_log`` and kept; that is the loop's only synchronisation.  ``resume``: ``None``, ``"last"`` or a
        path (``training_io.resolve_resume``); training continues at the epoch after the saved one (the position inside
        an epoch is not kept: checkpoints are written at epoch ends).  A second call continues where the first stopped.
        ``preview``: after every ``preview_every``-th epoch (after its flush) ``sync_module("ema")`` and then
        ``preview(trainer, epoch)`` - the module samples with the averaged weights there; ``None`` leaves the loop as it is.
        -> the logged dicts."""
        path = IO.resolve_resume(resume, ckpt_dir)
        if path is not None:
            self.resume(path)
        epochs = self.max_epochs if epochs is None else int(epochs)
        log_every = self.log_every if log_every is None else max(1, int(log_every))
        logged: List[dict] = []

        def log():
            if self.steps % log_every == 0:
                logged.append(self.pop_metrics())
                if on_log is not None:
                    on_log(logged[-1])
        try:
            for e in range(self.next_epoch, epochs):
                self.set_epoch(e)
                for batch in batches:
                    before = self.steps
                    self.step(tuple(v.to(self.device, non_blocking=True) for v in batch))
                    if self.steps != before:
                        log()
                if self.flush():
                    log()
                self.next_epoch = e + 1
                if preview is not None and (e + 1) % max(1, int(preview_every)) == 0:
                    self.sync_module("ema")
                    preview(self, e)
                if ckpt_dir is not None:
                    self.save_checkpoint(os.path.join(str(ckpt_dir), IO.LAST), wait=False)
        finally:
            self.close()
        return logged
