"""The file layer of a training run: the two schedule decisions of ``training.Trainer`` as pure functions, the checkpoint
layout (``pack`` / ``load``), the atomic writer, the one-thread background writer and the resume rule.  Plain torch: it
imports without a device, works on any ``optim.ParamArena`` + ``optim.FusedAdamW`` (``be=None`` included) and launches no
kernel.

The layout is Lightning-shaped where ``checkpoint.select_state`` and the reference read it:

  ``epoch``, ``global_step``   ints (``global_step`` counts optimizer steps)
  ``state_dict``               the EMA of the weights (the reference's EMA callback rewrites the file this way,
                               src/callbacks/ema_callback.py:291-324); the raw weights when the EMA part is left out
  ``current_model_state``      the raw weights (absent when the EMA or the raw part is left out)
  ``optimizer_states``         ``[FusedAdamW.state_dict()]`` plus ``"format": OPTIMIZER_FORMAT``: torch.optim.AdamW's
                               layout with the parameters in ARENA order and the UNet's convs in the library layout
                               ``[O][kh*kw*I]``, the loss scale under ``"scaler"``.  The reference's optimizer numbers its
                               parameters in module order and holds OIHW moments: it cannot load this entry.
  ``lr_schedulers``            ``[{"last_epoch": epoch}]``
  ``callbacks``                ``{"EMAWeightAveraging": {"latest_update_step": ...}}``
  ``rng``                      ``{"cpu": ..., "cuda": ...}``: generator states (uint8 tensors)
  ``dadd``                     ``{"format": FORMAT, "operand_dtype": "torch.float16", "accumulate": k}``

Plain containers, numbers, strings and tensors only: the file passes ``checkpoint.read_raw``
(``torch.load(weights_only=True)``) unchanged.
"""
from __future__ import annotations

import os
import threading
import warnings
from collections import OrderedDict
from pathlib import Path
from typing import Callable, Dict, List, Mapping, Optional, Sequence

import torch

FORMAT = 1
OPTIMIZER_FORMAT = "dadd.FusedAdamW/1"
PARTS = ("ema", "raw", "optimizer")
EMA_CALLBACK = "EMAWeightAveraging"
LAST = "last.ckpt"


# ---- the two schedule decisions ------------------------------------------------------------------------------------------
def optimizer_step_due(pending: int, accumulate: int) -> bool:
    """Does the call that made ``pending`` micro-batches wait step the optimizer?  Every ``accumulate``-th one does."""
    if accumulate < 1:
        raise ValueError(f"accumulate_grad_batches must be at least 1, got {accumulate}")
    return pending >= accumulate


def ema_due(step: int, start: int, every: int) -> bool:
    """Is the EMA updated at optimizer step ``step`` (1 = the first)?  From ``update_starting_at_step`` on, every
    ``update_every_n_steps``-th optimizer step; micro-batches do not count (src/callbacks/ema_callback.py:105-108)."""
    return step >= start and step % max(1, every) == 0


def run_schedule(batches: int, accumulate: int):
    """The optimizer steps of one epoch of ``batches`` calls: ``(steps, flush)`` with ``steps[i]`` whether call i + 1 steps
    and ``flush`` whether a short last group is left for ``Trainer.flush()``."""
    steps, pending = [], 0
    for _ in range(batches):
        pending += 1
        due = optimizer_step_due(pending, accumulate)
        steps.append(due)
        if due:
            pending = 0
    return steps, pending > 0


# ---- state <-> dict -------------------------------------------------------------------------------------------------------
def _named(arena, view) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, view(k)) for k in arena.names)


def _copy(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, copy=True)


def default_generators(device=None) -> Dict[str, torch.Generator]:
    """``{"cpu": torch's default generator}`` and, for a CUDA / ROCm device, ``"cuda"``: that device's default generator."""
    gens = {"cpu": torch.default_generator}
    device = torch.device(device) if device is not None else None
    if device is not None and device.type == "cuda":
        torch.cuda.init()
        gens["cuda"] = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    return gens


def pack(arena, optimizer, *, epoch: int, global_step: int, latest_update_step: int, accumulate: int = 1,
         parts: Sequence[str] = PARTS, device="cpu", export: Optional[Callable] = None,
         generators: Optional[Mapping[str, torch.Generator]] = None) -> dict:
    """The checkpoint dict of the module docstring, every tensor a copy on ``device``.

    ``export(view)`` turns a name -> tensor accessor of the arena (``arena.param`` / ``arena.ema_param``) into the weight
    dict to store, already on ``device`` (``Trainer`` gives reference key names, OIHW convs, gates and frozen tensors);
    the default stores the arena's tensors under their own names.  ``parts`` chooses among ``"ema"``, ``"raw"`` and
    ``"optimizer"``; only a dict with all three restores a run.  ``generators``: name -> ``torch.Generator`` whose state
    goes under ``rng`` (default ``default_generators(arena.device)``).  Synchronises (``FusedAdamW.state_dict``)."""
    parts = tuple(parts)
    bad = [p for p in parts if p not in PARTS]
    if bad or not ({"ema", "raw"} & set(parts)):
        raise ValueError(f"parts {parts}: choose among {PARTS}, with at least one of 'ema' and 'raw'")
    if "ema" in parts and arena.ema is None:
        raise ValueError("the arena has no EMA to save")
    if export is None:
        def export(view):
            return OrderedDict((k, _copy(v, device)) for k, v in _named(arena, view).items())
    out = {"epoch": int(epoch), "global_step": int(global_step)}
    if "ema" in parts:
        out["state_dict"] = export(arena.ema_param)
        if "raw" in parts:
            out["current_model_state"] = export(arena.param)
    else:
        out["state_dict"] = export(arena.param)
    if "optimizer" in parts:
        osd = optimizer.state_dict()
        osd["state"] = {i: {"step": st["step"].clone(), "exp_avg": _copy(st["exp_avg"], device),
                            "exp_avg_sq": _copy(st["exp_avg_sq"], device)} for i, st in osd["state"].items()}
        osd["format"] = OPTIMIZER_FORMAT
        out["optimizer_states"] = [osd]
    gens = generators if generators is not None else default_generators(arena.device)
    out["lr_schedulers"] = [{"last_epoch": int(epoch)}]
    out["callbacks"] = {EMA_CALLBACK: {"latest_update_step": int(latest_update_step)}}
    out["rng"] = {k: g.get_state().clone() for k, g in gens.items()}
    out["dadd"] = {"format": FORMAT, "operand_dtype": str(arena.p16.dtype) if arena.p16 is not None else "none",
                   "accumulate": int(accumulate), "parts": list(parts)}
    return out


def _first(items: List[str], n: int = 6) -> str:
    return "; ".join(items[:n]) + (f" ... ({len(items)} in all)" if len(items) > n else "")


def check(state: Mapping, arena, *, to_masters: Optional[Callable] = None, ignore: Sequence[str] = ()):
    """Everything ``load`` refuses, before it changes anything: an unknown ``format``, a dict without all three parts,
    another operand type, weight names / shapes and optimizer groups that are not the arena's.  ``ValueError`` names the
    first mismatches.  -> ``(raw masters, EMA masters)`` by arena name."""
    tag = state.get("dadd") if isinstance(state, Mapping) else None
    if not isinstance(tag, Mapping) or tag.get("format") != FORMAT:
        raise ValueError(f"checkpoint format {None if not isinstance(tag, Mapping) else tag.get('format')!r}: this library "
                         f"reads format {FORMAT} (the 'dadd' entry of a file that Trainer.save_checkpoint wrote)")
    lacking = [k for k in ("state_dict", "current_model_state", "optimizer_states", "rng") if k not in state]
    if lacking:
        raise ValueError(f"the checkpoint lacks {lacking} (saved with parts {tag.get('parts')}): a run resumes only from "
                         f"the three parts {PARTS}")
    want = str(arena.p16.dtype) if arena.p16 is not None else "none"
    if tag.get("operand_dtype") != want:
        raise ValueError(f"the checkpoint was trained with {tag.get('operand_dtype')} operands, this trainer runs {want}")
    to_masters = to_masters if to_masters is not None else (lambda sd: sd)
    raw, ema = to_masters(state["current_model_state"]), to_masters(state["state_dict"])
    ignore = set(ignore)
    for label, sd in (("current_model_state", raw), ("state_dict", ema)):
        missing = [k for k in arena.names if k not in sd]
        extra = [k for k in sd if k not in arena.offsets and k not in ignore]
        if missing or extra:
            raise ValueError(f"{label} does not hold the trainer's parameters: missing {_first(missing) or 'none'}; "
                             f"unexpected {_first(extra) or 'none'}")
        shapes = [f"{k}: file {tuple(sd[k].shape)} vs trainer {tuple(arena.shapes[k])}" for k in arena.names
                  if tuple(sd[k].shape) != tuple(arena.shapes[k])]
        if shapes:
            raise ValueError(f"{label}: shape mismatch for {_first(shapes)}")
    osd = state["optimizer_states"][0]
    if osd.get("format") != OPTIMIZER_FORMAT:
        raise ValueError(f"optimizer_states[0] has format {osd.get('format')!r}, expected {OPTIMIZER_FORMAT!r} (arena order, "
                         "library layout); another optimizer's state is not loadable")
    sizes = [len(g["params"]) for g in osd["param_groups"]]
    if sizes != [len(n) for n in arena.group_names]:
        raise ValueError(f"the optimizer's parameter groups hold {sizes} tensors, the trainer's {[len(n) for n in arena.group_names]}")
    names = [k for gi in range(arena.n_groups) for k in arena.group_names[gi]]
    order = [i for g in osd["param_groups"] for i in g["params"]]
    shapes = [f"{k}: exp_avg {tuple(osd['state'][i]['exp_avg'].shape)} vs trainer {tuple(arena.shapes[k])}"
              for k, i in zip(names, order) if i in osd["state"] and
              tuple(osd["state"][i]["exp_avg"].shape) != tuple(arena.shapes[k])]
    if shapes:
        raise ValueError(f"optimizer_states: shape mismatch for {_first(shapes)}")
    return raw, ema


def load(state: Mapping, arena, optimizer, *, to_masters: Optional[Callable] = None, ignore: Sequence[str] = (),
         generators: Optional[Mapping[str, torch.Generator]] = None) -> dict:
    """Restore ``p``, the EMA, ``m``, ``v``, the optimizer's state block (step, rates, loss scale, growth tracker), the
    16-bit copy and the generators from a dict of ``pack`` (or a file of it read with ``checkpoint.read_raw``), after
    ``check``.  ``to_masters`` is the inverse of ``pack``'s ``export`` (weight dict -> tensors by arena name); keys it
    leaves that are listed in ``ignore`` are not the arena's business.  -> ``{"epoch", "global_step",
    "latest_update_step", "accumulate"}`` for the caller's own counters."""
    raw, ema = check(state, arena, to_masters=to_masters, ignore=ignore)
    with torch.no_grad():
        for k in arena.names:
            arena.param(k).copy_(raw[k])
            arena.ema_param(k).copy_(ema[k])
        optimizer.load_state_dict(state["optimizer_states"][0])
        if arena.p16 is not None:
            arena.p16.copy_(arena.p)
    gens = generators if generators is not None else default_generators(arena.device)
    for k, g in gens.items():
        if k in state["rng"]:
            g.set_state(state["rng"][k].cpu())
    cb = state.get("callbacks", {}).get(EMA_CALLBACK, {})
    return {"epoch": int(state["epoch"]), "global_step": int(state["global_step"]),
            "latest_update_step": int(cb.get("latest_update_step", 0)), "accumulate": int(state["dadd"].get("accumulate", 1))}


# ---- files ---------------------------------------------------------------------------------------------------------------
def to_host(obj):
    """The same containers with every tensor on the CPU."""
    if isinstance(obj, torch.Tensor):
        return obj.cpu()
    if isinstance(obj, Mapping):
        return type(obj)((k, to_host(v)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_host(v) for v in obj)
    return obj


def write_checkpoint(state: Mapping, path, serializer: Callable = torch.save) -> str:
    """``serializer(state, path + ".tmp")`` and then ``os.replace``: a reader sees the previous file or the new one, never
    a part of one.  When the serializer raises, the temporary file is removed and the previous file stays."""
    path = str(path)
    tmp = path + ".tmp"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    try:
        serializer(state, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


class BackgroundWriter:
    """One write at a time on one background thread, in the manner of ``generation.FrameSink``: ``submit(job)`` joins the
    previous job and starts ``job()``; ``join()`` waits for it and re-raises what it raised; ``close()`` joins."""

    def __init__(self):
        self._thread: Optional[threading.Thread] = None
        self._error: Optional[BaseException] = None

    def _run(self, job):
        try:
            job()
        except BaseException as e:      # surfaces at the join
            self._error = e

    def submit(self, job: Callable[[], None]) -> None:
        self.join()
        self._thread = threading.Thread(target=self._run, args=(job,), name="checkpoint-writer", daemon=False)
        self._thread.start()

    @property
    def busy(self) -> bool:
        return self._thread is not None and self._thread.is_alive()

    def join(self) -> None:
        t, self._thread = self._thread, None
        if t is not None:
            t.join()
        e, self._error = self._error, None
        if e is not None:
            raise e

    close = join


def resolve_resume(resume, ckpt_dir=None) -> Optional[str]:
    """The reference's ``_resolve_checkpoint_path`` (src/pipelines/training/training_pipeline_ip.py:30-51): ``None`` ->
    ``None`` (train from scratch); ``"last"`` (any case) -> ``ckpt_dir/last.ckpt``; any other value -> that path, resolved,
    and ``FileNotFoundError`` when it does not exist.  The reference hands ``"last"`` to Lightning, which starts from
    scratch when the directory holds no ``last.ckpt`` yet; so does this: it warns and returns ``None``, and a job that is
    always started with ``resume="last"`` runs its first time too."""
    if resume is None:
        return None
    resume = str(resume)
    if resume.lower() == "last":
        if ckpt_dir is None:
            raise ValueError('resume="last" needs ckpt_dir: it names ckpt_dir/last.ckpt')
        last = Path(ckpt_dir).expanduser().resolve() / LAST
        if not last.exists():
            warnings.warn(f'resume="last": {last} does not exist yet; training starts from scratch', RuntimeWarning,
                          stacklevel=2)
            return None
        return str(last)
    resolved = Path(resume).expanduser().resolve()
    if not resolved.exists():
        raise FileNotFoundError(f"Resume checkpoint not found: {resolved}\n"
                                "Pass resume=None to train from scratch.")
    return str(resolved)
