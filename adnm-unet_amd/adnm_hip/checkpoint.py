"""Checkpoint compatibility with the reference: train.py:169-178 saves `model.state_dict()` as
<model>_best.pth — with a `module.` prefix on every key when train.py:99-102 wrapped the model in nn.DataParallel — and
validate.py:86 / train.py:210 load it back.  The 992 keys and shapes are part of the drop-in boundary."""
import torch

PREFIX = "module."


def strip_prefix(state_dict):
    """nn.DataParallel's `module.` prefix off every key (a no-op for plain checkpoints)."""
    if state_dict and all(k.startswith(PREFIX) for k in state_dict):
        return {k[len(PREFIX):]: v for k, v in state_dict.items()}
    return dict(state_dict)


def load_reference_checkpoint(model, source, map_location="cpu"):
    """Load a reference `*_best.pth` (path or already-loaded state_dict, with or without the DataParallel prefix) into `model`
    after checking that the two key sets and every shape agree.  Works on a model whose parameters FlatTrainer has already re-homed
    into its flat buffer: load_state_dict copies in place, so the flat buffer receives the values, and the copies move the parameters'
    version counters, so the trainer's narrow bf16 / fp8 weight shadow is rewritten (fp8: weight scales re-derived) before the next eager
    forward, GraphedForward replay or training step reads it (ops.ShadowSet).  Returns the number of tensors."""
    sd = torch.load(source, map_location=map_location) if isinstance(source, (str, bytes)) or hasattr(source, "read") else source
    if _is_training_state(sd):   # a save_training_state file: its model part is a reference checkpoint
        sd = sd["model"]
    sd = strip_prefix(sd)
    own = model.state_dict()
    missing, unexpected = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    if missing or unexpected:
        raise RuntimeError(f"checkpoint does not match the model: {len(missing)} missing (e.g. {missing[:3]}), {len(unexpected)} unexpected (e.g. {unexpected[:3]})")
    bad = [(k, tuple(sd[k].shape), tuple(own[k].shape)) for k in own if tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError(f"checkpoint shapes differ from the model's for {len(bad)} tensors, e.g. {bad[:3]}")
    model.load_state_dict(sd, strict=True)
    return len(sd)


def save_reference_checkpoint(model, path, data_parallel_prefix=False):
    """torch.save(model.state_dict()) as train.py:174 does: logical shapes, contiguous CPU tensors (independent of the flat buffer's
    layout), optionally with the `module.` prefix a DataParallel run of the reference would have written."""
    sd = {(PREFIX + k if data_parallel_prefix else k): v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.save(sd, path)
    return len(sd)


# ------------------------------------------------------------------------------------------------ stop and go on
TRAINING_STATE = "adnm_training_state"


def _is_training_state(blob):
    return isinstance(blob, dict) and blob.get("format") == TRAINING_STATE


def _read(source, map_location="cpu"):
    return torch.load(source, map_location=map_location) if isinstance(source, (str, bytes)) or hasattr(source, "read") else source


def _model_part(model):
    """model.state_dict() as save_reference_checkpoint writes it; every tensor owns its memory (a CPU parameter is a view into the
    trainer's flat buffer: saving the view would save the buffer)"""
    return {k: v.detach().to("cpu", copy=True).contiguous() for k, v in model.state_dict().items()}


def save_training_state(trainer, path, schedule_stats=None):
    """One file to stop a run and go on bit for bit: model.state_dict() (the reference's checkpoint: load_reference_checkpoint reads
    this file too), FlatTrainer.state_dict(), and optionally the last stats() dict of a monitored epoch, which
    schedule.ReferenceSchedule.apply needs for the next epoch's clip threshold.  SYNCHRONISES (FlatTrainer.snapshot() is the form that
    does not).  Returns the number of model tensors."""
    blob = {"format": TRAINING_STATE, "version": 1, "model": _model_part(trainer.model), "trainer": trainer.state_dict(),
            "schedule_stats": None if schedule_stats is None else dict(schedule_stats)}
    torch.save(blob, path)
    return len(blob["model"])


def load_training_state(trainer, source, strict=True):
    """The other direction, in this order: the parameters through model.load_state_dict (in place; the copies move the version
    counters, so a narrow weight shadow counts as stale), then FlatTrainer.load_state_dict (which rewrites the shadow, fp8 with the
    restored scales).  Works on a prepared trainer (its graphs stay valid) and on a fresh one (the state waits for the flat layout).
    Returns the stored schedule_stats (None when none were saved)."""
    blob = _read(source)
    if not _is_training_state(blob):
        raise RuntimeError("load_training_state: not a file written by save_training_state (a reference checkpoint holds the model only: "
                           "load_reference_checkpoint)")
    load_reference_checkpoint(trainer.model, blob["model"])
    trainer.load_state_dict(blob["trainer"], strict=strict)
    return blob.get("schedule_stats")


def to_torch_adamw_state(trainer, sd=None):
    """The optimiser state in torch.optim.AdamW.state_dict() form, for an optimiser built over model.parameters() in one group:
    state[i] = {"step", "exp_avg", "exp_avg_sq"} with i the position in model.parameters() — only for the parameters the trainer
    updates, as torch keeps no state for a parameter that never had a gradient — and one param group with lr, betas, eps and
    weight_decay.  A run started here goes on under the unmodified reference (train_untils.py:35-42).  sd: a state_dict() / snapshot
    state to convert instead of the trainer's current one."""
    sd = trainer.state_dict() if sd is None else sd
    params = list(trainer.model.parameters())
    index = {id(p): i for i, p in enumerate(params)}
    named = dict(trainer.model.named_parameters())
    # the optimiser steps APPLIED: the device's counter where the fused kernels keep it (a skipped step leaves it alone)
    step = float(sd["state_bits"].view(torch.float32)[0]) if trainer.fused else float(sd["steps"])
    state = {}
    for name, ent in sd["params"].items():
        state[index[id(named[name])]] = {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": ent["exp_avg"].clone(),
                                         "exp_avg_sq": ent["exp_avg_sq"].clone()}
    probe = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=sd["lr"], betas=tuple(sd["betas"]), eps=sd["eps"],
                              weight_decay=sd["weight_decay"])
    group = dict(probe.state_dict()["param_groups"][0])   # (this torch's full set of group keys)
    group["params"] = list(range(len(params)))
    return {"state": dict(sorted(state.items())), "param_groups": [group]}


def from_torch_adamw_state(trainer, opt_sd, strict=True):
    """Take over a torch.optim.AdamW.state_dict() (one param group over model.parameters()): moments, step count and lr; betas, eps and
    weight_decay must be the trainer's (strict=False: the trainer keeps its own).  max_norm, an accumulation cycle, the monitor block,
    the fp8 table and the average of the weights (ema_decay) are not torch's to give and stay as they are.  Like load_state_dict: in place on a prepared trainer, kept for
    the flat layout on a fresh one."""
    groups = opt_sd["param_groups"]
    if len(groups) != 1:
        raise RuntimeError(f"from_torch_adamw_state: one param group over model.parameters() expected, got {len(groups)}")
    if trainer.micro_step != 0:
        raise RuntimeError(f"from_torch_adamw_state: an accumulation cycle is open (micro-step {trainer.micro_step}); finish it first")
    g = groups[0]
    params = list(trainer.model.parameters())
    if len(g["params"]) != len(params):
        raise RuntimeError(f"from_torch_adamw_state: the group names {len(g['params'])} parameters, the model has {len(params)}")
    name_of = {id(p): n for n, p in trainer.model.named_parameters()}
    pos = {idx: i for i, idx in enumerate(g["params"])}
    per, steps = {}, set()
    for idx, st in opt_sd["state"].items():
        per[name_of[id(params[pos[idx]])]] = {"exp_avg": st["exp_avg"].detach().cpu(), "exp_avg_sq": st["exp_avg_sq"].detach().cpu()}
        steps.add(float(st["step"]))
    if len(steps) > 1:
        raise RuntimeError(f"from_torch_adamw_state: the parameters are at different steps {sorted(steps)}; the flat optimiser keeps one")
    step = steps.pop() if steps else 0.0
    bits = trainer.state.detach().cpu().clone() if trainer.used is not None else torch.zeros(4, dtype=torch.float32)
    if trainer.fused:   # the device's step counter (the bias corrections behind it are re-made from it by every optimiser pass before
        bits[0] = step  # they are read); the torch-ops path counts on the host alone
    sd = trainer._scalars()
    sd.update(steps=int(step), lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]), eps=float(g["eps"]),
              weight_decay=float(g["weight_decay"]), micro_step=0, state_bits=bits.view(torch.int32), params=per, monitor=None, fp8=None)
    trainer._load(sd, strict, quant=False, ema=False)
