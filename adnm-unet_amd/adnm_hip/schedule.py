"""The reference recipe's per-epoch schedules in closed form, host only: no torch optimiser, no device call.

  * learning rate (train_untils.py:44-46): LinearLR(start_factor=0.01, total_iters=3) for the warm-up, then CosineAnnealingLR(T_max=50,
    eta_min=5e-7), joined by SequentialLR at epoch 3; stepped once per epoch;
  * clip threshold (train.py:78-94, 122-130): norm_max through the warm-up, then a multiple of the PREVIOUS epoch's mean pre-clip
    gradient norm, eased in by a ramp; two parameter sets, chosen by frame_interval < 120 / input_frames.

`epoch` counts from 0 everywhere in this module (for epoch in range(schedule.epochs)): epoch e is the one train.py's loop calls e + 1,
and lr(e) is what the optimiser holds after e calls of lr_scheduler.step().

    sched = ReferenceSchedule(input_frames=5, frame_interval=6)
    prev = None
    for epoch in range(sched.epochs):
        sched.apply(trainer, epoch, prev)      # trainer.lr, trainer.max_norm: two host floats (the tail graph follows them)
        for x, tgt in loader:
            trainer.step(x, tgt)
        prev = trainer.stats(reset=True)       # FlatTrainer(monitor=True): the one synchronising read of the epoch
        for x, tgt in val_loader:
            validator.step(x, tgt)             # adnm_hip.validate.Validator
        d = selection.update(epoch, validator.done(reset=True)["loss_sum"])     # ReferenceSelection(sched)
        if d["save"]: ...                      # the best checkpoint (train.py:169-178)
        if d["stop"]: break                    # the early stop (train.py:205)
"""
import math


class ReferenceSchedule:
    # train.py:78-94: (save_epoch, norm_ratio, norm_max, norm_initial, grad_epoch_excursion)
    SHORT_INTERVAL = dict(save_epoch=34, norm_ratio=1.75, norm_max=0.025, norm_initial=0.175, excursion=1)   # frame_interval < 120 / input_frames
    LONG_INTERVAL = dict(save_epoch=20, norm_ratio=3.0, norm_max=0.035, norm_initial=0.065, excursion=0)

    def __init__(self, input_frames, frame_interval, base_lr=1e-3, eta_min=5e-7, warmup_epochs=3, t_max=50, epochs=40):
        if input_frames <= 0 or warmup_epochs < 1 or t_max < 1 or epochs < 1:
            raise ValueError("ReferenceSchedule: input_frames, warmup_epochs, t_max and epochs must be positive")
        self.input_frames, self.frame_interval = input_frames, frame_interval
        self.base_lr, self.eta_min = float(base_lr), float(eta_min)
        self.warmup_epochs, self.t_max, self.epochs = int(warmup_epochs), int(t_max), int(epochs)
        self.short_interval = frame_interval < 120 / input_frames
        p = self.SHORT_INTERVAL if self.short_interval else self.LONG_INTERVAL
        self.save_epoch, self.norm_ratio, self.norm_max = p["save_epoch"], p["norm_ratio"], p["norm_max"]
        self.norm_initial, self.excursion = p["norm_initial"], p["excursion"]
        # train.py:127: the last epoch (train.py's numbering) of the ramp, and the ramp's denominator
        self.ramp_end = self.save_epoch - self.warmup_epochs + self.excursion

    def lr(self, epoch):
        """learning rate of epoch `epoch` (0-based): base_lr * (0.01 + 0.99 * epoch / warmup) during the warm-up, then the cosine from
        base_lr at epoch == warmup towards eta_min at warmup + t_max"""
        if epoch < 0:
            raise ValueError(f"ReferenceSchedule.lr: epoch {epoch} < 0")
        w = self.warmup_epochs
        if epoch < w:
            return self.base_lr * (0.01 + (1.0 - 0.01) * epoch / w)
        return self.eta_min + (self.base_lr - self.eta_min) * (1.0 + math.cos(math.pi * (epoch - w) / self.t_max)) / 2.0

    def max_norm(self, epoch, prev_avg_norm):
        """clip_grad_norm_ threshold of epoch `epoch` (0-based) given the mean pre-clip norm of the epoch before (ignored, and may be
        None, while the threshold is norm_max).  With e1 = epoch + 1, train.py's own counter:
            e1 <= warmup + 1:   norm_max
            e1 <= ramp_end:     (norm_initial + (1 - norm_initial) * (e1 - warmup) / ramp_end) * norm_ratio * prev_avg_norm
            later:              norm_ratio * prev_avg_norm
        The ramp's factor reaches norm_initial + (1 - norm_initial) * (ramp_end - warmup) / ramp_end < 1 in its last epoch: the
        threshold steps up to the plain multiple one epoch later, as in the reference."""
        if epoch < 0:
            raise ValueError(f"ReferenceSchedule.max_norm: epoch {epoch} < 0")
        e1 = epoch + 1
        if e1 <= self.warmup_epochs + 1:
            return self.norm_max
        if prev_avg_norm is None:
            raise ValueError(f"ReferenceSchedule.max_norm: epoch {epoch} needs the previous epoch's mean gradient norm")
        if e1 <= self.ramp_end:
            alpha = self.norm_initial + (1 - self.norm_initial) * (e1 - self.warmup_epochs) / self.ramp_end
            return alpha * self.norm_ratio * prev_avg_norm
        return self.norm_ratio * prev_avg_norm

    def apply(self, trainer, epoch, prev_stats=None):
        """set trainer.lr and trainer.max_norm for epoch `epoch`; prev_stats: what trainer.stats() returned at the end of the epoch
        before (its "norm_mean" is read), None before the first epoch.  Returns (lr, max_norm)."""
        prev = None if prev_stats is None else prev_stats["norm_mean"]
        lr, mn = self.lr(epoch), self.max_norm(epoch, prev)
        trainer.lr = lr
        trainer.max_norm = mn
        return lr, mn


class ReferenceSelection:
    """The decisions train.py takes on the validation loss of every epoch, in closed form, for the ADNM-UNet recipe (if_save_epoch and
    if_early_stop both true): save the best checkpoint only after `save_epoch` epochs (train.py:169-178), count the epochs that did not
    improve on it, stop at `early_stop` of them in a row (train.py:179-183, 205; train_untils.py:47-50: 3 for the short-interval recipe,
    5 for the long one).  `val_loss_sum` is the SUM of the per-batch validation losses (train.py:163), Validator.done()["loss_sum"].

    With e1 = epoch + 1 (train.py's counter; `epoch` is 0-based as everywhere in this module) and best = 10000 at the start:
        e1 <= save_epoch:                      nothing changes (no save, no count, however good the loss)
        e1 >  save_epoch and loss <  best:     save, best = loss, bad_epochs = 0
        e1 >  save_epoch and not (loss < best): bad_epochs += 1        (an equal loss and a NaN loss are "not better")
        stop = bad_epochs >= early_stop"""

    def __init__(self, schedule):
        self.save_epoch = int(schedule.save_epoch)
        self.early_stop = 3 if schedule.short_interval else 5
        self.best, self.bad_epochs = 10000.0, 0

    def update(self, epoch, val_loss_sum):
        if epoch < 0:
            raise ValueError(f"ReferenceSelection.update: epoch {epoch} < 0")
        loss, save = float(val_loss_sum), False
        if epoch + 1 > self.save_epoch:
            if loss < self.best:   # False for a NaN
                save, self.best, self.bad_epochs = True, loss, 0
            else:
                self.bad_epochs += 1
        return {"save": save, "stop": self.bad_epochs >= self.early_stop, "best": self.best, "bad_epochs": self.bad_epochs}

    def state_dict(self):
        """plain Python scalars: fits checkpoint.save_training_state's schedule_stats as it is"""
        return {"best": float(self.best), "bad_epochs": int(self.bad_epochs), "save_epoch": int(self.save_epoch), "early_stop": int(self.early_stop)}

    def load_state_dict(self, sd):
        if int(sd["save_epoch"]) != self.save_epoch or int(sd["early_stop"]) != self.early_stop:
            raise ValueError(f"ReferenceSelection.load_state_dict: saved for save_epoch {sd['save_epoch']} / early_stop {sd['early_stop']}, "
                             f"this recipe has {self.save_epoch} / {self.early_stop}")
        self.best, self.bad_epochs = float(sd["best"]), int(sd["bad_epochs"])
