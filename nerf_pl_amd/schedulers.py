"""Learning-rate warm-up of the reference's recipe (`--warmup_epochs`, `--warmup_multiplier`; utils/__init__.py:45-47 wraps the
scheduler of get_scheduler in utils/warmup_scheduler.py:4-58).

`GradualWarmupScheduler` ramps every group's lr linearly from its base value at epoch 0 to `multiplier` times that at epoch
`total_epoch`, then hands over to `after_scheduler`, whose base lrs it first rescales to the ramp's end value.  An lr change is
all the training step sees of it (`GraphedTrainStep` re-captures on one), so this is host code only.
"""
import warnings

from torch.optim.lr_scheduler import LRScheduler, ReduceLROnPlateau


class GradualWarmupScheduler(LRScheduler):
    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        if multiplier < 1.0:
            raise ValueError("multiplier must be >= 1 (the warm-up raises the lr towards multiplier * base lr), got %r" % (multiplier,))
        if isinstance(after_scheduler, ReduceLROnPlateau):
            # stepped with a metric, not an epoch: no recipe of configure_optimizers builds one
            raise NotImplementedError("GradualWarmupScheduler over ReduceLROnPlateau is not implemented")
        self.multiplier = multiplier
        self.total_epoch = total_epoch
        self.after_scheduler = after_scheduler
        self.finished = False             # True once the after-scheduler has taken over
        super().__init__(optimizer)       # performs the epoch-0 step: lr = base lr

    def get_lr(self):
        if self.last_epoch <= self.total_epoch:
            ramp = (self.multiplier - 1.0) * self.last_epoch / self.total_epoch + 1.0
            return [base * ramp for base in self.base_lrs]
        reached = [base * self.multiplier for base in self.base_lrs]
        if self.after_scheduler is None:
            return reached
        if not self.finished:
            self.after_scheduler.base_lrs = reached
            self.finished = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)      # torch: "use get_last_lr()" — the hand-over needs get_lr() itself
            return self.after_scheduler.get_lr()

    def step(self, epoch=None):
        if self.finished and self.after_scheduler is not None:
            self.after_scheduler.step(None if epoch is None else epoch - self.total_epoch)
            self._last_lr = self.after_scheduler.get_last_lr()
        elif epoch is None:
            super().step()
        else:
            super().step(epoch)
