"""`lvdm.lr_scheduler.get_scheduler`: the learning-rate schedules of the training yaml's `lr_g_scheduler_config` /
`lr_d_scheduler_config` as plain `torch.optim.lr_scheduler.LambdaLR`s.  Nothing here needs `transformers`."""
import math
from typing import Optional

from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

SCHEDULES = ("constant", "constant_with_warmup", "linear", "cosine")


def _warmup(step: int, warmup: int) -> float:
    return float(step) / float(max(1, warmup))


def constant_with_warmup_multiplier(step: int, num_warmup_steps: int) -> float:
    return _warmup(step, num_warmup_steps) if step < num_warmup_steps else 1.0


def linear_multiplier(step: int, num_warmup_steps: int, num_training_steps: int) -> float:
    """0 -> 1 over the warm-up, then a straight line down to 0 at num_training_steps"""
    if step < num_warmup_steps:
        return _warmup(step, num_warmup_steps)
    return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))


def cosine_multiplier(step: int, num_warmup_steps: int, num_training_steps: int, min_lr_ratio: float = 0.0) -> float:
    """s / max(1, W) for s < W, else max(0, 1/2 ((1 + r) + (1 - r) cos(pi (s - W) / max(1, N - W)))): half a cosine from 1 at the end of
    the warm-up down to r = min_lr_ratio at N (and back up beyond N, as the formula goes)"""
    if step < num_warmup_steps:
        return _warmup(step, num_warmup_steps)
    progress = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
    return max(0.0, 0.5 * ((1.0 + min_lr_ratio) + (1.0 - min_lr_ratio) * math.cos(math.pi * progress)))


def get_scheduler(name, optimizer: Optimizer, num_warmup_steps: Optional[int] = None, num_training_steps: Optional[int] = None,
                  min_lr_ratio: Optional[float] = 0.0) -> LambdaLR:
    """name: 'constant' | 'constant_with_warmup' | 'linear' | 'cosine' (a str, or an enum whose value is one).  min_lr_ratio shapes the
    cosine schedule only."""
    name = str(getattr(name, "value", name))
    if name not in SCHEDULES:
        raise NotImplementedError(f"lr schedule {name!r}: this repository implements {', '.join(SCHEDULES)}")
    if name == "constant":
        return LambdaLR(optimizer, lambda _: 1.0)
    if num_warmup_steps is None:
        raise ValueError(f"{name} requires `num_warmup_steps`, please provide that argument.")
    if name == "constant_with_warmup":
        return LambdaLR(optimizer, lambda s: constant_with_warmup_multiplier(s, num_warmup_steps))
    if num_training_steps is None:
        raise ValueError(f"{name} requires `num_training_steps`, please provide that argument.")
    if name == "linear":
        return LambdaLR(optimizer, lambda s: linear_multiplier(s, num_warmup_steps, num_training_steps))
    r = 0.0 if min_lr_ratio is None else float(min_lr_ratio)
    return LambdaLR(optimizer, lambda s: cosine_multiplier(s, num_warmup_steps, num_training_steps, r))
