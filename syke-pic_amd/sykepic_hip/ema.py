"""Exponential moving average (EMA) of the weights during training (the usual fine-tuning recipe, e.g. timm's
``ModelEmaV2`` and torchvision's classification reference; not in sykefi/syke-pic).

The average lives inside the library, in a second flat float32 buffer in the layout of the model's own
(``spk_model_ema_*``, include/sykepic_hip.h): every parameter and every float buffer - BatchNorm running mean and
variance too - but not the int64 ``num_batches_tracked``.  It starts as a COPY of the model when it is enabled, and after
every optimizer step one kernel moves it towards the model, ``avg += (1 - d) * (model - avg)``.  `ModelEma` keeps the
schedule of ``d`` and the count of updates on the host; `HipNet.ema_swap` exchanges model and average, so that
validation and the ``best_state.pth`` save see the average while the raw weights keep training.
"""

import contextlib
import math

import numpy as np

WARMUP_NUM, WARMUP_DEN = 1.0, 10.0


def decay_at(decay, warmup, t):
    """The decay ``d`` of update number `t` (1-based).  With warm-up ``min(decay, (1 + t) / (10 + t))``: 2/11 at the
    first update, so that the first steps are not averaged against the start for thousands of updates; it reaches
    `decay` where ``(1 + t) / (10 + t) >= decay``.  Without warm-up `decay` itself."""
    t = int(t)
    if t < 1:
        raise ValueError(f"updates are counted from 1. Got: {t}")
    decay = float(decay)
    return min(decay, (WARMUP_NUM + t) / (WARMUP_DEN + t)) if warmup else decay


def weight_of(d):
    """The kernel's float32 weight ``1 - d``: formed in double, rounded once."""
    return float(np.float32(1.0 - float(d)))


def describe(decay, warmup):
    """What `train_state.pth` records of the settings (`ModelEma.describe`); None when the average is off."""
    decay = float(decay)
    return {"decay": decay, "warmup": bool(warmup)} if decay > 0.0 else None


def same_settings(a, b):
    """Two `describe` dicts (None: no average) name the same averaging."""
    if not a or not b:
        return not a and not b
    return float(a.get("decay", -1.0)) == float(b.get("decay", -1.0)) and bool(a.get("warmup", True)) == bool(b.get("warmup", True))


def show_settings(d):
    return "off" if not d else f"decay {float(d.get('decay', 0.0)):g}, warmup {'yes' if d.get('warmup', True) else 'no'}"


class ModelEma:
    """``ModelEma(net, decay, warmup=True)``: enables the average of `net` (a copy of its tensors as they are now) and
    counts the updates.  `decay` inside (0, 1)."""

    def __init__(self, net, decay, warmup=True):
        self.decay, self.warmup = float(decay), bool(warmup)
        if not (0.0 < self.decay < 1.0) or not math.isfinite(self.decay):
            raise ValueError(f"ema_decay must be inside (0, 1) for a ModelEma. Got: {decay}")
        w = weight_of(self.decay)
        if not 0.0 < w < 1.0:
            raise ValueError(f"ema_decay {decay}: 1 - decay is not a float32 inside (0, 1)")
        self.net = net
        self.updates = 0
        net.ema_enable(True)

    def describe(self):
        return describe(self.decay, self.warmup)

    def update(self):
        """After `optimizer.step()`: one more update, with the decay of its number."""
        self.updates += 1
        self.net.ema_update(weight_of(decay_at(self.decay, self.warmup, self.updates)))

    @contextlib.contextmanager
    def applied(self):
        """``with model_ema.applied():`` the net IS the average (evaluation, `state_dict()`); the raw weights come back
        at the end of the block, whatever ends it (`KeyboardInterrupt` included)."""
        self.net.ema_swap()
        try:
            yield self.net
        finally:
            self.net.ema_swap()

    def state_dict(self):
        """For `train_state.pth`: the averaged tensors (float keys of `state_dict()`, in its order) and the count."""
        return {"tensors": dict(self.net.ema_state_dict()), "updates": int(self.updates)}

    def load_state_dict(self, state):
        self.net.load_ema_state_dict(state["tensors"])
        self.updates = int(state["updates"])
        return self
