"""Mixup / CutMix of a training batch on the GPU (torchvision's reference recipe: ``RandomMixup`` / ``RandomCutmix`` of
its classification references; not in sykefi/syke-pic).

A batch is mixed with itself rolled by one image (row ``i`` with row ``i - 1``); one ``lam`` - and for CutMix one box -
serves the whole batch.  The draws stay on the host, in a generator of this object's own (the loader's batch thread
draws the augmentation parameters of later batches from the module-level ``random`` meanwhile); the kernel
(``spk_mix_batch``, csrc/augment.hip) applies them to the device batch, uint8 NHWC or float32 NCHW.  The loss of a mixed
batch is ``lam * CE(out, ya) + (1 - lam) * CE(out, yb)`` (``HipNet.forward_backward(x, ya, y2=yb, lam=lam)``).
"""

import math
import random
import struct
from collections import namedtuple

MIXUP, CUTMIX = "mixup", "cutmix"

# kind: MIXUP / CUTMIX; lam: the weight of the batch's own labels (for CutMix recomputed from the clipped box);
# ca, cb: the float32 coefficients of the kernel; box: (y1, x1, y2, x2), half open
MixPlan = namedtuple("MixPlan", "kind lam ca cb box")


def f32(v):
    """v rounded to the nearest float32, as a Python float."""
    return struct.unpack("f", struct.pack("f", v))[0]


class BatchMix:
    """``BatchMix(mixup_alpha, cutmix_alpha, prob, switch_prob, seed)``: with probability `prob` a batch is mixed - by
    CutMix with probability `switch_prob` when both alphas are positive, else by the one whose alpha is - with
    ``lam ~ Beta(alpha, alpha)``."""

    def __init__(self, mixup_alpha, cutmix_alpha, prob=1.0, switch_prob=0.5, seed=0):
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        if not (self.mixup_alpha >= 0.0 and self.cutmix_alpha >= 0.0 and math.isfinite(self.mixup_alpha + self.cutmix_alpha)):
            raise ValueError(f"mixup_alpha and cutmix_alpha must be >= 0. Got: {mixup_alpha}, {cutmix_alpha}")
        if self.mixup_alpha == 0.0 and self.cutmix_alpha == 0.0:
            raise ValueError("BatchMix needs mixup_alpha > 0 or cutmix_alpha > 0 (both 0: build no BatchMix)")
        if not (0.0 <= self.prob <= 1.0 and 0.0 <= self.switch_prob <= 1.0):
            raise ValueError(f"prob and switch_prob must be between 0.0 and 1.0. Got: {prob}, {switch_prob}")
        self.seed = int(seed)
        self._rng = random.Random(self.seed)    # never the module-level generator: see the module docstring

    def describe(self):
        """The four settings, for `train_state.pth`: a resumed run must mix as the run that wrote the file."""
        return {"mixup_alpha": self.mixup_alpha, "cutmix_alpha": self.cutmix_alpha, "prob": self.prob,
                "switch_prob": self.switch_prob}

    def getstate(self):
        return self._rng.getstate()

    def setstate(self, state):
        # (through torch.save / torch.load the tuples of random.getstate() may come back as lists)
        version, internal, gauss = state
        self._rng.setstate((int(version), tuple(int(v) for v in internal), gauss))

    def plan(self, n, h, w):
        """The draws of one batch of n images h x w, host only: None (no mixing) or a `MixPlan`.  Draw order: u =
        random() and nothing more when u >= prob; random() < switch_prob picks CutMix when both alphas are positive;
        lam = betavariate(alpha, alpha); for CutMix cx = randrange(w), cy = randrange(h), the box of half sizes
        int(r w), int(r h) with r = sqrt(1 - lam) / 2 around (cx, cy), clipped, and lam = 1 - box area / (h w).  The
        sequence does not depend on n."""
        rng = self._rng
        if rng.random() >= self.prob:
            return None
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            kind = CUTMIX if rng.random() < self.switch_prob else MIXUP
        else:
            kind = CUTMIX if self.cutmix_alpha > 0.0 else MIXUP
        alpha = self.cutmix_alpha if kind == CUTMIX else self.mixup_alpha
        lam = rng.betavariate(alpha, alpha)
        if kind == MIXUP:
            return MixPlan(kind, lam, f32(lam), f32(1.0 - lam), (0, 0, int(h), int(w)))
        cx, cy = rng.randrange(w), rng.randrange(h)
        r = 0.5 * math.sqrt(1.0 - lam)
        hw, hh = int(r * w), int(r * h)
        x1, y1, x2, y2 = max(cx - hw, 0), max(cy - hh, 0), min(cx + hw, w), min(cy + hh, h)
        lam = 1.0 - (x2 - x1) * (y2 - y1) / (h * w)
        return MixPlan(kind, lam, 0.0, 1.0, (y1, x1, y2, x2))

    def __call__(self, x, y):
        """x: a device batch (uint8 [N,H,W,C] or float32 [N,C,H,W]), y: its labels.  Returns (x_mixed, ya, yb, lam):
        a new tensor, ya = y, yb = y.roll(1), lam float32-rounded; without mixing (x, y, None, 1.0)."""
        from . import ops
        if x.dim() != 4:
            raise ValueError(f"BatchMix expects a 4-d image batch, got {tuple(x.shape)}")
        import torch
        n = x.shape[0]
        nhwc = x.dtype == torch.uint8
        h, w = (x.shape[1], x.shape[2]) if nhwc else (x.shape[2], x.shape[3])
        p = self.plan(n, h, w)
        if p is None:
            return x, y, None, 1.0
        if not nhwc:
            x = x.float()
        return ops.mix_batch(x.contiguous(), p.ca, p.cb, p.box, shift=1 if n > 1 else 0), y, y.roll(1), f32(p.lam)
