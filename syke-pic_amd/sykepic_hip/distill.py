"""Knowledge distillation during training (Hinton, Vinyals, Dean: "Distilling the Knowledge in a Neural Network", 2015;
not in sykefi/syke-pic): a small network learns from the logits of a trained large one.

The teacher is a model directory as `sykepic train` leaves it.  It is loaded into a second `HipNet` in eval mode, on
the student's device, and sees exactly the tensor the student's step gets - behind the GPU augmentations, the train
pipeline's normalisation and Mixup / CutMix.  Its logits go into one reused buffer, and the student's step runs the
distillation criterion in its loss kernel (csrc/head.hip `ce_loss_kernel<.., KD>`):

    L = (1 - alpha) L_hard + alpha T^2 KL(softmax(teacher / T) || softmax(student / T))          ("batchmean")

with L_hard the loss the step computes without a teacher (class weights, smoothing, the two-label criterion of a mixed
batch).  Validation and test stay on the hard loss.
"""

import math
from configparser import ConfigParser
from pathlib import Path

import torch


def check_settings(alpha, temperature):
    """The house wording for the two numbers, wherever they come from."""
    alpha, temperature = float(alpha), float(temperature)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"distill_alpha must be between 0.0 and 1.0. Got: {alpha}")
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"distill_temperature must be a finite number above 0.0. Got: {temperature}")
    return alpha, temperature


def describe(network, state_sha256, alpha, temperature):
    """What `train_state.pth` records of a distilled run (`Distiller.describe`)."""
    return {"teacher": str(network), "teacher_sha256": str(state_sha256), "alpha": float(alpha),
            "temperature": float(temperature)}


def same_settings(a, b):
    """Two `describe` dicts (None: no distillation) name the same teacher, weight and temperature."""
    if not a or not b:
        return not a and not b
    return (str(a.get("teacher")) == str(b.get("teacher")) and str(a.get("teacher_sha256")) == str(b.get("teacher_sha256"))
            and float(a.get("alpha", -1.0)) == float(b.get("alpha", -1.0))
            and float(a.get("temperature", -1.0)) == float(b.get("temperature", -1.0)))


def show_settings(d):
    if not d:
        return "off"
    return (f"teacher {d.get('teacher')} (best_state.pth sha256 {str(d.get('teacher_sha256'))[:12]}), "
            f"alpha {float(d.get('alpha', 0.0)):g}, temperature {float(d.get('temperature', 0.0)):g}")


class Distiller:
    """``Distiller(teacher_net, alpha, temperature)``: holds the teacher, a `HipNet` with its weights loaded, in eval
    mode, and the two numbers of the criterion.  The teacher's `state_sha256` - the digest of the `best_state.pth` it
    was loaded from, set by `load_teacher` - goes into `describe()`; "" for a teacher built in memory."""

    def __init__(self, teacher_net, alpha, temperature):
        self.alpha, self.temperature = check_settings(alpha, temperature)
        self.teacher = teacher_net.eval()
        self.state_sha256 = str(getattr(teacher_net, "state_sha256", ""))
        self._buf = None

    def logits(self, x):
        """The teacher's logits of the device batch `x` (what the student's step is about to get), float32 [n, classes]
        in a buffer that the next call of the same batch size overwrites.  Asynchronous on the current stream."""
        n = int(x.shape[0])
        if self._buf is None or self._buf.shape[0] != n:
            self._buf = torch.empty((n, self.teacher.num_classes), dtype=torch.float32, device=self.teacher.device)
        if self.teacher.training:
            self.teacher.eval()
        return self.teacher.forward(x, out=self._buf)

    def describe(self):
        return describe(self.teacher.graph.network, self.state_sha256, self.alpha, self.temperature)


def check_teacher_dir(model_dir, classes, img_shape):
    """The teacher must classify the run's classes, in the run's order, on the run's image shape: a ValueError naming
    both sides otherwise.  Reads `class_names.txt` and `config.ini` only (no GPU).  Returns the teacher's config."""
    from .config import get_img_shape
    model_dir = Path(model_dir)
    for name in ("class_names.txt", "config.ini", "best_state.pth"):
        if not (model_dir / name).is_file():
            raise ValueError(f"distill_from: {model_dir} is not a model directory ({name} not found)")
    theirs = (model_dir / "class_names.txt").read_text().splitlines()
    ours = [str(c) for c in classes]
    if theirs != ours:
        diff = sorted(set(theirs) ^ set(ours))
        raise ValueError(f"distill_from: class list differs, the teacher in {model_dir} has {len(theirs)} classes, the run "
                         f"has {len(ours)} classes (differing: {', '.join(diff[:5]) or 'order'})")
    config = ConfigParser()
    config.read(model_dir / "config.ini")
    shape = [int(v) for v in get_img_shape(config)]
    if shape != [int(v) for v in img_shape]:
        raise ValueError(f"distill_from: image shape differs, the teacher in {model_dir} has {shape}, the run has "
                         f"{[int(v) for v in img_shape]}")
    return config


def describe_dir(model_dir, classes, img_shape, alpha, temperature):
    """`Distiller.describe()` of the teacher in `model_dir` without building it (no GPU): for the resume check, which
    comes before any network exists.  Validates the directory as `load_teacher` does."""
    from . import prob
    from .config import Settings
    alpha, temperature = check_settings(alpha, temperature)
    config = check_teacher_dir(model_dir, classes, img_shape)
    return describe(Settings(config).model.network, prob.state_digest(model_dir), alpha, temperature)


def load_teacher(model_dir, classes, img_shape, device):
    """The `HipNet` of a model directory, built as `prob.prepare_model` builds it, for teaching: the calibrated
    single-pass mode when the directory carries activation means of its own weights (`prob.use_act_means`), else the
    default eval mode.  Auto-calibration is never armed: nothing is written into the teacher's directory, and its logits
    do not depend on which batch came first.  The net carries the sha256 of the `best_state.pth` it was loaded from as
    `state_sha256`, for `Distiller.describe`."""
    from . import prob
    from .config import get_network
    model_dir = Path(model_dir)
    config = check_teacher_dir(model_dir, classes, img_shape)
    device = torch.device(device)
    net = get_network(config, len(classes), device=device, pretrained_ok=False)
    net.load_state_dict(torch.load(model_dir / "best_state.pth", map_location="cpu"))
    prob.use_act_means(net, model_dir)
    net.eval()
    net.state_sha256 = prob.state_digest(model_dir)
    return net
