"""The loss of `sykepic train`: ``nn.CrossEntropyLoss(weight, label_smoothing)`` as a description.

The reference constructs ``nn.CrossEntropyLoss()`` (``sykepic/train/train.py:127``) and hands it to ``train_net``; here
the loss is fused into the training and validation steps of libsykepic_hip.so (``csrc/head.hip``), so what travels is
its two options.  ``CrossEntropyLoss`` below holds them; ``from_loss_fn`` reads them off a ``torch.nn.CrossEntropyLoss``
as well, and ``train_net`` passes them to ``HipNet.set_loss``.  The ``[train]`` keys ``label_smoothing`` and
``class_weights`` (``none`` / ``balanced`` / a file of ``name weight`` lines) are resolved here too.
"""

import math
from collections import Counter
from pathlib import Path

CLASS_WEIGHTS_FILE = "class_weights.txt"


class CrossEntropyLoss:
    """``weight``: one positive number per class (None: all ones); ``label_smoothing`` in [0, 1]; the mean reduction."""

    reduction = "mean"

    def __init__(self, weight=None, label_smoothing=0.0):
        if weight is not None:
            weight = [float(v) for v in (weight.tolist() if hasattr(weight, "tolist") else weight)]
            for i, v in enumerate(weight):
                if not math.isfinite(v) or not v > 0:
                    raise ValueError(f"class weight {i} is {v}: every weight must be a finite number above 0")
        label_smoothing = float(label_smoothing)
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
        self.weight, self.label_smoothing = weight, label_smoothing

    @property
    def is_default(self):
        return self.weight is None and self.label_smoothing == 0.0

    def describe(self):
        """What `train_state.pth` keeps of the loss: plain numbers (`weights_only=True` loads them)."""
        return {"label_smoothing": self.label_smoothing, "class_weights": self.weight}

    def __repr__(self):
        w = "None" if self.weight is None else f"[{len(self.weight)} classes]"
        return f"CrossEntropyLoss(weight={w}, label_smoothing={self.label_smoothing})"


def from_loss_fn(loss_fn):
    """None (the defaults), a `CrossEntropyLoss` of this module or a `torch.nn.CrossEntropyLoss` -> `CrossEntropyLoss`.
    Anything the fused kernel does not compute is refused: another reduction, an `ignore_index` that is not torch's
    default, another kind of object."""
    if loss_fn is None:
        return CrossEntropyLoss()
    if isinstance(loss_fn, CrossEntropyLoss):
        return loss_fn
    if not (hasattr(loss_fn, "label_smoothing") and hasattr(loss_fn, "weight") and hasattr(loss_fn, "reduction")):
        raise TypeError(f"loss_fn must be None or a CrossEntropyLoss (this module's or torch.nn's), got {type(loss_fn).__name__}")
    if loss_fn.reduction != "mean":
        raise ValueError(f"the fused loss computes reduction='mean' only, loss_fn has reduction={loss_fn.reduction!r}")
    if getattr(loss_fn, "ignore_index", -100) != -100:
        raise ValueError("the fused loss has no ignore_index")
    return CrossEntropyLoss(loss_fn.weight, loss_fn.label_smoothing)


def same_loss(a, b):
    """Two `describe()` dictionaries (None / a missing key: the defaults) name the same loss."""
    a, b = a or {}, b or {}
    wa, wb = a.get("class_weights"), b.get("class_weights")
    return (float(a.get("label_smoothing") or 0.0) == float(b.get("label_smoothing") or 0.0)
            and (None if wa is None else [float(v) for v in wa]) == (None if wb is None else [float(v) for v in wb]))


def balanced_weights(labels, num_classes):
    """w_c = N / (C n_c) over the label ids the train loader iterates (after oversampling): sklearn's "balanced" rule.
    Every class weighs the same in sum_i w[y_i], and the weights of a balanced set are all 1."""
    counts = Counter(int(v) for v in labels)
    missing = [c for c in range(num_classes) if not counts.get(c)]
    if missing:
        raise ValueError(f"class_weights = balanced: no training image of class id {missing[0]}")
    total = sum(counts.values())
    return [total / (num_classes * counts[c]) for c in range(num_classes)]


def read_weight_file(path, classes):
    """`name weight` per line, as the reference's threshold files (`sykepic/compute/prediction.py`): one line for
    every class of `classes`, in any order; blank lines are skipped.  Returns the weights in class-id order."""
    classes = [str(c) for c in classes]
    ids = {c: i for i, c in enumerate(classes)}
    out = {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            if not line.strip():
                continue
            parts = line.split()
            if len(parts) != 2:
                raise ValueError(f"{path}:{no}: expected `name weight`, got {line.strip()!r}")
            name, text = parts
            if name not in ids:
                raise ValueError(f"{path}:{no}: {name!r} is not a class of this dataset")
            if name in out:
                raise ValueError(f"{path}:{no}: class {name!r} listed twice")
            try:
                value = float(text)
            except ValueError:
                raise ValueError(f"{path}:{no}: {text!r} is not a number") from None
            if not math.isfinite(value) or not value > 0:
                raise ValueError(f"{path}:{no}: the weight of {name!r} must be a finite number above 0, got {text}")
            out[name] = value
    missing = [c for c in classes if c not in out]
    if missing:
        raise ValueError(f"{path}: no weight for class {missing[0]!r}" +
                         (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    return [out[c] for c in classes]


def write_weight_file(model_dir, classes, weights):
    """The weights a run trained with, in the format `read_weight_file` reads (`repr`: they read back exactly)."""
    path = Path(model_dir) / CLASS_WEIGHTS_FILE
    path.write_text("".join(f"{c} {float(w)!r}\n" for c, w in zip(classes, weights)))
    return path


def resolve_class_weights(spec, classes, train_labels):
    """`[train] class_weights`: `none` -> None, `balanced` -> `balanced_weights`, anything else is a file path."""
    if spec is None or spec.strip().lower() in ("", "none"):
        return None
    if spec.strip().lower() == "balanced":
        return balanced_weights(train_labels, len(classes))
    return read_weight_file(spec.strip(), classes)


def balanced_accuracy(counts):
    """Mean per-class recall from [(rows seen, rows correct)] per class, over the classes that were seen."""
    recalls = [float(ok) / float(seen) for seen, ok in counts if seen > 0]
    return sum(recalls) / len(recalls) if recalls else 0.0
