"""``train.ini`` / model-dir ``config.ini``: one declarative table of every key the hot path reads.

The drop-in contract is the FILE FORMAT of the reference (``sykepic/train/config.py:20-77`` and the ini block of
``sykepic/train/train.py:17-125``): section and key names, value syntax, which keys may be absent.  Here that
contract is data - ``KEYS[section][key] = (parser, default)`` - and ``Settings(config).section.key`` parses a value
when it is first asked for, so a key that the chosen options never reach (``max_rotation`` without ``rotate``,
``[lr_warmup]`` factors with ``use = no``) may be missing, exactly as with the reference's statement-by-statement
reads; a missing REQUIRED key raises configparser's own ``NoOptionError`` / ``NoSectionError``.
"""

from configparser import NoOptionError, RawConfigParser
from pathlib import Path

from . import preprocess as P

REQUIRED = object()


def _csv(item):
    return lambda s: tuple(item(v) for v in s.split(","))


def _optional(item):
    return lambda s: item(s) if s else None


def _names(s):
    return [v.strip() for v in s.split(",")]


def _flag(s):
    try:
        return RawConfigParser.BOOLEAN_STATES[s.lower()]
    except KeyError:
        raise ValueError(f"Not a boolean: {s}") from None


def _smoothing(s):
    v = float(s) if s.strip() else 0.0
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {v}")
    return v


def _class_weights(s):
    """``none`` / ``balanced`` (lower-cased) or the path of a file of ``name weight`` lines (loss.read_weight_file)."""
    v = s.strip()
    return (v.lower() or "none") if v.lower() in ("", "none", "balanced") else v


def _checkpoint_on(s):
    v = s.strip().lower() or "accuracy"
    if v not in ("accuracy", "balanced_accuracy"):
        raise ValueError(f"checkpoint_on must be accuracy or balanced_accuracy. Got: {s}")
    return v


def _alpha(key):
    """``mixup_alpha`` / ``cutmix_alpha``: the Beta(alpha, alpha) parameter of the mix, 0 (or empty) = off."""
    def parse(s):
        v = float(s) if s.strip() else 0.0
        if not (v >= 0.0 and v != float("inf")):
            raise ValueError(f"{key} must be a finite number >= 0.0. Got: {v}")
        return v
    return parse


def _probability(key, default):
    def parse(s):
        v = float(s) if s.strip() else default
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"{key} must be between 0.0 and 1.0. Got: {v}")
        return v
    return parse


def get_batch_mix(config, seed=0):
    """The `mix.BatchMix` of ``[train] mixup_alpha / cutmix_alpha / mix_prob / mix_switch_prob``, or None when both
    alphas are 0 (the default): no object, no draw, the training step of a run without the keys."""
    tr = Settings(config).train
    if tr.mixup_alpha == 0.0 and tr.cutmix_alpha == 0.0:
        return None
    from .mix import BatchMix
    return BatchMix(tr.mixup_alpha, tr.cutmix_alpha, tr.mix_prob, tr.mix_switch_prob, seed=seed)


def _ema_decay(s):
    """``ema_decay``: the decay of the weights' moving average (ema.py), 0 (or empty) = off."""
    v = float(s) if s.strip() else 0.0
    if not 0.0 <= v < 1.0:
        raise ValueError(f"ema_decay must be at least 0.0 and below 1.0. Got: {v}")
    return v


def get_model_ema(config, net):
    """The `ema.ModelEma` of ``[train] ema_decay / ema_warmup`` over `net`, or None when the decay is 0 (the default):
    no object, no second buffer, no launch - the run of a file without the keys."""
    tr = Settings(config).train
    if tr.ema_decay == 0.0:
        return None
    from .ema import ModelEma
    return ModelEma(net, tr.ema_decay, tr.ema_warmup)


def _distill_alpha(s):
    """``distill_alpha``: the weight of the distillation term (distill.py); read only with ``distill_from`` set."""
    v = float(s) if s.strip() else 0.5
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"distill_alpha must be between 0.0 and 1.0. Got: {v}")
    return v


def _distill_temperature(s):
    v = float(s) if s.strip() else 2.0
    if not (v > 0.0 and v != float("inf")):
        raise ValueError(f"distill_temperature must be a finite number above 0.0. Got: {v}")
    return v


def get_distill_info(config, classes, img_shape):
    """`Distiller.describe()` of those keys without building the teacher (no GPU), or None when off: what a resumed run
    is checked against before any network exists.  Raises what `get_distiller` would raise for the directory."""
    tr = Settings(config).train
    if not tr.distill_from:
        return None
    from .distill import describe_dir
    return describe_dir(tr.distill_from, classes, img_shape, tr.distill_alpha, tr.distill_temperature)


def get_distiller(config, classes, img_shape, device):
    """The `distill.Distiller` of ``[train] distill_from / distill_alpha / distill_temperature``, or None when
    ``distill_from`` is empty (the default): no teacher, no second handle - the run of a file without the keys.  A teacher
    with other classes or another image shape is a ValueError here, before any training."""
    tr = Settings(config).train
    if not tr.distill_from:
        return None
    from .distill import Distiller, load_teacher
    alpha, temperature = tr.distill_alpha, tr.distill_temperature     # (a bad number: before the teacher is built)
    return Distiller(load_teacher(tr.distill_from, classes, img_shape, device), alpha, temperature)


def _test_tta(s):
    """``test_tta``: the test-time augmentation mode (tta.py) of a second report per test set, empty = none."""
    from .tta import MODES
    v = s.strip().lower() or "none"
    if v not in MODES:
        raise ValueError(f"test_tta must be one of {', '.join(MODES)}. Got: {s}")
    return v


def _index_prob_pairs(s):
    """``dropout = 1,0.5;2,0.3`` -> [(1, 0.5), (2, 0.3)] (list index in the head, probability)."""
    return [(int(i), float(p)) for i, p in (pair.split(",") for pair in s.split(";"))] if s else []


KEYS = {
    "dataset": {
        "path": (Path, REQUIRED), "split": (_csv(float), REQUIRED), "min_N": (_optional(int), REQUIRED),
        "max_N": (_optional(int), REQUIRED), "exclude": (_names, REQUIRED), "random_seed": (int, REQUIRED),
        "oversample_until": (_optional(int), ""), "oversample_with_decay": (_optional(float), ""),
        "external_test": (str, ""),
    },
    "image": {
        "shape": (_csv(int), REQUIRED), "batch_size": (int, REQUIRED), "num_workers": (int, REQUIRED),
        "augmentations": (_names, REQUIRED), "border": (str, REQUIRED), "max_rotation": (int, REQUIRED),
        "zoom_range": (_csv(float), REQUIRED), "brightness_range": (_csv(float), REQUIRED),
        "imagenet_normalization": (_flag, REQUIRED),
    },
    "model": {
        "network": (str, REQUIRED), "id": (str, REQUIRED), "path": (Path, REQUIRED), "exist_ok": (_flag, REQUIRED),
        # legacy model directories have no `weights` key (quirk Q7): "DEFAULT", and nothing is downloaded here
        "weights": (lambda s: s or None, "DEFAULT"),
        "head": (_csv(int), REQUIRED), "dropout": (_index_prob_pairs, REQUIRED),
    },
    "train": {
        "gpu": (_flag, REQUIRED), "max_epochs": (int, REQUIRED), "early_stop_patience": (int, REQUIRED),
        "learning_rate": (float, REQUIRED), "optimizer": (str, REQUIRED),
        # not in the reference: train_state.pth, written at the end of every epoch for `sykepic train --resume`
        "save_train_state": (_flag, "yes"),
        # not in the reference either (its loss is nn.CrossEntropyLoss() with the defaults): the options of the fused
        # loss (loss.py) and which validation figure selects best_state.pth; the defaults are the reference's behaviour
        "label_smoothing": (_smoothing, "0"), "class_weights": (_class_weights, "none"),
        "checkpoint_on": (_checkpoint_on, "accuracy"),
        # Mixup / CutMix of every training batch on the GPU (mix.py); both alphas 0: off, the run of a file without the keys
        "mixup_alpha": (_alpha("mixup_alpha"), "0"), "cutmix_alpha": (_alpha("cutmix_alpha"), "0"),
        "mix_prob": (_probability("mix_prob", 1.0), "1"), "mix_switch_prob": (_probability("mix_switch_prob", 0.5), "0.5"),
        # exponential moving average of the weights (ema.py): validated, checkpointed and shipped as best_state.pth while the
        # raw weights keep training; decay 0: off, the run of a file without the keys
        "ema_decay": (_ema_decay, "0"), "ema_warmup": (_flag, "yes"),
        # test-time augmentation (tta.py) of the test split(s): a second report, test_report*_tta.txt, beside the plain one;
        # none: the run of a file without the key
        "test_tta": (_test_tta, "none"),
        # knowledge distillation from a trained model directory (distill.py): the training loss becomes (1 - alpha) * hard +
        # alpha * T^2 * KL(teacher || student); empty distill_from: off, the run of a file without the keys
        "distill_from": (lambda s: s.strip(), ""), "distill_alpha": (_distill_alpha, "0.5"),
        "distill_temperature": (_distill_temperature, "2"),
    },
    "lr_warmup": {
        "use": (_flag, REQUIRED), "factor_1": (float, REQUIRED), "factor_2": (float, REQUIRED), "step_1": (int, REQUIRED),
        "step_2": (int, REQUIRED), "step_3": (int, REQUIRED), "verbose": (_flag, REQUIRED),
    },
    "lr_reduction": {
        "use": (_flag, REQUIRED), "factor": (float, REQUIRED), "patience": (int, REQUIRED), "verbose": (_flag, REQUIRED),
    },
}


class _Section:
    def __init__(self, config, name):
        self._config, self._name = config, name

    def __getattr__(self, key):
        try:
            parser, default = KEYS[self._name][key]
        except KeyError:
            raise AttributeError(f"[{self._name}] has no key {key!r} in the settings table") from None
        if default is REQUIRED:
            raw = self._config.get(self._name, key)
        else:
            try:
                raw = self._config.get(self._name, key)
            except NoOptionError:
                raw = default
        return parser(raw)


class Settings:
    """``Settings(config).image.batch_size`` -> parsed value of ``[image] batch_size`` (see KEYS)."""

    def __init__(self, config):
        for name in KEYS:
            setattr(self, name, _Section(config, name))


# augmentation name in `[image] augmentations` -> the transforms it adds to the TRAIN pipeline (in this order)
AUGMENTATIONS = {
    "flip": lambda im: [P.FlipHorizontal(), P.FlipVertical()],
    "translate": lambda im: [P.Translate()],
    "rotate": lambda im: [P.Rotate(im.max_rotation)],
    "zoom": lambda im: [P.Zoom(im.zoom_range)],
    "brightness": lambda im: [P.ChangeBrightness(im.brightness_range)],
}


def get_img_shape(config):
    return Settings(config).image.shape


def get_transforms(config, img_shape):
    """(train, eval) ``Compose`` pipelines (reference config.py:25-60).  Unknown augmentation names are ignored and,
    as in the reference, only the TRAIN pipeline gets the ImageNet normalisation (:55-56)."""
    im = Settings(config).image
    extra = [t for name in im.augmentations for t in AUGMENTATIONS.get(name, lambda _: [])(im)]
    tail = [P.Normalize(P.IMAGENET_MEAN, P.IMAGENET_STD)] if im.imagenet_normalization else []
    size, border = img_shape[1:], im.border
    return (P.Compose([P.Resize()] + extra + [P.ToTensor()] + tail, size, border),
            P.Compose([P.Resize(), P.ToTensor()], size, border))


def get_network(config, num_classes, device=None, pretrained_ok=True):
    """The only constructor call site of the network (reference config.py:63-77).
    Returns the MI355X-native ``HipNet``; raises if no GPU / library."""
    from .net import HipNet
    mo = Settings(config).model
    # pretrained_ok=False: the caller loads a checkpoint next (prob.prepare_model) - skip the random initialisation
    return HipNet(mo.network, num_classes, mo.weights, list(mo.head), mo.dropout, device=device, init=pretrained_ok)
