"""`sykepic train` with `class_weights = balanced`, `label_smoothing = 0.1` and `checkpoint_on = balanced_accuracy` on a
tiny imbalanced directory (12 / 6 / 3 images): the run finishes, prints the balanced-accuracy line, writes the weights
it trained with, and a `--resume` of it is the uninterrupted run."""

import random
from collections import namedtuple

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

INI = """[dataset]
path = {ds}
split = 0.5, 0.5
external_test =
min_N =
max_N =
exclude =
random_seed = 42
oversample_until =
oversample_with_decay =
[model]
path = {models}
network = resnet18
weights =
id = auto
exist_ok = no
head = 32
dropout =
[image]
shape = 3, 64, 64
augmentations = flip
imagenet_normalization = no
border = mode
zoom_range = 0.8, 1.2
brightness_range = 0.95, 1.1
max_rotation = 10
batch_size = 16
num_workers = 0
[train]
gpu = yes
max_epochs = {epochs}
early_stop_patience = 12
learning_rate = 0.01
optimizer = Adam
class_weights = balanced
label_smoothing = 0.1
checkpoint_on = balanced_accuracy
[lr_warmup]
use = no
[lr_reduction]
use = no
"""

COUNTS = {"blob": 12, "bars": 6, "flat": 3}


def _dataset(ds):
    rng = np.random.RandomState(0)
    for name, count in COUNTS.items():
        (ds / name).mkdir(parents=True)
        for i in range(count):
            h, w = rng.randint(30, 70), rng.randint(30, 90)
            img = np.full((h, w), 180, np.uint8)
            if name == "blob":
                img[h // 4: h // 2, w // 4: w // 2] = 40
            elif name == "bars":
                img[:, ::6] = 60
            img = np.clip(img.astype(np.int32) + rng.randint(-10, 10, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(ds / name / f"{name}_{i:02d}.png")


def _seed_all(v):
    random.seed(v)
    np.random.seed(v)
    torch.manual_seed(v)


def test_weighted_smoothed_run_and_its_resume(tmp_path, capsys):
    from sykepic_hip import loss, train
    A = namedtuple("A", "config collage dist save_images resume")
    ds = tmp_path / "ds"
    _dataset(ds)

    def ini(tag, epochs):
        f = tmp_path / f"{tag}.ini"
        f.write_text(INI.format(ds=ds, models=tmp_path / tag, epochs=epochs))
        return str(f)

    _seed_all(1234)
    train.main(A(ini("a", 2), None, None, None, None))
    out_a = capsys.readouterr().out
    dir_a, dir_b = tmp_path / "a" / "resnet18_1", tmp_path / "b" / "resnet18_1"
    assert "[ERROR]" not in out_a, out_a
    val_lines = [ln for ln in out_a.splitlines() if ln.startswith("[STAT] Val Acc")]
    assert len(val_lines) == 2 and all(", Val Balanced Acc: " in ln for ln in val_lines), val_lines
    assert "[INFO] Increased balanced accuracy, saving model state" in out_a
    for ln in val_lines:
        assert 0.0 <= float(ln.rsplit(": ", 1)[1]) <= 1.0
    # the train half of each class: round(12 / 2), round(6 / 2), round(3 / 2) = 6, 3, 2 images, N = 11, C = 3;
    # class ids are alphabetical
    want = {"bars": 11 / (3 * 3), "blob": 11 / (3 * 6), "flat": 11 / (3 * 2)}
    text = (dir_a / loss.CLASS_WEIGHTS_FILE).read_text()
    got = {ln.split()[0]: float(ln.split()[1]) for ln in text.splitlines()}
    assert got == want and [ln.split()[0] for ln in text.splitlines()] == ["bars", "blob", "flat"]
    end_a = torch.load(dir_a / train.TRAIN_STATE_FILE, weights_only=True)
    assert end_a["format"] == 1 and end_a["epoch"] == 2 and end_a["checkpoint_on"] == "balanced_accuracy"
    assert end_a["loss"] == {"label_smoothing": 0.1, "class_weights": [want["bars"], want["blob"], want["flat"]]}

    _seed_all(1234)
    train.main(A(ini("b", 1), None, None, None, None))
    _seed_all(777)                              # a new process would not stand where the old one stopped
    train.main(A(ini("b", 2), None, None, None, str(dir_b)))
    out_c = capsys.readouterr().out
    assert "[ERROR]" not in out_c and "[INFO] Resuming after epoch 1" in out_c, out_c
    assert [ln for ln in out_c.splitlines() if ln.startswith("[STAT] Val Acc")][-1] == val_lines[-1]
    end_c = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert end_c["epoch"] == 2 and end_a["book"] == end_c["book"]
    best_a, best_c = torch.load(dir_a / "best_state.pth"), torch.load(dir_b / "best_state.pth")
    assert list(best_a) == list(best_c) and [k for k in best_a if not torch.equal(best_a[k], best_c[k])] == []
    assert [k for k in end_a["net"] if not torch.equal(end_a["net"][k], end_c["net"][k])] == []
    # the same directory under another loss: refused in one line before any network is built
    f = tmp_path / "b.ini"
    f.write_text(f.read_text().replace("label_smoothing = 0.1", "label_smoothing = 0.2").replace("max_epochs = 2", "max_epochs = 3"))
    with pytest.raises(ValueError, match="cannot resume: loss differs"):
        train.main(A(str(f), None, None, None, str(dir_b)))
