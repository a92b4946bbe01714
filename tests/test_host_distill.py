"""Knowledge distillation, host side (no GPU): the three `[train]` keys and their error wording, what `train_state.pth`
records of a distilled run and how a resume is refused, the teacher-directory checks, and the float64 formula the kernel
implements against torch autograd."""

from configparser import ConfigParser

import pytest
import torch
import torch.nn.functional as F

from sykepic_hip import config, distill, train


def _config(**train_keys):
    cp = ConfigParser()
    cp.read_dict({"train": {k: str(v) for k, v in train_keys.items()}})
    return cp


def test_keys_defaults_and_error_wording():
    keys = config.KEYS["train"]
    assert keys["distill_from"][1] == "" and keys["distill_alpha"][1] == "0.5" and keys["distill_temperature"][1] == "2"
    tr = config.Settings(_config()).train
    assert tr.distill_from == "" and tr.distill_alpha == 0.5 and tr.distill_temperature == 2.0
    tr = config.Settings(_config(distill_from=" /models/resnet50_1 ", distill_alpha="0.25", distill_temperature="3.5")).train
    assert (tr.distill_from, tr.distill_alpha, tr.distill_temperature) == ("/models/resnet50_1", 0.25, 3.5)
    tr = config.Settings(_config(distill_alpha="", distill_temperature="")).train          # empty: the defaults
    assert (tr.distill_alpha, tr.distill_temperature) == (0.5, 2.0)
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match=r"distill_alpha must be between 0.0 and 1.0. Got: "):
            config.Settings(_config(distill_alpha=bad)).train.distill_alpha
    for bad in ("0", "-2", "inf", "nan"):
        with pytest.raises(ValueError, match=r"distill_temperature must be a finite number above 0.0. Got: "):
            config.Settings(_config(distill_temperature=bad)).train.distill_temperature
    # off: no object, whatever the other two keys say, and nothing is looked up on disk
    assert config.get_distiller(_config(distill_alpha="7"), ["a"], (3, 8, 8), "cuda:0") is None
    assert config.get_distill_info(_config(), ["a"], (3, 8, 8)) is None


def test_describe_same_and_show_settings():
    d = distill.describe("resnet50", "ab" * 32, 0.5, 2)
    assert d == {"teacher": "resnet50", "teacher_sha256": "ab" * 32, "alpha": 0.5, "temperature": 2.0}
    assert distill.same_settings(d, dict(d)) and distill.same_settings(None, None) and distill.same_settings(None, {})
    assert not distill.same_settings(d, None) and not distill.same_settings(None, d)
    for key, other in (("teacher", "resnet101"), ("teacher_sha256", "cd" * 32), ("alpha", 0.3), ("temperature", 4.0)):
        assert not distill.same_settings(d, {**d, key: other}), key
    assert distill.show_settings(None) == "off"
    assert distill.show_settings(d) == "teacher resnet50 (best_state.pth sha256 abababababab), alpha 0.5, temperature 2"
    with pytest.raises(ValueError, match="distill_alpha must be between 0.0 and 1.0. Got: 1.5"):
        distill.check_settings(1.5, 2.0)
    with pytest.raises(ValueError, match="distill_temperature must be a finite number above 0.0. Got: 0.0"):
        distill.check_settings(0.5, 0.0)


class _Teacher:
    """What `Distiller` touches of a `HipNet`, without a GPU."""
    num_classes, device, training = 3, "cpu", True

    class graph:
        network = "resnet50"

    def eval(self):
        self.training = False
        return self


def test_distiller_describes_its_teacher():
    t = _Teacher()
    assert distill.Distiller(_Teacher(), 0.25, 3.5).describe()["teacher_sha256"] == ""      # a teacher built in memory
    t.state_sha256 = "12" * 32                                                             # as `load_teacher` leaves it
    d = distill.Distiller(t, 0.25, 3.5)
    assert t.training is False
    assert d.describe() == distill.describe("resnet50", "12" * 32, 0.25, 3.5)
    with pytest.raises(ValueError, match="distill_alpha"):
        distill.Distiller(_Teacher(), -1.0, 2.0)
    with pytest.raises(ValueError, match="distill_temperature"):
        distill.Distiller(_Teacher(), 0.5, float("inf"))


def _state(**extra):
    return {"format": train.TRAIN_STATE_FORMAT, "network": "resnet18", "classes": ["a", "b"], "img_shape": [3, 8, 8],
            "optimizer": "Adam", "world": 1, **extra}


def test_check_train_state_messages():
    run = dict(network="resnet18", classes=["a", "b"], img_shape=(3, 8, 8), optimizer="Adam", world=1)
    d = distill.describe("resnet50", "ab" * 32, 0.5, 2.0)
    train.check_train_state(_state(), **run)                                  # a file without the key: written without
    train.check_train_state(_state(), **run, distill=None)
    train.check_train_state(_state(distill=d), **run, distill=dict(d))
    shown = "teacher resnet50 \\(best_state.pth sha256 abababababab\\), alpha 0.5, temperature 2"
    with pytest.raises(ValueError, match=f"cannot resume: distill differs, train_state.pth has {shown}, the config gives off") as e:
        train.check_train_state(_state(distill=d), **run)
    assert "\n" not in str(e.value)
    with pytest.raises(ValueError, match=f"cannot resume: distill differs, train_state.pth has off, the config gives {shown}"):
        train.check_train_state(_state(), **run, distill=d)
    for key, other, text in (("alpha", 0.3, "alpha 0.3, temperature 2"), ("temperature", 4.0, "alpha 0.5, temperature 4"),
                             ("teacher_sha256", "cd" * 32, "sha256 cdcdcdcdcdcd"), ("teacher", "resnet101", "teacher resnet101")):
        with pytest.raises(ValueError, match=f"cannot resume: distill differs, train_state.pth has {shown}, the config "
                                             f"gives .*{text}"):
            train.check_train_state(_state(distill=d), **run, distill={**d, key: other})


def _model_dir(tmp, classes, shape, network="resnet50"):
    tmp.mkdir(parents=True, exist_ok=True)
    (tmp / "class_names.txt").write_text("\n".join(classes) + "\n")
    (tmp / "config.ini").write_text(f"[image]\nshape = {', '.join(str(v) for v in shape)}\n[model]\nnetwork = {network}\n")
    (tmp / "best_state.pth").write_bytes(b"weights")
    return tmp


def test_teacher_directory_is_checked_without_a_gpu(tmp_path):
    import hashlib
    d = _model_dir(tmp_path / "t", ["a", "b", "c"], (3, 64, 64))
    info = distill.describe_dir(d, ["a", "b", "c"], (3, 64, 64), 0.5, 2.0)
    assert info == distill.describe("resnet50", hashlib.sha256(b"weights").hexdigest(), 0.5, 2.0)
    cp = _config(distill_from=str(d), distill_alpha="0.25")
    assert config.get_distill_info(cp, ["a", "b", "c"], (3, 64, 64)) == {**info, "alpha": 0.25}
    with pytest.raises(ValueError, match=r"distill_from: class list differs, the teacher in .* has 3 classes, the run has 2 "
                                         r"classes \(differing: c\)"):
        distill.check_teacher_dir(d, ["a", "b"], (3, 64, 64))
    with pytest.raises(ValueError, match=r"has 3 classes, the run has 3 classes \(differing: order\)"):
        distill.check_teacher_dir(d, ["b", "a", "c"], (3, 64, 64))
    with pytest.raises(ValueError, match=r"distill_from: image shape differs, the teacher in .* has \[3, 64, 64\], the run has "
                                         r"\[3, 32, 32\]"):
        distill.check_teacher_dir(d, ["a", "b", "c"], (3, 32, 32))
    with pytest.raises(ValueError, match=r"is not a model directory \(class_names.txt not found\)"):
        distill.check_teacher_dir(tmp_path / "nothing", ["a"], (3, 64, 64))
    with pytest.raises(ValueError, match="distill_alpha"):                   # a bad number: before the directory is read
        config.get_distill_info(_config(distill_from=str(tmp_path / "nothing"), distill_alpha="2"), ["a"], (3, 8, 8))


@pytest.mark.parametrize("T", [1.0, 2.0, 3.5])
@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_formula_against_autograd(T, alpha):
    """dz = (1 - alpha) g_hard + (alpha T / n) (softmax(z / T) - softmax(t / T)) and KD formed term by term as
    q (log q - log pT), in float64 against autograd of the torch expression; the underflow row gives 160."""
    g = torch.Generator().manual_seed(5)
    n, c = 7, 11
    z = (torch.randn(n, c, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    t = torch.randn(n, c, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, c, (n,), generator=g)
    w = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    hard = F.cross_entropy(z, y, weight=w, label_smoothing=0.1)
    kd = T * T * F.kl_div(F.log_softmax(z / T, 1), F.softmax(t / T, 1), reduction="batchmean")
    ((1 - alpha) * hard + alpha * kd).backward()
    zd = z.detach()
    zh = zd.clone().requires_grad_(True)
    F.cross_entropy(zh, y, weight=w, label_smoothing=0.1).backward()
    g_hard = zh.grad
    pT, q = F.softmax(zd / T, 1), F.softmax(t / T, 1)
    dz = (1 - alpha) * g_hard + (alpha * T / n) * (pT - q)
    assert float((dz - z.grad).abs().max()) < 1e-15
    lse_z, lse_t = torch.logsumexp(zd / T, 1, keepdim=True), torch.logsumexp(t / T, 1, keepdim=True)
    rows = (q * ((t / T - lse_t) - (zd / T - lse_z))).sum(1)
    assert abs(float(T * T / n * rows.sum()) - float(kd.detach())) < 1e-13
    zu, tu = torch.tensor([[80.0, -80.0, 0.0]], dtype=torch.float64), torch.tensor([[-90.0, 90.0, 0.0]], dtype=torch.float64)
    qu = F.softmax(tu, 1)
    row = (qu * ((tu - torch.logsumexp(tu, 1, keepdim=True)) - (zu - torch.logsumexp(zu, 1, keepdim=True)))).sum()
    assert abs(float(row) - 160.0) < 1e-9
