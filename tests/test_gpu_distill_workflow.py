"""`sykepic train` with `[train] distill_from`: the workflow of tests/test_gpu_resume.py (its dataset, ini template and
helpers).  A ResNet-34 teacher is trained for one epoch; ResNet-18 students then learn from its directory.  The run ends
and prints its `[STAT] Distill` line, `train_state.pth` records the teacher and the two numbers, a resumed run is the
uninterrupted run, other settings refuse to resume, a teacher of other classes or another image shape is refused before
the first step, and a config without the keys leaves no trace of any of it."""

import contextlib
import io
import re
import shutil
from collections import namedtuple

import pytest
import torch

import test_gpu_resume as R

pytestmark = pytest.mark.gpu

Args = namedtuple("Args", "config collage dist save_images resume")
KEYS = "optimizer = Adam\ndistill_from = {teacher}\ndistill_alpha = {alpha}\ndistill_temperature = {temperature}\n"
DISTILL_INI = R.INI.replace("optimizer = Adam\n", KEYS)
assert DISTILL_INI != R.INI


def _ini(tmp, ds, tag, epochs, teacher=None, alpha="0.5", temperature="2", network="resnet18", shape=None):
    f = tmp / f"{tag}.ini"
    text = (DISTILL_INI if teacher is not None else R.INI).format(
        ds=ds, models=tmp / tag, epochs=epochs, steps=(1, 2, 3), dropout="", teacher=teacher, alpha=alpha,
        temperature=temperature)
    text = text.replace("network = resnet18\n", f"network = {network}\n")
    if shape is not None:
        text = text.replace("shape = 3, 64, 64\n", f"shape = {shape}\n")
    f.write_text(text)
    return str(f)


def _main(ini, resume=None, seed=1234):
    """`train.main` in this process (one tuner table for every run of the module); returns what it printed."""
    from sykepic_hip import train
    R._seed_all(seed)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        train.main(Args(ini, None, None, None, resume))
    return out.getvalue()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """T: the teacher, ResNet-34, one epoch.  A: a ResNet-18 student of T, two epochs.  B: the same stopped after one
    epoch; C: `--resume` of B up to two, from other generator seeds.  F: one epoch without the keys."""
    from sykepic_hip import train
    tmp = tmp_path_factory.mktemp("distill")
    ds = tmp / "ds"
    R._dataset(ds)
    out = {"tmp": tmp, "ds": ds}
    out["t"] = _main(_ini(tmp, ds, "t", 1, network="resnet34"))
    teacher = tmp / "t" / "resnet34_1"
    out["teacher"] = teacher
    out["teacher_files"] = {p.name: p.read_bytes() for p in sorted(teacher.iterdir()) if p.is_file()}
    out["a"] = _main(_ini(tmp, ds, "a", 2, teacher=teacher))
    out["b"] = _main(_ini(tmp, ds, "b", 1, teacher=teacher))
    dir_b = tmp / "b" / "resnet18_1"
    out["mid"] = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    out["c"] = _main(_ini(tmp, ds, "b", 2, teacher=teacher), resume=str(dir_b), seed=777)
    out["f"] = _main(_ini(tmp, ds, "f", 1))
    out["dirs"] = {t: tmp / t / "resnet18_1" for t in "abf"}
    return out


def _distill_lines(out):
    return [ln for ln in out.splitlines() if ln.startswith("[STAT] Distill")]


def test_the_run_ends_and_reports(runs):
    from sykepic_hip import prob, train
    for tag in "tabc":
        assert "[ERROR]" not in runs[tag], runs[tag][-3000:]
    assert _distill_lines(runs["t"]) == []
    lines = _distill_lines(runs["a"])
    assert len(lines) == 2
    for ln in lines:
        m = re.fullmatch(r"\[STAT\] Distill Loss: (\d+\.\d{3}), Teacher Agreement: ([01]\.\d{3})", ln)
        assert m, ln
        assert float(m.group(1)) >= 0.0 and 0.0 <= float(m.group(2)) <= 1.0
    stats = R._stat_lines(runs["a"])
    assert sorted(stats) == [1, 2]
    for e in stats:                      # Train, Distill, Val - in that order
        assert [ln.split(":")[0] for ln in stats[e]] == ["[STAT] Train Acc", "[STAT] Distill Loss", "[STAT] Val Acc"]
    st = torch.load(runs["dirs"]["a"] / train.TRAIN_STATE_FILE, weights_only=True)
    assert st["distill"] == {"teacher": "resnet34", "teacher_sha256": prob.state_digest(runs["teacher"]), "alpha": 0.5,
                             "temperature": 2.0}
    assert st["network"] == "resnet18" and st["epoch"] == 2
    assert (runs["dirs"]["a"] / "best_state.pth").is_file()
    # nothing was written into the teacher's directory, nothing in it changed
    teacher = runs["teacher"]
    assert {p.name: p.read_bytes() for p in sorted(teacher.iterdir()) if p.is_file()} == runs["teacher_files"]


def test_resume_is_the_uninterrupted_run(runs):
    from sykepic_hip import train
    sa, sb, sc = R._stat_lines(runs["a"]), R._stat_lines(runs["b"]), R._stat_lines(runs["c"])
    assert sorted(sa) == [1, 2] and sorted(sb) == [1] and sorted(sc) == [2]
    assert sb[1] == sa[1]
    assert sc[2] == sa[2], (sc[2], sa[2])
    dir_a, dir_b = runs["dirs"]["a"], runs["dirs"]["b"]
    end_a = torch.load(dir_a / train.TRAIN_STATE_FILE, weights_only=True)
    end_c = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    mid = runs["mid"]
    assert mid["epoch"] == 1 and end_a["epoch"] == end_c["epoch"] == 2
    assert mid["distill"] == end_a["distill"] == end_c["distill"]
    assert R._differing(end_a["net"], end_c["net"]) == []
    assert R._differing(torch.load(dir_a / "best_state.pth"), torch.load(dir_b / "best_state.pth")) == []
    assert end_a["book"] == end_c["book"]


def test_a_config_without_the_keys_leaves_no_trace(runs):
    from sykepic_hip import train
    assert "[ERROR]" not in runs["f"] and "Distill" not in runs["f"] and "Teacher" not in runs["f"]
    st = torch.load(runs["dirs"]["f"] / train.TRAIN_STATE_FILE, weights_only=True)
    assert "distill" not in st and all("distill" not in r for r in st["ranks"])
    stats = R._stat_lines(runs["f"])
    assert [ln.split(":")[0] for ln in stats[1]] == ["[STAT] Train Acc", "[STAT] Val Acc"]
    # the teacher changes the training: the students' first epoch is not the plain run's
    assert R._stat_lines(runs["a"])[1][0] != stats[1][0]


def test_other_settings_refuse_to_resume(runs, monkeypatch):
    from sykepic_hip import train
    tmp, ds, teacher, dir_b = runs["tmp"], runs["ds"], runs["teacher"], runs["dirs"]["b"]

    def no_network(*a, **k):
        raise AssertionError("a network was built before the refusal")
    monkeypatch.setattr(train, "get_network", no_network)
    monkeypatch.setattr(train, "get_distiller", no_network)
    before = (dir_b / train.TRAIN_STATE_FILE).read_bytes()
    has = r"cannot resume: distill differs, train_state.pth has teacher resnet34 \(best_state.pth sha256 [0-9a-f]{12}\), " \
          r"alpha 0.5, temperature 2, the config gives "
    with pytest.raises(ValueError, match=has + r"teacher resnet34 \(best_state.pth sha256 [0-9a-f]{12}\), alpha 0.25, "
                                               r"temperature 2") as e:
        _main(_ini(tmp, ds, "b", 3, teacher=teacher, alpha="0.25"), resume=str(dir_b))
    assert "\n" not in str(e.value)
    with pytest.raises(ValueError, match=has + r"teacher resnet34 .*, alpha 0.5, temperature 4"):
        _main(_ini(tmp, ds, "b", 3, teacher=teacher, temperature="4"), resume=str(dir_b))
    with pytest.raises(ValueError, match=has + "off"):
        _main(_ini(tmp, ds, "b", 3), resume=str(dir_b))
    # another teacher: the same directory with other weights in it
    other = tmp / "other_teacher"
    if not other.exists():
        shutil.copytree(teacher, other)
        sd = torch.load(other / "best_state.pth")
        key = next(k for k, v in sd.items() if v.dtype == torch.float32)
        sd[key] = sd[key] + 1.0
        torch.save(sd, other / "best_state.pth")
    with pytest.raises(ValueError, match=has + r"teacher resnet34 \(best_state.pth sha256 [0-9a-f]{12}\), alpha 0.5, "
                                               r"temperature 2") as e:
        _main(_ini(tmp, ds, "b", 3, teacher=other), resume=str(dir_b))
    shown = re.findall(r"sha256 ([0-9a-f]{12})", str(e.value))
    assert len(shown) == 2 and shown[0] != shown[1]
    with pytest.raises(ValueError, match=r"cannot resume: distill differs, train_state.pth has off, the config gives teacher"):
        _main(_ini(tmp, ds, "f", 3, teacher=teacher), resume=str(runs["dirs"]["f"]))
    assert (dir_b / train.TRAIN_STATE_FILE).read_bytes() == before


def test_a_teacher_of_other_classes_or_shape_is_refused_before_the_first_step(runs, monkeypatch):
    from sykepic_hip import train
    tmp, ds, teacher = runs["tmp"], runs["ds"], runs["teacher"]

    def no_network(*a, **k):
        raise AssertionError("a network was built before the refusal")
    monkeypatch.setattr(train, "get_network", no_network)
    monkeypatch.setattr(train, "get_distiller", no_network)
    with pytest.raises(ValueError, match=r"distill_from: image shape differs, the teacher in .*resnet34_1 has \[3, 64, 64\], "
                                         r"the run has \[3, 32, 32\]"):
        _main(_ini(tmp, ds, "g", 1, teacher=teacher, shape="3, 32, 32"))
    fewer = tmp / "fewer_classes"
    if not fewer.exists():
        shutil.copytree(teacher, fewer)
        (fewer / "class_names.txt").write_text("bars\nblob\n")
    with pytest.raises(ValueError, match=r"distill_from: class list differs, the teacher in .*fewer_classes has 2 classes, "
                                         r"the run has 3 classes \(differing: flat\)"):
        _main(_ini(tmp, ds, "h", 1, teacher=fewer))
    reordered = tmp / "reordered_classes"
    if not reordered.exists():
        shutil.copytree(teacher, reordered)
        (reordered / "class_names.txt").write_text("flat\nblob\nbars\n")
    with pytest.raises(ValueError, match=r"has 3 classes, the run has 3 classes \(differing: order\)"):
        _main(_ini(tmp, ds, "i", 1, teacher=reordered))
    with pytest.raises(ValueError, match=r"distill_from: .*nowhere is not a model directory"):
        _main(_ini(tmp, ds, "j", 1, teacher=tmp / "nowhere"))
    for tag in "ghij":                    # refused before a model directory was made
        assert not (tmp / tag).exists(), tag
