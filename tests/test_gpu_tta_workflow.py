"""Test-time augmentation through the entry points: `sykepic prob` with `tta = flip` on the reference's raw fixture
(the synthetic model directory of tests/test_gpu_workflows.py), and `sykepic train` with `[train] test_tta = flip` on
the dataset of tests/test_gpu_resume.py."""

import contextlib
import io
import logging
import shutil
from collections import namedtuple

import pytest

import test_gpu_resume as R
import test_gpu_workflows as W

pytestmark = pytest.mark.gpu

SAMPLE = "D20180712T065600_IFCB114"
TtaArgs = namedtuple("TtaArgs", W.Args._fields + ("tta",))


def _raw(tmp_path, golden_dir):
    raw = tmp_path / "raw" / "valid"
    raw.mkdir(parents=True)
    for ext in ("adc", "hdr", "roi"):
        shutil.copy(golden_dir / "ref_data" / f"{SAMPLE}.{ext}", raw)
    return raw


def test_prob_call_with_flip_views(tmp_path, golden_dir, caplog):
    from sykepic_hip import gpu_preprocess, prob, tta
    raw = _raw(tmp_path, golden_dir)
    model, _ = W._model_dir(tmp_path, golden_dir)
    out_plain, out_tta, out_none = tmp_path / "plain", tmp_path / "tta", tmp_path / "none"
    # a caller that knows nothing of the field, and one that names `none`: the plain file, byte for byte
    prob.call(W.Args(str(raw), None, None, None, str(model), out_plain, 64, 2, False))
    prob.call(TtaArgs(str(raw), None, None, None, str(model), out_none, 64, 2, False, "none"))
    with caplog.at_level(logging.INFO, logger="prob"):
        prob.call(TtaArgs(str(raw), None, None, None, str(model), out_tta, 64, 2, False, "flip"))
    said = [r.message for r in caplog.records if "test-time augmentation" in r.message]
    assert len(said) == 1 and "flip" in said[0] and "4 views" in said[0]
    rel = f"2018/07/12/{SAMPLE}.prob.csv"
    for out in (out_plain, out_tta, out_none):
        assert [p.relative_to(out).as_posix() for p in out.glob("**/*.csv")] == [rel]
    plain, got = (out_plain / rel).read_text(), (out_tta / rel).read_text()
    assert (out_none / rel).read_bytes() == (out_plain / rel).read_bytes()
    lp, lg = plain.splitlines(), got.splitlines()
    assert len(lg) == len(lp) == 3 and lg[0] == lp[0] and lg[0].startswith("roi,") and len(lg[0].split(",")) == 51
    assert [ln.split(",")[0] for ln in lg[1:]] == [ln.split(",")[0] for ln in lp[1:]] == ["2", "3"]
    assert got != plain                                         # the views say something else than the original alone
    rows = [[float(v) for v in ln.split(",")[1:]] for ln in lg[1:]]
    for row in rows:
        assert len(row) == 50 and abs(sum(row) - 1.0) <= 50 * 0.5e-5 + 1e-4       # `%.5f` rounding of 50 values
    # every row is `probabilities_tta` of that ROI's preprocessed tensor, formatted
    net, classes, img_shape, transform, device = prob.prepare_model(model)
    assert gpu_preprocess.supported(transform, img_shape[0])
    gs = gpu_preprocess.SampleOnGpu(raw / f"{SAMPLE}.adc", raw / f"{SAMPLE}.roi", device)
    th, tw = transform.target_dims
    x = gs.batch(0, len(gs), th, tw, gpu_preprocess.border_code(transform))
    want = net.probabilities_tta(x, tta.views_of("flip")).cpu().tolist()
    assert [int(v) for v in gs.numbers[:len(gs)]] == [2, 3]
    fmt = "%d," + ",".join(["%.5f"] * 50)
    assert lg[1:] == [fmt % (num, *p) for num, p in zip((2, 3), want)]
    # an unknown mode is refused before anything is loaded
    with pytest.raises(ValueError, match="test-time augmentation"):
        prob.call(TtaArgs(str(raw), None, None, None, str(model), tmp_path / "bad", 64, 2, False, "rotate"))
    assert not (tmp_path / "bad").exists()
    # a mode the image shape cannot take is refused before the first sample: `dihedral` on a rectangular [image] shape,
    # which `flip` classifies
    cfg = (model / "config.ini").read_text()
    assert "shape = 3, 180, 180" in cfg
    (model / "config.ini").write_text(cfg.replace("shape = 3, 180, 180", "shape = 3, 180, 120"))
    with pytest.raises(ValueError, match=r"\[image\] shape"):
        prob.call(TtaArgs(str(raw), None, None, None, str(model), tmp_path / "rect", 64, 2, False, "dihedral"))
    assert not (tmp_path / "rect").exists()
    prob.call(TtaArgs(str(raw), None, None, None, str(model), tmp_path / "rect", 64, 2, False, "flip"))
    lr = (tmp_path / "rect" / rel).read_text().splitlines()
    assert len(lr) == 3 and lr[0] == lg[0] and [ln.split(",")[0] for ln in lr[1:]] == ["2", "3"]
    for ln in lr[1:]:
        assert abs(sum(float(v) for v in ln.split(",")[1:]) - 1.0) <= 50 * 0.5e-5 + 1e-4


def test_train_main_writes_both_reports(tmp_path):
    """Two epochs on the three synthetic classes with `test_tta = flip`: the plain report as ever, and beside it the
    report of the averaged views, whose first printed line names the mode."""
    from sykepic_hip import train
    ds = tmp_path / "ds"
    R._dataset(ds)
    ini = tmp_path / "t.ini"
    text = R.INI.replace("optimizer = Adam\n", "optimizer = Adam\ntest_tta = flip\n")
    assert text != R.INI
    ini.write_text(text.format(ds=ds, models=tmp_path / "m", epochs=2, steps=(1, 2, 3), dropout=""))
    R._seed_all(1234)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(namedtuple("A", "config collage dist save_images resume")(str(ini), None, None, None, None))
    out = buf.getvalue()
    assert "[ERROR]" not in out, out
    mdir = tmp_path / "m" / "resnet18_1"
    plain, tta_report = (mdir / "test_report.txt").read_text(), (mdir / "test_report_tta.txt").read_text()
    for report in (plain, tta_report):
        assert "accuracy" in report and "precision" in report and "macro avg" in report
        assert all(name in report for name in ("bars", "blob", "flat"))
    heads = [ln for ln in out.splitlines() if ln.startswith("----- Model Evaluation")]
    assert heads == ["----- Model Evaluation -----", "----- Model Evaluation, test-time augmentation flip: 4 views -----"]
    assert out.count("[STAT] Test Accuracy") == 2
    assert sorted(p.name for p in mdir.glob("test_report*")) == ["test_report.txt", "test_report_tta.txt"]
    # a bad mode, and a mode the shape cannot take, end the run before any training
    for bad, what in (("test_tta = rotate\n", "test_tta"), ("test_tta = dihedral\n", r"\[image\] shape")):
        t2 = R.INI.replace("optimizer = Adam\n", "optimizer = Adam\n" + bad)
        if "dihedral" in bad:
            t2 = t2.replace("shape = 3, 64, 64", "shape = 3, 64, 48")
        ini2 = tmp_path / "bad.ini"
        ini2.write_text(t2.format(ds=ds, models=tmp_path / "bad", epochs=1, steps=(1, 2, 3), dropout=""))
        with pytest.raises(ValueError, match=what):
            train.main(namedtuple("A", "config collage dist save_images resume")(str(ini2), None, None, None, None))
        assert not (tmp_path / "bad").exists()
