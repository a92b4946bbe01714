"""Test-time augmentation, the parts that need no GPU: the argument checks of `spk_tta_views` / `spk_tta_mean` (made
before any HIP call), the mode table of tta.py, the `--tta` flag, the trailing field of `EvalParams` and the
`[train] test_tta` key."""

import ctypes
from configparser import ConfigParser

import pytest

from sykepic_hip import config, lib, tta

ARG = -1                       # SPK_ERR_ARG
NHWC, NCHW = lib.LAYOUT_NHWC, lib.LAYOUT_NCHW
U8, F32, I64 = lib.DTYPE_U8, lib.DTYPE_F32, lib.DTYPE_I64


def _codes(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_refused_calls_of_both_entry_points():
    so = lib.load()
    buf = (ctypes.c_float * 4096)()                      # host memory: a refused call never touches it
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)
    q = ctypes.c_void_p(base + 8192)
    flip, one = _codes(0, 1, 2, 3), _codes(0)
    at = lambda off: ctypes.c_void_p(base + off)        # noqa: E731
    bad_views = [
        # (in, out, n, h, w, c, layout, dtype, views, k, stream)
        (None, q, 2, 4, 4, 3, NHWC, U8, flip, 4, None),
        (p, None, 2, 4, 4, 3, NHWC, U8, flip, 4, None),
        (p, q, 2, 4, 4, 3, NHWC, U8, None, 4, None),
        (p, q, 0, 4, 4, 3, NHWC, U8, flip, 4, None),
        (p, q, 2, 0, 4, 3, NHWC, U8, flip, 4, None),
        (p, q, 2, 4, -3, 3, NHWC, U8, flip, 4, None),
        (p, q, 2, 4, 4, 2, NHWC, U8, flip, 4, None),      # c
        (p, q, 2, 4, 4, 4, NCHW, F32, flip, 4, None),
        (p, q, 2, 4, 4, 3, NCHW, U8, flip, 4, None),      # the pair
        (p, q, 2, 4, 4, 3, NHWC, F32, flip, 4, None),
        (p, q, 2, 4, 4, 3, NCHW, I64, flip, 4, None),
        (p, q, 2, 4, 4, 3, NHWC, U8, flip, 0, None),      # k
        (p, q, 2, 4, 4, 3, NHWC, U8, _codes(0, 1, 2, 3, 4, 5, 6, 7, 0), 9, None),
        (p, q, 2, 4, 4, 3, NHWC, U8, _codes(0, 8), 2, None),        # a code
        (p, q, 2, 4, 4, 3, NHWC, U8, _codes(-1), 1, None),
        (p, q, 2, 4, 6, 3, NHWC, U8, _codes(0, 4), 2, None),        # transposing, h != w
        (p, q, 2, 6, 4, 3, NCHW, F32, _codes(7), 1, None),
        (p, p, 2, 4, 4, 3, NHWC, U8, one, 1, None),                 # overlap: the same buffer,
        (at(96), p, 2, 4, 4, 3, NHWC, U8, flip, 4, None),           # in inside out's second view,
        (p, at(95), 2, 4, 4, 3, NHWC, U8, flip, 4, None),           # out from in's last byte,
        (at(4 * 96 * 4 - 4), p, 2, 4, 4, 3, NCHW, F32, flip, 4, None),   # in from out's last float
    ]
    for args in bad_views:
        rc = so.spk_tta_views(*args)
        assert rc == ARG, f"spk_tta_views{args[2:8] + args[9:10]}: rc {rc}"
        assert b"spk_tta_views" in so.spk_last_error(), so.spk_last_error()
    bad_mean = [
        # (p, out, k, numel, stream)
        (None, q, 4, 10, None),
        (p, None, 4, 10, None),
        (p, q, 0, 10, None),
        (p, q, 9, 10, None),
        (p, q, -1, 10, None),
        (p, q, 4, 0, None),
        (p, q, 4, -5, None),
        (p, p, 1, 10, None),                               # overlap: the same buffer,
        (p, at(4 * 39), 4, 10, None),                      # out from p's last float,
        (at(36), p, 4, 10, None),                          # p from out's last float
    ]
    for args in bad_mean:
        rc = so.spk_tta_mean(*args)
        assert rc == ARG, f"spk_tta_mean{args[2:4]}: rc {rc}"
        assert b"spk_tta_mean" in so.spk_last_error(), so.spk_last_error()


def test_modes_and_shape_check():
    assert tta.MODES == {"none": (0,), "flip": (0, 1, 2, 3), "dihedral": (0, 1, 2, 3, 4, 5, 6, 7)}
    for name, codes in tta.MODES.items():
        assert tta.views_of(name) == codes
    for bad in ("rotate", "", "Flip", None, 4):
        with pytest.raises(ValueError, match="test-time augmentation"):
            tta.views_of(bad)
    for mode in tta.MODES:
        tta.check_shape(tta.views_of(mode), (3, 180, 180))
        tta.check_shape(tta.views_of(mode), [1, 64, 64])
    tta.check_shape(tta.views_of("none"), (3, 64, 48))
    tta.check_shape(tta.views_of("flip"), (3, 64, 48))
    tta.check_shape((0, 3, 3), (3, 1, 9))
    with pytest.raises(ValueError, match=r"\[image\] shape"):
        tta.check_shape(tta.views_of("dihedral"), (3, 64, 48))
    for v in (4, 5, 6, 7):
        with pytest.raises(ValueError, match=r"\[image\] shape"):
            tta.check_shape((0, v), (1, 48, 64))


def test_parser_takes_the_flag_on_prob_and_predict():
    from sykepic_hip.__main__ import build_parser
    parser = build_parser()
    for cmd in ("prob", "predict"):
        base = [cmd, "-r", "raw", "-m", "model", "-o", "out"]
        assert parser.parse_args(base).tta == "none"
        for mode in ("none", "flip", "dihedral"):
            assert parser.parse_args(base + ["--tta", mode]).tta == mode
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--tta", "rotate"])
    assert not hasattr(parser.parse_args(["train", "cfg.ini"]), "tta")


def test_eval_params_keeps_its_six_argument_form():
    from sykepic_hip import prob
    six = prob.EvalParams(64, 2, ["a", "b"], (3, 64, 64), None, "cuda:0")
    assert six.tta == "none" and six[:6] == (64, 2, ["a", "b"], (3, 64, 64), None, "cuda:0")
    assert prob.EvalParams._fields[:6] == ("batch_size", "num_workers", "classes", "img_shape", "transform", "device")
    assert prob.EvalParams._fields[-1] == "tta" and len(prob.EvalParams._fields) == 7
    assert prob.EvalParams(64, 2, [], (3, 64, 64), None, "cuda:0", "flip").tta == "flip"
    assert prob._views(six) is None and prob._views(six._replace(tta="dihedral")) == tuple(range(8))
    # callers that hand over their own six-field tuple keep working
    import collections
    old = collections.namedtuple("Old", prob.EvalParams._fields[:6])(64, 2, [], (3, 64, 64), None, "cuda:0")
    assert prob._views(old) is None


def _cfg(extra=""):
    cp = ConfigParser()
    cp.read_string("[train]\ngpu = yes\n" + extra)
    return cp


def test_config_key():
    assert config.KEYS["train"]["test_tta"][1] == "none"
    assert config.Settings(_cfg()).train.test_tta == "none"
    assert config.Settings(_cfg("test_tta =\n")).train.test_tta == "none"
    for mode in ("none", "flip", "dihedral"):
        assert config.Settings(_cfg(f"test_tta = {mode}\n")).train.test_tta == mode
    for bad in ("rotate", "4", "flip, dihedral"):
        with pytest.raises(ValueError, match="test_tta"):                 # the error names the key
            config.Settings(_cfg(f"test_tta = {bad}\n")).train.test_tta
