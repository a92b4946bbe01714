"""Host side of Mixup / CutMix (no GPU): the draw order of `mix.BatchMix.plan`, its properties and state, the four
`[train]` keys, what a resumed run checks and saves, and the argument checks of the three C entry points."""

import ctypes
import math
import random
import struct
from configparser import ConfigParser

import pytest
import torch

from sykepic_hip import config, lib, train
from sykepic_hip.mix import CUTMIX, MIXUP, BatchMix, f32

KINDS = [(0.4, 0.0), (0.0, 1.0), (0.4, 1.0)]          # Mixup only, CutMix only, both
SIZES = [(1, 1), (7, 12), (180, 180)]
PROBS = [0.0, 0.5, 1.0]


def _restated(rng, mixup_alpha, cutmix_alpha, prob, switch_prob, h, w):
    """The contract, written out again: what one batch draws from `rng`, in this order."""
    if rng.random() >= prob:
        return None
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cut = rng.random() < switch_prob
    else:
        cut = cutmix_alpha > 0
    alpha = cutmix_alpha if cut else mixup_alpha
    lam = rng.betavariate(alpha, alpha)
    if not cut:
        return MIXUP, lam, (0, 0, h, w)
    cx = rng.randrange(w)
    cy = rng.randrange(h)
    r = 0.5 * math.sqrt(1.0 - lam)
    rw, rh = int(r * w), int(r * h)
    y1, y2 = max(cy - rh, 0), min(cy + rh, h)
    x1, x2 = max(cx - rw, 0), min(cx + rw, w)
    return CUTMIX, 1.0 - (x2 - x1) * (y2 - y1) / (h * w), (y1, x1, y2, x2)


@pytest.mark.parametrize("alphas", KINDS, ids=["mixup", "cutmix", "both"])
@pytest.mark.parametrize("prob", PROBS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_plan_follows_the_draw_order(alphas, prob, hw):
    h, w = hw
    seed = 1000 + int(prob * 10)
    bm = BatchMix(*alphas, prob=prob, switch_prob=0.3, seed=seed)
    rng = random.Random(seed)
    kinds, mixed = set(), 0
    for step in range(200):
        got = bm.plan(8, h, w)
        want = _restated(rng, *alphas, prob, 0.3, h, w)
        if want is None:
            assert got is None, step
            continue
        mixed += 1
        kind, lam, box = want
        kinds.add(kind)
        assert (got.kind, got.lam, got.box) == (kind, lam, box), step
        y1, x1, y2, x2 = got.box
        assert 0 <= y1 <= y2 <= h and 0 <= x1 <= x2 <= w                  # inside the image
        assert 0.0 <= got.lam <= 1.0
        if kind == CUTMIX:
            assert got.lam == 1.0 - (x2 - x1) * (y2 - y1) / (h * w)       # recomputed from the clipped box
            assert (got.ca, got.cb) == (0.0, 1.0)
        else:
            assert got.box == (0, 0, h, w)
            assert got.ca == f32(lam) and got.cb == f32(1.0 - lam)        # 1 - lam in double, then rounded
            assert struct.pack("f", got.ca) == struct.pack("f", lam)
    assert bm.getstate() == rng.getstate()                                 # nothing else was drawn
    if prob == 0.0:
        assert mixed == 0
    elif prob == 1.0:
        assert mixed == 200
    else:
        assert 60 < mixed < 140
    if mixed:
        assert kinds == ({MIXUP, CUTMIX} if min(alphas) > 0 else {MIXUP} if alphas[0] > 0 else {CUTMIX})


def test_sequences_depend_on_the_seed_and_not_on_n():
    def seq(seed, n):
        bm = BatchMix(0.4, 1.0, prob=0.8, seed=seed)
        return [bm.plan(n, 33, 20) for _ in range(50)]
    assert seq(84, 1) == seq(84, 16) == seq(84, 5)
    assert seq(84, 16) != seq(85, 16)                   # seed * world + rank of two ranks of one job
    # the module-level generator is neither read nor moved
    random.seed(5)
    before = random.getstate()
    seq(3, 4)
    assert random.getstate() == before
    random.seed(6)
    assert seq(3, 4) == seq(3, 4)


def test_state_round_trip_mid_sequence():
    a = BatchMix(0.4, 1.0, seed=11)
    for _ in range(7):
        a.plan(4, 64, 64)
    buf = __import__("io").BytesIO()
    torch.save({"mix_rng": a.getstate()}, buf)
    buf.seek(0)
    saved = torch.load(buf, weights_only=True)["mix_rng"]
    rest = [a.plan(4, 64, 64) for _ in range(20)]
    b = BatchMix(0.4, 1.0, seed=999)
    b.setstate(saved)
    assert [b.plan(4, 64, 64) for _ in range(20)] == rest
    assert a.describe() == {"mixup_alpha": 0.4, "cutmix_alpha": 1.0, "prob": 1.0, "switch_prob": 0.5}


def test_constructor_refuses_bad_settings():
    for bad in ((0.0, 0.0), (-1.0, 1.0), (1.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(ValueError):
            BatchMix(*bad)
    for kw in ({"prob": 1.5}, {"prob": -0.1}, {"switch_prob": 2.0}, {"switch_prob": float("nan")}):
        with pytest.raises(ValueError):
            BatchMix(0.4, 1.0, **kw)


def _cfg(extra=""):
    cp = ConfigParser()
    cp.read_string("[train]\ngpu = yes\n" + extra)
    return cp


def test_config_keys_and_parsers():
    tr = config.Settings(_cfg()).train
    assert (tr.mixup_alpha, tr.cutmix_alpha, tr.mix_prob, tr.mix_switch_prob) == (0.0, 0.0, 1.0, 0.5)
    for key, default in (("mixup_alpha", "0"), ("cutmix_alpha", "0"), ("mix_prob", "1"), ("mix_switch_prob", "0.5")):
        assert config.KEYS["train"][key][1] == default
    assert config.get_batch_mix(_cfg(), seed=3) is None                               # absent keys: no object at all
    assert config.get_batch_mix(_cfg("mixup_alpha = 0\ncutmix_alpha =\n"), seed=3) is None
    tr = config.Settings(_cfg("mixup_alpha = 0.4\ncutmix_alpha = 1\nmix_prob = 0.75\nmix_switch_prob = 0\n")).train
    assert (tr.mixup_alpha, tr.cutmix_alpha, tr.mix_prob, tr.mix_switch_prob) == (0.4, 1.0, 0.75, 0.0)
    bm = config.get_batch_mix(_cfg("cutmix_alpha = 1.0\nmix_prob = 0.5\n"), seed=42 * 2 + 1)
    assert isinstance(bm, BatchMix) and bm.seed == 85
    assert bm.describe() == {"mixup_alpha": 0.0, "cutmix_alpha": 1.0, "prob": 0.5, "switch_prob": 0.5}
    for key, bad in (("mixup_alpha", "-0.1"), ("cutmix_alpha", "-1"), ("mixup_alpha", "nan"), ("cutmix_alpha", "inf"),
                     ("mix_prob", "1.5"), ("mix_prob", "-0.1"), ("mix_switch_prob", "2"), ("mix_switch_prob", "nan")):
        with pytest.raises(ValueError, match=key):                                    # the error names the key
            getattr(config.Settings(_cfg(f"{key} = {bad}\n")).train, key)


def _state(**over):
    s = {"format": train.TRAIN_STATE_FORMAT, "network": "resnet18", "classes": ["bars", "blob", "flat"],
         "img_shape": [3, 64, 64], "optimizer": "Adam", "world": 1}
    s.update(over)
    return s


_NOW = dict(network="resnet18", classes=["bars", "blob", "flat"], img_shape=(3, 64, 64), optimizer="Adam", world=1)


def test_resume_checks_the_mix_settings():
    on = BatchMix(0.4, 1.0).describe()
    train.check_train_state(_state(), **_NOW)                       # a file without the key, a config without mixing
    train.check_train_state(_state(), **_NOW, mix=None)
    train.check_train_state(_state(mix=None), **_NOW, mix=None)
    train.check_train_state(_state(mix=on), **_NOW, mix=dict(on))
    with pytest.raises(ValueError, match=r"cannot resume: mix differs, train_state.pth has off, the config gives .*mixup_alpha 0.4"):
        train.check_train_state(_state(), **_NOW, mix=on)
    with pytest.raises(ValueError, match=r"cannot resume: mix differs, train_state.pth has .*cutmix_alpha 1.*the config gives off"):
        train.check_train_state(_state(mix=on), **_NOW)
    other = BatchMix(0.4, 1.0, prob=0.5).describe()
    with pytest.raises(ValueError, match=r"mix differs.*prob 1.*prob 0.5") as e:
        train.check_train_state(_state(mix=on), **_NOW, mix=other)
    assert "\n" not in str(e.value)


class _Counters:
    def train_counters(self):
        return {"steps": 3, "seed": 7}


def test_rank_state_has_no_new_key_without_mixing():
    off = train._rank_state(_Counters())
    assert sorted(off) == ["model", "python_rng", "torch_rng"]
    assert sorted(train._rank_state(_Counters(), None)) == sorted(off)
    bm = BatchMix(0.4, 0.0, seed=5)
    bm.plan(2, 8, 8)
    on = train._rank_state(_Counters(), bm)
    assert sorted(on) == ["mix_rng", "model", "python_rng", "torch_rng"] and on["mix_rng"] == bm.getstate()


def test_new_entry_points_reject_bad_arguments_without_gpu():
    """Every argument check comes before any HIP call: one rejected call per class of bad argument."""
    so = lib.load()
    ARG = -1
    a = (ctypes.c_float * 256)()
    b = (ctypes.c_float * 256)()
    p, q = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)
    inside = ctypes.c_void_p(p.value + 16)
    odd = ctypes.c_void_p(q.value + 2)
    NCHW, NHWC, F32, U8 = lib.LAYOUT_NCHW, lib.LAYOUT_NHWC, lib.DTYPE_F32, lib.DTYPE_U8
    nan, inf = float("nan"), float("inf")
    bad = [
        # (in, out, n, h, w, c, layout, dtype, shift, ca, cb, y1, x1, y2, x2, stream)
        ("spk_mix_batch", (None, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, None, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, q, 0, 4, 4, 3, NHWC, U8, 0, 0.5, 0.5, 0, 0, 4, 4, None)),          # n < 1
        ("spk_mix_batch", (p, q, 2, 0, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 0, 4, None)),          # h < 1
        ("spk_mix_batch", (p, q, 2, 4, 4, 2, NHWC, U8, 1, 0.5, 0.5, 0, 0, 4, 4, None)),          # c
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NCHW, U8, 1, 0.5, 0.5, 0, 0, 4, 4, None)),          # layout / dtype pair
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, F32, 1, 0.5, 0.5, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NCHW, lib.DTYPE_I64, 1, 0.5, 0.5, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, -1, 0.5, 0.5, 0, 0, 4, 4, None)),         # shift
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 2, 0.5, 0.5, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, nan, 0.5, 0, 0, 4, 4, None)),          # ca / cb
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, inf, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 5, 4, None)),          # box outside
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 4, 5, None)),
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, -1, 0, 4, 4, None)),
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 3, 0, 2, 4, None)),          # inverted
        ("spk_mix_batch", (p, q, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 3, 4, 2, None)),
        ("spk_mix_batch", (p, p, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 4, 4, None)),          # in place
        ("spk_mix_batch", (p, inside, 2, 4, 4, 3, NHWC, U8, 1, 0.5, 0.5, 0, 0, 4, 4, None)),     # overlapping
        ("spk_mix_batch", (inside, p, 2, 4, 4, 3, NCHW, F32, 1, 0.5, 0.5, 0, 0, 4, 4, None)),
        ("spk_mix_batch", (p, odd, 2, 4, 4, 3, NCHW, F32, 1, 0.5, 0.5, 0, 0, 4, 4, None)),       # a float32 batch at +2 bytes
        # (z, ya, yb, lam, n, c, w, label_smoothing, stats, counts, dz, stream)
        ("spk_op_cross_entropy_pair", (None, p, p, 0.5, 1, 4, None, 0.0, p, None, None, None)),
        ("spk_op_cross_entropy_pair", (p, None, p, 0.5, 1, 4, None, 0.0, p, None, None, None)),
        ("spk_op_cross_entropy_pair", (p, p, p, 0.5, 1, 4, None, 0.0, None, None, None, None)),
        ("spk_op_cross_entropy_pair", (p, p, p, 0.5, 0, 4, None, 0.0, p, None, None, None)),     # n < 1
        ("spk_op_cross_entropy_pair", (p, p, p, -0.1, 1, 4, None, 0.0, p, None, None, None)),    # lam
        ("spk_op_cross_entropy_pair", (p, p, p, 1.5, 1, 4, None, 0.0, p, None, None, None)),
        ("spk_op_cross_entropy_pair", (p, p, p, nan, 1, 4, None, 0.0, p, None, None, None)),
        ("spk_op_cross_entropy_pair", (p, p, p, inf, 1, 4, None, 0.0, p, None, None, None)),
        ("spk_op_cross_entropy_pair", (p, p, None, nan, 1, 4, None, 0.0, p, None, None, None)),  # ... also without yb
        ("spk_op_cross_entropy_pair", (p, p, p, 0.5, 1, 4, None, 1.5, p, None, None, None)),     # label_smoothing
        # (m, x, n, h, w, layout, dtype, ya, yb, lam, stats, logits): none of these reaches the handle
        ("spk_train_forward_backward_pair", (None, p, 2, 4, 4, NCHW, F32, p, p, 0.5, p, None)),
        ("spk_train_forward_backward_pair", (q, None, 2, 4, 4, NCHW, F32, p, p, 0.5, p, None)),
        ("spk_train_forward_backward_pair", (q, p, 2, 4, 4, NCHW, F32, None, p, 0.5, p, None)),
        ("spk_train_forward_backward_pair", (q, p, 2, 4, 4, NCHW, F32, p, p, 0.5, None, None)),
        ("spk_train_forward_backward_pair", (q, p, 0, 4, 4, NCHW, F32, p, p, 0.5, p, None)),     # n < 1
        ("spk_train_forward_backward_pair", (q, p, 2, 4, 4, NCHW, F32, p, p, 1.5, p, None)),     # lam
        ("spk_train_forward_backward_pair", (q, p, 2, 4, 4, NCHW, F32, p, p, -0.5, p, None)),
        ("spk_train_forward_backward_pair", (q, p, 2, 4, 4, NCHW, F32, p, None, nan, p, None)),
    ]
    for name, args in bad:
        rc = getattr(so, name)(*args)
        assert rc == ARG, f"{name}{args[2:-1]}: rc {rc}"
        assert name[4:].encode() in so.spk_last_error(), (name, so.spk_last_error())
