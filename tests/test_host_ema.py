"""Host side of the weights' moving average (no GPU): the exactness of the tests' float64 oracle, the decay schedule,
`ema.ModelEma` on a recording stand-in for the net, the two `[train]` keys, what a resumed run checks and saves, and the
argument checks of the new C entry points."""

import ctypes
from collections import OrderedDict
from configparser import ConfigParser

import numpy as np
import pytest
import torch

import ema_util as U
from sykepic_hip import arch, config, ema, lib, train


def test_oracle_is_the_correctly_rounded_fused_result():
    """For every seeded element and every planted case, at each of the three weights, the float64 oracle equals the
    exactly computed e + w * float32(p - e) rounded once to float32 - what a fused multiply-add returns.  So the GPU
    tests compare bit for bit and exclude nothing."""
    e, p = U.seeded(U.N_SEEDED)
    for w in U.WEIGHTS:
        assert 0.0 < w < 1.0 and float(np.float32(w)) == w
        r = U.oracle(e, p, w)
        bad = [i for i in range(U.N_SEEDED) if not U.correctly_rounded(e[i], p[i], w, r[i])]
        assert not bad, (w, len(bad), bad[:5])
        for pe, pp, want in U.PLANTED:
            got = U.oracle(pe, pp, w)
            assert U.correctly_rounded(pe, pp, w, got), (w, pe, pp, got)
            if want is not None:      # the stated bits, sign of zero included
                assert U.bits1(got) == U.bits1(want), (w, pe, pp, got, want)
    # the inputs of the GPU test are these elements with the planted cases over the front
    e2, p2 = U.inputs(64)
    k = len(U.PLANTED)
    assert np.array_equal(U.bits(e2[k:]), U.bits(e[k:64])) and np.array_equal(U.bits(p2[k:]), U.bits(p[k:64]))
    assert U.bits1(e2[4]) == 0x80000000 and U.bits1(p2[4]) == 0x80000000
    assert [len(U.inputs(n)[0]) for n in (1, 2, 5)] == [1, 2, 5]
    big_e, big_p = U.inputs(U.N_SEEDED + 20)          # longer than the proven set: the same pairs again
    assert np.array_equal(U.bits(big_e[U.N_SEEDED:]), U.bits(e[:20])) and np.array_equal(U.bits(big_p[U.N_SEEDED:]), U.bits(p[:20]))


def test_decay_schedule():
    assert ema.decay_at(0.9998, True, 1) == 2.0 / 11.0
    assert ema.decay_at(0.9998, True, 2) == 3.0 / 12.0
    assert ema.decay_at(0.9, True, 1) == 2.0 / 11.0
    # the crossover: (1 + t) / (10 + t) >= 0.9 from t = 80 on (81 / 90 = 0.9 exactly in the reals; below it in double or not,
    # the minimum of the two is taken)
    assert ema.decay_at(0.9, True, 79) == 80.0 / 89.0 < 0.9
    assert ema.decay_at(0.9, True, 81) == 0.9 and ema.decay_at(0.9, True, 10 ** 6) == 0.9
    assert ema.decay_at(0.9, True, 80) == min(0.9, 81.0 / 90.0)
    seq = [ema.decay_at(0.9998, True, t) for t in range(1, 60000)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[-1] == 0.9998
    assert seq.index(0.9998) + 1 == 44990                       # (1 + t) / (10 + t) >= 0.9998  <=>  t >= 44990
    for t in (1, 2, 1000):
        assert ema.decay_at(0.9998, False, t) == 0.9998
    with pytest.raises(ValueError):
        ema.decay_at(0.9, True, 0)
    # the kernel's weight: 1 - d formed in double, rounded once
    assert ema.weight_of(0.9) == U.WEIGHTS[0] and ema.weight_of(0.9998) == U.WEIGHTS[1]
    assert ema.weight_of(ema.decay_at(0.9998, True, 1)) == U.WEIGHTS[2]


class _Net:
    """Records what `ModelEma` asks of a `HipNet`."""

    def __init__(self):
        self.calls, self.tensors = [], OrderedDict(a=torch.ones(2), b=torch.zeros(3))

    def ema_enable(self, on=True):
        self.calls.append(("enable", on))

    def ema_update(self, w):
        self.calls.append(("update", w))

    def ema_swap(self):
        self.calls.append(("swap",))

    def ema_state_dict(self):
        return OrderedDict(self.tensors)

    def load_ema_state_dict(self, sd):
        self.calls.append(("load", sorted(sd)))


def test_model_ema_drives_the_net():
    net = _Net()
    m = ema.ModelEma(net, 0.9)
    assert net.calls == [("enable", True)] and m.updates == 0 and m.describe() == {"decay": 0.9, "warmup": True}
    for _ in range(3):
        m.update()
    want = [float(np.float32(1.0 - d)) for d in (2.0 / 11.0, 3.0 / 12.0, 4.0 / 13.0)]
    assert net.calls[1:] == [("update", w) for w in want] and m.updates == 3
    flat = ema.ModelEma(_Net(), 0.9, warmup=False)
    flat.update()
    assert flat.net.calls[-1] == ("update", U.WEIGHTS[0]) and flat.describe() == {"decay": 0.9, "warmup": False}
    # applied(): swapped in for the block, swapped back whatever ends it
    del net.calls[:]
    with m.applied() as inner:
        assert inner is net and net.calls == [("swap",)]
    assert net.calls == [("swap",), ("swap",)]
    for exc in (KeyboardInterrupt, RuntimeError):
        del net.calls[:]
        with pytest.raises(exc):
            with m.applied():
                raise exc()
        assert net.calls == [("swap",), ("swap",)]
    # state: the tensors and the count
    sd = m.state_dict()
    assert sorted(sd) == ["tensors", "updates"] and sd["updates"] == 3 and list(sd["tensors"]) == ["a", "b"]
    other = ema.ModelEma(_Net(), 0.9)
    other.load_state_dict(sd)
    assert other.updates == 3 and other.net.calls[-1] == ("load", ["a", "b"])
    other.update()
    assert other.net.calls[-1] == ("update", float(np.float32(1.0 - 5.0 / 14.0)))
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), 1e-9):           # (the last: 1 - decay rounds to the float32 1.0)
        with pytest.raises(ValueError, match="ema_decay"):
            ema.ModelEma(_Net(), bad)


def _cfg(extra=""):
    cp = ConfigParser()
    cp.read_string("[train]\ngpu = yes\n" + extra)
    return cp


def test_config_keys_and_parsers():
    tr = config.Settings(_cfg()).train
    assert (tr.ema_decay, tr.ema_warmup) == (0.0, True)
    assert config.KEYS["train"]["ema_decay"][1] == "0" and config.KEYS["train"]["ema_warmup"][1] == "yes"
    assert config.get_model_ema(_cfg(), object()) is None                 # absent keys: no object, the net is not touched
    assert config.get_model_ema(_cfg("ema_decay = 0\n"), object()) is None
    assert config.get_model_ema(_cfg("ema_decay =\nema_warmup = no\n"), object()) is None
    tr = config.Settings(_cfg("ema_decay = 0.9998\nema_warmup = no\n")).train
    assert (tr.ema_decay, tr.ema_warmup) == (0.9998, False)
    net = _Net()
    m = config.get_model_ema(_cfg("ema_decay = 0.9\n"), net)
    assert isinstance(m, ema.ModelEma) and m.describe() == {"decay": 0.9, "warmup": True} and net.calls == [("enable", True)]
    for bad in ("1", "-0.1", "nan", "1.5", "inf"):
        with pytest.raises(ValueError, match="ema_decay"):                # the error names the key
            config.Settings(_cfg(f"ema_decay = {bad}\n")).train.ema_decay
    with pytest.raises(ValueError):
        config.Settings(_cfg("ema_warmup = maybe\n")).train.ema_warmup
    assert ema.describe(0.0, True) is None and ema.describe(0.9, False) == {"decay": 0.9, "warmup": False}


def _state(**over):
    s = {"format": train.TRAIN_STATE_FORMAT, "network": "resnet18", "classes": ["bars", "blob", "flat"],
         "img_shape": [3, 64, 64], "optimizer": "Adam", "world": 1}
    s.update(over)
    return s


_NOW = dict(network="resnet18", classes=["bars", "blob", "flat"], img_shape=(3, 64, 64), optimizer="Adam", world=1)


def test_resume_checks_the_ema_settings():
    on = {"decay": 0.9, "warmup": True}
    saved = dict(on, tensors={"a": torch.ones(1)}, updates=12)            # what the file's entry holds
    train.check_train_state(_state(), **_NOW)                             # a file without the key, a config without
    train.check_train_state(_state(), **_NOW, ema=None)
    train.check_train_state(_state(ema=saved), **_NOW, ema=dict(on))
    with pytest.raises(ValueError, match=r"cannot resume: ema differs, train_state.pth has off, the config gives decay 0.9, warmup yes"):
        train.check_train_state(_state(), **_NOW, ema=on)
    with pytest.raises(ValueError, match=r"cannot resume: ema differs, train_state.pth has decay 0.9, warmup yes, the config gives off"):
        train.check_train_state(_state(ema=saved), **_NOW)
    with pytest.raises(ValueError, match=r"cannot resume: ema differs, .*decay 0.9, .*decay 0.99,"):
        train.check_train_state(_state(ema=saved), **_NOW, ema={"decay": 0.99, "warmup": True})
    with pytest.raises(ValueError, match=r"cannot resume: ema differs, .*warmup yes.*warmup no") as e:
        train.check_train_state(_state(ema=saved), **_NOW, ema={"decay": 0.9, "warmup": False})
    assert "\n" not in str(e.value)


class _Param:
    key, requires_grad = "w", True


class _TrainNet(_Net):
    def train_counters(self):
        return {"steps": 3, "seed": 7}

    def state_dict(self):
        return {"w": torch.ones(1)}

    def parameters(self):
        return [_Param()]


class _Opt:
    param_groups = [{"params": [_Param()]}]

    def state_dict(self):
        return {}


def test_saved_state_has_no_new_key_without_ema():
    net = _TrainNet()
    assert sorted(train._rank_state(net)) == ["model", "python_rng", "torch_rng"]
    info = {"network": "resnet18", "classes": ["a"], "img_shape": [3, 8, 8], "optimizer": "Adam", "world": 1}
    off = train.collect_train_state(info, 2, False, False, net, _Opt(), None, {}, [], None)
    assert "ema" not in off
    assert sorted(train.collect_train_state(info, 2, False, False, net, _Opt(), None, {}, [], None, None)) == sorted(off)
    m = ema.ModelEma(net, 0.9, warmup=False)
    m.update()
    on = train.collect_train_state(dict(info, ema=m.describe()), 2, False, False, net, _Opt(), None, {}, [], None, m)
    assert sorted(on) == sorted(list(off) + ["ema"])
    assert sorted(on["ema"]) == ["decay", "tensors", "updates", "warmup"]
    assert (on["ema"]["decay"], on["ema"]["warmup"], on["ema"]["updates"]) == (0.9, False, 1)
    assert list(on["ema"]["tensors"]) == ["a", "b"]
    train.check_train_state(dict(on), network="resnet18", classes=["a"], img_shape=(3, 8, 8), optimizer="Adam", world=1,
                            ema=m.describe())


def test_average_has_float_keys_only():
    """`HipNet.load_ema_state_dict` takes exactly the float keys of `state_dict()`: an int64 `num_batches_tracked`
    entry, or a missing tensor, is refused on the host, before any library call (the handle does not exist here)."""
    from sykepic_hip.net import HipNet
    net = HipNet.__new__(HipNet)
    net._specs = arch.param_specs(arch.build_graph("resnet18", 5))
    keys = [k for k, _ in net._ema_specs()]
    kinds = {k: kind for k, _, kind in net._specs}
    assert keys == [k for k, _, kind in net._specs if kind != "bn_nbt"]
    assert "base.1.running_mean" in keys and "base.1.running_var" in keys and "base.0.weight" in keys
    assert not any(k.endswith("num_batches_tracked") for k in keys) and "bn_nbt" in kinds.values()
    full = {k: torch.zeros(shape) for k, shape in net._ema_specs()}
    with pytest.raises(RuntimeError, match=r"unexpected keys \['base.1.num_batches_tracked'\].*not averaged"):
        net.load_ema_state_dict(dict(full, **{"base.1.num_batches_tracked": torch.zeros((), dtype=torch.int64)}))
    del full["base.0.weight"]
    with pytest.raises(RuntimeError, match=r"missing keys \['base.0.weight'\]"):
        net.load_ema_state_dict(full)


def test_new_entry_points_reject_bad_arguments_without_gpu():
    """Every argument check comes before any HIP call: one rejected call per class of bad argument.  (The int64-key
    refusal of spk_model_ema_read / _load needs a handle: tests/test_gpu_ema_model.py.)"""
    so = lib.load()
    ARG = -1
    a = (ctypes.c_float * 256)()
    b = (ctypes.c_float * 256)()
    p, q = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)
    inside = ctypes.c_void_p(p.value + 16)
    odd = ctypes.c_void_p(q.value + 2)
    en, sw = ctypes.c_int(), ctypes.c_int()
    nan, inf = float("nan"), float("inf")
    bad = [
        ("spk_model_ema_enable", (None, 1)),
        ("spk_model_ema_enable", (None, 0)),
        ("spk_model_ema_swap", (None,)),
        ("spk_model_ema_state", (None, ctypes.byref(en), ctypes.byref(sw))),
        ("spk_model_ema_read", (None, b"base.0.weight", p, 4)),
        ("spk_model_ema_load", (None, b"base.0.weight", p, 4)),
        ("spk_model_ema_update", (None, 0.1)),
        # (e, p, n, w, stream)
        ("spk_op_ema_lerp", (None, q, 8, 0.1, None)),
        ("spk_op_ema_lerp", (p, None, 8, 0.1, None)),
        ("spk_op_ema_lerp", (p, q, 0, 0.1, None)),                       # n < 1
        ("spk_op_ema_lerp", (p, q, -4, 0.1, None)),
        ("spk_op_ema_lerp", (p, p, 8, 0.1, None)),                       # in place
        ("spk_op_ema_lerp", (p, inside, 8, 0.1, None)),                  # overlapping
        ("spk_op_ema_lerp", (inside, p, 8, 0.1, None)),
        ("spk_op_ema_lerp", (p, odd, 8, 0.1, None)),                     # a float at +2 bytes
        # (a, b, n, stream)
        ("spk_op_swap_f32", (None, q, 8, None)),
        ("spk_op_swap_f32", (p, None, 8, None)),
        ("spk_op_swap_f32", (p, q, 0, None)),
        ("spk_op_swap_f32", (p, p, 8, None)),
        ("spk_op_swap_f32", (inside, p, 5, None)),
        ("spk_op_swap_f32", (odd, p, 8, None)),
    ]
    for w in (0.0, 1.0, -0.5, nan, inf, -inf, 1.5):
        bad.append(("spk_op_ema_lerp", (p, q, 8, w, None)))
        # (a handle that is never reached: the weight is checked first)
        bad.append(("spk_model_ema_update", (None, w)))
    for name, args in bad:
        rc = getattr(so, name)(*args)
        assert rc == ARG, f"{name}{args}: rc {rc}"
        assert name[4:].encode() in so.spk_last_error(), (name, so.spk_last_error())
