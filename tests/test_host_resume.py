"""Host side of `sykepic train --resume` (no GPU): scheduler round trip, the command line, the checks a resumed run
makes against train_state.pth, atomic writes of the two checkpoint files, the rank gather, and the argument checks of
the new C entry points."""

import contextlib
import ctypes
import io
import json
import os
import random
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

from sykepic_hip import lib, schedule, train

ROOT = Path(__file__).resolve().parent.parent


class _Opt:
    """What the epoch loop and the schedulers touch of an optimizer."""

    def __init__(self, lr=1.0):
        self.param_groups = [{"params": [], "lr": lr}, {"params": [], "lr": 0.0}, {"params": [], "lr": 0.0}]
        self.grad_scale, self.steps = 1.0, 0

    def zero_grad(self):
        pass

    def step(self):
        self.steps += 1

    def sync_groups(self):
        pass

    def state_dict(self):
        return {"state": {}, "param_groups": [{"lr": g["lr"], "params": []} for g in self.param_groups],
                "spk_exact": {}, "steps": self.steps}

    def load_state_dict(self, sd):
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g["lr"] = s["lr"]
        self.steps = sd["steps"]


@pytest.mark.parametrize("config", ["plateau_q3", "sane"])
def test_plateau_scheduler_round_trip_mid_window(golden_dir, config):
    """Saved after any epoch - in the middle of a patience window in particular - and loaded into a fresh scheduler,
    the learning rates that follow are those of the uninterrupted scheduler: with the reference's quirk Q3 (`verbose`
    lands in `threshold`, the configuration of schedules.json) and with a sane threshold on a loss that stalls."""
    gold = json.loads((golden_dir / "schedules.json").read_text())["plateau_q3"]
    if config == "plateau_q3":
        factor, patience, threshold, losses = gold["factor"], gold["patience"], gold["threshold"], gold["val_loss"]
    else:
        factor, patience, threshold = 0.5, 2, 1e-4
        losses = [1.0, 0.9, 0.95, 0.93, 0.92, 0.91, 0.5, 0.6, 0.7, 0.8, 0.9, 0.4, 0.41, 0.42, 0.43]
    whole = _Opt()
    s = schedule.ReduceLROnPlateau(whole, "min", factor, patience, threshold)
    want = []
    for v in losses:
        s.step(v)
        want.append(whole.param_groups[0]["lr"])
    if config == "plateau_q3":
        assert want == pytest.approx(gold["lr_after"])
    assert want[-1] < 1.0                                  # the learning rate was cut somewhere: the comparison can fail
    mid_window = differs = 0
    for cut in range(1, len(losses)):
        first = _Opt()
        s1 = schedule.ReduceLROnPlateau(first, "min", factor, patience, threshold)
        for v in losses[:cut]:
            s1.step(v)
        mid_window += s1.state_dict()["num_bad_epochs"] > 0
        buf = io.BytesIO()
        torch.save({"sched": s1.state_dict(), "lr": first.param_groups[0]["lr"]}, buf)
        buf.seek(0)
        saved = torch.load(buf, weights_only=True)
        second = _Opt(saved["lr"])
        s2 = schedule.ReduceLROnPlateau(second, "min", factor, patience, threshold)
        s2.load_state_dict(saved["sched"])
        got = []
        for v in losses[cut:]:
            s2.step(v)
            got.append(second.param_groups[0]["lr"])
        assert got == want[cut:], cut
        # the control: the same learning rate but a fresh scheduler
        third = _Opt(saved["lr"])
        s3 = schedule.ReduceLROnPlateau(third, "min", factor, patience, threshold)
        for v in losses[cut:]:
            s3.step(v)
        differs += third.param_groups[0]["lr"] != want[-1]
    assert mid_window >= 2 and differs >= 1


def test_parser_accepts_resume():
    from sykepic_hip.__main__ import build_parser
    args = build_parser().parse_args(["train", "train.ini", "--resume", "models/resnet18_3"])
    assert args.resume == "models/resnet18_3" and args.config == "train.ini"
    assert build_parser().parse_args(["train", "train.ini"]).resume is None
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
        build_parser().parse_args(["train", "-h"])
    assert "--resume" in out.getvalue() and "repeats" in out.getvalue()


def _state(**over):
    s = {"format": train.TRAIN_STATE_FORMAT, "network": "resnet18", "classes": ["bars", "blob", "flat"],
         "img_shape": [3, 64, 64], "optimizer": "Adam", "world": 1}
    s.update(over)
    return s


_NOW = dict(network="resnet18", classes=["bars", "blob", "flat"], img_shape=(3, 64, 64), optimizer="Adam", world=1)


def test_resume_checks_name_what_differs():
    train.check_train_state(_state(), **_NOW)
    with pytest.raises(ValueError, match=r"class list differs.*2 classes.*3 classes.*flat"):
        train.check_train_state(_state(classes=["bars", "blob"]), **_NOW)
    with pytest.raises(ValueError, match=r"class list differs.*order"):
        train.check_train_state(_state(classes=["blob", "bars", "flat"]), **_NOW)
    with pytest.raises(ValueError, match=r"network differs.*resnet50.*resnet18"):
        train.check_train_state(_state(network="resnet50"), **_NOW)
    with pytest.raises(ValueError, match=r"format number 99"):
        train.check_train_state(_state(format=99, network="resnet50"), **_NOW)   # the format is looked at first
    with pytest.raises(ValueError, match=r"world size differs.*has 2.*gives 1"):
        train.check_train_state(_state(world=2), **_NOW)
    with pytest.raises(ValueError, match=r"image shape differs"):
        train.check_train_state(_state(img_shape=[3, 32, 32]), **_NOW)
    with pytest.raises(ValueError, match=r"optimizer differs.*SGD.*Adam"):
        train.check_train_state(_state(optimizer="SGD"), **_NOW)
    for bad in (_state(classes=["a"]), _state(world=2)):
        with pytest.raises(ValueError) as e:
            train.check_train_state(bad, **_NOW)
        assert "\n" not in str(e.value)


class _Param:
    def __init__(self, key):
        self.key, self.requires_grad = key, True


class _Net:
    """The calls `train_net` makes on a network, on the CPU: a weight that counts the steps and a scripted
    validation accuracy."""

    def __init__(self, val_acc):
        self.w, self.val_acc, self.val_calls = torch.zeros(3), list(val_acc), 0
        self.training, self.counters = True, {"steps": 0, "seed": 7}
        self._params = {"w": _Param("w")}

    def to(self, device):
        return self

    def train(self):
        self.training = True

    def eval(self):
        self.training = False

    def reset_stats(self):
        self.n = 0

    def forward_backward(self, x, y):
        self.w += 1
        self.counters["steps"] += 1
        self.n += len(y)

    def eval_step(self, x, y):
        self.n += len(y)

    def read_stats(self):
        if self.training:
            return 1.0 * self.n, 0.5 * self.n
        acc = self.val_acc[self.val_calls]
        self.val_calls += 1
        return (1.0 - acc) * self.n, acc * self.n

    def parameters(self):
        return iter(self._params.values())

    def named_parameters(self):
        return iter(self._params.items())

    def state_dict(self):
        return {"w": self.w.clone()}

    def load_state_dict(self, sd):
        self.w = sd["w"].clone()

    def train_counters(self):
        return dict(self.counters)

    def set_train_counters(self, c):
        self.counters = dict(c)


class _Sync:
    def __init__(self, net, dist=None):
        pass

    def all_reduce(self, optimizer=None):
        pass

    def reduce_stats(self, *a):
        return a

    def close(self):
        pass


_INFO = {"network": "stub", "classes": ["a", "b"], "img_shape": [3, 8, 8], "optimizer": "Adam", "world": 1}
_ACC = [0.50, 0.60, 0.70, 0.65, 0.80, 0.90]


def _run(monkeypatch, model_dir, max_epochs, resume=None, run_info=_INFO, net=None):
    monkeypatch.setattr(train, "GradSync", _Sync)
    monkeypatch.setattr(train, "_plot", lambda *a, **k: None)
    net = net or _Net(_ACC)
    if resume is not None:
        net.val_calls = resume["epoch"]
    opt = _Opt(0.01)
    sched = schedule.ReduceLROnPlateau(opt, "min", 0.1, 0, 1e-4)      # cuts the learning rate after epoch 4
    batches = [(torch.zeros(2, 1), torch.zeros(2, dtype=torch.int64))] * 3
    train.train_net(net, batches, batches[:1], opt, None, max_epochs, 50, model_dir, "cpu", sched, None,
                    run_info=run_info, resume=resume)
    return net, opt, sched


def test_train_state_file_round_trip_and_atomic_writes(tmp_path, monkeypatch, capsys):
    """The epoch loop on CPU stand-ins: train_state.pth is written every epoch, reads back with `weights_only=True`,
    and a run resumed from it ends where the uninterrupted one ends.  A `torch.save` that dies in the middle of the
    file leaves the previous train_state.pth and best_state.pth as they were, leaves no temporary file, and the loop
    goes on to the last epoch."""
    d = tmp_path / "m"
    d.mkdir()
    random.seed(11)
    torch.manual_seed(11)
    whole, wopt, wsched = _run(monkeypatch, d, 6)
    end = torch.load(d / train.TRAIN_STATE_FILE, weights_only=True)
    assert end["epoch"] == 6 and end["ended"] and not end["early_stopped"] and end["format"] == train.TRAIN_STATE_FORMAT
    assert end["book"]["val_accs"] == pytest.approx(_ACC) and end["book"]["max_val_acc"] == pytest.approx(0.9)
    assert torch.equal(torch.load(d / "best_state.pth")["w"], torch.full((3,), 18.0))

    d2 = tmp_path / "m2"
    d2.mkdir()
    random.seed(11)
    torch.manual_seed(11)
    _run(monkeypatch, d2, 3)
    random.seed(99)                  # a new process starts from other generator positions
    torch.manual_seed(99)
    state = train.load_train_state(d2)             # weights_only=True inside
    train.check_train_state(state, network="stub", classes=["a", "b"], img_shape=(3, 8, 8), optimizer="Adam", world=1)
    with pytest.raises(ValueError, match="optimizer differs, train_state.pth has Adam, the config gives SGD"):
        train.check_train_state(state, network="stub", classes=["a", "b"], img_shape=(3, 8, 8), optimizer="SGD", world=1)
    assert state["epoch"] == 3 and state["ended"] and state["network"] == "stub" and state["world"] == 1
    assert torch.equal(state["net"]["w"], torch.full((3,), 9.0)) and state["ranks"][0]["model"] == {"steps": 9, "seed": 7}
    assert isinstance(state["ranks"][0]["python_rng"], tuple) and state["ranks"][0]["torch_rng"].dtype == torch.uint8
    before = {f: (d2 / f).read_bytes() for f in (train.TRAIN_STATE_FILE, "best_state.pth")}

    real_save = torch.save
    calls = []

    def dying_save(obj, f, *a, **k):
        calls.append(str(f))
        with open(f, "wb") as fh:
            fh.write(b"half a file")
        raise OSError("No space left on device")

    monkeypatch.setattr(torch, "save", dying_save)
    capsys.readouterr()
    failed = _Net(_ACC)
    _run(monkeypatch, d2, 6, resume=state, net=failed)
    out = capsys.readouterr().out
    monkeypatch.setattr(torch, "save", real_save)
    assert failed.counters["steps"] == 18 and "----- Epoch 6 -----" in out and "[ERROR]" not in out
    assert out.count(f"Could not write {train.TRAIN_STATE_FILE}") == 3 and out.count("Could not write best_state.pth") == 2
    assert len(calls) == 5 and all(".tmp" in c for c in calls)
    assert {f: (d2 / f).read_bytes() for f in before} == before
    assert sorted(p.name for p in d2.iterdir()) == sorted(before)          # no temporary file left behind
    assert torch.load(d2 / train.TRAIN_STATE_FILE, weights_only=True)["epoch"] == 3
    assert torch.equal(torch.load(d2 / "best_state.pth")["w"], torch.full((3,), 9.0))

    # resumed for real: the same end as the uninterrupted run, generator positions included
    state = train.load_train_state(d2)
    _, ropt, rsched = _run(monkeypatch, d2, 6, resume=state)
    after_resumed = (random.random(), float(torch.rand(())))
    got = torch.load(d2 / train.TRAIN_STATE_FILE, weights_only=True)
    for k in ("epoch", "ended", "early_stopped", "book", "lr_scheduler", "groups", "requires_grad"):
        assert got[k] == end[k], k
    assert torch.equal(got["net"]["w"], end["net"]["w"]) and got["ranks"][0]["model"] == end["ranks"][0]["model"]
    assert [g["lr"] for g in ropt.param_groups] == [g["lr"] for g in wopt.param_groups]
    assert rsched.state_dict() == wsched.state_dict() and ropt.steps == wopt.steps == 18
    random.setstate(end["ranks"][0]["python_rng"])
    torch.set_rng_state(end["ranks"][0]["torch_rng"])
    assert after_resumed == (random.random(), float(torch.rand(())))
    assert torch.equal(torch.load(d2 / "best_state.pth")["w"], torch.full((3,), 18.0))


def test_save_train_state_no_writes_nothing(tmp_path, monkeypatch):
    from configparser import ConfigParser
    from sykepic_hip.config import Settings
    cp = ConfigParser()
    cp.read_string("[train]\ngpu = yes\n")
    assert Settings(cp).train.save_train_state is True            # on unless the ini says otherwise
    cp.set("train", "save_train_state", "no")
    assert Settings(cp).train.save_train_state is False
    d = tmp_path / "m"
    d.mkdir()
    _run(monkeypatch, d, 2, run_info=None)                        # what train.main passes for `save_train_state = no`
    assert sorted(p.name for p in d.iterdir()) == ["best_state.pth"]
    with pytest.raises(FileNotFoundError, match="nothing to resume"):
        train.load_train_state(d)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, out_dir):
    for p in (ROOT, ROOT / "syke-pic_amd"):
        sys.path.insert(0, str(p))
    import torch.distributed as dist
    from sykepic_hip import dp
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    random.seed(100 + rank)
    torch.manual_seed(200 + rank)
    mine = {"torch_rng": torch.get_rng_state(), "python_rng": random.getstate(), "model": {"steps": 3, "seed": 10 + rank}}
    got = dp.gather_object(mine, dist)
    again = dp.gather_object(rank, dist, dst=1)
    torch.save({"got": got, "again": again}, Path(out_dir) / f"g{rank}.pt")
    dist.destroy_process_group()


def test_gather_object_world2(tmp_path):
    """Every rank's generator positions arrive on the chief in rank order; the other ranks get None."""
    from sykepic_hip import dp
    assert dp.gather_object("x") == ["x"]                 # no process group: a list of one
    mp.spawn(_gather_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"g{i}.pt", weights_only=True) for i in range(2))
    assert r1["got"] is None and r0["again"] is None and r1["again"] == [0, 1]
    assert [s["model"]["seed"] for s in r0["got"]] == [10, 11]
    for rank, s in enumerate(r0["got"]):
        random.seed(100 + rank)
        assert s["python_rng"] == random.getstate()
        torch.manual_seed(200 + rank)
        assert torch.equal(s["torch_rng"], torch.get_rng_state())


def test_new_entry_points_reject_a_null_model_without_gpu():
    """Argument checks come before any HIP call.  (An unknown key needs a model handle, and a handle needs a device:
    that half is in tests/test_gpu_resume.py.)"""
    so = lib.load()
    ARG = -1
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    step, mu = ctypes.c_int64(), ctypes.c_double()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    bad = [
        ("spk_model_optim_state_read", (None, b"head.0.weight", 0, p, 8)),
        ("spk_model_optim_state_load", (None, b"head.0.weight", 1, p, 8)),
        ("spk_model_param_counters_get", (None, b"head.0.weight", ctypes.byref(step), ctypes.byref(mu))),
        ("spk_model_param_counters_set", (None, b"head.0.weight", 1, 1.0)),
        ("spk_model_train_counters_get", (None, ctypes.byref(a), ctypes.byref(b))),
        ("spk_model_train_counters_set", (None, 1, 2)),
    ]
    for name, args in bad:
        rc = getattr(so, name)(*args)
        assert rc == ARG, f"{name}: rc {rc}"
        assert name[4:].encode() in so.spk_last_error(), (name, so.spk_last_error())
