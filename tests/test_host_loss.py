"""The class-weighted / label-smoothed loss away from the GPU: the argument checks of its three C-ABI symbols, the three
`[train]` keys, `balanced` weights, weight files, the descriptor, the resume check and the counter sum over two ranks."""

import ctypes
import os
import socket
import sys
from configparser import ConfigParser
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

from sykepic_hip import config, lib, train
from sykepic_hip import loss as L

ROOT = Path(__file__).resolve().parent.parent


def test_new_symbols_check_arguments_before_any_hip_call():
    so = lib.load()
    ARG = -1                       # SPK_ERR_ARG
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")
    bad = [
        ("spk_model_set_loss", (None, None, 0.0)),
        ("spk_model_set_loss", (None, p, 0.1)),
        ("spk_model_class_counts_read", (None, p, 0)),
        ("spk_model_class_counts_read", (None, None, 1)),
        ("spk_op_cross_entropy_ex", (None, p, 1, 4, None, 0.1, p, None, None, None)),      # no logits
        ("spk_op_cross_entropy_ex", (p, None, 1, 4, None, 0.1, p, None, None, None)),      # no labels
        ("spk_op_cross_entropy_ex", (p, p, 1, 4, None, 0.1, None, None, None, None)),      # no stats
        ("spk_op_cross_entropy_ex", (p, p, 0, 4, p, 0.1, p, None, None, None)),            # n
        ("spk_op_cross_entropy_ex", (p, p, 1, 0, p, 0.1, p, None, None, None)),            # c
        ("spk_op_cross_entropy_ex", (p, p, 1, 4, p, -0.01, p, None, None, None)),          # torch's range is [0, 1]
        ("spk_op_cross_entropy_ex", (p, p, 1, 4, p, 1.01, p, None, None, None)),
        ("spk_op_cross_entropy_ex", (p, p, 1, 4, p, nan, p, None, None, None)),
        ("spk_op_cross_entropy_ex", (p, p, 1, 4, p, inf, p, None, None, None)),
    ]
    for name, args in bad:
        rc = getattr(so, name)(*args)
        assert rc == ARG, f"{name}{args}: rc {rc}, expected {ARG}"
        assert name[4:].encode() in so.spk_last_error(), (name, so.spk_last_error())


INI = """[train]
gpu = yes
max_epochs = 3
early_stop_patience = 5
learning_rate = 0.01
optimizer = Adam
{extra}
"""


def _train_section(extra=""):
    c = ConfigParser()
    c.read_string(INI.format(extra=extra))
    return config.Settings(c).train


def test_config_keys_and_defaults():
    tr = _train_section()
    assert tr.label_smoothing == 0.0 and tr.class_weights == "none" and tr.checkpoint_on == "accuracy"
    for key in ("label_smoothing", "class_weights", "checkpoint_on"):
        assert config.KEYS["train"][key][1] is not config.REQUIRED
    tr = _train_section("label_smoothing = 0.1\nclass_weights = Balanced\ncheckpoint_on = balanced_accuracy")
    assert tr.label_smoothing == 0.1 and tr.class_weights == "balanced" and tr.checkpoint_on == "balanced_accuracy"
    tr = _train_section("class_weights = /some/Dir/weights.txt\nlabel_smoothing =\ncheckpoint_on =")
    assert tr.class_weights == "/some/Dir/weights.txt" and tr.label_smoothing == 0.0 and tr.checkpoint_on == "accuracy"
    assert _train_section("class_weights = none").class_weights == "none"
    with pytest.raises(ValueError, match="label_smoothing"):
        _train_section("label_smoothing = 1.5").label_smoothing
    with pytest.raises(ValueError, match="label_smoothing"):
        _train_section("label_smoothing = -0.1").label_smoothing
    with pytest.raises(ValueError, match="checkpoint_on"):
        _train_section("checkpoint_on = f1").checkpoint_on


def test_balanced_weights_by_hand():
    # 12 / 6 / 3 labels: N = 21, C = 3 -> 21 / 36, 21 / 18, 21 / 9
    labels = [0] * 12 + [1] * 6 + [2] * 3
    w = L.balanced_weights(labels, 3)
    assert w == [21 / 36, 21 / 18, 21 / 9]
    assert sum(w[y] for y in labels) == pytest.approx(21.0)          # W = N: every class contributes N / C
    assert L.balanced_weights([1, 0, 0, 1], 2) == [1.0, 1.0]
    with pytest.raises(ValueError, match="class id 2"):
        L.balanced_weights([0, 1, 1], 3)
    assert L.resolve_class_weights("none", ["a", "b"], [0, 1]) is None
    assert L.resolve_class_weights("", ["a", "b"], [0, 1]) is None
    assert L.resolve_class_weights("balanced", ["a", "b"], [0, 1, 1, 1]) == [2.0, 4 / 6]
    assert L.balanced_accuracy([(4, 2), (0, 0), (2, 2)]) == pytest.approx(0.75)   # unseen classes do not count


def test_weight_file_round_trip_and_errors(tmp_path):
    classes = ["bars", "blob", "flat"]
    f = tmp_path / "w.txt"
    f.write_text("flat 3.5\n\nbars 0.583333\nblob\t1.25\n")
    assert L.read_weight_file(f, classes) == [0.583333, 1.25, 3.5]
    assert L.resolve_class_weights(str(f), classes, []) == [0.583333, 1.25, 3.5]
    w = [21 / 36, 21 / 18, 21 / 9]
    out = L.write_weight_file(tmp_path, classes, w)
    assert out.name == L.CLASS_WEIGHTS_FILE and L.read_weight_file(out, classes) == w      # exact
    cases = {
        "bars 1\nblob 1\nflat 1\nblub 2\n": r"w.txt:4: 'blub' is not a class",
        "bars 1\nflat 1\n": r"no weight for class 'blob'",
        "bars 1\nblob 0\nflat 1\n": r"w.txt:2: the weight of 'blob' must be a finite number above 0",
        "bars 1\nblob -2\nflat 1\n": r"w.txt:2: .*above 0",
        "bars 1\nblob nan\nflat 1\n": r"w.txt:2: .*above 0",
        "bars 1\nblob inf\nflat 1\n": r"w.txt:2: .*above 0",
        "bars 1\nblob x\nflat 1\n": r"w.txt:2: 'x' is not a number",
        "bars 1\nblob 1 2\nflat 1\n": r"w.txt:2: expected `name weight`",
        "bars 1\nblob 1\nbars 2\nflat 1\n": r"w.txt:3: class 'bars' listed twice",
    }
    for text, pattern in cases.items():
        f.write_text(text)
        with pytest.raises(ValueError, match=pattern) as e:
            L.read_weight_file(f, classes)
        assert "\n" not in str(e.value)


def test_descriptor_from_torch_loss():
    assert L.from_loss_fn(None).is_default
    d = L.from_loss_fn(torch.nn.CrossEntropyLoss())
    assert d.is_default and d.describe() == {"label_smoothing": 0.0, "class_weights": None}
    d = L.from_loss_fn(torch.nn.CrossEntropyLoss(weight=torch.tensor([0.5, 2.0, 1.0]), label_smoothing=0.1))
    assert not d.is_default and d.weight == [0.5, 2.0, 1.0] and d.label_smoothing == 0.1
    ours = L.CrossEntropyLoss([1.0, 3.0], 0.25)
    assert L.from_loss_fn(ours) is ours and ours.reduction == "mean"
    for reduction in ("sum", "none"):
        with pytest.raises(ValueError, match="reduction"):
            L.from_loss_fn(torch.nn.CrossEntropyLoss(reduction=reduction))
    with pytest.raises(ValueError, match="ignore_index"):
        L.from_loss_fn(torch.nn.CrossEntropyLoss(ignore_index=3))
    with pytest.raises(TypeError):
        L.from_loss_fn(torch.nn.MSELoss())
    with pytest.raises(ValueError, match="class weight 1"):
        L.CrossEntropyLoss([1.0, 0.0])
    with pytest.raises(ValueError, match="class weight 0"):
        L.CrossEntropyLoss([float("nan"), 1.0])
    with pytest.raises(ValueError, match="label_smoothing"):
        L.CrossEntropyLoss(None, 1.5)


def test_train_net_refuses_another_reduction_before_touching_the_net():
    class Untouchable:
        def to(self, device):
            return self

        def __getattr__(self, name):
            raise AssertionError(f"train_net used net.{name} before it refused the loss")

    with pytest.raises(ValueError, match="reduction"):
        train.train_net(Untouchable(), [], [], None, torch.nn.CrossEntropyLoss(reduction="sum"), 1, 1, "unused", "cpu")


_NOW = dict(network="resnet18", classes=["bars", "blob", "flat"], img_shape=(3, 64, 64), optimizer="Adam", world=1)


def _state(**over):
    s = {"format": train.TRAIN_STATE_FORMAT, "network": "resnet18", "classes": ["bars", "blob", "flat"],
         "img_shape": [3, 64, 64], "optimizer": "Adam", "world": 1}
    s.update(over)
    return s


def test_resume_check_of_the_loss():
    assert train.TRAIN_STATE_FORMAT == 1
    w = [21 / 36, 21 / 18, 21 / 9]
    new = L.CrossEntropyLoss(w, 0.1).describe()
    default = L.CrossEntropyLoss().describe()
    # a file from before the loss had options: the defaults
    train.check_train_state(_state(), **_NOW)
    train.check_train_state(_state(), **_NOW, loss=default)
    train.check_train_state(_state(loss=default), **_NOW)
    train.check_train_state(_state(loss=new), **_NOW, loss=L.CrossEntropyLoss(list(w), 0.1).describe())
    through = torch.load(_saved(_state(loss=new)), weights_only=True)            # plain numbers: loads with weights_only
    train.check_train_state(through, **_NOW, loss=new)
    for state, now, pattern in (
            (_state(), new, r"loss differs.*has label_smoothing 0.0, class_weights none.*gives label_smoothing 0.1"),
            (_state(loss=new), None, r"loss differs.*has label_smoothing 0.1.*gives label_smoothing 0.0, class_weights none"),
            (_state(loss=new), L.CrossEntropyLoss(w, 0.2).describe(), r"loss differs"),
            (_state(loss=new), L.CrossEntropyLoss([1.0, 1.0, 2.0], 0.1).describe(), r"loss differs"),
            (_state(loss=new), L.CrossEntropyLoss(None, 0.1).describe(), r"loss differs")):
        with pytest.raises(ValueError, match=pattern) as e:
            train.check_train_state(state, **_NOW, loss=now)
        assert "\n" not in str(e.value)
    train.check_train_state(_state(checkpoint_on="balanced_accuracy"), **_NOW, checkpoint_on="balanced_accuracy")
    with pytest.raises(ValueError, match=r"checkpoint_on differs.*has accuracy.*gives balanced_accuracy"):
        train.check_train_state(_state(), **_NOW, checkpoint_on="balanced_accuracy")


def _saved(obj):
    import io
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return buf


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _counts_worker(rank, world, port, out_dir):
    for p in (ROOT, ROOT / "syke-pic_amd"):
        sys.path.insert(0, str(p))
    import torch.distributed as dist
    from sykepic_hip import dp
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sync = dp.GradSync(None, dist, view=torch.zeros(4))
    mine = torch.tensor([[5, 3], [0, 0], [2 ** 40, 7]]) if rank == 0 else torch.tensor([[1, 1], [4, 0], [1, 1]])
    keep = mine.clone()
    total = sync.reduce_class_counts(mine)
    torch.save({"total": total, "mine_after": mine, "mine_before": keep}, Path(out_dir) / f"c{rank}.pt")
    dist.destroy_process_group()


def test_class_counters_sum_over_two_ranks(tmp_path):
    mp.spawn(_counts_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(tmp_path / f"c{i}.pt") for i in range(2)]
    want = torch.tensor([[6, 4], [4, 0], [2 ** 40 + 1, 8]])
    for part in r:
        assert part["total"].dtype == torch.int64 and torch.equal(part["total"], want)
        assert torch.equal(part["mine_after"], part["mine_before"])        # the caller's tensor is not reduced in place
    # one process: the counters as they are
    from sykepic_hip import dp
    one = dp.GradSync(None, None, view=torch.zeros(4)).reduce_class_counts(torch.tensor([[3, 2]]))
    assert torch.equal(one, torch.tensor([[3, 2]]))
