"""`sykepic train --resume`: the resumed run IS the uninterrupted run.

Library state (optimizer moments, per-tensor and per-model counters) through `HipOptimizer.state_dict()` and the model's
counters, exactly; interchange of the optimizer state with torch.optim in both directions; the workflow in one process
and under two ranks."""

import io
import os
import random
import subprocess
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from sykepic_hip import arch, synth
from sykepic_hip.optim import HipOptimizer

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
OPTIMIZERS = ["SGD", "Adam", "AdamW", "RMSprop", "Adagrad", "Adamax", "NAdam", "RAdam", "Adadelta", "ASGD", "Rprop"]
LRS = (0.01, 0.003, 0.001)


def _start(network, classes, seed, **kw):
    g = arch.build_graph(network, classes, **kw)
    sd = synth.synth_state_dict(arch.param_specs(g), seed=seed, logit_gain=2.0)
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _fresh(network, classes, state, name, seed=None, **kw):
    """A new HipNet + HipOptimizer over `state`: every parameter trainable, spread over three groups."""
    from sykepic_hip.net import HipNet
    net = HipNet(network, classes, weights=None, **kw)
    net.load_state_dict(state)
    if seed is not None:
        net.set_seed(seed)
    params = list(net.parameters())
    for p in params:
        p.requires_grad = True
    groups = [{"params": params[i::3], "lr": lr} for i, lr in enumerate(LRS)]
    net.train()
    return net, HipOptimizer(net, name, groups)


def _batches(n, classes, hw, count):
    return [(torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=100 + s)).cuda(),
             torch.from_numpy(synth.synth_labels(n, classes, seed=200 + s)).cuda()) for s in range(count)]


def _steps(net, opt, batches):
    for x, y in batches:
        net.forward_backward(x, y)
        opt.step()


def _through_a_file(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


def _differing(a, b):
    assert list(a) == list(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_exact_continuation(name):
    """Run A: all steps.  Run B: all but the last, then weights + optimizer state + counters through torch.save /
    torch.load into a FRESH net and optimizer, which take the last step: every tensor equal to A's.  The control - the
    same fresh pair without the optimizer state - differs from A for every optimizer that keeps state (plain SGD keeps
    none and is equal)."""
    classes, n, hw = 10, 8, 64
    total = 8 if name == "RAdam" else 4      # RAdam: the save falls behind the switch to its rectified branch (step 6)
    batches = _batches(n, classes, hw, 4)
    batches = [batches[i % 4] for i in range(total)]
    start = _start("resnet18", classes, seed=7)
    net_a, opt_a = _fresh("resnet18", classes, start, name)
    _steps(net_a, opt_a, batches)
    final_a = net_a.state_dict()

    net_b, opt_b = _fresh("resnet18", classes, start, name)
    _steps(net_b, opt_b, batches[:-1])
    saved = _through_a_file({"net": dict(net_b.state_dict()), "opt": opt_b.state_dict(), "model": net_b.train_counters()})
    assert saved["model"]["steps"] == total - 1
    assert set(saved["opt"]) == {"state", "param_groups", "spk_exact"}
    assert [g["lr"] for g in saved["opt"]["param_groups"]] == list(LRS)
    assert sum(len(g["params"]) for g in saved["opt"]["param_groups"]) == len(list(net_b.parameters()))
    assert all(e["step"] == total - 1 for e in saved["opt"]["spk_exact"].values())
    del net_b, opt_b

    net_c, opt_c = _fresh("resnet18", classes, saved["net"], name)
    for g in opt_c.param_groups:
        g["lr"] = 0.5                      # load_state_dict brings the group's lr back
    opt_c.load_state_dict(saved["opt"])
    net_c.set_train_counters(saved["model"])
    assert [g["lr"] for g in opt_c.param_groups] == list(LRS)
    _steps(net_c, opt_c, batches[-1:])
    assert _differing(final_a, net_c.state_dict()) == []

    net_d, opt_d = _fresh("resnet18", classes, saved["net"], name)      # the control: no optimizer state
    net_d.set_train_counters(saved["model"])
    _steps(net_d, opt_d, batches[-1:])
    diff = _differing(final_a, net_d.state_dict())
    if name == "SGD":
        assert saved["opt"]["state"] == {} and diff == []
    else:
        assert saved["opt"]["state"] and diff, f"{name}: a step without its state gave the same tensors"


def test_sgd_momentum_buffer_continues():
    """SGD keeps state only with momentum: `momentum_buffer`, and the first-step rule must not fire again."""
    classes = 10
    batches = _batches(8, classes, 64, 3)
    start = _start("resnet18", classes, seed=7)
    net_a, opt_a = _fresh("resnet18", classes, start, "SGD")
    opt_a.defaults["momentum"] = 0.9
    _steps(net_a, opt_a, batches)
    net_b, opt_b = _fresh("resnet18", classes, start, "SGD")
    opt_b.defaults["momentum"] = 0.9
    _steps(net_b, opt_b, batches[:2])
    saved = _through_a_file({"net": dict(net_b.state_dict()), "opt": opt_b.state_dict()})
    assert set(saved["opt"]["state"][0]) == {"momentum_buffer"}
    net_c, opt_c = _fresh("resnet18", classes, saved["net"], "SGD")
    opt_c.load_state_dict(saved["opt"])
    assert opt_c.defaults["momentum"] == 0.9
    _steps(net_c, opt_c, batches[2:])
    assert _differing(net_a.state_dict(), net_c.state_dict()) == []


def test_mask_streams_continue():
    """EfficientNet-B0 (stochastic depth) with Dropout in the head: the masks of a step are a function of the model's
    seed and step counter, so the two steps after a restore equal the uninterrupted ones only if both come back."""
    classes, n, hw, kw = 10, 8, 32, dict(head=(256, 128), dropout=[(1, 0.5)])
    batches = _batches(n, classes, hw, 4)
    start = _start("efficientnet_b0", classes, seed=7, **kw)
    net_a, opt_a = _fresh("efficientnet_b0", classes, start, "Adam", seed=31, **kw)
    _steps(net_a, opt_a, batches)
    final_a = net_a.state_dict()
    net_b, opt_b = _fresh("efficientnet_b0", classes, start, "Adam", seed=31, **kw)
    _steps(net_b, opt_b, batches[:2])
    saved = _through_a_file({"net": dict(net_b.state_dict()), "opt": opt_b.state_dict(), "model": net_b.train_counters()})
    assert saved["model"] == {"steps": 2, "seed": 31}
    del net_b, opt_b

    def finish(counters):
        net, opt = _fresh("efficientnet_b0", classes, saved["net"], "Adam", **kw)
        opt.load_state_dict(saved["opt"])
        if counters:
            net.set_train_counters(counters)
        _steps(net, opt, batches[2:])
        return net.state_dict()

    assert _differing(final_a, finish(saved["model"])) == []
    assert _differing(final_a, finish({"steps": 0, "seed": 31}))        # the masks of steps 1 and 2 again
    assert _differing(final_a, finish({"steps": 2, "seed": 32}))        # another seed


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_state_interchange_with_torch(name):
    """Both directions, at the bound of the step-by-step comparison with torch.optim (test_gpu_train.py).  HIP -> torch:
    after three HIP steps the torch optimizer of the same name over CPU copies of the parameters loads
    `opt.state_dict()`, takes the HIP gradients of step four and lands where the HIP step lands.  torch -> HIP: three
    torch steps on HIP gradients (the HIP net follows on identical parameters, with an optimizer that is thrown away),
    then a fresh HipOptimizer loads `topt.state_dict()` and step four agrees."""
    classes, n, hw = 10, 8, 64
    batches = _batches(n, classes, hw, 4)
    start = _start("resnet18", classes, seed=7)

    def torch_side(net, params):
        before = net.state_dict()
        tparams = {p.key: torch.nn.Parameter(before[p.key].clone()) for p in params}
        topt = getattr(torch.optim, name)([{"params": [tparams[p.key] for p in params[i::3]], "lr": lr}
                                           for i, lr in enumerate(LRS)])
        return tparams, topt

    # HIP -> torch
    net, opt = _fresh("resnet18", classes, start, name)
    params = list(net.parameters())
    _steps(net, opt, batches[:3])
    tparams, topt = torch_side(net, params)
    topt.load_state_dict(_through_a_file(opt.state_dict()))
    assert [g["lr"] for g in topt.param_groups] == list(LRS)
    net.forward_backward(*batches[3])
    for p in params:
        tparams[p.key].grad = net._read_grad(p.key, p.shape)
    opt.step()
    topt.step()
    after = net.state_dict()
    bad = [k for k, tp in tparams.items() if not _close(after[k], tp.detach())]
    assert not bad, (name, "HIP -> torch", bad[:5])
    # ... and the two state dicts describe the same state after that step
    ts, hs = topt.state_dict()["state"], opt.state_dict()["state"]
    assert set(ts) == set(hs)
    for i in ts:
        assert set(ts[i]) == set(hs[i]), (i, set(ts[i]), set(hs[i]))
        assert float(ts[i].get("step", 4.0)) == float(hs[i].get("step", 4.0)) == 4.0
    del net, opt

    # torch -> HIP
    net, scratch = _fresh("resnet18", classes, start, name)
    params = list(net.parameters())
    tparams, topt = torch_side(net, params)
    for x, y in batches[:3]:
        net.forward_backward(x, y)
        for p in params:
            tparams[p.key].grad = net._read_grad(p.key, p.shape)
        topt.step()
        net.load_state_dict({k: tp.detach().clone() for k, tp in tparams.items()}, strict=False)
    sd = {k: v for k, v in net.state_dict().items()}
    net2, opt2 = _fresh("resnet18", classes, sd, name)
    opt2.load_state_dict(_through_a_file(topt.state_dict()))
    net2.forward_backward(*batches[3])
    for p in params:
        tparams[p.key].grad = net2._read_grad(p.key, p.shape)
    opt2.step()
    topt.step()
    after = net2.state_dict()
    bad = [k for k, tp in tparams.items() if not _close(after[k], tp.detach())]
    assert not bad, (name, "torch -> HIP", bad[:5])
    # torch's step counts came along (plain SGD keeps none in torch: its tensors count from this step)
    assert all(net2.param_counters(p.key)[0] == (1 if name == "SGD" else 4) for p in params)


def test_entry_points_before_any_step_and_their_errors():
    """A read before any training step returns zeros; an unknown key is SPK_ERR_KEY; a buffer, a wrong size or a slot
    other than 0 / 1 SPK_ERR_ARG; a load creates the training state and reads back, OIHW for a conv weight."""
    import ctypes as C
    from sykepic_hip import lib
    from sykepic_hip.net import HipNet
    net = HipNet("resnet18", 10, weights=None)
    net.load_state_dict(_start("resnet18", 10, seed=7))
    so, h = lib.load(), net._h
    key, shape = "base.0.weight", (64, 3, 7, 7)
    assert net.train_counters()["steps"] == 0 and net.param_counters(key) == (0, 1.0)
    assert float(net._read_optim_state(key, 0, shape).abs().max()) == 0.0
    buf = np.zeros(shape, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    KEY, ARG = -3, -1
    for fn in ("spk_model_optim_state_read", "spk_model_optim_state_load"):
        assert getattr(so, fn)(h, b"no.such.key", 0, p, buf.size) == KEY and b"no.such.key" in so.spk_last_error()
        assert getattr(so, fn)(h, key.encode(), 0, p, buf.size - 1) == ARG
        assert getattr(so, fn)(h, key.encode(), 2, p, buf.size) == ARG
        assert getattr(so, fn)(h, b"base.1.running_mean", 0, p, 64) == ARG
    step, mu = C.c_int64(), C.c_double()
    assert so.spk_model_param_counters_get(h, b"no.such.key", C.byref(step), C.byref(mu)) == KEY
    assert so.spk_model_param_counters_set(h, b"no.such.key", 1, 1.0) == KEY
    assert so.spk_model_param_counters_set(h, b"base.1.running_mean", 1, 1.0) == ARG
    assert so.spk_model_param_counters_set(h, key.encode(), -1, 1.0) == ARG
    val = torch.arange(buf.size, dtype=torch.float32).reshape(shape)
    net._load_optim_state(key, 1, val)
    assert torch.equal(net._read_optim_state(key, 1, shape), val)
    assert float(net._read_optim_state(key, 0, shape).abs().max()) == 0.0
    net.set_param_counters(key, 2 ** 40 + 1, 0.123456789012345678)
    assert net.param_counters(key) == (2 ** 40 + 1, 0.123456789012345678)
    net.set_train_counters({"steps": 2 ** 33, "seed": 2 ** 64 - 1})
    assert net.train_counters() == {"steps": 2 ** 33, "seed": 2 ** 64 - 1}


INI = """[dataset]
path = {ds}
split = 0.6, 0.2, 0.2
external_test =
min_N =
max_N =
exclude =
random_seed = 42
oversample_until = 12
oversample_with_decay =
[model]
path = {models}
network = resnet18
weights =
id = auto
exist_ok = no
head = 32, 16
dropout = {dropout}
[image]
shape = 3, 64, 64
augmentations = flip, translate, zoom, brightness
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
[lr_warmup]
use = yes
factor_1 = 0.1
factor_2 = 0.5
step_1 = {steps[0]}
step_2 = {steps[1]}
step_3 = {steps[2]}
verbose = no
[lr_reduction]
use = yes
factor = 0.1
patience = 4
verbose = yes
"""


def _dataset(ds):
    """The three synthetic classes of tests/test_gpu_workflows.py::test_train_main_end_to_end."""
    rng = np.random.RandomState(0)
    for ci, name in enumerate(("blob", "bars", "flat")):
        (ds / name).mkdir(parents=True)
        for i in range(20):
            h, w = rng.randint(30, 70), rng.randint(30, 90)
            img = np.full((h, w), 180, np.uint8)
            if ci == 0:
                img[h // 4: h // 2, w // 4: w // 2] = 40
            elif ci == 1:
                img[:, ::6] = 60
            img = np.clip(img.astype(np.int32) + rng.randint(-10, 10, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(ds / name / f"{name}_{i:02d}.png")


def _seed_all(v):
    random.seed(v)
    np.random.seed(v)
    torch.manual_seed(v)


def _stat_lines(out):
    """[STAT] Train / Val lines per epoch number."""
    epochs, cur = {}, None
    for ln in out.splitlines():
        if ln.startswith("----- Epoch "):
            cur = int(ln.split()[2])
            epochs[cur] = []
        elif ln.startswith("[STAT]") and cur is not None and "Test" not in ln:
            epochs[cur].append(ln)
    return epochs


def test_workflow_resume_is_the_uninterrupted_run(tmp_path, capsys):
    """`train.main` three times in one process (one tuner table): A six epochs; B the same ini stopped by
    `max_epochs = 3`; C `--resume` of B's directory with `max_epochs = 6`, started from other generator positions.
    Warm-up steps at epochs 2 / 3 / 4 and the plateau scheduler straddle the cut.  C's epochs 4-6 print A's [STAT]
    lines, and its final weights and best model are A's bit for bit; a finished directory resumed again trains no epoch
    and still reports."""
    from sykepic_hip import train
    A = namedtuple("A", "config collage dist save_images resume")
    ds = tmp_path / "ds"
    _dataset(ds)

    def ini(tag, epochs):
        f = tmp_path / f"{tag}.ini"
        f.write_text(INI.format(ds=ds, models=tmp_path / tag, epochs=epochs, steps=(2, 3, 4), dropout=""))
        return str(f)

    _seed_all(1234)
    train.main(A(ini("a", 6), None, None, None, None))
    out_a = capsys.readouterr().out
    _seed_all(1234)
    train.main(A(ini("b", 3), None, None, None, None))
    out_b = capsys.readouterr().out
    dir_a, dir_b = tmp_path / "a" / "resnet18_1", tmp_path / "b" / "resnet18_1"
    mid = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert mid["epoch"] == 3 and mid["ended"] and not mid["early_stopped"] and mid["world"] == 1
    assert mid["classes"] == ["bars", "blob", "flat"] and mid["img_shape"] == [3, 64, 64]
    assert [len(g) for g in mid["groups"]] == [len(g["params"]) for g in mid["optimizer_state"]["param_groups"]]
    assert mid["optimizer"] == "Adam" and mid["network"] == "resnet18"
    assert len(mid["groups"][1]) > 0 and len(mid["groups"][2]) == 0        # epoch 3: base[-2:] unfrozen, the rest not yet
    stamp = {f: (dir_b / f).read_bytes() for f in ("config.ini", "class_names.txt", "class_distribution.csv")}
    (dir_b / "test_report.txt").unlink()
    _seed_all(777)                              # a new process would not stand where the old one stopped
    train.main(A(ini("b", 6), None, None, None, str(dir_b)))
    out_c = capsys.readouterr().out
    assert "[ERROR]" not in out_a + out_b + out_c, out_c
    assert {f: (dir_b / f).read_bytes() for f in stamp} == stamp and not (tmp_path / "b" / "resnet18_2").exists()
    sa, sb, sc = _stat_lines(out_a), _stat_lines(out_b), _stat_lines(out_c)
    assert sorted(sa) == [1, 2, 3, 4, 5, 6] and sorted(sb) == [1, 2, 3] and sorted(sc) == [4, 5, 6]
    assert all(len(v) == 2 for v in sa.values())
    for e in (1, 2, 3):
        assert sb[e] == sa[e], e
    for e in (4, 5, 6):
        assert sc[e] == sa[e], (e, sc[e], sa[e])
    end_a = torch.load(dir_a / train.TRAIN_STATE_FILE, weights_only=True)
    end_c = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert end_a["epoch"] == end_c["epoch"] == 6 and end_c["ended"]
    assert _differing(end_a["net"], end_c["net"]) == []
    assert _differing(torch.load(dir_a / "best_state.pth"), torch.load(dir_b / "best_state.pth")) == []
    assert end_a["book"] == end_c["book"] and end_a["groups"] == end_c["groups"]
    assert len(end_c["groups"][2]) > 0
    assert (dir_b / "test_report.txt").is_file()
    # finished: nothing to train, the reports are written again
    (dir_b / "test_report.txt").unlink()
    train.main(A(ini("b", 6), None, None, None, str(dir_b)))
    out_d = capsys.readouterr().out
    assert "----- Epoch" not in out_d and "nothing to resume" in out_d and "[ERROR]" not in out_d
    assert "accuracy" in (dir_b / "test_report.txt").read_text()
    # another class list: refused in one line before any network is built
    (ds / "extra").mkdir()
    for i in range(10):
        Image.fromarray(np.full((40, 40), 10 * i, np.uint8)).save(ds / "extra" / f"extra_{i}.png")
    with pytest.raises(ValueError, match="class list differs"):
        train.main(A(ini("b", 6), None, None, None, str(dir_b)))


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_resume_two_ranks(tmp_path):
    """Two ranks over gloo on the one GPU (`torch.distributed.run`): four epochs uninterrupted against two epochs plus
    `--resume` to four; the chief's file holds both ranks' generator positions, the final weights are equal, and a
    resume with one rank is refused.  Dropout in the head: every rank keeps its own mask seed.  The command line seeds
    nothing but the dataset split (as the reference), so every process starts through a launcher that seeds the global
    generators - the resumed one with OTHER values, which the file must override.  One tuning cache, filled by a first
    run, serves the compared runs, so that all of them run the same kernel configurations."""
    ds = tmp_path / "ds"
    _dataset(ds)
    env = dict(os.environ, PYTHONPATH=f"{ROOT / 'syke-pic_amd'}:{os.environ.get('PYTHONPATH', '')}",
               MASTER_ADDR="127.0.0.1", SPK_TUNE_CACHE=str(tmp_path / "tune.txt"))

    launcher = tmp_path / "seeded_train.py"
    launcher.write_text("import random, sys\nimport numpy as np\nimport torch\n"
                        "seed = int(sys.argv[1])\nrandom.seed(seed); np.random.seed(seed); torch.manual_seed(seed)\n"
                        "from sykepic_hip.__main__ import main\nmain(sys.argv[2:])\n")

    def run(tag, epochs, resume=None, ranks=2, seed=1234):
        f = tmp_path / f"{tag}.ini"
        f.write_text(INI.format(ds=ds, models=tmp_path / tag, epochs=epochs, steps=(1, 2, 3), dropout="1,0.5"))
        cmd = ["timeout", "-k", "10", "300", sys.executable]
        if ranks > 1:
            cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                    "--master-port", str(_free_port())]
        cmd += [str(launcher), str(seed), "train", str(f)] + (["--resume", str(resume)] if resume else [])
        return subprocess.run(cmd, env=dict(env, SPK_DIST_BACKEND="gloo") if ranks > 1 else env, capture_output=True,
                              text=True, timeout=320)

    from sykepic_hip import train
    warm = run("w", 4)
    assert warm.returncode == 0, warm.stderr[-3000:]
    a = run("a", 4)
    assert a.returncode == 0, a.stderr[-3000:]
    b = run("b", 2)
    assert b.returncode == 0, b.stderr[-3000:]
    dir_a, dir_b = tmp_path / "a" / "resnet18_1", tmp_path / "b" / "resnet18_1"
    mid = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert mid["epoch"] == 2 and mid["world"] == 2 and len(mid["ranks"]) == 2 and mid["sampler_epoch"] == 2
    assert mid["ranks"][1]["model"]["seed"] == mid["ranks"][0]["model"]["seed"] + 1 == 42 * 2 + 1
    one = run("b", 4, resume=dir_b, ranks=1)
    assert one.returncode != 0 and "world size differs" in one.stderr, one.stderr[-3000:]
    c = run("b", 4, resume=dir_b, seed=777)
    assert c.returncode == 0, c.stderr[-3000:]
    assert "[ERROR]" not in a.stdout + b.stdout + c.stdout
    sa, sb, sc = _stat_lines(a.stdout), _stat_lines(b.stdout), _stat_lines(c.stdout)
    for e in (1, 2, 3, 4):
        print(f"epoch {e}: uninterrupted {sa.get(e)} | stopped after 2 {sb.get(e)} | resumed {sc.get(e)}")
    assert sorted(sc) == [3, 4]
    assert [sb[e] == sa[e] for e in (1, 2)] == [True, True], "two runs of the same two-rank job differ before any resume"
    assert [sc[e] == sa[e] for e in (3, 4)] == [True, True]
    end_a = torch.load(dir_a / train.TRAIN_STATE_FILE, weights_only=True)
    end_c = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert end_a["epoch"] == end_c["epoch"] == 4
    assert _differing(end_a["net"], end_c["net"]) == []
