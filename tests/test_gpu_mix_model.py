"""Mixup / CutMix in the training step and the training workflow: `HipNet.forward_backward(x, y, y2=, lam=)` leaves the
loss, the counters and dlogits of the two-label criterion (checked on the step's own logits under the bounds of
tests/test_gpu_loss_pair_ops.py), `lam = 1` is the step that never heard of a second label vector, `train_net` mixes
every training batch once and no validation batch, and a resumed run with mixing on is the uninterrupted run."""

from collections import namedtuple

import numpy as np
import pytest
import torch

import test_gpu_loss_model as M
import test_gpu_loss_ops as K
import test_gpu_loss_pair_ops as P
import test_gpu_resume as R
from sykepic_hip import dp
from sykepic_hip.mix import BatchMix
from sykepic_hip.optim import HipOptimizer

pytestmark = pytest.mark.gpu

CLASSES, N = M.CLASSES, M.N
LAM = float(np.float32(0.3))


@pytest.mark.parametrize("loss", ["weights+smoothing", "default"])
def test_pair_step_matches_float64_on_its_own_logits(loss):
    net, _ = M._net()
    x, ya = M._batch(0)
    yb = ya.roll(1)
    assert not torch.equal(ya, yb)
    w, eps = (torch.tensor(M.WEIGHTS, dtype=torch.float32), K._f32(M.SMOOTH)) if loss != "default" else (None, 0.0)
    if w is not None:
        net.set_loss(M.WEIGHTS, M.SMOOTH)
    net.train()
    for lam in (LAM, 0.5):
        net.reset_stats()
        logits = net.forward_backward(x, ya, want_logits=True, y2=yb, lam=lam)
        z, la, lb = logits.cpu(), ya.cpu(), yb.cpu()
        ref_loss, ref_dz = P._reference(z, la, lb, lam, w, eps)
        dz_bound, loss_bound = P._pair_bounds(z, la, lb, lam, w, eps)
        loss_n, correct = net.read_stats()
        what = f"pair step ({loss}, lam {lam:.3g})"
        K.H._ratio(torch.tensor([loss_n]), torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1), f"{what} n*loss")
        want_counts, want_correct = K._counts_ref(z, la if lam >= 0.5 else lb)
        assert correct == want_correct, what
        if w is not None:
            assert torch.equal(net.read_class_counts(reset=True), want_counts), what
        else:
            with pytest.raises(RuntimeError, match="default loss keeps no per-class counters"):
                net.read_class_counts()
        t = net.graph.ops[-1].dst
        K.H._ratio(net.read_activation_grad(t, N, (N, CLASSES)), ref_dz, dz_bound, f"{what} dlogits")
    # the criterion really is another loss than CE on ya alone
    net.reset_stats()
    net.forward_backward(x, ya)
    assert abs(net.read_stats()[0] - loss_n) > 1e-3


@pytest.mark.parametrize("loss", ["default", "weights+smoothing"])
def test_lam_one_is_the_single_label_step_bit_for_bit(loss):
    """Twin models, two steps with an Adam step between them: `forward_backward(x, y, y2=other, lam=1.0)` (and
    `y2=None` with any lam) against `forward_backward(x, y)` - equal statistics and flat gradient buffers.  With the
    default loss that is the plain kernel."""
    def run(how):
        net, _ = M._net()
        if loss != "default":
            net.set_loss(M.WEIGHTS, M.SMOOTH)
        params = list(net.parameters())
        for p in params:
            p.requires_grad = True
        opt = HipOptimizer(net, "Adam", [{"params": params, "lr": 0.01}])
        net.train()
        net.reset_stats()
        for s in range(2):
            x, y = M._batch(s)
            if how == "plain":
                net.forward_backward(x, y)
            elif how == "lam1":
                net.forward_backward(x, y, y2=y.roll(1), lam=1.0)
            else:
                net.forward_backward(x, y, y2=None, lam=0.25)
            if s == 0:
                opt.step()
        ptr, numel = net.grad_buffer()
        flat = torch.as_tensor(dp._DevicePtr(ptr, numel), device=net.device).clone()
        return torch.tensor(net.read_stats()), flat.cpu()

    stats_a, flat_a = run("plain")
    assert float(flat_a.abs().max()) > 0
    for how in ("lam1", "no-y2"):
        stats_b, flat_b = run(how)
        assert torch.equal(stats_a, stats_b) and torch.equal(flat_a, flat_b), how


class _Counting:
    """A `BatchMix` that notes how it is called."""

    def __init__(self, inner, net):
        self.inner, self.net, self.calls, self.mixed, self.bad = inner, net, 0, 0, []

    def __call__(self, x, y):
        self.calls += 1
        if not self.net.training:
            self.bad.append("called in eval mode")
        if not (x.is_cuda and y.is_cuda):
            self.bad.append("called on a host batch")
        out = self.inner(x, y)
        self.mixed += out[2] is not None
        return out

    def getstate(self):
        return self.inner.getstate()

    def setstate(self, s):
        self.inner.setstate(s)

    def describe(self):
        return self.inner.describe()


def test_train_net_mixes_every_training_batch_once_and_no_other(tmp_path, capsys):
    """Two host batches per epoch (CPU tensors, as the host loader delivers them), one validation batch, two epochs."""
    from sykepic_hip import train
    net, _ = M._net()
    params = list(net.parameters())
    for p in params:
        p.requires_grad = True
    opt = HipOptimizer(net, "Adam", [{"params": params, "lr": 0.001}, {"params": [], "lr": 0.0}, {"params": [], "lr": 0.0}])
    batches = [tuple(t.cpu() for t in M._batch(s)) for s in range(3)]
    mix = _Counting(BatchMix(0.4, 1.0, seed=5), net)
    train.train_net(net, batches[:2], batches[2:], opt, None, 2, 50, tmp_path, net.device, batch_mix=mix)
    out = capsys.readouterr().out
    assert "[ERROR]" not in out, out
    assert out.count("[STAT] Train Acc") == 2 and out.count("[STAT] Val Acc") == 2
    assert mix.calls == 4 and mix.mixed == 4 and mix.bad == []
    assert net.train_counters()["steps"] == 4


def test_resume_with_mixing_is_the_uninterrupted_run(tmp_path, capsys):
    """`train.main` with `mixup_alpha = 0.4`, `cutmix_alpha = 1.0`: A two epochs; B one epoch; C `--resume` of B's
    directory to two, started from other generator positions.  C's epoch 2 prints A's [STAT] lines, and its final
    `train_state.pth` tensors and `best_state.pth` are A's bit for bit.  The file names the mix and holds its generator;
    resuming it with mixing off in the config is refused in one line."""
    from sykepic_hip import train
    A = namedtuple("A", "config collage dist save_images resume")
    ds = tmp_path / "ds"
    R._dataset(ds)

    def ini(tag, epochs, mix=True):
        text = R.INI.format(ds=ds, models=tmp_path / tag, epochs=epochs, steps=(2, 3, 4), dropout="")
        if mix:
            text = text.replace("optimizer = Adam\n", "optimizer = Adam\nmixup_alpha = 0.4\ncutmix_alpha = 1.0\n")
            assert "cutmix_alpha" in text
        f = tmp_path / f"{tag}{'' if mix else '_off'}.ini"
        f.write_text(text)
        return str(f)

    R._seed_all(1234)
    train.main(A(ini("a", 2), None, None, None, None))
    out_a = capsys.readouterr().out
    R._seed_all(1234)
    train.main(A(ini("b", 1), None, None, None, None))
    out_b = capsys.readouterr().out
    dir_a, dir_b = tmp_path / "a" / "resnet18_1", tmp_path / "b" / "resnet18_1"
    mid = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert mid["epoch"] == 1 and mid["mix"] == BatchMix(0.4, 1.0).describe()
    fresh = BatchMix(0.4, 1.0, seed=42)                     # random_seed * world + rank
    assert mid["ranks"][0]["mix_rng"] != fresh.getstate()   # the generator moved during the epoch ...
    moved = BatchMix(0.4, 1.0, seed=42)
    moved.setstate(mid["ranks"][0]["mix_rng"])              # ... and its position loads
    with pytest.raises(ValueError, match=r"cannot resume: mix differs, train_state.pth has .*mixup_alpha 0.4.*the config gives off"):
        train.main(A(ini("b", 2, mix=False), None, None, None, str(dir_b)))
    capsys.readouterr()
    R._seed_all(777)
    train.main(A(ini("b", 2), None, None, None, str(dir_b)))
    out_c = capsys.readouterr().out
    assert "[ERROR]" not in out_a + out_b + out_c, out_c
    sa, sb, sc = R._stat_lines(out_a), R._stat_lines(out_b), R._stat_lines(out_c)
    assert sorted(sa) == [1, 2] and sorted(sb) == [1] and sorted(sc) == [2]
    assert sb[1] == sa[1] and sc[2] == sa[2], (sa, sb, sc)
    end_a = torch.load(dir_a / train.TRAIN_STATE_FILE, weights_only=True)
    end_c = torch.load(dir_b / train.TRAIN_STATE_FILE, weights_only=True)
    assert end_a["epoch"] == end_c["epoch"] == 2 and end_c["ended"]
    assert R._differing(end_a["net"], end_c["net"]) == []
    assert R._differing(torch.load(dir_a / "best_state.pth"), torch.load(dir_b / "best_state.pth")) == []
    assert end_a["book"] == end_c["book"] and end_a["mix"] == end_c["mix"]
    assert end_a["ranks"][0]["mix_rng"] == end_c["ranks"][0]["mix_rng"]
