"""`HipNet.forward_backward(..., teacher_logits=, distill_alpha=, distill_temperature=)`: the distilled training step.
ResNet-18, 5 classes, 6 images of 32 x 32, with the helpers of test_gpu_loss_model.py.

- On the step's own logits the loss, the distillation statistics and dlogits equal float64 torch within the bounds of the
  single-operator test (tests/test_gpu_distill_ops.py).
- No teacher, or alpha = 0, is the step that never heard of a teacher, bit for bit (plain and two-label).
- Two live library handles on one device and stream: teacher forwards interleaved with student steps change neither.
- It learns: the KD term of a fixed batch falls under SGD at alpha = 1.  lr = 0.01 and 4 steps were chosen on the CPU:
  the float64 `oracle/` model (RefNet, train-mode BatchNorm, every parameter trainable, the teacher a RefNet of another
  seed in eval mode, T = 2) gives KD = 0.0351, 0.0174, 0.0097, 0.0056 at the four steps - the last below half the first.
"""

import numpy as np
import pytest
import torch

import test_gpu_distill_ops as D
import test_gpu_loss_model as M
import test_gpu_loss_ops as K
from sykepic_hip import dp
from sykepic_hip.optim import HipOptimizer

pytestmark = pytest.mark.gpu

N, CLASSES = M.N, M.CLASSES
ALPHA, T = float(np.float32(0.3)), 2.0


def _teacher(seed=11):
    net, _ = M._net(seed)
    return net.eval()


def _all_trainable(net, name, lr):
    params = list(net.parameters())
    for p in params:
        p.requires_grad = True
    return HipOptimizer(net, name, [{"params": params, "lr": lr}])


def _flat_grad(net):
    ptr, numel = net.grad_buffer()
    return torch.as_tensor(dp._DevicePtr(ptr, numel), device=net.device).clone().cpu()


@pytest.mark.parametrize("pair", [False, True], ids=["one-label", "two-labels"])
@pytest.mark.parametrize("loss", ["default", "weighted"])
def test_step_against_float64_on_its_own_logits(loss, pair):
    net, _ = M._net()
    teacher = _teacher()
    x, y = M._batch(0)
    w, eps = None, 0.0
    if loss != "default":
        net.set_loss(M.WEIGHTS, M.SMOOTH)
        w, eps = torch.tensor(M.WEIGHTS, dtype=torch.float32), K._f32(M.SMOOTH)
    y2, lam = (y.roll(1), D.LAM) if pair else (None, 1.0)
    t = teacher.forward(x)
    net.train()
    net.reset_stats()
    logits = net.forward_backward(x, y, want_logits=True, y2=y2, lam=lam, teacher_logits=t, distill_alpha=ALPHA,
                                  distill_temperature=T)
    z, tc, ya, yb = logits.cpu(), t.cpu(), y.cpu(), None if y2 is None else y2.cpu()
    ref_loss, ref_dz, ref_kd = D._reference(z, ya, yb, lam, tc, ALPHA, T, w, eps)
    dz_bound, loss_bound, kd_bound = D._bounds(z, ya, yb, lam, tc, ALPHA, T, w, eps)
    loss_n, correct = net.read_stats()
    kd_n, agree = net.read_distill_stats()
    what = f"distilled step {loss} {'pair' if pair else 'single'}"
    K.H._ratio(torch.tensor([loss_n]), torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1), f"{what} n*loss")
    K.H._ratio(torch.tensor([kd_n]), torch.tensor([ref_kd], dtype=torch.float64), kd_bound.reshape(1), f"{what} n*KD")
    dom = ya if yb is None else D.P._dominant(ya, yb, lam)
    assert correct == K._counts_ref(z, dom)[1]
    assert agree == D._agreement(z, tc)
    last = net.graph.ops[-1].dst
    K.H._ratio(net.read_activation_grad(last, N, (N, CLASSES)), ref_dz, dz_bound, f"{what} dlogits")
    net.reset_stats()
    assert net.read_stats() == (0.0, 0.0) and net.read_distill_stats() == (0.0, 0.0)


def test_bad_arguments_are_refused():
    net, _ = M._net()
    x, y = M._batch(0)
    t = torch.zeros((N, CLASSES), dtype=torch.float32, device="cuda")
    net.train()
    net.reset_stats()
    with pytest.raises(RuntimeError, match="alpha must be in"):
        net.forward_backward(x, y, teacher_logits=t, distill_alpha=1.5)
    with pytest.raises(RuntimeError, match="temperature must be"):
        net.forward_backward(x, y, teacher_logits=t, distill_alpha=0.5, distill_temperature=0.0)
    for bad in (t[:, :4], t.double(), t.cpu(), torch.zeros((N + 1, CLASSES), dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError, match="teacher_logits must be a contiguous float32"):
            net.forward_backward(x, y, teacher_logits=bad, distill_alpha=0.5)
    assert net.read_stats() == (0.0, 0.0) and net.read_distill_stats() == (0.0, 0.0)


@pytest.mark.parametrize("pair", [False, True], ids=["one-label", "two-labels"])
@pytest.mark.parametrize("loss", ["default", "weighted"])
def test_no_teacher_and_alpha_zero_are_the_step_of_today_bit_for_bit(loss, pair):
    """Twin models, two steps with an Adam step between them: `teacher_logits=None` (whatever alpha says) and
    `distill_alpha=0` (whatever the teacher holds) against the call without the arguments - equal statistics and flat
    gradient buffers, and no distillation statistics."""
    teacher_logits = torch.randn((N, CLASSES), generator=torch.Generator().manual_seed(3)).cuda()

    def run(how):
        net, _ = M._net()
        if loss != "default":
            net.set_loss(M.WEIGHTS, M.SMOOTH)
        opt = _all_trainable(net, "Adam", 0.01)
        net.train()
        net.reset_stats()
        for s in range(2):
            x, y = M._batch(s)
            kw = dict(y2=y.roll(1), lam=D.LAM) if pair else {}
            if how == "none":
                kw.update(teacher_logits=None, distill_alpha=0.7, distill_temperature=3.0)
            elif how == "alpha0":
                kw.update(teacher_logits=teacher_logits, distill_alpha=0.0, distill_temperature=3.0)
            net.forward_backward(x, y, **kw)
            if s == 0:
                opt.step()
        assert net.read_distill_stats() == (0.0, 0.0)
        return torch.tensor(net.read_stats()), _flat_grad(net)

    stats_a, flat_a = run("today")
    assert float(flat_a.abs().max()) > 0
    for how in ("none", "alpha0"):
        stats_b, flat_b = run(how)
        assert torch.equal(stats_a, stats_b) and torch.equal(flat_a, flat_b), how


def test_two_live_handles_do_not_disturb_each_other():
    """Run A interleaves `teacher.forward` with the student's steps (three steps, Adam between them), as the workflow
    does.  Run B takes the same steps on a twin student with the logits precomputed by a teacher that does nothing else.
    The student's statistics and flat gradient buffer, and the teacher's logits, are equal bit for bit; the teacher's
    tensors are what they were and it is still in eval mode."""
    batches = [M._batch(s) for s in range(3)]

    lone = _teacher()
    lone_logits = [lone.forward(x).clone() for x, _ in batches]
    del lone

    def run(interleaved):
        net, _ = M._net()
        opt = _all_trainable(net, "Adam", 0.01)
        teacher = _teacher() if interleaved else None
        before = {k: v.clone() for k, v in teacher.state_dict().items()} if interleaved else None
        buf = torch.empty((N, CLASSES), dtype=torch.float32, device="cuda")
        seen = []
        net.train()
        net.reset_stats()
        for s, (x, y) in enumerate(batches):
            if interleaved:
                t = teacher.forward(x, out=buf)
                seen.append(t.clone())
            else:
                t = lone_logits[s]
            net.forward_backward(x, y, teacher_logits=t, distill_alpha=ALPHA, distill_temperature=T)
            opt.step()
        out = (torch.tensor(net.read_stats() + net.read_distill_stats()), _flat_grad(net))
        if interleaved:
            after = teacher.state_dict()
            assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
            assert teacher.training is False
            assert all(torch.equal(a, b) for a, b in zip(seen, lone_logits)), "the teacher's logits moved beside a student"
        return out

    stats_a, flat_a = run(True)
    stats_b, flat_b = run(False)
    assert float(flat_a.abs().max()) > 0 and float(stats_a[2]) > 0
    assert torch.equal(stats_a, stats_b) and torch.equal(flat_a, flat_b)


def test_distiller_reuses_its_buffer_and_keeps_the_teacher_in_eval_mode():
    from sykepic_hip.distill import Distiller
    teacher = _teacher()
    d = Distiller(teacher, 0.5, 2.0)
    x0, x1 = M._batch(0)[0], M._batch(1)[0]
    want0, want1 = teacher.forward(x0).clone(), teacher.forward(x1).clone()
    a = d.logits(x0)
    assert torch.equal(a, want0)
    ptr = a.data_ptr()
    teacher.train()                      # someone flipped it: the next call puts it back
    b = d.logits(x1)
    assert b.data_ptr() == ptr and torch.equal(b, want1) and teacher.training is False
    assert tuple(d.logits(x0[:4]).shape) == (4, CLASSES)
    assert d.describe() == {"teacher": "resnet18", "teacher_sha256": "", "alpha": 0.5, "temperature": 2.0}


def test_it_learns_from_the_teacher():
    """One fixed batch, alpha = 1 (the labels carry no weight), SGD lr 0.01, every parameter trainable, four steps (chosen
    on the CPU, module docstring): the KD term of the last step is below that of the first."""
    net, _ = M._net()
    teacher = _teacher()
    opt = _all_trainable(net, "SGD", 0.01)
    x, y = M._batch(0)
    t = teacher.forward(x)
    net.train()
    kds = []
    for _ in range(4):
        net.reset_stats()
        net.forward_backward(x, y, teacher_logits=t, distill_alpha=1.0, distill_temperature=T)
        opt.step()
        kd_n, _ = net.read_distill_stats()
        loss_n, _ = net.read_stats()
        assert loss_n == kd_n                 # alpha = 1: the loss IS the distillation term (1 * KD + 0 * hard)
        kds.append(kd_n / N)
    print(f"[distill] KD over the steps: {[round(k, 5) for k in kds]}")
    assert all(np.isfinite(kds)) and kds[0] > 0
    assert kds[-1] < kds[0], kds
