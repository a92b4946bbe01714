"""`HipNet.set_loss` in the training and validation steps: the loss and dlogits a step leaves equal torch's on the
step's own logits within the kernel's bounds (tests/test_gpu_loss_ops.py), and a model whose loss was set and set back
is the model that never heard of it, bit for bit."""

import numpy as np
import pytest
import torch

import test_gpu_loss_ops as K
from sykepic_hip import arch, dp, synth
from sykepic_hip.optim import HipOptimizer

pytestmark = pytest.mark.gpu

CLASSES, N, HW = 5, 6, 32
WEIGHTS = [0.25, 4.0, 1.0, 0.05, 20.0]
SMOOTH = 0.1


def _net(seed=7):
    from sykepic_hip.net import HipNet
    g = arch.build_graph("resnet18", CLASSES)
    sd = synth.synth_state_dict(arch.param_specs(g), seed=seed, logit_gain=2.0)
    net = HipNet("resnet18", CLASSES, weights=None)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net, g


def _batch(s):
    return (torch.from_numpy(synth.synth_images(N, 3, HW, HW, seed=100 + s)).cuda(),
            torch.from_numpy(synth.synth_labels(N, CLASSES, seed=200 + s)).cuda())


def _check_step(net, logits, y, want_dz, what):
    """float64 torch on exactly the logits the step produced, under the bounds of the single-operator test."""
    z, labels = logits.cpu(), y.cpu()
    w = torch.tensor(WEIGHTS, dtype=torch.float32)
    eps = K._f32(SMOOTH)
    ref_loss, ref_dz = K._reference(z, labels, w, eps)
    dz_bound, loss_bound = K._bounds(z, labels, w, eps)
    loss_n, correct = net.read_stats()
    K.H._ratio(torch.tensor([loss_n]), torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1), f"{what} n*loss")
    want_counts, want_correct = K._counts_ref(z, labels)
    assert correct == want_correct
    assert torch.equal(net.read_class_counts(reset=True), want_counts)
    assert int(net.read_class_counts().sum()) == 0            # the read above reset them
    if want_dz:
        t = net.graph.ops[-1].dst
        K.H._ratio(net.read_activation_grad(t, N, (N, CLASSES)), ref_dz, dz_bound, f"{what} dlogits")


def test_train_and_eval_steps_use_the_set_loss():
    net, _ = _net()
    x, y = _batch(0)
    net.set_loss(WEIGHTS, SMOOTH)
    net.train()
    net.reset_stats()
    logits = net.forward_backward(x, y, want_logits=True)
    _check_step(net, logits, y, True, "train step")
    net.eval()
    net.reset_stats()
    logits = net.eval_step(x, y, want_logits=True)
    _check_step(net, logits, y, False, "eval step")
    # label smoothing alone (no weights) also counts; the plain loss keeps no counters and says so
    net.set_loss(None, SMOOTH)
    net.reset_stats()
    net.eval_step(x, y)
    assert int(net.read_class_counts()[:, 0].sum()) == N
    net.set_loss()
    with pytest.raises(RuntimeError, match="default loss keeps no per-class counters"):
        net.read_class_counts()


def test_set_loss_refuses_bad_arguments():
    net, _ = _net()
    for bad in ([1.0, 0.0, 1.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0, 1.0],
                [1.0, float("inf"), 1.0, 1.0, 1.0]):
        with pytest.raises(RuntimeError, match="model_set_loss: weight of class 1"):
            net.set_loss(bad, 0.0)
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="label_smoothing"):
            net.set_loss(None, eps)
    with pytest.raises(ValueError, match="4 entries"):
        net.set_loss([1.0] * 4, 0.0)
    with pytest.raises(RuntimeError, match="no per-class counters"):      # nothing was set by the refused calls
        net.read_class_counts()


def test_default_loss_is_untouched_by_set_and_reset():
    """A never calls set_loss; B calls set_loss(w, 0.1), then set_loss(None, 0.0) before its first step.  Two steps
    (Adam) later their statistics and their flat gradient buffers are equal bit for bit."""
    def run(touch):
        net, _ = _net()
        if touch:
            net.set_loss(WEIGHTS, SMOOTH)
            net.set_loss(None, 0.0)
        params = list(net.parameters())
        for p in params:
            p.requires_grad = True
        opt = HipOptimizer(net, "Adam", [{"params": params, "lr": 0.01}])
        net.train()
        net.reset_stats()
        for s in range(2):
            net.forward_backward(*_batch(s))
            if s == 0:
                opt.step()
        ptr, numel = net.grad_buffer()
        flat = torch.as_tensor(dp._DevicePtr(ptr, numel), device=net.device).clone()
        return torch.tensor(net.read_stats()), flat.cpu()

    stats_a, flat_a = run(False)
    stats_b, flat_b = run(True)
    assert float(flat_a.abs().max()) > 0
    assert torch.equal(stats_a, stats_b) and torch.equal(flat_a, flat_b)
