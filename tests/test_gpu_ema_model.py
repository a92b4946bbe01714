"""The weights' moving average on a model (`HipNet.ema_*`, spk_model_ema_*): every update follows the oracle of
tests/ema_util.py on every float tensor, the average does not disturb training, a swap exchanges model and average and
rebuilds the packed images, training steps are refused while swapped in.

Bit for bit.  The float64 oracle is proven equal to the fused result on the seeded inputs of the operator test; on the
~11 M values of a trained model it can differ from it by double rounding, about once in 2^29 elements.  So an element
that differs from the oracle is checked against the exactly computed, once-rounded result instead (rational
arithmetic, `ema_util.correctly_rounded`) - the kernel's specification - and more than a handful of such elements
fails at once."""

import ctypes as C

import numpy as np
import pytest
import torch

import ema_util as U
import test_gpu_loss_model as M
from sykepic_hip import arch, dp, synth
from sykepic_hip.optim import HipOptimizer

pytestmark = pytest.mark.gpu

FROZEN = "base.0.weight"


def _floats(sd):
    return {k: v for k, v in sd.items() if v.dtype == torch.float32}


def _same_bits(a, b):
    return np.array_equal(U.bits(a.numpy()), U.bits(b.numpy()))


def _differing(a, b):
    assert list(a) == list(b)
    return [k for k in a if not (_same_bits(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k]))]


def _trainable(net, frozen=(FROZEN,)):
    params = list(net.parameters())
    for p in params:
        p.requires_grad = p.key not in frozen
    net.train()
    return HipOptimizer(net, "Adam", [{"params": [p for p in params if p.requires_grad], "lr": 0.01}])


def _follows_oracle(before, model, after, w, what):
    """after[k] == oracle(before[k], model[k], w) for every float tensor (see the module docstring for the exception)."""
    assert list(after) == list(before) == list(_floats(model))
    odd = 0
    for k in after:
        e, p, got = before[k].numpy().reshape(-1), model[k].numpy().reshape(-1), after[k].numpy().reshape(-1)
        bad = np.nonzero(U.bits(got) != U.bits(U.oracle(e, p, w)))[0]
        odd += bad.size
        assert odd <= 4, (what, k, bad.size, bad[:5], got[bad[:5]], U.oracle(e, p, w)[bad[:5]])
        for i in bad:
            assert U.correctly_rounded(e[i], p[i], w, got[i]), (what, k, int(i), e[i], p[i], got[i])


def _grad_flat(net):
    ptr, numel = net.grad_buffer()
    return torch.as_tensor(dp._DevicePtr(ptr, numel), device=net.device).clone().cpu()


def _mobilenet(seed=7):
    from sykepic_hip.net import HipNet
    g = arch.build_graph("mobilenet_v3_small", M.CLASSES)
    sd = synth.synth_state_dict(arch.param_specs(g), seed=seed, logit_gain=2.0)
    net = HipNet("mobilenet_v3_small", M.CLASSES, weights=None)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net


def test_updates_follow_the_oracle_and_do_not_disturb_training():
    net, _ = M._net()
    twin, _ = M._net()
    opt, twin_opt = _trainable(net), _trainable(twin)
    assert net.ema_state() == {"enabled": False, "swapped": False}
    net.ema_enable()
    assert net.ema_state() == {"enabled": True, "swapped": False}
    start = net.state_dict()
    avg = net.ema_state_dict()
    assert list(avg) == list(_floats(start)) and all(v.dtype == torch.float32 for v in avg.values())
    assert _differing(avg, _floats(start)) == []
    assert any(k.endswith("running_var") for k in avg) and not any(k.endswith("num_batches_tracked") for k in avg)
    net.reset_stats()
    twin.reset_stats()
    for s, w in enumerate(U.WEIGHTS):
        x, y = M._batch(s)
        net.forward_backward(x, y)
        opt.step()
        net.ema_update(w)
        twin.forward_backward(x, y)
        twin_opt.step()
        model, after = net.state_dict(), net.ema_state_dict()
        _follows_oracle(avg, model, after, w, f"step {s + 1}")
        assert _same_bits(after[FROZEN], start[FROZEN])             # a frozen tensor's average stays the tensor
        assert not _same_bits(after["base.1.running_mean"], avg["base.1.running_mean"])     # buffers are averaged too
        assert not _same_bits(after["base.1.weight"], model["base.1.weight"])               # ... and it IS an average
        avg = after
    # the twin never had an average: the same parameters, buffers, statistics and gradients, bit for bit
    assert _differing(net.state_dict(), twin.state_dict()) == []
    assert net.read_stats() == twin.read_stats()
    assert torch.equal(_grad_flat(net).view(torch.int32), _grad_flat(twin).view(torch.int32))
    assert int(net.state_dict()["base.1.num_batches_tracked"]) == 3


def test_updates_follow_the_oracle_on_mobilenet_v3():
    """Another flat layout: depthwise convs, squeeze-excitation weights and biases, a 16-channel stem."""
    net = _mobilenet()
    opt = _trainable(net, frozen=())
    net.ema_enable()
    avg = net.ema_state_dict()
    assert any(".fc1.bias" in k for k in avg)
    assert _differing(avg, _floats(net.state_dict())) == []
    for s, w in enumerate(U.WEIGHTS[:2]):
        x = torch.from_numpy(synth.synth_images(M.N, 3, 64, 64, seed=100 + s)).cuda()
        net.forward_backward(x, M._batch(s)[1])
        opt.step()
        net.ema_update(w)
        after = net.ema_state_dict()
        _follows_oracle(avg, net.state_dict(), after, w, f"mobilenet step {s + 1}")
        avg = after


def test_swap_exchanges_model_and_average():
    from sykepic_hip.net import HipNet
    net, _ = M._net()
    twin, _ = M._net()
    opt, twin_opt = _trainable(net), _trainable(twin)
    net.ema_enable()
    for s in range(2):
        x, y = M._batch(s)
        net.forward_backward(x, y)
        opt.step()
        net.ema_update(U.WEIGHTS[2])
        twin.forward_backward(x, y)
        twin_opt.step()
    model, avg = net.state_dict(), net.ema_state_dict()
    assert _differing(avg, _floats(model))                                     # there is something to exchange
    x, y = M._batch(5)
    net.eval()
    raw_logits = net.eval_step(x, y, want_logits=True).cpu()

    net.ema_swap()
    assert net.ema_state() == {"enabled": True, "swapped": True}
    swapped = net.state_dict()
    assert _differing(_floats(swapped), avg) == []                             # the model now IS the former average
    assert _differing(net.ema_state_dict(), _floats(model)) == []              # ... and the other buffer the former model
    nbt = [k for k in model if k.endswith("num_batches_tracked")]
    assert nbt and all(int(swapped[k]) == int(model[k]) == 2 for k in nbt)     # the model's own counters serve both
    # every packed image was rebuilt: a fresh net that loaded these tensors computes the same logits
    fresh = HipNet("resnet18", M.CLASSES, weights=None)
    fresh.load_state_dict(swapped)
    fresh.eval()
    avg_logits = net.eval_step(x, y, want_logits=True).cpu()
    assert torch.equal(avg_logits.view(torch.int32), fresh.eval_step(x, y, want_logits=True).cpu().view(torch.int32))
    assert not torch.equal(avg_logits, raw_logits)
    # no training on the average
    net.train()
    with pytest.raises(RuntimeError, match="moving average is swapped in"):
        net.forward_backward(*M._batch(2))
    with pytest.raises(RuntimeError, match="moving average is swapped in"):
        opt.step()
    with pytest.raises(RuntimeError, match="moving average is swapped in"):
        net.ema_update(0.1)
    with pytest.raises(RuntimeError, match="moving average is swapped in"):
        net.ema_enable()
    assert _differing(net.state_dict(), swapped) == []                         # the refused calls changed nothing

    net.ema_swap()
    assert net.ema_state() == {"enabled": True, "swapped": False}
    assert _differing(net.state_dict(), model) == [] and _differing(net.ema_state_dict(), avg) == []
    net.eval()
    assert torch.equal(net.eval_step(x, y, want_logits=True).cpu().view(torch.int32), raw_logits.view(torch.int32))
    # training goes on as if nothing had happened: one more step and update, then the model equals the twin's
    net.train()
    x2, y2 = M._batch(2)
    net.forward_backward(x2, y2)
    opt.step()
    net.ema_update(U.WEIGHTS[0])
    twin.forward_backward(x2, y2)
    twin_opt.step()
    assert _differing(net.state_dict(), twin.state_dict()) == []
    _follows_oracle(avg, net.state_dict(), net.ema_state_dict(), U.WEIGHTS[0], "after the swaps")
    # load_state_dict on a model that is not swapped in leaves the average alone; load_ema_state_dict sets it
    kept = net.ema_state_dict()
    net.load_state_dict(model)
    assert _differing(net.ema_state_dict(), kept) == []
    net.load_ema_state_dict(avg)
    assert _differing(net.ema_state_dict(), avg) == [] and _differing(net.state_dict(), model) == []
    # dropping a swapped-in average gives the model its own weights back
    net.ema_swap()
    net.ema_enable(False)
    assert net.ema_state() == {"enabled": False, "swapped": False}
    assert _differing(net.state_dict(), model) == []


def test_errors_and_disable():
    from sykepic_hip import lib
    net, _ = M._net()
    twin, _ = M._net()
    opt, twin_opt = _trainable(net), _trainable(twin)
    for call in (lambda: net.ema_update(0.1), net.ema_swap, net.ema_state_dict):
        with pytest.raises(RuntimeError, match="not enabled"):
            call()
    net.ema_enable(False)                                                      # nothing to drop: fine
    net.ema_enable()
    for w in (0.0, 1.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"w must be finite and inside \(0, 1\)"):
            net.ema_update(w)
    # the C entry points' own refusals, with a handle: an int64 key, an unknown key, a wrong size
    so, h = lib.load(), net._h
    buf = np.zeros((64, 3, 7, 7), np.float32)
    p = C.c_void_p(buf.ctypes.data)
    ARG, KEY = -1, -3
    for fn in (so.spk_model_ema_read, so.spk_model_ema_load):
        assert fn(h, b"base.1.num_batches_tracked", p, 1) == ARG and b"int64" in so.spk_last_error()
        assert fn(h, b"no.such.key", p, 1) == KEY
        assert fn(h, b"base.0.weight", p, buf.size - 1) == ARG
        assert fn(h, b"base.0.weight", None, buf.size) == ARG
        assert fn(h, None, p, buf.size) == ARG
    x, y = M._batch(0)
    net.forward_backward(x, y)
    opt.step()
    net.ema_update(0.25)
    net.ema_enable(False)
    assert net.ema_state() == {"enabled": False, "swapped": False}
    with pytest.raises(RuntimeError, match="not enabled"):
        net.ema_update(0.25)
    twin.forward_backward(x, y)
    twin_opt.step()
    x, y = M._batch(1)                                                         # ... and the model trains on as before
    net.forward_backward(x, y)
    opt.step()
    twin.forward_backward(x, y)
    twin_opt.step()
    assert _differing(net.state_dict(), twin.state_dict()) == []
    net.ema_enable()                                                           # enabled again: a copy of the model as it is now
    assert _differing(net.ema_state_dict(), _floats(net.state_dict())) == []
