"""MobileNetV3 Large / Small on the MI355X path: the Hardswish / ReLU depthwise kernels, inference against the fp32
restatement of torchvision's model (tests/mobilenet_ref.py), the training backward against torch autograd at the GPU's
operating point, a training run, trained-net parity in the eval modes, and the fp8 refusal."""

import numpy as np
import pytest
import torch

from sykepic_hip import arch, synth

pytestmark = pytest.mark.gpu
PROB_TOL = 1e-3
BOUND = 4e-2
NETS = ("mobilenet_v3_large", "mobilenet_v3_small")


def _state(network, classes, seed, logit_gain=2.0):
    g = arch.build_graph(network, classes)
    specs = arch.param_specs(g)
    sd = synth.synth_state_dict(specs, seed=seed, logit_gain=logit_gain)
    return g, specs, {k: torch.from_numpy(np.asarray(v)).clone() for k, v in sd.items()}


def _hipnet(network, classes, state, **kw):
    from sykepic_hip.net import HipNet
    net = HipNet(network, classes, weights=None, **kw)
    net.load_state_dict(state)
    return net


def _calibrated(network, classes, seed, hw):
    """Synthetic weights whose BatchNorm running statistics are the batch statistics of generator-seeded images (a random
    net's stored statistics do not describe its activations)."""
    from mobilenet_ref import TorchVisionNet, load
    g, specs, state = _state(network, classes, seed)
    ref = load(TorchVisionNet(network, classes), state)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = None   # cumulative average: one batch sets the statistics
            mod.reset_running_stats()
    ref.train()
    with torch.no_grad():
        ref(torch.from_numpy(synth.synth_images(16, 3, hw, hw, seed=99)))
    ref.eval()
    return g, {k: v.clone() for k, v in ref.state_dict().items()}, ref


@pytest.mark.parametrize("case", [(2, 16, 112, 112, 3, 1), (3, 16, 57, 45, 3, 2), (2, 72, 56, 56, 3, 1),
                                  (2, 96, 23, 29, 5, 2), (4, 240, 14, 14, 5, 1), (3, 480, 15, 13, 3, 1),
                                  (2, 960, 7, 7, 5, 1), (5, 576, 9, 11, 5, 2)])
def test_depthwise_relu_and_hardswish_match_torch(case):
    """Depthwise KxK conv + folded BN + ReLU / Hardswish on both kernels against F.conv2d(groups=C) on the same fp16
    input, with the tolerances of the SiLU test (tests/test_gpu_effnet.py): 2e-3 of the tensor maximum, pool sums 1e-4."""
    import torch.nn.functional as F
    from sykepic_hip import ops
    n, c, h, w, k, s = case
    g = torch.Generator().manual_seed(c + h)
    x = (torch.randn((n, c, h, w), generator=g)).half()
    wt = torch.randn((c, 1, k, k), generator=g) * (1.0 / k)
    sc = torch.rand(c, generator=g) + 0.5
    bi = torch.randn(c, generator=g) * 0.3
    v = F.conv2d(x.float(), wt, None, s, (k - 1) // 2, groups=c) * sc.view(1, -1, 1, 1) + bi.view(1, -1, 1, 1)
    for act, want in ((arch.ACT_RELU, F.relu(v)), (arch.ACT_HSWISH, F.hardswish(v))):
        for lds in (1, 0):
            try:
                y, pool = ops.dwconv(x.cuda(), wt.cuda(), sc.cuda(), bi.cuda(), k, s, act=act, lds=lds)
            except RuntimeError as e:
                assert lds == 1 and "cannot run this shape" in str(e), e   # (the LDS ring has no plan for every shape)
                continue
            y, pool = y.float().cpu(), pool.cpu()
            assert torch.isfinite(y).all(), "unwritten outputs"
            err = float((y - want).abs().max() / want.abs().max())
            perr = float((pool - want.sum((2, 3))).abs().max() / want.sum((2, 3)).abs().max())
            print(f"dwconv {case} act={act} lds={lds}: max error / max {err:.2e}, pool {perr:.2e}")
            assert err < 2e-3 and perr < 1e-4


@pytest.mark.parametrize("network", NETS)
def test_inference_matches_the_restatement_on_fresh_images(network):
    """Eval forward (fp16 storage, default mode) against the fp32 restatement on fresh images at 224 and at 180 (odd maps
    45 / 23 / 12 ...), 16 images each: per-image logit rms error / logit std, and probabilities at the reference's base
    1.3.  Measured (MI355X, default mode = hi + lo weights on every conv of these graphs): logit rms error / std median
    6.2e-4 ... 1.4e-3, max 1.7e-3 ... 3.3e-3; max |dp| median 1.3e-6 ... 2.8e-6, max <= 6.6e-6 (this synthetic net's logits
    have std 0.13-0.18, so its probabilities are flat); top-1 16 / 16 everywhere.  Bounds: median 5e-3, max 2e-2 (4-6x);
    |dp| median 1e-3, p90 3e-3; top-1 >= 0.9.  The steep-softmax check is the golden test below."""
    from mobilenet_ref import probabilities
    classes = 50
    for hw in (224, 180):
        g, state, ref = _calibrated(network, classes, 2, hw)
        net = _hipnet(network, classes, state).eval()
        x = torch.from_numpy(synth.synth_images(16, 3, hw, hw, seed=21 + hw))
        z = probabilities(ref, x, base=0).numpy()
        zg = net.forward(x.cuda()).cpu().numpy()
        per_img = np.sqrt(np.mean((zg - z) ** 2, 1)) / z.std()
        pr = probabilities(ref, x).numpy()
        pg = net.probabilities(x.cuda()).cpu().numpy()
        dp = np.abs(pg - pr).max(1)
        print(f"{network}@{hw}: logit std {z.std():.2f}; logit rms error / std median {np.median(per_img):.2e} max "
              f"{per_img.max():.2e}; max|dp| median {np.median(dp):.2e} max {dp.max():.2e}; top-1 "
              f"{(pg.argmax(1) == pr.argmax(1)).mean():.3f}")
        assert np.median(per_img) < 5e-3 and per_img.max() < 2e-2
        assert np.median(dp) <= PROB_TOL and np.percentile(dp, 90) <= 3 * PROB_TOL
        assert (pg.argmax(1) == pr.argmax(1)).mean() >= 0.9


@pytest.mark.parametrize("network", NETS)
def test_probabilities_match_the_reference_golden(golden_dir, network):
    """net_pass of the reference's own TorchVisionNet (tests/golden/make_golden_mobilenet.py: base = [features, avgpool],
    head width read off classifier[0]) on 8 ROIs at 224 with logits of a trained classifier's spread (std ~4): max |dp|
    <= 1e-3, top-1 identical where the reference's margin exceeds 2e-3, ROI order as net_pass sorts it.  Measured: max |dp|
    6.6e-4 (large), 5.7e-4 (small)."""
    from mobilenet_ref import TorchVisionNet, load
    from oracle import refnet
    from sykepic_hip.prob import net_pass
    gold = np.load(golden_dir / "net_pass_mobilenet.npz")
    tag = f"{network}_224"
    gain = {"mobilenet_v3_large": 85.0, "mobilenet_v3_small": 50.0}[network]   # as the generator
    g = arch.build_graph(network, 50)
    sd = synth.synth_state_dict(arch.param_specs(g), seed=2, logit_gain=gain)
    ref = load(TorchVisionNet(network, 50), {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    refnet.calibrate_bn(ref, torch.from_numpy(synth.synth_images(16, 3, 224, 224, seed=99)))
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    last = [k for k in state if k.startswith("head.") and k.endswith(".bias")][-1]
    state[last] = state[last] + torch.from_numpy(gold[f"{tag}_bias_adj"])
    net = _hipnet(network, 50, state).eval()
    n = len(gold[f"{tag}_rois_in"])
    x = torch.from_numpy(synth.synth_images(n, 3, 224, 224, seed=0))
    paths = [f"/x/D20180712T065600_IFCB114_{int(r):05d}.png" for r in gold[f"{tag}_rois_in"]]
    half = n // 2
    res = net_pass(net, [(x[:half].cuda(), paths[:half]), (x[half:].cuda(), paths[half:])], "cuda:0")
    assert [r for r, _ in res] == gold[f"{tag}_rois_out"].tolist()
    p = np.array([q for _, q in res], dtype=np.float64)
    want = gold[f"{tag}_probs"].astype(np.float64)
    err = np.abs(p - want).max()
    zerr = np.abs(net.forward(x.cuda()).cpu().numpy() - gold[f"{tag}_logits"]).max()
    print(f"{tag}: max |dp| vs reference golden = {err:.2e}, max |dlogit| {zerr:.2e}")
    assert err <= PROB_TOL
    top2 = np.sort(want, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2 * PROB_TOL
    assert decided.sum() >= 3
    assert (p.argmax(1)[decided] == want.argmax(1)[decided]).all()


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.mark.parametrize("network", NETS)
def test_backward_matches_teacher_forced_autograd(network):
    """Every backward kernel of the graph (Hardswish / ReLU BatchNorm backward, depthwise data and weight gradients at
    16 ... 960 channels, the ReLU / Hardsigmoid gate, the 16-channel stem) at the GPU's own operating point: the
    restatement's train-mode forward with every activation overwritten (straight through) by what the GPU produced, then
    torch autograd.  Head gradients <= 1e-3 relative L2, every other gradient <= 4e-2."""
    import torch.nn.functional as F
    from mobilenet_ref import run, run_train_forced
    classes, n, hw = 10, 8, 64
    g, specs, state = _state(network, classes, seed=5)
    net = _hipnet(network, classes, state)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11))
    net.train()
    net.reset_stats()
    net.forward_backward(x.cuda(), y.cuda())
    kinds = {k: kind for k, _, kind in specs}
    shapes = {t: tuple(v.shape) for t, v in run(g, state, x, train=True).items()}
    forced = {op.dst: net.read_activation(op.dst, n, shapes[op.dst]) for op in g.ops}
    tsd = {k: v.clone().requires_grad_(v.dtype == torch.float32 and kinds[k] not in ("bn_mean", "bn_var"))
           for k, v in state.items()}
    acts = run_train_forced(g, tsd, x, forced)
    leaf = {}
    for t, v in acts.items():
        if t != 0 and v.requires_grad:
            v.retain_grad()
            leaf[t] = v
    loss = F.cross_entropy(acts[g.ops[-1].dst], y)
    loss.backward()
    lv = float(loss.detach())
    assert abs(net.read_stats()[0] / n - lv) < 1e-4 * max(1.0, lv)
    closing = {op.bn + ".bias" for op in g.ops if op.kind == arch.OP_CONV and int(op.relu) == arch.ACT_NONE}
    table = []
    for k, _, kind in specs:
        if tsd[k].grad is None:
            continue
        got = net._read_grad(k, tuple(tsd[k].shape))
        if k in closing:
            # a block-closing BatchNorm's bias feeds only 1x1 conv -> train-mode BatchNorm (which removes per-channel
            # constants) where no depthwise conv reads the trunk directly: its exact gradient is 0 and autograd returns
            # rounding noise.  Then the error is held against the gradient of the same layer's weight.
            scale = float(tsd[k[:-4] + "weight"].grad.norm())
            if float(tsd[k].grad.norm()) < 0.1 * scale:
                err = float((got.double() - tsd[k].grad.double()).norm())
                assert err < 0.1 * scale, (k, err, scale)
                continue
        r = _rel(got, tsd[k].grad)
        if k.startswith("head."):
            assert r < 1e-3, f"{k}: {r:.3e}"
            continue
        table.append((k, r))
    for op in g.ops:
        t = op.src
        if t == 0 or t not in leaf or leaf[t].grad is None:
            continue
        got = net.read_activation_grad(t, n, shapes[t])
        table.append((f"d/d input of {op.name or op.kind}", _rel(got, leaf[t].grad)))
    worst = max(table, key=lambda kr: kr[1])
    print(f"{network}@{hw}x{n}: worst gradient {worst[1]:.3e} at {worst[0]}")
    import os
    if os.environ.get("SPK_TEST_VERBOSE"):
        for k, r in table:
            print(f"   {r:.3e}  {k}")
    # Measured (64^2, batch 8; SPK_TEST_VERBOSE=1 prints every value): the activation gradients grow smoothly from 7e-3
    # behind the head to 6e-2 at the first block (bf16 gradient storage random-walks through ~45 stored tensors; the
    # BatchNorms of the 2x2 / 4x4 maps see 32-128 values per channel), no jump at any layer.  Behind the last stride-2 block
    # every gradient keeps the 4e-2 bound; the earlier layers are held to 0.1 (worst 8.2e-2).  The BatchNorm of a layer
    # whose output a depthwise conv reads (stem, expand convs): depthwise conv -> train-mode BatchNorm removes any
    # per-channel scale and shift, and ReLU / Hardswish are nearly homogeneous, so its exact gradients are sums that
    # nearly cancel (worst 0.12 large, 0.19 small) - held to 0.25.
    feeds_dw = {op.bn for op in g.ops if op.kind in (arch.OP_CONV, arch.OP_DWCONV)
                and any(q.kind == arch.OP_DWCONV and q.src == op.dst for q in g.ops)}
    last_s2 = max(i + 1 for i, row in enumerate(arch._MOBILENETS[network][0]) if row[-1] == 2)

    def bound(k):
        name = k.replace("d/d input of ", "")
        if name.rsplit(".", 1)[0] in feeds_dw:
            return 0.25
        if not name.startswith("base.0."):
            return BOUND
        return BOUND if int(name.split(".")[2]) > last_s2 else 0.1

    bad = [(k, r) for k, r in table if r >= bound(k)]
    assert not bad, bad[:8]
    # ... and no jump: from the head towards the stem, the error of each activation gradient stays within 2x (+ 5e-3) of
    # the largest one behind it (measured: at most 1.9x at the step from a block's gate input to its depthwise input)
    acts = [(k, r) for k, r in table if k.startswith("d/d input of ")][::-1]
    seen = 0.0
    for k, r in acts:
        assert r <= 2.0 * seen + 5e-3 or seen == 0.0, (k, r, seen)
        seen = max(seen, r)


@pytest.mark.parametrize("network", NETS)
def test_forward_train_mode_matches_the_interpreter_layer_by_layer(network):
    """Train-mode forward of every layer from the GPU's own input (batch statistics, Hardswish / ReLU, gates, residual
    adds): <= 6e-3 relative L2 (bf16 storage)."""
    from mobilenet_ref import run
    classes, n, hw = 10, 8, 64
    g, specs, state = _state(network, classes, seed=7)
    net = _hipnet(network, classes, state)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=3))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=4))
    net.train()
    net.forward_backward(x.cuda(), y.cuda())
    shapes = {t: tuple(v.shape) for t, v in run(g, state, x, train=True).items()}
    got = {0: x}
    got.update({op.dst: net.read_activation(op.dst, n, shapes[op.dst]) for op in g.ops})
    worst = ("", 0.0)
    for op in g.ops:
        if op.kind in (arch.OP_LINEAR, arch.OP_GAVGPOOL):
            continue
        want = _one_layer(op, state, got)
        r = _rel(got[op.dst], want)
        if r > worst[1]:
            worst = (op.name, r)
        assert r < 6e-3, (op.name, r)
    print(f"{network}: worst train-mode layer {worst[1]:.2e} at {worst[0]}")


def _one_layer(op, state, acts):
    """One train-mode layer of the interpreter on the GPU's own operands (source and shortcut)."""
    import torch.nn.functional as F
    from mobilenet_ref import EPS, _act, _gate
    a = acts[op.src]
    if op.kind == arch.OP_SE:
        return _gate(a, op, state)
    groups = op.cin if op.kind == arch.OP_DWCONV else 1
    y = F.conv2d(a, state[op.name + ".weight"], None, op.stride, op.pad, groups=groups)
    y = F.batch_norm(y, None, None, state[op.bn + ".weight"], state[op.bn + ".bias"], True, 0.1, EPS)
    if op.res >= 0:
        y = y + acts[op.res]
    return _act(y, op.relu)


def test_training_reduces_the_loss_and_round_trips_the_state():
    """A few Adam steps on a fixed batch: the loss goes down, every trainable tensor moves, the state_dict round-trips
    into the eval path and the restatement."""
    from mobilenet_ref import TorchVisionNet, load, probabilities
    from sykepic_hip.optim import HipOptimizer
    classes, n, hw = 6, 16, 64
    network = "mobilenet_v3_small"
    g, specs, state = _state(network, classes, seed=3)
    net = _hipnet(network, classes, state)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=21))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=22))
    opt = HipOptimizer(net, "Adam", [{"params": list(net.parameters()), "lr": 2e-3}])
    losses = []
    net.train()
    for _ in range(12):
        net.reset_stats()
        net.forward_backward(x.cuda(), y.cuda())
        opt.step()
        losses.append(net.read_stats()[0] / n)
    assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[0], losses
    after = net.state_dict()
    trainable = [k for k, _, kind in specs if kind not in ("bn_mean", "bn_var", "bn_nbt")]
    moved = [k for k in trainable if not torch.equal(state[k], after[k])]
    assert len(moved) == len(trainable), sorted(set(trainable) - set(moved))[:5]
    assert int(after["base.0.0.1.num_batches_tracked"]) == 12
    ref = load(TorchVisionNet(network, classes), after)
    net.eval()
    p = net.probabilities(x.cuda()).cpu()
    assert float((p - probabilities(ref, x)).abs().max()) <= 2 * PROB_TOL


@pytest.mark.parametrize("network", NETS)
def test_trained_net_parity_in_the_eval_modes(network):
    """The headline check: trained with the HIP path for 300 Adam steps on the separable labelled set of
    tests/test_gpu_trained.py, then the default eval mode and the calibrated single pass against the fp32 restatement on
    256 fresh images: max |dp| <= 1e-3, top-1 identical on every decided image."""
    from mobilenet_ref import TorchVisionNet, load, probabilities
    from sykepic_hip import lib
    from test_gpu_trained import CLASSES, labelled_images, train_hip
    net, acc = train_hip(network, 300, 1e-3, seed=11)
    # torchvision builds MobileNetV3 with BatchNorm momentum 0.01: the running statistics average over ~100 steps, so the 30
    # steps without an update at the end of train_hip leave them describing weights Adam has moved on from (chance accuracy
    # in eval mode, in the fp32 restatement too).  Settle them on the final weights at momentum 0.1 first.
    lib.check(net._lib.spk_model_set_bn(net._h, arch.bn_params(network)[0], 0.1))
    net.train()
    for s in range(60):
        xs, ys = labelled_images(64, 20_000 + s)
        net.reset_stats()
        net.forward_backward(xs.cuda(), ys.cuda())
    lib.check(net._lib.spk_model_set_bn(net._h, *arch.bn_params(network)))
    net.eval()
    ref = load(TorchVisionNet(network, CLASSES, head=(64, 32)), net.state_dict())
    x, y = labelled_images(256, 77)
    pr = probabilities(ref, x).numpy().astype(np.float64)
    ref_acc = float((pr.argmax(1) == y.numpy()).mean())
    print(f"{network} trained 300 steps: train accuracy {acc:.3f}, restatement accuracy on fresh images {ref_acc:.3f}")
    assert acc > 0.8 and ref_acc > 0.7
    top2 = np.sort(pr, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2 * PROB_TOL

    def check(label):
        p = net.probabilities(x.cuda()).cpu().numpy().astype(np.float64)
        d = np.abs(p - pr).max(1)
        same = p.argmax(1) == pr.argmax(1)
        print(f"  {label:12s} max |dp| {d.max():.2e}  p90 {np.percentile(d, 90):.2e}  median {np.median(d):.2e}  "
              f"top-1 decided {same[decided].mean():.3f} ({int(decided.sum())})")
        assert d.max() <= PROB_TOL and same[decided].all(), label

    # Measured (worst of 256 images, run to run): default mode (on MobileNetV3 graphs hi + lo weights on every conv)
    # large 3.4e-4 ... 5.8e-4, small 2.6e-4 ... 3.5e-4.  With one fp16 product per conv the large net read 7.1e-4 ... 1.06e-3
    # and the calibrated mode 5.3e-4 ... 1.05e-3 (small: 2.9e-4 ... 4.5e-4): that mode does not hold the tolerance on this
    # family and is refused.
    net.set_precision(split_weights=3)
    check("mixed")
    net.calibrate(labelled_images(64, 5555)[0].cuda())
    with pytest.raises(RuntimeError, match="calibrated"):
        net.set_precision("calibrated")
    net.set_precision(split_weights=3)
    check("mixed again")


def test_fp8_is_refused():
    network = "mobilenet_v3_small"
    g, specs, state = _state(network, 10, seed=1)
    net = _hipnet(network, 10, state).eval()
    with pytest.raises(RuntimeError, match="fp8"):
        net.set_fp8(True, calibration_batch=torch.from_numpy(synth.synth_images(2, 3, 64, 64, seed=0)).cuda())


def test_local_torchvision_checkpoint_loads(tmp_path):
    """`weights = <local mobilenet_v3_*.pth>` (torchvision layout) loads into `base`; the classifier is dropped."""
    from mobilenet_ref import MobileNetV3
    from sykepic_hip.net import HipNet
    network = "mobilenet_v3_large"
    torch.manual_seed(0)
    tv = MobileNetV3(network)
    path = tmp_path / "mobilenet_v3_large-local.pth"
    torch.save(tv.state_dict(), path)
    net = HipNet(network, 10, weights=str(path))
    sd = net.state_dict()
    for k, v in tv.state_dict().items():
        nk = arch.backbone_key(network, k)
        if nk is not None:
            assert torch.equal(sd[nk], v), nk


def test_train_and_prob_workflows_end_to_end(tmp_path, capsys, golden_dir):
    """`sykepic train` with `network = mobilenet_v3_small` (the test_gpu_workflows.py setup: 3 synthetic classes, 8 epochs
    through the unfreeze schedule), then `sykepic prob` on the directory it wrote.  The best_state.pth loads into the
    restatement; no act_means.pth is written (these graphs have no calibrated mode), so `prob` runs the default mode
    without a warning and its CSV is within 1e-3 (+ the 5 printed decimals) of the restatement on the same ROIs."""
    import logging
    import random
    import shutil
    from collections import namedtuple
    from configparser import ConfigParser
    from PIL import Image
    from mobilenet_ref import TorchVisionNet, load, probabilities
    from sykepic_hip import ifcb, prob, train
    from sykepic_hip.config import get_img_shape, get_transforms
    from test_gpu_workflows import INI, Args
    network = "mobilenet_v3_small"
    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    rng = np.random.RandomState(0)
    ds = tmp_path / "ds"
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
    ini = tmp_path / "train.ini"
    ini.write_text(INI.format(ds=ds, models=tmp_path / "models", network=network))
    train.main(namedtuple("A", "config collage dist save_images")(str(ini), None, None, None))
    out = capsys.readouterr().out
    assert "[ERROR]" not in out, out
    mdir = tmp_path / "models" / f"{network}_1"
    for f in ("config.ini", "class_names.txt", "best_state.pth", "test_report.txt"):
        assert (mdir / f).is_file(), f
    losses = [float(s.split("Train Loss: ")[1]) for s in out.splitlines() if s.startswith("[STAT] Train")]
    assert len(losses) == 8 and all(np.isfinite(losses)), losses
    assert not (mdir / prob.ACT_MEANS_FILE).exists()
    sd = torch.load(mdir / "best_state.pth")
    ref = load(TorchVisionNet(network, 3, head=(32, 16)), sd)
    assert int(sd["base.0.0.1.num_batches_tracked"]) > 0
    # `sykepic prob` on the reference's raw fixture with this model directory
    raw = tmp_path / "raw" / "valid"
    raw.mkdir(parents=True)
    for ext in ("adc", "hdr", "roi"):
        shutil.copy(golden_dir / "ref_data" / f"D20180712T065600_IFCB114.{ext}", raw)
    out_dir = tmp_path / "out"
    logger = logging.getLogger("sykepic_hip")
    seen = []
    handler = logging.Handler(level=logging.WARNING)
    handler.emit = lambda rec: seen.append(rec.getMessage())
    logger.addHandler(handler)
    try:
        prob.call(Args(raw=str(raw), samples=None, image_dir=None, images=None, model=str(mdir), out=out_dir,
                       batch_size=64, num_workers=0, force=False))
    finally:
        logger.removeHandler(handler)
    assert not seen, seen
    csvs = list(out_dir.glob("**/*.csv"))
    assert len(csvs) == 1
    lines = csvs[0].read_text().splitlines()
    assert lines[0] == "roi," + ",".join((mdir / "class_names.txt").read_text().splitlines())
    cfg = ConfigParser()
    cfg.read(mdir / "config.ini")
    _, ev = get_transforms(cfg, get_img_shape(cfg))
    rois = ifcb.read_rois(raw / "D20180712T065600_IFCB114.adc", raw / "D20180712T065600_IFCB114.roi")
    x = torch.stack([ev(np.repeat(img[:, :, None], 3, axis=2)) for _, img in rois])
    want = probabilities(ref, x).numpy()
    got = np.array([[float(v) for v in ln.split(",")[1:]] for ln in lines[1:]])
    assert [int(ln.split(",")[0]) for ln in lines[1:]] == [2, 3]
    err = np.abs(got - want).max()
    print(f"{network} trained by train.main, prob CSV vs restatement: max |dp| {err:.2e}")
    assert err <= 1e-3 + 5e-6
