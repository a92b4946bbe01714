"""Parity of the HIP training step (through the C-ABI) with the oracle's
torch fp32 autograd, and with the golden vectors the reference's own
train_net produced.  bf16 activations/gradients vs fp32: tolerances are
relative L2 per tensor (stated at each check)."""

import numpy as np
import pytest
import torch

from sykepic_hip import arch, schedule, synth
from sykepic_hip.optim import HipOptimizer

pytestmark = pytest.mark.gpu


def _pair(network, classes, seed, gain=2.0):
    from oracle import refnet
    from sykepic_hip.net import HipNet
    g = arch.build_graph(network, classes)
    specs = arch.param_specs(g)
    sd = synth.synth_state_dict(specs, seed=seed, logit_gain=gain)
    ref = refnet.load_numpy_state(refnet.RefNet(network, classes), sd)
    net = HipNet(network, classes, weights=None)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return g, specs, ref, net


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _torch_state(ref):
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _fp32_autograd(g, specs, state, x, y):
    """{key: gradient} of the reference's pure-fp32 train-mode forward + mean CE (torch autograd)."""
    import torch.nn.functional as F
    from oracle import graph_eval
    kinds = {k: kind for k, _, kind in specs}
    tsd = {k: v.clone().requires_grad_(v.dtype == torch.float32 and kinds[k] not in ("bn_mean", "bn_var"))
           for k, v in state.items()}
    acts = graph_eval.run(g, tsd, x, train=True)
    out = acts[g.ops[-1].dst]
    loss = F.cross_entropy(out, y)
    loss.backward()
    return out.detach(), float(loss.detach()), {k: t.grad for k, t in tsd.items() if t.grad is not None}


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("network,hw,n", [("resnet18", 64, 8), ("resnet50", 64, 6), ("resnet18", 75, 5),
                                          ("resnet50", 96, 16), ("resnet34", 64, 4)])
def test_backward_matches_the_bf16_emulating_oracle(network, hw, n):
    """Whole-network check of every backward kernel at the GPU's own operating point.
    oracle.graph_eval.train_step_bf16 restates the training step with a bf16 rounding exactly where the HIP path
    stores a tensor and is evaluated layer by layer from the activations the GPU produced (each layer starts from
    the GPU's own input; its own output decides its ReLU mask and BatchNorm statistics).  Two settings:
      exact  (round_grads=False): float32 gradients = exact backpropagation through that forward;
      bf16   (round_grads=True):  gradients rounded where the GPU stores them.
    |bf16 - exact| is what bf16 gradient STORAGE costs by construction: a random walk that grows from 2e-3 behind
    the loss to ~1e-2 at the stem of ResNet-50 (measured, tests/archive/diagnostics/grad_err_depth.py).  Two
    implementations of the same rounding points decorrelate within ~4 layers (one flipped ulp perturbs every sum
    it enters), so beyond the tail of the net the GPU cannot equal the emulation bit for bit; what must hold is
      (1) near the loss (last block + head) the GPU equals the bf16 emulation: <= 3e-3 (measured 3e-5 ... 1.9e-3);
      (2) everywhere the GPU is as close to EXACT backpropagation as the emulation of its rounding points is:
          |GPU - exact| <= 1.5 |bf16 - exact| + 2e-3 for 95 % of the parameter tensors (mean ratio <= 1.1), <= 2.5x for
          every single one, and <= 3e-2 absolutely; activation gradients <= 1.5x each;
      (3) the forward of every layer from the GPU's own input equals the GPU's output to <= 4e-3 (measured 1e-4).
    Round 1 compared with autograd through a forward that did NOT round the raw conv output before BatchNorm
    (rel-L2 0.12): its ReLU masks differed from the GPU's on ~0.4 % of the elements of every layer.  The single
    kernels are pinned to their own output rounding (1.7e-3 bf16, 2e-7 float32) in tests/test_gpu_train_ops.py."""
    from oracle import graph_eval
    classes = 10
    g, specs, ref, net = _pair(network, classes, seed=5)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11))
    net.train()
    net.reset_stats()
    net.forward_backward(x.cuda(), y.cuda())
    state = _torch_state(ref)
    shapes = {t: tuple(v.shape) for t, v in graph_eval.run(g, state, x, train=True).items()}
    forced = {op.dst: net.read_activation(op.dst, n, shapes[op.dst]) for op in g.ops}
    emu = graph_eval.train_step_bf16(g, state, x, y, forced=forced)
    exact = graph_eval.train_step_bf16(g, state, x, y, forced=forced, round_grads=False)
    for op in g.ops:   # (3)
        r = _rel(forced[op.dst], emu["own"][op.dst])
        assert r < 4e-3, f"forward of {op.name or op.kind} from the GPU's own input: relative L2 {r:.3e}"
    assert abs(net.read_stats()[0] / n - float(emu["loss"])) < 1e-4 * max(1.0, float(emu["loss"]))
    convs = [o for o in g.ops if o.kind == arch.OP_CONV]
    blk = convs[-1].name.rsplit(".", 1)[0]                      # last residual block, e.g. base.7.2
    tail_keys = set()
    for o in convs:
        if o.name.startswith(blk + "."):
            tail_keys |= {o.name + ".weight", o.bn + ".weight", o.bn + ".bias"}
    worst, worst_tail = ("", 0.0, 0.0), ("", 0.0)
    ratios = []
    for k, _, kind in specs:
        if k not in emu["grads"]:
            continue
        got = net._read_grad(k, tuple(emu["grads"][k].shape))
        if k.startswith("head."):
            assert _rel(got, exact["grads"][k]) < 1e-4, k
            continue
        noise, err = _rel(emu["grads"][k], exact["grads"][k]), _rel(got, exact["grads"][k])
        if err > worst[1]:
            worst = (k, err, noise)
        ratios.append(max(0.0, err - 2e-3) / max(noise, 1e-12))
        # (a single tensor: 2.5x - the two are independent realisations of the same noise, and with ~60-160 tensors per
        # network a 2-sigma tensor turns up: ResNet-50 @64 x 6 reads 2.0x at the stem's BatchNorm bias, whose sum cancels
        # the most; the population bound below is the sharp one)
        assert err <= 2.5 * noise + 2e-3 and err < 3e-2, f"{k}: |GPU - exact| {err:.3e} vs |bf16 emulation - exact| {noise:.3e}"
        if k in tail_keys:   # (1)
            r = _rel(got, emu["grads"][k])
            worst_tail = max(worst_tail, (k, r), key=lambda t: t[1])
            assert r < 3e-3, f"{k} (last block): |GPU - bf16 emulation| {r:.3e}"
    # ... over all parameter tensors: 95 % within 1.5x of the emulation's own distance from exact backpropagation, and
    # no larger on average
    assert np.percentile(ratios, 95) <= 1.5 and float(np.mean(ratios)) <= 1.1, (np.percentile(ratios, 95), np.mean(ratios))
    worst_a = ("", 0.0, 0.0)
    for op in g.ops:
        t = op.src
        if t == 0 or t not in emu["act_grads"]:
            continue
        got = net.read_activation_grad(t, n, shapes[t])
        noise, err = _rel(emu["act_grads"][t], exact["act_grads"][t]), _rel(got, exact["act_grads"][t])
        if err > worst_a[1]:
            worst_a = (f"input of {op.name}", err, noise)
        assert err <= 1.5 * noise + 2e-3 and err < 3e-2, f"gradient w.r.t. the input of {op.name}: {err:.3e} vs {noise:.3e}"
    print(f"{network}@{hw}x{n}: worst |GPU - exact| {worst[1]:.3e} at {worst[0]} (bf16 emulation there: {worst[2]:.3e}); "
          f"activation gradients {worst_a[1]:.3e} at {worst_a[0]} (emulation {worst_a[2]:.3e}); "
          f"last block |GPU - bf16 emulation| {worst_tail[1]:.3e} at {worst_tail[0]}")


@pytest.mark.parametrize("network,hw,n", [("resnet18", 64, 8), ("resnet50", 96, 16)])
def test_gradients_vs_fp32_autograd(network, hw, n):
    """Against the reference's pure-fp32 forward/backward (sykepic/train/train.py:240-242 on the CPU).

    A bf16 FORWARD differs from the fp32 one by ~1e-2 deep in the net, which flips the ReLU mask of the ~1 % of
    activations that sit next to zero; on these random-weight networks with train-mode BatchNorm over a handful
    of samples that moves whole gradient tensors.  The decomposition is measured here, not assumed: the same
    comparison is made for the CPU oracle `train_step_bf16(round_grads=False)` — a bf16-storage forward with EXACT
    float32 backpropagation and no GPU kernel involved.  It lands at min cosine 0.95 (ResNet-18) / 0.81 (ResNet-50
    @96 x16; 0.76-0.81 also at 128^2 x32 and 224^2 x32, and two float32 evaluation orders of that same oracle agree
    with each other only to cosine 0.90) — the cost of bf16 activations on this problem for ANY implementation.
    Asserted: the GPU is no further from fp32 autograd than that oracle (min and median cosine within 0.05 /
    0.03), every gradient norm within 20 %, loss to 2e-2, logits to 8e-2 relative L2, accuracy counter exact.
    The kernels themselves are pinned to <= 1e-2 by test_backward_matches_the_bf16_emulating_oracle and to
    <= 5e-3 per layer by tests/test_gpu_train_ops.py."""
    from oracle import graph_eval
    classes = 10
    g, specs, ref, net = _pair(network, classes, seed=5)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11))
    state = _torch_state(ref)
    out, loss, want = _fp32_autograd(g, specs, state, x, y)
    emu = graph_eval.train_step_bf16(g, state, x, y, round_grads=False)
    ref.train()
    ref(x)  # running statistics of the reference module
    net.train()
    net.reset_stats()
    logits = net.forward_backward(x.cuda(), y.cuda(), want_logits=True).cpu()
    loss_n, correct = net.read_stats()
    assert abs(loss_n / n - loss) < 2e-2 * max(1.0, abs(loss))
    assert correct == float((out.argmax(1) == y).sum())
    assert _rel(logits, out) < 8e-2
    cos_gpu, cos_emu = {}, {}
    for name, wg in want.items():
        got = net._read_grad(name, tuple(wg.shape))
        cos_gpu[name], cos_emu[name] = _cos(got, wg), _cos(emu["grads"][name], wg)
        ratio = float(got.double().norm() / (wg.double().norm() + 1e-30))
        assert 0.8 < ratio < 1.2, f"{name}: gradient norm ratio {ratio:.3f}"
    gmin, emin = min(cos_gpu.values()), min(cos_emu.values())
    gmed, emed = float(np.median(list(cos_gpu.values()))), float(np.median(list(cos_emu.values())))
    print(f"{network}: cosine vs fp32 autograd  GPU min {gmin:.4f} median {gmed:.4f} | "
          f"CPU bf16-forward oracle min {emin:.4f} median {emed:.4f}")
    assert gmin > emin - 0.05 and gmed > emed - 0.03
    # BatchNorm running statistics (momentum 0.1, unbiased variance) and counter
    sd_ref, sd_hip = ref.state_dict(), net.state_dict()
    for k, _, kind in specs:
        if kind in ("bn_mean", "bn_var"):
            assert torch.allclose(sd_hip[k], sd_ref[k], rtol=2e-2, atol=2e-3), k
        if kind == "bn_nbt":
            assert int(sd_hip[k]) == int(sd_ref[k]) == 1


def test_last_batch_of_one_image_trains_as_in_torch():
    """The reference's loaders keep drop_last=False (data.py:178-180): len(train) % batch_size == 1 yields a batch
    of ONE image.  torch trains it (BatchNorm2d normalises over H*W) unless a feature map has shrunk to 1x1, where
    it raises ValueError.  Same here: a 64x64 image (layer4: 2x2) trains and matches the bf16-emulating oracle;
    a 32x32 image (layer4: 1x1) raises ValueError with torch's message."""
    from oracle import graph_eval
    g, specs, ref, net = _pair("resnet18", 10, seed=5)
    x = torch.from_numpy(synth.synth_images(1, 3, 64, 64, seed=10))
    y = torch.from_numpy(synth.synth_labels(1, 10, seed=11))
    net.train()
    net.reset_stats()
    net.forward_backward(x.cuda(), y.cuda())
    state = _torch_state(ref)
    shapes = {t: tuple(v.shape) for t, v in graph_eval.run(g, state, x, train=True).items()}
    forced = {op.dst: net.read_activation(op.dst, 1, shapes[op.dst]) for op in g.ops}
    exact = graph_eval.train_step_bf16(g, state, x, y, forced=forced, round_grads=False)
    assert abs(net.read_stats()[0] - float(exact["loss"])) < 1e-4 * max(1.0, float(exact["loss"]))
    for k, v in exact["grads"].items():
        r = _rel(net._read_grad(k, tuple(v.shape)), v)
        assert r < (1e-4 if k.startswith("head.") else 3e-2), f"{k}: {r:.3e}"
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        net.forward_backward(torch.from_numpy(synth.synth_images(1, 3, 32, 32, seed=1)).cuda(), y.cuda())
    net.forward_backward(torch.from_numpy(synth.synth_images(2, 3, 32, 32, seed=1)).cuda(),
                         torch.from_numpy(synth.synth_labels(2, 10, seed=2)).cuda())   # two images: fine


def test_resnet50_train_step_at_the_benched_size():
    """BASELINE config 3 at its real size — ResNet-50, batch 256, 224 x 224, 50 classes, head 256,128 (what
    bench.py times) — against the oracle: (a) loss / logits of the whole batch vs the fp32 CPU forward with
    train-mode BatchNorm (bf16 storage: loss 2e-2, logits 8e-2 relative L2), (b) every gradient of layer4 + head
    and the gradient entering layer4 vs the bf16-emulating oracle run over that tail of the network from the
    GPU's own activations (<= 1e-2; these are the batch-256 shapes of dgrad / wgrad / bn_bwd: M = 12544 and
    50176 rows, split-K plans of the real step), (c) every gradient tensor of the net finite and non-zero."""
    from oracle import graph_eval
    classes, n, hw = 50, 256, 224
    g, specs, ref, net = _pair("resnet50", classes, seed=5)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11))
    net.train()
    net.reset_stats()
    logits = net.forward_backward(x.cuda(), y.cuda(), want_logits=True).cpu()
    loss_n, correct = net.read_stats()
    state = _torch_state(ref)
    with torch.no_grad():
        acts = graph_eval.run(g, state, x, train=True)
    out = acts[g.ops[-1].dst]
    loss = float(torch.nn.functional.cross_entropy(out, y))
    assert abs(loss_n / n - loss) < 2e-2 * max(1.0, loss)
    assert _rel(logits, out) < 8e-2
    assert abs(correct - float((out.argmax(1) == y).sum())) <= 3    # near-ties may flip under bf16
    first = next(i for i, op in enumerate(g.ops) if op.child == 7)
    need = {t for op in g.ops[first:] for t in (op.src, op.res, op.dst) if t > 0}
    forced = {t: net.read_activation(t, n, tuple(acts[t].shape)) for t in need}
    del acts
    emu = graph_eval.train_step_bf16(g, state, None, y, forced=forced, first_op=first)
    worst = ("", 0.0)
    for k, v in emu["grads"].items():
        r = _rel(net._read_grad(k, tuple(v.shape)), v)
        if r > worst[1]:
            worst = (k, r)
        assert r < (1e-4 if k.startswith("head.") else 1e-2), f"{k}: relative L2 gradient error {r:.3e}"
    t_in = g.ops[first].src
    r_in = _rel(net.read_activation_grad(t_in, n, tuple(forced[t_in].shape)), emu["act_grads"][t_in])
    assert r_in < 1e-2, f"gradient entering layer4: relative L2 {r_in:.3e}"
    for name, p in net.named_parameters():
        gr = net._read_grad(name, p.shape)
        assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0, name
    print(f"resnet50 b256 224^2: loss {loss_n / n:.4f} vs fp32 {loss:.4f}; logits rel-L2 {_rel(logits, out):.3e}; "
          f"layer4+head worst gradient rel-L2 {worst[1]:.3e} at {worst[0]}; gradient entering layer4 {r_in:.3e}")


GOLD_SLICES = ("base.0.weight", "base.1.weight", "base.1.running_mean", "base.1.running_var", "base.4.0.conv1.weight",
               "base.7.1.conv2.weight", "base.7.1.bn2.bias", "head.0.weight", "head.2.weight", "head.2.bias")


@pytest.mark.parametrize("optim_name", ["SGD", "Adam"])
def test_unfreeze_schedule_matches_reference_golden(golden_dir, optim_name):
    """Same 3-epoch run as tests/golden/make_golden.py drove through the reference's train_net: freeze -> LRWarmup
    steps at epochs 1,2,3, one optimizer step per phase of the unfreeze schedule.

    Round 3: besides losses and per-tensor norms (a norm barely moves in one lr = 0.01 step, so a wrong-signed or
    mis-scaled update would pass those), the UPDATE of every stored 64-element parameter slice, p_after - p_before, is
    compared with the reference's: direction (cosine) and length for SGD, element signs for Adam (whose first steps
    are lr * sign(g) up to eps), for every phase in which the reference moved that slice at all - and the training
    logits of every step against the reference's (bf16 forward vs fp32)."""
    gold = np.load(golden_dir / f"train_{optim_name.lower()}.npz")
    n, hw, classes = 8, 64, 10
    g, specs, ref, net = _pair("resnet18", classes, seed=5)
    schedule.freeze(net.base)
    first = [p for p in net.parameters() if p.requires_grad]
    assert sum(p.numel() for p in first) == int(gold["group_sizes"][0])
    opt = HipOptimizer(net, optim_name, [{"params": first, "lr": 0.01}, {"params": [], "lr": 0.0},
                                         {"params": [], "lr": 0.0}])
    warm = schedule.LRWarmup(net, opt, 0.1, 0.5, 1, 2, 3, verbose=False)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10)).cuda()
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11)).cuda()
    xv = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=12)).cuda()
    yv = torch.from_numpy(synth.synth_labels(n, classes, seed=13)).cuda()
    keys = [k for k, _, _ in specs]
    sd0 = net.state_dict()
    prev_hip = {k: sd0[k].flatten()[:64].double().cpu().numpy() for k in GOLD_SLICES}
    prev_gold = dict(prev_hip)          # both runs start from the same synthetic state (seed 5)
    moved, report = 0, []
    for epoch in (1, 2, 3):
        warm(epoch)
        net.train()
        net.reset_stats()
        logits = net.forward_backward(x, y, want_logits=True)
        opt.step()
        loss_n, _ = net.read_stats()
        # loss within 3 % of the reference's fp32 run (bf16 forward)
        assert abs(loss_n / n - gold["train_loss"][epoch - 1]) < 0.03 * gold["train_loss"][epoch - 1] + 0.02
        gl = gold["train_logits"][epoch - 1]
        rel = float(np.linalg.norm(logits.float().cpu().numpy() - gl) / np.linalg.norm(gl))
        assert rel <= 3e-2, f"epoch {epoch}: training logits rel-L2 {rel:.3e} vs the reference's"
        net.eval()
        net.reset_stats()
        net.eval_step(xv, yv)
        vloss_n, _ = net.read_stats()
        assert abs(vloss_n / n - gold["val_loss"][epoch - 1]) < 0.05 * gold["val_loss"][epoch - 1] + 0.02
        sd = net.state_dict()
        l2 = np.array([float(sd[k].double().norm()) for k in keys])
        assert np.allclose(l2, gold[f"e{epoch}_l2"], rtol=2e-2, atol=1e-3), epoch
        assert int(sd["base.1.num_batches_tracked"]) == int(gold[f"e{epoch}_nbt"])
        for k in GOLD_SLICES:
            cur_hip = sd[k].flatten()[:64].double().cpu().numpy()
            cur_gold = gold[f"e{epoch}_{k}"].astype(np.float64)
            du_hip, du_gold = cur_hip - prev_hip[k], cur_gold - prev_gold[k]
            prev_hip[k], prev_gold[k] = cur_hip, cur_gold
            scale = max(float(np.abs(cur_gold).max()), 1e-6)
            if np.abs(du_gold).max() < 1e-7 * scale:
                # the reference did not move this slice in this phase (frozen): neither may the HIP path
                assert np.abs(du_hip).max() < 1e-6 * scale, (epoch, k)
                continue
            moved += 1
            if k.endswith(("running_mean", "running_var")):
                # BatchNorm buffers: momentum update from the batch statistics (no optimizer involved)
                assert np.allclose(du_hip, du_gold, rtol=5e-2, atol=2e-3 * scale), (epoch, k)
                continue
            big = np.abs(du_gold) > 0.05 * np.abs(du_gold).max()
            if optim_name == "Adam":
                agree = float((np.sign(du_hip[big]) == np.sign(du_gold[big])).mean())
                ratio = np.linalg.norm(du_hip[big]) / np.linalg.norm(du_gold[big])
                report.append((epoch, k, agree, float(ratio)))
            else:
                cos = float(du_hip @ du_gold / (np.linalg.norm(du_hip) * np.linalg.norm(du_gold)))
                ratio = float(np.linalg.norm(du_hip) / np.linalg.norm(du_gold))
                report.append((epoch, k, cos, ratio))
    for epoch, k, a, ratio in report:
        print(f"   epoch {epoch} {k}: {'sign agreement' if optim_name == 'Adam' else 'cosine'} {a:.4f}, norm ratio {ratio:.3f}")
    # Bounds.  Head and last residual block (what the reference's fp32 run and a bf16 run agree on): cosine >= 0.98 and
    # norm +- 5 % (SGD), sign agreement >= 0.97 (Adam).  Measured there: cosine 0.9979-1.0000, norm ratio 0.993-1.013,
    # signs 0.984-1.0.  The slices deep in the base (stem conv / stem BatchNorm / layer1) compare a bf16 FORWARD with the
    # reference's fp32 forward on a random-weight net with batch statistics over 8 images: the CPU oracle with bf16
    # storage and EXACT float32 backpropagation - no GPU kernel involved - is itself only at cosine 0.95 to fp32 autograd
    # on whole tensors there (test_gradients_vs_fp32_autograd), and a 64-element slice is noisier than a tensor.
    # Measured on those slices over the realisations seen so far: cosine 0.894-0.983, norm ratio 0.81-1.13, signs
    # 0.80-0.98; asserted: every slice cosine >= 0.85 AND their mean >= 0.93, norm +- 35 %, signs >= 0.75.  (These slices
    # are chaotic, not just noisy: re-associating ONE fp32 sum of the BatchNorm-backward reduction - two rows per loop
    # iteration instead of one - moved the stem conv's ratio from 0.81 to 0.75 in round 3; taking the reduction's sums
    # from the fp32 gradient before it is rounded to bf16 (round 4, csrc/conv_igemm.hip: closer to exact
    # backpropagation, see test_backward_matches_the_bf16_emulating_oracle) moved layer1's conv slice from 0.936 to 0.894
    # and the stem conv's from 0.94 to 0.983.  One 64-element slice says "same direction" at either value; the mean over
    # the deep slices is the stable statistic.)  (The backward kernels are pinned at the GPU's own operating point by
    # test_backward_matches_the_bf16_emulating_oracle; this test adds that sign and scale of every update follow the
    # reference's through its whole unfreeze schedule.)
    deep = []
    for epoch, k, a, ratio in report:
        near = k.startswith(("head.", "base.7.1."))
        if optim_name == "Adam":
            # deep slices: every element of an Adam update is +-lr whatever |g| is, so the elements whose gradient is
            # noise count like the others, and the state has drifted through two sign-like steps before the stem first
            # moves: one 64-element slice has read 0.59 (stem conv, round 4) as well as 0.98 - asserted: each above what
            # coin flips give with margin, and their MEAN >= 0.80 (measured 0.875-0.93)
            assert a >= (0.97 if near else 0.55), f"epoch {epoch} {k}: update signs agree on {a:.2f} of the elements"
            assert 0.85 <= ratio <= 1.15, (epoch, k, ratio)
            if not near:
                deep.append(a)
        else:
            assert a >= (0.98 if near else 0.85), f"epoch {epoch} {k}: update cosine {a:.4f}"
            lo, hi = (0.95, 1.05) if near else (0.65, 1.35)
            assert lo <= ratio <= hi, f"epoch {epoch} {k}: update norm ratio {ratio:.3f}"
            if not near:
                deep.append(a)
    assert deep and float(np.mean(deep)) >= (0.80 if optim_name == "Adam" else 0.93), \
        f"mean update {'sign agreement' if optim_name == 'Adam' else 'cosine'} of the deep-base slices {np.mean(deep):.4f}"
    assert moved >= 12      # head + BN slices move in every phase, the conv slices from their unfreeze epoch on
    assert np.allclose([gp["lr"] for gp in opt.param_groups], gold["group_lr"][0])
    assert [sum(p.numel() for p in gp["params"]) for gp in opt.param_groups] == gold["group_sizes"].tolist()


@pytest.mark.parametrize("name", ["SGD", "Adam", "AdamW", "RMSprop", "Adagrad", "Adamax", "NAdam", "RAdam", "Adadelta", "ASGD",
                                  "Rprop"])
def test_optimizers_match_torch_update_rule(name):
    """The reference builds `getattr(optim, name)(groups)` with nothing but `lr` (train.py:131-138): every
    first-order torch.optim class with its torch defaults has a fused multi-tensor kernel.  After each of 3 steps
    every updated parameter equals torch.optim's result on the same (HIP) gradients (RAdam runs 7 steps: its
    rho_t > 5 switch to the rectified update happens at step 6)."""
    classes, n, hw = 10, 8, 64
    for name in (name,):
        g, specs, ref, net = _pair("resnet18", classes, seed=7)
        x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10)).cuda()
        y = torch.from_numpy(synth.synth_labels(n, classes, seed=11)).cuda()
        params = list(net.parameters())
        opt = HipOptimizer(net, name, [{"params": params, "lr": 0.01}])
        net.train()
        before = net.state_dict()
        tparams = {p.key: torch.nn.Parameter(before[p.key].clone()) for p in params}
        topt = getattr(torch.optim, name)(list(tparams.values()), lr=0.01)
        for step in range(7 if name == "RAdam" else 3):   # RAdam: rho_t > 5 from step 6 on (rectified branch)
            net.forward_backward(x, y)
            for p in params:
                tparams[p.key].grad = net._read_grad(p.key, p.shape)
            opt.step()
            topt.step()
            after = net.state_dict()
            for k, tp in tparams.items():
                assert torch.allclose(after[k], tp.detach(), rtol=1e-5, atol=1e-6), (name, step, k)
            # keep the two trajectories on identical parameters
            for k, tp in tparams.items():
                tp.data.copy_(after[k])


def test_head_dropout_trains():
    """`[model] dropout = 1,0.5` (reference network.py:59-61): nn.Dropout between the head's Linear layers, active
    in train mode, identity in eval mode.  The kept set comes from the library's own counter-based generator
    (seeded: spk_model_set_seed); checked: kept fraction, the 1/(1-p) scale, a fresh mask every step, the same
    masks for the same seed, eval = identity, and every gradient against the oracle evaluated on the GPU's kept
    set."""
    from oracle import graph_eval
    from sykepic_hip.net import HipNet
    classes, n, hw, p = 10, 64, 64, 0.5
    g = arch.build_graph("resnet18", classes, [256, 128], [(1, p)])
    specs = arch.param_specs(g)
    sd = synth.synth_state_dict(specs, seed=5, logit_gain=2.0)
    drop = next(op for op in g.ops if op.kind == arch.OP_DROPOUT)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11))

    def run(seed, steps=1):
        net = HipNet("resnet18", classes, weights=None, dropout=[(1, p)])
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        net.set_seed(seed)
        net.train()
        outs = []
        for _ in range(steps):
            net.reset_stats()
            net.forward_backward(x.cuda(), y.cuda())
            outs.append((net.read_activation(drop.src, n, (n, 256)), net.read_activation(drop.dst, n, (n, 256))))
        return net, outs

    net, (first, second) = run(seed=3, steps=2)
    for a, b in (first, second):
        keep = b != 0
        frac = float(keep.float().mean())
        assert abs(frac - (1 - p)) < 4 * (p * (1 - p) / keep.numel()) ** 0.5 + 0.01, frac
        assert torch.allclose(b[keep], a[keep] / (1 - p), rtol=1e-6, atol=0)
    assert not torch.equal(first[1] != 0, second[1] != 0)                     # a new mask every step
    _, (again,) = run(seed=3)
    assert torch.equal(again[1] != 0, first[1] != 0)                          # same seed, same first mask
    _, (other,) = run(seed=4)
    assert not torch.equal(other[1] != 0, first[1] != 0)
    # gradients of the second step of `net` on its kept set
    state = {k: v.clone() for k, v in net.state_dict().items()}
    # (the state moved by no optimizer step: only BN running statistics changed, which train mode does not read)
    shapes = {t: tuple(v.shape) for t, v in graph_eval.run(g, state, x, train=True).items()}
    forced = {op.dst: net.read_activation(op.dst, n, shapes[op.dst]) for op in g.ops}
    exact = graph_eval.train_step_bf16(g, state, x, y, forced=forced, round_grads=False)
    assert _rel(forced[drop.dst], exact["own"][drop.dst]) < 1e-6
    for k, v in exact["grads"].items():
        r = _rel(net._read_grad(k, tuple(v.shape)), v)
        assert r < (1e-4 if k.startswith("head.") else 3e-2), f"{k}: {r:.3e}"
    net.eval()
    z = net(x[:4].cuda())
    assert torch.equal(net.read_activation(drop.dst, 4, (4, 256)), net.read_activation(drop.src, 4, (4, 256)))
    assert torch.isfinite(z).all()


def test_training_is_bitwise_reproducible():
    classes, n, hw = 10, 8, 64
    grads = []
    for _ in range(2):
        g, specs, ref, net = _pair("resnet18", classes, seed=5)
        x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10)).cuda()
        y = torch.from_numpy(synth.synth_labels(n, classes, seed=11)).cuda()
        net.train()
        net.forward_backward(x, y)
        grads.append({p.key: net._read_grad(p.key, p.shape) for p in net.parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_launch_forms_of_the_step_give_the_same_weights():
    """Round 5 changed HOW two things are launched, not what they compute: the stem pool's backward handles pixel pairs, and
    the step returns before the last weight gradient is done (the optimizer updates that tensor last, behind a join).
    Five Adam steps of ResNet-50 at 64 x 64, batch 32, each form switched off in turn and everything on one stream: the
    same weights and running statistics, bit for bit."""
    import hashlib
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    code = (
        "import sys, hashlib, numpy as np, torch\n"
        f"sys.path[:0] = [{str(root)!r}, {str(root / 'syke-pic_amd')!r}]\n"
        "from sykepic_hip import synth\n"
        "from sykepic_hip.net import HipNet\n"
        "from sykepic_hip.optim import HipOptimizer\n"
        "net = HipNet('resnet50', 10, weights=None, head=(64, 32))\n"
        "net.reset_parameters(seed=3); net.set_seed(3)\n"
        "for p in net.parameters(): p.requires_grad = True\n"
        "opt = HipOptimizer(net, 'Adam', [{'params': list(net.parameters()), 'lr': 1e-3}])\n"
        "net.train()\n"
        "for s in range(5):\n"
        "    x = torch.from_numpy(synth.synth_images(32, 3, 64, 64, seed=100 + s)).cuda()\n"
        "    y = torch.from_numpy(synth.synth_labels(32, 10, seed=200 + s)).cuda()\n"
        "    net.forward_backward(x, y); opt.step()\n"
        "h = hashlib.sha256()\n"
        "for k, v in sorted(net.state_dict().items()): h.update(v.cpu().numpy().tobytes())\n"
        "print('SHA', h.hexdigest())\n")
    seen = {}
    for env in ({}, {"SPK_POOL_PAIR": "0"}, {"SPK_TAIL_DEFER": "0"}, {"SPK_WGRAD_STREAM": "0"}):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPK_TUNE_CACHE="off", SPK_AUTOTUNE="0", **env),
                             capture_output=True, text=True, timeout=900)   # (tile choice pinned: it groups the BatchNorm partial sums)
        assert out.returncode == 0, out.stderr[-2000:]
        sha = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("SHA")]
        assert len(sha) == 1, out.stdout[-500:]
        seen[str(env)] = sha[0]
    assert len(set(seen.values())) == 1, seen


@pytest.mark.parametrize("network", ["resnet50", "efficientnet_b0", "mobilenet_v3_small", "resnext50_32x4d"])
def test_single_stream_step_gives_the_two_stream_gradients(network):
    """The per-phase profile runs the step on ONE stream (weight gradients behind the data gradients, in line), every other
    caller on two.  Same seed, same batch, same step counter - so dropout and stochastic depth draw the same masks - and
    everything trainable: the second step of a handle that ran `forward_backward` twice and the single-stream step of
    `profile_train` (behind its two-stream warm-up step) leave the same gradients, bit for bit.  ResNet-50: deferral and
    the fused reductions; EfficientNet-B0: 3x3 stem, depthwise, squeeze-excitation, stochastic depth, the padded reduce;
    MobileNetV3-Small: ReLU / Hardsigmoid gates; ResNeXt-50: grouped convs."""
    from sykepic_hip.net import HipNet
    classes, n, hw = 10, 6, 64
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10)).cuda()
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11)).cuda()
    grads = []
    for single_stream in (False, True):
        net = HipNet(network, classes, weights=None)
        net.reset_parameters(seed=3)
        net.set_seed(3)
        for p in net.parameters():
            p.requires_grad = True
        net.train()
        if single_stream:
            net.profile_train(x, y, iters=1)
        else:
            net.forward_backward(x, y)
            net.forward_backward(x, y)
        grads.append({p.key: p.grad for p in net.parameters()})
    assert len(grads[0]) > 0 and grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.isfinite(grads[0][k]).all(), k
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_fresh_network_is_randomly_initialised_and_learns():
    """A HipNet built with weights=None starts from torch/torchvision's initial distributions (the
    reference's TorchVisionNet(weights=None)), reproducibly under torch.manual_seed, and a few Adam steps on one
    batch reduce the loss (an all-zero start would leave every conv dead)."""
    from sykepic_hip.net import HipNet
    from sykepic_hip.optim import HipOptimizer
    torch.manual_seed(7)
    net = HipNet("resnet18", 5, weights=None, head=(32,))
    sd = net.state_dict()
    w = sd["base.4.0.conv1.weight"]                     # [64, 64, 3, 3]: std = sqrt(2 / (64*9))
    assert abs(float(w.std()) - (2.0 / (64 * 9)) ** 0.5) < 0.1 * (2.0 / (64 * 9)) ** 0.5 and abs(float(w.mean())) < 2e-3
    assert torch.all(sd["base.1.weight"] == 1) and torch.all(sd["base.1.bias"] == 0)
    assert torch.all(sd["base.1.running_var"] == 1) and int(sd["base.1.num_batches_tracked"]) == 0
    hw_ = sd["head.0.weight"]                           # U(+-1/sqrt(512))
    assert float(hw_.abs().max()) <= 512 ** -0.5 + 1e-7 and float(hw_.std()) > 0.5 * 512 ** -0.5 / 3 ** 0.5
    torch.manual_seed(7)
    again = HipNet("resnet18", 5, weights=None, head=(32,)).state_dict()
    assert all(torch.equal(again[k], v) for k, v in sd.items())
    x = torch.from_numpy(synth.synth_images(16, 3, 64, 64, seed=3)).cuda()
    y = torch.from_numpy(synth.synth_labels(16, 5, seed=4)).cuda()
    opt = HipOptimizer(net, "Adam", [{"params": list(net.parameters()), "lr": 1e-3}])
    net.train()
    losses = []
    for _ in range(12):
        net.reset_stats()
        net.forward_backward(x, y)
        opt.step()
        losses.append(net.read_stats()[0] / 16)
    print("losses", [round(l, 3) for l in losses])
    assert losses[-1] < 0.7 * losses[0]


def test_weights_argument_loads_a_local_backbone_checkpoint(tmp_path):
    """`weights=<path to a torchvision checkpoint>` fills `base` (what `weights="DEFAULT"` downloads in the
    reference), the head keeps its fresh initialisation."""
    from oracle import backbones
    from sykepic_hip.net import HipNet
    tv = backbones.make("resnet18")
    torch.manual_seed(3)
    for p in tv.parameters():
        p.data.normal_(0, 0.05)
    path = tmp_path / "resnet18-local.pth"
    torch.save(tv.state_dict(), path)
    net = HipNet("resnet18", 4, weights=str(path), head=(16,))
    sd = net.state_dict()
    assert torch.equal(sd["base.0.weight"], tv.state_dict()["conv1.weight"])
    assert torch.equal(sd["base.7.1.bn2.running_var"], tv.state_dict()["layer4.1.bn2.running_var"])
    assert float(sd["head.0.weight"].abs().max()) <= 512 ** -0.5 + 1e-7
    with pytest.raises(RuntimeError, match="not a resnet50 backbone"):
        HipNet("resnet50", 4, weights=str(path))


@pytest.mark.parametrize("network,hw", [("resnet50", 64), ("efficientnet_b0", 64)])
def test_activations_read_after_a_train_step_are_the_train_steps(network, hw):
    """The eval path leaves some tensors to fused kernels (stem + max-pool, the shortcut conv inside the block-closing conv,
    the squeeze-excitation scaling inside the project conv) and `read_activation` recomputes them on demand from the last
    EVAL forward.  After a TRAINING pass on the same handle every tensor has really been written - in train mode, with
    batch statistics - and must be returned as it is: an eval forward, then a train step, then every activation must
    equal what a handle that never ran eval returns (the train step is bitwise reproducible)."""
    n, classes = 6, 10
    g, specs, ref, net = _pair(network, classes, seed=5)
    _, _, _, fresh = _pair(network, classes, seed=5)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10)).cuda()
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11)).cuda()
    net.eval()
    p = net.probabilities(x)
    assert torch.isfinite(p).all()
    from oracle import graph_eval
    shapes = {t: tuple(v.shape) for t, v in graph_eval.run(g, _torch_state(ref), x.cpu(), train=True).items()}
    for h in (net, fresh):
        h.train()
        h.reset_stats()
        h.forward_backward(x, y)
    for op in g.ops:
        a, b = net.read_activation(op.dst, n, shapes[op.dst]), fresh.read_activation(op.dst, n, shapes[op.dst])
        assert torch.equal(a, b), f"{op.name or op.kind}: read back differs after an earlier eval forward"
