"""ResNeXt / Wide ResNet on the GPU: the grouped-conv kernels (csrc/conv_group.hip) one by one through their C-ABI hooks
against torch on the CPU, whole-network inference and training against a torch module built here from
nn.Conv2d(groups=...), batch independence, the calibrated mode and `prob` on a ResNeXt model directory."""

import ctypes
import math
import shutil
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sykepic_hip import arch, lib, synth
from test_host_grouped import GROUPED, TorchVisionNet, torch_resnet

pytestmark = pytest.mark.gpu

SPK_ERR_UNSUPPORTED = -4


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# (channels per group, stride, input size, batch): every C/g, both strides, sizes 7 / 14 / 15 / 56, batches 1 / 3 / 64
CASES = [(4, 1, 56, 3), (4, 2, 15, 64), (4, 1, 7, 1), (8, 1, 14, 64), (8, 2, 56, 1), (16, 1, 7, 3), (16, 2, 14, 3),
         (32, 1, 15, 1), (32, 2, 7, 64), (64, 1, 14, 3), (64, 2, 15, 3), (64, 2, 56, 1)]


def _problem(cpg, n, hw, seed):
    c = max(64, 2 * cpg)
    groups = c // cpg
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, hw, hw, generator=gen)
    w = torch.randn(c, cpg, 3, 3, generator=gen) * (2.0 / (9 * cpg)) ** 0.5
    return c, groups, x, w


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def _ohwi(w):
    """[c][c/g][3][3] -> the hooks' weight layout [c][3][3][c/g] on the device."""
    return w.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("cpg,stride,hw,n", CASES)
def test_grouped_forward_bn_relu_hook(cpg, stride, hw, n):
    """Eval forward (fp16 activations, fp32 weights and sums) + folded BatchNorm + ReLU against torch on the same
    fp16-rounded input in float64; and the raw bf16 output the training forward stores."""
    so = lib.load()
    c, groups, x, w = _problem(cpg, n, hw, seed=cpg * 7 + stride)
    scale, bias = torch.rand(c) + 0.5, torch.randn(c) * 0.1
    xh = x.half()
    want = F.conv2d(xh.double(), w.double(), stride=stride, padding=1, groups=groups)
    want_bn = torch.relu(want * scale.double()[:, None, None] + bias.double()[:, None, None])
    ho = (hw - 1) // stride + 1
    # (every device operand is held by a name until the synchronous call returns)
    y = torch.empty(n, ho, ho, c, dtype=torch.float16, device="cuda")
    xg, wg, sg, bg = _nhwc(xh, torch.float16), _ohwi(w), scale.cuda(), bias.cuda()
    rc = so.spk_op_conv_group(_p(xg), _p(wg), _p(sg), _p(bg), _p(y), n, hw, hw, c, groups, stride, 1, 0, None)
    assert rc == 0, so.spk_last_error()
    assert _rel(_nchw(y), want_bn) < 2e-3
    xb = x.bfloat16()
    want_raw = F.conv2d(xb.double(), w.double(), stride=stride, padding=1, groups=groups)
    yb = torch.empty(n, ho, ho, c, dtype=torch.bfloat16, device="cuda")
    xg = _nhwc(xb, torch.bfloat16)
    rc = so.spk_op_conv_group(_p(xg), _p(wg), None, None, _p(yb), n, hw, hw, c, groups, stride, 0, 1, None)
    assert rc == 0, so.spk_last_error()
    assert _rel(_nchw(yb), want_raw) < 1e-2


@pytest.mark.parametrize("cpg,stride,hw,n", CASES)
def test_grouped_backward_hooks(cpg, stride, hw, n):
    """dgrad (overwrite and accumulate) and wgrad, bf16 operands, against float64 autograd on the same rounded operands."""
    so = lib.load()
    c, groups, x, w = _problem(cpg, n, hw, seed=cpg * 11 + stride)
    xb = x.bfloat16()
    ho = (hw - 1) // stride + 1
    dy = torch.randn(n, c, ho, ho, generator=torch.Generator().manual_seed(3)).bfloat16()
    xd = xb.double().requires_grad_()
    wd = w.double().requires_grad_()
    F.conv2d(xd, wd, stride=stride, padding=1, groups=groups).backward(dy.double())
    dx = torch.empty(n, hw, hw, c, dtype=torch.bfloat16, device="cuda")
    dyg, wg, xg = _nhwc(dy, torch.bfloat16), _ohwi(w), _nhwc(xb, torch.bfloat16)
    rc = so.spk_op_conv_group_dgrad(_p(dyg), _p(wg), _p(dx), 0, n, hw, hw, c, groups, stride, None)
    assert rc == 0, so.spk_last_error()
    assert _rel(_nchw(dx), xd.grad) < 1e-2
    prior = torch.randn(n, c, hw, hw, generator=torch.Generator().manual_seed(4)).bfloat16()
    dx2 = _nhwc(prior, torch.bfloat16)
    rc = so.spk_op_conv_group_dgrad(_p(dyg), _p(wg), _p(dx2), 1, n, hw, hw, c, groups, stride, None)
    assert rc == 0, so.spk_last_error()
    assert _rel(_nchw(dx2), xd.grad + prior.double()) < 1e-2
    dw = torch.empty(c, 3, 3, cpg, dtype=torch.float32, device="cuda")
    rc = so.spk_op_conv_group_wgrad(_p(xg), _p(dyg), _p(dw), n, hw, hw, c, groups, stride, None)
    assert rc == 0, so.spk_last_error()
    assert _rel(dw.cpu().permute(0, 3, 1, 2), wd.grad) < 1e-4


def test_unsupported_group_shapes_are_refused():
    so = lib.load()
    buf = torch.zeros(1 << 16, device="cuda")
    for c, groups, stride in ((48, 8, 1), (64, 64, 1), (64, 1, 1), (256, 2, 1), (64, 16, 3)):   # C/g 6, 1, dense, 128
        rc = so.spk_op_conv_group(_p(buf), _p(buf), None, None, _p(buf), 1, 4, 4, c, groups, stride, 0, 1, None)
        assert rc == SPK_ERR_UNSUPPORTED and b"per group" in so.spk_last_error()
    g = arch.build_graph("resnext50_32x4d", 10)
    descs = (lib.LayerDesc * len(g.ops))()
    for d, op in zip(descs, g.ops):
        d.kind, d.cin, d.cout, d.k, d.stride, d.pad = op.kind, op.cin, op.cout, op.k, op.stride, op.pad
        d.relu, d.src, d.dst, d.res, d.child, d.p = int(op.relu), op.src, op.dst, op.res, op.child, op.p
        d.name, d.bn = op.name.encode(), op.bn.encode()
    groups = [op.groups for op in g.ops]
    groups[[i for i, op in enumerate(g.ops) if op.k == 1 and op.kind == arch.OP_CONV][0]] = 2   # a grouped 1x1 conv
    h = ctypes.c_void_p()
    rc = lib.load().spk_model_create_grouped(descs, (ctypes.c_int32 * len(groups))(*groups), len(descs), 3, 10, 0,
                                             ctypes.byref(h))
    assert rc == SPK_ERR_UNSUPPORTED


def _pair(network, classes, seed, head=(256, 128)):
    from sykepic_hip.net import HipNet
    depths, groups, wpg, _ = GROUPED[network]
    g = arch.build_graph(network, classes, list(head))
    sd = synth.synth_state_dict(arch.param_specs(g), seed=seed)
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    ref = TorchVisionNet(torch_resnet(depths, groups, wpg), classes, head)
    ref.load_state_dict(state)
    net = HipNet(network, classes, weights=None, head=head)
    net.load_state_dict(state)
    return ref, net, state


def _ref_probs(ref, x):
    ref.eval()
    with torch.no_grad():
        return F.softmax(ref(x) * math.log(1.3), dim=1)


@pytest.mark.parametrize("network", ["resnext50_32x4d", "wide_resnet50_2"])
def test_inference_parity_and_batch_independence(network):
    torch.set_num_threads(16)
    ref, net, _ = _pair(network, 50, seed=2)
    net.eval()
    x = torch.from_numpy(synth.synth_images(32, 3, 224, 224, seed=0))
    p = net.probabilities(x.cuda()).cpu()
    want = _ref_probs(ref, x)
    err = float((p - want).abs().max())
    print(f"{network} 32x224^2: max |dp| = {err:.2e}")
    assert err < 1e-3
    one = net.probabilities(x[5:6].cuda()).cpu()
    assert torch.equal(one[0], p[5])


def test_resnext101_32x8d_forward_at_a_small_size():
    ref, net, _ = _pair("resnext101_32x8d", 20, seed=4)
    net.eval()
    x = torch.from_numpy(synth.synth_images(3, 3, 64, 64, seed=1))
    err = float((net.probabilities(x.cuda()).cpu() - _ref_probs(ref, x)).abs().max())
    print(f"resnext101_32x8d 3x64^2: max |dp| = {err:.2e}")
    assert err < 1e-3


def test_calibrated_mode_on_resnext():
    """Calibrated single-pass mode: grouped layers keep their fp32 weights (nothing to round), the dense ones are
    zero-sum rounded - the means vector covers only the dense convs - and the result stays within 1e-3."""
    ref, net, _ = _pair("resnext50_32x4d", 50, seed=2)
    net.eval()
    x = torch.from_numpy(synth.synth_images(32, 3, 128, 128, seed=6))
    net.calibrate(x.cuda())
    g = net.graph
    dense_cin = sum(op.cin for op in g.ops if op.kind == arch.OP_CONV and op.groups == 1)
    assert net.act_means().numel() == dense_cin
    net.set_precision("calibrated")
    p = net.probabilities(x.cuda()).cpu()
    err = float((p - _ref_probs(ref, x)).abs().max())
    print(f"resnext50_32x4d calibrated: max |dp| = {err:.2e}")
    assert err < 1e-3
    assert torch.equal(net.probabilities(x[:1].cuda()).cpu()[0], p[0])


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def test_train_step_matches_autograd_and_learns():
    from sykepic_hip.optim import HipOptimizer
    torch.set_num_threads(16)
    classes, n, hw = 10, 16, 64
    ref, net, state = _pair("resnext50_32x4d", classes, seed=5)
    x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=10))
    y = torch.from_numpy(synth.synth_labels(n, classes, seed=11))
    ref.train()
    out = ref(x)
    loss = F.cross_entropy(out, y)
    loss.backward()
    net.train()
    net.reset_stats()
    net.forward_backward(x.cuda(), y.cuda())
    loss_n, _ = net.read_stats()
    print(f"loss GPU {loss_n / n:.5f} fp32 autograd {float(loss.detach()):.5f}")
    loss = float(loss.detach())
    assert abs(loss_n / n - loss) < 2e-2 * max(1.0, loss)
    cos, ratios, grouped, dense = {}, {}, {}, {}
    for name, prm in ref.named_parameters():
        got = net._read_grad(name, tuple(prm.shape))
        cos[name] = _cos(got, prm.grad)
        ratios[name] = float(got.double().norm() / (prm.grad.double().norm() + 1e-30))
        if name.endswith("conv2.weight"):
            grouped[name] = cos[name]
        elif name.endswith(".weight") and prm.dim() == 4:
            dense[name] = cos[name]
    # bf16 activations put any implementation of this step at median cosine ~0.9 / min ~0.8 from fp32 autograd on a
    # random-weight bottleneck net (tests/test_gpu_train.py measures the same floor for ResNet-50 with a CPU bf16
    # emulation); the grouped convs must sit on that floor like the dense convs of the same step
    med, gmed, dmed = (float(np.median(list(v.values()))) for v in (cos, grouped, dense))
    print(f"cosine vs fp32 autograd: median {med:.4f}, min {min(cos.values()):.4f}; grouped convs median {gmed:.4f}, "
          f"min {min(grouped.values()):.4f}; dense convs median {dmed:.4f}")
    assert med > 0.85 and min(cos.values()) > 0.75
    assert gmed > dmed - 0.03 and min(grouped.values()) > min(dense.values()) - 0.05
    assert np.mean([0.8 < r < 1.2 for r in ratios.values()]) > 0.9
    # a few Adam steps on one batch: the loss goes down (lr 1e-4: at 1e-3 these synthetic weights make the dense ResNet-50
    # jump for a few steps as well)
    opt = HipOptimizer(net, "Adam", [{"params": list(net.parameters()), "lr": 1e-4}])
    losses = []
    for _ in range(6):
        net.reset_stats()
        net.forward_backward(x.cuda(), y.cuda())
        opt.step()
        losses.append(net.read_stats()[0] / n)
    print("losses", losses)
    assert losses[-1] < 0.5 * losses[0] and losses[-1] < losses[1]
    # state_dict round trip, bit-exact
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    _, net2, _ = _pair("resnext50_32x4d", classes, seed=9)
    net2.load_state_dict(sd)
    sd2 = net2.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert tuple(sd["base.4.0.conv2.weight"].shape) == (128, 4, 3, 3)


Args = namedtuple("Args", "raw samples image_dir images model out batch_size num_workers force")


def test_prob_on_a_resnext_model_directory(tmp_path, golden_dir):
    """`prob` on a directory as the reference leaves it (config.ini naming the network, class_names.txt,
    best_state.pth): auto-calibration arms, the CSVs have the reference's format and stay within 1e-3."""
    from sykepic_hip import ifcb, prob
    from sykepic_hip.config import get_img_shape, get_transforms
    from configparser import ConfigParser
    from test_gpu_workflows import _synthetic_sample
    model = tmp_path / "model"
    model.mkdir()
    shutil.copy(golden_dir / "ref_data" / "class_names.txt", model / "class_names.txt")
    text = (golden_dir / "ref_data" / "config.ini").read_text().replace("network = resnet18",
                                                                        "network = resnext50_32x4d")
    (model / "config.ini").write_text(text)
    ref, _, state = _pair("resnext50_32x4d", 50, seed=2)
    torch.save(state, model / "best_state.pth")
    raw = tmp_path / "raw"
    name = "D20200101T000000_IFCB114"
    _synthetic_sample(raw, name, 120, seed=1)
    out = tmp_path / "out"
    prob.call(Args(str(raw), None, None, None, str(model), out, 64, 2, False))
    csv = out / "2020" / "01" / "01" / f"{name}.prob.csv"
    lines = csv.read_text().splitlines()
    header = lines[0].split(",")
    assert len(header) == 51 and header[0] == "roi" and len(lines) == 1 + 120
    assert [int(ln.split(",")[0]) for ln in lines[1:]] == list(range(1, 121))
    assert (model / prob.ACT_MEANS_FILE).exists()
    cfg = ConfigParser()
    cfg.read(model / "config.ini")
    _, ev = get_transforms(cfg, get_img_shape(cfg))
    rois = ifcb.read_rois(raw / f"{name}.adc", raw / f"{name}.roi")
    x = torch.stack([ev(np.repeat(img[:, :, None], 3, axis=2)) for _, img in rois])
    want = _ref_probs(ref, x).numpy()
    got = np.array([[float(v) for v in ln.split(",")[1:]] for ln in lines[1:]])
    err = float(np.abs(got - want).max())
    print(f"prob on resnext50_32x4d: {len(rois)} ROIs, max |dp| = {err:.2e}")
    assert err <= 1e-3 + 5e-6
