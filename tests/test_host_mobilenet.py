"""MobileNetV3 Large / Small on the host side: the layer graph, its state_dict layout against a torch.nn restatement
of torchvision's model, parameter counts against torchvision's published totals, checkpoint key mapping and FLOPs."""

import math

import pytest
import torch

from sykepic_hip import arch

NETS = ("mobilenet_v3_large", "mobilenet_v3_small")


@pytest.mark.parametrize("network", NETS)
def test_param_specs_match_the_restatement_state_dict(network):
    from mobilenet_ref import TorchVisionNet
    g = arch.build_graph(network, 50)
    specs = arch.param_specs(g)
    ref = TorchVisionNet(network, 50).state_dict()
    assert [k for k, _, _ in specs] == list(ref)
    for k, shape, _ in specs:
        assert tuple(ref[k].shape) == tuple(shape), k
    assert g.feat == (960 if network == "mobilenet_v3_large" else 576)
    assert g.n_base_children == 2


@pytest.mark.parametrize("network,backbone,classifier", [
    ("mobilenet_v3_large", 2_971_952, 2_511_080),   # Linear 960 -> 1280 -> 1000
    ("mobilenet_v3_small", 927_008, 1_615_848),     # Linear 576 -> 1024 -> 1000
])
def test_parameter_counts_add_up_to_torchvision_totals(network, backbone, classifier):
    from mobilenet_ref import MobileNetV3
    specs = arch.param_specs(arch.build_graph(network, 1000, head=()))
    n = sum(math.prod(s) for k, s, kind in specs
            if k.startswith("base.") and kind not in ("bn_mean", "bn_var", "bn_nbt"))
    assert n == backbone
    assert n + classifier == (5_483_032 if network == "mobilenet_v3_large" else 2_542_856)
    assert sum(p.numel() for p in MobileNetV3(network).parameters()) == n + classifier


@pytest.mark.parametrize("network", NETS)
def test_graph_activations_and_gates(network):
    g = arch.build_graph(network, 50)
    stem = g.ops[0]
    assert (stem.kind, stem.cin, stem.cout, stem.k, stem.stride, int(stem.relu)) == (arch.OP_CONV, 3, 16, 3, 2,
                                                                                  arch.ACT_HSWISH)
    ses = [op for op in g.ops if op.kind == arch.OP_SE]
    assert ses and all(int(op.relu) == arch.ACT_RELU for op in ses)
    assert all(op.k % 8 == 0 and op.cin % 8 == 0 for op in ses)
    for op in g.ops:
        if op.kind in (arch.OP_CONV, arch.OP_DWCONV, arch.OP_SE):
            assert op.cout % 8 == 0 and (op.cin <= 4 or op.cin % 8 == 0), op.name
    acts = {int(op.relu) for op in g.ops if op.kind in (arch.OP_CONV, arch.OP_DWCONV)}
    assert acts == {arch.ACT_NONE, arch.ACT_RELU, arch.ACT_HSWISH}
    assert arch.bn_params(network) == (1e-3, 0.01)
    assert network in arch.supported_networks()


@pytest.mark.parametrize("network", NETS)
def test_backbone_key_maps_a_torchvision_checkpoint(network):
    from mobilenet_ref import MobileNetV3, TorchVisionNet
    tv = MobileNetV3(network).state_dict()
    mapped = {arch.backbone_key(network, k): v for k, v in tv.items()}
    assert all(k is None for k in (arch.backbone_key(network, k) for k in tv if k.startswith("classifier.")))
    mapped.pop(None)
    want = {k: v for k, v in TorchVisionNet(network, 50).state_dict().items() if k.startswith("base.")}
    assert set(mapped) == set(want)
    for k, v in want.items():
        assert mapped[k].shape == v.shape, k


@pytest.mark.parametrize("network,gmac", [("mobilenet_v3_large", 0.214), ("mobilenet_v3_small", 0.055)])
def test_conv_flops_per_image(network, gmac):
    g = arch.build_graph(network, 50, head=())
    head = 2 * g.feat * 50
    backbone = (arch.conv_flops_per_image(g, 224, 224) - head) / 2e9
    assert abs(backbone - gmac) < 0.003, backbone


def test_restatement_matches_the_interpreter():
    """The graph interpreter the GPU tests use against the restatement module, fp32, eval mode."""
    import numpy as np
    from mobilenet_ref import TorchVisionNet, load, run
    from sykepic_hip import synth
    for network in NETS:
        g = arch.build_graph(network, 50)
        sd = synth.synth_state_dict(arch.param_specs(g), seed=3, logit_gain=2.0)
        net = load(TorchVisionNet(network, 50), {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        x = torch.from_numpy(synth.synth_images(2, 3, 96, 96, seed=1))
        with torch.no_grad():
            want = net(x)
            got = run(g, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, x)[g.ops[-1].dst]
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("network", NETS)
def test_graph_activations_match_the_restatement(network):
    """Per conv / depthwise layer the graph's activation code is the activation module torchvision puts behind it
    (the restatement writes the RE / HS column of the paper's tables out on its own), and every gate is ReLU /
    Hardsigmoid."""
    import torch.nn as nn
    from mobilenet_ref import TorchVisionNet
    ref = TorchVisionNet(network, 50)
    mods = dict(ref.named_modules())
    code = {nn.Hardswish: arch.ACT_HSWISH, nn.ReLU: arch.ACT_RELU}
    g = arch.build_graph(network, 50)
    for op in g.ops:
        if op.kind in (arch.OP_CONV, arch.OP_DWCONV):
            seq = mods[op.name.rsplit(".", 1)[0]]
            act = seq[2] if len(seq) > 2 else None
            assert int(op.relu) == (code[type(act)] if act is not None else arch.ACT_NONE), op.name
        elif op.kind == arch.OP_SE:
            se = mods[op.name]
            assert isinstance(se.activation, nn.ReLU) and isinstance(se.scale_activation, nn.Hardsigmoid)
            assert int(op.relu) == arch.ACT_RELU and op.k == se.fc1.out_channels
