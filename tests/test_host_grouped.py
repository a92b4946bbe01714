"""ResNeXt and Wide ResNet graphs on the host (no GPU): state_dict layout against a torch module built here from
nn.Conv2d(groups=...), parameter counts against torchvision's published numbers, FLOP count, checkpoint key mapping,
the C-ABI entry point of the grouped graphs, and the freezing / warm-up param groups."""

import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

from sykepic_hip import arch, lib, schedule
from sykepic_hip.net import HipNet

# name: (depths, groups, width_per_group, torchvision's parameter count with its 1000-class fc)
GROUPED = {
    "resnext50_32x4d": ((3, 4, 6, 3), 32, 4, 25_028_904),
    "resnext101_32x8d": ((3, 4, 23, 3), 32, 8, 88_791_336),
    "resnext101_64x4d": ((3, 4, 23, 3), 64, 4, 83_455_272),
    "wide_resnet50_2": ((3, 4, 6, 3), 1, 128, 68_883_240),
    "wide_resnet101_2": ((3, 4, 23, 3), 1, 128, 126_886_696),
}


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: stride on the 3x3), restated."""

    def __init__(self, inplanes, planes, stride, groups, width_per_group):
        super().__init__()
        width = int(planes * (width_per_group / 64.0)) * groups
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes * 4))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        return self.relu(self.bn3(self.conv3(y)) + idt)


def torch_resnet(depths, groups, width_per_group, num_classes=1000):
    """torchvision.models.ResNet(Bottleneck, depths, groups=, width_per_group=): children conv1, bn1, relu, maxpool,
    layer1..4, avgpool, fc."""
    mods = OrderedDict(conv1=nn.Conv2d(3, 64, 7, 2, 3, bias=False), bn1=nn.BatchNorm2d(64), relu=nn.ReLU(inplace=True),
                       maxpool=nn.MaxPool2d(3, 2, 1))
    inplanes = 64
    for i, (planes, n) in enumerate(zip((64, 128, 256, 512), depths)):
        blocks = []
        for b in range(n):
            blocks.append(Bottleneck(inplanes, planes, 2 if (b == 0 and i > 0) else 1, groups, width_per_group))
            inplanes = planes * 4
        mods[f"layer{i + 1}"] = nn.Sequential(*blocks)
    mods["avgpool"] = nn.AdaptiveAvgPool2d(1)
    mods["fc"] = nn.Linear(2048, num_classes)
    return nn.Sequential(mods)


class TorchVisionNet(nn.Module):
    """The reference's TorchVisionNet around a backbone: base = children minus the last, then the Linear head."""

    def __init__(self, backbone, num_classes, head=(256, 128)):
        super().__init__()
        self.base = nn.Sequential(*list(backbone.children())[:-1])
        widths = [2048, *head, num_classes]
        self.head = nn.Sequential(*[nn.Linear(widths[i], widths[i + 1]) for i in range(len(widths) - 1)])

    def forward(self, x):
        return self.head(torch.flatten(self.base(x), 1))


def _trainable_count(specs):
    return sum(int(np.prod(s)) for _, s, kind in specs if not kind.startswith(("bn_mean", "bn_var", "bn_nbt")))


@pytest.mark.parametrize("network", sorted(GROUPED))
def test_grouped_graph_matches_torch_module(network):
    depths, groups, wpg, published = GROUPED[network]
    assert network in arch.supported_networks()
    with torch.device("meta"):
        ref = TorchVisionNet(torch_resnet(depths, groups, wpg), 50).state_dict()
    specs = arch.param_specs(arch.build_graph(network, 50))
    assert [k for k, _, _ in specs] == list(ref.keys())
    assert [tuple(s) for _, s, _ in specs] == [tuple(v.shape) for v in ref.values()]
    # torchvision's published count: its own 1000-class fc in place of the head
    assert _trainable_count(arch.param_specs(arch.build_graph(network, 1000, head=()))) == published
    convs2 = [op for op in arch.build_graph(network, 50).ops if op.name.endswith(".conv2")]
    assert convs2 and all(op.groups == groups and op.k == 3 for op in convs2)
    assert all(op.groups == 1 for op in arch.build_graph(network, 50).ops if not op.name.endswith(".conv2"))


def test_grouped_flops_counted_by_hand():
    # resnext50_32x4d at 224^2: torchvision's 4.23 GMACs (stem 118.0 M, fc of 1000 classes 2.048 M)
    g = arch.build_graph("resnext50_32x4d", 1000, head=())
    total = arch.conv_flops_per_image(g, 224, 224)
    macs = 112 * 112 * 64 * 3 * 49 + 2048 * 1000
    inplanes = 64
    for i, (planes, n, hw) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3), (56, 28, 14, 7))):
        width = planes * 2
        for b in range(n):
            s = 2 if (b == 0 and i > 0) else 1
            hin = hw * s
            macs += hin * hin * width * inplanes                      # conv1 (1x1, at the input size)
            macs += hw * hw * width * (width // 32) * 9               # conv2: 32 groups
            macs += hw * hw * planes * 4 * width                      # conv3
            if b == 0:
                macs += hw * hw * planes * 4 * inplanes               # downsample
            inplanes = planes * 4
    assert total == 2 * macs
    assert abs(total / 2 - 4.26e9) < 0.05e9
    # the grouped conv is counted at 1/groups of the dense cost
    dense = arch.build_graph("wide_resnet50_2", 1000, head=())
    assert arch.conv_flops_per_image(dense, 224, 224) / 2 == pytest.approx(11.4e9, rel=0.01)


def test_resnext_checkpoint_keys_map_fully():
    for network in ("resnext50_32x4d", "wide_resnet101_2"):
        depths, groups, wpg, _ = GROUPED[network]
        with torch.device("meta"):
            tv = torch_resnet(depths, groups, wpg).state_dict()
        specs = {k: tuple(s) for k, s, _ in arch.param_specs(arch.build_graph(network, 50))}
        mapped = {}
        for k, v in tv.items():
            dst = arch.backbone_key(network, k)
            if k.startswith("fc."):
                assert dst is None
                continue
            assert dst in specs, k
            assert specs[dst] == tuple(v.shape)
            mapped[dst] = k
        assert set(mapped) == {k for k in specs if k.startswith("base.")}


def test_existing_networks_unchanged():
    g = arch.build_graph("resnet50", 50)
    assert all(op.groups == 1 for op in g.ops)
    assert abs(arch.conv_flops_per_image(g, 224, 224) - 8.175e9) < 5e6
    with pytest.raises(ValueError):
        arch.build_graph("efficientnet_v2_s", 50)


def test_grouped_entry_point_exported_and_desc_size_kept():
    so = ctypes.CDLL(str(lib.LIB_PATH))
    for name in ("spk_model_create_grouped", "spk_op_conv_group", "spk_op_conv_group_dgrad", "spk_op_conv_group_wgrad"):
        assert hasattr(so, name)
    assert ctypes.sizeof(lib.LayerDesc) == 11 * 4 + 4 + 96 + 96
    h = ctypes.c_void_p()
    rc = lib.load().spk_model_create_grouped(None, None, 0, 3, 50, 0, ctypes.byref(h))
    assert rc != 0


class _StubNet:
    """Module views of HipNet without the GPU library (as tests/test_host_train.py builds them)."""

    def __init__(self, network, classes):
        self.graph = arch.build_graph(network, classes)
        self._specs = arch.param_specs(self.graph)
        self._params = OrderedDict()
        self.groups = {}
        HipNet._build_views(self)

    def _set_requires_grad(self, key, flag):
        pass

    def set_param_group(self, key, group):
        self.groups[key] = group

    def parameters(self):
        return iter(self._params.values())


class _StubOpt:
    def __init__(self, groups):
        self.param_groups = groups


def test_freeze_and_warmup_groups_on_resnext():
    """Same children as a ResNet: freeze() leaves BatchNorm + head trainable, LRWarmup unfreezes layer4 (+ avgpool) into
    group 1 at step_2 and the rest of the base into group 2 at step_3 - element counts as the torch module's children."""
    net = _StubNet("resnext50_32x4d", 50)
    with torch.device("meta"):
        ref = TorchVisionNet(torch_resnet((3, 4, 6, 3), 32, 4), 50)
    is_bn = lambda k: ".bn" in k or k.startswith("base.1.") or ".downsample.1." in k  # noqa: E731
    schedule.freeze(net.base)
    first = [p for p in net.parameters() if p.requires_grad]
    n_bn_head = sum(p.numel() for n, p in ref.named_parameters() if is_bn(n) or n.startswith("head."))
    assert sum(p.numel() for p in first) == n_bn_head
    opt = _StubOpt([{"params": first, "lr": 0.01}, {"params": [], "lr": 0.0}, {"params": [], "lr": 0.0}])
    warm = schedule.LRWarmup(net, opt, 0.1, 0.5, 4, 14, 24, verbose=False)
    warm(4)
    warm(14)
    layer4 = sum(p.numel() for n, p in ref.named_parameters() if n.startswith("base.7.") and not is_bn(n))
    assert sum(p.numel() for p in opt.param_groups[1]["params"]) == layer4
    warm(24)
    rest = sum(p.numel() for n, p in ref.named_parameters()
               if n.startswith("base.") and not n.startswith("base.7.") and not is_bn(n))
    assert sum(p.numel() for p in opt.param_groups[2]["params"]) == rest
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters())
