"""Test reference for the MobileNetV3 backbones (torch fp32, CPU or GPU).

- ``MobileNetV3``: a plain torch.nn restatement of torchvision's ``mobilenet_v3_large`` / ``mobilenet_v3_small``
  (width_mult 1.0, no dilation, full tail) with torchvision's module names, so its ``state_dict`` keys are torchvision's.
  Its block tables, squeeze rule and BatchNorm constants are written out here from Howard et al. 2019 (tables 1-2) as
  torchvision implements them, not taken from ``sykepic_hip.arch``: a change to the graph under test does not move
  this side with it.
- ``TorchVisionNet``: the reference's wrapper (sykepic/train/network.py): ``base`` = every child but the last
  ([features, avgpool]), flattened, then the Linear head whose input width is read off the first ``Linear`` of the
  dropped classifier.  (tests/golden/make_golden_mobilenet.py runs the reference's own wrapper on ``MobileNetV3``.)
- ``run`` / ``run_train_forced``: a layer-graph interpreter that knows Hardswish and the ReLU / Hardsigmoid
  squeeze-excitation gate (the oracle's interpreter knows ReLU / SiLU only).
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from sykepic_hip import arch

EPS, MOMENTUM = 1e-3, 0.01   # torchvision: norm_layer = partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)
RE, HS = "RE", "HS"
# (input channels, kernel, expanded channels, output channels, SE, activation, stride) per InvertedResidual
LARGE = [(16, 3, 16, 16, False, RE, 1), (16, 3, 64, 24, False, RE, 2), (24, 3, 72, 24, False, RE, 1),
         (24, 5, 72, 40, True, RE, 2), (40, 5, 120, 40, True, RE, 1), (40, 5, 120, 40, True, RE, 1),
         (40, 3, 240, 80, False, HS, 2), (80, 3, 200, 80, False, HS, 1), (80, 3, 184, 80, False, HS, 1),
         (80, 3, 184, 80, False, HS, 1), (80, 3, 480, 112, True, HS, 1), (112, 3, 672, 112, True, HS, 1),
         (112, 5, 672, 160, True, HS, 2), (160, 5, 960, 160, True, HS, 1), (160, 5, 960, 160, True, HS, 1)]
SMALL = [(16, 3, 16, 16, True, RE, 2), (16, 3, 72, 24, False, RE, 2), (24, 3, 88, 24, False, RE, 1),
         (24, 5, 96, 40, True, HS, 2), (40, 5, 240, 40, True, HS, 1), (40, 5, 240, 40, True, HS, 1),
         (40, 5, 120, 48, True, HS, 1), (48, 5, 144, 48, True, HS, 1), (48, 5, 288, 96, True, HS, 2),
         (96, 5, 576, 96, True, HS, 1), (96, 5, 576, 96, True, HS, 1)]
TABLES = {"mobilenet_v3_large": (LARGE, 960, 1280), "mobilenet_v3_small": (SMALL, 576, 1024)}


def make_divisible(v, divisor=8):
    """torchvision's _make_divisible (SqueezeExcitation width = make_divisible(expanded // 4))."""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _cna(cin, cout, k, stride, groups, act):
    """torchvision Conv2dNormActivation: Sequential(Conv2d, BatchNorm2d[, activation])."""
    layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False),
              nn.BatchNorm2d(cout, eps=EPS, momentum=MOMENTUM)]
    if act is not None:
        layers.append(act(inplace=True))
    return nn.Sequential(*layers)


class SqueezeExcitation(nn.Module):
    def __init__(self, c, squeeze):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(c, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, c, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Hardsigmoid()

    def forward(self, x):
        s = self.fc2(self.activation(self.fc1(self.avgpool(x))))
        return x * self.scale_activation(s)


class InvertedResidual(nn.Module):
    def __init__(self, cin, k, exp, cout, se, act, stride):
        super().__init__()
        act = nn.Hardswish if act == HS else nn.ReLU
        layers = []
        if exp != cin:
            layers.append(_cna(cin, exp, 1, 1, 1, act))
        layers.append(_cna(exp, exp, k, stride, exp, act))
        if se:
            layers.append(SqueezeExcitation(exp, make_divisible(exp // 4)))
        layers.append(_cna(exp, cout, 1, 1, 1, None))
        self.block = nn.Sequential(*layers)
        self.use_res_connect = stride == 1 and cin == cout

    def forward(self, x):
        y = self.block(x)
        return y + x if self.use_res_connect else y


class MobileNetV3(nn.Module):
    def __init__(self, name, num_classes=1000):
        super().__init__()
        rows, last, hidden = TABLES[name]
        feats = [_cna(3, 16, 3, 2, 1, nn.Hardswish)] + [InvertedResidual(*r) for r in rows]
        feats.append(_cna(rows[-1][3], last, 1, 1, 1, nn.Hardswish))
        self.features = nn.Sequential(*feats)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(last, hidden), nn.Hardswish(inplace=True), nn.Dropout(0.2, inplace=True),
                                        nn.Linear(hidden, num_classes))

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


class TorchVisionNet(nn.Module):
    """The reference's wrapper around a torchvision model (network.py:48-72)."""

    def __init__(self, name, num_classes, head=(256, 128), dropout=()):
        super().__init__()
        model = MobileNetV3(name)
        layers = list(model.children())
        first = next(m for m in layers[-1] if isinstance(m, nn.Linear))
        widths = [first.in_features] + list(head) + [num_classes]
        head_layers = [nn.Linear(widths[i], widths[i + 1]) for i in range(len(widths) - 1)]
        for idx, p in dropout:
            head_layers.insert(idx, nn.Dropout(p))
        self.base = nn.Sequential(*layers[:-1])
        self.head = nn.Sequential(*head_layers)

    def forward(self, x):
        x = self.base(x)
        return self.head(x.view(x.size(0), -1))


def load(net, sd):
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return net.eval()


def probabilities(net, x, base=1.3):
    """net_pass's softmax(logits * ln(base)) in fp32 (base <= 0: the logits)."""
    with torch.no_grad():
        z = net(x.float())
    if base <= 0:
        return z
    return torch.softmax(z * float(torch.log(torch.tensor(base))), 1)


def _act(v, a):
    a = int(a)
    if a == arch.ACT_HSWISH:
        return F.hardswish(v)
    if a == arch.ACT_SILU:
        return F.silu(v)
    return F.relu(v) if a == arch.ACT_RELU else v


def _gate(a, op, state):
    s = a.mean((2, 3), keepdim=True)
    s = F.conv2d(s, state[op.name + ".fc1.weight"], state[op.name + ".fc1.bias"])
    s = F.relu(s) if int(op.relu) == arch.ACT_RELU else F.silu(s)
    s = F.conv2d(s, state[op.name + ".fc2.weight"], state[op.name + ".fc2.bias"])
    s = F.hardsigmoid(s) if int(op.relu) == arch.ACT_RELU else torch.sigmoid(s)
    return a * s


def run(graph, state, x, train=False, eps=EPS, momentum=MOMENTUM):
    """fp32 interpreter of the layer graph: {tensor id: activation}.  train: batch statistics (the running statistics in
    `state` are left alone)."""
    acts = {0: x}
    for op in graph.ops:
        a = acts[op.src]
        if op.kind in (arch.OP_CONV, arch.OP_DWCONV):
            groups = op.cin if op.kind == arch.OP_DWCONV else 1
            y = F.conv2d(a, state[op.name + ".weight"], None, op.stride, op.pad, groups=groups)
            y = F.batch_norm(y, state[op.bn + ".running_mean"].clone(), state[op.bn + ".running_var"].clone(),
                             state[op.bn + ".weight"], state[op.bn + ".bias"], train, momentum, eps)
            if op.res >= 0:
                y = y + acts[op.res]
            y = _act(y, op.relu)
        elif op.kind == arch.OP_SE:
            y = _gate(a, op, state)
        elif op.kind == arch.OP_GAVGPOOL:
            y = a.mean((2, 3))
        elif op.kind == arch.OP_LINEAR:
            y = F.linear(a, state[op.name + ".weight"], state[op.name + ".bias"])
        else:
            y = a
        acts[op.dst] = y
    return acts


def _bf16_st(t):
    return t + (t.detach().bfloat16().float() - t.detach())


def run_train_forced(graph, state, x, forced, eps=EPS):
    """Train-mode forward in which every activation is overwritten (straight through) by the value the GPU produced
    (`forced[id]`): autograd then gives each layer's exact local derivatives at the GPU's operating point (the method of
    the oracle's run_train_forced, with Hardswish and the ReLU / Hardsigmoid gate)."""
    def force(v, t):
        return v + (forced[t].to(v.dtype) - v).detach() if t in forced else v

    acts = {0: _bf16_st(x * 255.0) / 255.0}
    for op in graph.ops:
        a = acts[op.src]
        if op.kind in (arch.OP_CONV, arch.OP_DWCONV):
            groups = op.cin if op.kind == arch.OP_DWCONV else 1
            y = F.conv2d(a, _bf16_st(state[op.name + ".weight"]), None, op.stride, op.pad, groups=groups)
            v = F.batch_norm(y, None, None, state[op.bn + ".weight"], state[op.bn + ".bias"], True, 0.1, eps)
            if op.res >= 0:
                v = v + acts[op.res]
            v = _act(v, op.relu)
        elif op.kind == arch.OP_SE:
            v = _gate(a, op, state)
        elif op.kind == arch.OP_GAVGPOOL:
            v = a.mean((2, 3))
        elif op.kind == arch.OP_LINEAR:
            v = F.linear(a, state[op.name + ".weight"], state[op.name + ".bias"])
        else:
            v = a
        acts[op.dst] = force(v, op.dst)
    return acts
