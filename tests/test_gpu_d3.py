"""The direct 3x3 kernel of the 64 -> 64 channel convs (csrc/conv_d3.hip: weight panel resident in LDS, activation
fragments loaded straight into registers, spk_op_conv3x3_direct).

Every configuration accumulates taps 0..8 as two 32-deep steps each, the implicit GEMM's order for Cin = 64, and runs
the same fp32 epilogue: its output must equal the implicit GEMM's and every other configuration's bit for bit, and lie
within the per-element float64 bound tests/test_gpu_conv_candidates.py::_eval_case uses for fp16 eval outputs (computed
the same way from the same rounded operands).  At network level the kernel forced on and forced off (SPK_D3) must give
the same probabilities bit for bit."""

import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# (n, h, w), all 64 -> 64
PROBLEMS = [
    (1, 1, 5),      # fewer pixels than one MFMA tile, every tap of most pixels is padding
    (1, 15, 17),    # odd sizes, M 255
    (3, 7, 7),      # tiles that span image boundaries
    (1, 1, 257),    # one long row
    (2, 9, 16),     # row wrap at a multiple of 16
    (4, 28, 28),    # whole tiles, 13 to 49 of them: still one tile per persistent block
]
# The kernel is persistent: a launch has up to two blocks per CU (512 on a whole MI355X) and a block walks a contiguous
# range of tiles.  Every problem above has fewer tiles than that, so each block runs the tile loop once.  200 704 pixels
# are 784 (256-pixel tiles, one block per CU) to 3 136 (64-pixel tiles) tiles: every block of every configuration walks
# three to six - the activation and shortcut loads one tile ahead, the hand-over of the tile state, the weight base
# wrapping back to the start of the panel.  This is the shape the networks run (stage 1 at 224 x 224 input).
MANY_TILES = (64, 56, 56)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).half()


_REF = {}


def _reference(n, h, w, with_res, relu):
    """Operands (fp16 values) and the float64 result with its per-element bound, computed once per problem."""
    key = (n, h, w, with_res, relu)
    if key not in _REF:
        x = _f16((n, 64, h, w), 31)
        wt = _f16((64, 64, 3, 3), 32).float()
        scale = torch.rand(64, generator=_gen(34)) + 0.5
        shift = torch.randn(64, generator=_gen(35)) * 0.2
        res = _f16((n, 64, h, w), 36) if with_res else None
        if n * h * w > 65536:   # (the float64 convolutions of the large problem on the GPU: seconds on the CPU)
            x, wt, scale, shift, res = (None if t is None else t.cuda() for t in (x, wt, scale, shift, res))
        conv = F.conv2d(x.double(), wt.double(), padding=1)
        a = F.conv2d(x.double().abs(), wt.double().abs(), padding=1)
        s64, b64 = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
        pre = conv * s64 + b64
        mag = a * s64.abs() + b64.abs()
        if with_res:
            pre = pre + res.double()
            mag = mag + res.double().abs()
        ref = pre.clamp_min(0) if relu else pre
        bound = ref.abs() * 2.0 ** -11 + mag * 2.0 ** -16 + 2.0 ** -24
        _REF[key] = tuple(None if t is None else t.cuda() for t in (x, wt, scale, shift, res, ref, bound))
    return _REF[key]


def _check_every_configuration(prob, with_res, relu):
    from sykepic_hip import ops
    n, h, w = prob
    x, wt, scale, shift, res, ref, bound = _reference(n, h, w, with_res, relu)
    ncfg = ops.conv3x3_direct_num_configs()
    assert ncfg >= 2
    # every configuration fits every 64 -> 64 stride-1 problem: one that answers "does not fit" here fails the test
    outs = {cfg: ops.conv3x3_direct(x, wt, scale, shift, relu=relu, cfg=cfg, res=res).contiguous() for cfg in range(-1, ncfg)}
    assert sorted(outs) == list(range(-1, ncfg))
    base = outs[-1]
    for cfg, y in outs.items():
        assert not torch.isnan(y).any(), cfg
        err = (y.double() - ref).abs()
        worst = (err - bound).max().item()
        print("cfg %d: max err %.3e, max (err - bound) %.3e" % (cfg, err.max().item(), worst))
        assert worst <= 0, (cfg, worst)
        assert torch.equal(y.view(torch.int16), base.view(torch.int16)), ("bits differ from the implicit GEMM", cfg,
                                                                         int((y != base).sum()))


@pytest.mark.parametrize("with_res,relu", [(False, False), (True, True), (False, True), (True, False)],
                         ids=["plain", "res_relu", "relu", "res"])
@pytest.mark.parametrize("prob", PROBLEMS, ids=lambda p: "n%d_%dx%d" % p)
def test_every_configuration_equals_the_implicit_gemm(prob, with_res, relu):
    _check_every_configuration(prob, with_res, relu)


@pytest.mark.parametrize("with_res,relu", [(False, False), (True, True)], ids=["plain", "res_relu"])
def test_every_configuration_over_several_tiles_per_block(with_res, relu):
    _check_every_configuration(MANY_TILES, with_res, relu)
    _REF.clear()   # (0.4 GB of float64 reference on the device)


def test_does_not_fit_exactly_when_ineligible():
    from sykepic_hip import ops
    scale, shift = torch.ones(128).cuda(), torch.zeros(128).cuda()

    def run(cin, cout, stride=1, split=False, cfg=0):
        x = _f16((1, cin, 8, 8), 1).cuda()
        wt = _f16((cout, cin, 3, 3), 2).float().cuda()
        return ops.conv3x3_direct(x, wt, scale[:cout], shift[:cout], cfg=cfg, stride=stride, split=split)

    ncfg = ops.conv3x3_direct_num_configs()
    assert ncfg >= 2
    for cfg in range(ncfg):
        assert run(64, 64, cfg=cfg).shape == (1, 64, 8, 8)          # eligible: every configuration runs
    for kw in (dict(cin=128, cout=64), dict(cin=64, cout=128), dict(cin=64, cout=64, stride=2),
               dict(cin=64, cout=64, split=True), dict(cin=64, cout=64, cfg=ncfg)):
        with pytest.raises(RuntimeError, match="does not fit"):
            run(**kw)
        kw = dict(kw, cfg=-1)                                       # the implicit GEMM takes each of these problems
        assert run(**kw).shape[1] == kw["cout"]


@pytest.mark.parametrize("network", ["resnet50", "resnet18"])
def test_networks_do_not_change_a_bit(network):
    """SPK_D3=2 (the kernel wherever it fits) against SPK_D3=0 (never): identical probabilities in the calibrated and the
    mixed mode."""
    code = (
        "import sys, hashlib, numpy as np, torch\n"
        f"sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'syke-pic_amd')!r}]\n"
        "from sykepic_hip import arch, synth\n"
        "from sykepic_hip.net import HipNet\n"
        f"g = arch.build_graph({network!r}, 50)\n"
        "sd = synth.synth_state_dict(arch.param_specs(g), seed=2)\n"
        f"net = HipNet({network!r}, 50, weights=None)\n"
        "net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}); net.eval()\n"
        "net.calibrate(torch.from_numpy(synth.synth_images(8, 3, 64, 64, seed=9000)).cuda())\n"
        "x = torch.from_numpy(synth.synth_images(8, 3, 64, 64, seed=5)).cuda()\n"
        "for mode in ('calibrated', 3):\n"
        "    net.set_precision(mode)\n"
        "    p = net.probabilities(x).cpu().numpy()\n"
        "    assert np.isfinite(p).all()\n"
        "    print('SHA', mode, hashlib.sha256(p.tobytes()).hexdigest())\n")
    outs = []
    for d3 in ("2", "0"):
        out = subprocess.run([sys.executable, "-c", code],
                             env=dict(os.environ, SPK_D3=d3, SPK_TUNE_CACHE="off", SPK_TUNE_LOG="1", SPK_AUTOTUNE="1"),
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        outs.append([ln for ln in out.stdout.splitlines() if ln.startswith("SHA")])
        # the forced run really took the direct kernel (its chooser logs the configuration it keeps), the other never
        picked = [ln for ln in out.stderr.splitlines() if ln.startswith("[spk tune d3]")]
        if d3 == "2":
            assert picked and all(": d3 " in ln for ln in picked), out.stderr[-2000:]
        else:
            assert not picked, picked
    assert len(outs[0]) == 2 and outs[0] == outs[1], (outs[0], outs[1])
