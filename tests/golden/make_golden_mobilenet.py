#!/usr/bin/env python3
"""Generate tests/golden/net_pass_mobilenet.npz by running the REFERENCE's own code (imported from the reference
checkout, read-only): ``TorchVisionNet.__init__ / forward`` (sykepic/train/network.py) and ``probability.net_pass``.

``torchvision`` is not installed here; the ``sys.modules`` shim of make_golden.py is installed and its
``torchvision.models.mobilenet_v3_large`` / ``mobilenet_v3_small`` return the torch.nn restatement in
tests/mobilenet_ref.py.  Everything above the shim is the reference's: which children become ``base`` (features +
avgpool), the flattening, and the head width read off the first ``Linear`` of the dropped classifier (960 / 576).

Weights: generator-seeded (sykepic_hip.synth), BatchNorm running statistics set to the statistics of a seeded
calibration batch (as a trained net's match its data), logits centred on that batch.  The last Linear's gain is chosen
so that the logits have the spread of a trained classifier (std ~4), where top-1 margins exceed the 1e-3 tolerance.

Run:  python tests/golden/make_golden_mobilenet.py      (needs the reference checkout)
Only data is written: 8 ROIs x 50 classes per network at 224 (probabilities, logits, ROI ids, the bias shift).
"""

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT / "tests"))

import make_golden  # noqa: E402  (puts the repository, the package and the reference on sys.path)
from oracle import refnet  # noqa: E402
from sykepic_hip import arch, synth  # noqa: E402

CASES = (("mobilenet_v3_large", 224, 8, 85.0), ("mobilenet_v3_small", 224, 8, 50.0))   # last-Linear gain: logit std ~4


def install_shims():
    import mobilenet_ref
    make_golden.install_shims()
    models = sys.modules["torchvision.models"]
    for name in ("mobilenet_v3_large", "mobilenet_v3_small"):
        setattr(models, name, (lambda n: lambda weights=None, **kw: mobilenet_ref.MobileNetV3(n))(name))


def golden_net_pass():
    from sykepic.compute.probability import net_pass
    from sykepic.train.config import get_network
    out = {}
    for network, hw, n, gain in CASES:
        net = get_network(make_golden.ref_config(network, (3, hw, hw)), 50)
        g = arch.build_graph(network, 50)
        sd = synth.synth_state_dict(arch.param_specs(g), seed=2, logit_gain=gain)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        xc = torch.from_numpy(synth.synth_images(16, 3, hw, hw, seed=99))
        refnet.calibrate_bn(net, xc)
        with torch.no_grad():
            net.eval()
            adj = -net(xc).mean(0)
            net.head[-1].bias += adj
        x = torch.from_numpy(synth.synth_images(n, 3, hw, hw, seed=0))
        rois = [int(r) for r in (synth.hash_u32(n, 77) % 1000 + 2)]
        paths = [f"/x/D20180712T065600_IFCB114_{r:05d}.png" for r in rois]
        half = n // 2
        res = net_pass(net, [(x[:half], paths[:half]), (x[half:], paths[half:])], "cpu")
        tag = f"{network}_{hw}"
        out[f"{tag}_rois_in"] = np.array(rois, dtype=np.int64)
        out[f"{tag}_bias_adj"] = adj.numpy()
        out[f"{tag}_rois_out"] = np.array([r for r, _ in res], dtype=np.int64)
        out[f"{tag}_probs"] = np.array([p for _, p in res], dtype=np.float32)
        with torch.no_grad():
            out[f"{tag}_logits"] = net(x).numpy()
        top2 = np.sort(out[f"{tag}_probs"], 1)[:, -2:]
        print(tag, "logit std", float(out[f"{tag}_logits"].std()), "top1", out[f"{tag}_probs"].argmax(1),
              "margins", np.round(top2[:, 1] - top2[:, 0], 4))
    np.savez_compressed(HERE / "net_pass_mobilenet.npz", **out)


if __name__ == "__main__":
    install_shims()
    torch.set_num_threads(8)
    golden_net_pass()
