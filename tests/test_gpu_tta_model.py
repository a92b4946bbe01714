"""`HipNet.probabilities_tta`: one view launch, k eval forwards, one mean launch - against the same forwards on views
that torch made on the CPU, BIT FOR BIT.  The eval forward gives an image the same bits whatever batch it arrives in
(tests/test_gpu_infer.py, tests/test_gpu_calibrated.py), and here the k forwards even see the very batches the oracle
feeds, so nothing but the two new kernels can differ.  Seeded resnet18 and mobilenet_v3_small, n = 3, 64 x 64, once as
a uint8 NHWC batch and once as a float32 NCHW batch."""

import numpy as np
import pytest
import torch

from sykepic_hip import arch, synth, tta

pytestmark = pytest.mark.gpu

CLASSES, N, HW = 50, 3, 64
NETS = {"resnet18": 2.0, "mobilenet_v3_small": 50.0}          # logit gain of the synthetic weights
KINDS = ("u8nhwc", "f32nchw")


@pytest.fixture(scope="module", params=list(NETS))
def net(request):
    from sykepic_hip.net import HipNet
    network = request.param
    sd = synth.synth_state_dict(arch.param_specs(arch.build_graph(network, CLASSES)), seed=2, logit_gain=NETS[network])
    net = HipNet(network, CLASSES, weights=None)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).clone() for k, v in sd.items()})
    net.eval()
    return net


def _batch(kind, h=HW, w=HW, n=N, seed=0):
    g = torch.Generator().manual_seed(seed + h + w)
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    u8[:, : h // 3, : w // 2] //= 4                       # no symmetry of its own: a dark corner
    if kind == "u8nhwc":
        return u8
    return (u8.permute(0, 3, 1, 2).float() / 255.0).contiguous()


def _view(x, v):
    hd, wd = (1, 2) if x.dtype == torch.uint8 else (2, 3)
    if v & 4:
        x = x.transpose(hd, wd)
    if v & 2:
        x = x.flip(hd)
    if v & 1:
        x = x.flip(wd)
    return x.contiguous()


def _oracle(net, x, views):
    """((p_0 + p_1) + ...) / k in float32 on the CPU, p_j = net.probabilities of the view torch made."""
    ps = [net.probabilities(_view(x, v).cuda()).cpu() for v in views]
    s = ps[0].clone()
    for p in ps[1:]:
        s = s + p
    return s / torch.tensor(float(len(views)), dtype=torch.float32), ps


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_mean_of_the_forwards_of_torch_made_views(net, kind):
    x = _batch(kind)
    xd = x.cuda()
    plain = net.probabilities(xd).cpu()
    for views in (tta.views_of("flip"), tta.views_of("dihedral"), (0, 5)):
        got = net.probabilities_tta(xd, views)
        assert got.shape == (N, CLASSES) and got.dtype == torch.float32 and got.is_cuda
        want, ps = _oracle(net, x, views)
        assert torch.equal(_bits(ps[0]), _bits(plain))                              # view 0 is the batch itself
        assert any(not torch.equal(_bits(p), _bits(plain)) for p in ps[1:]), "the views classify like the original"
        assert torch.equal(_bits(got.cpu()), _bits(want)), views
        assert float((got.sum(1) - 1).abs().max()) <= 1e-4
    assert torch.equal(xd.cpu(), x), "the batch was written"
    # no view but the identity: the bits of `probabilities`
    assert torch.equal(_bits(net.probabilities_tta(xd, (0,)).cpu()), _bits(plain))
    assert torch.equal(_bits(net.probabilities_tta(xd, tta.views_of("none")).cpu()), _bits(plain))
    # another softmax base reaches the forwards
    got2 = net.probabilities_tta(xd, (0, 3), base=2.0).cpu()
    ps = [net.probabilities(_view(x, v).cuda(), 2.0).cpu() for v in (0, 3)]
    assert torch.equal(_bits(got2), _bits((ps[0] + ps[1]) / torch.tensor(2.0)))


@pytest.mark.parametrize("kind", KINDS)
def test_dihedral_mean_is_symmetric(net, kind):
    """The eight views of x and of x flipped are the same eight batches in another order, so the two calls average the
    same eight rows in another order.  Seven float32 adds of values <= 1 err by at most 7 * 2^-22 on a sum <= 8 (half
    an ulp of at most 2^-21 each), the division by 8 is exact and leaves at most 7 * 2^-25: two orders differ by at most
    twice that, 7 * 2^-24."""
    x = _batch(kind)
    a = net.probabilities_tta(x.cuda(), tta.views_of("dihedral")).cpu()
    b = net.probabilities_tta(_view(x, 1).cuda(), tta.views_of("dihedral")).cpu()
    d = float((a - b).abs().max())
    print(f"dihedral mean of x and of x flipped: max |dp| = {d:.3e} (bound {7 * 2.0 ** -24:.3e})")
    assert d <= 7 * 2.0 ** -24
    # the plain forward is not symmetric: the bound above is not met by chance
    assert float((net.probabilities(x.cuda()) - net.probabilities(_view(x, 1).cuda())).abs().max()) > 7 * 2.0 ** -24


@pytest.mark.parametrize("kind", KINDS)
def test_rectangular_batch(net, kind):
    x = _batch(kind, 64, 48)
    with pytest.raises(ValueError, match=r"\[image\] shape"):
        net.probabilities_tta(x.cuda(), tta.views_of("dihedral"))
    got = net.probabilities_tta(x.cuda(), tta.views_of("flip"))
    want, _ = _oracle(net, x, tta.views_of("flip"))
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert float((got.sum(1) - 1).abs().max()) <= 1e-4


def test_test_net_predicts_the_argmax_of_the_mean(net, capsys):
    from sykepic_hip import train
    batches = [(_batch("f32nchw", seed=s), torch.tensor(y)) for s, y in ((1, [0, 1, 2]), (2, [2, 1, 0]))]
    classes = [f"c{i}" for i in range(CLASSES)]
    views = tta.views_of("flip")
    preds = torch.cat([net.probabilities_tta(x.cuda(), views).argmax(1).cpu() for x, _ in batches]).tolist()
    plain = torch.cat([net(x.cuda()).argmax(1).cpu() for x, _ in batches]).tolist()

    seen = []
    import sklearn.metrics

    def spy(true, predicted, **kw):
        seen.append((list(true), list(predicted)))
        return "report"
    real = sklearn.metrics.classification_report
    sklearn.metrics.classification_report = spy
    try:
        assert train.test_net(net, batches, classes, net.device, tta="flip") == "report"
        out_tta = capsys.readouterr().out
        assert train.test_net(net, batches, classes, net.device) == "report"
        out_plain = capsys.readouterr().out
    finally:
        sklearn.metrics.classification_report = real
    assert seen[0] == ([0, 1, 2, 2, 1, 0], preds) and seen[1] == ([0, 1, 2, 2, 1, 0], plain)
    first = [ln for ln in out_tta.splitlines() if ln.strip()][0]
    assert "flip" in first and "4 views" in first
    assert [ln for ln in out_plain.splitlines() if ln.strip()][0] == "----- Model Evaluation -----"
    with pytest.raises(ValueError, match="test-time augmentation"):
        train.test_net(net, batches, classes, net.device, tta="rotate")
