"""`ce_loss_kernel<EX>` (csrc/head.hip) through `spk_op_cross_entropy_ex`: CrossEntropyLoss with class weights and label
smoothing against `F.cross_entropy(weight=, label_smoothing=)` and its autograd gradient in float64 on the CPU.

Shapes: every n of {1, 2, 16, 17, 33} (below / at / above the 16 rows a pass of the 16 waves takes, a third pass) x
every c of {1, 2, 50, 64, 65, 130} (below / at / above the lane stride 64, a third stride), each with weights only,
label smoothing only (0.1 and 1.0) and both.  Weights are 10^u, u uniform in [-2, 2].  The smoothing value the reference
gets is the float32 the hook is handed (float32(0.1)), as a double.

BOUNDS.  None is fitted to what the kernel gives: each counts the roundings of the kernel's own arithmetic, with
d = EPS = 2^-24 the unit round-off and E = E_EXPF = 3 ulp the error of expf / logf, both taken from
test_gpu_head_pool_ops.py, whose softmax derivation is reused as it stands:
  e1 = 2 d max|z| + E  relative error of one exponential,  t = (ceil(c / 64) + 7) d  that of their sum and its
  reciprocal, so the kernel's p^ = expf(z - mx) * (1 / s) has |p^ - p| <= ep p with ep = 2 e1 + t.
Sums of positive terms: a chain of k additions has relative error k d.
  W  = sum_i w[y_i]: a thread's own terms (ceil(n / 1024) - 1 additions), the 6 levels of the wave butterfly, the 16 wave
       partials (15): kW = ceil(n / 1024) + 20 roundings; 1 / W one more: eW = (kW + 1) d.  Without weights W = n exactly
       (kW = 0).
  Sw = sum_c w[c]: ceil(c / 64) - 1 own terms + 6 levels: kS = ceil(c / 64) + 5.  Without weights Sw = c exactly.
dz = T1 + T2,  T1 = ca (p^ - onehot),  T2 = cb (p^ Sw - w_j),  ca = ((1 - eps) w_y) (1 / W),  cb = (eps / c) (1 / W):
  ca: the roundings of 1 - eps, of its product with w_y and of the product with 1 / W, plus eW; the difference and
      the product with it one each:                   |T1 err| <= ca [ep p + (eW + 5 d) |p - onehot|]
  cb: the roundings of eps / c and of the product with 1 / W, plus eW; p^ Sw carries ep + kS d + d, the difference
      and the product one each:                       |T2 err| <= cb [(ep + (kS + 1) d) p Sw + (eW + 4 d) |p Sw - w_j|]
  and d (|T1| + |T2|) for the addition.  A fused multiply-add rounds once where this count has two, so contraction
  can only lower the error.  The same bounds, summed over a row, bound the row's sum (which is 0 in exact arithmetic).
loss: lse = mx + logf(s) has |err| <= el = (e1 + t) + E |log s| + d |lse| (head_pool's row bound: the relative error
  of s, logf, the addition).  Row i gives  (1 - eps) w_y r_i + (eps / c) S_i,  r_i = lse - z_y,  S_i = sum_j w_j (lse - z_j)
  (every term >= 0):
      first part:  (1 - eps) w_y [el + 4 d r_i]        (the difference; 1 - eps, its product with w_y, the product)
      S_i:         Sw el + (kS + 2) d S_i               (each difference and each product one rounding, the sum kS with
                                                         kS = ceil(c / 64) + 5 here whether or not there are weights)
      second part: (eps / c) [Sw el + (kS + 4) d S_i]  (eps / c and the product two more)
      their sum:   d row_i
  The rows are summed as the plain loss sums them, (n / 16 + 17) d sum rows (head_pool), and stats[0] = sum (1 / W) n adds
  eW + 2 d:  |stats[0] - n loss| <= (n / W) [sum of the row bounds + (n / 16 + 17 + kW + 3) d sum rows].
Worst observed error / bound on an MI355X (printed by every bounded test): dz 0.33, n loss 0.08, row sums of dz 0.07.
Exactness: correct rows and the per-class counters are integers and must EQUAL the reference (arg-max = lowest index
among the maxima) on integer logits with planted ties, the label on the lower or the higher tied index.
"""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_head_pool_ops as H
from test_gpu_head_pool_ops import EPS, E_EXPF

pytestmark = pytest.mark.gpu

NS = [1, 2, 16, 17, 33]
CS = [1, 2, 50, 64, 65, 130]
MODES = [("w", True, 0.0), ("eps0.1", False, 0.1), ("eps1", False, 1.0), ("w+eps0.1", True, 0.1)]
CASES = [(n, c, m) for n in NS for c in CS for m in range(len(MODES))]
IDS = [f"{n}x{c}-{MODES[m][0]}" for n, c, m in CASES]
GUARD = -777


def _weights(c, seed):
    u = torch.rand(c, generator=H._gen(seed), dtype=torch.float64) * 4 - 2
    w = (10.0 ** u).float()
    assert float(w.min()) >= 1e-2 * (1 - 1e-6) and float(w.max()) <= 1e2 * (1 + 1e-6)
    return w.contiguous()


def _f32(v):
    return float(np.float32(v))


def _reference(z, labels, w, eps):
    """float64 torch: (n * loss, dloss/dz)."""
    z64 = z.double().requires_grad_(True)
    loss = F.cross_entropy(z64, labels, weight=None if w is None else w.double(), label_smoothing=eps, reduction="mean")
    loss.backward()
    return float(loss.detach()) * z.shape[0], z64.grad.detach()


def _bounds(z, labels, w, eps):
    """(bound of dz per element, bound of stats[0]) as derived in the module docstring."""
    n, c = z.shape
    p, e1, t, zs, s = H._softmax_ref(z, 1.0)
    ep = 2 * e1 + t
    w64 = torch.ones(c, dtype=torch.float64) if w is None else w.double()
    kW = (n + 1023) // 1024 + 20 if w is not None else 0
    kS = (c + 63) // 64 + 5
    kSw = kS if w is not None else 0
    eW = (kW + 1) * EPS
    W, Sw = w64[labels].sum(), w64.sum()
    wy = w64[labels].unsqueeze(1)
    onehot = F.one_hot(labels, c).double()
    a, b = 1.0 - eps, eps / c
    ca, cb = a * wy / W, b / W
    d1, d2 = p - onehot, p * Sw - w64
    dz_bound = (ca * (ep * p + (eW + 5 * EPS) * d1.abs()) +
                cb * ((ep + (kSw + 1) * EPS) * p * Sw + (eW + 4 * EPS) * d2.abs()) +
                EPS * ((ca * d1).abs() + (cb * d2).abs()))
    logs = torch.log(s).squeeze(1)
    lse = zs.max(1).values + logs
    el = (e1.squeeze(1) + t) + E_EXPF * logs.abs() + EPS * lse.abs()
    r = lse - zs[torch.arange(n), labels]
    S = (w64 * (lse.unsqueeze(1) - zs)).sum(1)
    rows = a * wy.squeeze(1) * r + b * S
    row_bound = a * wy.squeeze(1) * (el + 4 * EPS * r.abs()) + b * (Sw * el + (kS + 4) * EPS * S.abs()) + EPS * rows.abs()
    loss_bound = (n / W) * (row_bound.sum() + (n / 16 + 17 + kW + 3) * EPS * rows.abs().sum())
    return dz_bound, loss_bound


def _counts_ref(z, labels):
    c = z.shape[1]
    hit = H._argmax_lowest(z) == labels
    return torch.stack([torch.bincount(labels, minlength=c), torch.bincount(labels[hit], minlength=c)], 1), int(hit.sum())


def _counts_buffer(c, base):
    """int32 device buffer with 64 guard words on both sides of counts [c][2], which start at `base`."""
    flat = torch.full((64 + 2 * c + 64,), GUARD, dtype=torch.int32, device="cuda")
    view = flat[64:64 + 2 * c]
    view.fill_(base)
    return flat, view


def _run(z, labels, w, eps, want_dz=True, counts_base=0):
    from sykepic_hip import ops
    n, c = z.shape
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    flat, (dz,), outside = H._carve([(n, c)])
    cflat, counts = _counts_buffer(c, counts_base)
    ops.cross_entropy_ex(H._dev(z), labels.cuda(), stats, None if w is None else H._dev(w), eps, counts,
                         dz if want_dz else None)
    return stats, flat, dz, outside, cflat, counts


@pytest.mark.parametrize("n,c,mode", CASES, ids=IDS)
def test_random_against_float64(n, c, mode):
    name, use_w, eps = MODES[mode]
    eps = _f32(eps)
    z = H._normal((n, c), 1000 * n + c, 3.0)
    labels = H._ints((n,), 0, c - 1, 1000 * n + c + 1)
    w = _weights(c, 7 * c + n) if use_w else None
    ref_loss, ref_dz = _reference(z, labels, w, eps)
    dz_bound, loss_bound = _bounds(z, labels, w, eps)
    stats, flat, dz, outside, cflat, counts = _run(z, labels, w, eps, counts_base=5)
    what = f"ce_ex {name} {n}x{c}"
    H._assert_untouched(flat, outside, f"{what} dz")
    H._ratio(dz, ref_dz, dz_bound, f"{what} dz")
    H._ratio(stats[:1], torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1), f"{what} n*loss")
    # every row of dz sums to 0 (sum_j p = 1 in both terms), within the sum of the row's bounds
    H._ratio(dz.cpu().double().sum(1), torch.zeros(n, dtype=torch.float64), dz_bound.sum(1), f"{what} row sums of dz")
    want_counts, correct = _counts_ref(z, labels)
    assert float(stats[1]) == correct
    cf = cflat.cpu()
    assert bool((cf[:64] == GUARD).all()) and bool((cf[64 + 2 * c:] == GUARD).all()), f"{what}: counts guard written"
    assert torch.equal(counts.cpu().view(c, 2).long(), want_counts + 5), f"{what}: counters are added to the buffer"
    # the same call once more: the same bits
    stats2, flat2, _, _, _, counts2 = _run(z, labels, w, eps, counts_base=5)
    assert torch.equal(stats, stats2) and torch.equal(flat, flat2) and torch.equal(counts, counts2), \
        f"{what}: two identical calls differ"
    # without dz (and without counters) nothing but stats is written
    from sykepic_hip import ops
    keep, ckeep = flat.clone(), cflat.clone()
    stats3 = torch.zeros(2, dtype=torch.float32, device="cuda")
    ops.cross_entropy_ex(H._dev(z), labels.cuda(), stats3, None if w is None else H._dev(w), eps, None, None)
    assert torch.equal(flat, keep) and torch.equal(cflat, ckeep), f"{what}: a call without dz / counts wrote them"
    assert torch.equal(stats3, stats), f"{what}: the statistics depend on whether dz is asked for"


TIE_CASES = [(n, c, m) for n in NS for c in CS for m in (0, 3)]


@pytest.mark.parametrize("n,c,mode", TIE_CASES, ids=[f"{n}x{c}-{MODES[m][0]}" for n, c, m in TIE_CASES])
def test_exact_counts_with_planted_ties(n, c, mode):
    """Integer logits with two equal maxima per row (neighbouring lanes, lanes 33 apart, the same lane 64 apart), the
    label on the lower or the higher one: correct rows and the per-class counters equal the reference's, twice over
    after a second call on the same buffers."""
    from sykepic_hip import ops
    _, use_w, eps = MODES[mode]
    eps = _f32(eps)
    z, labels, planted = H._ce_case(n, c, 100 * n + c)
    assert c < 2 or planted >= max(1, (5 * n) // 6 - 1)
    want_counts, correct = _counts_ref(z, labels)
    assert c < 2 or n < 3 or 0 < correct < n        # both outcomes occur
    assert int(want_counts[:, 0].sum()) == n and int(want_counts[:, 1].sum()) == correct
    w = _weights(c, 3 * c + n) if use_w else None
    stats, flat, dz, outside, cflat, counts = _run(z, labels, w, eps)
    H._assert_untouched(flat, outside, "dz")
    assert float(stats[1]) == correct, f"correct rows: got {float(stats[1])}, expected {correct}"
    assert torch.equal(counts.cpu().view(c, 2).long(), want_counts)
    assert math.isfinite(float(stats[0])) and float(stats[0]) >= 0 and bool(torch.isfinite(dz).all())
    ops.cross_entropy_ex(H._dev(z), labels.cuda(), stats, None if w is None else H._dev(w), eps, counts, None)
    assert float(stats[1]) == 2 * correct and torch.equal(counts.cpu().view(c, 2).long(), 2 * want_counts)
    cf = cflat.cpu()
    assert bool((cf[:64] == GUARD).all()) and bool((cf[64 + 2 * c:] == GUARD).all())


PLAIN_CASES = [(n, c, ones) for n in NS for c in CS for ones in (True, False)]


@pytest.mark.parametrize("n,c,ones", PLAIN_CASES, ids=[f"{n}x{c}-{'ones' if o else 'null'}" for n, c, o in PLAIN_CASES])
def test_unit_weights_without_smoothing_agree_with_the_plain_kernel(n, c, ones):
    """w = ones (and w = NULL), eps = 0 is the plain loss: both kernels lie within their own bound of the float64 value
    (head_pool's for the plain instantiation), so they lie within the sum of the two bounds of each other."""
    from sykepic_hip import ops
    z = H._normal((n, c), 2000 * n + c, 3.0)
    labels = H._ints((n,), 0, c - 1, 2000 * n + c + 1)
    w = torch.ones(c) if ones else None
    stats, _, dz, _, _, _ = _run(z, labels, w, 0.0)
    dz_bound, loss_bound = _bounds(z, labels, w, 0.0)
    plain_stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    plain_dz = torch.full((n, c), float("nan"), dtype=torch.float32, device="cuda")
    ops.cross_entropy(H._dev(z), labels.cuda(), plain_stats, plain_dz)
    # the plain loss's bounds, as test_random_cross_entropy states them (dz there is (p - onehot) / n)
    p, e1, t, zs, s = H._softmax_ref(z, 1.0)
    onehot = F.one_hot(labels, c).double()
    plain_dz_bound = ((2 * e1 + t) * p + 3 * EPS * (p - onehot).abs()) / n
    logs = torch.log(s).squeeze(1)
    lse = zs.max(1).values + logs
    rows = lse - zs[torch.arange(n), labels]
    plain_loss_bound = ((e1.squeeze(1) + t) + E_EXPF * logs.abs() + EPS * (lse.abs() + rows.abs())).sum() + \
        (n / 16 + 17) * EPS * rows.abs().sum()
    what = f"ce_ex vs ce {n}x{c}"
    H._ratio(dz, plain_dz.cpu().double(), dz_bound + plain_dz_bound, f"{what} dz")
    H._ratio(stats[:1], plain_stats[:1].cpu().double(), (loss_bound + plain_loss_bound).reshape(1), f"{what} n*loss")
    assert float(stats[1]) == float(plain_stats[1])
