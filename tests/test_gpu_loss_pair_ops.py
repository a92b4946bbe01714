"""`ce_loss_kernel<EX, PAIR>` (csrc/head.hip) through `spk_op_cross_entropy_pair`: the Mixup / CutMix criterion
    L = lam CE(z, ya; w, eps) + (1 - lam) CE(z, yb; w, eps)
against float64 `lam * F.cross_entropy(z, ya, ...) + (1 - lam) * F.cross_entropy(z, yb, ...)` and its autograd
gradient on the CPU; lam is the float32 the hook is handed, as a double, and 1 - lam exact in the reference.

Shapes: every n of {1, 2, 16, 17, 33} x every c of {1, 2, 50, 65, 130} (the row and lane strides of the kernel, as in
test_gpu_loss_ops.py) x the four modes of that file plus "no weights, no smoothing" x lam of {0, float32(0.3), 0.5, 1}.

BOUNDS.  None is fitted to what the kernel gives.  The kernel forms, per row, the soft-max, lse and the smoothing sum
once and then the two row losses and the two gradients g_a, g_b by the pieces that form the single label's (`hard_row_loss`,
`hard_grad` and the shared smoothing term: one kernel template, so the expressions are the same by construction), each
with its own label and its own 1 / W (W_a = sum_i w[ya_i], W_b = sum_i w[yb_i], summed as W is there).  So the computed
g_a^ and A^ = n CE_a^ carry the roundings `test_gpu_loss_ops._bounds` counts for the label vector ya - call its two
results bg_a (per element of dz) and bA (of n * loss) - and g_b^, B^ those of yb: bg_b, bB.  (A fused multiply-add
rounds once where that count has two: contraction can only lower the error.)  What the pair kernel adds, with
d = EPS = 2^-24, is
    l' = fl(1 - lam) = (1 - lam)(1 + d0)                               one rounding (forming 1 - lam)
    dz = fl(fl(lam g_a^) + fl(l' g_b^))                                the two products, the final sum
and the same three operations on A^, B^ for stats[0].  No combined smoothing coefficient is formed.  Hence
    |dz - (lam g_a + (1 - lam) g_b)| <= lam bg_a + (1 - lam) bg_b                      (what the two terms bring along)
                                      + d lam G_a                                      (the product with lam)
                                      + 2 d (1 - lam) G_b                              (1 - lam, and the product with it)
                                      + d (lam G_a + (1 - lam) G_b)                    (the sum)
with G_a = |g_a| + bg_a >= |g_a^| and G_b likewise; the three d terms are multiplied by 1 + 2^-20, which covers the
products of two or three of the (1 + d) factors.  stats[0] the same with A, B, bA, bB.  lam = 1 runs the one-label
instantiation itself (bg_a, bA alone: the formula gives that too, the d terms only add).  Summed over a row the dz bounds bound the
row's sum, which is 0 in exact arithmetic.
Worst observed error / bound on an MI355X (printed by every bounded test, 500 combinations): dz 0.35, n loss 0.08, row
sums of dz 0.06.
Exactness: lam = 1 and yb = None give the BITS of `ops.cross_entropy_ex` on ya (stats, dz, counters); correct rows and
the per-class counters are integers and must EQUAL the reference's on the dominant label - ya when lam >= 0.5, else
yb - on integer logits with planted ties.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_head_pool_ops as H
import test_gpu_loss_ops as K
from test_gpu_head_pool_ops import EPS

pytestmark = pytest.mark.gpu

NS = [1, 2, 16, 17, 33]
CS = [1, 2, 50, 65, 130]
MODES = list(K.MODES) + [("plain", False, 0.0)]
LAMS = [0.0, float(np.float32(0.3)), 0.5, 1.0]
CASES = [(n, c, m) for n in NS for c in CS for m in range(len(MODES))]
IDS = [f"{n}x{c}-{MODES[m][0]}" for n, c, m in CASES]
GUARD = K.GUARD


def _labels(n, c, seed):
    return H._ints((n,), 0, c - 1, seed), H._ints((n,), 0, c - 1, seed + 7)


def _reference(z, ya, yb, lam, w, eps):
    """float64 torch: (n * L, dL/dz) of L = lam CE_a + (1 - lam) CE_b, by autograd on the combined loss."""
    z64 = z.double().requires_grad_(True)
    w64 = None if w is None else w.double()
    loss = lam * F.cross_entropy(z64, ya, weight=w64, label_smoothing=eps, reduction="mean") + \
        (1.0 - lam) * F.cross_entropy(z64, yb, weight=w64, label_smoothing=eps, reduction="mean")
    loss.backward()
    return float(loss.detach()) * z.shape[0], z64.grad.detach()


def _pair_bounds(z, ya, yb, lam, w, eps):
    """(bound of dz per element, bound of stats[0]) as derived in the module docstring."""
    A, ga = K._reference(z, ya, w, eps)
    B, gb = K._reference(z, yb, w, eps)
    bga, bA = K._bounds(z, ya, w, eps)
    bgb, bB = K._bounds(z, yb, w, eps)
    second = 1.0 + 2.0 ** -20

    def combine(va, ba, vb, bb):
        Ma, Mb = abs(va) + ba, abs(vb) + bb
        extra = EPS * (lam * Ma + 2 * (1.0 - lam) * Mb + (lam * Ma + (1.0 - lam) * Mb))
        return lam * ba + (1.0 - lam) * bb + second * extra

    return combine(ga, bga, gb, bgb), combine(torch.tensor(A, dtype=torch.float64), bA, torch.tensor(B, dtype=torch.float64), bB)


def _run(z, ya, yb, lam, w, eps, want_dz=True, counts_base=0):
    from sykepic_hip import ops
    n, c = z.shape
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    flat, (dz,), outside = H._carve([(n, c)])
    cflat, counts = K._counts_buffer(c, counts_base)
    ops.cross_entropy_pair(H._dev(z), ya.cuda(), None if yb is None else yb.cuda(), lam, stats,
                           None if w is None else H._dev(w), eps, counts, dz if want_dz else None)
    return stats, flat, dz, outside, cflat, counts


def _dominant(ya, yb, lam):
    return ya if np.float32(lam) >= np.float32(0.5) else yb


@pytest.mark.parametrize("n,c,mode", CASES, ids=IDS)
def test_random_against_float64(n, c, mode):
    from sykepic_hip import ops
    name, use_w, eps = MODES[mode]
    eps = K._f32(eps)
    z = H._normal((n, c), 3000 * n + c, 3.0)
    ya, yb = _labels(n, c, 3000 * n + c + 1)
    w = K._weights(c, 11 * c + n) if use_w else None
    for lam in LAMS:
        ref_loss, ref_dz = _reference(z, ya, yb, lam, w, eps)
        dz_bound, loss_bound = _pair_bounds(z, ya, yb, lam, w, eps)
        stats, flat, dz, outside, cflat, counts = _run(z, ya, yb, lam, w, eps, counts_base=5)
        what = f"ce_pair {name} {n}x{c} lam {lam:.3g}"
        H._assert_untouched(flat, outside, f"{what} dz")
        H._ratio(dz, ref_dz, dz_bound, f"{what} dz")
        H._ratio(stats[:1], torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1), f"{what} n*loss")
        # every row of dz sums to 0 (each of the two gradients does), within the sum of the row's bounds
        H._ratio(dz.cpu().double().sum(1), torch.zeros(n, dtype=torch.float64), dz_bound.sum(1), f"{what} row sums of dz")
        want_counts, correct = K._counts_ref(z, _dominant(ya, yb, lam))
        assert float(stats[1]) == correct, what
        cf = cflat.cpu()
        assert bool((cf[:64] == GUARD).all()) and bool((cf[64 + 2 * c:] == GUARD).all()), f"{what}: counts guard written"
        assert torch.equal(counts.cpu().view(c, 2).long(), want_counts + 5), f"{what}: counters are added to the buffer"
        # the same call once more: the same bits
        stats2, flat2, _, _, _, counts2 = _run(z, ya, yb, lam, w, eps, counts_base=5)
        assert torch.equal(stats, stats2) and torch.equal(flat, flat2) and torch.equal(counts, counts2), \
            f"{what}: two identical calls differ"
        # without dz (and without counters) nothing but stats is written
        keep, ckeep = flat.clone(), cflat.clone()
        stats3 = torch.zeros(2, dtype=torch.float32, device="cuda")
        ops.cross_entropy_pair(H._dev(z), ya.cuda(), yb.cuda(), lam, stats3, None if w is None else H._dev(w), eps, None, None)
        assert torch.equal(flat, keep) and torch.equal(cflat, ckeep), f"{what}: a call without dz / counts wrote them"
        assert torch.equal(stats3, stats), f"{what}: the statistics depend on whether dz is asked for"


@pytest.mark.parametrize("n,c,mode", CASES, ids=IDS)
def test_lam_one_and_one_label_vector_are_the_single_label_kernel(n, c, mode):
    """lam = 1 (whatever yb holds) and yb = None (whatever lam in [0, 1] says): stats, dz and the counters carry the bits
    of `ops.cross_entropy_ex` on ya."""
    from sykepic_hip import ops
    _, use_w, eps = MODES[mode]
    eps = K._f32(eps)
    z = H._normal((n, c), 4000 * n + c, 3.0)
    ya, yb = _labels(n, c, 4000 * n + c + 1)
    w = K._weights(c, 13 * c + n) if use_w else None
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    flat, (dz,), _ = H._carve([(n, c)])
    cflat, counts = K._counts_buffer(c, 0)
    ops.cross_entropy_ex(H._dev(z), ya.cuda(), stats, None if w is None else H._dev(w), eps, counts, dz)
    for other, lam in ((yb, 1.0), (None, 1.0), (None, 0.25), (None, 0.0)):
        s2, f2, _, _, cf2, _ = _run(z, ya, other, lam, w, eps)
        assert torch.equal(s2, stats) and torch.equal(f2, flat) and torch.equal(cf2, cflat), (other is None, lam)


TIE_CASES = [(n, c, m) for n in NS for c in CS for m in (0, 3, 4)]


@pytest.mark.parametrize("n,c,mode", TIE_CASES, ids=[f"{n}x{c}-{MODES[m][0]}" for n, c, m in TIE_CASES])
def test_exact_counts_on_the_dominant_label(n, c, mode):
    """Integer logits with two equal maxima per row (test_gpu_head_pool_ops._ce_case); ya labels the lower or the higher
    tied index, yb the class after it.  lam = 0 and lam just below 0.5 count against yb, lam = 0.5 and above against
    ya: correct rows and the per-class counters equal the reference's, and twice that after a second call."""
    from sykepic_hip import ops
    _, use_w, eps = MODES[mode]
    eps = K._f32(eps)
    z, ya, planted = H._ce_case(n, c, 100 * n + c)
    yb = (ya + 1) % c
    w = K._weights(c, 3 * c + n) if use_w else None
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    for lam, dom in ((0.0, yb), (float(np.float32(0.3)), yb), (below, yb), (0.5, ya), (float(np.float32(0.7)), ya)):
        want_counts, correct = K._counts_ref(z, dom)
        assert int(want_counts[:, 0].sum()) == n and int(want_counts[:, 1].sum()) == correct
        stats, flat, dz, outside, cflat, counts = _run(z, ya, yb, lam, w, eps)
        H._assert_untouched(flat, outside, "dz")
        assert float(stats[1]) == correct, f"lam {lam}: correct rows {float(stats[1])}, expected {correct}"
        assert torch.equal(counts.cpu().view(c, 2).long(), want_counts), f"lam {lam}"
        assert bool(torch.isfinite(stats).all()) and float(stats[0]) >= 0 and bool(torch.isfinite(dz).all())
        ops.cross_entropy_pair(H._dev(z), ya.cuda(), yb.cuda(), lam, stats, None if w is None else H._dev(w), eps, counts, None)
        assert float(stats[1]) == 2 * correct and torch.equal(counts.cpu().view(c, 2).long(), 2 * want_counts)
        cf = cflat.cpu()
        assert bool((cf[:64] == GUARD).all()) and bool((cf[64 + 2 * c:] == GUARD).all())
    if c >= 2 and n >= 3:
        # the two label vectors really disagree on what is correct
        assert K._counts_ref(z, ya)[1] != K._counts_ref(z, yb)[1] or not torch.equal(K._counts_ref(z, ya)[0], K._counts_ref(z, yb)[0])
