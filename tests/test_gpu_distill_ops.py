"""`ce_loss_kernel<EX, PAIR, KD>` (csrc/head.hip) through `spk_op_cross_entropy_distill`: knowledge distillation
    L  = (1 - alpha) L_hard + alpha KD,      KD = T^2 / n sum_i KL(softmax(t_i / T) || softmax(z_i / T)),
    dz = (1 - alpha) g_hard + (alpha T / n) (pT - q),     pT = softmax(z / T),  q = softmax(t / T)
against float64 `(1 - a) * L_hard + a * T * T * F.kl_div(F.log_softmax(z / T, 1), F.softmax(t / T, 1), reduction=
"batchmean")` and its autograd gradient on the CPU.  L_hard is `F.cross_entropy` (one label vector) or the Mixup /
CutMix criterion of test_gpu_loss_pair_ops.py (two); alpha, T and lam are the float32 values the hook is handed, as
doubles, and 1 - alpha exact in the reference.

Shapes: every n of {1, 2, 16, 17, 33} x every c of {1, 2, 50, 65, 130} (the row and lane strides, as in
test_gpu_loss_pair_ops.py) x three modes (plain; weights + smoothing; weights + smoothing with a second label vector at
lam = float32(0.3)) x T of {1, 2, float32(3.5)} x alpha of {float32(0.3), 1}.

BOUNDS.  None is fitted to what the kernel gives; d = EPS = 2^-24, E = E_EXPF = 3 ulp, both from
test_gpu_head_pool_ops.py.  Every first-order sum below is multiplied by SECOND = 1 + 2^-12, which covers the products of
the (1 + x) factors: every relative error x here is below 2^-13 (asserted in `_soft`).  TINY = 2^-126 is added wherever a
relative bound is claimed for a number that may be subnormal or flushed to 0 (an underflowing exp, a product with it).

The hard part.  g_hard^ and H^ = n L_hard^ are formed by the very code of the undistilled instantiations (one label vector
or two: the same kernel template, the KD terms under `if constexpr`), so they carry `test_gpu_loss_ops._bounds` (bg, bH) or `test_gpu_loss_pair_ops._pair_bounds`.
(A fused multiply-add rounds once where a count has two: contraction can only lower the error.)

The two extra soft-maxes.  u_j = z_j / T is divided once, u^_j = u_j (1 + d_j), |d_j| <= d (T = 1: exact), and the
maximum m^ is taken of the quotients (the division is monotone), so the largest exponent is exactly 0.  An exponential
  e^_j = expf(fl(u^_j - m^)) = exp(u_j - m^) (1 + x),  |x| <= e1 = 3 d max|u| + E
(the division d |u_j|, the subtraction d |u^_j - m^| <= 2 d max|u|, expf itself E) - the count of head_pool's softmax
with one more d max|u|, because there the rounded product is compared against itself and here against the exact u.  The
sum of c such terms and its reciprocal: t = (ceil(c / 64) + 7) d as there.  Hence |pT^ - pT| <= ep_z pT + TINY,
ep = 2 e1 + t, and the same for q with t's own maximum; lse^ = fl(m^ + logf(s^)) has |err| <= el = (e1 + t) + E |log s|
+ d |lse| (head_pool's row bound).

KD.  A term is q^_j fl(fl(u^t_j - lse^_t) - fl(u^z_j - lse^_z)).  With lq_j = log q_j, lp_j = log pT_j, D_j = lq_j - lp_j:
  the first difference:  d |u_t_j| (the division) + el_t + d |lq_j| (the subtraction);  the second likewise with z;
  their difference:      + d |D_j|                       -> eD_j = d (|u_t_j| + |u_z_j| + |lq_j| + |lp_j| + |D_j|) + el_t + el_z
  the product with q^_j: q_j ((ep_t + d) |D_j| + eD_j) + TINY (|D_j| + eD_j + 1)
The row sum: a thread's own terms (ceil(c / 64) - 1 additions) and the 6 levels of the butterfly, kS = ceil(c / 64) + 5
roundings over terms of either sign: kS d sum_j (|q_j D_j| + term bound).  The rows as every loss sums them:
(n / 16 + 17) d sum_i (|row_i| + row bound).  n KD^ = fl(fl(T T) tk): two more roundings.  So
  |n KD^ - n KD| <= T^2 [ sum of the row bounds + (n / 16 + 17) d sum_i (|row_i| + row bound_i) + 2 d |sum of the rows| ].
stats[0] = fl(fl(fl(1 - alpha) H^) + fl(alpha nKD^)): the combination `_pair_bounds` counts, with alpha in the place of
lam, n KD in the place of the first term (one product) and H in the place of the second (1 - alpha, and the product).

dz = fl(fl(hard g^) + fl(ck fl(pT^ - q^))), hard = fl(1 - alpha), ck = fl(fl(alpha T) / n) (n exact):
  soft part:  (alpha T / n) [ep_z pT + ep_t q + 2 TINY + 4 d |pT - q|]       (the difference; ck two; the product)  =: bs
  hard part:  (1 - alpha) bg + 2 d (1 - alpha) G,  G = |g| + bg              (1 - alpha, the product)
  the sum:    d ((1 - alpha) G + S),  S = |soft| + bs.
alpha = 1 makes hard exactly 0 and the hard product exactly 0.  Summed over a row the dz bounds bound the row's sum, which
is 0 in exact arithmetic (each soft-max sums to 1).

Worst observed error / bound on an MI355X (printed by every bounded test, 450 combinations): dz 0.26, n loss 0.04,
n KD 0.03, row sums of dz 0.06.  Wall time of this file there: 4.0 s for its 303 tests.
Exactness: alpha = 0 and teacher = None give the BITS of `ops.cross_entropy_pair` (stats, dz, counters) and leave
kd_stats alone; t = z gives KD = 0 within its bound and, at alpha = 1, |dz| within its bound of 0; correct rows, the
per-class counters and the teacher agreement are integers and must EQUAL the reference's on integer logits with planted
ties in both z and t; the row z = (80, -80, 0), t = (-90, 90, 0) at T = 1 gives KD = 160 and finite dz within bound.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_head_pool_ops as H
import test_gpu_loss_ops as K
import test_gpu_loss_pair_ops as P
from test_gpu_head_pool_ops import EPS, E_EXPF

pytestmark = pytest.mark.gpu

NS = [1, 2, 16, 17, 33]
CS = [1, 2, 50, 65, 130]
LAM = float(np.float32(0.3))
# (name, weights, smoothing, second label vector)
MODES = [("plain", False, 0.0, False), ("w+eps0.1", True, 0.1, False), ("w+eps0.1+pair", True, 0.1, True)]
TS = [1.0, 2.0, float(np.float32(3.5))]
ALPHAS = [float(np.float32(0.3)), 1.0]
CASES = [(n, c, m) for n in NS for c in CS for m in range(len(MODES))]
IDS = [f"{n}x{c}-{MODES[m][0]}" for n, c, m in CASES]
GUARD = K.GUARD
SECOND = 1.0 + 2.0 ** -12
TINY = 2.0 ** -126
WORST = {}


def _note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print(f"[distill] worst so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _hard_reference(z, ya, yb, lam, w, eps):
    return K._reference(z, ya, w, eps) if yb is None else P._reference(z, ya, yb, lam, w, eps)


def _hard_bounds(z, ya, yb, lam, w, eps):
    return K._bounds(z, ya, w, eps) if yb is None else P._pair_bounds(z, ya, yb, lam, w, eps)


def _kd_reference(z, t, T):
    """float64 torch: (n * KD, dKD/dz) of KD = T^2 kl_div(log_softmax(z / T), softmax(t / T), "batchmean")."""
    z64 = z.double().requires_grad_(True)
    kd = T * T * F.kl_div(F.log_softmax(z64 / T, 1), F.softmax(t.double() / T, 1), reduction="batchmean")
    kd.backward()
    return float(kd.detach()) * z.shape[0], z64.grad.detach()


def _reference(z, ya, yb, lam, t, alpha, T, w, eps):
    """float64 torch, by autograd on the combined loss: (n * L, dL/dz, n * KD)."""
    z64 = z.double().requires_grad_(True)
    w64 = None if w is None else w.double()
    hard = F.cross_entropy(z64, ya, weight=w64, label_smoothing=eps, reduction="mean")
    if yb is not None:
        hard = lam * hard + (1.0 - lam) * F.cross_entropy(z64, yb, weight=w64, label_smoothing=eps, reduction="mean")
    kd = T * T * F.kl_div(F.log_softmax(z64 / T, 1), F.softmax(t.double() / T, 1), reduction="batchmean")
    loss = (1.0 - alpha) * hard + alpha * kd
    loss.backward()
    n = z.shape[0]
    return float(loss.detach()) * n, z64.grad.detach(), float(kd.detach()) * n


def _soft(x, T):
    """float64 soft-max of x / T with the per-row quantities of the module docstring."""
    c = x.shape[1]
    u = x.double() / T
    m = u.max(1, keepdim=True).values
    e = torch.exp(u - m)
    s = e.sum(1, keepdim=True)
    e1 = 3 * EPS * u.abs().max(1, keepdim=True).values + E_EXPF
    tt = ((c + 63) // 64 + 7) * EPS
    ep = 2 * e1 + tt
    assert float(ep.max()) < 2.0 ** -13, "the second-order factor of the bounds assumes relative errors below 2^-13"
    logs = torch.log(s)
    lse = m + logs
    el = (e1 + tt) + E_EXPF * logs.abs() + EPS * lse.abs()
    return u, e / s, u - lse, ep, el


def _bounds(z, ya, yb, lam, t, alpha, T, w, eps):
    """(bound of dz per element, bound of stats[0], bound of kd_stats[0]) as derived in the module docstring."""
    n, c = z.shape
    kS = (c + 63) // 64 + 5
    uz, pT, lp, ep_z, el_z = _soft(z, T)
    ut, q, lq, ep_t, el_t = _soft(t, T)
    D = lq - lp
    eD = EPS * (ut.abs() + uz.abs() + lq.abs() + lp.abs() + D.abs()) + el_t + el_z
    term = q * D
    term_bound = q * ((ep_t + EPS) * D.abs() + eD) + TINY * (D.abs() + eD + 1.0)
    rows = term.sum(1)
    row_bound = term_bound.sum(1) + kS * EPS * (term.abs() + term_bound).sum(1)
    nkd = T * T * rows.sum()
    kd_bound = SECOND * T * T * (row_bound.sum() + (n / 16 + 17) * EPS * (rows.abs() + row_bound).sum() +
                                 2 * EPS * rows.sum().abs())
    hard_n, g = _hard_reference(z, ya, yb, lam, w, eps)
    bg, bH = _hard_bounds(z, ya, yb, lam, w, eps)
    hard_n = torch.tensor(hard_n, dtype=torch.float64)
    MH, MK = hard_n.abs() + bH, nkd.abs() + kd_bound
    loss_bound = (1.0 - alpha) * bH + alpha * kd_bound + \
        SECOND * EPS * (alpha * MK + 2 * (1.0 - alpha) * MH + (alpha * MK + (1.0 - alpha) * MH))
    k = alpha * T / n
    soft = k * (pT - q)
    bs = SECOND * k * (ep_z * pT + ep_t * q + 2 * TINY + 4 * EPS * (pT - q).abs())
    G, S = g.abs() + bg, soft.abs() + bs
    dz_bound = (1.0 - alpha) * bg + bs + SECOND * EPS * (3 * (1.0 - alpha) * G + S)
    return dz_bound, loss_bound, kd_bound


def _run(z, ya, yb, lam, t, alpha, T, w, eps, want_dz=True, counts_base=0, want_kd=True):
    from sykepic_hip import ops
    n, c = z.shape
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    flat, (dz, kd), outside = H._carve([(n, c), (2,)])
    kd.zero_()
    cflat, counts = K._counts_buffer(c, counts_base)
    ops.cross_entropy_distill(H._dev(z), ya.cuda(), None if yb is None else yb.cuda(), lam, None if t is None else H._dev(t),
                              alpha, T, stats, None if w is None else H._dev(w), eps, counts, kd if want_kd else None,
                              dz if want_dz else None)
    return stats, flat, dz, kd, outside, cflat, counts


def _case(n, c, mode, seed):
    name, use_w, eps, pair = MODES[mode]
    eps = K._f32(eps)
    z = H._normal((n, c), seed, 3.0)
    t = H._normal((n, c), seed + 3, 3.0)
    ya, yb = P._labels(n, c, seed + 1)
    w = K._weights(c, 11 * c + n) if use_w else None
    return name, z, t, ya, (yb if pair else None), (LAM if pair else 1.0), w, eps


def _agreement(z, t):
    return int((H._argmax_lowest(z) == H._argmax_lowest(t)).sum())


@pytest.mark.parametrize("n,c,mode", CASES, ids=IDS)
def test_random_against_float64(n, c, mode):
    from sykepic_hip import ops
    name, z, t, ya, yb, lam, w, eps = _case(n, c, mode, 5000 * n + c)
    dom = ya if yb is None else P._dominant(ya, yb, lam)
    want_counts, correct = K._counts_ref(z, dom)
    for T in TS:
        for alpha in ALPHAS:
            ref_loss, ref_dz, ref_kd = _reference(z, ya, yb, lam, t, alpha, T, w, eps)
            dz_bound, loss_bound, kd_bound = _bounds(z, ya, yb, lam, t, alpha, T, w, eps)
            stats, flat, dz, kd, outside, cflat, counts = _run(z, ya, yb, lam, t, alpha, T, w, eps, counts_base=5)
            what = f"ce_distill {name} {n}x{c} T {T:g} alpha {alpha:.3g}"
            H._assert_untouched(flat, outside, f"{what} dz / kd_stats")
            _note("dz", H._ratio(dz, ref_dz, dz_bound, f"{what} dz"))
            _note("n*loss", H._ratio(stats[:1], torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1),
                                     f"{what} n*loss"))
            _note("n*KD", H._ratio(kd[:1], torch.tensor([ref_kd], dtype=torch.float64), kd_bound.reshape(1), f"{what} n*KD"))
            # every row of dz sums to 0 (the hard gradient's rows do, and both soft-maxes sum to 1)
            _note("row sums", H._ratio(dz.cpu().double().sum(1), torch.zeros(n, dtype=torch.float64), dz_bound.sum(1),
                                       f"{what} row sums of dz"))
            assert float(stats[1]) == correct, what
            assert float(kd[1]) == _agreement(z, t), what
            cf = cflat.cpu()
            assert bool((cf[:64] == GUARD).all()) and bool((cf[64 + 2 * c:] == GUARD).all()), f"{what}: counts guard written"
            assert torch.equal(counts.cpu().view(c, 2).long(), want_counts + 5), f"{what}: counters are added to the buffer"
            # the same call once more: the same bits
            stats2, flat2, _, _, _, _, counts2 = _run(z, ya, yb, lam, t, alpha, T, w, eps, counts_base=5)
            assert torch.equal(stats, stats2) and torch.equal(flat, flat2) and torch.equal(counts, counts2), \
                f"{what}: two identical calls differ"
            # without dz, counters and kd_stats nothing but stats is written, and stats is the same
            keep, ckeep = flat.clone(), cflat.clone()
            stats3 = torch.zeros(2, dtype=torch.float32, device="cuda")
            ops.cross_entropy_distill(H._dev(z), ya.cuda(), None if yb is None else yb.cuda(), lam, H._dev(t), alpha, T, stats3,
                                      None if w is None else H._dev(w), eps, None, None, None)
            assert torch.equal(flat, keep) and torch.equal(cflat, ckeep), f"{what}: a call without dz / counts / kd wrote them"
            assert torch.equal(stats3, stats), f"{what}: the statistics depend on whether dz is asked for"
            # without dz alone the distillation statistics are the same too
            _, flat4, _, kd4, _, _, _ = _run(z, ya, yb, lam, t, alpha, T, w, eps, want_dz=False, counts_base=5)
            assert torch.equal(kd4, kd), f"{what}: kd_stats depend on whether dz is asked for"
            assert bool((flat4.cpu()[:64 + n * c] == H.SENTINEL).all()), f"{what}: dz written though not asked for"


@pytest.mark.parametrize("n,c,mode", CASES, ids=IDS)
def test_alpha_zero_and_no_teacher_are_the_pair_kernel(n, c, mode):
    """alpha = 0 (whatever the teacher holds) and teacher = None (whatever alpha and T say): stats, dz and the counters
    carry the bits of `ops.cross_entropy_pair`, and kd_stats is not written."""
    from sykepic_hip import ops
    _, z, t, ya, yb, lam, w, eps = _case(n, c, mode, 6000 * n + c)
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    flat, (dz, kd), _ = H._carve([(n, c), (2,)])
    kd.zero_()
    cflat, counts = K._counts_buffer(c, 0)
    ops.cross_entropy_pair(H._dev(z), ya.cuda(), None if yb is None else yb.cuda(), lam, stats,
                           None if w is None else H._dev(w), eps, counts, dz)
    for teacher, alpha, T, want_kd in ((t, 0.0, 2.0, True), (None, 0.0, 2.0, False), (None, 0.5, 3.5, False),
                                       (None, 1.0, 1.0, False)):
        s2, f2, _, _, _, cf2, _ = _run(z, ya, yb, lam, teacher, alpha, T, w, eps, want_kd=want_kd)
        assert torch.equal(s2, stats) and torch.equal(f2, flat) and torch.equal(cf2, cflat), (teacher is None, alpha, T)


@pytest.mark.parametrize("n,c,mode", CASES, ids=IDS)
def test_teacher_equal_to_student(n, c, mode):
    """t = z: KD = 0 and, at alpha = 1, dz = 0, each within its bound; every row agrees with the teacher."""
    name, z, _, ya, yb, lam, w, eps = _case(n, c, mode, 7000 * n + c)
    for T in TS:
        dz_bound, loss_bound, kd_bound = _bounds(z, ya, yb, lam, z, 1.0, T, w, eps)
        stats, flat, dz, kd, outside, _, _ = _run(z, ya, yb, lam, z, 1.0, T, w, eps)
        what = f"ce_distill t = z {name} {n}x{c} T {T:g}"
        H._assert_untouched(flat, outside, what)
        zero = torch.zeros(1, dtype=torch.float64)
        H._ratio(kd[:1], zero, kd_bound.reshape(1), f"{what} n*KD")
        H._ratio(stats[:1], zero, loss_bound.reshape(1), f"{what} n*loss")
        H._ratio(dz, torch.zeros(n, c, dtype=torch.float64), dz_bound, f"{what} dz")
        assert float(kd[1]) == n


TIE_CASES = [(n, c, m) for n in NS for c in CS for m in range(len(MODES))]


@pytest.mark.parametrize("n,c,mode", TIE_CASES, ids=[f"{n}x{c}-{MODES[m][0]}" for n, c, m in TIE_CASES])
def test_exact_counts_and_teacher_agreement(n, c, mode):
    """Integer logits with two equal maxima per row in z (test_gpu_head_pool_ops._ce_case) and, from another seed, in t:
    correct rows, the per-class counters and the rows that agree with the teacher equal the reference's (arg-max = lowest
    index among the maxima on both sides), and twice that after a second call on the same buffers.  With t = z rolled by
    three rows some rows agree and some do not; with t = z all do."""
    from sykepic_hip import ops
    _, use_w, eps, pair = MODES[mode]
    eps = K._f32(eps)
    z, ya, _ = H._ce_case(n, c, 100 * n + c)
    yb = (ya + 1) % c if pair else None
    lam = LAM if pair else 1.0
    dom = ya if yb is None else P._dominant(ya, yb, lam)
    w = K._weights(c, 3 * c + n) if use_w else None
    want_counts, correct = K._counts_ref(z, dom)
    teachers = [H._ce_case(n, c, 900 * n + c)[0], z.roll(3, 0).contiguous(), z.clone()]
    seen = set()
    for t in teachers:
        agree = _agreement(z, t)
        seen.add(agree)
        stats, flat, dz, kd, outside, cflat, counts = _run(z, ya, yb, lam, t, 0.5, 2.0, w, eps)
        H._assert_untouched(flat, outside, "dz / kd_stats")
        assert float(stats[1]) == correct, f"correct rows {float(stats[1])}, expected {correct}"
        assert float(kd[1]) == agree, f"teacher agreement {float(kd[1])}, expected {agree}"
        assert torch.equal(counts.cpu().view(c, 2).long(), want_counts)
        assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(kd).all()) and bool(torch.isfinite(dz).all())
        ops.cross_entropy_distill(H._dev(z), ya.cuda(), None if yb is None else yb.cuda(), lam, H._dev(t), 0.5, 2.0, stats,
                                  None if w is None else H._dev(w), eps, counts, kd, None)
        assert float(stats[1]) == 2 * correct and float(kd[1]) == 2 * agree
        assert torch.equal(counts.cpu().view(c, 2).long(), 2 * want_counts)
        cf = cflat.cpu()
        assert bool((cf[:64] == GUARD).all()) and bool((cf[64 + 2 * c:] == GUARD).all())
    assert _agreement(z, z) == n
    if c >= 50 and n >= 16:
        assert len(seen) >= 2          # the teachers really differ in how many rows agree


@pytest.mark.parametrize("alpha", [float(np.float32(0.3)), 1.0], ids=["alpha0.3", "alpha1"])
def test_underflowing_teacher_probabilities(alpha):
    """z = (80, -80, 0), t = (-90, 90, 0) at T = 1: q = (0, 1, 0) in float32 (exp(-180) and exp(-90) times 1 underflow or
    are far below one ulp of 1), pT = (1, 0, 0).  KD = log q_1 - log pT_1 = 0 - (-160) = 160, finite, and dz finite; a
    second row keeps ordinary values beside it."""
    z = torch.tensor([[80.0, -80.0, 0.0], [0.5, -1.0, 2.0]])
    t = torch.tensor([[-90.0, 90.0, 0.0], [1.0, 0.0, -2.0]])
    ya = torch.tensor([0, 2])
    ref_loss, ref_dz, ref_kd = _reference(z, ya, None, 1.0, t, alpha, 1.0, None, 0.0)
    one_row = _kd_reference(z[:1], t[:1], 1.0)[0]
    assert abs(one_row - 160.0) < 1e-9
    dz_bound, loss_bound, kd_bound = _bounds(z, ya, None, 1.0, t, alpha, 1.0, None, 0.0)
    stats, flat, dz, kd, outside, _, _ = _run(z, ya, None, 1.0, t, alpha, 1.0, None, 0.0)
    H._assert_untouched(flat, outside, "underflow row")
    assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(kd).all()) and bool(torch.isfinite(dz).all())
    H._ratio(kd[:1], torch.tensor([ref_kd], dtype=torch.float64), kd_bound.reshape(1), "underflow n*KD")
    H._ratio(stats[:1], torch.tensor([ref_loss], dtype=torch.float64), loss_bound.reshape(1), "underflow n*loss")
    H._ratio(dz, ref_dz, dz_bound, "underflow dz")
    assert float(kd[1]) == 0.0


def test_bad_arguments_are_refused():
    from sykepic_hip import ops
    z, t = H._dev(H._normal((4, 5), 1)), H._dev(H._normal((4, 5), 2))
    y = H._ints((4,), 0, 4, 3).cuda()
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    kd = torch.zeros(2, dtype=torch.float32, device="cuda")
    for alpha, T, match in ((1.5, 2.0, "alpha must be in"), (-0.1, 2.0, "alpha must be in"), (float("nan"), 2.0, "alpha"),
                            (0.5, 0.0, "temperature"), (0.5, -1.0, "temperature"), (0.5, float("inf"), "temperature"),
                            (0.5, float("nan"), "temperature")):
        with pytest.raises(RuntimeError, match=match):
            ops.cross_entropy_distill(z, y, None, 1.0, t, alpha, T, stats, kd_stats=kd)
    with pytest.raises(RuntimeError, match="kd_stats without teacher"):
        ops.cross_entropy_distill(z, y, None, 1.0, None, 0.5, 2.0, stats, kd_stats=kd)
    assert not bool(stats.ne(0).any()) and not bool(kd.ne(0).any())
